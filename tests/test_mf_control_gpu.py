"""-m gpu: the loop control of the DBM mean-field loop - the per-workgroup residual slots (ActArgs::maxdiff_blk),
the verdict the next sweep's first kernel forms from them (ActSide::preload / post_fill), the `done` latch, mf_ctl_kernel, and
the driver that queues groups of sweeps and reads verdicts one group late (MfRing, mf_loop_device, mf_prologue).

Every model here (tests/mf_control_cases.py) has a trip count that one planted (layer, row, unit) decides: a slot that is not
written, is read at a wrong offset or is masked by a wrong bound ends the loop at least 3 sweeps early - tests/test_mf_control.py
shows that on the CPU for every case.  Everything asserted is an integer trip count or a bit pattern against the float32 oracle;
there is no tolerance.  BM355_DEBUG is read once per process, so each forced path is one fresh child under its own time limit."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mf_control_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ('mf_geo=8', 'mf_geo=1', 'mf_fold=0')            # the wide kernel | the narrow kernel | the separate step-0 residual kernels


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_engine(shape, P, max_mf=K.MAX_MF, literal=False):
    from boltzmann_machines_amd.engine import DbmEngine
    eng = DbmEngine(shape['V'], list(shape['n']), n_particles=shape['N'], batch_size=shape['N'], max_mf_updates=max_mf, mf_tol=K.MF_TOL)
    for k, v in P.items():
        eng.set(k, v)
    for k in K.names(len(shape['n'])):
        eng.set(k, 0.5)
    if literal:
        eng.set_sigmoid_literal(True)
    return eng


def check_call(eng, X, T, mu, what, h):
    """one mean_field: the trip count, then every mu bit for bit; h collects what the device returned"""
    from boltzmann_machines_amd.engine import as_device
    got = eng.mean_field(as_device(X))
    h.update(np.int32(got).tobytes())
    assert got == T, '%s: %d sweeps, the oracle makes %d' % (what, got, T)
    for k, want in mu.items():
        g = eng.get(k)
        h.update(bits(g).tobytes())
        bad = bits(g) != bits(want)
        assert not bad.any(), '%s: %s differs in %d of %d entries (first at row, unit %r; max abs %.3g)' % (
            what, k, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(np.abs(g - want).max()))


def run_case(key, h, literal=False, path='the default rule'):
    c = K.case(key)
    p, u, r = c['planted']
    what = '%s [%s%s], planted tile (layer %d, units %d.., rows %d.. narrow / %d.. wide)' % (
        K.case_id(key), path, ', literal sigmoid' if literal else '', p, 32 * (u // 32), 32 * (r // 32), 64 * (r // 64))
    o = c['oracle'][literal]
    eng = make_engine(c['shape'], c['P'], literal=literal)
    check_call(eng, c['X'][0], o['T'][0], o['mu'][0], what + ', first call', h)
    # other data on the same handle: the step-0 condition compares against the mu left behind, so a launch queued past the end
    # of the first loop that wrote anything shows here
    check_call(eng, c['X'][1], o['T'][1], o['mu'][1], what + ', second call', h)
    eng.close()


def run_list(keys, literal=False, path='the default rule'):
    h = hashlib.sha256()
    for key in keys:
        run_case(key, h, literal, path)
    return h.hexdigest()


def run_driver(h, path='the default rule'):
    """the boundary sequence on one handle (mf_control_cases.DRIVER_CALLS), then the capped handles"""
    from boltzmann_machines_amd.engine import as_device
    shape = K.DRIVER['shape']
    L = len(shape['n'])
    runs = K.driver_oracle()
    eng = make_engine(shape, K.driver_params(), max_mf=K.DRIVER['max_mf'])
    eng.set('v', K.driver_twin().p['v'])
    eng.seed(K.DRIVER_SEED)
    for idx, run in enumerate(runs):
        what = 'driver sequence [%s], call %d (x = %r)' % (path, idx, run['x'])
        if run['aside']:
            # one update and one validation fetch: the prediction also passes through the update's second-stream path
            Xt = as_device(K.driver_input(K.DRIVER_TRAIN_X))
            got = (eng.train_step(Xt, K.DRIVER_LR, K.DRIVER_MOM, K.DRIVER_K)[0], eng.metrics(Xt, K.DRIVER_K)[0])
            assert got == run['aside'], '%s: the update and the fetch in front of it made %r sweeps, the oracle %r' % (what, got, run['aside'])
            for k in K.names(L, ('W', 'hb')):
                assert np.array_equal(bits(eng.get(k)), bits(run['P'][k])), '%s: %s after the update' % (what, k)
        if run['preset']:
            for k, v in run['preset'].items():
                eng.set(k, v)
        check_call(eng, run['X'], run['T'], run['mu'], what, h)
    eng.close()
    c = K.case(K.CASES[0])
    for cap in K.CAPS:
        eng = make_engine(c['shape'], c['P'], max_mf=cap)
        want = K.capped(cap)
        check_call(eng, c['X'][0], want['T'], want['mu'], 'max_mf_updates = %d [%s]' % (cap, path), h)
        eng.close()


CHILD = r'''
import hashlib
import sys
sys.path.insert(0, %(root)r)
from tests import mf_control_cases as K
from tests import test_mf_control_gpu as T
what, path = %(what)r, %(path)r
if what == 'driver':
    h = hashlib.sha256()
    T.run_driver(h, path)
    print('MF_CONTROL_DIGEST', h.hexdigest())
else:
    print('MF_CONTROL_DIGEST', T.run_list(K.CASES if what == 'cases' else K.OVER_CASES, path=path))
'''


FAILED_CHILD = []          # the first child that did not exit 0: no further child is started after it


def child(what, path, timeout=120):
    assert not FAILED_CHILD, 'not started: %s did not exit 0' % FAILED_CHILD[0]
    env = dict(os.environ, BM355_DEBUG=path)
    FAILED_CHILD.append('%s under %s' % (what, path))        # (stays if the time limit ends the child)
    r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, what=what, path=path)], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0 and 'MF_CONTROL_DIGEST' in r.stdout, '%s under %s: %s' % (what, path, r.stdout[-2000:] + r.stderr[-4000:])
    FAILED_CHILD.pop()
    return r.stdout.split('MF_CONTROL_DIGEST', 1)[1].split()[0]


@pytest.fixture(scope='module')
def default_digest(gpu_lib):
    return run_list(K.CASES)


# ---- 1. every path forms the same verdict
@pytest.mark.parametrize('key', K.CASES, ids=[K.case_id(k) for k in K.CASES])
def test_default_rule(gpu_lib, key):
    run_case(key, hashlib.sha256())


@pytest.mark.parametrize('key', K.CASES, ids=[K.case_id(k) for k in K.CASES])
def test_literal_sigmoid(gpu_lib, key):
    """the MF + LIT kernel against the oracle's literal mode"""
    run_case(key, hashlib.sha256(), literal=True)


def test_forced_paths(gpu_lib, default_digest):
    """the whole list in one fresh child per path, each under its own time limit, the first failure ends the test; the child
    asserts every call against the oracle and prints the digest of what the device returned, which is that of the default rule"""
    for path in PATHS:
        assert child('cases', path) == default_digest, path


# ---- 2. past the self-control rule: a control step per sweep sums up slots (wide h1 pass, h2 pass) and the atomic cell
# (narrow h1 pass of more than 1024 workgroups)
def test_oversize_default_rule(gpu_lib):
    run_list(K.OVER_CASES)


def test_oversize_forced_geometries(gpu_lib):
    want = run_list(K.OVER_CASES)
    for path in PATHS[:2]:
        assert child('oversize', path) == want, path


# ---- 3. the driver's boundaries
def test_driver_boundaries_default_rule(gpu_lib):
    run_driver(hashlib.sha256())


def test_driver_boundaries_wide_kernel(gpu_lib):
    h = hashlib.sha256()
    run_driver(h)
    assert child('driver', 'mf_geo=8') == h.hexdigest()
