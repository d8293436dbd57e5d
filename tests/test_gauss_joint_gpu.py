"""-m gpu: GaussianRBM as one joint model (RbmEngine.gauss_ais / gauss_free_energy_rows / gauss_pt_*, GaussianRBM.ais_log_Z /
free_energy / log_density / sample_v_tempered) against the CPU twin (tests/gauss_twin.py), which
tests/test_gauss_joint.py holds to ground truth without a GPU.

The shapes are the smallest at which the epilogue can go wrong: an aligned width (12 x 8), ragged quads and slots (13 x 7), several
slots and a ragged last one (67 x 33), several tiles (144 x 80); 12, 15 and 39 rows (39 crosses a row tile)."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gauss_twin as G

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5                     # the project's tolerance for AIS values
STATE = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means', 'sigma')
ENSEMBLE = ('v', 'h', 'part_v', 'part_h', 'mult')
# (V, H, chains, ladder, param seed)
PT_CASES = [
    (12, 8, 3, (0.25, 0.5, 0.75, 1.0), 31),
    (13, 7, 5, (0.3, 0.6, 1.0), 32),
    (67, 33, 13, (0.4, 0.7, 1.0), 33),
    (144, 80, 3, (0.2, 0.5, 0.8, 1.0), 34),
]
# (V, H, param seed, std, n_betas, n_runs, k, AIS seed, chain0, base: None | 'data')
AIS_CASES = [
    (12, 8, 41, 0.3, 20, 12, 1, 2222, 5, None),
    (13, 7, 42, 0.3, 25, 15, 2, 2223, 77, 'data'),
    (67, 33, 43, 0.2, 12, 39, 1, 901, 1234, 'data'),
    (144, 80, 44, 0.1, 8, 39, 2, 902, 3, None),
]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def pt_id(c):
    return '%dx%d-%dx%d' % (c[0], c[1], c[2], len(c[3]))


def ais_id(c):
    return '%dx%d-b%d-r%d-k%d-%s' % (c[0], c[1], c[4], c[5], c[6], c[9])


def engine(p, B=8, **kw):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = p['W'].shape
    eng = RbmEngine(V, H, v_unit=_ffi.UNIT_GAUSSIAN, max_batch=B, **kw)
    for n in ('W', 'vb', 'hb', 'sigma'):
        eng.set(n, p[n])
    return eng


def assert_same_ensemble(got, want, what):
    for n in ENSEMBLE:
        assert got[n].shape == want[n].shape, (what, n)
        assert np.array_equal(bits(got[n]), bits(want[n])), '%s: %s differs in %d places' % (what, n, np.sum(bits(got[n]) != bits(want[n])))
    assert np.array_equal(got['idx'], want['idx']), what + ': idx'
    assert np.array_equal(got['swaps'], want['swaps']), what + ': swap counters'


def run_pt_case(c, seed=515, chain0=7, V0=None, steps=(3, 2)):
    """init and len(steps) sweeps on the engine -> the whole ensemble after every call"""
    from boltzmann_machines_amd.engine import as_device
    V, H, M, betas, pseed = c
    p = G.make_params(V, H, seed=pseed)
    eng = engine(p)
    eng.seed(seed)
    eng.gauss_pt_init(M, betas, as_device(V0) if V0 is not None else None, chain0=chain0)
    out = []
    first = eng.gauss_pt.pt_state()
    first.pop('part_h'), first.pop('h')                 # (no prop-up yet)
    out.append(first)
    for n in steps:
        eng.gauss_pt_sweep(n)
        out.append(eng.gauss_pt.pt_state())
    eng.close()
    return out


# ---- 1. the whole ensemble against the twin after every call
@pytest.mark.parametrize('case', PT_CASES, ids=pt_id)
def test_ensemble_against_the_twin(gpu_lib, case):
    V, H, M, betas, pseed = case
    p = G.make_params(V, H, seed=pseed)
    got = run_pt_case(case)
    e = G.Ensemble(p, M, betas, 515, chain0=7)
    for n, start in (('v', e.v), ('part_v', e.part_v.T), ('mult', e.mult)):
        assert np.array_equal(bits(got[0][n]), bits(start)), 'start: ' + n
    assert np.array_equal(got[0]['idx'], e.idx)
    e.sweep(3, call=0)
    assert_same_ensemble(got[1], e.state(), 'sweep 1')
    e.sweep(2, call=1)                                  # (the call counter advanced; the step parity continues)
    assert_same_ensemble(got[2], e.state(), 'sweep 2')
    if len(betas) > 1:
        assert got[2]['swaps'][0].sum() > 0


def test_one_temperature_from_V_init_is_the_plain_chain_and_read_is_in_data_units(gpu_lib):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    V, H, M = 13, 7, 5
    p = G.make_params(V, H, seed=32)
    V0 = G.data(M, V, 3, p['sigma'])
    eng = engine(p)
    eng.seed(99)
    eng.gauss_pt_init(M, [1.0], as_device(V0), chain0=4)
    st = eng.gauss_pt.pt_state()
    assert np.array_equal(bits(st['v']), bits(G.scale_in(V0, p['sigma'])))
    eng.gauss_pt_sweep(5)
    Vd, Hd = DeviceArray((M, V), f32), DeviceArray((M, H), f32)
    eng.gauss_pt_read(Vd, Hd)
    X, Hs = G.plain_chain(p, V0, 5, 99, row0=4)
    assert np.array_equal(bits(Vd.numpy()), bits(X)) and np.array_equal(Hd.numpy(), Hs)
    # a ladder from V_init: the twin's ensemble, and the beta = 1 rows in data units
    eng.seed(100)
    betas = [0.3, 0.6, 1.0]
    eng.gauss_pt_init(M, betas, as_device(V0))
    eng.gauss_pt_sweep(4)
    swaps, idx = eng.gauss_pt_read(Vd, Hd)
    e = G.Ensemble(p, M, betas, 100, V0=V0)
    e.sweep(4)
    assert_same_ensemble(eng.gauss_pt.pt_state(), e.state(), 'ladder from V_init')
    X, Hs = e.read()
    assert np.array_equal(bits(Vd.numpy()), bits(X)) and np.array_equal(Hd.numpy(), Hs)
    assert np.array_equal(swaps, e.cnt) and np.array_equal(idx.reshape(-1), e.idx)
    eng.close()


def test_chain_slices_and_repeated_runs(gpu_lib):
    case = PT_CASES[2]
    V, H, M, betas, pseed = case
    whole = run_pt_case(case, chain0=10)
    again = run_pt_case(case, chain0=10)
    for a, b in zip(whole[1:], again[1:]):
        assert_same_ensemble(a, b, 'repeated run')
    R = len(betas)
    part = run_pt_case((V, H, 4, betas, pseed), chain0=15)          # chains [5, 9) of the whole run
    rows = slice(5 * R, 9 * R)
    for w, q in zip(whole[1:], part[1:]):
        for n in ('v', 'h', 'mult'):
            assert np.array_equal(bits(w[n][rows]), bits(q[n])), n
        for n in ('part_v', 'part_h'):
            assert np.array_equal(bits(w[n][:, rows]), bits(q[n])), n
        assert np.array_equal(w['idx'][rows], q['idx'])


# ---- 2. the fused flavour against the generic route, and in every geometry
@functools.lru_cache(maxsize=None)
def pt_digests():
    """one digest per case of the whole ensemble after two sweeps"""
    out = []
    for c in PT_CASES:
        last = run_pt_case(c)[-1]
        h = hashlib.sha1()
        for n in ENSEMBLE:
            h.update(bits(last[n]).tobytes())
        h.update(np.ascontiguousarray(last['idx'], np.int32).tobytes() + np.ascontiguousarray(last['swaps'], np.int64).tobytes())
        out.append(h.hexdigest())
    return tuple(out)


# what launch_act_xm_as tells apart (8, 1, 3 with either staging, the half-wave DMA) and two codes that change the prop-up's tile
GEOMETRIES = ('8', '1', '3', '108', '101', '103', '208', '4', '5')
CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_gauss_joint_gpu as T
print('GAUSS_PT_DIGEST', ' '.join(T.pt_digests()))
'''


@pytest.mark.parametrize('dbg', ('gt_fused=0',) + tuple('act_geo=' + g for g in GEOMETRIES))
def test_routes_and_geometries_give_the_same_bits(gpu_lib, dbg):
    """every case in a fresh child process (BM355_DEBUG is read once per process): under gt_fused=0 - the raw pass and the row kernel -
    and under every forced act_geo"""
    want = pt_digests()
    r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=dict(os.environ, BM355_DEBUG=dbg), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and 'GAUSS_PT_DIGEST' in r.stdout, '%s: %s' % (dbg, r.stdout[-2000:] + r.stderr[-4000:])
    got = r.stdout.split('GAUSS_PT_DIGEST', 1)[1].split()
    assert tuple(got) == want, '%s: cases %r differ from the default run' % (dbg, [pt_id(c) for c, g, w in zip(PT_CASES, got, want) if g != w])


# ---- 3. AIS: states bit for bit, values against the float64 re-scoring of the same states
def ais_inputs(c):
    V, H, pseed, std = c[:4]
    p = G.make_params(V, H, std=std, seed=pseed)
    a = G.base_mean(G.data(40, V, pseed, p['sigma']), p['sigma']) if c[9] == 'data' else None
    return p, a


@pytest.mark.parametrize('case', AIS_CASES, ids=ais_id)
def test_ais_against_the_twin(gpu_lib, case):
    n_betas, n_runs, k, seed, chain0 = case[4:9]
    assert n_betas <= 50 and chain0 != 0
    p, a = ais_inputs(case)
    want, wu, wh = G.ais(p, n_betas, n_runs, k, seed, chain0, a)
    eng = engine(p, B=4)                                # n_runs > max_batch: the chain workspaces are the run's own
    got = eng.gauss_ais(n_betas, n_runs, k, seed, chain0=chain0, base_mean=a)
    gu, gh = eng.ais_state(n_runs)
    assert np.array_equal(bits(gu), bits(wu)), 'visible states differ in %d places' % np.sum(bits(gu) != bits(wu))
    assert np.array_equal(gh, wh)
    err = np.abs(got.astype(f64) - want) / np.abs(want)
    print('%s: max relative error %.3e' % (ais_id(case), err.max()))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    # slices by chain0, and a second run: the same bits
    mid = n_runs // 3
    head = eng.gauss_ais(n_betas, mid, k, seed, chain0=chain0, base_mean=a)
    tail = eng.gauss_ais(n_betas, n_runs - mid, k, seed, chain0=chain0 + mid, base_mean=a)
    assert np.array_equal(bits(got), bits(np.concatenate([head, tail])))
    eng.close()


# ---- 4. free energy and log-density
U32 = 2.0 ** -24                # float32 unit roundoff


def fe_bound(p, X):
    """A forward-error bound of the engine's F per row against free_energy64 (both start from the same float32 u = fl(x / sigma) and
    c = fl(vb / sigma)).  With u the unit roundoff of float32:
      * 1/2 (u_i - c_i)^2 is formed and summed in double from the floats: no float32 error;
      * t_j = (u W)_j + hb_j is a float32 chain of V multiply-adds and one add: |dt_j| <= (V + 1) u (sum_i |u_i W_ij| + |hb_j|);
      * softplus is 1-Lipschitz, so dt_j moves it by no more than |dt_j|; its own evaluation is within 4 float32 ulp = 8 u of the
        exact value (asserted by tests/test_epilogue_numerics_gpu.py);
      * a 16-column slot adds its terms in float32, 15 additions: <= 15 u times the slot's sum; the slots are added in double.
    |dF| <= u [ (V + 1) sum_j (sum_i |u_i W_ij| + |hb_j|) + (8 + 15) sum_j softplus(t_j) ], and 1 % for the second-order terms."""
    W, hb, c, sigma = (a.astype(f64) for a in G.params(p))
    V = W.shape[0]
    u = G.scale_in(X, p['sigma']).astype(f64)
    mag = np.abs(u).dot(np.abs(W)) + np.abs(hb)[None, :]
    sp = np.logaddexp(0., u.dot(W) + hb)
    return 1.01 * U32 * ((V + 1) * mag.sum(axis=1) + 23. * sp.sum(axis=1))


@pytest.mark.parametrize('shape', [(12, 8), (13, 7), (67, 33), (144, 80)])
def test_free_energy_rows(gpu_lib, shape):
    from boltzmann_machines_amd.engine import as_device
    V, H = shape
    p = G.make_params(V, H, seed=51)
    N = 39
    X = G.data(N, V, 6, p['sigma'])
    eng = engine(p, B=8)                                # more rows than max_batch
    Xd = as_device(X)
    got = eng.gauss_free_energy_rows(Xd, N)
    assert got.dtype == f64 and got.shape == (N,)
    want, bound = G.free_energy64(p, X), fe_bound(p, X)
    print('%dx%d: max |F - F64| %.3e, bound %.3e .. %.3e, worst ratio %.3f' % (V, H, np.abs(got - want).max(), bound.min(), bound.max(),
                                                                               (np.abs(got - want) / bound).max()))
    assert np.all(np.abs(got - want) <= bound)
    part = eng.gauss_free_energy_rows(Xd, 7, row=13)
    assert np.array_equal(part, got[13:20])
    eng.close()


# ---- 5. a call leaves the handle as it was
def test_calls_leave_the_handle_as_it_was(gpu_lib):
    """parameters, momentum buffers and the call counter behind an AIS run and a free-energy call (the update that follows is the
    update of a handle that never ran them, bit for bit); parameters and momentum buffers behind a tempered sweep"""
    from boltzmann_machines_amd.engine import as_device
    V, H, B = 13, 7, 8
    p = G.make_params(V, H, seed=61)
    X = G.data(B, V, 7, p['sigma'])

    def run(with_calls):
        eng = engine(p, B)
        eng.seed(77)
        eng.train_step(as_device(X), B, 0.01, 0.5, 1)                  # (momenta that are not zero)
        before = {n: eng.get(n) for n in STATE}
        if with_calls:
            eng.gauss_ais(6, 11, 2, 3, chain0=1)
            eng.gauss_free_energy_rows(as_device(X), B)
            for n in STATE:
                assert np.array_equal(bits(eng.get(n)), bits(before[n])), n
        eng.train_step(as_device(X), B, 0.01, 0.5, 1)
        out = {n: eng.get(n) for n in STATE}
        if with_calls:
            eng.gauss_pt_init(3, [0.5, 1.0])
            eng.gauss_pt_sweep(2)
            eng.gauss_pt_read()
            for n in STATE:
                assert np.array_equal(bits(eng.get(n)), bits(out[n])), n
        eng.close()
        return out
    a, b = run(True), run(False)
    for n in STATE:
        assert np.array_equal(bits(a[n]), bits(b[n])), 'the update after the calls differs in ' + n


# ---- 6. the C ABI
def test_entry_point_refusals(gpu_lib):
    from boltzmann_machines_amd.engine import RbmEngine, as_device
    lib = gpu_lib
    V, H = 12, 8
    p = G.make_params(V, H, seed=71)
    out, outd = np.zeros(16, f32), np.zeros(16, f64)
    op, odp = out.ctypes.data_as(C.c_void_p), outd.ctypes.data_as(C.c_void_p)
    good = np.array([0.5, 1.0], f32)
    gp = good.ctypes.data_as(C.c_void_p)
    Xd = as_device(G.data(4, V, 1))

    def refused(rc, entry, what):
        assert rc != 0, what + ' was accepted'
        msg = lib.bm_last_error().decode()
        assert entry in msg, '%s: %s' % (what, msg)
        return msg
    plain = RbmEngine(V, H, max_batch=8)                                 # a Bernoulli handle
    h = plain._h
    for call, entry in ((lambda: lib.bm_rbm_gauss_ais(h, 4, 4, 1, None, 1, 0, op), 'bm_rbm_gauss_ais'),
                        (lambda: lib.bm_rbm_gauss_free_energy_rows(h, Xd.ptr, 4, odp), 'bm_rbm_gauss_free_energy_rows'),
                        (lambda: lib.bm_rbm_gauss_pt_init(h, 2, 2, gp, None, 0), 'bm_rbm_gauss_pt_init'),
                        (lambda: lib.bm_rbm_gauss_pt_sweep(h, 1), 'bm_rbm_gauss_pt_sweep'),
                        (lambda: lib.bm_rbm_gauss_pt_read(h, None, None, None, None), 'bm_rbm_gauss_pt_read')):
        assert 'Gaussian visible units' in refused(call(), entry, entry + ' on a Bernoulli handle')
    assert plain.ais(4, 4, 1, 1).shape == (4,)                           # the handle is what it was
    plain.close()
    eng = engine(p)
    h = eng._h
    refused(lib.bm_rbm_gauss_ais(h, 1, 4, 1, None, 1, 0, op), 'bm_rbm_gauss_ais', 'n_betas = 1')
    refused(lib.bm_rbm_gauss_ais(h, 4, 0, 1, None, 1, 0, op), 'bm_rbm_gauss_ais', 'n_runs = 0')
    refused(lib.bm_rbm_gauss_ais(h, 4, 4, 0, None, 1, 0, op), 'bm_rbm_gauss_ais', 'n_gibbs_steps = 0')
    refused(lib.bm_rbm_gauss_ais(h, 4, 4, 1, None, 1, -1, op), 'bm_rbm_gauss_ais', 'chain0 = -1')
    refused(lib.bm_rbm_gauss_ais(h, 4, 4, 1, None, 1, 0, None), 'bm_rbm_gauss_ais', 'null values')
    refused(lib.bm_rbm_gauss_ais(None, 4, 4, 1, None, 1, 0, op), 'bm_rbm_gauss_ais', 'a null handle')
    refused(lib.bm_rbm_gauss_free_energy_rows(h, None, 4, odp), 'bm_rbm_gauss_free_energy_rows', 'null rows')
    refused(lib.bm_rbm_gauss_free_energy_rows(h, Xd.ptr, 4, None), 'bm_rbm_gauss_free_energy_rows', 'null output')
    refused(lib.bm_rbm_gauss_free_energy_rows(h, Xd.ptr, 0, odp), 'bm_rbm_gauss_free_energy_rows', 'no rows')
    refused(lib.bm_rbm_gauss_pt_sweep(h, 1), 'bm_rbm_gauss_pt_sweep', 'a sweep before init')
    refused(lib.bm_rbm_gauss_pt_read(h, None, None, None, None), 'bm_rbm_gauss_pt_read', 'a read before init')
    for bad, what in (([0.5, 0.9], 'a ladder that does not end at 1'), ([0.0, 1.0], 'beta = 0'), ([0.7, 0.6, 1.0], 'a ladder that decreases'),
                      ([1.0, 1.0], 'a repeated beta')):
        b = np.ascontiguousarray(bad, f32)
        assert lib.bm_rbm_gauss_pt_init(h, 2, len(b), b.ctypes.data_as(C.c_void_p), None, 0) != 0, what
    assert lib.bm_rbm_gauss_pt_init(h, 0, 2, gp, None, 0) != 0 and lib.bm_rbm_gauss_pt_init(h, 2, 2, None, None, 0) != 0
    assert lib.bm_rbm_gauss_pt_init(h, 2, 2, gp, None, -1) != 0 and lib.bm_rbm_gauss_pt_init(None, 2, 2, gp, None, 0) != 0
    eng.gauss_pt_init(2, good)
    refused(lib.bm_rbm_gauss_pt_sweep(h, 0), 'bm_rbm_gauss_pt_sweep', 'n_steps = 0')
    refused(lib.bm_rbm_gauss_pt_read(h, None, Xd.ptr, None, None), 'bm_rbm_gauss_pt_read', 'H_dev without V_dev')
    eng.gauss_pt_sweep(1)                                                 # the handle is usable
    # the entries of the Bernoulli model keep refusing the Gaussian handle, with the same words
    for call in (lambda: lib.bm_rbm_ais(h, 4, 4, 1, None, 1, 0, op), lambda: lib.bm_rbm_free_energy_rows(h, Xd.ptr, 4, op),
                 lambda: lib.bm_rbm_pt_init(h, 2, 2, gp, None, 0)):
        assert call() != 0 and "needs Bernoulli visible units (this handle's are Gaussian)" in lib.bm_last_error().decode()
    assert lib.bm_rbm_pt_sweep(h, 1) != 0 and 'no ensemble' in lib.bm_last_error().decode()      # (the Gaussian ensemble is not theirs)
    with pytest.raises(ValueError):
        eng.gauss_ais(5, 4, 1, 3, base_mean=np.zeros(V + 1, f32))
    eng.close()


# ---- 7. the public API end to end
def test_public_api(gpu_lib, tmp_path):
    """fit a small GaussianRBM with a per-unit sigma, then ais_log_Z, log_density and sample_v_tempered against the twin; exactly
    one host seed is consumed per sampling call, none by free_energy / log_density; no parameter changes"""
    from boltzmann_machines_amd import GaussianRBM
    V, H, BS = 13, 7, 10
    sigma = (0.5 + 0.1 * np.arange(V)).astype(f32)
    X = G.data(30, V, 9, sigma)
    m = GaussianRBM(n_visible=V, n_hidden=H, sigma=list(sigma), learning_rate=1e-3, batch_size=BS, max_epoch=2, random_seed=1337,
                    verbose=False, model_path=str(tmp_path / 'm') + '/').fit(X)
    w = m.get_tf_params(scope='weights')
    p = dict(W=w['W'], vb=w['vb'], hb=w['hb'], sigma=sigma)
    rng = m._rng

    def seed_of_next_call():
        st = rng.get_state()
        s = m.make_random_seed()
        after = rng.get_state()
        rng.set_state(st)
        return s, after

    def same_state(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    seed, after = seed_of_next_call()
    lz, (lo, hi), vals = m.ais_log_Z(n_betas=30, n_runs=16, n_gibbs_steps=1, X_base=X)
    assert same_state(rng.get_state(), after)                               # exactly one host seed
    want, _, _ = G.ais(p, 30, 16, 1, seed, a=G.base_mean(X, sigma))
    np.testing.assert_allclose(vals, want, rtol=RTOL, atol=0)
    assert np.isfinite(lz) and lo <= lz <= hi
    st = rng.get_state()
    F = m.free_energy(X)
    lp = m.log_density(X, lz)
    assert same_state(rng.get_state(), st)                                  # neither draws
    assert F.dtype == f64 and np.all(np.abs(F - G.free_energy64(p, X)) <= fe_bound(p, X))
    assert np.array_equal(lp, -F - lz)
    betas = [0.3, 0.6, 1.0]
    seed, after = seed_of_next_call()
    S, acc = m.sample_v_tempered(5, n_gibbs_steps=4, betas=betas, return_stats=True)
    assert same_state(rng.get_state(), after)
    e = G.Ensemble(p, 5, betas, seed)
    e.sweep(4)
    assert np.array_equal(bits(S), bits(e.read()[0]))
    np.testing.assert_array_equal(acc, e.cnt[1] / np.maximum(e.cnt[0], 1))
    seed, after = seed_of_next_call()
    S1 = m.sample_v_tempered(5, n_gibbs_steps=3, n_temperatures=1, V_init=X[:5])
    assert same_state(rng.get_state(), after)
    assert np.array_equal(bits(S1), bits(G.plain_chain(p, X[:5], 3, seed)[0]))
    after_w = m.get_tf_params(scope='weights')
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(after_w[n]), bits(w[n])), n
    with pytest.raises(ValueError):
        m.sample_v_tempered(5, n_gibbs_steps=2, V_init=X[:4])
    # the old names stay refused on the fitted model
    for call in (lambda: m.log_Z(n_betas=5, n_runs=4), lambda: m.log_proba(X, 0.), lambda: m.sample_v(3)):
        with pytest.raises(NotImplementedError, match='Gaussian visible units are not supported'):
            call()
