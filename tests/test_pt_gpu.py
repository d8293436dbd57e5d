"""-m gpu: parallel tempering - the RT flavour of act_kernel, pt_init / pt_swap / pt_gather,
bm_rbm_pt_init / _sweep / _read and BernoulliRBM.sample_v.

The engine is compared BIT FOR BIT (view(uint32)) with the CPU twin of tests/pt_twin.py.  Shapes: 37 x 22 with 7 chains x 5
temperatures (35 rows: ragged in I and J, I % 4 != 0 - the generic draw path, a k-major prop-up) and 100 x 72 with 40 chains x 4
temperatures (160 rows: several row tiles, x-major operands, temperatures that differ inside and across tiles after swaps);
N(0, 1) weights, 6 steps per call: both swap parities, acceptance neither 0 nor 1.  The swap decision compares a uniform with
a double exp(): the test first asserts on the twin that NO draw of its cases lies within 1e-9 of its threshold (the seeds were
chosen so; the closest is 2.9e-4), and then excludes nothing."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import clamp_twin
from tests import pt_twin as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 424242
SHAPES = [(37, 22, 5, 7), (100, 72, 4, 40)]            # V, H, R, M
STEPS = 6


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rbm_params(V, H):
    return dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H),
                vb=(orc.uniform(SEED, 2, 0, V) - np.float32(0.5)) * np.float32(0.6),
                hb=(orc.uniform(SEED, 3, 0, H) - np.float32(0.5)) * np.float32(0.6), sigma=np.ones(V, np.float32))


def ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(np.float32)


def start(M, V):
    return (orc.uniform(SEED, 6, 0, M * V) < 0.5).astype(np.float32).reshape(M, V)


def rbm_engine(V, H, p, max_batch=4, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    eng = RbmEngine(V, H, max_batch=max_batch, **kw)       # (max_batch does not bound the ensemble)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, p[n])
    eng.seed(SEED)
    return eng


def snapshot(V, H, idx, swaps):
    return dict(V=np.array(V), H=np.array(H), idx=np.array(idx, np.int32).reshape(-1), swaps=np.array(swaps, np.int64))


def engine_read(eng, M):
    from boltzmann_machines_amd._ffi import DeviceArray
    Vd, Hd = DeviceArray((M, eng.V)), DeviceArray((M, eng.H))
    swaps, idx = eng.pt_read(Vd, Hd)
    return snapshot(Vd.numpy(), Hd.numpy(), idx, swaps)


def engine_run(eng, M, R, calls, V0=None, chain0=0):
    """pt_init, then one pt_sweep per entry of `calls`; the snapshot after every call"""
    from boltzmann_machines_amd._ffi import DeviceArray
    eng.pt_init(M, ladder(R), DeviceArray.from_numpy(V0) if V0 is not None else None, chain0=chain0)
    out = []
    for n in calls:
        eng.pt_sweep(n)
        out.append(engine_read(eng, M))
    return out


@functools.lru_cache(maxsize=None)
def twin_run(V, H, R, M, calls, with_v0=False, chain0=0):
    """the same on the twin (computed once per case, shared, never modified), + the tie margins and the final counters"""
    e = T.Ensemble(rbm_params(V, H), M, ladder(R), seed=SEED, chain0=chain0, V0=start(M, V) if with_v0 else None)
    out = []
    for call, n in enumerate(calls):
        e.sweep(n, call=call)
        v, h = e.read()
        out.append(snapshot(v, h, e.idx, e.cnt))
    return out, (min(e.margins) if e.margins else np.inf)


def assert_twin_is_decisive(V, H, R, M, calls, **kw):
    want, margin = twin_run(V, H, R, M, calls, **kw)
    assert margin >= 1e-9, 'a swap draw of this case lies within 1e-9 of its threshold: choose another seed'
    acc, att = want[-1]['swaps'][1], want[-1]['swaps'][0]
    assert np.all(att > 0) and 0 < acc.sum() < att.sum()
    return want


def assert_same_snapshot(got, want, what):
    for k in ('V', 'H'):
        assert same(got[k], want[k]), '%s: %s differs from the twin in %d entries' % (what, k, int(np.sum(bits(got[k]) != bits(want[k]))))
    assert np.array_equal(got['idx'], want['idx']), '%s: ladder indices differ' % what
    assert np.array_equal(got['swaps'], want['swaps']), '%s: swap counters %s against %s' % (what, got['swaps'].tolist(), want['swaps'].tolist())


@pytest.mark.parametrize('with_v0', [False, True])
@pytest.mark.parametrize('V,H,R,M', SHAPES)
def test_engine_matches_twin(gpu_lib, V, H, R, M, with_v0):
    """after one call and after two consecutive calls (call counter, parity continuation); random start and a given one"""
    calls = (STEPS, STEPS)
    want = assert_twin_is_decisive(V, H, R, M, calls, with_v0=with_v0)
    eng = rbm_engine(V, H, rbm_params(V, H))
    got = engine_run(eng, M, R, calls, V0=start(M, V) if with_v0 else None)
    eng.close()
    for n, (g, w) in enumerate(zip(got, want)):
        assert_same_snapshot(g, w, '%dx%d R=%d M=%d, call %d' % (V, H, R, M, n))
        assert set(np.unique(g['V'])) <= {0.0, 1.0}
        assert np.array_equal(np.sort(g['idx'].reshape(M, R), axis=1), np.tile(np.arange(R), (M, 1)))


def test_parity_continues_across_calls(gpu_lib):
    """an odd number of steps in the first call: the second one starts with the odd pairs"""
    V, H, R, M = SHAPES[0]
    calls = (3, 4)
    want = assert_twin_is_decisive(V, H, R, M, calls)
    eng = rbm_engine(V, H, rbm_params(V, H))
    got = engine_run(eng, M, R, calls)
    eng.close()
    for n, (g, w) in enumerate(zip(got, want)):
        assert_same_snapshot(g, w, 'calls of 3 and 4 steps, call %d' % n)


@pytest.mark.parametrize('V,H,M', [(37, 22, 7), (100, 72, 40)])
def test_one_temperature_is_the_unclamped_gibbs_sweep(gpu_lib, V, H, M):
    """R = 1, betas = (1,): bit-identical to bm_rbm_gibbs_clamped with an all-zero mask from the same V0, seed and call -
    and to the twin's plain loop"""
    from boltzmann_machines_amd._ffi import DeviceArray
    p = rbm_params(V, H)
    V0 = start(M, V)
    eng = rbm_engine(V, H, p, max_batch=M)
    Vd, Hd, Zd = DeviceArray.from_numpy(V0), DeviceArray((M, H)), DeviceArray.from_numpy(np.zeros((M, V), np.float32))
    eng.gibbs_clamped(Vd, Hd, M, STEPS, Zd, Zd)
    eng.sync()
    eng.seed(SEED)
    got = engine_run(eng, M, 1, (STEPS,), V0=V0)[0]
    eng.close()
    assert same(got['V'], Vd.numpy()) and same(got['H'], Hd.numpy())
    assert got['swaps'].size == 0 and np.all(got['idx'] == 0)
    v, h, _ = clamp_twin.rbm_gibbs_clamped(p, V0, None, None, STEPS, seed=SEED, clamped=False)
    assert same(got['V'], v) and same(got['H'], h)


GEO_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tests import test_pt_gpu as G
V, H, R, M = G.SHAPES[%(shape)d]
eng = G.rbm_engine(V, H, G.rbm_params(V, H))
got = G.engine_run(eng, M, R, (G.STEPS,))[0]
eng.close()
np.savez(%(out)r, **got)
print('PT_GEOMETRY_OK')
'''


@pytest.mark.parametrize('shape,geos', [(0, ('4', '1')), (1, ('8', '103'))])
def test_forced_geometries_give_the_same_bits(gpu_lib, tmp_path, shape, geos):
    """the same call under two forced act_geo values (read once per process: one subprocess each, as test_geometries_gpu.py):
    identical states and - through the slot partials - identical swap decisions; both equal the twin.  37 x 22: the 64 x 32
    tile with two quads per lane (k-major prop-up) against 32 x 32; 100 x 72: 8 waves against 32 x 32 / BK = 32 with
    register staging"""
    V, H, R, M = SHAPES[shape]
    want = assert_twin_is_decisive(V, H, R, M, (STEPS, STEPS))[0]
    for geo in geos:
        out = str(tmp_path / ('geo%s.npz' % geo))
        r = subprocess.run([sys.executable, '-c', GEO_SCRIPT % dict(root=ROOT, shape=shape, out=out)],
                           env=dict(os.environ, BM355_DEBUG='act_geo=' + geo), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and 'PT_GEOMETRY_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
        assert_same_snapshot(dict(np.load(out)), want, 'act_geo=%s' % geo)


def test_chain_slices_reproduce_the_whole(gpu_lib):
    """chains 3..6 of the 7-chain run are the 4-chain run at chain0 = 3 (random start: the start draws at the global row too)"""
    V, H, R, M = SHAPES[0]
    eng = rbm_engine(V, H, rbm_params(V, H))
    whole = engine_run(eng, M, R, (STEPS,))[0]
    eng.seed(SEED)
    part = engine_run(eng, 4, R, (STEPS,), chain0=3)[0]
    eng.close()
    assert same(whole['V'][3:], part['V']) and same(whole['H'][3:], part['H'])
    assert np.array_equal(whole['idx'].reshape(M, R)[3:], part['idx'].reshape(4, R))
    want = assert_twin_is_decisive(V, H, R, 4, (STEPS,), chain0=3)[0]
    assert_same_snapshot(part, want, 'chain0 = 3')


def test_default_paths_are_untouched(gpu_lib):
    """bm_rbm_gibbs and one bm_rbm_train_step give the same bits whether or not a tempered call ran before them on the handle"""
    from boltzmann_machines_amd._ffi import DeviceArray
    V, H, R, M = SHAPES[1]
    B = 16
    p = rbm_params(V, H)
    X = start(B, V)
    H0 = (orc.uniform(SEED, 7, 0, B * H) < 0.5).astype(np.float32).reshape(B, H)
    results = []
    for tempered in (False, True):
        eng = rbm_engine(V, H, p, max_batch=B, sample_v_states=True)
        if tempered:
            engine_run(eng, M, R, (2,))
            eng.seed(SEED)
        Hd, Vd = DeviceArray.from_numpy(H0), DeviceArray((B, V))
        eng.gibbs(Hd, Vd, B, 3)
        eng.train_step(DeviceArray.from_numpy(X), B, 0.05, 0.9, 1)
        eng.sync()
        results.append([Hd.numpy(), Vd.numpy()] + [eng.get(n) for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb')])
        if tempered:                                   # ... and the ensemble is still there behind them
            assert engine_read(eng, M)['idx'].size == M * R
        eng.close()
    for a, b in zip(*results):
        assert same(a, b)


def test_entry_point_errors(gpu_lib):
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray, UNIT_GAUSSIAN, UNIT_MULTINOMIAL
    V, H = 20, 12
    p = rbm_params(V, H)
    eng = rbm_engine(V, H, p)
    with pytest.raises(Bm355Error, match='pt_init first'):
        eng.pt_sweep(1)
    with pytest.raises(Bm355Error, match='pt_init first'):
        eng.pt_read(DeviceArray((3, V)))
    for bad in ([0.5, 0.5, 1.0], [0.6, 0.4, 1.0], [0.0, 1.0], [-0.5, 1.0], [0.5, 0.9], [0.5, 1.5], [1.0, 1.0]):
        with pytest.raises(Bm355Error, match='beta'):
            eng.pt_init(3, bad)
    with pytest.raises(Bm355Error, match='n_temps'):
        eng.pt_init(3, [])
    with pytest.raises(Bm355Error, match='n_chains'):
        eng.pt_init(0, [1.0])
    with pytest.raises(Bm355Error, match='pt_init first'):       # a failed init leaves no ensemble behind
        eng.pt_sweep(1)
    eng.pt_init(3, [0.5, 1.0])
    with pytest.raises(Bm355Error, match='n_steps'):
        eng.pt_sweep(0)
    eng.pt_sweep(1)
    eng.close()
    for kw, word in ((dict(v_unit=UNIT_GAUSSIAN), 'Gaussian'), (dict(h_unit=UNIT_MULTINOMIAL, n_samples=3), 'Multinomial'),
                     (dict(dbm_first=True), 'dbm_first'), (dict(dbm_last=True), 'dbm_first')):
        eng = rbm_engine(V, H, p, **kw)
        with pytest.raises(Bm355Error, match=word):
            eng.pt_init(3, [0.5, 1.0])
        eng.close()
    from boltzmann_machines_amd.engine import RbmEngine64
    assert not hasattr(RbmEngine64, 'pt_init')


# ------------------------------------------------------------------------------------------------ public API
NV, NH, BS = 12, 8, 5
XTRAIN = (orc.uniform(SEED, 60, 0, 20 * NV) < 0.4).astype(np.float32).reshape(20, NV)


def test_public_sample_v(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM
    rbm = BernoulliRBM(n_visible=NV, n_hidden=NH, batch_size=BS, max_epoch=2, random_seed=1337, verbose=False,
                       model_path=str(tmp_path / 'm') + '/').fit(XTRAIN)
    before = {k: np.array(v) for k, v in rbm.get_tf_params(scope='weights').items()}
    st = rbm._rng.get_state()
    V1, rates = rbm.sample_v(9, n_gibbs_steps=5, n_temperatures=4, return_stats=True)          # 9 > batch_size
    assert V1.shape == (9, NV) and set(np.unique(V1)) <= {0.0, 1.0}
    assert rates.shape == (3,) and np.all((rates >= 0) & (rates <= 1))
    swaps, idx = rbm._engine.pt_read()
    assert idx.shape == (9, 4) and np.array_equal(rates, swaps[1] / swaps[0].astype(np.float64))
    assert np.all(swaps[0] > 0)
    after_call = rbm.make_random_seed()
    rbm._rng.set_state(st)
    rbm.make_random_seed()
    assert after_call == rbm.make_random_seed()                # exactly one seed was drawn from the host stream
    rbm._rng.set_state(st)
    V2 = rbm.sample_v(9, n_gibbs_steps=5, n_temperatures=4)   # the same host seed: the same samples
    assert same(V1, V2)
    for k, v in rbm.get_tf_params(scope='weights').items():
        assert same(v, before[k])
    # an explicit ladder and start; one temperature is plain Gibbs (no pair, no rate)
    rbm._rng.set_state(st)
    V3 = rbm.sample_v(9, n_gibbs_steps=5, betas=np.linspace(0, 1, 5)[1:], V_init=np.zeros((9, NV)))
    assert V3.shape == (9, NV)
    V4, r4 = rbm.sample_v(3, n_gibbs_steps=2, n_temperatures=1, return_stats=True)
    assert V4.shape == (3, NV) and r4.shape == (0,)
    for bad in (dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.5, 0.9]), dict(n_temperatures=0), dict(n_gibbs_steps=0),
                dict(V_init=np.zeros((8, NV)))):
        with pytest.raises(ValueError):
            rbm.sample_v(9, **bad)


def test_public_refusals(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM, MultinomialRBM
    kw = dict(n_visible=NV, n_hidden=NH, batch_size=BS, max_epoch=1, random_seed=1337, verbose=False)
    g = GaussianRBM(learning_rate=1e-3, model_path=str(tmp_path / 'g') + '/', **kw).fit(XTRAIN)
    with pytest.raises(NotImplementedError, match='Gaussian'):
        g.sample_v(3)
    m = MultinomialRBM(n_samples=3, model_path=str(tmp_path / 'm') + '/', **kw).fit(XTRAIN)
    with pytest.raises(NotImplementedError, match='Multinomial'):
        m.sample_v(3)
    r64 = BernoulliRBM(dtype='float64', model_path=str(tmp_path / 'f') + '/', **kw).fit(XTRAIN)
    with pytest.raises(NotImplementedError, match='float64'):
        r64.sample_v(3)
    for flag in ('dbm_first', 'dbm_last'):
        r = BernoulliRBM(model_path=str(tmp_path / flag) + '/', **dict(kw, **{flag: True})).fit(XTRAIN)
        with pytest.raises(NotImplementedError, match='dbm_first'):
            r.sample_v(3)
