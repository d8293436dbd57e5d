"""-m gpu: parallel tempering of a DBM - the two-segment RT flavour of act_kernel, pt_init_kernel with an h2
layer, the shared pt_swap / pt_gather kernels, bm_dbm_pt_init / _sweep / _read and DBM.sample_v_tempered.

The engine is compared BIT FOR BIT (view(uint32)) with the CPU twin of tests/dbm_pt_twin.py: the states of all three layers at
beta = 1, the ladder index of every row and the swap counters, after each of two consecutive calls.  Shapes (v, h1, h2), the
smallest at which the two-segment RT kernel can go wrong: (37, 20, 11) with 5 chains x 3 temperatures (ragged in every dimension
and in both K segments, fewer rows than a tile), (70, 65, 33) with 7 x 4 (both segments cross a BK boundary with a remainder, I
crosses a tile), (64, 64, 64) with 8 x 4 (the aligned fast path, x-major operands in the single-segment passes); 0.5 N(0, 1)
weights, 4 steps per call: both swap parities, acceptance neither 0 nor 1.  The swap decision compares a uniform with a double
exp(): every case first asserts on the twin that NO draw lies within 1e-9 of its threshold (the seed was chosen so), and then
excludes nothing."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import clamp_twin
from tests import dbm_pt_twin as T
from tests import pt_twin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 515151
SHAPES = [((37, 20, 11), 3, 5), ((70, 65, 33), 4, 7), ((64, 64, 64), 4, 8)]            # (V, n1, n2), R, M
FULL = (784, 512, 1024)
STEPS = 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def dbm_params(n):
    """0.5 N(0, 1) weights (0.05 N(0, 1) at the full size: energies of a few tens, not thousands), biases in +-0.3"""
    sc = np.float32(0.05 if n[0] > 256 else 0.5)
    return dict(W=[orc.normal(SEED, 1 + i, 0, n[i] * n[i + 1]).reshape(n[i], n[i + 1]) * sc for i in range(len(n) - 1)],
                vb=(orc.uniform(SEED, 10, 0, n[0]) - np.float32(0.5)) * np.float32(0.6),
                hb=[(orc.uniform(SEED, 11 + i, 0, n[i + 1]) - np.float32(0.5)) * np.float32(0.6) for i in range(len(n) - 1)])


def ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(np.float32)


def start(M, V):
    return (orc.uniform(SEED, 20, 0, M * V) < 0.5).astype(np.float32).reshape(M, V)


def dbm_engine(n, p, rows=4, **kw):
    from boltzmann_machines_amd.engine import DbmEngine
    eng = DbmEngine(n[0], list(n[1:]), n_particles=rows, batch_size=rows, **kw)     # (neither bounds the ensemble)
    for i in range(len(n) - 1):
        s = '_%d' % i if i else ''
        eng.set('W' + s, p['W'][i])
        eng.set('hb' + s, p['hb'][i])
    eng.set('vb', p['vb'])
    eng.seed(SEED)
    return eng


def snapshot(V, H, idx, swaps):
    d = dict(V=np.array(V), idx=np.array(idx, np.int32).reshape(-1), swaps=np.array(swaps, np.int64))
    for i, h in enumerate(H):
        d['H%d' % (i + 1)] = np.array(h)
    return d


def engine_read(eng, M):
    from boltzmann_machines_amd._ffi import DeviceArray
    Vd = DeviceArray((M, eng.V))
    Hd = [DeviceArray((M, k)) for k in eng.n_hiddens]
    swaps, idx = eng.pt_read(Vd, *Hd)
    return snapshot(Vd.numpy(), [h.numpy() for h in Hd], idx, swaps)


def engine_run(eng, M, R, calls, V0=None, chain0=0):
    """pt_init, then one pt_sweep per entry of `calls`; the snapshot after every call"""
    from boltzmann_machines_amd._ffi import DeviceArray
    eng.pt_init(M, ladder(R), DeviceArray.from_numpy(V0) if V0 is not None else None, chain0=chain0)
    out = []
    for k in calls:
        eng.pt_sweep(k)
        out.append(engine_read(eng, M))
    return out


@functools.lru_cache(maxsize=None)
def twin_run(n, R, M, calls, with_v0=False, chain0=0, rbm_sites=False):
    """the same on the twin (computed once per case, shared, never modified), + the smallest tie margin"""
    sites = dict(h=clamp_twin.SITE_H, v=clamp_twin.SITE_V, swap=pt_twin.SITE_PT_SWAP, start=pt_twin.SITE_PT_V0) if rbm_sites else None
    e = T.Ensemble(dbm_params(n), M, ladder(R), seed=SEED, chain0=chain0, V0=start(M, n[0]) if with_v0 else None, sites=sites)
    out = []
    for call, k in enumerate(calls):
        e.sweep(k, call=call)
        v, H = e.read()
        out.append(snapshot(v, H, e.idx, e.cnt))
    return out, (min(e.margins) if e.margins else np.inf)


def assert_twin_is_decisive(n, R, M, calls, mixed=True, **kw):
    want, margin = twin_run(n, R, M, calls, **kw)
    assert margin >= 1e-9, 'a swap draw of this case lies within 1e-9 of its threshold: choose another seed'
    att, acc = want[-1]['swaps']
    assert np.all(att > 0) and (not mixed or 0 < acc.sum() < att.sum())
    return want


def assert_same_snapshot(got, want, what):
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        if k[0] in 'VH':
            assert same(got[k], want[k]), '%s: %s differs from the twin in %d entries' % (what, k, int(np.sum(bits(got[k]) != bits(want[k]))))
    assert np.array_equal(got['idx'], want['idx']), '%s: ladder indices differ' % what
    assert np.array_equal(got['swaps'], want['swaps']), '%s: swap counters %s against %s' % (what, got['swaps'].tolist(), want['swaps'].tolist())


@pytest.mark.parametrize('with_v0', [False, True])
@pytest.mark.parametrize('n,R,M', SHAPES)
def test_engine_matches_twin(gpu_lib, n, R, M, with_v0):
    """after one call and after two consecutive calls (call counter, parity continuation); random start and a given one"""
    calls = (STEPS, STEPS)
    want = assert_twin_is_decisive(n, R, M, calls, with_v0=with_v0)
    eng = dbm_engine(n, dbm_params(n))
    got = engine_run(eng, M, R, calls, V0=start(M, n[0]) if with_v0 else None)
    eng.close()
    for c, (g, w) in enumerate(zip(got, want)):
        assert_same_snapshot(g, w, '%s R=%d M=%d, call %d' % (n, R, M, c))
        assert all(set(np.unique(g[k])) <= {0.0, 1.0} for k in ('V', 'H1', 'H2'))
        assert np.array_equal(np.sort(g['idx'].reshape(M, R), axis=1), np.tile(np.arange(R), (M, 1)))


def test_parity_continues_across_calls(gpu_lib):
    """an odd number of steps in the first call: the second one starts with the odd pairs"""
    n, R, M = SHAPES[0]
    calls = (3, 2)
    want = assert_twin_is_decisive(n, R, M, calls)
    eng = dbm_engine(n, dbm_params(n))
    got = engine_run(eng, M, R, calls)
    eng.close()
    for c, (g, w) in enumerate(zip(got, want)):
        assert_same_snapshot(g, w, 'calls of 3 and 2 steps, call %d' % c)


def test_full_size_two_steps(gpu_lib):
    """784-512-1024, 8 chains x 4 temperatures, 2 steps"""
    want = assert_twin_is_decisive(FULL, 4, 8, (2,), mixed=False)
    eng = dbm_engine(FULL, dbm_params(FULL))
    got = engine_run(eng, 8, 4, (2,))
    eng.close()
    assert_same_snapshot(got[0], want[0], '784-512-1024')


GEO_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tests import test_dbm_pt_gpu as G
n, R, M = G.SHAPES[%(shape)d]
eng = G.dbm_engine(n, G.dbm_params(n))
got = G.engine_run(eng, M, R, (G.STEPS,))[0]
eng.close()
np.savez(%(out)r, **got)
print('DBM_PT_GEOMETRY_OK')
'''


@pytest.mark.parametrize('shape,geo', [(0, '4'), (0, '1'), (1, '8'), (1, '103'), (1, '5'), (2, '6'), (2, '7'), (2, '9')])
def test_forced_geometries_give_the_twins_bits(gpu_lib, tmp_path, shape, geo):
    """the same call under a forced act_geo value (read once per process: one subprocess each, as test_pt_gpu.py): the states
    and - through the slot partials of the two-segment pass - the swap decisions of the twin.  64 x 32 and 32 x 32 tiles at the
    ragged shape; 8 waves, 32 x 32 / BK = 32 with register staging and 64 x 32 / BK = 32 at three workgroups per CU where the
    segments cross BK; the 64 x 64 tiles and 64 x 32 / BK = 32 at two workgroups per CU at the aligned shape"""
    n, R, M = SHAPES[shape]
    want = assert_twin_is_decisive(n, R, M, (STEPS, STEPS))[0]
    out = str(tmp_path / ('geo%s.npz' % geo))
    r = subprocess.run([sys.executable, '-c', GEO_SCRIPT % dict(root=ROOT, shape=shape, out=out)],
                       env=dict(os.environ, BM355_DEBUG='act_geo=' + geo), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'DBM_PT_GEOMETRY_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert_same_snapshot(dict(np.load(out)), want, 'act_geo=%s' % geo)


def test_chain_slices_reproduce_the_whole(gpu_lib):
    """chains 2..4 of the 5-chain run are the 3-chain run at chain0 = 2 (random start: the start draws at the global row too)"""
    n, R, M = SHAPES[0]
    eng = dbm_engine(n, dbm_params(n))
    whole = engine_run(eng, M, R, (STEPS,))[0]
    eng.seed(SEED)
    part = engine_run(eng, 3, R, (STEPS,), chain0=2)[0]
    eng.close()
    assert all(same(whole[k][2:], part[k]) for k in ('V', 'H1', 'H2'))
    assert np.array_equal(whole['idx'].reshape(M, R)[2:], part['idx'].reshape(3, R))
    want = assert_twin_is_decisive(n, R, 3, (STEPS,), mixed=False, chain0=2)[0]
    assert_same_snapshot(part, want, 'chain0 = 2')


def test_one_hidden_layer_against_the_rbm_entry_points(gpu_lib):
    """L = 1 on the parameters of the first layer: bm_dbm_pt_* equals the twin, and bm_rbm_pt_* on the same parameters equals the
    SAME twin told the RBM's RNG sites (4 / 3 / 10 / 11 where the DBM draws at 8 / 12 / 14 / 15: the two engines cannot give the
    same bits, they are the same algorithm on different streams)"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    n3, R, M = SHAPES[0]
    n = n3[:2]
    p = dbm_params(n)
    calls = (STEPS, STEPS)
    want = assert_twin_is_decisive(n, R, M, calls)
    eng = dbm_engine(n, p)
    got = engine_run(eng, M, R, calls)
    with pytest.raises(Exception, match='one hidden layer'):
        eng.pt_read(DeviceArray((M, n[0])), DeviceArray((M, n[1])), DeviceArray((M, 4)))
    eng.close()
    for c, (g, w) in enumerate(zip(got, want)):
        assert_same_snapshot(g, w, 'L = 1, call %d' % c)
    want_r = assert_twin_is_decisive(n, R, M, calls, rbm_sites=True)
    rbm = RbmEngine(n[0], n[1], max_batch=4)
    for k, v in (('W', p['W'][0]), ('vb', p['vb']), ('hb', p['hb'][0])):
        rbm.set(k, v)
    rbm.seed(SEED)
    rbm.pt_init(M, ladder(R))
    for c, k in enumerate(calls):
        rbm.pt_sweep(k)
        Vd, Hd = DeviceArray((M, n[0])), DeviceArray((M, n[1]))
        swaps, idx = rbm.pt_read(Vd, Hd)
        assert_same_snapshot(snapshot(Vd.numpy(), [Hd.numpy()], idx, swaps), want_r[c], 'bm_rbm_pt_*, call %d' % c)
    rbm.close()


def test_other_entry_points_are_untouched(gpu_lib):
    """bm_dbm_sample_v and one bm_dbm_train_step give the same bits whether or not a tempered call ran before them on the handle"""
    from boltzmann_machines_amd._ffi import DeviceArray
    n, R, M = SHAPES[1]
    B = 8
    p = dbm_params(n)
    X = start(B, n[0])
    init = dict(v=start(B, n[0]), h=(orc.uniform(SEED, 21, 0, B * n[1]) < 0.5).astype(np.float32).reshape(B, n[1]),
                h_1=(orc.uniform(SEED, 22, 0, B * n[2]) < 0.5).astype(np.float32).reshape(B, n[2]))
    names = ('W', 'W_1', 'vb', 'hb', 'hb_1', 'dW', 'dW_1', 'v', 'h', 'h_1', 'mu', 'mu_1')
    results = []
    for tempered in (False, True):
        eng = dbm_engine(n, p, rows=B, max_mf_updates=5, mf_tol=1e-5)
        for k, v in init.items():
            eng.set(k, v)
        if tempered:
            before = [eng.get(k) for k in names]
            engine_run(eng, M, R, (2,))
            assert all(same(a, eng.get(k)) for a, k in zip(before, names))        # nothing of the handle moved
            eng.seed(SEED)
        Vd = DeviceArray((B, n[0]))
        eng.sample_v(2, Vd)
        eng.train_step(DeviceArray.from_numpy(X), 0.05, 0.9, 1)
        eng.sync()
        results.append([Vd.numpy()] + [eng.get(k) for k in names])
        if tempered:                                   # ... and the ensemble is still there behind them
            assert engine_read(eng, M)['idx'].size == M * R
        eng.close()
    for a, b in zip(*results):
        assert same(a, b)


def test_entry_point_errors(gpu_lib):
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray, UNIT_GAUSSIAN, UNIT_MULTINOMIAL
    n = (20, 12, 9)
    p = dbm_params(n)
    eng = dbm_engine(n, p)
    with pytest.raises(Bm355Error, match='pt_init first'):
        eng.pt_sweep(1)
    with pytest.raises(Bm355Error, match='pt_init first'):
        eng.pt_read(DeviceArray((3, n[0])))
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
    eng.set_sigmoid_literal(True)                                # switched on behind the init: the sweep refuses as well
    with pytest.raises(Bm355Error, match='literal'):
        eng.pt_sweep(1)
    with pytest.raises(Bm355Error, match='literal'):
        eng.pt_init(3, [0.5, 1.0])
    eng.close()
    for kw, word in ((dict(v_unit=UNIT_GAUSSIAN), 'Gaussian'), (dict(h_units=[0, UNIT_MULTINOMIAL], n_samples=[0, 3]), 'Multinomial')):
        eng = dbm_engine(n, p, **kw)
        with pytest.raises(Bm355Error, match=word):
            eng.pt_init(3, [0.5, 1.0])
        eng.close()
    n4 = (20, 12, 9, 7)
    eng = dbm_engine(n4, dbm_params(n4))
    with pytest.raises(Bm355Error, match='OLD layer above'):
        eng.pt_init(3, [0.5, 1.0])
    eng.close()
    from boltzmann_machines_amd.engine import DbmEngine64
    with pytest.raises(NotImplementedError, match='float64'):
        DbmEngine64.pt_init(None, 3, [1.0])


# ------------------------------------------------------------------------------------------------ public API
NV, NH, NH2, BS = 12, 8, 6, 5
XTRAIN = (orc.uniform(SEED, 60, 0, 20 * NV) < 0.4).astype(np.float32).reshape(20, NV)


def _fitted_dbm(tmp_path, tag='', first=None, second=None, third=False, **dbm_kw):
    from boltzmann_machines_amd import DBM, BernoulliRBM
    kw = dict(max_epoch=1, batch_size=BS, verbose=False)
    r1 = first or BernoulliRBM(n_visible=NV, n_hidden=NH, dbm_first=True, random_seed=11,
                               model_path=str(tmp_path / (tag + 'r1')) + '/', **kw)
    r1.fit(XTRAIN)
    r2 = second or BernoulliRBM(n_visible=NH, n_hidden=NH2, dbm_last=not third, random_seed=12,
                                model_path=str(tmp_path / (tag + 'r2')) + '/', **kw)
    H1 = r1.transform(XTRAIN)
    r2.fit(H1)
    rbms = [r1, r2]
    if third:
        r3 = BernoulliRBM(n_visible=NH2, n_hidden=4, dbm_last=True, random_seed=13, model_path=str(tmp_path / (tag + 'r3')) + '/', **kw)
        r3.fit(r2.transform(H1))
        rbms.append(r3)
    dbm = DBM(rbms=rbms, n_particles=BS, n_gibbs_steps=1, max_mf_updates=5, mf_tol=1e-5, learning_rate=0.01, max_epoch=1,
              batch_size=BS, random_seed=1337, verbose=False, model_path=str(tmp_path / (tag + 'dbm')) + '/', **dbm_kw)
    return dbm


def test_public_sample_v_tempered(gpu_lib, tmp_path):
    dbm = _fitted_dbm(tmp_path).fit(XTRAIN)
    state = lambda: [dbm._engine.get(k) for k in ('W', 'W_1', 'vb', 'hb', 'hb_1', 'v', 'h', 'h_1', 'mu', 'mu_1')]
    before = state()
    st = dbm._rng.get_state()
    V1, rates = dbm.sample_v_tempered(9, n_gibbs_steps=5, n_temperatures=4, return_stats=True)          # 9 > n_particles
    assert V1.shape == (9, NV) and set(np.unique(V1)) <= {0.0, 1.0}
    assert rates.shape == (3,) and np.all((rates >= 0) & (rates <= 1))
    swaps, idx = dbm._engine.pt_read()
    assert idx.shape == (9, 4) and np.array_equal(rates, swaps[1] / swaps[0].astype(np.float64))
    assert np.all(swaps[0] > 0)
    after_call = dbm.make_random_seed()
    dbm._rng.set_state(st)
    dbm.make_random_seed()
    assert after_call == dbm.make_random_seed()                # exactly one seed was drawn from the host stream
    dbm._rng.set_state(st)
    V2 = dbm.sample_v_tempered(9, n_gibbs_steps=5, n_temperatures=4)   # the same host seed: the same samples
    assert same(V1, V2)
    assert all(same(a, b) for a, b in zip(before, state()))
    # the default ladder is BernoulliRBM.sample_v's
    dbm._rng.set_state(st)
    V3 = dbm.sample_v_tempered(9, n_gibbs_steps=5, betas=np.linspace(0., 1., 5)[1:])
    assert same(V1, V3)
    V4 = dbm.sample_v_tempered(9, n_gibbs_steps=3, betas=[0.25, 0.5, 1.0], V_init=np.zeros((9, NV)))
    assert V4.shape == (9, NV)
    V5, r5 = dbm.sample_v_tempered(3, n_gibbs_steps=2, n_temperatures=1, return_stats=True)
    assert V5.shape == (3, NV) and r5.shape == (0,)
    for bad in (dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.5, 0.9]), dict(n_temperatures=0), dict(n_gibbs_steps=0),
                dict(V_init=np.zeros((8, NV)))):
        with pytest.raises(ValueError):
            dbm.sample_v_tempered(9, **bad)
    # sample_v keeps the reference's signature and behaviour: activation probabilities of the particles
    P = dbm.sample_v(n_gibbs_steps=1)
    assert P.shape == (BS, NV) and np.all((P >= 0) & (P <= 1))


def test_public_refusals(gpu_lib, tmp_path):
    from boltzmann_machines_amd import GaussianRBM, MultinomialRBM
    kw = dict(max_epoch=1, batch_size=BS, verbose=False)
    d = _fitted_dbm(tmp_path, 'm', second=MultinomialRBM(n_visible=NH, n_hidden=NH2, n_samples=3, dbm_last=True, random_seed=3,
                                                        model_path=str(tmp_path / 'm2') + '/', **kw))
    with pytest.raises(NotImplementedError, match='Multinomial'):
        d.sample_v_tempered(3)
    d = _fitted_dbm(tmp_path, 'g', first=GaussianRBM(n_visible=NV, n_hidden=NH, dbm_first=True, learning_rate=1e-3, random_seed=4,
                                                     model_path=str(tmp_path / 'g1') + '/', **kw))
    with pytest.raises(NotImplementedError, match='Gaussian'):
        d.sample_v_tempered(3)
    d = _fitted_dbm(tmp_path, 't', third=True)
    with pytest.raises(NotImplementedError, match='OLD layer above'):
        d.sample_v_tempered(3)
    d = _fitted_dbm(tmp_path, 'f', dtype='float64')
    with pytest.raises(NotImplementedError, match='float64'):          # (refused before anything is built)
        d.sample_v_tempered(3)
    d = _fitted_dbm(tmp_path, 'l')
    d.set_mean_field_arithmetic('reference')
    with pytest.raises(NotImplementedError, match='literal'):
        d.sample_v_tempered(3)
