"""Softmax (categorical) visible units (bm_rbm_set_visible_groups) on the GPU: every state-carrying result bit for
bit against the CPU twin (tests/softmax_v_twin.py) - bm_rbm_sample_v_from_h, the edges of the softmax through the ABI, the update,
the epoch loop, transform / gibbs / metrics, CategoricalRBM - and the C-ABI refusals."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import multinomial_probes as P
from tests import softmax_v_twin as T
from tests.clamp_twin import act2

pytestmark = pytest.mark.gpu
f32 = np.float32
STATE = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')
# (K, G): V = 68, 132, 72, 80 - past one tile, no multiples of the tile, V % 4 == 0 - and widths / layer sizes off the quad
ALIGNED = [(2, 34), (4, 33), (8, 9), (16, 5)]
GENERIC = [(2, 35), (3, 1), (5, 13), (10, 7), (26, 3)]


def bits_equal(g, c, what=''):
    g, c = np.ascontiguousarray(g, f32), np.ascontiguousarray(c, f32)
    bad = int(np.sum(g.view(np.uint32) != c.view(np.uint32)))
    assert bad == 0, '%s: %d / %d elements differ bitwise (max abs diff %.3e)' % (what, bad, g.size, float(np.nanmax(np.abs(g - c))))


def params(V, H, seed=1, w_std=0.5, sigma=False):
    rng = np.random.RandomState(seed)
    p = dict(W=(w_std * rng.randn(V, H)).astype(f32), vb=(0.3 * rng.randn(V)).astype(f32), hb=(0.3 * rng.randn(H)).astype(f32))
    if sigma:
        p['sigma'] = np.linspace(0.5, 1.5, V).astype(f32)
    return p


def bitmap(B, n, seed):
    return (np.random.RandomState(seed).uniform(size=(B, n)) < 0.5).astype(f32)


def categories(B, G, K, seed):
    return T.one_hot(np.random.RandomState(seed).randint(0, K, (B, G)), K)


def engine(p, B, K=0, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = p['W'].shape
    eng = RbmEngine(V, H, max_batch=B, v_groups=K, **kw)
    for n, a in p.items():
        eng.set(n, a)
    return eng


def pair(K, G, H, B, seed, p=None, w_std=0.05, **kw):
    p = p or params(G * K, H, w_std=w_std)
    eng = engine(p, B, K, **kw)
    twin = T.SoftmaxVRBM(p, K, seed, **{k: v for k, v in kw.items()})
    eng.seed(seed)
    return eng, twin


def state_equal(eng, twin, what=''):
    for n in STATE:
        bits_equal(eng.get(n), twin.p[n], '%s %s' % (what, n))


def run_sample_v(eng, Hs, seed, row0, means=True, states=True):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    B = len(Hs)
    Md = DeviceArray((B, eng.V), f32) if means else None
    Sd = DeviceArray((B, eng.V), f32) if states else None
    eng.seed(seed)
    eng.set_row_offset(row0)
    eng.sample_v_from_h(as_device(Hs), B, Md, Sd)
    eng.sync()
    eng.set_row_offset(0)
    return (Md.numpy() if means else None), (Sd.numpy() if states else None)


# ---- 1. bm_rbm_sample_v_from_h
@pytest.mark.parametrize('K,G', ALIGNED + GENERIC)
def test_sample_v_from_h(gpu_lib, K, G):
    B, H, V = 37, 24, G * K
    p = params(V, H)
    Hs = bitmap(B, H, 3)
    eng = engine(p, B, K)
    for row0 in (0, 1000):
        gm, gs = run_sample_v(eng, Hs, 7, row0)
        cm, cs = T.sample_v_from_h(p, Hs, K, 7, 0, row0)
        bits_equal(gm, cm, 'means row0=%d' % row0)
        bits_equal(gs, cs, 'states row0=%d' % row0)
        assert np.all(gs.reshape(B, G, K).sum(axis=2) == 1) and np.all((gs == 0) | (gs == 1))
    _, gs = run_sample_v(eng, Hs, 7, 1000, means=False)                    # either output may be null
    bits_equal(gs, cs, 'states alone')
    gm, _ = run_sample_v(eng, Hs, 7, 1000, states=False)
    bits_equal(gm, cm, 'means alone')
    # the call counter advances by one: a second call under the same seed draws at call 1
    eng.seed(7)
    eng.set_row_offset(1000)
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    Sd = DeviceArray((B, V), f32)
    eng.sample_v_from_h(as_device(Hs), B, None, Sd)
    eng.sample_v_from_h(as_device(Hs), B, None, Sd)
    eng.sync()
    bits_equal(Sd.numpy(), T.sample_v_from_h(p, Hs, K, 7, 1, 1000)[1], 'second call')
    # K = 0 turns the groups off again: the Bernoulli conditional
    eng.set_visible_groups(0)
    gm, gs = run_sample_v(eng, Hs, 7, 1000)
    cm, cs = act2(Hs, np.ascontiguousarray(p['W'].T), None, None, p['vb'], None, 1.0, 0, 1, 7, T.SITE_V, 0, 1000)
    bits_equal(gm, cm, 'Bernoulli means after set_visible_groups(0)')
    bits_equal(gs, cs, 'Bernoulli states after set_visible_groups(0)')
    eng.close()


@pytest.mark.parametrize('v_unit', [0, 1])
@pytest.mark.parametrize('V', [68, 65])
def test_sample_v_from_h_other_units(gpu_lib, v_unit, V):
    """the same call on a Bernoulli and on a Gaussian handle against act2"""
    B, H = 37, 24
    p = params(V, H, sigma=bool(v_unit))
    Hs = bitmap(B, H, 4)
    eng = engine(p, B, 0, v_unit=v_unit)
    Wt = np.ascontiguousarray(p['W'].T)
    for row0 in (0, 1000):
        cm, cs = act2(Hs, Wt, None, None, p['vb'], p.get('sigma'), 1.0, v_unit, 1, 9, T.SITE_V, 0, row0)
        gm, gs = run_sample_v(eng, Hs, 9, row0)
        bits_equal(gm, cm, 'means')
        bits_equal(gs, cs, 'states')
        _, gs = run_sample_v(eng, Hs, 9, row0, means=False)
        bits_equal(gs, cs, 'states alone')
    eng.close()


# ---- 2. the fused flavour against the generic pair, and in every geometry
def sample_v_digests():
    """one digest per fused shape of the means and states bm_rbm_sample_v_from_h returns (row0 = 1000)"""
    out = []
    for K, G in ALIGNED:
        eng = engine(params(G * K, 24), 37, K)
        gm, gs = run_sample_v(eng, bitmap(37, 24, 3), 7, 1000)
        eng.close()
        out.append(hashlib.sha1(gm.tobytes() + gs.tobytes()).hexdigest())
    return out


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ('8', '4', '1', '3', '108', '104', '101', '103', '208', '6', '5', '7', '9')      # what launch_act_as accepts
CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_softmax_v_gpu as G
print('SOFTMAX_V_DIGEST', ' '.join(G.sample_v_digests()))
'''


def test_fused_generic_and_every_geometry_hold_the_twins_bits(gpu_lib):
    """the four fused shapes in fresh child processes (BM355_DEBUG is read once per process): one under sm_fused=0 - the generic
    logits + softmax_groups_kernel pair - and one per forced act_geo, each under its own time limit; the first failure ends the
    test (as tests/test_nrelu_gpu.py::test_every_geometry_holds_the_twins_bits)"""
    want = []
    for K, G in ALIGNED:
        cm, cs = T.sample_v_from_h(params(G * K, 24), bitmap(37, 24, 3), K, 7, 0, 1000)
        want.append(hashlib.sha1(cm.tobytes() + cs.tobytes()).hexdigest())
    assert sample_v_digests() == want
    for dbg in ('sm_fused=0',) + tuple('act_geo=' + g for g in GEOMETRIES):
        env = dict(os.environ, BM355_DEBUG=dbg)
        r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'SOFTMAX_V_DIGEST' in r.stdout, '%s: %s' % (dbg, r.stdout[-2000:] + r.stderr[-4000:])
        got = r.stdout.split('SOFTMAX_V_DIGEST', 1)[1].split()
        assert got == want, '%s: shapes %r differ from the twin' % (dbg, [s_ for s_, g, w in zip(ALIGNED, got, want) if g != w])


# ---- 3. edges through the ABI: W = 0, the logit families in vb
@pytest.mark.parametrize('K', [8, 10])
def test_edges_through_the_abi(gpu_lib, K):
    """W = 0 makes the prop-down give 0 + vb exactly.  250 groups per row, 640 rows in one call: 160 000 draws per family, taken
    as 8 rows of 20 000 draws (the probes' ROWS x M): the derived bound on the means, the exact count checks, and the chi-square
    of the drawn categories against Z_CAP wherever dof >= 10; families a, b and g at K >= 7 can carry a test
    (multinomial_probes.carries_a_test, fixed before any run)"""
    G, B, H, M = 250, 640, 4, 20000
    assert G * B == P.ROWS * M
    V = G * K
    p = dict(W=np.zeros((V, H), f32), vb=np.zeros(V, f32), hb=np.zeros(H, f32))
    eng = engine(p, B, K)
    Hs = bitmap(B, H, 5)
    tally = P.Tally()
    for name, l in P.logit_sets(K):
        eng.set('vb', np.tile(l, G))
        gm, gs = run_sample_v(eng, Hs, 31, 0)
        what = 'device %s K=%d' % (name, K)
        P.check_means(l, gm.reshape(B * G, K), 1, P.F32, what)
        s3 = gs.reshape(B * G, K)
        assert np.all((s3 == 0) | (s3 == 1)) and np.all(s3.sum(axis=1) == 1), what
        P.check_counts(l, s3, 1, P.F32, name, what)
        bits_equal(gm, T.softmax_groups(np.tile(l, (B, G)).astype(f32), K, 0)[0], what + ' against the twin')
        tally.add(l, s3.reshape(P.ROWS, M, K).sum(axis=1), M, P.F32, name, what)
    tested = tally.assert_statistical_leg()
    assert len(tested) >= 3
    eng.close()


# ---- 4. training bit for bit with the twin
def three_updates(eng, twin, X, k, lr=0.05, mom=0.9, what=''):
    from boltzmann_machines_amd.engine import as_device
    Xd = as_device(X)
    for s in range(3):
        eng.train_step(Xd, len(X), lr, mom, k)
        twin.train_step(X, lr, mom, k)
        state_equal(eng, twin, '%s update %d' % (what, s))


TRAIN_SHAPES = [(4, 33, 24, 37), (8, 9, 40, 16), (5, 13, 24, 37), (2, 35, 17, 10)]


@pytest.mark.parametrize('sample_v', [False, True])
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('K,G,H,B', TRAIN_SHAPES)
def test_train_step(gpu_lib, K, G, H, B, k, sample_v):
    eng, twin = pair(K, G, H, B, 3, sample_v_states=sample_v, l2=1e-3)
    three_updates(eng, twin, categories(B, G, K, 5), k)
    eng.close()


def test_train_step_sparsity(gpu_lib):
    K, G, H, B = 5, 13, 24, 37
    eng, twin = pair(K, G, H, B, 3, sparsity_cost=0.1, sparsity_target=0.2)
    three_updates(eng, twin, categories(B, G, K, 6), 1)
    eng.close()


def test_train_epoch(gpu_lib):
    from boltzmann_machines_amd.engine import as_device
    K, G, H, B = 4, 33, 24, 37
    N = 2 * B + 7
    X = categories(N, G, K, 8)
    eng, twin = pair(K, G, H, B, 5)
    loop, _ = pair(K, G, H, B, 5)
    Xd = as_device(X)
    eng.train_epoch(Xd, N, B, 0.05, 0.9, 1)
    for s in range(0, N, B):
        loop.train_step(Xd, min(B, N - s), 0.05, 0.9, 1, row=s)
    twin.train_epoch(X, B, 0.05, 0.9, 1)
    for n in STATE:
        bits_equal(eng.get(n), loop.get(n), 'epoch against loop: ' + n)
    state_equal(eng, twin, 'epoch against twin')
    eng.close(); loop.close()


@pytest.mark.parametrize('K,G,H,B', [(4, 33, 24, 37), (5, 13, 24, 37)])
def test_transform_gibbs_metrics(gpu_lib, K, G, H, B):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    V = G * K
    eng, twin = pair(K, G, H, B, 11, w_std=0.3, sample_v_states=True)
    X = categories(B, G, K, 9)
    Xd = as_device(X)
    Hd = DeviceArray((B, H), f32)
    eng.transform(Xd, B, 2, Hd)
    bits_equal(Hd.numpy(), twin.transform(X, 2), 'transform')
    H0 = bitmap(B, H, 10)
    Hd, Vd = as_device(H0), DeviceArray((B, V), f32)
    eng.gibbs(Hd, Vd, B, 2)
    ch, cv = twin.gibbs(H0, 2)
    bits_equal(Hd.numpy(), ch, 'gibbs h')
    bits_equal(Vd.numpy(), cv, 'gibbs v')
    assert np.all(cv.reshape(B, G, K).sum(axis=2) == 1)
    assert gpu_lib.bm_rbm_set_fast_binary(eng._h, 2) == 0             # accepted: the handle keeps running fp32
    Hd = as_device(H0)
    eng.gibbs(Hd, Vd, B, 2)
    ch, cv = twin.gibbs(H0, 2)
    bits_equal(Vd.numpy(), cv, 'gibbs v with fast-binary requested')
    out = eng.metrics(Xd, B, 1)
    msre, l2, fe = twin.metrics(X, 1)
    np.testing.assert_allclose([out[0], out[2], out[3]], [msre, l2, fe], rtol=1e-5)
    assert np.isnan(out[1])
    fe1 = eng.free_energy(Xd, B)
    rows = eng.free_energy_rows(Xd, B)
    np.testing.assert_allclose(fe1, twin.free_energy(X), rtol=1e-5)
    np.testing.assert_allclose(rows, T.free_energy64(twin.p, X), rtol=1e-5, atol=1e-5)
    # train_step_metrics (blocking and asynchronous) leaves the parameters train_step leaves
    out = eng.train_step_metrics(Xd, B, 0.05, 0.9, 1)
    assert np.isnan(out[1]) and np.all(np.isfinite(out[[0, 2, 3]]))
    twin.train_step(X, 0.05, 0.9, 1)
    state_equal(eng, twin, 'train_step_metrics')
    eng.train_step_metrics_async(Xd, B, 0.05, 0.9, 1)
    twin.train_step(X, 0.05, 0.9, 1)
    got = eng.collect_metrics()
    assert got.shape == (1, 4) and np.isnan(got[0, 1]) and np.all(np.isfinite(got[0, [0, 2, 3]]))
    state_equal(eng, twin, 'train_step_metrics_async')
    eng.close()


# ---- 5. the public class
def twin_sample_v(p, K, V0, seed, n_steps):
    """CategoricalRBM.sample_v: h ~ p(h | v_0) at call 0, then per step one bm_rbm_sample_v_from_h and one bm_rbm_sample_h call"""
    call = 0
    _, h = act2(V0, p['W'], None, None, p['hb'], None, 1.0, 0, 1, seed, T.SITE_H0, call, 0)
    v = None
    for _ in range(n_steps):
        call += 1
        _, v = T.visible_pass(h, p['W'], p['vb'], K, 1, seed, T.SITE_V, call, 0)
        call += 1
        _, h = act2(v, p['W'], None, None, p['hb'], None, 1.0, 0, 1, seed, T.SITE_H0, call, 0)
    return v


def test_categorical_rbm(gpu_lib, tmp_path):
    """CategoricalRBM fits the planted data of tests/test_softmax_v.py and reproduces the twin's parameters bit for bit; save /
    load_model; sample_v one-hot and independent of batch_size; sample_v_from_h against the twin"""
    import boltzmann_machines_amd as bm
    from boltzmann_machines_amd.utils import RNG
    from tests.test_softmax_v import PLANTED, planted_twin
    c = PLANTED
    G, K, H = c['G'], c['K'], c['H']
    host = RNG(seed=1337)
    seeds = [host.randint(2 ** 31 - 1) for _ in range(4)]          # of fit() and of the three stochastic calls after load_model
    twin, X, p0 = planted_twin(seeds[0])
    path = lambda n: str(tmp_path) + '/%s/' % n
    kw = dict(n_groups=G, n_categories=K, n_hidden=H, W_init=p0['W'], vb_init=p0['vb'], hb_init=p0['hb'], batch_size=c['batch'],
              learning_rate=c['lr'], momentum=c['mom'], l2=1e-4, max_epoch=c['epochs'], random_seed=1337, verbose=False,
              save_after_each_epoch=False, v_shape=(4, 3))
    m = bm.CategoricalRBM(model_path=path('a'), **kw)
    assert np.array_equal(m.encode(m.decode(X)), X)
    m.fit(X)
    w, acc = m.get_tf_params(scope='weights'), m.get_tf_params(scope='grads_accumulators')
    for n in ('W', 'vb', 'hb'):
        bits_equal(w[n], twin.p[n], 'fit ' + n)
    for n in ('dW', 'dvb', 'dhb'):
        bits_equal(acc[n], twin.p[n], 'fit ' + n)
    loaded = bm.CategoricalRBM.load_model(path('a'))
    assert (loaded.n_groups, loaded.n_categories, loaded.n_visible, loaded.epoch_) == (G, K, G * K, c['epochs'])
    bits_equal(loaded.get_tf_params(scope='weights')['W'], twin.p['W'], 'load_model W')
    bits_equal(loaded.transform(X), bm.CategoricalRBM.load_model(path('a')).transform(X), 'transform of two loads')
    # sample_v: one-hot rows, the same whatever batch_size, the twin's bits from a given start
    p = twin.state()
    V0 = categories(50, G, K, 12)
    loaded, small = bm.CategoricalRBM.load_model(path('a')), bm.CategoricalRBM.load_model(path('a')).set_params(batch_size=7)
    va, vb_ = loaded.sample_v(50, n_gibbs_steps=5, V_init=V0), small.sample_v(50, n_gibbs_steps=5, V_init=V0)
    bits_equal(va, vb_, 'sample_v over batch sizes')
    assert va.shape == (50, G * K) and np.all((va == 0) | (va == 1)) and np.all(va.reshape(50, G, K).sum(axis=2) == 1)
    bits_equal(va, twin_sample_v(p, K, V0, seeds[1], 5), 'sample_v against the twin')
    va, vb_ = loaded.sample_v(50, n_gibbs_steps=3), small.sample_v(50, n_gibbs_steps=3)
    bits_equal(va, vb_, 'sample_v from uniform categories over batch sizes')
    assert np.all(va.reshape(50, G, K).sum(axis=2) == 1)
    # sample_v_from_h: sliced by batch_size with the row offset set
    Hs = bitmap(50, H, 13)
    sa, ma = loaded.sample_v_from_h(Hs, return_means=True)                 # (the loaded model's third stochastic call)
    cm, cs = T.sample_v_from_h(p, Hs, K, seeds[3], 0, 0)
    sb = small.sample_v_from_h(Hs)
    bits_equal(sa, sb, 'sample_v_from_h over batch sizes')
    bits_equal(sa, cs, 'sample_v_from_h states against the twin')
    bits_equal(ma, cm, 'sample_v_from_h means against the twin')


def test_log_proba(gpu_lib, tmp_path):
    """log_proba = -F - log Z with the enumerated log Z of the 3 x 3 x 3 model, over all 27 states; log_Z is refused"""
    import boltzmann_machines_amd as bm
    p = T.small_model()
    _, X = T.all_visible_states(3, 3)
    logz = T.log_z_visible(p, 3, 3)
    m = bm.CategoricalRBM(3, 3, 3, W_init=p['W'], vb_init=p['vb'], hb_init=p['hb'], batch_size=10, random_seed=1, verbose=False,
                          model_path=str(tmp_path) + '/m/', v_shape=(3, 3)).init()
    lp = m.log_proba(X, logz)
    np.testing.assert_allclose(lp, -T.free_energy64(p, X) - logz, atol=1e-4, rtol=0)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-3
    with pytest.raises(ValueError) as e:
        m.log_Z()
    assert 'softmax visible units' in str(e.value)


# ---- 6. the C-ABI refusals
def test_set_visible_groups_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, as_device
    lib = gpu_lib
    V, H, B = 12, 8, 16

    def refused(rc, what):
        assert rc != 0, what + ' was accepted'
        msg = lib.bm_last_error().decode()
        assert 'softmax visible' in msg, '%s: %s' % (what, msg)

    p = params(V, H, w_std=0.05)
    X = categories(B, 4, 3, 2)
    for bad in (dict(v_unit=1), dict(h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=5), dict(h_unit=_ffi.UNIT_NRELU), dict(dbm_first=True),
                dict(dbm_last=True), dict(dropout=0.8)):
        eng = engine(p, B, 0, **bad)
        refused(lib.bm_rbm_set_visible_groups(eng._h, 3), 'set_visible_groups with %r' % (bad,))
        eng.train_step(as_device(X), B, 0.01, 0.9, 1)             # the handle is what it was
        eng.sync()
        eng.close()
        with pytest.raises(_ffi.Bm355Error) as e:
            RbmEngine(V, H, max_batch=B, v_groups=3, **bad)
        assert 'softmax visible' in str(e.value)
    eng = engine(p, B, 0)
    for K in (5, 1, -2, 24):
        refused(lib.bm_rbm_set_visible_groups(eng._h, K), 'K = %d' % K)
    for attach, detach in ((lambda: lib.bm_rbm_set_centering(eng._h, 1, 0.01, 0.01), lambda: lib.bm_rbm_set_centering(eng._h, 0, 0.0, 0.0)),
                           (lambda: lib.bm_rbm_set_classes(eng._h, 3), lambda: lib.bm_rbm_set_classes(eng._h, 0)),
                           (lambda: lib.bm_rbm_set_fast_weights(eng._h, 1, 0.01, 0.95), lambda: lib.bm_rbm_set_fast_weights(eng._h, 0, 0.0, 0.0))):
        assert attach() == 0
        refused(lib.bm_rbm_set_visible_groups(eng._h, 3), 'set_visible_groups on a handle with a mode attached')
        assert detach() == 0
    betas = np.array([0.5, 1.0], f32)
    assert lib.bm_rbm_pt_init(eng._h, B, 2, betas.ctypes.data_as(C.c_void_p), None, 0) == 0
    refused(lib.bm_rbm_set_visible_groups(eng._h, 3), 'set_visible_groups on a handle with a tempered ensemble')
    # a handle that never had groups is the Bernoulli handle it was: three updates against the Bernoulli twin
    from oracle import oracle as orc
    twin = orc.OracleRBM(V, H, l2=1e-4)
    for n in ('W', 'vb', 'hb'):
        twin.p[n][...] = p[n]
    twin.set_seed(3)
    eng.close()
    eng = engine(p, B, 0)
    eng.seed(3)
    Xd = as_device(X)
    for s in range(3):
        eng.train_step(Xd, B, 0.05, 0.9, 1)
        twin.train_step(X, 0.05, 0.9, 1)
        for n in STATE:
            bits_equal(eng.get(n), twin.p[n], 'Bernoulli handle, update %d, %s' % (s, n))
    eng.close()


def test_c_abi_refusals(gpu_lib):
    from boltzmann_machines_amd._ffi import DeviceArray
    lib = gpu_lib
    K, G, H, B = 3, 4, 8, 16
    V = G * K

    def refused(rc, what):
        assert rc != 0, what + ' was accepted'
        msg = lib.bm_last_error().decode()
        assert 'softmax visible' in msg, '%s: %s' % (what, msg)

    eng, twin = pair(K, G, H, B, 3)
    X = categories(B, G, K, 2)
    D = DeviceArray((4 * B, max(V, H)), f32)                # a device buffer for every pointer argument of a refused call
    hostf = np.zeros(4 * B * max(V, H), f32)
    hp = hostf.ctypes.data_as(C.c_void_p)
    lr3 = (C.c_float * 3)(0.01, 0.01, 0.01)
    h, d = eng._h, D.ptr
    one = (C.c_void_p * 1)(h)
    out = C.c_void_p()
    calls = [
        ('bm_rbm_ais', lambda: lib.bm_rbm_ais(h, 4, 4, 1, None, 1, 0, hp)),
        ('bm_rbm_pt_init', lambda: lib.bm_rbm_pt_init(h, B, 2, hp, None, 0)),
        ('bm_rbm_pt_sweep', lambda: lib.bm_rbm_pt_sweep(h, 1)),
        ('bm_rbm_pt_read', lambda: lib.bm_rbm_pt_read(h, d, None, None, None)),
        ('bm_rbm_train_step_pt', lambda: lib.bm_rbm_train_step_pt(h, d, B, 0.01, 0.9, 1)),
        ('bm_rbm_train_epoch_pt', lambda: lib.bm_rbm_train_epoch_pt(h, d, B, B, 0.01, 0.9, 1)),
        ('bm_rbm_set_fast_weights', lambda: lib.bm_rbm_set_fast_weights(h, 1, 0.01, 0.95)),
        ('bm_rbm_set_centering', lambda: lib.bm_rbm_set_centering(h, 1, 0.01, 0.01)),
        ('bm_rbm_set_classes', lambda: lib.bm_rbm_set_classes(h, 3)),
        ('bm_rbm_class_log_proba', lambda: lib.bm_rbm_class_log_proba(h, d, B, hp)),
        ('bm_rbm_class_train_step', lambda: lib.bm_rbm_class_train_step(h, d, d, B, 0.01, 0.9, None)),
        ('bm_rbm_class_train_epoch', lambda: lib.bm_rbm_class_train_epoch(h, d, d, B, B, 0.01, 0.9, None)),
        ('bm_rbm_class_joint_train_step', lambda: lib.bm_rbm_class_joint_train_step(h, d, d, B, 1, 0.01, 0.9, 0.0, None)),
        ('bm_rbm_class_joint_train_epoch', lambda: lib.bm_rbm_class_joint_train_epoch(h, d, d, B, B, 1, 0.01, 0.9, 0.0, None)),
        ('bm_rbm_class_joint_chain', lambda: lib.bm_rbm_class_joint_chain(h, d, d, B, 1, hp, hp, hp, hp, hp)),
        ('bm_rbm_class_unsup_train_step', lambda: lib.bm_rbm_class_unsup_train_step(h, d, B, 1, 0.01, 0.9, None)),
        ('bm_rbm_class_unsup_chain', lambda: lib.bm_rbm_class_unsup_chain(h, d, B, 1, hp, hp, hp, hp, hp, hp)),
        ('bm_rbm_class_semi_train_epoch', lambda: lib.bm_rbm_class_semi_train_epoch(h, d, d, B, d, B, 0, B, 1, 0.01, 0.9, 0.0, 1.0, None)),
        ('bm_rbm_class_gibbs', lambda: lib.bm_rbm_class_gibbs(h, d, d, B, 1, d, None)),
        ('bm_rbm_gibbs_clamped', lambda: lib.bm_rbm_gibbs_clamped(h, d, d, None, B, 1, d, d)),
        ('bm_rbm_grad_step', lambda: lib.bm_rbm_grad_step(h, d, B, 1)),
        ('bm_rbm_apply_step', lambda: lib.bm_rbm_apply_step(h, B, 0.01, 0.9)),
        ('bm_rbm_set_grad_slot', lambda: lib.bm_rbm_set_grad_slot(h, 1)),
        ('bm_rbm_xchg_create', lambda: lib.bm_rbm_xchg_create(h, 0, 1, C.byref(out))),
        ('bm_rbm_backprop_down', lambda: lib.bm_rbm_backprop_down(h, d, B, None, V, d, V)),
        ('bm_rbm_delta_update', lambda: lib.bm_rbm_delta_update(h, d, d, B, 0.01, 0.9)),
        ('bm_rbm_class_stack_train_step', lambda: lib.bm_rbm_class_stack_train_step(h, None, 0, d, d, B, lr3, 0.9, None)),
        ('bm_rbm_class_stack_train_epoch', lambda: lib.bm_rbm_class_stack_train_epoch(h, None, 0, d, d, B, B, lr3, 0.9, None)),
        ('bm_rbm_class_stack_log_proba', lambda: lib.bm_rbm_class_stack_log_proba(h, None, 0, d, B, hp)),
        ('bm_rbm_stack_transform', lambda: lib.bm_rbm_stack_transform(one, 1, d, B, d)),
    ]
    for what, f in calls:
        refused(f(), what)
        three_updates(eng, twin, X, 1, what='after the refusal of ' + what)          # the handle still trains
    eng.close()
