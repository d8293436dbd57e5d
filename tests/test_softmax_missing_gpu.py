"""Softmax visible units with incomplete rows, clamped groups and exact group conditionals on the GPU: the
clamped sweep and the training chain bit for bit against the CPU twin (tests/softmax_missing_twin.py), bm_rbm_groups_scores within
its forward-error bound of the float64 statement, CategoricalRBM(missing_values=True), and the C-ABI refusals."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import softmax_missing_twin as M
from tests import softmax_v_twin as T
from tests.test_softmax_v_gpu import GEOMETRIES, ROOT, STATE, TRAIN_SHAPES, bitmap, bits_equal, categories, engine, params, state_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
# (K, G, H, B)
FUSED = [(4, 6, 40, 37), (8, 5, 33, 20), (16, 3, 24, 9), (2, 10, 17, 33)]
GENERIC = [(3, 5, 19, 21), (5, 7, 40, 13), (26, 2, 16, 8), (2, 3, 8, 5)]             # (the last: V % 4 != 0)


def group_flags(kind, B, G, seed):
    """[B][G] clamp flags: all free, all clamped, or random per group - with a first group and a last group clamped next to free
    ones, and both free somewhere else"""
    if kind == 'zero':
        return np.zeros((B, G), bool)
    if kind == 'one':
        return np.ones((B, G), bool)
    f = np.random.RandomState(seed).uniform(size=(B, G)) < 0.5
    f[0, 0], f[0, G - 1] = True, False
    f[1, 0], f[1, G - 1] = False, True
    return f


def clamp_case(K, G, H, B, kind, seed=1):
    """parameters, start states, clamp values (a one-hot group, or an absent - all-zero - group in every third clamped place) and
    the mask"""
    p = params(G * K, H)
    V0 = categories(B, G, K, seed + 10)
    clamp = categories(B, G, K, seed + 20)
    absent = np.random.RandomState(seed + 30).uniform(size=(B, G)) < 1.0 / 3
    clamp[M.group_mask(absent, K) != 0] = 0.0
    return p, V0, clamp, M.group_mask(group_flags(kind, B, G, seed + 40), K)


def run_clamped(eng, V0, clamp, mask, n_steps, seed, row0=0, means=True):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    B = len(V0)
    Vd, Hd = as_device(V0), DeviceArray((B, eng.H), f32)
    Pd = DeviceArray((B, eng.V), f32) if means else None
    eng.seed(seed)
    eng.set_row_offset(row0)
    eng.groups_gibbs_clamped(Vd, Hd, B, n_steps, as_device(clamp), as_device(mask), Pd)
    eng.sync()
    eng.set_row_offset(0)
    return Vd.numpy(), Hd.numpy(), (Pd.numpy() if means else None)


def unclamped_sweep(p, K, V0, n_steps, seed, row0=0):
    """the sweep without any clamp, from tests/softmax_v_twin.py alone"""
    from tests.clamp_twin import SITE_H, SITE_V, act2
    v, h, vm = np.ascontiguousarray(V0, f32), None, None
    for t in range(n_steps):
        _, h = act2(v, p['W'], None, None, p['hb'], None, 1.0, 0, 1, seed, SITE_H + 16 * t, 0, row0)
        vm, v = T.visible_pass(h, p['W'], p['vb'], K, 1, seed, SITE_V + 16 * t, 0, row0)
    return v, h, vm


# ---- 1. bm_rbm_groups_gibbs_clamped
@pytest.mark.parametrize('K,G,H,B', FUSED + GENERIC)
def test_groups_gibbs_clamped(gpu_lib, K, G, H, B):
    eng = engine(params(G * K, H), B, K)
    for kind in ('zero', 'one', 'random'):
        p, V0, clamp, mask = clamp_case(K, G, H, B, kind)
        for n_steps in (1, 3):
            what = '%s mask, %d steps' % (kind, n_steps)
            gv, gh, gm = run_clamped(eng, V0, clamp, mask, n_steps, 7)
            cv, ch, cm = M.groups_gibbs_clamped(p, K, V0, clamp, mask, n_steps, 7)
            bits_equal(gv, cv, what + ': v')
            bits_equal(gh, ch, what + ': h')
            bits_equal(gm, cm, what + ': v means')
            held = mask != 0
            assert np.array_equal(gv[held], clamp[held]) and np.array_equal(gm[held], clamp[held])
            assert np.all(gv.reshape(B, G, K).sum(axis=2)[~held.reshape(B, G, K)[:, :, 0]] == 1)
            if kind == 'zero':                      # the unclamped sweep, bit for bit
                uv, uh, um = unclamped_sweep(p, K, V0, n_steps, 7)
                bits_equal(gv, uv, what + ': v against the unclamped sweep')
                bits_equal(gh, uh, what + ': h against the unclamped sweep')
                bits_equal(gm, um, what + ': v means against the unclamped sweep')
    # a slice under its row offset reproduces its rows of the whole; the means output may be null
    p, V0, clamp, mask = clamp_case(K, G, H, B, 'random')
    whole = run_clamped(eng, V0, clamp, mask, 3, 7, row0=1000)
    lo, hi = 2, min(B, 9)
    part = run_clamped(eng, V0[lo:hi], clamp[lo:hi], mask[lo:hi], 3, 7, row0=1000 + lo)
    for a, b, n in zip(part, whole, ('v', 'h', 'v means')):
        bits_equal(a, b[lo:hi], 'slice: ' + n)
    bits_equal(run_clamped(eng, V0, clamp, mask, 3, 7, row0=1000, means=False)[0], whole[0], 'without the means output')
    eng.close()


# ---- 2. the fused flavour against the generic pair, and in every geometry
def clamped_digests():
    """one digest per fused shape of what three clamped steps under the random mask return"""
    out = []
    for K, G, H, B in FUSED:
        p, V0, clamp, mask = clamp_case(K, G, H, B, 'random')
        eng = engine(p, B, K)
        gv, gh, gm = run_clamped(eng, V0, clamp, mask, 3, 7, row0=1000)
        eng.close()
        out.append(hashlib.sha1(gv.tobytes() + gh.tobytes() + gm.tobytes()).hexdigest())
    return out


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_softmax_missing_gpu as G
print('SOFTMAX_MISSING_DIGEST', ' '.join(G.%(fn)s()))
'''


def run_child(dbg, fn, tag='SOFTMAX_MISSING_DIGEST'):
    env = dict(os.environ, BM355_DEBUG=dbg)
    r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, fn=fn)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and tag in r.stdout, '%s: %s' % (dbg, r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout.split(tag, 1)[1].split()


def test_fused_generic_and_every_geometry_hold_the_twins_bits(gpu_lib):
    """the four fused shapes in fresh child processes (BM355_DEBUG is read once per process): one under sm_fused=0 - the generic
    pair with the clamp in softmax_groups_kernel - and one per forced act_geo, each under its own time limit; the first failure
    ends the test (as tests/test_softmax_v_gpu.py's geometry test)"""
    want = []
    for K, G, H, B in FUSED:
        p, V0, clamp, mask = clamp_case(K, G, H, B, 'random')
        cv, ch, cm = M.groups_gibbs_clamped(p, K, V0, clamp, mask, 3, 7, row0=1000)
        want.append(hashlib.sha1(cv.tobytes() + ch.tobytes() + cm.tobytes()).hexdigest())
    assert clamped_digests() == want
    for dbg in ('sm_fused=0',) + tuple('act_geo=' + g for g in GEOMETRIES):
        got = run_child(dbg, 'clamped_digests')
        assert got == want, '%s: shapes %r differ from the twin' % (dbg, [s_ for s_, g, w in zip(FUSED, got, want) if g != w])


# ---- 3. training on incomplete rows
def gappy(B, G, K, seed):
    """one-hot rows with 30 % of the groups empty, row 0 fully empty, row 1 complete"""
    X, _ = M.remove_groups(categories(B, G, K, seed), K, 0.3, seed + 1, keep_rows=(1,))
    X[0] = 0.0
    return X


def missing_pair(K, G, H, B, seed, **kw):
    p = params(G * K, H, w_std=0.05)
    eng = engine(p, B, K, **kw)
    eng.groups_set_missing(True)
    eng.seed(seed)
    return eng, M.MissingRBM(p, K, seed, **kw)


@pytest.mark.parametrize('sample_v', [False, True])
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('K,G,H,B', TRAIN_SHAPES)
def test_train_step_with_missing_groups(gpu_lib, K, G, H, B, k, sample_v):
    """three updates with the mode on: every parameter and accumulator is the twin's, whose chain holds the empty groups at exact
    zeros (asserted on the twin's vs and vm here; test_empty_groups_stay_zero_on_the_device reads the device's); on complete
    rows the mode changes no bit"""
    from boltzmann_machines_amd.engine import as_device
    X = gappy(B, G, K, 5)
    eng, twin = missing_pair(K, G, H, B, 3, sample_v_states=sample_v, l2=1e-3)
    Xd = as_device(X)
    gone = M.missing_mask(X, K) != 0
    assert gone[0].all() and not gone[1].any() and 0.2 < gone.mean() < 0.45
    for s in range(3):
        eng.train_step(Xd, B, 0.05, 0.9, k)
        ch = twin.train_step(X, 0.05, 0.9, k)
        assert np.all(ch['vs'][gone] == 0) and np.all(ch['vm'][gone] == 0)
        state_equal(eng, twin, 'update %d' % s)
    eng.close()
    Xc = categories(B, G, K, 6)
    on, _ = missing_pair(K, G, H, B, 3, sample_v_states=sample_v, l2=1e-3)
    off = engine(params(G * K, H, w_std=0.05), B, K, sample_v_states=sample_v, l2=1e-3)
    off.seed(3)
    Xd = as_device(Xc)
    for s in range(3):
        on.train_step(Xd, B, 0.05, 0.9, k)
        off.train_step(Xd, B, 0.05, 0.9, k)
    for n in STATE:
        bits_equal(on.get(n), off.get(n), 'complete rows, mode on against mode off: ' + n)
    mo, mf = on.metrics(Xd, B, k), off.metrics(Xd, B, k)
    assert np.array_equal(mo[[0, 2, 3]].view(np.uint32), mf[[0, 2, 3]].view(np.uint32)) and np.isnan(mo[1]) and np.isnan(mf[1])
    on.close(); off.close()


@pytest.mark.parametrize('K,G,H,B', [(4, 33, 24, 37), (5, 13, 24, 37)])
def test_empty_groups_stay_zero_on_the_device(gpu_lib, K, G, H, B):
    """the last group empty in EVERY row: after one update from zero accumulators with momentum 0, dvb = lr sum_b (x - v_k) / B of
    its units is exactly 0 only if every v_k state there is exactly 0 (states are >= 0); the clamped sweep shows the same of
    states and means directly"""
    from boltzmann_machines_amd.engine import as_device
    X = gappy(B, G, K, 7)
    X[:, (G - 1) * K:] = 0.0
    for sample_v in (False, True):
        eng, twin = missing_pair(K, G, H, B, 3, sample_v_states=sample_v)
        eng.train_step(as_device(X), B, 0.05, 0.0, 2)
        twin.train_step(X, 0.05, 0.0, 2)
        state_equal(eng, twin, 'one update')
        dvb = eng.get('dvb')
        assert np.all(dvb[(G - 1) * K:] == 0) and np.any(dvb[:(G - 1) * K] != 0)
        gv, _, gm = run_clamped(eng, X, X, M.missing_mask(X, K), 2, 9)
        gone = M.missing_mask(X, K) != 0
        assert np.all(gv[gone] == 0) and np.all(gm[gone] == 0) and np.all(gv.reshape(B, G, K).sum(axis=2)[~gone[:, ::K]] == 1)
        eng.close()


def test_train_epoch_and_metrics_with_missing_groups(gpu_lib):
    from boltzmann_machines_amd.engine import as_device
    for K, G, H, B in [(4, 33, 24, 37), (5, 13, 24, 37)]:
        N = 2 * B + 7
        X = gappy(N, G, K, 8)
        eng, twin = missing_pair(K, G, H, B, 5, sample_v_states=True)
        Xd = as_device(X)
        eng.train_epoch(Xd, N, B, 0.05, 0.9, 1)
        twin.train_epoch(X, B, 0.05, 0.9, 1)
        state_equal(eng, twin, 'epoch')
        out = eng.metrics(Xd, B, 2)
        msre, l2, fe = twin.metrics(X[:B], 2)
        np.testing.assert_allclose([out[0], out[2], out[3]], [msre, l2, fe], rtol=1e-5)
        assert np.isnan(out[1])
        out = eng.train_step_metrics(Xd, B, 0.05, 0.9, 1)
        assert np.isnan(out[1]) and np.all(np.isfinite(out[[0, 2, 3]]))
        twin.train_step(X[:B], 0.05, 0.9, 1)
        state_equal(eng, twin, 'train_step_metrics')
        eng.train_step_metrics_async(Xd, B, 0.05, 0.9, 1)
        twin.train_step(X[:B], 0.05, 0.9, 1)
        assert eng.collect_metrics().shape == (1, 4)
        state_equal(eng, twin, 'train_step_metrics_async')
        # transform does not look at the mode: the plain twin's chain from the same rows
        from boltzmann_machines_amd._ffi import DeviceArray
        Hd = DeviceArray((B, H), f32)
        eng.transform(Xd, B, 2, Hd)
        plain = T.SoftmaxVRBM(twin.state(), K, 5, sample_v_states=True)
        plain.call = twin.call
        bits_equal(Hd.numpy(), plain.transform(X[:B], 2), 'transform')
        eng.close()


# ---- 4. refusals on a handle without groups
def test_refused_without_groups(gpu_lib):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    from oracle import oracle as orc
    lib = gpu_lib
    V, H, B = 12, 8, 16
    p = params(V, H, w_std=0.05)
    X = categories(B, 4, 3, 2)
    eng = engine(p, B, 0)
    eng.seed(3)
    twin = orc.OracleRBM(V, H, l2=1e-4)
    for n in ('W', 'vb', 'hb'):
        twin.p[n][...] = p[n]
    twin.set_seed(3)
    D = DeviceArray((4 * B, max(V, H)), f32)
    host = np.zeros((B, V), np.float64)
    h, d = eng._h, D.ptr
    Xd = as_device(X)
    for what, f in (('bm_rbm_groups_set_missing', lambda: lib.bm_rbm_groups_set_missing(h, 1)),
                    ('bm_rbm_groups_gibbs_clamped', lambda: lib.bm_rbm_groups_gibbs_clamped(h, d, d, None, B, 1, d, d)),
                    ('bm_rbm_groups_scores', lambda: lib.bm_rbm_groups_scores(h, d, B, host.ctypes.data_as(C.c_void_p)))):
        assert f() != 0, what + ' was accepted'
        msg = lib.bm_last_error().decode()
        assert 'visible groups' in msg and what in msg, '%s: %s' % (what, msg)
        eng.train_step(Xd, B, 0.05, 0.9, 1)                          # the handle still trains: the Bernoulli handle it was
        twin.train_step(X, 0.05, 0.9, 1)
        for n in STATE:
            bits_equal(eng.get(n), twin.p[n], 'after the refusal of %s: %s' % (what, n))
    eng.close()
    # set_visible_groups(0) takes the mode off with the groups
    eng = engine(p, B, 3)
    eng.groups_set_missing(True)
    eng.set_visible_groups(0)
    assert lib.bm_rbm_groups_set_missing(eng._h, 0) != 0
    eng.close()


# ---- 5. bm_rbm_groups_scores against group_scores64
def score_rows(B, G, K, seed):
    """rows with empty groups, complete rows and (B >= 2) one fully empty row"""
    X, _ = M.remove_groups(categories(B, G, K, seed), K, 0.3, seed + 1, keep_rows=(1, 3))
    if B >= 2:
        X[0] = 0.0
    return X


def check_scores(p, K, B, max_batch, X, cap, what):
    from boltzmann_machines_amd.engine import as_device
    eng = engine(p, max_batch, K)
    call0 = eng.get('W').copy()
    S = eng.groups_scores(as_device(X), B)
    bits_equal(eng.get('W'), call0, what + ': W')
    eng.close()
    S64, bound = M.group_scores64(p, X, K)
    ratio = float((np.abs(S - S64) / bound).max())
    print('%s: worst |S_dev - S_64| / bound = %.4f, largest bound %.3e' % (what, ratio, bound.max()))
    assert np.all(np.isfinite(S)) and bound.max() < cap
    assert np.all(np.abs(S - S64) <= 2 * bound), what
    return S, ratio


SCORE_SHAPES = FUSED + GENERIC + [(16, 3, 130, 9), (4, 6, 1, 37)]


@pytest.mark.parametrize('K,G,H,B', SCORE_SHAPES)
def test_groups_scores(gpu_lib, K, G, H, B):
    check_scores(params(G * K, H), K, B, B, score_rows(B, G, K, 4), 5e-4, 'K=%d G=%d H=%d B=%d' % (K, G, H, B))


@pytest.mark.parametrize('B', [1, 65, 130])
def test_groups_scores_slices_past_max_batch(gpu_lib, B):
    """max_batch = 64: B = 65 and 130 cross a wave's 64 rows and the internal slicing"""
    K, G, H = 4, 6, 40
    check_scores(params(G * K, H), K, B, 64, score_rows(B, G, K, 4), 5e-4, 'B=%d' % B)


def test_groups_scores_wide_weights(gpu_lib):
    K, G, H, B = 4, 6, 40, 37
    check_scores(params(G * K, H, w_std=3.0), K, B, B, score_rows(B, G, K, 4), 5e-4, 'weights of std 3')


def test_groups_scores_both_linear_regimes(gpu_lib):
    """hb = +-40: softplus(x) = x on one half of the hidden units and e^x on the other.  The cap on the bound, from the bound's own
    terms with |hb_j| = 40 and |w| <= wmax: A_j <= 40 + G wmax, |a_j| and |a_j + w| <= 40 + (G + 1) wmax, softplus <= the same:
    H u ((G + 1)(40 + G wmax) + 10 (40 + (G + 1) wmax))"""
    K, G, H, B = 4, 6, 40, 37
    p = params(G * K, H)
    p['hb'] = np.where(np.arange(H) % 2 == 0, 40.0, -40.0).astype(f32)
    wmax = float(np.abs(p['W']).max())
    cap = H * M.U * ((G + 1) * (40 + G * wmax) + 10 * (40 + (G + 1) * wmax))
    check_scores(p, K, B, B, score_rows(B, G, K, 4), cap, 'hb = +-40')


def score_digests():
    from boltzmann_machines_amd.engine import as_device
    out = []
    for K, G, H, B in (FUSED[0], GENERIC[1]):
        eng = engine(params(G * K, H), B, K)
        out.append(hashlib.sha1(eng.groups_scores(as_device(score_rows(B, G, K, 4)), B).tobytes()).hexdigest())
        eng.close()
    return out


def test_groups_scores_do_not_depend_on_debug_switches(gpu_lib):
    """a fresh child process under a forced geometry (and the generic softmax path) returns this process's bits"""
    want = score_digests()
    assert run_child('act_geo=3,sm_fused=0', 'score_digests') == want


# ---- 6. the public class
CLASS_CASES = [dict(G=4, K=4, H=8), dict(G=4, K=3, H=8)]
FIT = dict(n_train=200, batch=20, lr=0.1, mom=0.5, epochs=2, frac=0.3)


def class_data(c):
    X, _ = M.remove_groups(T.one_hot(T.planted_data(FIT['n_train'], 1, c['G'], c['K']), c['K']), c['K'], FIT['frac'], 21)
    rng = np.random.RandomState(3)
    V = c['G'] * c['K']
    return X, dict(W=(0.1 * rng.randn(V, c['H'])).astype(f32), vb=np.zeros(V, f32), hb=np.zeros(c['H'], f32))


def near_ties(lp, margin):
    """[B][G] bool: the two best log-probabilities of the cell differ by less than its margin"""
    top = np.sort(lp, axis=2)
    return (top[:, :, -1] - top[:, :, -2]) < margin


@pytest.mark.parametrize('c', CLASS_CASES, ids=['fused', 'generic'])
def test_categorical_rbm_with_missing_values(gpu_lib, tmp_path, c):
    import boltzmann_machines_amd as bm
    from boltzmann_machines_amd.utils import RNG
    G, K, H = c['G'], c['K'], c['H']
    X, p0 = class_data(c)
    seed = RNG(seed=1337).randint(2 ** 31 - 1)                              # the graph seed fit() draws
    twin = M.MissingRBM(p0, K, seed=seed, l2=1e-4)
    for _ in range(FIT['epochs']):
        twin.train_epoch(X, FIT['batch'], FIT['lr'], FIT['mom'], 1)
    path = str(tmp_path) + '/a/'
    m = bm.CategoricalRBM(n_groups=G, n_categories=K, n_hidden=H, missing_values=True, W_init=p0['W'], vb_init=p0['vb'],
                          hb_init=p0['hb'], batch_size=FIT['batch'], learning_rate=FIT['lr'], momentum=FIT['mom'], l2=1e-4,
                          max_epoch=FIT['epochs'], random_seed=1337, verbose=False, save_after_each_epoch=False, v_shape=(G, K),
                          model_path=path)
    assert np.array_equal(m.encode(m.decode(X, missing=-1), missing=-1), X)
    m.fit(X)
    w, acc = m.get_tf_params(scope='weights'), m.get_tf_params(scope='grads_accumulators')
    for n in ('W', 'vb', 'hb'):
        bits_equal(w[n], twin.p[n], 'fit ' + n)
    for n in ('dW', 'dvb', 'dhb'):
        bits_equal(acc[n], twin.p[n], 'fit ' + n)
    # group_log_proba: log-sum-exp is 1-Lipschitz in the largest deviation of a group's scores, so a log-probability moves by at
    # most the deviation of its own score plus the largest of its group: 2 max_k (2 bound)
    p = twin.state()
    Xt, gone = M.remove_groups(T.one_hot(T.planted_data(100, 2, G, K), K), K, 0.3, 22)
    Xt[0] = 0.0
    lp = m.group_log_proba(Xt)
    S64, bound = M.group_scores64(p, Xt, K)
    lp64 = M.log_softmax_groups(S64, K)
    margin = 2 * (2 * bound).reshape(len(Xt), G, K).max(axis=2)
    assert lp.shape == (len(Xt), G, K) and lp.dtype == np.float64
    assert np.all(np.abs(lp - lp64) <= margin[:, :, None])
    np.testing.assert_allclose(m.predict_proba(Xt).sum(axis=2), 1.0, atol=1e-12)
    # predict: the twin's, except where the twin's own two best differ by less than the margin - at most 1 % of the cells
    ties = near_ties(lp64, 2 * margin)
    print('%d of %d cells are near-ties of the twin' % (ties.sum(), ties.size))
    assert ties.mean() <= 0.01
    pred, pred64 = m.predict(Xt), M.predict64(p, Xt, K)
    assert pred.dtype == np.int64 and np.array_equal(pred[~ties], pred64[~ties])
    obs = M.observed_groups(Xt, K)
    assert np.array_equal(pred[obs], Xt.reshape(len(Xt), G, K).argmax(axis=2)[obs])
    pll = m.pseudo_log_likelihood(Xt)
    np.testing.assert_allclose(pll, (lp * Xt.reshape(len(Xt), G, K)).sum(axis=(1, 2)), rtol=0, atol=1e-12)
    assert pll.shape == (len(Xt),) and pll[0] == 0.0 and np.all(pll[obs.any(axis=1)] < 0)
    # load_model restores the keyword; sample_groups_given keeps the observed groups, returns one-hot rows and does not depend on
    # the slicing
    a, b = bm.CategoricalRBM.load_model(path).set_params(batch_size=16), bm.CategoricalRBM.load_model(path).set_params(batch_size=37)
    assert a.missing_values is True
    bits_equal(a.get_tf_params(scope='weights')['W'], twin.p['W'], 'load_model W')
    va, ma = a.sample_groups_given(Xt, n_gibbs_steps=5, return_means=True)
    vb_ = b.sample_groups_given(Xt, n_gibbs_steps=5)
    bits_equal(va, vb_, 'sample_groups_given over batch sizes')
    held = np.repeat(obs, K, axis=1)
    assert np.array_equal(va[held], Xt[held]) and np.array_equal(ma[held], Xt[held])
    assert np.all((va == 0) | (va == 1)) and np.all(va.reshape(len(Xt), G, K).sum(axis=2) == 1)
    with pytest.raises(ValueError):
        a.sample_groups_given(np.ones_like(Xt))
    with pytest.raises(ValueError) as e:
        a.sample_v_given(Xt, np.ones(G * K))
    assert 'softmax visible units' in str(e.value)
