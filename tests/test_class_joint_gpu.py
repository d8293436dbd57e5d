"""-m gpu: joint training of the classification RBM and sampling by class - act_kernel's class-bias flavour,
class_draw / class_joint_update kernels, bm_rbm_class_joint_* / bm_rbm_class_gibbs, BernoulliRBM.fit_joint / sample_v_given_class.

Bit-exact comparisons (view(uint32)) are against the CPU twin (tests/class_joint_twin.py); the hybrid update's tolerances are
FACTOR = 10 x the float32 twin's own deviation from a float64 restatement on the same chain states, never anything the engine
produced."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import class_joint_cases as K
from tests import class_joint_twin as T
from tests import np_reference_class as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = K.NAMES
GEOMETRIES = ('8', '4', '1', '3', '108', '104', '101', '103', '208', '6', '5', '7', '9')      # what launch_act_as accepts


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev(a, dt=np.float32):
    from boltzmann_machines_amd._ffi import DeviceArray
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dt), dt)


def engine(V, H, C, B, p0, seed=K.SEED, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    eng = RbmEngine(V, H, max_batch=B, l2=K.L2, **kw)
    eng.set_classes(C)
    for n in NAMES:
        if n in p0:
            eng.set(n, p0[n])
    eng.seed(seed)
    return eng


def state(eng, names=NAMES):
    return {n: eng.get(n) for n in names}


def assert_same(got, want, what, names=None):
    for k in (names or want):
        assert np.array_equal(bits(got[k]), bits(want[k])), '%s: %s differs in %d of %d entries (max abs %.3g)' % (
            what, k, int(np.sum(bits(got[k]) != bits(want[k]))), want[k].size, float(np.abs(got[k] - want[k]).max()))


def chain_digest_lines():
    """one line per shape: the chain of the case's first batch (k = 2) as the engine runs it - h0 means and states, v_k, y_k, h_k"""
    import hashlib
    out = []
    for shape in K.SHAPES:
        V, H, C, B = shape
        c = K.inputs(*shape)
        eng = engine(V, H, C, B, c['p0'])
        ch = eng.class_joint_chain(dev(c['X']), dev(c['y'], np.int32), B, 2)
        eng.close()
        h = hashlib.sha256()
        for n in ('h0m', 'h0s', 'vk', 'yk', 'hk'):
            h.update(np.ascontiguousarray(ch[n]).tobytes())
        out.append(h.hexdigest())
    return out


def twin_chain_digest_lines():
    import hashlib
    out = []
    for shape in K.SHAPES:
        V, H, C, B = shape
        c = K.inputs(*shape)
        p = c['p0']
        h0m, h0s = T.cb_pass(p, c['X'][:B], c['y'][:B], 1, K.SEED, T.SITE_H0, 0)
        ch = T.chain(p, c['X'][:B], c['y'][:B], 2, K.SEED, 0)
        h = hashlib.sha256()
        for a in (h0m, h0s, ch['vk'], ch['yk'].astype(np.int32), ch['hk']):
            h.update(np.ascontiguousarray(a).tobytes())
        out.append(h.hexdigest())
    return out


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_class_joint_gpu as G
print('JOINT_DIGEST', ' '.join(G.chain_digest_lines()))
'''


# ---- 1. the CB pass alone
@pytest.mark.parametrize('shape', K.SHAPES)
def test_cb_pass_is_the_twins(gpu_lib, shape):
    """h0 means and states of the chain entry: the twin's, bit for bit; with a zero U the plain pass's"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    Xd, yd = dev(c['X']), dev(c['y'], np.int32)
    for name, p in (('the case', c['p0']), ('zero U', dict(c['p0'], U=np.zeros((C, H), np.float32)))):
        eng = engine(V, H, C, B, p)
        ch = eng.class_joint_chain(Xd, yd, B, 1)
        eng.close()
        m, s = T.cb_pass(p, c['X'][:B], c['y'][:B], 1, K.SEED, T.SITE_H0, 0)
        assert_same(ch, dict(h0m=m, h0s=s), 'CB pass, %s, shape %r' % (name, shape))
        if name == 'zero U':
            mp, sp = T.act2(c['X'][:B], p['W'], None, None, p['hb'], None, 1.0, 0, 1, K.SEED, T.SITE_H0, 0, 0)
            assert_same(ch, dict(h0m=mp, h0s=sp), 'CB pass with zero U against the plain pass, shape %r' % (shape,))


def test_cb_pass_with_zero_head_is_the_engines_plain_pass(gpu_lib):
    """the same engine, the same seed: class_gibbs with a zero U from V0 gives the visible states and means of the plain clamped
    sweep with an all-zero mask (every visible mean depends on every hidden state: the hidden draws are the same bits)"""
    from boltzmann_machines_amd._ffi import DeviceArray
    for shape in K.SHAPES:
        V, H, C, B = shape
        c = K.inputs(*shape)
        eng = engine(V, H, C, B, dict(c['p0'], U=np.zeros((C, H), np.float32)))
        out_v, out_m = DeviceArray((B, V), np.float32), DeviceArray((B, V), np.float32)
        eng.class_gibbs(dev(c['X'][:B]), dev(c['y'][:B], np.int32), B, 2, out_v, out_m)
        eng.sync()
        eng.seed(K.SEED)
        Vd, Hd, Pd = dev(c['X'][:B]), DeviceArray((B, H), np.float32), DeviceArray((B, V), np.float32)
        eng.gibbs_clamped(Vd, Hd, B, 2, dev(np.zeros((B, V))), dev(np.zeros((B, V))), Pd)
        eng.sync()
        assert_same(dict(v=out_v.numpy(), m=out_m.numpy()), dict(v=Vd.numpy(), m=Pd.numpy()), 'zero U against the plain sweep, shape %r' % (shape,))
        eng.close()


def test_every_geometry_holds_the_twins_bits(gpu_lib):
    """one fresh child per act_kernel geometry (BM355_DEBUG is read once per process), each under its own time limit; the first
    failure ends the test"""
    want = twin_chain_digest_lines()
    assert chain_digest_lines() == want
    for geo in GEOMETRIES:
        env = dict(os.environ, BM355_DEBUG='act_geo=' + geo)
        r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'JOINT_DIGEST' in r.stdout, 'act_geo=%s: %s' % (geo, r.stdout[-2000:] + r.stderr[-4000:])
        got = r.stdout.split('JOINT_DIGEST', 1)[1].split()
        assert got == want, 'act_geo=%s: shapes %r differ from the twin' % (geo, [s for s, g, w in zip(K.SHAPES, got, want) if g != w])


# ---- 2. the class draw, 3. the chain
@pytest.mark.parametrize('shape', K.SHAPES)
@pytest.mark.parametrize('k', [1, 3])
def test_chain_is_the_twins(gpu_lib, shape, k):
    """v_k, y_k, h_k means - and with them every class draw on the way, from hidden STATES - bit-identical to the twin"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    eng = engine(V, H, C, B, c['p0'])
    ch = eng.class_joint_chain(dev(c['X']), dev(c['y'], np.int32), B, k)
    eng.close()
    tw = T.chain(c['p0'], c['X'][:B], c['y'][:B], k, K.SEED, 0)
    assert np.array_equal(ch['yk'], tw['yk']), (ch['yk'], tw['yk'])
    assert len(set(tw['yk'])) > 1
    assert_same(ch, tw, 'chain k = %d, shape %r' % (k, shape), names=('h0m', 'vk', 'hk'))


@pytest.mark.parametrize('shape', K.SHAPES)
def test_class_draw_from_means(gpu_lib, shape):
    """sample_h_states = False: the chain feeds hidden MEANS downward, the class draw reads them"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    eng = engine(V, H, C, B, c['p0'], sample_h_states=False)
    ch = eng.class_joint_chain(dev(c['X']), dev(c['y'], np.int32), B, 2)
    eng.close()
    tw = T.chain(c['p0'], c['X'][:B], c['y'][:B], 2, K.SEED, 0, sample_h=False)
    assert np.array_equal(ch['yk'], tw['yk']), (ch['yk'], tw['yk'])
    assert_same(ch, tw, 'chain on means, shape %r' % (shape,), names=('h0m', 'vk', 'hk'))


# ---- 4. gamma = 0
def run_updates(shape, k=1, gamma=0.0, updates=K.UPDATES, fetch=False):
    V, H, C, B = shape
    c = K.inputs(*shape)
    eng = engine(V, H, C, B, c['p0'])
    Xd, yd = dev(c['X']), dev(c['y'], np.int32)
    states, out2 = [], []
    for u in range(updates):
        out2.append(eng.class_joint_train_step(Xd, yd, B, k, K.LR, K.MOM, gamma, row=u * B, fetch=fetch))
        states.append(state(eng))
    eng.close()
    return states, out2


@pytest.mark.parametrize('shape', K.SHAPES)
def test_generative_updates_are_the_twins(gpu_lib, shape):
    tw = K.trajectory(*shape, k=1)
    a, _ = run_updates(shape)
    for u in range(K.UPDATES):
        assert_same(a[u], tw['states'][u], 'gamma = 0, shape %r, update %d' % (shape, u))
    b, _ = run_updates(shape)
    for u in range(K.UPDATES):
        assert_same(b[u], a[u], 'two runs, shape %r, update %d' % (shape, u))


@pytest.mark.parametrize('shape', K.SHAPES[:2])
def test_epoch_is_the_loop_over_steps(gpu_lib, shape):
    V, H, C, B = shape
    c = K.inputs(*shape)
    N = 2 * B + max(1, B // 3)
    Xd, yd = dev(c['X'][:N]), dev(c['y'][:N], np.int32)
    a, b, a2 = (engine(V, H, C, B, c['p0']) for _ in range(3))
    lp, acc = a.class_joint_train_epoch(Xd, yd, N, B, 1, K.LR, K.MOM, 0.0)
    slp = sacc = 0.0
    for s in range(0, N, B):
        n = min(B, N - s)
        l, h = b.class_joint_train_step(Xd, yd, n, 1, K.LR, K.MOM, 0.0, row=s)
        slp, sacc = slp + l * n, sacc + h * n
    assert_same(state(a), state(b), 'epoch against steps, shape %r' % (shape,))
    assert abs(lp - slp / N) <= 1e-6 * abs(slp / N) and abs(acc - sacc / N) <= 1e-6
    assert a2.class_joint_train_epoch(Xd, yd, N, B, 1, K.LR, K.MOM, 0.0, fetch=False) is None
    assert_same(state(a2), state(a), 'epoch without the fetch')
    for e in (a, b, a2):
        e.close()


@pytest.mark.parametrize('shape', K.SHAPES)
def test_zero_head_first_update_is_the_plain_update(gpu_lib, shape):
    """U = 0: the first joint update moves W, hb, vb exactly as bm_rbm_train_step does from the same seed (U itself learns, so only
    the first update compares)"""
    from boltzmann_machines_amd.engine import RbmEngine
    V, H, C, B = shape
    c = K.inputs(*shape)
    names = ('W', 'hb', 'vb', 'dW', 'dhb', 'dvb', 'q_means')
    eng = engine(V, H, C, B, dict(c['p0'], U=np.zeros((C, H), np.float32)))
    plain = RbmEngine(V, H, max_batch=B, l2=K.L2)
    for n in ('W', 'hb', 'vb'):
        plain.set(n, c['p0'][n])
    plain.seed(K.SEED)
    Xd = dev(c['X'])
    eng.class_joint_train_step(Xd, dev(c['y'], np.int32), B, 1, K.LR, K.MOM, 0.0, fetch=False)
    plain.train_step(Xd, B, K.LR, K.MOM, 1)
    assert_same(state(eng, names), state(plain, names), 'zero head against bm_rbm_train_step, shape %r' % (shape,))
    eng.close()
    plain.close()


# ---- 5. the hybrid update
@pytest.mark.parametrize('shape', K.SHAPES)
def test_hybrid_update_against_float64(gpu_lib, shape):
    """gamma = 0.5, one update from the common start: the chain is still the twin's bit for bit (the discriminative launches
    run BEFORE it and touch none of its inputs), and every parameter is within FACTOR x the float32 twin's deviation from the
    float64 restatement evaluated on those chain states.

    Figures (MI355X): profiles/class_joint_parity.md"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    p0, X, y = c['p0'], c['X'][:B], c['y'][:B]
    tw = K.trajectory(*shape, k=1, gamma=K.GAMMA, updates=1)
    ch = tw['chains'][0]
    eng = engine(V, H, C, B, p0)
    got_chain = eng.class_joint_chain(dev(X), dev(y, np.int32), B, 1)
    eng.close()
    assert np.array_equal(got_chain['yk'], ch['yk'])
    assert_same(got_chain, ch, 'hybrid: chain states, shape %r' % (shape,), names=('h0m', 'vk', 'hk'))
    states, _ = run_updates(shape, gamma=K.GAMMA, updates=1)
    ref = float64_update(p0, X, y, ch, K.GAMMA)
    for n in NAMES:
        twin_dev = R.max_dev(tw['states'][0][n], ref[n])
        err = R.max_dev(states[0][n], ref[n])
        print('hybrid %r, %-3s: twin deviation %.3g, engine deviation %.3g, tolerance %.3g' % (shape, n, twin_dev, err, K.FACTOR * twin_dev))
        assert err <= K.FACTOR * twin_dev, (n, err, K.FACTOR * twin_dev)


def float64_update(p0, X, y, ch, gamma):
    """the update of L_gen + gamma L_disc in float64 on given chain states (h0m, vk, yk, hk)"""
    p = R.cast(p0, np.float64)
    B, C = len(X), p['U'].shape[0]
    gd, _ = R.gradients(p, X, y, np.float64)
    X64, h0, vk, hk = (np.asarray(a, np.float64) for a in (X, ch['h0m'], ch['vk'], ch['hk']))
    Y, Yk = np.eye(C)[y], np.eye(C)[ch['yk']]
    g = dict(W=(X64.T.dot(h0) - vk.T.dot(hk)) / B + gamma * gd['W'], hb=(h0 - hk).mean(axis=0) + gamma * gd['hb'], vb=(X64 - vk).mean(axis=0),
             U=(Y.T.dot(h0) - Yk.T.dot(hk)) / B + gamma * gd['U'], yb=(Y - Yk).mean(axis=0) + gamma * gd['yb'])
    lr, mom, l2 = (np.float64(np.float32(v)) for v in (K.LR, K.MOM, K.L2))
    for w in ('W', 'U'):
        p['d' + w] = lr * (mom * p['d' + w] + (g[w] - l2 * p[w]))
        p[w] = p[w] + p['d' + w]
    for b in ('hb', 'vb', 'yb'):
        p['d' + b] = lr * (mom * p['d' + b] + g[b])
        p[b] = p[b] + p['d' + b]
    return p


# ---- 6. call counter, out2, bad labels
def test_call_counter_and_out2(gpu_lib):
    shape = K.SHAPES[0]
    V, H, C, B = shape
    c = K.inputs(*shape)
    Xd, yd = dev(c['X']), dev(c['y'], np.int32)
    # the second update of a run draws at call 1: it is the first update of an engine whose counter was advanced by one other call
    a, b = engine(V, H, C, B, c['p0']), engine(V, H, C, B, c['p0'])
    a.class_joint_train_step(Xd, yd, B, 1, 0.0, 0.0, 0.0, fetch=False)              # lr = 0: nothing moves, the counter does
    b.class_joint_chain(Xd, yd, B, 1)
    for e in (a, b):
        e.class_joint_train_step(Xd, yd, B, 1, K.LR, K.MOM, 0.0, fetch=False)
    assert_same(state(a), state(b), 'call counter: one per update')
    tw = T.JointRBM(c['p0'], K.SEED, K.L2)
    tw.call = tw.rbm.call = 1
    tw.train_step(c['X'][:B], c['y'][:B], 1, K.LR, K.MOM)
    assert_same(state(a), tw.state(), 'the update at call 1 against the twin')
    # out2: the forward pass before the update, class_train_step's on the same parameters
    d, e = engine(V, H, C, B, c['p0']), engine(V, H, C, B, c['p0'])
    for gamma in (0.0, K.GAMMA):
        for n in NAMES:
            d.set(n, c['p0'][n])
            e.set(n, c['p0'][n])
        assert d.class_joint_train_step(Xd, yd, B, 1, K.LR, K.MOM, gamma) == e.class_train_step(Xd, yd, B, K.LR, K.MOM)
    for x in (a, b, d, e):
        x.close()


def test_bad_label_raises_once_and_leaves_its_row_out(gpu_lib):
    from boltzmann_machines_amd import _ffi
    shape = K.SHAPES[0]
    V, H, C, B = shape
    c = K.inputs(*shape)
    X, y = c['X'][:B], c['y'][:B].copy()
    row = C + 2
    results = []
    for label in (C, -1, 2 ** 30):
        yb = y.copy()
        yb[row] = label
        eng = engine(V, H, C, B, c['p0'])
        eng.class_joint_train_step(dev(X), dev(yb, np.int32), B, 1, K.LR, K.MOM, 0.0, fetch=False)
        with pytest.raises(_ffi.Bm355Error, match='label outside'):
            eng.sync()
        eng.sync()                                       # reported once, then cleared
        results.append(state(eng))
        eng.close()
    for other in results[1:]:
        assert_same(other, results[0], 'another bad value in the same row')
    yb = y.copy()
    yb[row] = C
    tw = T.JointRBM(c['p0'], K.SEED, K.L2)               # the twin: plain bias in the row's prop-up, the row out of the U / yb sums
    tw.train_step(X, yb, 1, K.LR, K.MOM)
    assert_same(results[0], tw.state(), 'bad label against the twin')
    eng = engine(V, H, C, B, c['p0'])
    with pytest.raises(_ffi.Bm355Error, match='label outside'):
        eng.class_joint_train_step(dev(X), dev(yb, np.int32), B, 1, K.LR, K.MOM, 0.0)
    lp, acc = eng.class_joint_train_step(dev(X), dev(y, np.int32), B, 1, K.LR, K.MOM, 0.0)
    assert np.isfinite(lp) and 0 <= acc <= 1
    eng.close()


def test_engine_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd._ffi import DeviceArray
    V, H, B = 12, 8, 4
    Xd, yd, out = dev(np.zeros((2 * B, V))), dev(np.zeros(2 * B), np.int32), DeviceArray((2 * B, V), np.float32)
    eng = RbmEngine(V, H, max_batch=B)
    with pytest.raises(_ffi.Bm355Error, match='no class head'):
        eng.class_joint_train_step(Xd, yd, B, 1, 0.1, 0.5)
    with pytest.raises(_ffi.Bm355Error, match='no class head'):
        eng.class_gibbs(None, yd, B, 1, out)
    eng.set_classes(3)
    with pytest.raises(_ffi.Bm355Error, match='max_batch'):
        eng.class_joint_train_step(Xd, yd, 2 * B, 1, 0.1, 0.5)
    with pytest.raises(_ffi.Bm355Error, match='n_gibbs_steps'):
        eng.class_joint_train_step(Xd, yd, B, 0, 0.1, 0.5)
    with pytest.raises(_ffi.Bm355Error, match='disc_weight'):
        eng.class_joint_train_epoch(Xd, yd, 2 * B, B, 1, 0.1, 0.5, -1.0)
    with pytest.raises(_ffi.Bm355Error, match='n_steps'):
        eng.class_gibbs(None, yd, B, 0, out)
    eng.set_centering(True)
    with pytest.raises(_ffi.Bm355Error, match='centr|centering'):
        eng.class_joint_train_step(Xd, yd, B, 1, 0.1, 0.5)
    eng.close()
    for kw, match in ((dict(dropout=0.8), 'dropout'), (dict(sparsity_cost=0.1), 'sparsity')):
        e = RbmEngine(V, H, max_batch=B, **kw)
        e.set_classes(3)
        with pytest.raises(_ffi.Bm355Error, match=match):
            e.class_joint_train_step(Xd, yd, B, 1, 0.1, 0.5)
        e.close()


# ---- 7. sampling by class
def small(tmp_path, batch_size):
    from boltzmann_machines_amd import BernoulliRBM
    S, m = K.SMALL, K.small_model()
    model = BernoulliRBM(n_visible=S['V'], n_hidden=S['H'], W_init=m['p']['W'], vb_init=m['p']['vb'], hb_init=m['p']['hb'], batch_size=batch_size,
                         random_seed=S['seed'], verbose=False, model_path=str(tmp_path) + '/b%d/' % batch_size)
    model.set_classes(S['C'], U=m['p']['U'], yb=m['p']['yb'])
    return model.init()


def test_sample_v_given_class_matches_enumeration(gpu_lib, tmp_path):
    S, m = K.SMALL, K.small_model()
    y = np.repeat(np.arange(S['C']), S['chains']).astype(np.int32)
    big = small(tmp_path, 4096)
    v, vm = big.sample_v_given_class(y, n_gibbs_steps=S['steps'], return_means=True)
    assert v.shape == (len(y), S['V']) and set(np.unique(v)) <= {0.0, 1.0} and vm.min() > 0 and vm.max() < 1
    for c in range(S['C']):
        est, ex = v[y == c].mean(axis=0), m['exact'][c]
        se = np.sqrt(ex * (1 - ex) / S['chains'])
        print('class %d: exact %s, estimate %s, 5 standard errors %s' % (c, np.round(ex, 4), np.round(est, 4), np.round(5 * se, 4)))
        assert np.all(np.abs(est - ex) <= 5 * se), (c, est, ex, se)
    assert np.abs(m['exact'][0] - m['exact'][1]).max() > 0.1          # the classes do differ: the clamp matters
    # independent of the slicing: the same seed in slices of 64 rows
    v2, vm2 = small(tmp_path, 64).sample_v_given_class(y, n_gibbs_steps=S['steps'], return_means=True)
    assert np.array_equal(bits(v2), bits(v)) and np.array_equal(bits(vm2), bits(vm))
    # from a start of the caller's: the twin's bits
    V0 = (v[:70] * 0 + 1).astype(np.float32)
    seed_model = small(tmp_path, 64)
    got = seed_model.sample_v_given_class(y[:70], n_gibbs_steps=3, V_init=V0)
    want, _ = T.class_gibbs(m['p'], V0, y[:70], 3, small(tmp_path, 64).make_random_seed())
    assert np.array_equal(bits(got), bits(want))
    got0 = small(tmp_path, 64).sample_v_given_class(y[:70], n_gibbs_steps=2)
    want0, _ = T.class_gibbs(m['p'], None, y[:70], 2, small(tmp_path, 64).make_random_seed())
    assert np.array_equal(bits(got0), bits(want0))


# ---- 8. learning, 9. checkpoints - through the public class
def test_fit_joint_learns_and_round_trips(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM
    L, d = K.LEARN, K.learning_data()
    m = BernoulliRBM(n_visible=L['V'], n_hidden=L['H'], W_init=d['W'], batch_size=L['batch'], l2=L['l2'], random_seed=L['seed'], verbose=False,
                     model_path=str(tmp_path) + '/m/')
    m.set_classes(L['C'], U=d['U'])
    m.init()
    before = m.score(d['X'], d['y'])
    hist = m.fit_joint(d['X'], d['y'], n_epochs=L['epochs'], n_gibbs_steps=L['k'], learning_rate=L['lr'], momentum=L['mom'],
                       discriminative_weight=L['gamma'])
    after = m.score(d['X'], d['y'])
    print('fit_joint: accuracy %.4f untrained, %.4f after %d epochs; epoch accuracies %s' % (before, after, L['epochs'], hist['accuracy']))
    assert after > before and after > L['threshold'], (before, after)
    assert sorted(hist) == ['accuracy', 'log_proba'] and len(hist['accuracy']) == L['epochs']
    assert m.epoch_ == 0 and m.iter_ == 0
    # hybrid, with validation data: the same dict as fit_discriminative's
    hist = m.fit_joint(d['X'], d['y'], X_val=d['X'][:64], y_val=d['y'][:64], n_epochs=2, learning_rate=0.05, discriminative_weight=1.0)
    assert sorted(hist) == ['accuracy', 'log_proba', 'val_accuracy', 'val_log_proba'] and len(hist['val_accuracy']) == 2
    assert m.score(d['X'], d['y']) > L['threshold']
    # fit_joint saved the model: load_model restores the head
    head, logp = m.class_variables(), m.predict_log_proba(d['X'])
    m2 = BernoulliRBM.load_model(str(tmp_path) + '/m/')
    assert m2.n_classes == L['C']
    assert_same(m2.class_variables(), head, 'head variables after load_model')
    assert np.array_equal(bits(m2.predict_log_proba(d['X'])), bits(logp))
