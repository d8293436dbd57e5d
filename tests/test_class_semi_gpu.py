"""-m gpu: semi-supervised training of the classification RBM - class_posterior / class_marginal /
class_unsup_update kernels, bm_rbm_class_unsup_* / bm_rbm_class_semi_train_epoch, BernoulliRBM.fit_semi_supervised.

Bit-exact comparisons (view(uint32)) are against the CPU twin (tests/class_semi_twin.py) wherever the twin's arithmetic is the
engine's: the posterior draw and every state of the chain.  The positive operand em and the parameters after an update pass
through t = x W + hb and prob, whose last places the host does not reproduce: their tolerances are FACTOR = 10 x the float32
twin's own deviation from a float64 restatement on the same chain states, never anything the engine produced."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import class_joint_cases as KJ
from tests import class_joint_twin as J
from tests import class_semi_cases as K
from tests import class_semi_twin as T
from tests import np_reference_class as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = K.NAMES
GEOMETRIES = ('8', '4', '1', '3', '108', '104', '101', '103', '208', '6', '5', '7', '9')      # what launch_act_as accepts
CHAIN_NAMES = ('h0s', 'vk', 'hk')


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


def assert_chain(got, want, what):
    for n in ('y0', 'yk'):
        assert np.array_equal(got[n], want[n]), (what, n, got[n], want[n])
    assert_same(got, want, what, names=CHAIN_NAMES)


def engine_chain(shape, k, **kw):
    V, H, C, B = shape
    c = K.inputs(*shape)
    eng = engine(V, H, C, B, c['p0'], **kw)
    ch = eng.class_unsup_chain(dev(c['X']), B, k)
    eng.close()
    return ch


# ---- 1. the posterior draw
@pytest.mark.parametrize('shape', K.SHAPES)
def test_posterior_draw_is_the_twins(gpu_lib, shape):
    tw = K.chain(*shape, k=1)
    got = engine_chain(shape, 1)
    assert np.array_equal(got['y0'], tw['y0']), (got['y0'], tw['y0'])
    assert len(set(got['y0'])) > 1
    if shape == K.WIDE:
        assert tw['y0'].max() >= 64                       # a class beyond one wave's lanes


# ---- 2. the chain and the positive operand
def check_em(shape, got, what):
    V, H, C, B = shape
    c = K.inputs(*shape)
    _, em64 = T.positive_stats64(c['p0'], c['X'][:B])
    twin_dev, err = R.max_dev(K.chain(*shape)['em'], em64), R.max_dev(got['em'], em64)
    print('%s %r em: twin deviation %.3g, engine deviation %.3g, tolerance %.3g' % (what, shape, twin_dev, err, K.FACTOR * twin_dev))
    assert err <= K.FACTOR * twin_dev, (err, K.FACTOR * twin_dev)


@pytest.mark.parametrize('shape', K.SHAPES)
@pytest.mark.parametrize('k', [1, 3])
def test_chain_is_the_twins(gpu_lib, shape, k):
    """y0, the draw of h0 ~ p(h | x, y0), v_k, y_k, h_k bit-identical to the twin; em within FACTOR x the twin's own deviation
    from float64"""
    got = engine_chain(shape, k)
    assert_chain(got, K.chain(*shape, k=k), 'chain k = %d, shape %r' % (k, shape))
    check_em(shape, got, 'k = %d' % k)


@pytest.mark.parametrize('shape', K.SHAPES)
def test_chain_on_means_is_the_twins(gpu_lib, shape):
    """sample_h_states = False: the chain feeds hidden MEANS downward"""
    got = engine_chain(shape, 2, sample_h_states=False)
    assert_chain(got, K.chain(*shape, k=2, sample_h=False), 'chain on means, shape %r' % (shape,))
    check_em(shape, got, 'means')


# ---- 3. the update
def run_updates(shape, k=1, updates=K.UPDATES, fetch=False, p0=None):
    V, H, C, B = shape
    c = K.inputs(*shape)
    eng = engine(V, H, C, B, p0 or c['p0'])
    Xd = dev(c['X'])
    states, out2 = [], []
    for u in range(updates):
        out2.append(eng.class_unsup_train_step(Xd, B, k, K.LR, K.MOM, row=u * B, fetch=fetch))
        states.append(state(eng))
    eng.close()
    return states, out2


PARITY = {}


def record_parity(shape, rows):
    """profiles/class_semi_parity.md, rewritten once every shape has reported (a run of the whole parametrised test)"""
    PARITY[shape] = rows
    if len(PARITY) < len(K.SHAPES):
        return
    out = ['# Unlabelled update: the engine and the float32 twin against a float64 update on the twin\'s chain states', '',
           'Written by `tests/test_class_semi_gpu.py::test_update_against_float64` on an MI355X: the first update of every case,',
           'max |.| over the entries; tolerance = %g x the twin\'s deviation.' % K.FACTOR, '',
           '| (V, H, C, B) | parameter | twin deviation | engine deviation | tolerance |', '|---|---|---|---|---|']
    for s in K.SHAPES:
        out += ['| %r | %s | %.3g | %.3g | %.3g |' % ((s,) + r) for r in PARITY[s]]
    try:
        with open(os.path.join(ROOT, 'profiles', 'class_semi_parity.md'), 'w') as f:
            f.write('\n'.join(out) + '\n')
    except OSError:
        pass


@pytest.mark.parametrize('shape', K.SHAPES)
def test_update_against_float64(gpu_lib, shape):
    """UPDATES unlabelled updates: the first one leaves every parameter and momentum buffer within FACTOR x the float32 twin's
    deviation from the float64 update evaluated on the twin's chain states (which are the engine's: test_chain_is_the_twins);
    out2 is the twin's mean entropy and confidence; two runs give identical bits at every update.

    Figures (MI355X): profiles/class_semi_parity.md"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    tw = K.trajectory(*shape)
    a, out2 = run_updates(shape, fetch=True)
    ref = T.float64_unsup_update(c['p0'], c['X'][:B], tw['chains'][0], K.LR, K.MOM, K.L2)
    rows, bad = [], []
    for n in NAMES:
        twin_dev, err = R.max_dev(tw['states'][0][n], ref[n]), R.max_dev(a[0][n], ref[n])
        print('unlabelled update %r, %-3s: twin deviation %.3g, engine deviation %.3g, tolerance %.3g' % (shape, n, twin_dev, err, K.FACTOR * twin_dev))
        rows.append((n, twin_dev, err, K.FACTOR * twin_dev))
        if not err <= K.FACTOR * twin_dev:
            bad.append((n, err, K.FACTOR * twin_dev))
    record_parity(shape, rows)
    assert not bad, bad
    for u in range(K.UPDATES):
        assert abs(out2[u][0] - tw['out2'][u][0]) <= 1e-4 and abs(out2[u][1] - tw['out2'][u][1]) <= 1e-4, (u, out2[u], tw['out2'][u])
    b, _ = run_updates(shape)
    for u in range(K.UPDATES):
        assert_same(b[u], a[u], 'two runs, shape %r, update %d' % (shape, u))


# ---- 4. every act_kernel geometry
def chain_digest_lines():
    """one line per shape: the chain of the case's first batch (k = 2) as the engine runs it - y0, h0 states, v_k, y_k, h_k - and
    a second digest of em"""
    out = []
    for shape in K.SHAPES:
        ch = engine_chain(shape, 2)
        h, e = hashlib.sha256(), hashlib.sha256()
        for n in ('y0', 'h0s', 'vk', 'yk', 'hk'):
            h.update(np.ascontiguousarray(ch[n]).tobytes())
        e.update(np.ascontiguousarray(ch['em']).tobytes())
        out.append(h.hexdigest() + ':' + e.hexdigest())
    return out


def twin_chain_digest_lines():
    out = []
    for shape in K.SHAPES:
        ch = K.chain(*shape, k=2)
        h = hashlib.sha256()
        for a in (ch['y0'].astype(np.int32), ch['h0s'], ch['vk'], ch['yk'].astype(np.int32), ch['hk']):
            h.update(np.ascontiguousarray(a).tobytes())
        out.append(h.hexdigest())
    return out


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_class_semi_gpu as G
print('SEMI_DIGEST', ' '.join(G.chain_digest_lines()))
'''


def test_every_geometry_holds_the_chain_digest(gpu_lib):
    """one fresh child per act_kernel geometry (BM355_DEBUG is read once per process), each under its own time limit; the first
    failure ends the test.  The chain's digest is the twin's; em's is that of this process's default geometry"""
    want = twin_chain_digest_lines()
    mine = chain_digest_lines()
    assert [m.split(':')[0] for m in mine] == want
    for geo in GEOMETRIES:
        env = dict(os.environ, BM355_DEBUG='act_geo=' + geo)
        r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'SEMI_DIGEST' in r.stdout, 'act_geo=%s: %s' % (geo, r.stdout[-2000:] + r.stderr[-4000:])
        got = r.stdout.split('SEMI_DIGEST', 1)[1].split()
        assert got == mine, 'act_geo=%s: shapes %r differ' % (geo, [s for s, g, w in zip(K.SHAPES, got, mine) if g != w])


# ---- 5. the epoch entry
@pytest.mark.parametrize('shape', KJ.SHAPES[:2])
def test_epoch_with_zero_weight_is_the_joint_epoch(gpu_lib, shape):
    V, H, C, B = shape
    c = KJ.inputs(*shape)
    N = 2 * B + max(1, B // 3)
    Xd, yd = dev(c['X'][:N]), dev(c['y'][:N], np.int32)
    a, b = engine(V, H, C, B, c['p0']), engine(V, H, C, B, c['p0'])
    for e in (a, b):                                      # ... from the same counter, not the fresh one
        e.class_joint_chain(Xd, yd, B, 1)
    out4 = a.class_semi_train_epoch(Xd, yd, N, None, 0, 0, B, 1, K.LR, K.MOM, 0.0, 0.0)
    out2 = b.class_joint_train_epoch(Xd, yd, N, B, 1, K.LR, K.MOM, 0.0)
    assert_same(state(a), state(b), 'unl_weight = 0 against the joint epoch, shape %r' % (shape,))
    assert out4[:2] == out2 and out4[2:] == (0.0, 0.0)
    a.class_joint_train_step(Xd, yd, B, 1, K.LR, K.MOM, 0.0, fetch=False)          # the counters agree as well
    b.class_joint_train_step(Xd, yd, B, 1, K.LR, K.MOM, 0.0, fetch=False)
    assert_same(state(a), state(b), 'the update after it')
    a.close()
    b.close()


@pytest.mark.parametrize('shape', KJ.SHAPES[:2])
def test_epoch_is_the_loop_over_steps(gpu_lib, shape):
    """three labelled batches (the last one short) against two unlabelled slices (the last one short) from slice 1: the slices
    taken are 1, 0, 1 - the cyclic wrap within one epoch"""
    V, H, C, B = shape
    c = KJ.inputs(*shape)
    N, Nu, beta, gamma = 2 * B + max(1, B // 3), B + B // 2, 0.5, KJ.GAMMA
    Xd, yd, Xud = dev(c['X'][:N]), dev(c['y'][:N], np.int32), dev(K.inputs(*shape)['X'][B:B + Nu])
    a, b, a2 = (engine(V, H, C, B, c['p0']) for _ in range(3))
    out4 = a.class_semi_train_epoch(Xd, yd, N, Xud, Nu, 1, B, 1, K.LR, K.MOM, gamma, beta)
    lr_u = float(np.float32(K.LR) * np.float32(beta))
    sums, u, rows_u = np.zeros(4), 1, 0
    for s in range(0, N, B):
        n = min(B, N - s)
        l, h = b.class_joint_train_step(Xd, yd, n, 1, K.LR, K.MOM, gamma, row=s)
        nu = min(B, Nu - u * B)
        e, f = b.class_unsup_train_step(Xud, nu, 1, lr_u, K.MOM, row=u * B)
        sums += (l * n, h * n, e * nu, f * nu)
        u, rows_u = (u + 1) % 2, rows_u + nu
    assert rows_u == B // 2 + B + B // 2
    assert_same(state(a), state(b), 'epoch against steps, shape %r' % (shape,))
    want = (sums[0] / N, sums[1] / N, sums[2] / rows_u, sums[3] / rows_u)
    assert all(abs(g - w) <= 1e-6 * abs(w) for g, w in zip(out4, want)), (out4, want)
    assert a2.class_semi_train_epoch(Xd, yd, N, Xud, Nu, 1, B, 1, K.LR, K.MOM, gamma, beta, fetch=False) is None
    assert_same(state(a2), state(a), 'epoch without the fetch')
    for e in (a, b, a2):
        e.close()


# ---- 6. the call counter
def test_call_counter(gpu_lib):
    shape = K.SHAPES[0]
    V, H, C, B = shape
    c = K.inputs(*shape)
    Xd = dev(c['X'])
    a, b = engine(V, H, C, B, c['p0']), engine(V, H, C, B, c['p0'])
    a.class_unsup_train_step(Xd, B, 1, 0.0, 0.0, fetch=False)              # lr = 0: nothing moves, the counter does
    assert all(np.array_equal(v, c['p0'][n]) for n, v in state(a).items())          # (values: a momentum buffer may hold -0)
    b.class_unsup_chain(Xd, B, 1)
    for e in (a, b):
        e.class_unsup_train_step(Xd, B, 1, K.LR, K.MOM, fetch=False)
    assert_same(state(a), state(b), 'call counter: one per update')
    # ... and the chain behind them draws at call 2
    got = a.class_unsup_chain(Xd, B, 1)
    p = {n: v for n, v in state(a).items()}
    assert_chain(got, T.unsup_chain(p, c['X'][:B], 1, K.SEED, 2), 'the chain at call 2 against the twin')
    a.close()
    b.close()


# ---- 7. the zero head
@pytest.mark.parametrize('shape', K.SHAPES)
def test_zero_head(gpu_lib, shape):
    """U = 0, yb = 0: p is uniform and em = sum_c p_c sigmoid(t) is the plain pass's means - to (C + 4) ulp of 1: C roundings of
    the fma chain, the rounding of p_c = 1 / C and of the sum of the p_c, the sigmoid's own.  The chain is the plain chain's
    bits (h0 ~ p(h | x, y0) with a zero U is the plain draw at the same site), so the first unlabelled update moves vb, dvb
    exactly as bm_rbm_train_step does from the same seed.  W, hb, dW, dhb, q_means take em where the plain update takes the
    plain means: bit-identical where the fma chain is exact - C a power of two: p_c = 2^-n - and otherwise unreachable, because
    float32(1 / C) summed C times through an fma chain does not return sigmoid(t) to the bit.  For those shapes W, hb, dW, dhb
    are compared with the zero-head twin instead, by the convention of test_update_against_float64"""
    from boltzmann_machines_amd.engine import RbmEngine
    V, H, C, B = shape
    c = K.inputs(*shape)
    p0 = dict(c['p0'], U=np.zeros((C, H), np.float32), yb=np.zeros(C, np.float32))
    X = c['X'][:B]
    Xd = dev(c['X'])
    eng = engine(V, H, C, B, p0)
    assert np.abs(np.exp(eng.class_log_proba(Xd, B).astype(np.float64)) - 1.0 / C).max() <= 1e-6
    ch = eng.class_unsup_chain(Xd, B, 1)
    plain_means, _ = J.act2(X, p0['W'], None, None, p0['hb'], None, 1.0, 0, 1, K.SEED, J.SITE_H0, 0, 0)
    err = R.max_dev(ch['em'], plain_means)
    print('zero head %r: em against the plain means %.3g, bound %.3g' % (shape, err, (C + 4) * 2.0 ** -23))
    assert err <= (C + 4) * 2.0 ** -23
    eng.seed(K.SEED)                                      # back to call 0
    plain = RbmEngine(V, H, max_batch=B, l2=K.L2)
    for n in ('W', 'hb', 'vb'):
        plain.set(n, p0[n])
    plain.seed(K.SEED)
    eng.class_unsup_train_step(Xd, B, 1, K.LR, K.MOM, fetch=False)
    plain.train_step(Xd, B, K.LR, K.MOM, 1)
    exact = ('W', 'hb', 'vb', 'dW', 'dhb', 'dvb', 'q_means') if C & (C - 1) == 0 else ('vb', 'dvb')
    got = state(eng, ('W', 'hb', 'vb', 'dW', 'dhb', 'dvb', 'q_means'))
    assert_same(got, state(plain, exact), 'zero head against bm_rbm_train_step, shape %r' % (shape,), names=exact)
    eng.close()
    plain.close()
    tw = T.SemiRBM(p0, K.SEED, K.L2)
    tw.unsup_step(X, 1, K.LR, K.MOM)
    ref = T.float64_unsup_update(p0, X, tw.last_unsup, K.LR, K.MOM, K.L2)
    for n in ('W', 'hb', 'dW', 'dhb'):
        twin_dev, e = R.max_dev(tw.state()[n], ref[n]), R.max_dev(got[n], ref[n])
        print('zero head %r, %-3s: twin deviation %.3g, engine deviation %.3g, tolerance %.3g' % (shape, n, twin_dev, e, K.FACTOR * twin_dev))
        assert e <= K.FACTOR * twin_dev, (n, e, K.FACTOR * twin_dev)


# ---- 8. refusals
def test_engine_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    V, H, B = 12, 8, 4
    Xd, yd = dev(np.zeros((2 * B, V))), dev(np.zeros(2 * B), np.int32)
    eng = RbmEngine(V, H, max_batch=B)
    for call in (lambda: eng.class_unsup_train_step(Xd, B, 1, 0.1, 0.5), lambda: eng.class_unsup_chain(Xd, B, 1),
                 lambda: eng.class_semi_train_epoch(Xd, yd, 2 * B, Xd, 2 * B, 0, B, 1, 0.1, 0.5)):
        with pytest.raises(_ffi.Bm355Error, match='no class head'):
            call()
    eng.set_classes(3)
    with pytest.raises(_ffi.Bm355Error, match='max_batch'):
        eng.class_unsup_train_step(Xd, 2 * B, 1, 0.1, 0.5)
    with pytest.raises(_ffi.Bm355Error, match='max_batch'):
        eng.class_semi_train_epoch(Xd, yd, 2, Xd, 2 * B, 0, 2 * B, 1, 0.1, 0.5)      # (labelled batches of 2 rows, unlabelled of 8)
    with pytest.raises(_ffi.Bm355Error, match='n_gibbs_steps'):
        eng.class_unsup_train_step(Xd, B, 0, 0.1, 0.5)
    with pytest.raises(_ffi.Bm355Error, match='n_gibbs_steps'):
        eng.class_unsup_chain(Xd, B, 0)
    with pytest.raises(_ffi.Bm355Error, match='disc_weight'):
        eng.class_semi_train_epoch(Xd, yd, 2 * B, Xd, 2 * B, 0, B, 1, 0.1, 0.5, -1.0, 1.0)
    with pytest.raises(_ffi.Bm355Error, match='unl_weight must be >= 0'):
        eng.class_semi_train_epoch(Xd, yd, 2 * B, Xd, 2 * B, 0, B, 1, 0.1, 0.5, 0.0, -0.5)
    with pytest.raises(_ffi.Bm355Error, match='needs unlabelled rows'):
        eng.class_semi_train_epoch(Xd, yd, 2 * B, None, 2 * B, 0, B, 1, 0.1, 0.5, 0.0, 1.0)
    with pytest.raises(_ffi.Bm355Error, match='needs unlabelled rows'):
        eng.class_semi_train_epoch(Xd, yd, 2 * B, Xd, 0, 0, B, 1, 0.1, 0.5, 0.0, 1.0)
    for bad in (-1, 2):
        with pytest.raises(_ffi.Bm355Error, match='u_slice'):
            eng.class_semi_train_epoch(Xd, yd, 2 * B, Xd, 2 * B, bad, B, 1, 0.1, 0.5, 0.0, 1.0)
    with pytest.raises(_ffi.Bm355Error, match='u_slice'):
        eng.class_semi_train_epoch(Xd, yd, 2 * B, None, 0, 1, B, 1, 0.1, 0.5, 0.0, 0.0)
    eng.set_centering(True)
    with pytest.raises(_ffi.Bm355Error, match='centr|centering'):
        eng.class_unsup_train_step(Xd, B, 1, 0.1, 0.5)
    eng.close()
    for kw, match in ((dict(dropout=0.8), 'dropout'), (dict(sparsity_cost=0.1), 'sparsity')):
        e = RbmEngine(V, H, max_batch=B, **kw)
        e.set_classes(3)
        with pytest.raises(_ffi.Bm355Error, match=match):
            e.class_unsup_train_step(Xd, B, 1, 0.1, 0.5)
        with pytest.raises(_ffi.Bm355Error, match=match):
            e.class_semi_train_epoch(Xd, yd, 2 * B, Xd, 2 * B, 0, B, 1, 0.1, 0.5)
        e.close()


# ---- 9. the public class
def learner(tmp_path, name):
    from boltzmann_machines_amd import BernoulliRBM
    L, d = K.LEARN, K.learning_data()
    m = BernoulliRBM(n_visible=L['V'], n_hidden=L['H'], W_init=d['W'], batch_size=L['batch'], l2=L['l2'], random_seed=L['seed'], verbose=False,
                     model_path=str(tmp_path) + '/%s/' % name)
    m.set_classes(L['C'], U=d['U'])
    return m.init()


def test_fit_semi_supervised_learns_and_round_trips(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM
    L, d = K.LEARN, K.learning_data()
    seed = learner(tmp_path, 'seed').make_random_seed()   # what the call below seeds the engine with
    twin = {beta: K.learning_twin(beta, None if seed == K.learning_seed() else seed) for beta in (L['beta'], 0.0)}
    acc, hist = {}, {}
    for beta in (L['beta'], 0.0):
        m = learner(tmp_path, 'b%g' % beta)
        hist[beta] = m.fit_semi_supervised(d['X'], d['y'], d['Xu'], n_epochs=L['epochs'], n_gibbs_steps=L['k'], learning_rate=L['lr'],
                                           momentum=L['mom'], discriminative_weight=L['gamma'], unlabelled_weight=beta)
        acc[beta] = m.score(d['Xval'], d['yval'])
        assert m.epoch_ == 0 and m.iter_ == 0
        print('unlabelled_weight %g: held-out accuracy %.4f, the twin\'s %.4f' % (beta, acc[beta], twin[beta]))
    for beta in acc:
        assert abs(acc[beta] - twin[beta]) <= L['tol'], (beta, acc[beta], twin[beta])
    assert acc[L['beta']] > acc[0.0], acc
    h = hist[L['beta']]
    assert sorted(h) == ['accuracy', 'log_proba', 'unlabelled_confidence', 'unlabelled_entropy']
    assert all(len(v) == L['epochs'] for v in h.values())
    assert all(0 <= e <= np.log(L['C']) + 1e-6 for e in h['unlabelled_entropy']) and all(1.0 / L['C'] - 1e-6 <= v <= 1 for v in h['unlabelled_confidence'])
    assert h['unlabelled_entropy'][-1] < h['unlabelled_entropy'][0]                # the posterior sharpens on the unlabelled rows
    assert all(np.isnan(v) for v in hist[0.0]['unlabelled_entropy'])
    # with validation data: fit_joint's keys beside the new ones; the model was saved: load_model restores the head
    h = m.fit_semi_supervised(d['X'], d['y'], d['Xu'], X_val=d['Xval'][:64], y_val=d['yval'][:64], n_epochs=2, learning_rate=0.05)
    assert sorted(h) == ['accuracy', 'log_proba', 'unlabelled_confidence', 'unlabelled_entropy', 'val_accuracy', 'val_log_proba']
    assert len(h['val_accuracy']) == 2 and m.epoch_ == 0 and m.iter_ == 0
    head, logp = m.class_variables(), m.predict_log_proba(d['Xval'])
    m2 = BernoulliRBM.load_model(str(tmp_path) + '/b0/')
    assert m2.n_classes == L['C']
    assert_same(m2.class_variables(), head, 'head variables after load_model')
    assert np.array_equal(bits(m2.predict_log_proba(d['Xval'])), bits(logp))
