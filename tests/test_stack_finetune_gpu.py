"""-m gpu: fine-tuning a stack of sigmoid layers below a class head by back-propagation - act_kernel's BP
flavour, stack_g_kernel, bm_rbm_backprop_down / bm_rbm_delta_update / bm_rbm_class_stack_*, StackClassifier.

Bounds are FACTOR = 10 x the float32 twin's own deviation from the float64 restatement on the same inputs
(tests/stack_cases.py), never anything the engine produced.  Bit-exact comparisons are view(uint32)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import np_reference_class as R
from tests import np_reference_stack as S
from tests import stack_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(K.STACKS)
GEOMETRIES = ('8', '4', '1', '3', '108', '104', '101', '103', '208', '6', '5', '7', '9')      # tests/test_class_head_gpu.py's


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev(a, dt=np.float32):
    from boltzmann_machines_amd._ffi import DeviceArray
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dt), dt)


def stack_engine(c, p=None, l2s=None, max_batch=None):
    """one RbmEngine per layer of case c holding the stack p (default: the start), the head on the last one"""
    from boltzmann_machines_amd.engine import RbmEngine, StackEngine
    p = c['p0'] if p is None else p
    l2s = c['l2s'] if l2s is None else l2s
    engines = []
    for i, l in enumerate(p['layers'] + [p['top']]):
        V, H = l['W'].shape
        e = RbmEngine(V, H, max_batch=max_batch or c['B'], l2=l2s[i])
        if 'U' in l:
            e.set_classes(c['C'])
        for n in l:
            e.set(n, l[n])
        engines.append(e)
    return StackEngine(engines)


def state(se):
    return dict(layers=[{n: e.get(n) for n in S.LAYER_NAMES} for e in se.below], top={n: se.top.get(n) for n in R.NAMES})


def close(*stacks):
    for se in stacks:
        for e in se.engines:
            e.close()


def flat(st):
    out = {'%s%d' % (n, i + 1): l[n] for i, l in enumerate(st['layers']) for n in l}
    out.update(st['top'])
    return out


def assert_same(got, want, what):
    got, want = flat(got), flat(want)
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), '%s: %s differs in %d of %d entries (max abs %.3g)' % (
            what, k, int(np.sum(bits(got[k]) != bits(want[k]))), want[k].size, float(np.abs(got[k] - want[k]).max()))


# ---- 1. gradient parity, per layer
@pytest.mark.parametrize('name', NAMES)
def test_gradient_parity(gpu_lib, name):
    """one step with momentum 0 and l2 0: (P_after - P_before) / lr of every W_l, hb_l, U, yb against the float64 gradient"""
    c = K.case(name)
    se = stack_engine(c, l2s=[0.0] * (c['D'] + 1))
    se.train_step(dev(c['X']), dev(c['y'], np.int32), c['B'], c['glr'], 0.0, fetch=False)
    se.sync()
    after = state(se)
    got = K.grad_like(c['p0'], after, K.GRAD_LR)
    for k in sorted(c['grad_ref']):
        twin_dev, err = c['grad_tol'][k] / K.FACTOR, S.max_dev(got[k], c['grad_ref'][k])
        print('PARITY %s %-4s: engine %.3g, twin %.3g, bound %.3g' % (name, k, err, twin_dev, c['grad_tol'][k]))
    for k in sorted(c['grad_ref']):
        err = S.max_dev(got[k], c['grad_ref'][k])
        assert err <= c['grad_tol'][k], (name, k, err, c['grad_tol'][k])
    for i, l in enumerate(after['layers'] + [after['top']]):
        before = (c['p0']['layers'] + [c['p0']['top']])[i]
        assert np.array_equal(bits(l['vb']), bits(before['vb'])) and not bits(l['dvb']).any(), 'vb of layer %d moved' % i
    close(se)


# ---- 2. no backward pass reads a weight its own step has written
@pytest.mark.parametrize('name', NAMES)
def test_three_steps_read_pre_update_weights(gpu_lib, name):
    """three consecutive steps with momentum 0.5 and l2 > 0 against the twin's bound, on the parameters themselves (the wrong
    order misses it by orders of magnitude: tests/test_stack_finetune.py)"""
    c = K.case(name)
    se = stack_engine(c)
    Xd, yd = dev(c['X']), dev(c['y'], np.int32)
    for u in range(K.UPDATES):
        se.train_step(Xd, yd, c['B'], c['lrs'], K.MOM)
        got, ref, twin = S.tensors(state(se)), S.tensors(c['ref'][u]), S.tensors(c['twin'][u])
        for k in sorted(ref):
            tol, err = K.FACTOR * S.max_dev(twin[k], ref[k]), S.max_dev(got[k], ref[k])
            print('STEPS %s step %d %-4s: engine %.3g, twin %.3g, bound %.3g' % (name, u, k, err, tol / K.FACTOR, tol))
            assert err <= tol, (name, u, k, err, tol)
    close(se)


# ---- 3. no layers below: bm_rbm_class_train_step
def test_empty_stack_is_the_class_train_step(gpu_lib):
    from boltzmann_machines_amd.engine import StackEngine
    c = K.case('S1')
    top = dict(layers=[], top=c['p0']['top'])
    V = top['top']['W'].shape[0]
    X = c['X'][:, :V]
    Xd, yd = dev(X), dev(c['y'], np.int32)
    a, b = stack_engine(c, top, l2s=[K.L2]), stack_engine(c, top, l2s=[K.L2])
    for u in range(2):
        oa = a.train_step(Xd, yd, c['B'], [K.LR], K.MOM, row=u * c['B'])
        ob = b.top.class_train_step(Xd, yd, c['B'], K.LR, K.MOM, row=u * c['B'])
        assert np.array_equal(bits(oa), bits(ob)), (oa, ob)
        assert_same(state(a), state(b), 'stack without layers below, step %d' % u)
    assert np.array_equal(bits(a.log_proba(Xd, len(X))), bits(b.top.class_log_proba(Xd, len(X))))
    assert isinstance(a, StackEngine) and a.n_below == 0
    close(a, b)


# ---- 4. the native epoch loop
def test_epoch_is_the_loop_over_steps(gpu_lib):
    """S1, N = 25 in batches of 10, 10 and 5: the same bits, and out2 averaged over the rows"""
    c = K.case('S1')
    N, B = c['N'], c['B']
    Xd, yd = dev(c['X'][:N]), dev(c['y'][:N], np.int32)
    a, b, q = stack_engine(c), stack_engine(c), stack_engine(c)
    lp, acc = a.train_epoch(Xd, yd, N, B, c['lrs'], K.MOM)
    slp = sacc = 0.0
    for s in range(0, N, B):
        n = min(B, N - s)
        l, h = b.train_step(Xd, yd, n, c['lrs'], K.MOM, row=s)
        slp, sacc = slp + l * n, sacc + h * n
    assert_same(state(a), state(b), 'epoch against steps')
    assert abs(lp - slp / N) <= 1e-6 * abs(slp / N) and abs(acc - sacc / N) <= 1e-6
    assert q.train_epoch(Xd, yd, N, B, c['lrs'], K.MOM, fetch=False) is None      # only queues
    q.sync()
    assert_same(state(q), state(a), 'epoch without the fetch')
    close(a, b, q)


# ---- 5. determinism
@pytest.mark.parametrize('name', NAMES)
def test_two_runs_hold_identical_bits(gpu_lib, name):
    c = K.case(name)
    Xd, yd = dev(c['X']), dev(c['y'], np.int32)
    out = []
    for _ in range(2):
        se = stack_engine(c)
        o = [se.train_step(Xd, yd, c['B'], c['lrs'], K.MOM) for _ in range(2)]
        out.append((state(se), o))
        close(se)
    assert_same(out[0][0], out[1][0], 'two runs from the same state')
    assert out[0][1] == out[1][1]


# ---- 6. / 7. the BP pass alone
def bp_inputs(c):
    """per handle of the stack: (W, Delta [B, H], A [B, V]) with Delta ~ N(0, 1) and A in (0, 1)"""
    from boltzmann_machines_amd.utils import philox
    out = []
    for i, l in enumerate(c['p0']['layers'] + [c['p0']['top']]):
        V, H = l['W'].shape
        D = philox.normal(K.SEED, 120 + i, 0, c['B'] * H).astype(np.float32).reshape(c['B'], H)
        A = philox.uniform(K.SEED, 140 + i, 0, c['B'] * V).astype(np.float32).reshape(c['B'], V)
        out.append((l['W'], D, A))
    return out


def run_bp(name):
    """[(Out with A, Out without A)] per handle of the stack, through bm_rbm_backprop_down"""
    from boltzmann_machines_amd._ffi import DeviceArray
    c = K.case(name)
    se = stack_engine(c)
    out = []
    for e, (W, D, A) in zip(se.engines, bp_inputs(c)):
        Oa, Oz = DeviceArray((c['B'], e.V), np.float32), DeviceArray((c['B'], e.V), np.float32)
        e.backprop_down(dev(D), c['B'], Oa, dev(A))
        e.backprop_down(dev(D), c['B'], Oz)
        e.sync()
        out.append((Oa.numpy(), Oz.numpy()))
    close(se)
    return out


def bp_digest(names=NAMES):
    h = hashlib.sha256()
    for name in names:
        for pair in run_bp(name):
            for o in pair:
                h.update(bits(o).tobytes())
    return h.hexdigest()


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_stack_finetune_gpu as T
print('BP_DIGEST', T.bp_digest())
'''


@pytest.fixture(scope='module')
def default_bp_digest(gpu_lib):
    return bp_digest()


@pytest.mark.parametrize('geo', GEOMETRIES)
def test_backprop_down_under_forced_geometries(gpu_lib, default_bp_digest, geo):
    """one fresh child per act_kernel geometry (BM355_DEBUG is read once per process), under its own time limit"""
    env = dict(os.environ, BM355_DEBUG='act_geo=' + geo)
    r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'BP_DIGEST' in r.stdout, 'act_geo=%s: %s' % (geo, r.stdout[-2000:] + r.stderr[-4000:])
    assert r.stdout.split('BP_DIGEST', 1)[1].split()[0] == default_bp_digest, 'act_geo=%s differs from the tuned geometry' % geo


@pytest.mark.parametrize('name', NAMES)
def test_backprop_down_against_float64(gpu_lib, name):
    """with A: (Delta W^T) .* A .* (1 - A); without: Delta W^T itself (no linear prop-down of the same operand is reachable through
    the C ABI, so both are held to the twin's bound); a padded pitch of A and of Out gives the bits of the dense call"""
    from boltzmann_machines_amd._ffi import DeviceArray
    c = K.case(name)
    for i, ((W, D, A), (Oa, Oz)) in enumerate(zip(bp_inputs(c), run_bp(name))):
        z64 = D.astype(np.float64).dot(W.astype(np.float64).T)
        z32 = D.dot(W.T)
        for what, got, ref, twin in (('z', Oz, z64, z32), ('delta', Oa, S.sigmoid_derivative(z64, A, np.float64),
                                                          S.sigmoid_derivative(z32, A, np.float32))):
            tol, err = K.FACTOR * S.max_dev(twin, ref), S.max_dev(got, ref)
            print('BP %s handle %d %-5s: engine %.3g, twin %.3g, bound %.3g' % (name, i, what, err, tol / K.FACTOR, tol))
            assert err <= tol, (name, i, what, err, tol)
        # the stated association, bit for bit, from the engine's own z
        assert np.array_equal(bits(Oa), bits(S.sigmoid_derivative(Oz, A, np.float32))), (name, i)
    # pitches: A and Out as the leading columns of wider matrices
    se = stack_engine(c)
    e, (W, D, A), (Oa, _) = se.engines[0], bp_inputs(c)[0], run_bp(name)[0]
    pad = 8
    Aw = np.full((c['B'], e.V + pad), 0.5, np.float32)
    Aw[:, :e.V] = A
    Ow = dev(np.full((c['B'], e.V + pad), -7.0, np.float32))
    e.backprop_down(dev(D), c['B'], Ow, dev(Aw), lda=e.V + pad, ldo=e.V + pad)
    e.sync()
    got = Ow.numpy()
    assert np.array_equal(bits(got[:, :e.V]), bits(Oa)) and np.all(got[:, e.V:] == -7.0), 'padded pitch'
    close(se)


def test_delta_update_is_the_layer_update(gpu_lib):
    """bm_rbm_delta_update alone: dW = X^T Delta / B, dhb = colmean(Delta), vb untouched - against float64 under the twin's bound"""
    c = K.case('S1')
    l = c['p0']['layers'][0]
    se = stack_engine(c)
    e = se.engines[0]
    X = c['X'][:c['B']]
    D = bp_inputs(c)[0][1] * np.float32(0.1)
    e.delta_update(dev(X), dev(D), c['B'], K.LR, K.MOM)
    e.sync()
    res = {}
    for dt in (np.float64, np.float32):
        p = R.cast(l, dt)
        S.apply_layer(p, S.layer_gradients(X.astype(dt), D.astype(dt), dt), np.float32(K.LR), np.float32(K.MOM), np.float32(K.L2), dt)
        res[dt] = p
    for n in ('W', 'hb', 'dW', 'dhb'):
        tol, err = K.FACTOR * S.max_dev(res[np.float32][n], res[np.float64][n]), S.max_dev(e.get(n), res[np.float64][n])
        assert err <= tol, (n, err, tol)
    assert np.array_equal(bits(e.get('vb')), bits(l['vb']))
    close(se)


# ---- 8. prediction
def test_log_proba_of_more_rows_than_max_batch(gpu_lib):
    c = K.case('S1')
    se = stack_engine(c)
    N, B = c['N'], c['B']
    Xd = dev(c['X'][:N])
    L = se.log_proba(Xd, N)
    parts = np.concatenate([se.log_proba(Xd, min(B, N - s), row=s) for s in range(0, N, B)])
    assert L.shape == (N, c['C']) and np.array_equal(bits(L), bits(parts))
    err = S.max_dev(L, c['logp_ref'][:N])
    print('LOGP S1: engine %.3g, bound %.3g' % (err, c['logp_tol']))
    assert err <= c['logp_tol'], (err, c['logp_tol'])
    # a_D of the same rows, in the same slices
    from boltzmann_machines_amd._ffi import DeviceArray
    Ad = DeviceArray((N, se.top.V), np.float32)
    se.transform(Xd, N, Ad)
    a64, a32 = S.activations(S.cast(c['p0'], np.float64), c['X'][:N])[-1], S.activations(S.cast(c['p0'], np.float32), c['X'][:N], np.float32)[-1]
    assert S.max_dev(Ad.numpy(), a64) <= K.FACTOR * S.max_dev(a32, a64)
    close(se)


# ---- 9. a label outside [0, C)
def test_bad_label_moves_no_parameter_through_its_row(gpu_lib):
    from boltzmann_machines_amd import _ffi
    c = K.case('S1')
    B, C = c['B'], c['C']
    X, y = c['X'][:B].copy(), c['y'][:B].copy()
    row = 4
    keep = np.ones(B, bool)
    keep[row] = False
    results = []
    for label, Xrow in ((C, X[row]), (-1, X[row]), (C, 1 - X[row])):
        yb, Xb = y.copy(), X.copy()
        yb[row], Xb[row] = label, Xrow
        se = stack_engine(c)
        se.train_step(dev(Xb), dev(yb, np.int32), B, c['lrs'], K.MOM, fetch=False)
        with pytest.raises(_ffi.Bm355Error, match='label outside'):
            se.sync()
        se.sync()                                        # reported once, then cleared
        results.append(state(se))
        close(se)
    for other in results[1:]:
        assert_same(other, results[0], 'bad label: another bad value / another input in the masked row')
    f = [np.float32(v) for v in c['lrs']], np.float32(K.MOM), [np.float32(v) for v in c['l2s']]
    ref, _ = S.step(c['p0'], X, y, f[0], f[1], f[2], np.float64, keep=keep)
    twin, _ = S.step(c['p0'], X, y, c['lrs'], K.MOM, c['l2s'], np.float32, keep=keep)
    got, ref, twin = S.tensors(results[0]), S.tensors(ref), S.tensors(twin)
    for k in sorted(ref):
        assert S.max_dev(got[k], ref[k]) <= K.FACTOR * S.max_dev(twin[k], ref[k]), k


# ---- 10. the public class
def toy_stack(tmp_path, tag='s'):
    from boltzmann_machines_amd import BernoulliRBM, StackClassifier
    c, T = K.toy_case(), K.TOY
    layers = []
    for i, l in enumerate(c['p0']['layers'] + [c['p0']['top']]):
        V, H = l['W'].shape
        layers.append(BernoulliRBM(n_visible=V, n_hidden=H, W_init=l['W'], vb_init=l['vb'], hb_init=l['hb'], batch_size=T['batch'],
                                   l2=T['l2'], random_seed=7 + i, verbose=False, model_path=str(tmp_path / ('%s_r%d' % (tag, i))) + '/'))
    layers[-1].set_classes(T['C'], U=c['p0']['top']['U'], yb=c['p0']['top']['yb'])
    s = StackClassifier.from_rbms(layers, T['C'], learning_rate=T['lr'], momentum=T['mom'], max_epoch=T['epochs'],
                                  model_path=str(tmp_path / (tag + '_stack')) + '/')
    return s, c, T


def test_stack_classifier_learns_saves_and_loads(gpu_lib, tmp_path):
    from boltzmann_machines_amd import StackClassifier
    s, c, T = toy_stack(tmp_path)
    X, y = c['X'], c['y']
    nll0 = -float(s.predict_log_proba(X)[np.arange(len(y)), y].astype(np.float64).mean())
    assert s.fit(X, y) is s
    L = s.predict_log_proba(X)
    nll = -float(L[np.arange(len(y)), y].astype(np.float64).mean())
    print('TOY: NLL %.4f -> %.4f, accuracy %.3f; float64 reference %r, twin %r' % (nll0, nll, s.score(X, y), c['ref'], c['twin']))
    assert nll < nll0 and s.score(X, y) == 1.0
    assert len(s.history_['log_proba']) == T['epochs'] and s.history_['log_proba'][0] < s.history_['log_proba'][-1]
    assert np.array_equal(s.predict(X), s.predict_proba(X).argmax(axis=1))
    A = s.transform(X)
    assert A.shape == (len(X), T['widths'][0]) and A.min() > 0 and A.max() < 1
    assert np.array_equal(bits(s.layers[-1].predict_log_proba(A)), bits(L))       # the head of the top model on a_D
    s2 = StackClassifier.load_model(s.model_path)
    assert s2.n_classes == T['C'] and len(s2.layers) == 2 and s2.batch_size == s.batch_size
    assert np.array_equal(bits(s2.predict_log_proba(X)), bits(L)) and np.array_equal(s2.predict(X), s.predict(X))


def test_from_dbm_fits_and_predicts(gpu_lib, tmp_path):
    from boltzmann_machines_amd import DBM, BernoulliRBM, StackClassifier
    c, T = K.toy_case(), K.TOY
    X, y = c['X'], c['y']
    kw = dict(max_epoch=1, batch_size=T['batch'], verbose=False)
    r1 = BernoulliRBM(n_visible=T['V'], n_hidden=12, random_seed=1, model_path=str(tmp_path / 'r1') + '/', **kw)
    r1.fit(X)
    r2 = BernoulliRBM(n_visible=12, n_hidden=10, random_seed=2, model_path=str(tmp_path / 'r2') + '/', **kw)
    r2.fit(r1.transform(X))
    dbm = DBM(rbms=[r1, r2], n_particles=T['batch'], max_mf_updates=10, random_seed=3, model_path=str(tmp_path / 'dbm') + '/', **kw)
    dbm.fit(X)
    w = {k: v.copy() for k, v in dbm.get_tf_params(scope='weights').items()}
    s = StackClassifier.from_dbm(dbm, T['C'], learning_rate=0.5, max_epoch=2, model_path=str(tmp_path / 'stack') + '/')
    assert [(m.n_visible, m.n_hidden) for m in s.layers] == [(16, 12), (12, 10)]
    assert np.array_equal(bits(s.layers[0].W_init), bits(w['W'] * np.float32(2))) and np.array_equal(bits(s.layers[1].W_init), bits(w['W_1']))
    s.fit(X, y)
    assert s.predict(X).shape == (len(X),) and np.isfinite(s.history_['log_proba']).all()
    after = dbm.get_tf_params(scope='weights')
    assert all(np.array_equal(bits(after[k]), bits(w[k])) for k in w), 'the DBM was modified'


# ---- 11. library refusals
def test_library_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, StackEngine
    V, H, H2, B, C = 12, 8, 6, 4, 3
    Xd, yd = dev(np.zeros((2 * B, V))), dev(np.zeros(2 * B), np.int32)

    def top(**kw):
        e = RbmEngine(H, H2, max_batch=B, **kw)
        e.set_classes(C)
        return e

    def refused(engines, match, B=B):
        with pytest.raises(_ffi.Bm355Error, match=match):
            StackEngine(engines).train_step(Xd, yd, B, 0.1, 0.5)
        with pytest.raises(_ffi.Bm355Error, match=match):
            StackEngine(engines).log_proba(Xd, B)
        for e in engines:
            e.close()

    good = StackEngine([RbmEngine(V, H, max_batch=B), top()])
    lp, acc = good.train_step(Xd, yd, B, 0.1, 0.5)
    assert np.isfinite(lp) and 0 <= acc <= 1
    with pytest.raises(_ffi.Bm355Error, match='max_batch'):
        good.train_step(Xd, yd, 2 * B, 0.1, 0.5)
    close(good)
    refused([RbmEngine(V, H, max_batch=B, v_unit=_ffi.UNIT_GAUSSIAN), top()], 'Gaussian')
    refused([RbmEngine(V, H, max_batch=B, h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=3), top()], 'Multinomial')
    refused([RbmEngine(V, H, max_batch=B, dbm_first=True), top()], 'dbm_first')
    refused([RbmEngine(V, H, max_batch=B, dbm_last=True), top()], 'dbm_last')
    refused([RbmEngine(V, H, max_batch=B, dropout=0.8), top()], 'dropout')
    refused([RbmEngine(V, H, max_batch=B, sparsity_cost=0.1), top()], 'sparsity')
    refused([RbmEngine(V, H, max_batch=B), top(dropout=0.8)], 'dropout')
    centred = RbmEngine(V, H, max_batch=B)
    centred.set_centering(True)
    refused([centred, top()], 'centr')
    refused([RbmEngine(V, H + 1, max_batch=B), top()], 'do not chain')
    refused([RbmEngine(V, H, max_batch=B), RbmEngine(H, H2, max_batch=B)], 'no class head')
    small = StackEngine([RbmEngine(V, H, max_batch=B - 1), top()])
    with pytest.raises(_ffi.Bm355Error, match='max_batch'):
        small.train_step(Xd, yd, B, 0.1, 0.5)
    close(small)
    twice = RbmEngine(H, H, max_batch=B)
    e = RbmEngine(H, H, max_batch=B)
    e.set_classes(C)
    with pytest.raises(_ffi.Bm355Error, match='twice'):
        StackEngine([twice, twice, e]).train_step(dev(np.zeros((B, H))), yd, B, 0.1, 0.5)
    with pytest.raises(_ffi.Bm355Error, match='twice'):
        StackEngine([e, e]).train_step(dev(np.zeros((B, H))), yd, B, 0.1, 0.5)
    twice.close()
    e.close()
    # the single-handle entries refuse the same handles
    g = RbmEngine(V, H, max_batch=B, v_unit=_ffi.UNIT_GAUSSIAN)
    with pytest.raises(_ffi.Bm355Error, match='Gaussian'):
        g.backprop_down(dev(np.zeros((B, H))), B, dev(np.zeros((B, V))))
    with pytest.raises(_ffi.Bm355Error, match='Gaussian'):
        g.delta_update(Xd, dev(np.zeros((B, H))), B, 0.1, 0.5)
    g.close()
