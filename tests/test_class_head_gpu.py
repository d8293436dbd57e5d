"""-m gpu: the class head of a BernoulliRBM - act_kernel's class-rows flavour, class_row / class_hidden /
class_head_update kernels, bm_rbm_set_classes / bm_rbm_class_*, BernoulliRBM.set_classes / fit_discriminative / predict.

Tolerances are FACTOR = 10 x the float32 twin's own deviation from the float64 reference on the same inputs
(tests/class_head_cases.py), never anything the engine produced.  Bit-exact comparisons are view(uint32)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import class_head_cases as K
from tests import np_reference_class as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = R.NAMES
GEOMETRIES = ('8', '4', '1', '3', '108', '104', '101', '103', '208', '6', '5', '7', '9')      # what launch_act_as accepts


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev(a, dt=np.float32):
    from boltzmann_machines_amd._ffi import DeviceArray
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dt), dt)


def engine(V, H, C, B, p0, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    eng = RbmEngine(V, H, max_batch=B, l2=K.L2, **kw)
    eng.set_classes(C)
    for n in NAMES:
        eng.set(n, p0[n])
    return eng


def state(eng, names=NAMES):
    return {n: eng.get(n) for n in names}


def assert_same(got, want, what):
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), '%s: %s differs in %d of %d entries (max abs %.3g)' % (
            what, k, int(np.sum(bits(got[k]) != bits(want[k]))), want[k].size, float(np.abs(got[k] - want[k]).max()))


def run_updates(shape, step=True):
    """3 updates of the case from its start: the state after each, and every out2"""
    V, H, C, B = shape
    c = K.case(*shape)
    eng = engine(V, H, C, B, c['p0'])
    Xd, yd = dev(c['X']), dev(c['y'], np.int32)
    states, out2 = [], []
    for u in range(K.UPDATES):
        out2.append(eng.class_train_step(Xd, yd, B, K.LR, K.MOM, row=u * B))
        states.append(state(eng))
    eng.close()
    return states, out2


def digest(states):
    h = hashlib.sha256()
    for s in states:
        for n in NAMES:
            h.update(bits(s[n]).tobytes())
    return h.hexdigest()


# ---- 1. forward
@pytest.mark.parametrize('shape', K.SHAPES)
def test_forward_against_float64(gpu_lib, shape):
    V, H, C, B = shape
    c = K.case(*shape)
    eng = engine(V, H, C, B, c['p0'])
    L = eng.class_log_proba(dev(c['X'][:B]), B)
    err = R.max_dev(L, c['logp_ref'])
    print('forward %r: twin deviation %.3g, engine deviation %.3g, tolerance %.3g' % (shape, c['logp_twin_dev'], err, c['logp_tol']))
    assert L.shape == (B, C) and L.dtype == np.float32
    assert err <= c['logp_tol'], (err, c['logp_tol'])
    clear = K.top_two_gap(c['logp_ref']) > c['logp_tol']
    assert clear.all()                                   # (asserted of the seed on the CPU as well: no row is left out)
    assert np.array_equal(L.argmax(axis=1)[clear], c['logp_ref'].argmax(axis=1)[clear])
    # any B: more rows than max_batch, in one call, gives the rows of the batch calls; the RNG call counter is not touched
    L3 = eng.class_log_proba(dev(c['X']), K.UPDATES * B)
    assert np.array_equal(bits(L3[:B]), bits(L))
    eng.close()


# ---- 2. update
@pytest.mark.parametrize('shape', K.SHAPES)
def test_update_against_float64(gpu_lib, shape):
    c = K.case(*shape)
    states, out2 = run_updates(shape)
    for u in range(K.UPDATES):
        for n in NAMES:
            twin_dev = R.max_dev(c['twin'][u][n], c['ref'][u][n])
            err = R.max_dev(states[u][n], c['ref'][u][n])
            print('update %r, step %d, %-3s: twin deviation %.3g, engine deviation %.3g, tolerance %.3g' % (shape, u, n, twin_dev, err, K.FACTOR * twin_dev))
            assert err <= K.FACTOR * twin_dev, (u, n, err, K.FACTOR * twin_dev)
        # vb sees the plain rule with a zero gradient, bit for bit: from dvb = 0 it never moves
        assert not bits(states[u]['dvb']).any() and np.array_equal(bits(states[u]['vb']), bits(c['p0']['vb']))
        # out2 comes back as float32: half an ulp of the value on top of FACTOR x the twin's deviation (whose mean is taken in
        # float64 and carries no such rounding)
        lp_tol = K.FACTOR * abs(c['out2_twin'][u][0] - c['out2'][u][0]) + float(np.spacing(np.float32(abs(c['out2'][u][0])))) / 2
        print('update %r, step %d, out2: reference %r, twin %r, engine %r, tolerance %.3g' % (shape, u, c['out2'][u], c['out2_twin'][u], out2[u], lp_tol))
        assert abs(out2[u][0] - c['out2'][u][0]) <= lp_tol, (u, out2[u], c['out2'][u], lp_tol)
        assert out2[u][1] == np.float32(c['out2'][u][1]), (u, out2[u], c['out2'][u])


def test_vb_momentum_decays_under_the_plain_rule(gpu_lib):
    """a non-zero dvb: d = lr * (mom * dvb + 0), vb += d, in float32, bit for bit"""
    shape = K.SHAPES[0]
    V, H, C, B = shape
    c = K.case(*shape)
    p0 = dict(c['p0'], dvb=(c['p0']['vb'] * np.float32(0.1)).astype(np.float32))
    eng = engine(V, H, C, B, p0)
    eng.class_train_step(dev(c['X']), dev(c['y'], np.int32), B, K.LR, K.MOM, fetch=False)
    d = np.float32(K.LR) * (np.float32(K.MOM) * p0['dvb'] + np.float32(0))
    assert_same(state(eng, ('dvb', 'vb')), dict(dvb=d, vb=p0['vb'] + d), 'vb under a zero gradient')
    eng.close()


# ---- 3. determinism and geometry independence
CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import class_head_cases as K
from tests import test_class_head_gpu as T
print('CLASS_DIGEST', ' '.join(T.digest(T.run_updates(s)[0]) for s in K.SHAPES))
'''


@pytest.fixture(scope='module')
def default_digests(gpu_lib):
    return [digest(run_updates(s)[0]) for s in K.SHAPES]


def test_two_runs_hold_identical_bits(gpu_lib, default_digests):
    for s, want in zip(K.SHAPES, default_digests):
        a, b = run_updates(s)[0], run_updates(s)[0]
        for u in range(K.UPDATES):
            assert_same(a[u], b[u], 'two engines, shape %r, update %d' % (s, u))
        assert digest(a) == want


def test_forced_geometries_hold_identical_bits(gpu_lib, default_digests):
    """one fresh child per act_kernel geometry (BM355_DEBUG is read once per process), each under its own time limit; the first
    failure ends the test"""
    for geo in GEOMETRIES:
        env = dict(os.environ, BM355_DEBUG='act_geo=' + geo)
        r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'CLASS_DIGEST' in r.stdout, 'act_geo=%s: %s' % (geo, r.stdout[-2000:] + r.stderr[-4000:])
        got = r.stdout.split('CLASS_DIGEST', 1)[1].split()
        assert got == default_digests, 'act_geo=%s: shapes %r differ from the tuned geometry' % (
            geo, [s for s, g, w in zip(K.SHAPES, got, default_digests) if g != w])


# ---- 4. the native epoch loop
@pytest.mark.parametrize('shape', K.SHAPES[:2])
def test_epoch_is_the_loop_over_steps(gpu_lib, shape):
    """N = 2 B + a short last batch: the same bits, and out2 averaged over the rows"""
    V, H, C, B = shape
    c = K.case(*shape)
    N = 2 * B + max(1, B // 3)
    Xd, yd = dev(c['X'][:N]), dev(c['y'][:N], np.int32)
    a, b = engine(V, H, C, B, c['p0']), engine(V, H, C, B, c['p0'])
    lp, acc = a.class_train_epoch(Xd, yd, N, B, K.LR, K.MOM)
    slp = sacc = 0.0
    for s in range(0, N, B):
        n = min(B, N - s)
        l, h = b.class_train_step(Xd, yd, n, K.LR, K.MOM, row=s)
        slp, sacc = slp + l * n, sacc + h * n
    assert_same(state(a), state(b), 'epoch against steps, shape %r' % (shape,))
    assert abs(lp - slp / N) <= 1e-6 * abs(slp / N) and abs(acc - sacc / N) <= 1e-6
    # ... and without the fetch the entry only queues: the same bits again
    a2 = engine(V, H, C, B, c['p0'])
    assert a2.class_train_epoch(Xd, yd, N, B, K.LR, K.MOM, fetch=False) is None
    assert_same(state(a2), state(a), 'epoch without the fetch')
    for e in (a, b, a2):
        e.close()


# ---- 5. learning, through the public class
def learning_model(tmp_path, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    c, L = K.learning_case(), K.LEARN
    m = BernoulliRBM(n_visible=L['V'], n_hidden=L['H'], W_init=c['p0']['W'], batch_size=L['batch'], l2=L['l2'], random_seed=1337,
                     verbose=False, model_path=str(tmp_path) + '/', **kw)
    return m, c, L


def test_fit_discriminative_learns(gpu_lib, tmp_path):
    m, c, L = learning_model(tmp_path)
    m.set_classes(L['C'], U=c['p0']['U'])
    hist = m.fit_discriminative(c['X'], c['y'], n_epochs=L['epochs'], learning_rate=L['lr'], momentum=L['mom'])
    lp = float(m.predict_log_proba(c['X'])[np.arange(L['N']), c['y']].astype(np.float64).mean())
    acc = m.score(c['X'], c['y'])
    print('learning: reference %r, twin %r, engine (%.7f, %.4f), tolerance %.3g' % (c['ref'], c['twin'], lp, acc, c['tol']))
    assert abs(lp - c['ref'][0]) <= c['tol'], (lp, c['ref'][0], c['tol'])
    assert acc == c['ref'][1]
    assert len(hist['log_proba']) == L['epochs'] and hist['log_proba'][0] < hist['log_proba'][-1] and hist['accuracy'][-1] >= hist['accuracy'][0]
    assert m.epoch_ == 0 and m.iter_ == 0
    assert np.array_equal(m.predict(c['X']), m.predict_proba(c['X']).argmax(axis=1))


# ---- 6. pre-train, fine-tune, save, load
def test_pretrain_finetune_roundtrip(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM
    from boltzmann_machines_amd.engine import RbmEngine
    m, c, L = learning_model(tmp_path, max_epoch=1, learning_rate=0.05)
    m.fit(c['X'])
    assert m.epoch_ == 1
    m.set_classes(L['C'], U_std=L['scale'])
    Xv, yv = c['X'][:64], c['y'][:64]
    hist = m.fit_discriminative(c['X'], c['y'], X_val=Xv, y_val=yv, n_epochs=3, learning_rate=[L['lr'], 0.25], momentum=L['mom'])
    assert sorted(hist) == ['accuracy', 'log_proba', 'val_accuracy', 'val_log_proba'] and len(hist['val_accuracy']) == 3
    assert m.epoch_ == 1
    pred, head, logp = m.predict(c['X']), m.class_variables(), m.predict_log_proba(c['X'])
    params = open(os.path.join(str(tmp_path), 'params.json')).read()
    assert '"n_classes": 4' in params
    m2 = BernoulliRBM.load_model(str(tmp_path) + '/')
    assert m2.n_classes == L['C']
    assert np.array_equal(m2.predict(c['X']), pred) and np.array_equal(bits(m2.predict_log_proba(c['X'])), bits(logp))
    assert_same(m2.class_variables(), head, 'head variables after load_model')
    # detached: a generative update gives the bits of an engine that never had a head
    names = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')
    start = {n: m._engine.get(n) for n in names}
    m.set_classes(None)
    assert m.n_classes is None and m.class_variables() is None
    with pytest.raises(Exception, match='unknown RBM variable'):
        m._engine.get('U')
    plain = RbmEngine(L['V'], L['H'], max_batch=L['batch'], l2=L['l2'])
    for n in names:
        plain.set(n, start[n])
    Xd = dev(c['X'])
    for e in (m._engine, plain):
        e.seed(99)
        e.train_step(Xd, L['batch'], 0.05, 0.5, 1)
    assert_same({n: m._engine.get(n) for n in names}, {n: plain.get(n) for n in names}, 'generative step after detaching the head')
    plain.close()
    m._save_model()
    m._join_save()
    assert 'n_classes' not in open(os.path.join(str(tmp_path), 'params.json')).read()
    with np.load(os.path.join(str(tmp_path), 'model.npz')) as z:
        assert not [k for k in z.files if k.startswith('class_')]


def test_engine_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    V, H, B = 12, 8, 4
    Xd, yd = dev(np.zeros((2 * B, V))), dev(np.zeros(2 * B), np.int32)
    eng = RbmEngine(V, H, max_batch=B)
    with pytest.raises(_ffi.Bm355Error, match='no class head'):
        eng.class_log_proba(Xd, B)
    with pytest.raises(_ffi.Bm355Error, match='no class head'):
        eng.class_train_step(Xd, yd, B, 0.1, 0.5)
    with pytest.raises(_ffi.Bm355Error, match='n_classes'):
        eng.set_classes(1)
    eng.set_classes(3)
    with pytest.raises(_ffi.Bm355Error, match='max_batch'):
        eng.class_train_step(Xd, yd, 2 * B, 0.1, 0.5)
    eng.set_centering(True)
    with pytest.raises(_ffi.Bm355Error, match='centr|centering'):
        eng.class_train_step(Xd, yd, B, 0.1, 0.5)
    eng.close()
    for kw, match in ((dict(v_unit=_ffi.UNIT_GAUSSIAN), 'Gaussian'), (dict(h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=3), 'Multinomial'),
                      (dict(dbm_first=True), 'dbm_first')):
        e = RbmEngine(V, H, max_batch=B, **kw)
        with pytest.raises(_ffi.Bm355Error, match=match):
            e.set_classes(3)
        e.close()
    for kw, match in ((dict(dropout=0.8), 'dropout'), (dict(sparsity_cost=0.1), 'sparsity')):
        e = RbmEngine(V, H, max_batch=B, **kw)
        e.set_classes(3)
        with pytest.raises(_ffi.Bm355Error, match=match):
            e.class_train_step(Xd, yd, B, 0.1, 0.5)
        e.close()


# ---- 7. a label outside [0, C) through the C ABI
def test_bad_label_leaves_its_row_out(gpu_lib):
    """The label C indexes nothing: the next sync reports it once, and the row is out of every sum (the divisor stays B) -
    the parameters are those of the float64 reference with that row masked, they do not depend on which bad value the label has
    nor on the row's input, and a valid batch afterwards runs as ever."""
    from boltzmann_machines_amd import _ffi
    shape = K.SHAPES[0]
    V, H, C, B = shape
    c = K.case(*shape)
    X, y = c['X'][:B].copy(), c['y'][:B].copy()
    row = 5
    keep = np.ones(B, bool)
    keep[row] = False
    results = []
    for label, Xrow in ((C, X[row]), (-1, X[row]), (2 ** 30, X[row]), (C, 1 - X[row])):
        yb, Xb = y.copy(), X.copy()
        yb[row], Xb[row] = label, Xrow
        eng = engine(V, H, C, B, c['p0'])
        eng.class_train_step(dev(Xb), dev(yb, np.int32), B, K.LR, K.MOM, fetch=False)
        with pytest.raises(_ffi.Bm355Error, match='label outside'):
            eng.sync()
        eng.sync()                                       # reported once, then cleared
        results.append(state(eng))
        eng.close()
    for other in results[1:]:
        assert_same(other, results[0], 'bad label: another bad value / another input in the masked row')
    ref, _ = R.step(c['p0'], X, y, np.float32(K.LR), np.float32(K.MOM), np.float32(K.L2), np.float64, keep=keep)
    twin, _ = R.step(c['p0'], X, y, K.LR, K.MOM, K.L2, np.float32, keep=keep)
    for n in NAMES:
        assert R.max_dev(results[0][n], ref[n]) <= K.FACTOR * R.max_dev(twin[n], ref[n]), n
    # the fetch reports it too, and the engine goes on
    eng = engine(V, H, C, B, c['p0'])
    yb = y.copy()
    yb[row] = C
    with pytest.raises(_ffi.Bm355Error, match='label outside'):
        eng.class_train_step(dev(X), dev(yb, np.int32), B, K.LR, K.MOM)
    lp, acc = eng.class_train_step(dev(X), dev(y, np.int32), B, K.LR, K.MOM)
    assert np.isfinite(lp) and 0 <= acc <= 1
    eng.close()
