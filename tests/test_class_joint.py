"""CPU: joint training of the classification RBM - the twin against the existing oracle, the conditions the
GPU tests rely on (no class draw of any case near a prefix sum), the twin's discriminative term against the float64 reference,
and the host surface (refusals, signatures, the C ABI).  Nothing here needs a device."""
import inspect
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import class_joint_cases as K
from tests import class_joint_twin as T
from tests import np_reference_class as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the twin against the oracle
@pytest.mark.parametrize('shape', K.SHAPES)
@pytest.mark.parametrize('k', [1, 2])
def test_twin_with_zero_head_is_the_oracle_update(shape, k):
    """U held at zero (and yb: it does not enter a prop-up): the CB pass is the plain pass, so W, hb, vb and their momenta after
    3 updates are those of OracleRBM.train_step with the same seed, bit for bit"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    p0 = dict(c['p0'], U=np.zeros((C, H), np.float32), yb=np.zeros(C, np.float32))
    tw = T.JointRBM(p0, K.SEED, K.L2)
    ref = orc.OracleRBM(V, H, l2=K.L2)
    for n in ('W', 'vb', 'hb'):
        ref.p[n][...] = p0[n]
    ref.set_seed(K.SEED)
    for u in range(K.UPDATES):
        Xb, yb = c['X'][u * B:(u + 1) * B], c['y'][u * B:(u + 1) * B]
        tw.train_step(Xb, yb, k, K.LR, K.MOM)
        assert tw.head['dU'].any()                       # the head did learn; it is put back to zero for the next update
        for n in ('U', 'yb', 'dU', 'dyb'):
            tw.head[n][...] = 0
        ref.train_step(Xb, K.LR, K.MOM, k)
        for n in ('W', 'hb', 'vb', 'dW', 'dhb', 'dvb', 'q_means'):
            assert np.array_equal(bits(tw.rbm.p[n]), bits(ref.p[n])), (u, n)
    assert tw.call == ref.call == K.UPDATES


def test_cb_pass_with_a_label_outside_takes_the_plain_bias():
    c = K.inputs(*K.SHAPES[0])
    V, H, C, B = K.SHAPES[0]
    X, y = c['X'][:B], c['y'][:B].copy()
    y[3], y[4] = C, -1
    m, s = T.cb_pass(c['p0'], X, y, 1, K.SEED, T.SITE_H0, 0)
    zero = dict(c['p0'], U=np.zeros((C, H), np.float32))
    mp, sp = T.cb_pass(zero, X, y, 1, K.SEED, T.SITE_H0, 0)
    for j in (3, 4):
        assert np.array_equal(bits(m[j]), bits(mp[j])) and np.array_equal(bits(s[j]), bits(sp[j]))
    assert not np.array_equal(bits(m[5]), bits(mp[5]))


# ---- 2. the condition of the bit-exact GPU comparisons
def test_no_class_draw_sits_on_a_prefix_sum():
    """device exp and libm's may differ in the last place: a draw whose u * total is within that of a prefix sum could land in
    another class.  No draw of any case is closer than MIN_MARGIN (relative to the total); every case is checked"""
    n = 0
    for shape in K.SHAPES:
        V, H, C, B = shape
        c = K.inputs(*shape)
        assert all(set(c['y'][u * B:(u + 1) * B]) == set(range(C)) for u in range(K.UPDATES))          # labels cover every class
        for kw in (dict(k=1), dict(k=3, updates=1), dict(k=1, gamma=K.GAMMA, updates=1)):
            m = K.trajectory(*shape, **kw)['margins']
            assert len(m) == B * kw['k'] * kw.get('updates', K.UPDATES)
            assert min(m) >= K.MIN_MARGIN, (shape, kw, min(m))
            n += len(m)
        # ... and the draws from hidden MEANS (sample_h_states = False) of the class-draw test
        tw = T.JointRBM(c['p0'], K.SEED, K.L2, sample_h_states=False)
        tw.train_step(c['X'][:B], c['y'][:B], 2, K.LR, K.MOM)
        assert min(tw.margins) >= K.MIN_MARGIN, (shape, min(tw.margins))
    assert n > 0


def test_class_draw_follows_the_posterior():
    """the draw is a draw from softmax(yb + h U^T): frequencies over many rows with one h"""
    p = dict(U=np.array([[1.0, -1.0, 0.5], [0.0, 0.3, -0.2], [-0.5, 0.5, 1.0]], np.float32), yb=np.array([0.1, -0.2, 0.3], np.float32))
    h = np.tile(np.array([1.0, 0.0, 1.0], np.float32), (20000, 1))
    y = T.class_draw(p, h, 99, T.SITE_CLASS_Y, 0)
    logit = p['yb'].astype(np.float64) + h[0].astype(np.float64).dot(p['U'].astype(np.float64).T)
    pr = np.exp(logit - logit.max())
    pr /= pr.sum()
    freq = np.bincount(y, minlength=3) / float(len(y))
    assert np.all(np.abs(freq - pr) <= 5 * np.sqrt(pr * (1 - pr) / len(y))), (freq, pr)


# ---- 3. the twin's discriminative term
@pytest.mark.parametrize('shape', K.SHAPES)
def test_twin_discriminative_term_against_float64(shape):
    """gamma x the float64 gradient of the batch mean of log p(t|x) (np_reference_class): the twin's contribution to dU, dyb and
    dW within FACTOR x the deviation of the float32 restatement of that reference"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    X, y, p0 = c['X'][:B], c['y'][:B], c['p0']
    g64, _ = R.gradients(R.cast(p0, np.float64), X, y, np.float64)
    g32, _ = R.gradients(R.cast(p0, np.float32), X, y, np.float32)
    Tt, coef, g, _ = T.disc_parts(p0, X, y)
    zero = np.zeros((B, H), np.float32)
    sU, syb = T.head_sums(C, y, y, zero, zero, K.GAMMA, coef, Tt, p0['U'])          # (y_k = y, h0m = h_k = 0: no generative term)
    mixed = T._fma(np.float32(K.GAMMA), g, zero)
    dW = (X.T.astype(np.float32).dot(mixed) / np.float32(B)).astype(np.float32)
    for name, got in (('U', sU / np.float32(B)), ('yb', syb / np.float32(B)), ('W', dW)):
        want = K.GAMMA * g64[name]
        own = R.max_dev(K.GAMMA * g32[name].astype(np.float64), want)
        err = R.max_dev(got, want)
        print('%r d%s: float32 restatement deviation %.3g, twin deviation %.3g, tolerance %.3g' % (shape, name, own, err, K.FACTOR * own))
        assert own > 0 and err <= K.FACTOR * own, (name, err, own)


# ---- 4. the twin learns the toy problem the GPU test fits
def test_twin_reaches_the_learning_threshold():
    L, d = K.LEARN, K.learning_data()
    from boltzmann_machines_amd import BernoulliRBM
    m = BernoulliRBM(n_visible=L['V'], n_hidden=L['H'], W_init=d['W'], batch_size=L['batch'], l2=L['l2'], random_seed=L['seed'], verbose=False)
    m.set_classes(L['C'], U=d['U'])
    seed = m.make_random_seed()                          # the first draw of the model's host stream: what fit_joint seeds the engine with
    z = lambda *s: np.zeros(s, np.float32)
    p0 = dict(W=d['W'], hb=z(L['H']), vb=z(L['V']), U=d['U'], yb=z(L['C']), dU=z(L['C'], L['H']), dyb=z(L['C']))
    tw = T.JointRBM(p0, seed, L['l2'])
    acc0 = float((tw.log_proba(d['X']).argmax(axis=1) == d['y']).mean())
    for _ in range(L['epochs']):
        tw.train_epoch(d['X'], d['y'], L['batch'], L['k'], L['lr'], L['mom'], L['gamma'])
    acc = float((tw.log_proba(d['X']).argmax(axis=1) == d['y']).mean())
    print('twin: accuracy %.4f untrained, %.4f after %d epochs' % (acc0, acc, L['epochs']))
    assert acc > acc0 and acc > L['threshold'], (acc0, acc)


# ---- 5. the host surface
def _model(cls=None, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    return (cls or BernoulliRBM)(n_visible=6, n_hidden=4, batch_size=5, random_seed=1337, verbose=False, **kw)


def test_fit_joint_refusals(monkeypatch):
    from boltzmann_machines_amd import GaussianRBM, MultinomialRBM
    X, y = np.zeros((4, 6), np.float32), np.zeros(4, int)
    with pytest.raises(ValueError, match='no class head'):
        _model().fit_joint(X, y)
    with pytest.raises(ValueError, match='no class head'):
        _model().sample_v_given_class(y)
    for cls, kw, match in ((GaussianRBM, {}, 'Gaussian'), (MultinomialRBM, {}, 'Multinomial'), (None, dict(dtype='float64'), 'float32'),
                           (None, dict(dbm_first=True), 'dbm_first')):
        m = _model(cls, **kw)
        m._class_head = dict(C=3, pending=None)          # (set_classes itself refuses these models)
        with pytest.raises(ValueError, match=match):
            m.fit_joint(X, y)
        with pytest.raises(ValueError, match=match):
            m.sample_v_given_class(y)
    with pytest.raises(ValueError, match='dropout'):
        _model(dropout=0.8).set_classes(3).fit_joint(X, y)
    with pytest.raises(ValueError, match='sparsity'):
        _model(sparsity_cost=0.1).set_classes(3).fit_joint(X, y)
    with pytest.raises(ValueError, match='centering'):
        _model().set_centering(True).set_classes(3).fit_joint(X, y)
    m = _model().set_classes(3)
    for bad, match in (([0, 1, 2, 3], 'outside'), ([0, -1, 2, 1], 'outside'), ([0, 1, 2], 'labels for 4 rows'), (np.zeros(4), 'integer')):
        with pytest.raises(ValueError, match=match):
            m.fit_joint(X, np.array(bad))
    with pytest.raises(ValueError, match='outside'):
        m.sample_v_given_class(np.array([0, 3]))
    with pytest.raises(ValueError, match='shape'):
        m.sample_v_given_class(np.zeros((2, 2), int))
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError, match='n_gibbs_steps'):
            m.fit_joint(X, y, n_gibbs_steps=k)
    with pytest.raises(ValueError, match='n_gibbs_steps'):
        m.sample_v_given_class(y, n_gibbs_steps=0)
    for g in (-0.5, float('nan')):
        with pytest.raises(ValueError, match='discriminative_weight'):
            m.fit_joint(X, y, discriminative_weight=g)
    with pytest.raises(ValueError, match='batch_size'):
        m.fit_joint(X, y, batch_size=6)
    with pytest.raises(ValueError, match='go together'):
        m.fit_joint(X, y, X_val=X)
    with pytest.raises(ValueError, match='V_init'):
        m.sample_v_given_class(y, V_init=np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match='rows for'):
        m.sample_v_given_class(y, V_init=np.zeros((3, 6), np.float32))
    assert m._engine is None                             # nothing was built or uploaded
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(ValueError, match='data parallelism'):
        _model().set_classes(3).fit_joint(X, y)


def test_signature_defaults():
    from boltzmann_machines_amd import BernoulliRBM
    s = inspect.signature(BernoulliRBM.fit_joint)
    assert list(s.parameters) == ['self', 'X', 'y', 'X_val', 'y_val', 'n_epochs', 'n_gibbs_steps', 'learning_rate', 'momentum',
                                  'discriminative_weight', 'batch_size', 'verbose']
    assert [s.parameters[n].default for n in list(s.parameters)[3:]] == [None, None, 10, 1, 0.05, 0.5, 0., None, None]
    s = inspect.signature(BernoulliRBM.sample_v_given_class)
    assert [(n, p.default) for n, p in list(s.parameters.items())[2:]] == [('n_gibbs_steps', None), ('V_init', None), ('return_means', False)]


def test_abi_surface():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'bm355.h')).read()
    for decl in ('int bm_rbm_class_joint_train_step(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [B] */, int32_t B, int32_t n_gibbs_steps,',
                 'int bm_rbm_class_joint_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [N] */, int64_t N, int32_t batch,',
                 'int bm_rbm_class_joint_chain(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int32_t B, int32_t n_gibbs_steps,',
                 'int bm_rbm_class_gibbs(bm_rbm *h, const float *V_dev /* nullable */, const int32_t *y_dev /* [B] */, int32_t B, int32_t n_steps,'):
        assert decl in header, decl
    names = ('bm_rbm_class_joint_train_step', 'bm_rbm_class_joint_train_epoch', 'bm_rbm_class_joint_chain', 'bm_rbm_class_gibbs')
    assert [len(_ffi.SIGNATURES[n]) for n in names] == [9, 10, 10, 7]
    lib = _ffi.load()
    for n in names:
        assert hasattr(lib, n), n
    for name in ('class_joint_train_step', 'class_joint_train_epoch', 'class_joint_chain', 'class_gibbs'):
        assert callable(getattr(RbmEngine, name)) and not hasattr(RbmEngine64, name)
