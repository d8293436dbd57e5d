"""Class head of a BernoulliRBM, the parts that need no GPU: the NumPy reference against finite differences, the
seed of the GPU cases, host-side label validation, refusals, checkpoints of a model without a head, the C-ABI surface."""
import json
import os

import numpy as np
import pytest

from tests import class_head_cases as K
from tests import np_reference_class as R


# ---- 1. the reference
@pytest.mark.parametrize('V,H,C,B', [(7, 5, 3, 6), (37, 29, 2, 33)])
def test_reference_gradients_against_finite_differences(V, H, C, B):
    """one random entry of each of W, U, hb, yb: central differences of the batch mean of log p(t|x) in float64"""
    p = R.cast(K.params(V, H, C), np.float64)
    X, y = K.data(B, V, C)
    g, (lp, _) = R.gradients(p, X, y)
    assert abs(lp - R.mean_log_proba(p, X, y)) < 1e-12
    assert not g['vb'].any()
    rng = np.random.RandomState(5)
    eps = 1e-5
    for name in ('W', 'U', 'hb', 'yb'):
        idx = tuple(rng.randint(n) for n in p[name].shape)
        hi, lo = R.cast(p, np.float64), R.cast(p, np.float64)
        hi[name][idx] += eps
        lo[name][idx] -= eps
        fd = (R.mean_log_proba(hi, X, y) - R.mean_log_proba(lo, X, y)) / (2 * eps)
        assert abs(fd - g[name][idx]) <= 1e-7 * max(1.0, abs(fd)), (name, idx, fd, g[name][idx])


def test_reference_masked_row_contributes_nothing():
    """keep[j] = False: every sum is the one without row j, the divisor stays B"""
    V, H, C, B = 7, 5, 3, 6
    p = R.cast(K.params(V, H, C), np.float64)
    X, y = K.data(B, V, C)
    keep = np.ones(B, bool)
    keep[2] = False
    g, out2 = R.gradients(p, X, y, keep=keep)
    sub, out2_sub = R.gradients(p, X[keep], y[keep])
    for name in g:
        np.testing.assert_allclose(g[name], sub[name] * (B - 1) / B, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(out2, np.array(out2_sub) * (B - 1) / B, rtol=1e-12)


@pytest.mark.parametrize('V,H,C,B', K.SHAPES)
def test_gpu_cases_have_a_clear_argmax(V, H, C, B):
    """the seed of the GPU cases: on every row the float64 top-two gap of log p(c|x) exceeds the tolerance of the forward test,
    so that test compares the argmax of EVERY row; the twin's own deviation is float32 round-off"""
    c = K.case(V, H, C, B)
    assert 0 < c['logp_twin_dev'] < 1e-4, c['logp_twin_dev']
    assert K.top_two_gap(c['logp_ref']).min() > c['logp_tol'], (K.top_two_gap(c['logp_ref']).min(), c['logp_tol'])
    for u in range(K.UPDATES):
        for name in ('vb', 'dvb'):          # vb sees a zero gradient: from dvb = 0 it never moves
            assert np.array_equal(c['twin'][u][name], c['p0'][name]) and np.array_equal(c['ref'][u][name], c['p0'][name])


def test_learning_case_learns_in_the_reference():
    c = K.learning_case()
    assert c['ref'][0] > -0.1 and c['ref'][1] == 1.0, c['ref']
    assert c['twin'][1] == c['ref'][1] and 0 < c['tol'] < 1e-3, (c['twin'], c['tol'])


# ---- 2. labels
def test_label_validation():
    from boltzmann_machines_amd.classification import validate_labels
    y = validate_labels(np.array([0, 2, 1], dtype=np.int64), 3, 3)
    assert y.dtype == np.int32 and y.flags['C_CONTIGUOUS'] and y.tolist() == [0, 2, 1]
    for bad, match in (([0, 3, 1], 'outside'), ([0, -1, 1], 'outside'), ([0, 1], 'labels for 3 rows'), ([0., 1., 2.], 'integer'),
                       ([[0], [1], [2]], 'shape')):
        with pytest.raises(ValueError, match=match):
            validate_labels(np.array(bad), 3, 3)


def _model(cls=None, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    return (cls or BernoulliRBM)(n_visible=6, n_hidden=4, batch_size=5, random_seed=1337, verbose=False, **kw)


def test_fit_discriminative_validates_on_the_host():
    """bad labels and shapes raise before an engine exists: nothing is uploaded"""
    m = _model().set_classes(3)
    X = np.zeros((4, 6), np.float32)
    for y, match in (([0, 1, 2, 3], 'outside'), ([0, 1, 2], 'labels for 4 rows'), (np.zeros(4), 'integer')):
        with pytest.raises(ValueError, match=match):
            m.fit_discriminative(X, np.array(y))
    with pytest.raises(ValueError, match='shape'):
        m.fit_discriminative(np.zeros((4, 5), np.float32), np.zeros(4, int))
    with pytest.raises(ValueError, match='batch_size'):
        m.fit_discriminative(X, np.zeros(4, int), batch_size=6)
    with pytest.raises(ValueError, match='go together'):
        m.fit_discriminative(X, np.zeros(4, int), X_val=X)
    assert m._engine is None


# ---- 3. refusals that need no device
def test_refusals(monkeypatch):
    from boltzmann_machines_amd import GaussianRBM, MultinomialRBM
    X, y = np.zeros((4, 6), np.float32), np.zeros(4, int)
    with pytest.raises(ValueError, match='Gaussian'):
        _model(GaussianRBM).set_classes(3)
    with pytest.raises(ValueError, match='Multinomial'):
        _model(MultinomialRBM).set_classes(3)
    with pytest.raises(ValueError, match='float32'):
        _model(dtype='float64').set_classes(3)
    with pytest.raises(ValueError, match='dbm_first'):
        _model(dbm_first=True).set_classes(3)
    for bad in (1, 2.5, 0):
        with pytest.raises(ValueError, match='n_classes'):
            _model().set_classes(bad)
    with pytest.raises(ValueError, match='shape'):
        _model().set_classes(3, U=np.zeros((3, 5)))
    for name in ('predict', 'predict_proba', 'predict_log_proba'):
        with pytest.raises(ValueError, match='no class head'):
            getattr(_model(), name)(X)
    with pytest.raises(ValueError, match='no class head'):
        _model().fit_discriminative(X, y)
    with pytest.raises(ValueError, match='dropout'):
        _model(dropout=0.8).set_classes(3).fit_discriminative(X, y)
    with pytest.raises(ValueError, match='sparsity'):
        _model(sparsity_cost=0.1).set_classes(3).fit_discriminative(X, y)
    with pytest.raises(ValueError, match='centering'):
        _model().set_centering(True).set_classes(3).fit_discriminative(X, y)
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(ValueError, match='data parallelism'):
        _model().set_classes(3).fit_discriminative(X, y)


# ---- 4. checkpoints
def test_model_without_a_head_serialises_as_before():
    """params.json and the variable list of a model that has no head - or no longer has one - carry nothing of the feature"""
    fresh = _model()
    want = json.dumps(fresh._serialize(dict(fresh.get_params(deep=False))), sort_keys=True, indent=4)
    assert 'n_classes' not in want and 'class' not in want
    assert fresh._class_variables() == {} and fresh.class_variables() is None and fresh.n_classes is None
    m = _model().set_classes(3, U_std=0.1)
    assert m.n_classes == 3 and m.get_params()['n_classes'] == 3
    v = m._class_variables()
    assert sorted(v) == ['class_U', 'class_dU', 'class_dyb', 'class_yb'] and v['class_U'].shape == (3, 4)
    assert v['class_U'].dtype == np.float32 and 0.01 < v['class_U'].std() < 0.3 and not v['class_dU'].any() and not v['class_yb'].any()
    # the draw comes from the model's seeded stream: the same seed, the same U
    assert np.array_equal(v['class_U'], _model().set_classes(3, U_std=0.1)._class_variables()['class_U'])
    m.set_classes(None)
    assert m.n_classes is None and m._class_variables() == {}
    # (the draw advanced the host stream; everything params.json holds is as before)
    assert json.dumps(m._serialize(dict(m.get_params(deep=False))), sort_keys=True, indent=4) == want


def test_restore_from_checkpoint_arrays():
    """load_model's hand-over: the class_* arrays leave the dict and wait for the engine; n_classes is a constructor keyword for
    load_model's sake only"""
    from boltzmann_machines_amd import BernoulliRBM
    U = np.arange(12, dtype=np.float32).reshape(3, 4)
    d = dict(W=np.zeros((6, 4), np.float32), class_U=U, class_yb=np.ones(3, np.float32), class_dU=U * 2, class_dyb=np.ones(3, np.float32) * 3)
    m = BernoulliRBM(n_visible=6, n_hidden=4, n_classes=3, verbose=False)
    assert m.n_classes is None
    m._class_restore(d)
    assert sorted(d) == ['W'] and m.n_classes == 3
    v = m.class_variables()
    assert np.array_equal(v['U'], U) and np.array_equal(v['dU'], U * 2) and np.array_equal(v['dyb'], np.ones(3) * 3)
    m2 = _model()
    m2._class_restore(dict(W=d['W']))
    assert m2.n_classes is None and m2._class_head is None


# ---- 5. surface
def test_abi_surface():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'bm355.h')).read()
    for decl in ('int bm_rbm_set_classes(bm_rbm *h, int32_t n_classes);',
                 'int bm_rbm_class_log_proba(bm_rbm *h, const float *X_dev, int32_t B, float *logp_host',
                 'int bm_rbm_class_train_step(bm_rbm *h, const float *X_dev, const int32_t *y_dev',
                 'int bm_rbm_class_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev'):
        assert decl in header, decl
    assert [len(_ffi.SIGNATURES[n]) for n in ('bm_rbm_set_classes', 'bm_rbm_class_log_proba', 'bm_rbm_class_train_step',
                                              'bm_rbm_class_train_epoch')] == [2, 4, 7, 8]
    for name in ('set_classes', 'class_log_proba', 'class_train_step', 'class_train_epoch'):
        assert callable(getattr(RbmEngine, name)) and not hasattr(RbmEngine64, name)
