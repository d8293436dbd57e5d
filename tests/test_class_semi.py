"""Semi-supervised training of the classification RBM without a GPU: the CPU twin (tests/class_semi_twin.py)
against float64 restatements and finite differences, the conditions the bit-exact GPU comparisons rest on, the condition on the
learning problem of the public-class test, and the host-side surface."""
import inspect
import os

import numpy as np
import pytest

from tests import class_joint_twin as J
from tests import class_semi_cases as K
from tests import class_semi_twin as T
from tests import np_reference_class as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the conditions of the bit-exact GPU comparisons
def test_no_draw_sits_on_a_prefix_sum():
    """the device's exp and the host's may differ in the last place of prob: a posterior draw whose u * total is within that of
    a prefix sum could land in another class.  No posterior draw of any case is closer than Y0_MARGIN (relative to the total),
    no class draw of the chain closer than MIN_MARGIN; every case the GPU tests run is checked"""
    n = 0
    for shape in K.SHAPES:
        V, H, C, B = shape
        runs = [K.trajectory(*shape), K.chain(*shape, k=1), K.chain(*shape, k=3), K.chain(*shape, k=2), K.chain(*shape, k=2, sample_h=False)]
        for r in runs:
            assert len(r['y0_margins']) >= B and len(r['margins']) >= B
            assert min(r['y0_margins']) >= K.Y0_MARGIN, (shape, min(r['y0_margins']))
            assert min(r['margins']) >= K.MIN_MARGIN, (shape, min(r['margins']))
            n += len(r['y0_margins'])
    assert n > 0


@pytest.mark.parametrize('shape', K.SHAPES)
def test_posterior_draws_cover_the_classes(shape):
    """more than one start class occurs in every case; on the wide shape a class beyond a wave's 64 lanes"""
    y0 = K.chain(*shape)['y0']
    assert len(set(y0)) > 1 and y0.min() >= 0 and y0.max() < shape[2]
    if shape == K.WIDE:
        assert y0.max() >= 64, y0


def test_posterior_draw_follows_the_posterior():
    """frequencies of the draw over many rows with one posterior; entropy and confidence against their definitions"""
    pr = np.array([0.1, 0.25, 0.0, 0.4, 0.25], np.float32)
    y0, ent, conf = T.posterior_draw(np.tile(pr, (20000, 1)), 99, 0)
    freq = np.bincount(y0, minlength=5) / float(len(y0))
    p64 = pr.astype(np.float64)
    assert np.all(np.abs(freq - p64) <= 5 * np.sqrt(p64 * (1 - p64) / len(y0)) + 1e-12), (freq, pr)
    nz = p64[p64 > 0]
    assert abs(float(ent[0]) + float((nz * np.log(nz)).sum())) < 1e-6 and conf[0] == pr.max()


# ---- 2. the exact positive phase
@pytest.mark.parametrize('shape', [(7, 5, 3, 4), (6, 4, 70, 3)])
def test_positive_phase_is_the_gradient_of_log_px(shape):
    """(X^T em, colsum em, sum_j p_jc S_jci, sum_j p_jc, colsum X) in float64 against central finite differences of
    sum_j (x_j . vb + logsumexp_c s_c(x_j)) in every entry of W, hb, U, yb, vb"""
    V, H, C, B = shape
    p = {k: v.astype(np.float64) for k, v in K.H.params(V, H, C).items()}
    X, _ = K.H.data(B, V, C)
    stats, _ = T.positive_stats64(p, X)
    eps = 1e-5
    for name in ('W', 'hb', 'U', 'yb', 'vb'):
        fd = np.zeros_like(p[name])
        for idx in np.ndindex(*p[name].shape):
            hi, lo = dict(p), dict(p)
            hi[name], lo[name] = p[name].copy(), p[name].copy()
            hi[name][idx] += eps
            lo[name][idx] -= eps
            fd[idx] = (T.log_px_unnorm64(hi, X) - T.log_px_unnorm64(lo, X)) / (2 * eps)
        err = R.max_dev(stats[name], fd)
        # central differences: truncation eps^2 f''' / 6 and rounding ~ 1e-16 |f| / eps, |f| ~ 1e2 here
        assert err <= 1e-7, (name, err)


@pytest.mark.parametrize('shape', K.SHAPES)
def test_twin_positive_operand_against_float64(shape):
    """em of the float32 twin against the float64 restatement: it deviates (float32 arithmetic) but by less than 1e-5"""
    V, H, C, B = shape
    c = K.inputs(*shape)
    _, em64 = T.positive_stats64(c['p0'], c['X'][:B])
    err = R.max_dev(K.chain(*shape)['em'], em64)
    print('%r em: float32 twin deviation %.3g' % (shape, err))
    assert 0 < err < 1e-5
    # ... and it is the exact negation of class_hidden_kernel's negm chain: fma(-p, S, .) from 0
    ch = K.chain(*shape)
    negm = np.zeros((B, H), np.float32)
    for cc in range(C):
        negm = J._fma(-ch['prob'][:, cc][:, None], J.sigmoid32((ch['T'] + c['p0']['U'][cc][None, :]).astype(np.float32)), negm)
    assert np.array_equal(bits(-negm), bits(ch['em']))


# ---- 3. the twin itself
def test_twin_is_deterministic():
    shape = K.SHAPES[0]
    V, H, C, B = shape
    c = K.inputs(*shape)
    want = K.trajectory(*shape)
    tw = T.SemiRBM(c['p0'], K.SEED, K.L2)
    for u in range(K.UPDATES):
        tw.unsup_step(c['X'][u * B:(u + 1) * B], 1, K.LR, K.MOM)
        got = tw.state()
        for n in K.NAMES:
            assert np.array_equal(bits(got[n]), bits(want['states'][u][n])), (u, n)
    assert tw.call == K.UPDATES


def test_twin_with_zero_unlabelled_weight_is_the_joint_twin():
    from tests import class_joint_cases as KJ
    shape = KJ.SHAPES[0]
    V, H, C, B = shape
    c = KJ.inputs(*shape)
    a, b = T.SemiRBM(c['p0'], K.SEED, K.L2), J.JointRBM(c['p0'], K.SEED, K.L2)
    cur = a.semi_epoch(c['X'], c['y'], None, 0, B, 1, K.LR, K.MOM, 0.0, 0.0)
    b.train_epoch(c['X'], c['y'], B, 1, K.LR, K.MOM, 0.0)
    assert cur == 0 and a.call == b.call == K.UPDATES
    sa, sb = a.state(), b.state()
    for n in K.NAMES:
        assert np.array_equal(bits(sa[n]), bits(sb[n])), n


def test_twin_semi_epoch_wraps_the_slices():
    shape = K.SHAPES[2]
    V, H, C, B = shape
    from tests import class_joint_cases as KJ
    c = KJ.inputs(*shape)
    Xu = K.inputs(*shape)['X'][:B + B // 2]              # two slices, the last one short: three labelled batches wrap
    tw = T.SemiRBM(c['p0'], K.SEED, K.L2)
    seen = []
    step = tw.unsup_step
    tw.unsup_step = lambda X, *a, **kw: (seen.append(len(X)), step(X, *a, **kw))[1]
    assert tw.semi_epoch(c['X'], c['y'], Xu, 1, B, 1, K.LR, K.MOM, 0.0, 0.5) == 0
    assert seen == [B // 2, B, B // 2] and tw.call == 2 * K.UPDATES


# ---- 4. the condition on the learning problem of the public-class test
def test_unlabelled_rows_help_the_twin():
    L = K.LEARN
    semi, sup = K.learning_twin(L['beta']), K.learning_twin(0.0)
    print('twin, held-out accuracy: %.4f semi-supervised, %.4f with unlabelled_weight = 0' % (semi, sup))
    assert semi - sup >= L['gain'], (semi, sup)
    d = K.learning_data()
    assert len(d['X']) == L['N'] and len(d['Xu']) == L['Nu'] >= 8 * L['N'] and len(d['Xval']) == L['Nval']
    from boltzmann_machines_amd import BernoulliRBM
    m = BernoulliRBM(n_visible=L['V'], n_hidden=L['H'], W_init=d['W'], batch_size=L['batch'], l2=L['l2'], random_seed=L['seed'], verbose=False)
    m.set_classes(L['C'], U=d['U'])
    assert m.make_random_seed() == K.learning_seed()      # the seed fit_semi_supervised hands the engine


# ---- 5. the host surface
def _model(cls=None, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    return (cls or BernoulliRBM)(n_visible=6, n_hidden=4, batch_size=5, random_seed=1337, verbose=False, **kw)


def test_fit_semi_supervised_refusals(monkeypatch):
    from boltzmann_machines_amd import GaussianRBM, MultinomialRBM
    X, y, Xu = np.zeros((4, 6), np.float32), np.zeros(4, int), np.zeros((7, 6), np.float32)
    with pytest.raises(ValueError, match='no class head'):
        _model().fit_semi_supervised(X, y, Xu)
    for cls, kw, match in ((GaussianRBM, {}, 'Gaussian'), (MultinomialRBM, {}, 'Multinomial'), (None, dict(dtype='float64'), 'float32'),
                           (None, dict(dbm_first=True), 'dbm_first')):
        m = _model(cls, **kw)
        m._class_head = dict(C=3, pending=None)          # (set_classes itself refuses these models)
        with pytest.raises(ValueError, match=match):
            m.fit_semi_supervised(X, y, Xu)
    with pytest.raises(ValueError, match='dropout'):
        _model(dropout=0.8).set_classes(3).fit_semi_supervised(X, y, Xu)
    with pytest.raises(ValueError, match='sparsity'):
        _model(sparsity_cost=0.1).set_classes(3).fit_semi_supervised(X, y, Xu)
    with pytest.raises(ValueError, match='centering'):
        _model().set_centering(True).set_classes(3).fit_semi_supervised(X, y, Xu)
    m = _model().set_classes(3)
    for bad, match in (([0, 1, 2, 3], 'outside'), ([0, -1, 2, 1], 'outside'), ([0, 1, 2], 'labels for 4 rows'), (np.zeros(4), 'integer')):
        with pytest.raises(ValueError, match=match):
            m.fit_semi_supervised(X, np.array(bad), Xu)
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError, match='n_gibbs_steps'):
            m.fit_semi_supervised(X, y, Xu, n_gibbs_steps=k)
    for g in (-0.5, float('nan')):
        with pytest.raises(ValueError, match='discriminative_weight'):
            m.fit_semi_supervised(X, y, Xu, discriminative_weight=g)
        with pytest.raises(ValueError, match='unlabelled_weight'):
            m.fit_semi_supervised(X, y, Xu, unlabelled_weight=g)
    with pytest.raises(ValueError, match='`X_unlabelled` has invalid shape'):
        m.fit_semi_supervised(X, y, np.zeros((7, 5), np.float32))
    with pytest.raises(ValueError, match='`X_unlabelled` has no rows'):
        m.fit_semi_supervised(X, y, np.zeros((0, 6), np.float32))
    with pytest.raises(ValueError, match='batch_size'):
        m.fit_semi_supervised(X, y, Xu, batch_size=6)
    with pytest.raises(ValueError, match='go together'):
        m.fit_semi_supervised(X, y, Xu, X_val=X)
    assert m._engine is None                             # nothing was built or uploaded
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(ValueError, match='data parallelism'):
        _model().set_classes(3).fit_semi_supervised(X, y, Xu)


def test_signature_defaults():
    from boltzmann_machines_amd import BernoulliRBM
    s = inspect.signature(BernoulliRBM.fit_semi_supervised)
    assert list(s.parameters) == ['self', 'X', 'y', 'X_unlabelled', 'X_val', 'y_val', 'n_epochs', 'n_gibbs_steps', 'learning_rate', 'momentum',
                                  'discriminative_weight', 'unlabelled_weight', 'batch_size', 'verbose']
    j = inspect.signature(BernoulliRBM.fit_joint)
    for n in ('X_val', 'y_val', 'n_epochs', 'n_gibbs_steps', 'learning_rate', 'momentum', 'discriminative_weight', 'batch_size', 'verbose'):
        assert s.parameters[n].default == j.parameters[n].default, n
    assert s.parameters['unlabelled_weight'].default == 1.0


def test_abi_surface():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'bm355.h')).read()
    for decl in ('int bm_rbm_class_unsup_train_step(bm_rbm *h, const float *X_dev, int32_t B, int32_t n_gibbs_steps, float learning_rate, float momentum,',
                 'int bm_rbm_class_unsup_chain(bm_rbm *h, const float *X_dev, int32_t B, int32_t n_gibbs_steps, int32_t *y0_host, float *em_host,',
                 'int bm_rbm_class_semi_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [N] */, int64_t N,'):
        assert decl in header, decl
    names = ('bm_rbm_class_unsup_train_step', 'bm_rbm_class_unsup_chain', 'bm_rbm_class_semi_train_epoch')
    assert [len(_ffi.SIGNATURES[n]) for n in names] == [7, 10, 14]
    lib = _ffi.load()
    for n in names:
        assert hasattr(lib, n), n
    for name in ('class_unsup_train_step', 'class_unsup_chain', 'class_semi_train_epoch'):
        assert callable(getattr(RbmEngine, name)) and not hasattr(RbmEngine64, name)
    src = open(os.path.join(os.path.dirname(__file__), '..', 'boltzmann_machines_amd', 'csrc', 'bm_rbm.hip')).read()
    assert 'SITE_CLASS_Y0 = %d' % T.SITE_CLASS_Y0 in src
