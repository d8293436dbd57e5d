"""Noisy rectified-linear hidden units (BM_UNIT_NRELU) without a GPU: the CPU twin (tests/nrelu_twin.py) against a
float64 restatement and against the unit's moments, its draws by position, learning on the twin, and what the Python classes
refuse before the engine is touched."""
import math

import numpy as np
import pytest

from oracle import oracle as orc
from tests import nrelu_twin as T

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def _params(V, H, seed, scale):
    rng = np.random.RandomState(seed)
    return dict(W=(rng.randn(V, H) * scale).astype(f32), hb=rng.uniform(-1, 1, H).astype(f32), vb=np.zeros(V, f32))


def _span_case():
    """random weights and inputs whose t spans [-30, 30]"""
    V, H, J = 24, 40, 64
    p = _params(V, H, 0, 4.0)
    X = (np.random.RandomState(1).uniform(0, 1, (J, V)) < 0.5).astype(f32)
    return p, X


# ---- 1. the twin against an independent float64 restatement
# (the seed is chosen so that the float64 restatement alone keeps the band |u| <= 1e-5 below 0.1 % of the elements: checked here)
SEED_64 = 11


def test_twin_against_float64():
    p, X = _span_case()
    J, H = len(X), p['W'].shape[1]
    t = T.pre_activation(X, p['W'], p['hb'])
    assert t.min() < -30 and t.max() > 30, (t.min(), t.max())
    m, s = T.hidden_pass(X, p['W'], p['hb'], 1, SEED_64, T.SITE_H0, 0, 0)
    n = T.normals(SEED_64, T.SITE_H0, 0, 0, J, H)
    t64, n64 = t.astype(np.float64), n.astype(np.float64)
    u64 = t64 + np.sqrt(1.0 / (1.0 + np.exp(-t64))) * n64
    s64 = np.maximum(0.0, u64)
    assert np.array_equal(m.astype(np.float64), np.maximum(0.0, t64))                      # means: equal
    band = np.abs(u64) <= 1e-5
    assert band.mean() <= 1e-3, band.mean()                                                # the restatement alone
    tol = 4 * EPS32 * np.maximum(1.0, np.abs(t64) + np.abs(n64))
    assert np.all(np.abs(s.astype(np.float64) - s64) <= tol), float(np.max(np.abs(s - s64) / tol))
    assert np.array_equal((s > 0)[~band], (s64 > 0)[~band])                                # kept / zeroed decision
    # a pass that does not sample stores the mean as the state; -0 and t <= 0 give +0
    m0, s0 = T.hidden_pass(X, p['W'], p['hb'], 0, SEED_64, T.SITE_H0, 0, 0)
    assert np.array_equal(m0.view(np.uint32), s0.view(np.uint32)) and np.array_equal(m0.view(np.uint32), m.view(np.uint32))
    z = T.rectify(f32([-0.0, 0.0, -1.0, np.nan, 2.0]))
    assert np.array_equal(z.view(np.uint32), f32([0.0, 0.0, 0.0, 0.0, 2.0]).view(np.uint32))


# ---- 2. moments of the rectified Gaussian
def _phi(x):
    return math.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _Phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize('t', [-2.0, 0.0, 0.5, 3.0])
def test_moments(t):
    N = 2 ** 18
    n = orc.normal(2024, T.SITE_H0, 0, N)
    s, _ = T.state_from(np.full(N, t, f32), n)
    mu, sd = t, math.sqrt(1.0 / (1.0 + math.exp(-t)))
    a = mu / sd
    mean = mu * _Phi(a) + sd * _phi(a)
    second = (mu * mu + sd * sd) * _Phi(a) + mu * sd * _phi(a)
    se = math.sqrt((second - mean * mean) / N)
    got = float(s.astype(np.float64).mean())
    print('t = %g: sample mean %.6f, rectified-Gaussian mean %.6f, standard error %.2e' % (t, got, mean, se))
    assert abs(got - mean) <= 5 * se, (t, got, mean, se)


# ---- 3. draws by position
def test_draws_by_position():
    p, X = _span_case()
    full_m, full_s = T.hidden_pass(X, p['W'], p['hb'], 1, 5, T.SITE_H, 3, 0)
    r, n = 17, 9
    part_m, part_s = T.hidden_pass(X[r:r + n], p['W'], p['hb'], 1, 5, T.SITE_H, 3, r)
    assert np.array_equal(part_s.view(np.uint32), full_s[r:r + n].view(np.uint32))
    assert np.array_equal(part_m.view(np.uint32), full_m[r:r + n].view(np.uint32))
    # a ragged I (I % 4 != 0) uses the draws of the flat stream
    I = 23
    q = dict(W=p['W'][:, :I].copy(), hb=p['hb'][:I].copy())
    t = T.pre_activation(X, q['W'], q['hb'])
    _, s = T.hidden_pass(X, q['W'], q['hb'], 1, 5, T.SITE_H, 3, 4)
    flat = orc.normal(5, T.SITE_H, 3, (4 + len(X)) * I)[4 * I:].reshape(len(X), I)
    want, _ = T.state_from(t, flat)
    assert np.array_equal(s.view(np.uint32), want.view(np.uint32))


# ---- 4. / 5. the Python classes: they exist, and every refusal is a ValueError before any engine call
def test_classes_exist():
    import boltzmann_machines_amd as bm
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.rbm import BaseRBM, GaussianRBM
    assert _ffi.UNIT_NRELU == 3
    assert issubclass(bm.ReLURBM, BaseRBM) and issubclass(bm.GaussianReLURBM, GaussianRBM)
    assert bm.ReLURBM._H_UNIT == _ffi.UNIT_NRELU and bm.GaussianReLURBM._H_UNIT == _ffi.UNIT_NRELU
    assert bm.ReLURBM._V_UNIT == _ffi.UNIT_BERNOULLI and bm.GaussianReLURBM._V_UNIT == _ffi.UNIT_GAUSSIAN
    assert callable(BaseRBM.sample_h) and 'bm_rbm_sample_h' in _ffi.SIGNATURES
    r, g = bm.ReLURBM(n_visible=6, n_hidden=4), bm.GaussianReLURBM(n_visible=6, n_hidden=4)
    assert r._model_dirpath.endswith('relu_rbm_model/') and g._model_dirpath.endswith('g_relu_rbm_model/')
    assert g.learning_rate == [1e-4] and r._engine is None and g._engine is None


def _no_engine(monkeypatch):
    """any attempt to build an engine fails the test"""
    from boltzmann_machines_amd import rbm as rbm_mod

    def boom(*a, **k):
        raise AssertionError('an engine call was made')
    monkeypatch.setattr(rbm_mod, 'RbmEngine', boom)
    monkeypatch.setattr(rbm_mod, 'RbmEngine64', boom)


def _refused(f, method):
    with pytest.raises(ValueError) as e:
        f()
    msg = str(e.value)
    assert 'NReLU' in msg and method in msg, msg


@pytest.mark.parametrize('cls_name', ['ReLURBM', 'GaussianReLURBM'])
def test_python_refusals(cls_name, monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    _no_engine(monkeypatch)
    cls = getattr(bm, cls_name)
    kw = dict(n_visible=6, n_hidden=4, batch_size=4, model_path=str(tmp_path) + '/m/')
    X = np.zeros((8, 6), f32)
    for bad in (dict(metrics_config=dict(pll=True)), dict(metrics_config=dict(feg=True)), dict(sparsity_cost=0.1), dict(dropout=0.8),
                dict(dbm_first=True), dict(dbm_last=True), dict(dtype='float64')):
        _refused(lambda: cls(**dict(kw, **bad)), '__init__')
    # ... and when set_params brings one of them in later: before the engine is built
    for name, value in (('sparsity_cost', 0.1), ('dropout', 0.5), ('dbm_first', True), ('dtype', 'float64')):
        m = cls(**kw)
        m.set_params(**{name: value})
        _refused(lambda: m.fit(X), 'fit')
    m = cls(**kw)
    m.metrics_config['pll'] = True
    _refused(lambda: m.fit(X), 'fit')
    m = cls(**kw)
    _refused(lambda: m.set_negative_phase('tempered'), 'set_negative_phase')
    assert m.set_negative_phase('cd') is m
    _refused(lambda: m.set_centering(), 'set_centering')
    _refused(lambda: m.set_classes(3), 'set_classes')
    _refused(lambda: m.sample_v(4), 'sample_v')
    _refused(lambda: m.sample_v_given(X, np.ones(6)), 'sample_v_given')
    _refused(lambda: m.log_Z(), 'log_Z')
    _refused(lambda: m.log_proba(X, 0.0), 'log_proba')
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    _refused(lambda: m.fit(X), 'fit')
    monkeypatch.delenv('BM355_DATA_PARALLEL')
    assert m._engine is None


def test_python_refusals_as_a_layer(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    _no_engine(monkeypatch)
    kw = dict(n_visible=6, n_hidden=4, batch_size=4, model_path=str(tmp_path) + '/m/')
    relu = bm.ReLURBM(**kw)
    _refused(lambda: bm.DBM(rbms=[relu], model_path=str(tmp_path) + '/d/'), 'DBM')
    _refused(lambda: bm.StackClassifier.from_rbms([relu], n_classes=3, model_path=str(tmp_path) + '/s/'), 'from_rbms')

    class FakeDBM(object):
        v_unit_, h_units_, dtype = 0, [0, 3], 'float32'
    _refused(lambda: bm.StackClassifier.from_dbm(FakeDBM(), n_classes=3), 'from_dbm')
    assert relu._engine is None


# ---- 6. learning on the twin
def _two_clusters():
    rng = np.random.RandomState(7)
    proto = np.zeros((2, 16), f32)
    proto[0, :8], proto[1, 8:] = 1, 1
    X = proto[rng.randint(0, 2, 64)]
    flip = rng.uniform(size=X.shape) < 0.05
    return np.where(flip, 1 - X, X).astype(f32)


def test_twin_learns():
    """CD-1 on 64 rows of a two-cluster set at 16 x 12, batch 16, lr 0.05, momentum 0.5: the msre of the chain from the whole
    set after every epoch.  Measured on the twin: 0.2498 after the first epoch, 0.0427 after the 30th; the assertion is the
    ordering only."""
    X = _two_clusters()
    rng = np.random.RandomState(3)
    p0 = dict(W=(rng.randn(16, 12) * 0.01).astype(f32), vb=np.zeros(16, f32), hb=np.zeros(12, f32))
    twin = T.NReLURBM(p0, seed=42, l2=1e-4)
    msre = []
    for epoch in range(30):
        twin.train_epoch(X, 16, 0.05, 0.5, 1)
        msre.append(twin.metrics(X, 1)[0])
    print('msre of epoch 1: %.4f, of epoch 30: %.4f' % (msre[0], msre[-1]))
    assert np.all(np.isfinite(list(twin.state().values())[0]))
    assert msre[-1] < msre[0], (msre[0], msre[-1])
