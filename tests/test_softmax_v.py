"""Softmax (categorical) visible units without a GPU: the CPU twin (tests/softmax_v_twin.py) against a float64
softmax and against the model's exact distribution, its draws by position, learning on the twin, and what the Python classes
refuse.  tests/test_softmax_v_gpu.py holds the engine to the same twin bit for bit."""
import numpy as np
import pytest

from tests import multinomial_probes as P
from tests import softmax_v_twin as T

f32 = np.float32
WIDTHS = (2, 3, 4, 5, 8, 10, 16, 26)
SEED = 20241


# ---- 1. the twin against a float64 softmax
@pytest.mark.parametrize('K', WIDTHS)
def test_twin_against_float64_softmax(K):
    """Every logit family of tests/multinomial_probes.logit_sets at width K, three groups per row (so that the groups' uniforms
    are read at stride K), 64 rows: the means inside the module's derived bound ((K - 1) + d) 2^-24 + 1e-6 for d <= 80 and
    1.81e-35 beyond the clamp; every group of the states one-hot; a unit with c[k] == c[k-1] never drawn; the hot unit of family
    d takes every draw."""
    G, J = 3, 64
    for name, l in P.logit_sets(K):
        L = np.tile(l, (J, G)).astype(f32)
        u = T.group_uniforms(SEED, T.SITE_V, 0, 0, J, G * K, K)
        m, s = T.softmax_groups(L, K, 1, u)
        what = 'twin %s K=%d' % (name, K)
        P.check_means(l, m.reshape(J * G, K), 1, P.F32, what)
        s3 = s.reshape(J * G, K)
        assert np.all((s3 == 0) | (s3 == 1)) and np.all(s3.sum(axis=1) == 1), what
        P.check_counts(l, s3, 1, P.F32, name, what)             # (dead units, the hot unit of family d)
        m0, s0 = T.softmax_groups(L, K, 0)
        P.assert_bits(m0, m, what)
        P.assert_bits(s0, m, what + ' (no draw: states = means)')


# ---- 2. the conditional is the model's
def test_log_z_two_ways():
    p = T.small_model()
    a, b = T.log_z_visible(p, 3, 3), T.log_z_hidden(p, 3, 3)
    print('log Z over the 27 visible states %.12f, over the 8 hidden states %.12f' % (a, b))
    assert abs(a - b) <= 1e-9


def test_gibbs_chain_samples_the_model():
    """G = K = H = 3: 512 twin chains, 400 block-Gibbs steps, every 10th state after step 100 - 15 360 states over 27 cells -
    against the exact p(v): z = (chi2 - 26) / sqrt(52), |z| <= 4 (the project's cap).  Seeds fixed here before any GPU run."""
    G = K = 3
    p = T.small_model()
    cats, X = T.all_visible_states(G, K)
    pv = np.exp(-T.free_energy64(p, X) - T.log_z_visible(p, G, K))
    assert abs(pv.sum() - 1.0) < 1e-12
    twin = T.SoftmaxVRBM(p, K, seed=777, sample_v_states=True, sample_h_states=True)
    counts = np.zeros(K ** G)
    weights = K ** np.arange(G - 1, -1, -1)

    def keep(t, v):
        if t >= 100 and t % 10 == 0:
            c = v.reshape(len(v), G, K)
            assert np.all(c.sum(axis=2) == 1)
            np.add.at(counts, c.argmax(axis=2).dot(weights), 1)
    H0 = (np.random.RandomState(5).uniform(size=(512, 3)) < 0.5).astype(f32)
    twin.gibbs(H0, 400, keep=keep)
    n = counts.sum()
    assert n == 15360
    ex = n * pv
    chi2 = float(((counts - ex) ** 2 / ex).sum())
    z = (chi2 - 26) / np.sqrt(52.0)
    print('chi-square of %d states over 27 cells: chi2 = %.2f, z = %+.2f, smallest expected cell %.1f' % (n, chi2, z, ex.min()))
    assert ex.min() >= 5.0
    assert abs(z) <= P.Z_CAP


# ---- 3. draws by position
@pytest.mark.parametrize('K,G', [(4, 5), (5, 3)])
def test_draws_by_position(K, G):
    rng = np.random.RandomState(K)
    V, H = G * K, 6
    W, vb = (0.5 * rng.randn(V, H)).astype(f32), (0.5 * rng.randn(V)).astype(f32)
    h = (rng.uniform(size=(20, H)) < 0.5).astype(f32)
    m, s = T.visible_pass(h, W, vb, K, 1, SEED, T.SITE_V, 3, row0=0)
    m7, s7 = T.visible_pass(h[5:12], W, vb, K, 1, SEED, T.SITE_V, 3, row0=5)
    P.assert_bits(m7, m[5:12], 'means')
    P.assert_bits(s7, s[5:12], 'states')
    assert np.all(s.reshape(20, G, K).sum(axis=2) == 1)


# ---- 4. learning on the twin
PLANTED = dict(G=4, K=3, H=8, n_train=200, n_val=100, batch=20, lr=0.1, mom=0.5, epochs=30, seed=42)


def planted_twin(seed=None):
    """the model of this test after its 30 epochs (tests/test_softmax_v_gpu.py trains CategoricalRBM on the same rows, under the
    seed its fit() draws) -> (twin, X, initial parameters)"""
    c = dict(PLANTED, seed=PLANTED['seed'] if seed is None else seed)
    Ctr = T.planted_data(c['n_train'], 1, c['G'], c['K'])
    X = T.one_hot(Ctr, c['K'])
    rng = np.random.RandomState(3)
    p0 = dict(W=(0.01 * rng.randn(c['G'] * c['K'], c['H'])).astype(f32), vb=np.zeros(c['G'] * c['K'], f32), hb=np.zeros(c['H'], f32))
    twin = T.SoftmaxVRBM(p0, c['K'], seed=c['seed'], l2=1e-4)
    for _ in range(c['epochs']):
        twin.train_epoch(X, c['batch'], c['lr'], c['mom'], 1)
    return twin, X, p0


def test_twin_learns_planted_groups():
    """4 groups of 3 whose categories copy one latent category with 10 % noise, 200 rows, CD-1, 30 epochs at 12 x 8, batch 20,
    lr 0.1, momentum 0.5.  Measured on the twin: mean free energy of 100 held-out rows -9.051, of the same rows with
    independently shuffled groups -6.295 (the assertion asks for a gap of 1.0: a model that learnt the marginals alone leaves none);
    the group-wise marginals of 2000 Gibbs samples (2000 chains, 50 steps from uniform categories) within 0.0420 of the
    data's (asserted: 0.05, the issue's figure)."""
    c = PLANTED
    G, K = c['G'], c['K']
    twin, X, _ = planted_twin()
    Cval = T.planted_data(c['n_val'], 2, G, K)
    fe_val = float(T.free_energy64(twin.p, T.one_hot(Cval, K)).mean())
    fe_shuf = float(T.free_energy64(twin.p, T.one_hot(T.shuffled_groups(Cval, 9), K)).mean())
    print('mean free energy: held-out %.3f, shuffled groups %.3f' % (fe_val, fe_shuf))
    assert fe_val < fe_shuf - 1.0
    sampler = T.SoftmaxVRBM(twin.state(), K, seed=99, sample_v_states=True, sample_h_states=True)
    V0 = T.one_hot(np.random.RandomState(8).randint(0, K, (2000, G)), K)
    _, h = sampler._up(V0, 1, T.SITE_H0)
    sampler.call += 1
    _, v = sampler.gibbs(h, 50)
    assert np.all(v.reshape(2000, G, K).sum(axis=2) == 1)
    d = np.abs(T.group_marginals(v, G, K) - T.group_marginals(X, G, K)).max()
    print('largest deviation of a group-wise marginal over 2000 samples: %.4f' % d)
    assert d <= 0.05


# ---- 5. the Python classes without an engine
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
    assert 'softmax visible units' in msg and method in msg, msg


def test_class_exists():
    import boltzmann_machines_amd as bm
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.rbm import BaseRBM
    assert issubclass(bm.CategoricalRBM, BaseRBM)
    assert bm.CategoricalRBM._V_UNIT == _ffi.UNIT_BERNOULLI and bm.CategoricalRBM._H_UNIT == _ffi.UNIT_BERNOULLI
    assert callable(BaseRBM.sample_v_from_h) and BaseRBM._V_GROUP_WIDTH == 0
    for name in ('bm_rbm_sample_v_from_h', 'bm_rbm_set_visible_groups'):
        assert name in _ffi.SIGNATURES
    m = bm.CategoricalRBM(5, 3, 4)
    assert (m.n_groups, m.n_categories, m.n_visible, m.n_hidden, m._V_GROUP_WIDTH) == (5, 3, 15, 4, 3)
    assert m._model_dirpath.endswith('c_rbm_model/') and m._engine is None
    params = m.get_params()
    assert params['n_groups'] == 5 and params['n_categories'] == 3
    with pytest.raises(ValueError):
        bm.CategoricalRBM(5, 1, 4)
    with pytest.raises(ValueError):
        bm.CategoricalRBM(5, 3, 4, n_visible=16)
    assert bm.CategoricalRBM(5, 3, 4, n_visible=15).n_visible == 15           # (params.json carries all three sizes)


def test_encode_decode():
    import boltzmann_machines_amd as bm
    m = bm.CategoricalRBM(4, 3, 2)
    C_ = np.random.RandomState(0).randint(0, 3, (11, 4))
    X = m.encode(C_)
    assert X.dtype == np.float32 and X.shape == (11, 12)
    assert np.array_equal(X, T.one_hot(C_, 3)) and np.all(X.reshape(11, 4, 3).sum(axis=2) == 1)
    assert np.array_equal(m.decode(X), C_)
    assert np.array_equal(m.decode(X * 0.7 + 0.1), C_)             # (means: the argmax per group)
    assert m.encode(np.zeros((0, 4), int)).shape == (0, 12)
    for bad in (np.full((2, 4), 3), np.full((2, 4), -1), np.full((2, 4), 0.5), np.zeros((2, 3), int), np.zeros(4, int)):
        with pytest.raises(ValueError):
            m.encode(bad)
    with pytest.raises(ValueError):
        m.decode(np.zeros((2, 11)))


def test_python_refusals(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    _no_engine(monkeypatch)
    kw = dict(n_groups=3, n_categories=2, n_hidden=4, batch_size=4, model_path=str(tmp_path) + '/m/')
    X = np.tile(np.array([1, 0], f32), (8, 3))
    for bad in (dict(metrics_config=dict(pll=True)), dict(dropout=0.8), dict(dbm_first=True), dict(dbm_last=True), dict(dtype='float64')):
        _refused(lambda: bm.CategoricalRBM(**dict(kw, **bad)), '__init__')
    for name, value in (('dropout', 0.5), ('dbm_first', True), ('dbm_last', True), ('dtype', 'float64')):
        m = bm.CategoricalRBM(**kw)
        m.set_params(**{name: value})
        _refused(lambda: m.fit(X), 'fit')
    m = bm.CategoricalRBM(**kw)
    m.metrics_config['pll'] = True
    _refused(lambda: m.fit(X), 'fit')
    m = bm.CategoricalRBM(**kw)
    _refused(lambda: m.set_negative_phase('tempered'), 'set_negative_phase')
    assert m.set_negative_phase('cd') is m
    _refused(lambda: m.set_centering(), 'set_centering')
    _refused(lambda: m.set_centering(True), 'set_centering')
    _refused(lambda: m.set_classes(3), 'set_classes')
    _refused(lambda: m.sample_v_given(X, np.ones(6)), 'sample_v_given')
    _refused(lambda: m.log_Z(), 'log_Z')
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    _refused(lambda: m.fit(X), 'fit')
    monkeypatch.delenv('BM355_DATA_PARALLEL')
    assert m._engine is None


def test_python_refusals_as_a_layer(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    _no_engine(monkeypatch)
    cat = bm.CategoricalRBM(3, 2, 4, batch_size=4, model_path=str(tmp_path) + '/m/')
    _refused(lambda: bm.DBM(rbms=[cat], model_path=str(tmp_path) + '/d/'), 'DBM')
    _refused(lambda: bm.StackClassifier.from_rbms([cat], n_classes=3, model_path=str(tmp_path) + '/s/'), 'from_rbms')
    assert cat._engine is None
