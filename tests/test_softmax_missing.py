"""Softmax visible units with incomplete rows, clamped groups and exact group conditionals without a GPU: the
float64 scores against enumeration, the chi-square of the twin's chains against the exact distributions, learning with missing
values on the twin, and the host logic of CategoricalRBM."""
import numpy as np
import pytest

from tests import multinomial_probes as P
from tests import softmax_missing_twin as M
from tests import softmax_v_twin as T

f32 = np.float32
G3 = K3 = 3


def _rows_with_gaps():
    """every one-hot-or-empty row of the 3 x 3 model: 4^3 = 64 rows, the empty row included"""
    cats = np.stack(np.meshgrid(*[np.arange(-1, K3)] * G3, indexing='ij'), axis=-1).reshape(-1, G3)
    X = np.zeros((len(cats), G3, K3), f32)
    for b, row in enumerate(cats):
        for g, k in enumerate(row):
            if k >= 0:
                X[b, g, k] = 1.0
    return cats, X.reshape(len(cats), G3 * K3)


# ---- 1. group_scores64 against enumeration
def test_group_scores_are_the_exact_conditionals():
    """over all 64 rows of the 3 x 3 x 3 model: for an observed group p(v_g | v_-g), for an empty group p(v_g | v_O) with the other
    empty groups removed from the model - both by enumerating every (v_g, h) of the model of the groups involved - to 1e-12"""
    p = T.small_model()
    cats, X = _rows_with_gaps()
    lp = M.group_log_proba64(p, X, K3)
    worst = 0.0
    for b in range(len(X)):
        for g in range(G3):
            ex = M.exact_group_conditional(p, X[b], g, K3)
            worst = max(worst, float(np.abs(lp[b, g] - ex).max()))
    print('largest deviation of a log-probability over %d rows x %d groups: %.3e' % (len(X), G3, worst))
    assert worst <= 1e-12
    assert np.allclose(np.exp(lp).sum(axis=2), 1.0, atol=1e-12)


def test_bound_is_small_and_positive():
    p = T.small_model()
    _, X = _rows_with_gaps()
    S, bound = M.group_scores64(p, X, K3)
    assert S.shape == bound.shape == X.shape and np.all(bound > 0) and bound.max() < 5e-4


# ---- 2. the chains sample the exact distributions
def _chi_square(counts, pv, what):
    n = counts.sum()
    ex = n * pv
    dof = len(pv) - 1
    chi2 = float(((counts - ex) ** 2 / ex).sum())
    z = (chi2 - dof) / np.sqrt(2.0 * dof)
    print('%s: %d states over %d cells, chi2 = %.2f, z = %+.2f, smallest expected cell %.1f' % (what, n, len(pv), chi2, z, ex.min()))
    assert ex.min() >= 5.0
    assert abs(z) <= P.Z_CAP


def _run_chain(p, x, free, seed, h_seed):
    """512 twin chains of the clamped sweep from the row x (its `free` groups drawn, every other group held - at its category, or
    at zero when it is empty), 400 steps, every 10th state after step 100 -> counts over the K^len(free) cells"""
    B = 512
    X = np.tile(np.asarray(x, f32), (B, 1))
    flags = np.ones((B, G3))
    flags[:, free] = 0
    mask = M.group_mask(flags, K3)
    rng = np.random.RandomState(h_seed)
    V0 = X.copy()
    for g in free:
        V0[:, g * K3:(g + 1) * K3] = T.one_hot(rng.randint(0, K3, (B, 1)), K3)
    counts = np.zeros(K3 ** len(free))
    weights = K3 ** np.arange(len(free) - 1, -1, -1)

    def keep(t, v):
        if t >= 100 and t % 10 == 0:
            c = v.reshape(B, G3, K3)
            assert np.all(c[:, free].sum(axis=2) == 1)
            assert np.array_equal(v * mask, X * mask)                 # the held groups never move
            np.add.at(counts, c[:, free].argmax(axis=2).dot(weights), 1)
    M.groups_gibbs_clamped(p, K3, V0, X, mask, 400, seed, keep=keep)
    assert counts.sum() == 15360
    return counts


def test_chain_with_an_empty_group_samples_the_marginal_model():
    """group 1 empty - held at zero, as the training chain holds a missing group: the chain over groups 0 and 2 samples the exact
    p(v_0, v_2) of the model without group 1 (9 cells).  Seeds fixed here before any GPU run."""
    p = T.small_model()
    x = np.zeros(G3 * K3, f32)
    pv = M.exact_joint(p, x, [0, 2], K3)
    sub = M.submodel(p, [0, 2], K3)                                   # the same distribution from the model that lacks the group
    _, X2 = T.all_visible_states(2, K3)
    pv2 = np.exp(-T.free_energy64(sub, X2) - T.log_z_visible(sub, 2, K3))
    assert np.abs(pv - pv2).max() < 1e-12
    _chi_square(_run_chain(p, x, [0, 2], seed=4242, h_seed=6), pv, 'one group empty')


def test_clamped_chain_samples_the_exact_conditional():
    """group 0 observed at category 2, groups 1 and 2 free: the clamped chain samples the exact p(v_1, v_2 | v_0 = 2) (9 cells).
    Seeds fixed here before any GPU run."""
    p = T.small_model()
    x = np.zeros(G3 * K3, f32)
    x[2] = 1.0
    pv = M.exact_joint(p, x, [1, 2], K3)
    _, X = T.all_visible_states(G3, K3)                               # ... the same from the full joint
    joint = np.exp(-T.free_energy64(p, X)).reshape(K3, K3 * K3)[2]
    assert np.abs(pv - joint / joint.sum()).max() < 1e-12
    _chi_square(_run_chain(p, x, [1, 2], seed=2424, h_seed=7), pv, 'one group observed')


# ---- 3. a free group gets the unclamped pass's bits; an all-zero mask is the unclamped sweep
def test_clamp_leaves_free_groups_their_bits():
    K, G, H, B = 4, 5, 6, 9
    rng = np.random.RandomState(1)
    p = dict(W=(0.5 * rng.randn(G * K, H)).astype(f32), vb=(0.3 * rng.randn(G * K)).astype(f32), hb=(0.3 * rng.randn(H)).astype(f32))
    h = (rng.uniform(size=(B, H)) < 0.5).astype(f32)
    clamp = T.one_hot(rng.randint(0, K, (B, G)), K)
    mask = M.group_mask(rng.uniform(size=(B, G)) < 0.5, K)
    m0, s0 = T.visible_pass(h, p['W'], p['vb'], K, 1, 5, T.SITE_V, 0, 0)
    m1, s1 = M.clamped_visible_pass(h, p['W'], p['vb'], K, 1, 5, T.SITE_V, 0, 0, clamp, mask)
    free = mask == 0
    P.assert_bits(m1[free], m0[free], 'means of the free groups')
    P.assert_bits(s1[free], s0[free], 'states of the free groups')
    P.assert_bits(m1[~free], clamp[~free], 'means of the clamped groups')
    V0 = T.one_hot(rng.randint(0, K, (B, G)), K)
    v, hh, vm = M.groups_gibbs_clamped(p, K, V0, clamp, np.zeros_like(mask), 2, 5)
    twin = T.SoftmaxVRBM(p, K, 5, sample_v_states=True)
    _, h1 = twin._up(V0, 1, T.SITE_H)
    _, v1 = twin._down(h1, 1, T.SITE_V)
    _, h2 = twin._up(v1, 1, T.SITE_H + 16)
    m2, v2 = twin._down(h2, 1, T.SITE_V + 16)
    P.assert_bits(v, v2, 'all-zero mask: states')
    P.assert_bits(vm, m2, 'all-zero mask: means')
    P.assert_bits(hh, h2, 'all-zero mask: hidden states')


def test_missing_mode_on_complete_rows_is_the_plain_twin():
    K, G, H, B = 3, 4, 5, 10
    rng = np.random.RandomState(2)
    p = dict(W=(0.1 * rng.randn(G * K, H)).astype(f32), vb=np.zeros(G * K, f32), hb=np.zeros(H, f32))
    X = T.one_hot(rng.randint(0, K, (B, G)), K)
    a, b = T.SoftmaxVRBM(p, K, 3, sample_v_states=True), M.MissingRBM(p, K, 3, sample_v_states=True)
    for _ in range(2):
        a.train_step(X, 0.05, 0.9, 2)
        b.train_step(X, 0.05, 0.9, 2)
    for n in ('W', 'vb', 'hb', 'dW'):
        P.assert_bits(a.p[n], b.p[n], n)
    Xm, gone = M.remove_groups(X, K, 0.3, 4)
    ch = b.chain(Xm, 2)
    assert gone.any() and np.all(ch['vs'][M.group_mask(gone, K) != 0] == 0) and np.all(ch['vm'][M.group_mask(gone, K) != 0] == 0)
    assert np.all(ch['vs'].reshape(B, G, K).sum(axis=2)[~gone] == 1)


# ---- 4. learning with missing values on the twin
MISSING = dict(G=4, K=3, H=8, n_train=200, n_val=100, batch=20, lr=0.1, mom=0.5, epochs=60, seed=42, frac=0.3)


def missing_twin(seed=None, epochs=None):
    """the twin after CD-1 on the planted rows of tests/test_softmax_v.py with 30 % of the groups removed -> (twin, X, p0)"""
    c = MISSING
    X, _ = M.remove_groups(T.one_hot(T.planted_data(c['n_train'], 1, c['G'], c['K']), c['K']), c['K'], c['frac'], 21)
    rng = np.random.RandomState(3)
    p0 = dict(W=(0.01 * rng.randn(c['G'] * c['K'], c['H'])).astype(f32), vb=np.zeros(c['G'] * c['K'], f32), hb=np.zeros(c['H'], f32))
    twin = M.MissingRBM(p0, c['K'], seed=c['seed'] if seed is None else seed, l2=1e-4)
    for _ in range(c['epochs'] if epochs is None else epochs):
        twin.train_epoch(X, c['batch'], c['lr'], c['mom'], 1)
    return twin, X, p0


def heldout_cells():
    """100 held-out planted rows with 30 % of their groups removed -> (X with gaps, removed [N][G], true categories [N][G])"""
    c = MISSING
    Cval = T.planted_data(c['n_val'], 2, c['G'], c['K'])
    Xg, gone = M.remove_groups(T.one_hot(Cval, c['K']), c['K'], c['frac'], 22)
    return Xg, gone, Cval


def test_twin_learns_with_missing_values():
    """4 groups of 3 that copy one latent category with 10 % noise, 200 rows with 30 % of the groups removed, CD-1, 60 epochs at
    12 x 8 with the missing-value mode on.  On 100 held-out rows with 30 % of their groups removed (116 cells; rows left without
    any observed group are not counted: nothing predicts them) the exact prediction of the removed cells is right in 0.793 of
    the cells, the majority category of the training data's observed cells in 0.336 (measured on the twin; 0.560 after 30
    epochs, 0.810 after 100).  Asserted: the prediction beats the baseline, and observed cells keep their category."""
    c = MISSING
    twin, X, _ = missing_twin()
    Xg, gone, Cval = heldout_cells()
    counted = gone & M.observed_groups(Xg, c['K']).any(axis=1)[:, None]
    pred = M.predict64(twin.p, Xg, c['K'])
    acc = float((pred == Cval)[counted].mean())
    seen = M.observed_groups(X, c['K'])
    majority = np.array([np.bincount(X.reshape(len(X), c['G'], c['K']).argmax(axis=2)[seen[:, g], g], minlength=c['K']).argmax()
                         for g in range(c['G'])])
    base = float((majority[None, :] == Cval)[counted].mean())
    print('accuracy on %d removed cells: prediction %.3f, majority category %.3f' % (counted.sum(), acc, base))
    assert acc > base
    assert np.array_equal(pred[~gone], Cval[~gone])


# ---- 5. host logic of the public class
def test_entries_exist():
    import boltzmann_machines_amd as bm
    from boltzmann_machines_amd import _ffi
    for name in ('bm_rbm_groups_set_missing', 'bm_rbm_groups_gibbs_clamped', 'bm_rbm_groups_scores'):
        assert name in _ffi.SIGNATURES
    for name in ('group_log_proba', 'predict_proba', 'predict', 'pseudo_log_likelihood', 'sample_groups_given'):
        assert callable(getattr(bm.CategoricalRBM, name))
    m = bm.CategoricalRBM(5, 3, 4)
    assert m.missing_values is False and m.get_params()['missing_values'] is False
    assert bm.CategoricalRBM(5, 3, 4, missing_values=True).get_params()['missing_values'] is True


def test_encode_decode_with_missing():
    import boltzmann_machines_amd as bm
    m = bm.CategoricalRBM(4, 3, 2)
    C_ = np.random.RandomState(0).randint(0, 3, (11, 4))
    Cm = C_.copy()
    Cm[0, 1] = Cm[3, 0] = Cm[3, 3] = -1
    Cm[5] = -1
    X = m.encode(Cm, missing=-1)
    assert X.dtype == np.float32 and X.shape == (11, 12)
    X3 = X.reshape(11, 4, 3)
    assert np.array_equal(X3.sum(axis=2), (Cm >= 0).astype(f32))
    assert np.array_equal(X3.argmax(axis=2)[Cm >= 0], Cm[Cm >= 0])
    assert np.array_equal(m.decode(X, missing=-1), Cm)
    assert np.array_equal(m.decode(X, missing=7)[Cm < 0], np.full((Cm < 0).sum(), 7))
    assert np.array_equal(m.decode(X)[Cm >= 0], Cm[Cm >= 0])               # without `missing`: today's argmax (0 for an empty group)
    assert np.all(m.decode(X)[Cm < 0] == 0)
    assert np.array_equal(m.encode(C_, missing=-1), m.encode(C_)) and np.array_equal(m.encode(C_), T.one_hot(C_, 3))
    with pytest.raises(ValueError):                                        # the default still refuses -1 ...
        m.encode(Cm)
    with pytest.raises(ValueError):                                        # ... and another marker does not admit it
        m.encode(Cm, missing=9)
    for bad in (np.full((2, 4), 3), np.full((2, 4), 0.5), np.zeros((2, 3), int)):
        with pytest.raises(ValueError):
            m.encode(bad, missing=-1)


def test_row_validation(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    from tests.test_softmax_v import _no_engine
    _no_engine(monkeypatch)
    m = bm.CategoricalRBM(3, 2, 4, batch_size=4, missing_values=True, model_path=str(tmp_path) + '/m/')
    good = np.array([[1, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0]], f32)
    X, obs = m._groups_of(good, 'fit')
    assert np.array_equal(obs, [[True, False, True], [False, False, False]])
    for bad in ([[1, 1, 0, 0, 0, 1]], [[0.5, 0, 0, 0, 0, 1]], [[2, 0, 0, 0, 0, 0]], [[1, 0, 0, 0, 0]]):
        with pytest.raises(ValueError):
            m._groups_of(np.array(bad, f32), 'fit')
        with pytest.raises(ValueError):
            m.fit(np.array(bad, f32))
        with pytest.raises(ValueError):
            m.fit(good, np.array(bad, f32))
    assert m._engine is None


def test_params_json_carries_missing_values(tmp_path):
    """the checkpoint's params.json as _save_model writes it (get_params, serialised, with the class name), written here by
    hand - saving needs an engine - and read back by load_model; tests/test_softmax_missing_gpu.py makes the real round trip"""
    import json
    import os
    import boltzmann_machines_amd as bm
    for flag in (True, False):
        path = str(tmp_path) + '/m%d/' % flag
        m = bm.CategoricalRBM(3, 2, 4, batch_size=4, missing_values=flag, model_path=path, random_seed=1, verbose=False)
        params = m._serialize(dict(m.get_params(deep=False)))
        assert params['missing_values'] is flag
        params['__class_name__'] = 'CategoricalRBM'
        os.makedirs(path)
        with open(m._params_filepath, 'w') as f:
            json.dump(params, f)
        np.savez(m._model_filepath + '.npz', W=np.zeros((6, 4), f32))
        loaded = bm.CategoricalRBM.load_model(path)
        assert loaded.missing_values is flag and (loaded.n_groups, loaded.n_categories, loaded.n_visible) == (3, 2, 6)


def test_old_refusals_still_raise(monkeypatch, tmp_path):
    import boltzmann_machines_amd as bm
    from tests.test_softmax_v import _no_engine, _refused
    _no_engine(monkeypatch)
    kw = dict(n_groups=3, n_categories=2, n_hidden=4, batch_size=4, missing_values=True, model_path=str(tmp_path) + '/m/')
    X = np.tile(np.array([1, 0], f32), (8, 3))
    m = bm.CategoricalRBM(**kw)
    _refused(lambda: m.sample_v_given(X, np.ones(6)), 'sample_v_given')
    _refused(lambda: m.log_Z(), 'log_Z')
    _refused(lambda: bm.CategoricalRBM(**dict(kw, metrics_config=dict(pll=True))), '__init__')
    m.metrics_config['pll'] = True
    _refused(lambda: m.fit(X), 'fit')
    assert m._engine is None
