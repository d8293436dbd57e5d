"""AIS log Z of softmax visible units without a GPU: the float64 twin (tests/softmax_ais_twin.py) against
enumeration, the zero-near-tie condition on the inputs of the GPU file's chain-by-chain cases, the host logic of
SoftmaxVisible.ais_log_Z / observed_patterns / ais_log_Z_rows, and the C ABI."""
import os
import re

import numpy as np
import pytest

from tests import softmax_ais_twin as st
from tests import softmax_missing_twin as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

GT = (4, 3, 6)                      # groups, categories, hidden units of the enumerated model
GT_PATTERN = np.array([False, True, True, False])


def _gt_params():
    G, K, H = GT
    return st.make_params(G, K, H, std=0.5, seed=7)


@pytest.mark.parametrize('observed', [None, GT_PATTERN], ids=['all', 'pattern'])
@pytest.mark.parametrize('base', [None, 'data'])
def test_twin_brackets_enumeration(observed, base):
    """3000 betas x 256 chains of the twin bracket its own enumerated log Z, by the project's rule |est - exact| < max(0.02, 4 sem)"""
    G, K, H = GT
    P = _gt_params()
    a = st.base_of(base, G, K)
    exact = st.exact_log_Z(P, K, observed)
    values, _ = st.ais(P, K, 3000, 256, 1, 777, 0, a, observed)
    ok, est, sem = st.bracketed(values, exact)
    print('estimate %.6f exact %.6f sem %.4g' % (est, exact, sem))
    assert ok, (est, exact, sem)


def test_submodel_log_Z_is_the_model_without_those_rows():
    """the enumerated log Z of a pattern equals the log Z of the model with the absent groups' rows of W and vb removed"""
    G, K, H = GT
    P = _gt_params()
    for observed in (GT_PATTERN, np.array([True, False, True, True]), np.array([False, False, False, True])):
        sub = mt.submodel(P, list(np.flatnonzero(observed)), K)
        np.testing.assert_allclose(st.exact_log_Z(P, K, observed), st.exact_log_Z(sub, K), rtol=0, atol=1e-12)
    # all observed: the 81 states of the model sum to one
    lp = st.exact_log_p(P, K, st.all_states(G, K))
    np.testing.assert_allclose(np.exp(lp).sum(), 1.0, rtol=0, atol=1e-12)
    # ... and so do the 9 states of the pattern's sub-model, written as incomplete rows of the full width
    X = st.all_states(G, K).reshape(-1, G, K)
    X[:, ~GT_PATTERN, :] = 0
    X = np.unique(X.reshape(len(X), -1), axis=0)
    assert len(X) == K ** int(GT_PATTERN.sum())
    np.testing.assert_allclose(np.exp(st.exact_log_p(P, K, X)).sum(), 1.0, rtol=0, atol=1e-12)


def test_twin_first_score_slices_and_patterns():
    G, K, H = 5, 3, 4
    P = st.make_params(G, K, H, std=0.3)
    a = st.base_of('vector', G, K)
    obs = np.array([True, False, True, True, False])
    # n_betas = 2: one score of v_0 between beta 0 and 1
    from boltzmann_machines_amd.utils import philox
    values, _ = st.ais(P, K, 2, 9, 3, 31, 4, a, obs)
    u = philox.uniform(31, st.SITE_V0, 0, 9 * G * K, idx0=4 * G * K).reshape(9, G, K)[:, :, 0].astype(np.float64)
    a3 = np.asarray(a, np.float64).reshape(G, K)
    c = np.cumsum(np.exp(a3) / np.exp(a3).sum(axis=1, keepdims=True), axis=1)
    cat = (u[:, :, None] >= c[None, :, :]).sum(axis=2)
    v0 = st.one_hot(np.where(obs[None, :], cat, -1), K).astype(np.float64)
    want = -st.free_energy_rows(P, v0) - v0.dot(np.asarray(a, np.float64)) - H * np.log(2.) + st.log_Z0(P, K, a, obs)
    np.testing.assert_allclose(values, want, rtol=0, atol=1e-10)
    # no weights, a = 0: every chain returns H log 2 + |O| log K exactly
    Z = dict(W=np.zeros((G * K, H), f32), vb=np.zeros(G * K, f32), hb=np.zeros(H, f32))
    values, _ = st.ais(Z, K, 7, 5, 1, 1, observed=obs)
    np.testing.assert_allclose(values, H * np.log(2.) + 3 * np.log(K), rtol=0, atol=1e-10)
    # chains [c, c + n) of a larger run are the run of n chains at chain0 = c; an all-True pattern is no pattern
    big, _ = st.ais(P, K, 10, 30, 2, 11, base_bias=a, observed=obs)
    part, _ = st.ais(P, K, 10, 10, 2, 11, chain0=15, base_bias=a, observed=obs)
    assert np.array_equal(big[15:25], part)
    assert np.array_equal(st.ais(P, K, 10, 8, 1, 11)[0], st.ais(P, K, 10, 8, 1, 11, observed=np.ones(G, bool))[0])


@pytest.mark.parametrize('case', st.CHAIN_CASES + st.FULL_CASES, ids=st.case_id)
def test_gpu_chain_cases_meet_no_near_tie(case):
    """the inputs of the GPU file's chain-by-chain comparisons stay inside the comparison: no draw of the twin within 1e-6 of a
    probability or of an interior cumulative probability, so no chain is excluded there"""
    assert case[9] != 0 and (case[6] % 16 != 0 or case in st.FULL_CASES)
    values, ties = st.run_case(case)
    assert np.all(np.isfinite(values))
    assert int(ties.sum()) == 0, ties


def test_case_table_covers_what_the_gpu_file_needs():
    shapes = {}
    for c in st.CHAIN_CASES:
        assert c[5] in (25, 40) and c[6] in (37, 21) and c[7] in (1, 2)
        shapes.setdefault(c[:3], set()).add(c[10])
    assert set(shapes) == {(6, 4, 12), (3, 8, 12), (2, 16, 17), (5, 2, 12), (11, 3, 17), (7, 5, 17)}
    assert all(b == {None, 'vector', 'data'} for b in shapes.values())
    with_pattern = [c for c in st.CHAIN_CASES if c[11] is not None]
    assert len(with_pattern) >= 2
    assert any(0 in c[11] and c[0] - 1 in c[11] for c in with_pattern)
    assert [c[:3] for c in st.FULL_CASES] == [(196, 4, 1024), (157, 5, 1024)]
    assert all(c[5] == 3 and c[6] == 16 and c[9] == 7000 and c[10] == 'data' for c in st.FULL_CASES)


# ---- host logic: no engine is ever built
def _no_engine(monkeypatch):
    """any attempt to build an engine fails the test (as tests/test_softmax_v.py)"""
    from boltzmann_machines_amd import rbm as rbm_mod

    def boom(*a, **k):
        raise AssertionError('an engine call was made')
    monkeypatch.setattr(rbm_mod, 'RbmEngine', boom)
    monkeypatch.setattr(rbm_mod, 'RbmEngine64', boom)


def _model(tmp_path, G=3, K=3, **kw):
    import boltzmann_machines_amd as bm
    return bm.CategoricalRBM(G, K, 4, batch_size=4, model_path=str(tmp_path) + '/m/', verbose=False, **kw)


def test_base_logits_of_data(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    C_ = np.array([[0, 1, -1], [0, 2, -1], [1, -1, -1], [0, 1, 2]])
    X = m.encode(C_, missing=-1)
    a = m._base_group_logits(X)
    count = np.array([[3, 1, 0], [0, 2, 1], [0, 0, 1.]])
    n_g = np.array([4, 3, 1.])
    np.testing.assert_allclose(a, np.log((count + 1) / (n_g[:, None] + 3)).reshape(9), rtol=1e-6)
    assert a.dtype == np.float32
    np.testing.assert_array_equal(a, st.base_group_logits(X, 3, 3))
    # every group's base distribution is normalised
    np.testing.assert_allclose(np.exp(a.astype(np.float64)).reshape(3, 3).sum(axis=1), 1.0, rtol=0, atol=1e-6)
    assert m._base_group_logits(None) is None
    np.testing.assert_array_equal(m._base_group_logits(np.arange(9.)), np.arange(9, dtype=f32))
    assert m._engine is None


def test_observed_patterns(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    C_ = np.array([[0, 1, -1], [2, 2, 2], [1, 0, -1], [-1, 1, 2], [0, 0, 0], [-1, 2, 1]])
    X = m.encode(C_, missing=-1)
    patterns, index = m.observed_patterns(X)
    assert patterns.dtype == np.bool_ and patterns.shape == (3, 3) and index.shape == (6,)
    np.testing.assert_array_equal(patterns[index], C_ >= 0)
    assert len({tuple(p) for p in patterns}) == 3
    assert index[0] == index[2] and index[1] == index[4] and index[3] == index[5]
    bad = X.copy()
    bad[1, 0:2] = 1
    with pytest.raises(ValueError, match='neither one-hot nor empty'):
        m.observed_patterns(bad)
    p0, i0 = m.observed_patterns(np.zeros((0, 9), f32))
    assert p0.shape == (0, 3) and i0.shape == (0,)
    assert m._engine is None


def test_argument_errors_come_before_the_engine(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    X = m.encode(np.array([[0, 1, 2], [1, 1, -1]]), missing=-1)
    for kw in (dict(n_betas=1), dict(n_runs=0), dict(n_gibbs_steps=0),
               dict(X_base=np.zeros(8)), dict(X_base=np.zeros((4, 8))), dict(X_base=np.ones((2, 9))),
               dict(observed=np.ones(4, bool)), dict(observed=np.ones((1, 3), bool)), dict(observed=np.array([1, 0, 1])),
               dict(observed=np.zeros(3, bool))):
        with pytest.raises(ValueError):
            m.ais_log_Z(**kw)
    with pytest.raises(ValueError, match='observes no group'):
        m.ais_log_Z_rows(np.vstack([X, np.zeros((1, 9), f32)]))
    with pytest.raises(ValueError, match='observed'):
        m.ais_log_Z_rows(X, observed=np.ones(3, bool))
    with pytest.raises(ValueError, match='neither one-hot nor empty'):
        m.ais_log_Z_rows(np.ones((1, 9), f32))
    # the refusal of log_Z stands, and names the estimator
    with pytest.raises(ValueError) as e:
        m.log_Z()
    assert 'softmax visible units' in str(e.value) and 'log_Z' in str(e.value) and 'ais_log_Z' in str(e.value)
    assert m._engine is None


def test_header_declares_library_exports_and_ffi_binds():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    header = open(os.path.join(ROOT, 'include', 'bm355.h')).read()
    declared = set(re.findall(r'\b(bm_[a-z0-9_]+)\s*\(', header))
    assert 'bm_rbm_groups_ais' in declared
    assert len(_ffi.SIGNATURES['bm_rbm_groups_ais']) == 9
    assert hasattr(_ffi.load(), 'bm_rbm_groups_ais')
    assert callable(getattr(RbmEngine, 'groups_ais', None))
