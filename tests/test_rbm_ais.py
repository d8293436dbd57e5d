"""AIS log Z and exact log-likelihood of a Bernoulli RBM, the part that needs no GPU: the float64 twin
(tests/np_reference_rbm_ais.py) against enumeration, the twin's AIS against the enumerated log Z, the inputs of the GPU
file's chain-by-chain comparisons (no near-tie in any of them), and the host-side surface (header, ffi, model methods)."""
import os
import re

import numpy as np
import pytest

from tests import np_reference_rbm_ais as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_model():
    """the 10 x 8 ground-truth model: weights N(0, 0.5^2)"""
    return ra.make_params(10, 8, std=0.5, seed=7)


def bracket(values, exact):
    est, sem = ra.sem_of(values)
    assert abs(est - exact) < max(0.02, 4 * sem), (est, exact, sem)


def test_exact_log_p_sums_to_one():
    P = small_model()
    allv = ra._bits(10)
    lp = ra.exact_log_p(P, allv)
    assert abs(np.sum(np.exp(lp)) - 1.) < 1e-10
    # ... and the enumeration over h agrees with the enumeration over every unit
    W, vb, hb = (np.asarray(P[n], dtype=np.float64) for n in ('W', 'vb', 'hb'))
    allh = ra._bits(8)
    negE = allv.dot(vb)[:, None] + allh.dot(hb)[None, :] + allv.dot(W).dot(allh.T)
    assert abs(ra._lse(negE.ravel()) - ra.exact_log_Z(P)) < 1e-10


@pytest.mark.parametrize('base', [None, 'data'])
def test_twin_ais_brackets_exact_log_Z(base):
    P = small_model()
    a = None
    if base == 'data':      # base rates of (approximate) samples of the model: a few Gibbs sweeps in NumPy
        rng = np.random.RandomState(5)
        W, vb, hb = (np.asarray(P[n], dtype=np.float64) for n in ('W', 'vb', 'hb'))
        v = (rng.rand(200, 10) < 0.5).astype(np.float64)
        for _ in range(50):
            h = (rng.rand(200, 8) < ra.sigmoid(v.dot(W) + hb)).astype(np.float64)
            v = (rng.rand(200, 10) < ra.sigmoid(h.dot(W.T) + vb)).astype(np.float64)
        a = ra.base_rate_bias(v)
    values, _ = ra.ais(P, n_betas=1000, n_runs=256, k=1, seed=777, base_bias=a)
    bracket(values, ra.exact_log_Z(P))


def test_twin_log_Z0_and_two_beta_identity():
    P = ra.make_params(20, 12)
    V, H = 20, 12
    assert abs(ra.log_Z0(P) - (V + H) * np.log(2.)) < 1e-12
    a = ra.base_of('vector', V)
    assert abs(ra.log_Z0(P, a) - (H * np.log(2.) + np.sum(np.log1p(np.exp(np.asarray(a, dtype=np.float64)))))) < 1e-10
    # n_betas = 2: one importance weight p*_1(v_0) / p*_0(v_0), v_0 ~ p_0, no transition
    from boltzmann_machines_amd.utils import philox
    values, _ = ra.ais(P, n_betas=2, n_runs=9, k=3, seed=31, chain0=4, base_bias=a)
    a64 = np.asarray(a, dtype=np.float64)
    u = philox.uniform(31, ra.SITE_V0, 0, 9 * V, idx0=4 * V).reshape(9, V)
    v0 = (u < ra.sigmoid(a64).astype(np.float32)).astype(np.float64)
    want = -ra.free_energy_rows(P, v0) - v0.dot(a64) - H * np.log(2.) + ra.log_Z0(P, a)
    np.testing.assert_allclose(values, want, rtol=0, atol=1e-10)
    # with a = 0 and no weights the estimate is exact: every chain returns (V + H) log 2
    Z = dict(W=np.zeros((V, H), np.float32), vb=np.zeros(V, np.float32), hb=np.zeros(H, np.float32))
    values, _ = ra.ais(Z, n_betas=7, n_runs=5, k=1, seed=1)
    np.testing.assert_allclose(values, (V + H) * np.log(2.), rtol=0, atol=1e-10)


def test_twin_slices():
    """chains [c, c + n) of a larger run are the run of n chains at chain0 = c"""
    P = ra.make_params(20, 12, std=0.3)
    a, _ = ra.ais(P, 10, 30, 2, seed=11)
    c, _ = ra.ais(P, 10, 10, 2, seed=11, chain0=15)
    assert np.array_equal(a[15:25], c)


@pytest.mark.parametrize('case', ra.CHAIN_CASES + [ra.FULL_CASE], ids=lambda c: '%dx%d-k%d-%s' % (c[0], c[1], c[6], c[9]))
def test_gpu_chain_cases_meet_no_near_tie(case):
    """the inputs of the GPU file's chain-by-chain comparisons stay inside the comparison: no draw of the twin within
    float32 round-off of its probability, so no chain is excluded there"""
    V, H, pseed, std, n_betas, n_runs, k, seed, chain0, base = case
    values, ties = ra.ais(ra.make_params(V, H, std=std, seed=pseed), n_betas, n_runs, k, seed, chain0, ra.base_of(base, V))
    assert np.all(np.isfinite(values))
    assert int(ties.sum()) == 0, ties


def test_header_declares_and_ffi_binds():
    from boltzmann_machines_amd import _ffi
    header = open(os.path.join(ROOT, 'include', 'bm355.h')).read()
    declared = set(re.findall(r'\b(bm_[a-z0-9_]+)\s*\(', header))
    for name in ('bm_rbm_ais', 'bm_rbm_free_energy_rows'):
        assert name in declared, name
        assert name in _ffi.SIGNATURES, name
    assert len(_ffi.SIGNATURES['bm_rbm_ais']) == 8 and len(_ffi.SIGNATURES['bm_rbm_free_energy_rows']) == 4


def test_model_surface_and_refusals(tmp_path):
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM, MultinomialRBM
    from boltzmann_machines_amd.engine import RbmEngine
    assert callable(getattr(BernoulliRBM, 'log_Z', None)) and callable(getattr(BernoulliRBM, 'log_proba', None))
    assert callable(getattr(RbmEngine, 'ais', None)) and callable(getattr(RbmEngine, 'free_energy_rows', None))
    kw = dict(n_visible=6, n_hidden=4, verbose=False)
    X = np.zeros((2, 6), dtype=np.float32)
    for model, word in ((GaussianRBM(model_path=str(tmp_path / 'g') + '/', **kw), 'Gaussian'),
                        (MultinomialRBM(model_path=str(tmp_path / 'm') + '/', **kw), 'Multinomial'),
                        (BernoulliRBM(model_path=str(tmp_path / 'd') + '/', dtype='float64', **kw), 'float64'),
                        (BernoulliRBM(model_path=str(tmp_path / 'f') + '/', dbm_first=True, **kw), 'dbm_first'),
                        (BernoulliRBM(model_path=str(tmp_path / 'l') + '/', dbm_last=True, **kw), 'dbm_last')):
        with pytest.raises(NotImplementedError, match=word):
            model.log_Z(n_betas=5, n_runs=4)
        with pytest.raises(NotImplementedError, match=word):
            model.log_proba(X, 0.)
    # the base-rate bias of data is Laplace-smoothed: finite for constant columns
    m = BernoulliRBM(model_path=str(tmp_path / 'b') + '/', **kw)
    Xb = np.array([[1, 0, 1, 0, 1, 1], [1, 0, 0, 0, 1, 0]], dtype=np.float32)
    a = m._base_rate_bias(Xb)
    np.testing.assert_allclose(a, np.log(np.array([3, 1, 2, 1, 3, 2.]) / np.array([1, 3, 2, 3, 1, 2.])), rtol=1e-6)
    np.testing.assert_array_equal(a, ra.base_rate_bias(Xb))
    assert m._base_rate_bias(None) is None
    np.testing.assert_array_equal(m._base_rate_bias(np.arange(6.)), np.arange(6, dtype=np.float32))
    with pytest.raises(ValueError):
        m._base_rate_bias(np.zeros(5))
