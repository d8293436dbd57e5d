"""CPU checks of the any-depth AIS / ELBO restatement (tests/np_reference_depth.py) against exact enumeration: the
ground truth the GPU tests of DBM.log_Z / log_proba at depths other than 2 (tests/test_ais_depth_gpu.py) rely on."""
import numpy as np
import pytest

from boltzmann_machines_amd.utils import log_mean_exp, log_std_exp, philox
from tests import np_reference as ref
from tests import np_reference_depth as rd


def model(V, nh, std=0.5, seed=3):
    """float64 DBM parameters (P dict of NumpyDBM) with N(0, std^2) weights and biases in [-0.2, 0.2)"""
    n = [V] + list(nh)
    P = {}
    for i in range(len(nh)):
        s = rd._sfx(i)
        P['W' + s] = philox.normal(4321, seed + i, 0, n[i] * n[i + 1]).astype(np.float64).reshape(n[i], n[i + 1]) * std
        P['hb' + s] = (philox.uniform(4321, seed + 10 + i, 0, n[i + 1]).astype(np.float64) - 0.5) * 0.4
    P['vb'] = (philox.uniform(4321, seed + 30, 0, V).astype(np.float64) - 0.5) * 0.4
    return P


def dbm(P, nh, N, **kw):
    d = rd.DepthDBM(P, len(nh), N, N, **kw)
    for i, n in enumerate(nh):
        P['mu' + rd._sfx(i)] = np.zeros((N, n))
    return d


def data(N, V, seed):
    return (philox.uniform(4321, 77 + seed, 0, N * V).reshape(N, V) < 0.3).astype(np.float64)


def test_exact_log_Z_matches_the_two_layer_enumeration():
    P = model(10, [6, 5])
    assert abs(rd.exact_log_Z(P, 2) - ref.dbm_exact_log_Z(P['W'], P['W_1'], P['vb'], P['hb'], P['hb_1'])) < 1e-10


@pytest.mark.parametrize('V,nh', [(5, [7]), (4, [3, 5]), (3, [3, 3, 3]), (3, [2, 3, 2, 2])])
def test_exact_log_Z_matches_brute_force(V, nh):
    P = model(V, nh, std=1.0)
    assert abs(rd.exact_log_Z(P, len(nh)) - rd.brute_log_Z(P, len(nh))) < 1e-10


@pytest.mark.parametrize('V,nh', [(4, [3, 5]), (3, [3, 3, 3]), (3, [2, 3, 2, 2])])
def test_exact_log_p_matches_brute_force(V, nh):
    """log p(v) from the odd-depth enumeration = log sum_h exp(-E(v, h)) - log Z over every hidden unit"""
    L = len(nh)
    P = model(V, nh, std=1.0)
    X = rd._bits(V)
    n = rd._widths(P, L)
    H = rd._bits(sum(n[1:]))
    for r, v in enumerate(X):
        S, c = [np.broadcast_to(v, (len(H), V))], 0
        for w in n[1:]:
            S.append(H[:, c:c + w])
            c += w
        negE = sum(S[d].dot(rd._b(P, d)) for d in range(L + 1))
        negE = negE + sum(np.sum(S[d].dot(rd._W(P, d)) * S[d + 1], axis=1) for d in range(L))
        assert abs(rd.exact_log_p(P, L, v[None])[0] - (rd._lse(negE) - rd.brute_log_Z(P, L))) < 1e-10


def test_two_layer_restatement_equals_np_reference():
    """at L = 2 the any-depth AIS and ELBO are NumpyDBM's (same draws, same arithmetic up to summation order)"""
    V, nh, N = 10, [6, 5], 7
    a = dbm(model(V, nh), nh, N)
    P = model(V, nh)
    b = ref.NumpyDBM(P, 2, N, N)
    P['mu'], P['mu_1'] = np.zeros((N, nh[0])), np.zeros((N, nh[1]))
    np.testing.assert_allclose(a.ais(40, 33, 2, seed=9, chain0=4), b.ais(40, 33, 2, 9, chain0=4), rtol=1e-12)
    X = data(N, V, 1)
    np.testing.assert_allclose(a.log_proba(X), b.log_proba(X), rtol=1e-12)


@pytest.mark.parametrize('V,nh,seed', [(10, [8], 1), (8, [6, 5, 4], 2), (6, [5, 4, 4, 3], 3)])
def test_numpy_ais_brackets_exact_log_Z(V, nh, seed):
    P = model(V, nh, seed=seed)
    exact = rd.exact_log_Z(P, len(nh))
    vals = dbm(P, nh, 4).ais(n_betas=2000, n_runs=256, k=1, seed=100 + seed)
    est = log_mean_exp(vals)
    sem = np.exp(log_std_exp(vals) - est) / np.sqrt(len(vals))
    assert abs(est - exact) < max(0.02, 4 * sem), (est, exact, sem)


@pytest.mark.parametrize('V,nh', [(10, [8]), (8, [6, 5]), (8, [6, 5, 4]), (6, [5, 4, 4, 3])])
def test_elbo_is_a_lower_bound(V, nh):
    L, N = len(nh), 12
    P = model(V, nh, seed=5)
    d = dbm(P, nh, N, max_mf=30, mf_tol=1e-9)
    X = data(N, V, 2)
    elbo = d.log_proba(X) - rd.exact_log_Z(P, L)
    exact = rd.exact_log_p(P, L, X)
    assert np.all(elbo <= exact + 1e-6), (elbo - exact)
    assert np.all(elbo > exact - 5.)


def test_one_layer_elbo_is_exact():
    """L = 1: after one mean-field sweep the posterior is exact, and the ELBO is log p(v) up to the 1e-7 entropy clip"""
    V, nh, N = 10, [8], 12
    P = model(V, nh, seed=6)
    d = dbm(P, nh, N, max_mf=2)
    X = data(N, V, 3)
    np.testing.assert_allclose(d.log_proba(X) - rd.exact_log_Z(P, 1), rd.exact_log_p(P, 1, X), rtol=0, atol=1e-5)
