"""AIS log Z and exact log-likelihood of a Bernoulli-Bernoulli RBM: a float64 NumPy restatement of RbmEngine.ais /
free_energy_rows (include/bm355.h: bm_rbm_ais, bm_rbm_free_energy_rows), and ground truth by enumeration.

    E(v, h) = -v.vb - h.hb - v W h,   base model p_0(v) ~ exp(a.v),   z = v W + hb
    log p*_beta(v) = (1 - beta) a.v + beta vb.v + sum_j softplus(beta z_j),   log Z_0 = H log 2 + sum_i softplus(a_i)
    v_0 ~ Ber(sigmoid(a));  for k = 1 .. n_betas - 1:  logw += log p*_{beta_k}(v_{k-1}) - log p*_{beta_{k-1}}(v_{k-1}),
    then n_gibbs_steps transitions  h ~ Ber(sigmoid(beta_k z)),  v ~ Ber(sigmoid(beta_k (h W^T + vb) + (1 - beta_k) a))
    (none behind the last score);  value = logw + log Z_0;  beta = float32(linspace(0, 1, n_betas)).

RNG: the pinned Philox stream of the engine - site 7 for v_0 (call 0), 8 for v, 9 for h, counter word site + 16 t (t the
Gibbs step), call = beta step k, row offset = chain0 + row.  A draw whose uniform lies within 1e-6 of its probability (the
rule of tests/np_reference.py) is recorded per chain in `ties`: there a float32 engine may legitimately draw the other bit."""
import numpy as np

from boltzmann_machines_amd.utils import philox
from tests.np_reference import sigmoid, softplus

SITE_V0, SITE_V, SITE_H = 7, 8, 9


def make_params(V, H, std=0.1, seed=3):
    """float32 W [V][H], vb [V], hb [H] from the pinned Philox stream (weights N(0, std^2), biases U(-0.2, 0.2))"""
    W = (philox.normal(2468, seed, 0, V * H) * np.float32(std)).reshape(V, H)
    hb = (philox.uniform(2468, seed + 10, 0, H) - np.float32(0.5)) * np.float32(0.4)
    vb = (philox.uniform(2468, seed + 30, 0, V) - np.float32(0.5)) * np.float32(0.4)
    return dict(W=W, vb=vb, hb=hb)


def data(N, V, s, p=0.25):
    return (philox.uniform(2468, 99 + s, 0, N * V) < p).astype(np.float32).reshape(N, V)


def base_rate_bias(X):
    """a_i = logit((sum_n X[n, i] + 1) / (N + 2)) in float32, as BernoulliRBM.log_Z(X_base=X) hands it to the engine"""
    X = np.asarray(X, dtype=np.float64)
    p = (X.sum(axis=0) + 1.) / (len(X) + 2.)
    return (np.log(p) - np.log1p(-p)).astype(np.float32)


def betas(n_betas):
    return np.linspace(0., 1., n_betas).astype(np.float32).astype(np.float64)


def _f64(P):
    return {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}


def log_Z0(P, a=None):
    V, H = P['W'].shape
    a = np.zeros(V) if a is None else np.asarray(a, dtype=np.float64)
    return H * np.log(2.) + np.sum(softplus(a))


def log_p_star(P, v, beta, a):
    P = _f64(P)
    z = v.dot(P['W']) + P['hb']
    return (1. - beta) * v.dot(a) + beta * v.dot(P['vb']) + np.sum(softplus(beta * z), axis=1)


def _draw(p, seed, site, t, call, chain0, ties):
    R, n = p.shape
    u = philox.uniform(seed, site + 16 * t, call, R * n, idx0=chain0 * n).reshape(R, n)
    ties += np.sum(np.abs(u.astype(np.float64) - p) < 1e-6, axis=1)
    return (u < p.astype(np.float32)).astype(np.float64)


def ais(P, n_betas, n_runs, k, seed, chain0=0, base_bias=None):
    """-> (values [n_runs] float64, ties [n_runs] int: near-tie draws per chain)"""
    P = _f64(P)
    W, vb, hb = P['W'], P['vb'], P['hb']
    V, H = W.shape
    a = np.zeros(V) if base_bias is None else np.asarray(np.asarray(base_bias, dtype=np.float32), dtype=np.float64)
    ties = np.zeros(n_runs, dtype=np.int64)
    b = betas(n_betas)
    v = _draw(np.tile(sigmoid(a), (n_runs, 1)), seed, SITE_V0, 0, 0, chain0, ties)
    logw = np.zeros(n_runs)
    for step in range(1, n_betas):
        ba, bb = b[step - 1], b[step]
        z = v.dot(W) + hb
        logw += (bb - ba) * v.dot(vb - a) + np.sum(softplus(bb * z) - softplus(ba * z), axis=1)
        if step == n_betas - 1:
            break
        for t in range(k):
            h = _draw(sigmoid(bb * (v.dot(W) + hb)), seed, SITE_H, t, step, chain0, ties)
            v = _draw(sigmoid(bb * (h.dot(W.T) + vb) + (1. - bb) * a), seed, SITE_V, t, step, chain0, ties)
    return logw + log_Z0(P, a), ties


def free_energy_rows(P, X):
    P = _f64(P)
    X = np.asarray(X, dtype=np.float64)
    return -X.dot(P['vb']) - np.sum(softplus(X.dot(P['W']) + P['hb']), axis=1)


def _bits(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)


def _lse(x):
    m = np.max(x)
    return m + np.log(np.sum(np.exp(x - m)))


def exact_log_Z(P):
    """log Z by enumeration of the hidden layer, the visible units summed analytically"""
    P = _f64(P)
    h = _bits(P['W'].shape[1])
    return float(_lse(h.dot(P['hb']) + np.sum(softplus(h.dot(P['W'].T) + P['vb']), axis=1)))


def exact_log_p(P, X):
    """log p(v) per row of X: the hidden layer summed analytically (the free energy), minus exact_log_Z"""
    return -free_energy_rows(P, X) - exact_log_Z(P)


def sem_of(values):
    """(log_mean_exp, relative standard error of the mean of exp(values)): the inputs of the bracket rule max(0.02, 4 sem)"""
    from boltzmann_machines_amd.utils import log_mean_exp, log_std_exp
    values = np.asarray(values, dtype=np.float64)
    est = log_mean_exp(values)
    return est, np.exp(log_std_exp(values) - est) / np.sqrt(len(values))


# ---- the chain-by-chain comparisons of tests/test_rbm_ais_gpu.py: tests/test_rbm_ais.py shows WITHOUT a GPU that none of them
# meets a near-tie in the twin (ties == 0), so every chain is compared.
# (V, H, param seed, std, n_betas, n_runs, k, AIS seed, chain0, base: None | 'vector' | 'data')
CHAIN_CASES = [
    (20, 12, 3, 0.1, 25, 37, 1, 2222, 5, None),
    (20, 12, 3, 0.1, 25, 37, 2, 2222, 5, 'data'),
    (20, 12, 3, 0.3, 40, 21, 2, 901, 1234, 'vector'),
    (33, 17, 4, 0.1, 25, 37, 1, 2223, 5, 'vector'),
    (33, 17, 4, 0.1, 25, 37, 2, 2223, 5, None),
    (33, 17, 4, 0.3, 40, 21, 1, 902, 77, 'data'),
]
# the full shape: 784 x 1024, weights N(0, 0.1^2), n_betas = 3, 16 chains at a chain0 in the thousands
FULL_CASE = (784, 1024, 5, 0.1, 3, 16, 1, 4242, 7000, 'data')


def base_of(kind, V, s=1):
    """the base bias of a case: None, a vector from the Philox stream, or the base rates of synthetic data"""
    if kind is None:
        return None
    if kind == 'vector':
        return (philox.uniform(2468, 300 + s, 0, V) - np.float32(0.5)) * np.float32(2.0)
    return base_rate_bias(data(50, V, 10 + s, p=0.3))
