"""AIS log Z of an RBM with softmax visible units and of its sub-models: a float64 NumPy restatement of RbmEngine.groups_ais
(include/bm355.h: bm_rbm_groups_ais), and ground truth by enumeration.

    V = G K one-hot groups, O the observed groups (v is zero on every other group), z = v W + hb, base logits a [V]
    p_0(v) = prod_{g in O} softmax(a_g)[v_g],   log Z_0 = H log 2 + sum_{g in O} logsumexp_k a_{gK+k}
    log p*_beta(v) = (1 - beta) a.v + beta vb.v + sum_j softplus(beta z_j),   beta = float32(linspace(0, 1, n_betas))
    v_0: one categorical draw per observed group from softmax(a_g);  for k = 1 .. n_betas - 1:
    logw += log p*_{beta_k}(v_{k-1}) - log p*_{beta_{k-1}}(v_{k-1}), then n_gibbs_steps transitions h ~ Ber(sigmoid(beta_k z)),
    v_g ~ softmax_k(beta_k (h W^T)_{gK+k} + a + beta_k (vb - a)) for g in O (none behind the last score);  value = logw + log Z_0.

RNG: the pinned Philox stream of the engine - site 7 for v_0 (call 0), 8 for v, 9 for h, counter word site + 16 t (t the Gibbs
step), call = beta step k, row offset = chain0 + row.  A group's uniform is the visible layer's per-element stream read at the
group's first unit (every K-th column); the group takes the first category whose cumulative probability exceeds it; the uniforms of
unobserved groups are skipped.  Near-ties are recorded per chain in `ties`: a Bernoulli draw whose uniform lies within 1e-6 of its
probability, a group draw whose uniform lies within 1e-6 of an interior cumulative probability - there a float32 engine may
legitimately draw the other state."""
import numpy as np

from boltzmann_machines_amd.utils import philox
from tests.np_reference import sigmoid, softplus

SITE_V0, SITE_V, SITE_H = 7, 8, 9
f64 = np.float64


def make_params(G, K, H, std=0.1, seed=3):
    """float32 W [GK][H], vb [GK], hb [H] from the pinned Philox stream (weights N(0, std^2), biases U(-0.2, 0.2))"""
    V = G * K
    W = (philox.normal(1357, seed, 0, V * H) * np.float32(std)).reshape(V, H)
    hb = (philox.uniform(1357, seed + 10, 0, H) - np.float32(0.5)) * np.float32(0.4)
    vb = (philox.uniform(1357, seed + 30, 0, V) - np.float32(0.5)) * np.float32(0.4)
    return dict(W=W, vb=vb, hb=hb)


def one_hot(C_, K):
    """categories [N][G] (-1: an empty group) -> float32 [N][G K]"""
    C_ = np.asarray(C_)
    return (C_[:, :, None] == np.arange(K)[None, None, :]).astype(np.float32).reshape(len(C_), -1)


def data(N, G, K, s, p_missing=0.0):
    """one-hot rows [N][G K] with skewed categories; every group is empty with probability p_missing, never a whole row"""
    u = philox.uniform(1357, 99 + s, 0, N * G).astype(f64).reshape(N, G)
    C_ = np.minimum((u ** 2 * K).astype(np.int64), K - 1)
    if p_missing > 0:
        gone = philox.uniform(1357, 199 + s, 0, N * G).reshape(N, G) < p_missing
        gone[gone.all(axis=1), 0] = False
        C_ = np.where(gone, -1, C_)
    return one_hot(C_, K)


def base_group_logits(X, G, K):
    """a_{gK+k} = log((count_{g,k} + 1) / (N_g + K)), N_g the rows that observe g, in float32: as SoftmaxVisible.ais_log_Z(X_base=X)
    hands it to the engine"""
    X3 = np.asarray(X, dtype=f64).reshape(len(X), G, K)
    count, n_g = X3.sum(axis=0), (X3.sum(axis=2) > 0).sum(axis=0).astype(f64)
    return np.log((count + 1.) / (n_g[:, None] + K)).reshape(G * K).astype(np.float32)


def betas(n_betas):
    return np.linspace(0., 1., n_betas).astype(np.float32).astype(f64)


def _f64(P):
    return {k: np.asarray(v, dtype=f64) for k, v in P.items()}


def _lse(x, axis=None):
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(m + np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True)), axis=axis)


def _observed(G, observed):
    return np.ones(G, dtype=bool) if observed is None else np.asarray(observed, dtype=bool)


def log_Z0(P, K, a=None, observed=None):
    V, H = P['W'].shape
    a = np.zeros(V) if a is None else np.asarray(a, dtype=f64)
    obs = _observed(V // K, observed)
    return H * np.log(2.) + np.sum(_lse(a.reshape(V // K, K), axis=1)[obs])


def _draw_h(p, seed, t, call, chain0, ties):
    R, n = p.shape
    u = philox.uniform(seed, SITE_H + 16 * t, call, R * n, idx0=chain0 * n).reshape(R, n)
    ties += np.sum(np.abs(u.astype(f64) - p) < 1e-6, axis=1)
    return (u < p.astype(np.float32)).astype(f64)


def _draw_groups(logits, K, obs, seed, site, t, call, chain0, ties):
    """one category per observed group of every row of logits [R][V]; zeros on the other groups"""
    R, V = logits.shape
    G = V // K
    u = philox.uniform(seed, site + 16 * t, call, R * V, idx0=chain0 * V).reshape(R, V)[:, ::K].astype(f64)
    l3 = logits.reshape(R, G, K)
    p = np.exp(l3 - l3.max(axis=2, keepdims=True))
    c = np.cumsum(p / p.sum(axis=2, keepdims=True), axis=2)
    ties += np.sum(np.any(np.abs(u[:, :, None] - c[:, :, :-1]) < 1e-6, axis=2) & obs[None, :], axis=1)
    c[:, :, -1] = 2.0                           # u < 1: the last category takes what is left
    first = np.argmax(c > u[:, :, None], axis=2)
    v = (first[:, :, None] == np.arange(K)[None, None, :]) & obs[None, :, None]
    return v.astype(f64).reshape(R, V)


def ais(P, K, n_betas, n_runs, k, seed, chain0=0, base_bias=None, observed=None):
    """-> (values [n_runs] float64, ties [n_runs] int: near-tie draws per chain)"""
    P = _f64(P)
    W, vb, hb = P['W'], P['vb'], P['hb']
    V, H = W.shape
    obs = _observed(V // K, observed)
    a = np.zeros(V) if base_bias is None else np.asarray(np.asarray(base_bias, dtype=np.float32), dtype=f64)
    ties = np.zeros(n_runs, dtype=np.int64)
    b = betas(n_betas)
    v = _draw_groups(np.tile(a, (n_runs, 1)), K, obs, seed, SITE_V0, 0, 0, chain0, ties)
    logw = np.zeros(n_runs)
    for step in range(1, n_betas):
        ba, bb = b[step - 1], b[step]
        z = v.dot(W) + hb
        logw += (bb - ba) * v.dot(vb - a) + np.sum(softplus(bb * z) - softplus(ba * z), axis=1)
        if step == n_betas - 1:
            break
        for t in range(k):
            h = _draw_h(sigmoid(bb * (v.dot(W) + hb)), seed, t, step, chain0, ties)
            v = _draw_groups(bb * h.dot(W.T) + a + bb * (vb - a), K, obs, seed, SITE_V, t, step, chain0, ties)
    return logw + log_Z0(P, K, a, obs), ties


# ---- ground truth
def free_energy_rows(P, X):
    P = _f64(P)
    X = np.asarray(X, dtype=f64)
    return -X.dot(P['vb']) - np.sum(softplus(X.dot(P['W']) + P['hb']), axis=1)


def _bits(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(f64)


def exact_log_Z(P, K, observed=None):
    """log Z of the model over the observed groups, by enumeration of the hidden layer with every observed group summed
    analytically: log sum_h exp(h.hb) prod_{g in O} sum_k exp((h W^T + vb)_{gK+k})"""
    P = _f64(P)
    V, H = P['W'].shape
    obs = _observed(V // K, observed)
    h = _bits(H)
    l3 = (h.dot(P['W'].T) + P['vb']).reshape(len(h), V // K, K)
    return float(_lse(h.dot(P['hb']) + np.sum(_lse(l3, axis=2)[:, obs], axis=1)))


def exact_log_p(P, K, X):
    """log p(x) per row of X (groups one-hot or empty), each row in the model of its own observed groups"""
    X = np.asarray(X, dtype=f64)
    G = X.shape[1] // K
    obs = X.reshape(len(X), G, K).sum(axis=2) > 0
    F = free_energy_rows(P, X)
    return np.array([-F[n] - exact_log_Z(P, K, obs[n]) for n in range(len(X))])


def all_states(G, K):
    """every one-hot state of G groups of K, [K^G][G K] float32"""
    C_ = np.stack(np.meshgrid(*[np.arange(K)] * G, indexing='ij'), axis=-1).reshape(-1, G)
    return one_hot(C_, K)


def sem_of(values):
    """(log_mean_exp, relative standard error of the mean of exp(values)): the inputs of the bracket rule max(0.02, 4 sem)"""
    from boltzmann_machines_amd.utils import log_mean_exp, log_std_exp
    values = np.asarray(values, dtype=f64)
    est = log_mean_exp(values)
    return est, np.exp(log_std_exp(values) - est) / np.sqrt(len(values))


def bracketed(values, exact):
    """the project's rule (tests/test_rbm_ais_gpu.py::bracket): |est - exact| < max(0.02, 4 sem)"""
    est, sem = sem_of(values)
    return abs(est - exact) < max(0.02, 4 * sem), est, sem


# ---- the chain-by-chain comparisons of tests/test_softmax_ais_gpu.py: tests/test_softmax_ais.py shows WITHOUT a GPU that none of
# them meets a near-tie in the twin (ties == 0), so every chain is compared.  In every case chain0 != 0, n_runs % 16 != 0 and
# n_runs exceeds the engine's max_batch.  Every shape runs with each of the three bases; the cases with a pattern leave out the
# first and the last group (G = 2: the last, or the first), or a middle one.
# (G, K, H, param seed, std, n_betas, n_runs, k, AIS seed, chain0, base: None | 'vector' | 'data', absent groups or None)
def _shape_cases(G, K, H, pseed, s):
    ends = (0, G - 1) if G >= 3 else (G - 1,)
    mid = (1,) if G >= 3 else (0,)
    return [(G, K, H, pseed, 0.1, 25, 37, 1, 3100 + s, 5, None, None),
            (G, K, H, pseed, 0.3, 40, 21, 2, 3200 + s, 1234, 'vector', ends),
            (G, K, H, pseed, 0.1, 25, 37, 2, 3300 + s, 77, 'data', mid)]


FUSED_SHAPES = [(6, 4, 12), (3, 8, 12), (2, 16, 17)]
GENERIC_SHAPES = [(5, 2, 12), (11, 3, 17), (7, 5, 17)]          # V % 4 != 0; groups that straddle a slot, a partial last slot
CHAIN_CASES = [c for i, (G, K, H) in enumerate(FUSED_SHAPES + GENERIC_SHAPES) for c in _shape_cases(G, K, H, 3 + i, i)]
# the full width: 196 x 4 (fused) and 157 x 5 (generic) visible, 1024 hidden, weights N(0, 0.1^2), n_betas = 3, 16 chains at a chain0
# in the thousands, data base
FULL_CASES = [(196, 4, 1024, 5, 0.1, 3, 16, 1, 4242, 7000, 'data', None),
              (157, 5, 1024, 6, 0.1, 3, 16, 1, 4243, 7000, 'data', None)]


def case_id(c):
    return '%dx%dx%d-b%d-k%d-%s-%s' % (c[0], c[1], c[2], c[5], c[7], c[10], 'all' if c[11] is None else 'no' + '_'.join(map(str, c[11])))


def base_of(kind, G, K, s=1):
    """the base logits of a case: None, a vector from the Philox stream, or the smoothed base rates of synthetic incomplete rows"""
    if kind is None:
        return None
    if kind == 'vector':
        return (philox.uniform(1357, 300 + s, 0, G * K) - np.float32(0.5)) * np.float32(2.0)
    return base_group_logits(data(50, G, K, 10 + s, p_missing=0.2), G, K)


def observed_of(absent, G):
    if absent is None:
        return None
    o = np.ones(G, dtype=bool)
    o[list(absent)] = False
    return o


def case_inputs(c):
    """(P, a, observed) of a case"""
    G, K, H, pseed, std = c[:5]
    return make_params(G, K, H, std=std, seed=pseed), base_of(c[10], G, K), observed_of(c[11], G)


def run_case(c):
    G, K, H, pseed, std, n_betas, n_runs, k, seed, chain0 = c[:10]
    P, a, obs = case_inputs(c)
    return ais(P, K, n_betas, n_runs, k, seed, chain0, a, obs)
