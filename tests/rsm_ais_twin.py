"""AIS log Z per document length of an RBM with replicated softmax visible units: a NumPy restatement of RbmEngine.rsm_ais
(include/bm355.h: bm_rbm_rsm_ais), and ground truth by enumeration of the hidden layer.

    chain r has length D_r;  t = D hb + v W;  base logits a [V] (float32), dvec = fl32(vb - a) as the engine's table kernel forms it
    p_0(v) = Multinomial(D, softmax(a)),   log Z_0(D) = H log 2 + D logsumexp(a)
    log p*_beta(v) = log(D!/prod v_i!) + (1 - beta) a.v + beta vb.v + sum_j softplus(beta t_j),   beta = float32(linspace(0, 1, n_betas))
    v_0 ~ p_0;  for k = 1 .. n_betas - 1:  logw += (beta_k - beta_{k-1}) v.dvec + sum_j [softplus(beta_k t_j) - softplus(beta_{k-1} t_j)],
    then n_gibbs_steps transitions h ~ Ber(sigmoid(beta_k t)), v ~ Multinomial(D, softmax(a + beta_k dvec + beta_k W h)) (none behind
    the last score);  value = logw + log Z_0(D).

The scores are float64.  The draws are the engine's: hidden unit j of global row r reads the uniform at r H + j of site 9 + 16 t, and
the counts come from tests/rsm_twin.py's restated sampler - float32 logits, e = exp_neg(min(mx - l, 80)), THE PREFIX ORDER, draw d of
global row r at r max_length + d of site 8 + 16 t (site 7, call 0 for v_0), the smallest i with c[i] > fl(u S) - with call = beta step
and global row = chain0 + r.

Near-ties are recorded per chain in `ties`: a hidden draw whose uniform lies within TIE of its probability, a token draw whose
threshold u S lies within TIE * S of the prefix sum on either side of the unit it lands on - there a float32 engine, whose logits
differ from these in the last bits, may legitimately draw the other state."""
import numpy as np

from boltzmann_machines_amd.utils import philox
from tests import rsm_twin as rt
from tests.np_reference import sigmoid, softplus

SITE_V0, SITE_V, SITE_H = 7, 8, 9
TIE = 1e-6
f32, f64 = np.float32, np.float64


def make_params(V, H, std=0.1, seed=3):
    """float32 W [V][H], vb [V], hb [H] from the pinned Philox stream (weights N(0, std^2), biases U(-0.2, 0.2))"""
    W = (philox.normal(2468, seed, 0, V * H) * f32(std)).reshape(V, H)
    hb = (philox.uniform(2468, seed + 10, 0, H) - f32(0.5)) * f32(0.4)
    vb = (philox.uniform(2468, seed + 30, 0, V) - f32(0.5)) * f32(0.4)
    return dict(W=W, vb=vb, hb=hb)


def peaked_base(V, s=1):
    """base logits that put most of the mass on a few words: U(-3, 3) from the Philox stream, float32"""
    return (philox.uniform(2468, 500 + s, 0, V) - f32(0.5)) * f32(6.0)


def unigram_base(X):
    """a_i = log((sum_n X[n,i] + 1) / (sum_n D_n + V)) in float64, as float32: what ais_log_Z(X_base=X) hands to the engine"""
    X = np.asarray(X, f64)
    return np.log((X.sum(axis=0) + 1.) / (X.sum() + X.shape[1])).astype(f32)


def betas(n_betas):
    return np.linspace(0., 1., n_betas).astype(f32).astype(f64)


def _lse(x, axis=None):
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(m + np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True)), axis=axis)


def _base(V, base_logits):
    return np.zeros(V, f32) if base_logits is None else np.ascontiguousarray(base_logits, f32)


def log_Z0(P, lengths, base_logits=None):
    V, H = P['W'].shape
    return H * np.log(2.) + np.asarray(lengths, f64) * _lse(_base(V, base_logits).astype(f64))


def _draw_h(p, seed, t, call, chain0, ties):
    R, n = p.shape
    u = philox.uniform(seed, SITE_H + 16 * t, call, R * n, idx0=chain0 * n).reshape(R, n)
    ties += np.sum(np.abs(u.astype(f64) - p) < TIE, axis=1)
    return (u < p.astype(f32)).astype(f64)


def _draw_counts(L, D, seed, site, t, call, chain0, max_length, ties):
    """count rows [R][V] of the float32 logits L [R][V] and the lengths D [R]: multinomial_counts_kernel's draws"""
    L = np.ascontiguousarray(L, f32)
    R, V = L.shape
    U = philox.uniform(seed, site + 16 * t, call, R * max_length, idx0=chain0 * max_length).reshape(R, max_length)
    out = np.zeros((R, V), f64)
    for j in range(R):
        c = rt.prefix_order(rt.softmax_e(L[j]))
        S = c[V - 1]
        thr = (U[j, :int(D[j])] * S).astype(f32)
        cat = np.minimum(np.searchsorted(c, thr, side='right'), V - 1)
        c64, t64, tol = c.astype(f64), thr.astype(f64), TIE * f64(S)
        above = (cat < V - 1) & (c64[cat] - t64 < tol)                              # (the last unit has no boundary above: the clamp)
        below = (cat > 0) & (t64 - c64[np.maximum(cat - 1, 0)] < tol)
        ties[j] += np.sum(above | below)
        out[j] = np.bincount(cat, minlength=V)
    return out


def ais(P, lengths, n_betas, k, seed, chain0=0, base_logits=None, max_length=None):
    """-> (values [R] float64, ties [R] int: near-tie draws per chain); chain r has length lengths[r]"""
    W, vb, hb = (np.asarray(P[n], f32) for n in ('W', 'vb', 'hb'))
    V, H = W.shape
    D = np.asarray(lengths, f64).reshape(-1)
    R = len(D)
    max_length = int(D.max()) if max_length is None else int(max_length)
    a32 = _base(V, base_logits)
    d32 = (vb - a32).astype(f32)
    a, d, W, hb = a32.astype(f64), d32.astype(f64), W.astype(f64), hb.astype(f64)
    ties = np.zeros(R, np.int64)
    b = betas(n_betas)
    v = _draw_counts(np.tile(a32, (R, 1)), D, seed, SITE_V0, 0, 0, chain0, max_length, ties)
    logw = np.zeros(R)
    for step in range(1, n_betas):
        ba, bb = b[step - 1], b[step]
        t = v.dot(W) + D[:, None] * hb
        logw += (bb - ba) * v.dot(d) + np.sum(softplus(bb * t) - softplus(ba * t), axis=1)
        if step == n_betas - 1:
            break
        for g in range(k):
            h = _draw_h(sigmoid(bb * (v.dot(W) + D[:, None] * hb)), seed, g, step, chain0, ties)
            v = _draw_counts(bb * h.dot(W.T) + (a + bb * d), D, seed, SITE_V, g, step, chain0, max_length, ties)
    return logw + log_Z0(P, D, a32), ties


# ---- ground truth
def _bits(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(f64)


def exact_log_Z(P, D):
    """log Z_D = log sum_h exp(D h.hb) (sum_i exp(vb_i + (W h)_i))^D over the 2^H hidden states (the counts summed by the
    multinomial theorem): cheap for H <= 16 at any V and D"""
    W, vb, hb = (np.asarray(P[n], f64) for n in ('W', 'vb', 'hb'))
    h = _bits(W.shape[1])
    return float(_lse(D * h.dot(hb) + D * _lse(h.dot(W.T) + vb, axis=1)))


def log_mean_and_se(values):
    """(log_mean_exp, its delta-method standard error std(w) / (mean(w) sqrt(n)), w = exp(values)) of one length's chains"""
    x = np.asarray(values, f64)
    w = np.exp(x - x.max())
    return float(x.max() + np.log(w.mean())), float(w.std(ddof=1) / (w.mean() * np.sqrt(len(w))))


# ---- the chain-by-chain comparisons of tests/test_rsm_ais_gpu.py.  tests/test_rsm_ais.py shows WITHOUT a GPU that none of them meets
# a near-tie in the twin (ties == 0): every chain is compared.  The seeds were chosen for that.
# (V, H, max_length, lengths, n_betas, k, seed, chain0, base: None | 'peaked', std, param seed)
def _ladder(n, max_length):
    """n lengths from 1 to max_length, mixed: 1, max_length, and a spread between"""
    return [1 + (r * 7919) % max_length if r > 1 else (1, max_length)[r] for r in range(n)]


CHAIN_CASES = [
    (2, 16, 9, _ladder(33, 9), 12, 1, 5101, 5, None, 0.3, 3),
    (16, 17, 12, _ladder(32, 12), 10, 2, 5201, 1234, 'peaked', 0.3, 4),
    (17, 40, 20, _ladder(33, 20), 8, 1, 5302, 77, 'peaked', 0.1, 5),
    (256, 16, 30, [30] * 2 + [1] * 2 + _ladder(8, 30), 6, 2, 5401, 3, None, 0.1, 6),
    (257, 17, 25, _ladder(9, 25), 6, 1, 5501, 40, 'peaked', 0.1, 7),
    (300, 40, 40, [1], 30, 1, 5601, 0, 'peaked', 0.1, 8),
    (300, 40, 40, [40], 2, 1, 5701, 9, None, 0.1, 8),
    (4096, 17, 6, [1, 6, 3, 2], 4, 1, 5801, 2, 'peaked', 0.05, 9),
    (4097, 16, 5, [5, 1, 3], 4, 2, 5901, 11, None, 0.05, 10),
]


def case_id(c):
    return '%dx%d-L%d-r%d-b%d-k%d-%s' % (c[0], c[1], c[2], len(c[3]), c[4], c[5], c[8])


def case_inputs(c):
    """(P, a) of a case"""
    V, H = c[:2]
    return make_params(V, H, std=c[9], seed=c[10]), (peaked_base(V, c[10]) if c[8] == 'peaked' else None)


def run_case(c):
    P, a = case_inputs(c)
    return ais(P, c[3], c[4], c[5], c[6], c[7], a, c[2])
