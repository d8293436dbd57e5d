"""CPU twin of softmax visible units with incomplete rows, clamped groups and exact group conditionals (bm_rbm_groups_set_missing,
bm_rbm_groups_gibbs_clamped, bm_rbm_groups_scores), for the tests.

Composed from what exists: the visible pass and the update are tests/softmax_v_twin.py's (visible_pass, SoftmaxVRBM), the clamp is
tests/clamp_twin.blend applied to the means and the states of that pass - a clamped group holds the clamp value, a free group
keeps what the unclamped pass gave it, uniform included.  New here: group_scores64, the float64 statement of the scores with the
forward-error bound the device is held to, and the exact conditionals by enumeration.
"""
import numpy as np

from tests import softmax_v_twin as T
from tests.clamp_twin import SITE_H, SITE_V, act2, blend

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                      # unit round-off of float32


def group_mask(flags, K):
    """[B][G] per-group flags -> [B][G K] float32, constant within every group"""
    return np.repeat(np.asarray(flags) != 0, K, axis=1).astype(f32)


def observed_groups(X, K):
    """[B][G] bool: the group holds a 1"""
    X = np.asarray(X)
    return X.reshape(len(X), -1, K).any(axis=2)


def missing_mask(X, K):
    """group_missing_mask_kernel: 1 where the unit's group is empty in its row"""
    return group_mask(~observed_groups(X, K), K)


def remove_groups(X, K, frac, seed, keep_rows=()):
    """X with a fraction `frac` of its groups emptied at random; rows in keep_rows stay complete -> (X', removed [B][G] bool)"""
    X = np.array(X, f32)
    G = X.shape[1] // K
    gone = np.random.RandomState(seed).uniform(size=(len(X), G)) < frac
    for r in keep_rows:
        if r < len(X):
            gone[r] = False
    X[group_mask(gone, K) != 0] = 0.0
    return X, gone


def clamped_visible_pass(h, W, vb, K, sample, seed, site, call, row0, clamp, mask):
    """(means, states) of the softmax visible pass with the clamped units replaced in both"""
    m, s = T.visible_pass(h, W, vb, K, sample, seed, site, call, row0)
    return blend(mask, clamp, m), blend(mask, clamp, s)


def groups_gibbs_clamped(p, K, V0, clamp, mask, n_steps, seed, call=0, row0=0, keep=None):
    """bm_rbm_groups_gibbs_clamped: (V, H, Vmean) after n_steps of h ~ p(h|v), v ~ p(v|h) with the clamped groups re-imposed in
    every visible pass (and on V0 first); keep(t, v): called with every step's v"""
    W = np.ascontiguousarray(p['W'], f32)
    v = blend(mask, clamp, np.ascontiguousarray(V0, f32))
    h = vm = None
    for t in range(n_steps):
        _, h = act2(v, W, None, None, p['hb'], None, 1.0, 0, 1, seed, SITE_H + 16 * t, call, row0)
        vm, v = clamped_visible_pass(h, W, p['vb'], K, 1, seed, SITE_V + 16 * t, call, row0, clamp, mask)
        if keep is not None:
            keep(t, v)
    return v, h, vm


class MissingRBM(T.SoftmaxVRBM):
    """SoftmaxVRBM with bm_rbm_groups_set_missing(on): every prop-down of the training chain holds the empty groups of the
    chain's input at zero; gibbs() - bm_rbm_gibbs - does not look at the mode"""

    _held = None

    def _down(self, h, sample, site):
        if self._held is None:
            return super(MissingRBM, self)._down(h, sample, site)
        X, M = self._held
        return clamped_visible_pass(h, self.p['W'], self.p['vb'], self.K, sample, self.seed, site, self.call, self.row0, X, M)

    def chain(self, X, k):
        Xin = np.ascontiguousarray(X, f32)
        self._held = (Xin, missing_mask(Xin, self.K))
        try:
            return super(MissingRBM, self).chain(Xin, k)
        finally:
            self._held = None


def softplus64(x):
    return np.logaddexp(0.0, x)


def group_scores64(p, X, K):
    """(S, bound), both [B][V] float64.  S[b][gK+k] = vb[gK+k] + sum_j softplus(a_j + W[gK+k][j]), a = z - W[c_g] (a = z for an
    empty group), z = x W + hb, everything in float64.  bound[b][gK+k] = sum_j [u ((G+1) A_j + |a_j| + |a_j + w_j|) + 8 u
    softplus(a_j + w_j)], A_j = sum_g |W[c_g][j]| + |hb_j|: the float32 accumulation of z over at most G + 1 non-zero terms, the two
    rounded operations that form the argument (softplus is 1-Lipschitz), and the 4 ulp of the device's softplus (twice: its own
    rounding on top)"""
    W, vb, hb = (np.asarray(p[n], f64) for n in ('W', 'vb', 'hb'))
    X = np.asarray(X, f64)
    B, V = X.shape
    G = V // K
    z = X.dot(W) + hb
    A = np.abs(X).dot(np.abs(W)) + np.abs(hb)
    S, bound = np.zeros((B, V)), np.zeros((B, V))
    for g in range(G):
        Wg = W[g * K:(g + 1) * K]
        a = z - X[:, g * K:(g + 1) * K].dot(Wg)                      # [B][H]; an empty group subtracts nothing
        arg = a[:, None, :] + Wg[None, :, :]                         # [B][K][H]
        sp = softplus64(arg)
        S[:, g * K:(g + 1) * K] = vb[g * K:(g + 1) * K] + sp.sum(axis=2)
        bound[:, g * K:(g + 1) * K] = (U * ((G + 1) * A + np.abs(a))[:, None, :] + U * np.abs(arg) + 8 * U * sp).sum(axis=2)
    return S, bound


def log_softmax_groups(S, K):
    S3 = np.asarray(S, f64).reshape(len(S), -1, K)
    return S3 - np.logaddexp.reduce(S3, axis=2, keepdims=True)


def group_log_proba64(p, X, K):
    """[B][G][K]: log p(v_g = k | v_-g) from group_scores64"""
    return log_softmax_groups(group_scores64(p, X, K)[0], K)


def predict64(p, X, K):
    """[B][G] categories: observed groups keep theirs, empty groups take the argmax of group_log_proba64"""
    X = np.asarray(X)
    return np.where(observed_groups(X, K), X.reshape(len(X), -1, K).argmax(axis=2), group_log_proba64(p, X, K).argmax(axis=2))


# ---- exact conditionals by enumeration of a small model
def hidden_states(H):
    return np.array([[(c >> b) & 1 for b in range(H)] for c in range(1 << H)], f64)


def log_p_star(p, v):
    """log sum_h exp(-E(v, h)) by enumerating h; v may have empty groups (their units are absent: they add nothing)"""
    W, vb, hb = (np.asarray(p[n], f64) for n in ('W', 'vb', 'hb'))
    hs = hidden_states(W.shape[1])
    v = np.asarray(v, f64)
    return float(np.logaddexp.reduce(v.dot(vb) + hs.dot(hb) + hs.dot(v.dot(W))))


def submodel(p, keep_groups, K):
    """the model of the listed groups alone: the rows of W and vb of every other group removed"""
    idx = np.concatenate([np.arange(g * K, (g + 1) * K) for g in keep_groups])
    return dict(W=np.asarray(p['W'])[idx], vb=np.asarray(p['vb'])[idx], hb=np.asarray(p['hb']))


def exact_group_conditional(p, x, g, K):
    """log p(v_g = . | the observed groups of x other than g) [K], in the model of group g and those groups alone, by enumeration
    of every (v_g, h)"""
    x = np.asarray(x, f64)
    G = len(x) // K
    obs = [q for q in range(G) if q != g and x[q * K:(q + 1) * K].any()]
    groups = sorted(obs + [g])
    sub = submodel(p, groups, K)
    at = groups.index(g)
    lp = np.zeros(K)
    for k in range(K):
        v = np.concatenate([x[q * K:(q + 1) * K] for q in groups])
        v[at * K:(at + 1) * K] = 0.0
        v[at * K + k] = 1.0
        lp[k] = log_p_star(sub, v)
    return lp - np.logaddexp.reduce(lp)


def exact_joint(p, x, free, K):
    """p(v_free | v_observed) over the K^len(free) category vectors of the `free` groups (row-major, first free group slowest), the
    other groups of x held as they are - observed, or empty and absent"""
    x = np.asarray(x, f64)
    cats = np.stack(np.meshgrid(*[np.arange(K)] * len(free), indexing='ij'), axis=-1).reshape(-1, len(free))
    lp = np.zeros(len(cats))
    for n, cv in enumerate(cats):
        v = x.copy()
        for g, k in zip(free, cv):
            v[g * K:(g + 1) * K] = 0.0
            v[g * K + k] = 1.0
        lp[n] = log_p_star(p, v)
    return np.exp(lp - np.logaddexp.reduce(lp))
