"""CPU twin of an RBM with softmax (categorical) visible units (bm_rbm_set_visible_groups), for the tests.

Built from what exists, in the style of tests/nrelu_twin.py:
  * the visible pass: the logits l = h W^T + vb are tests/clamp_twin.act2 with kind 1 and sigma = ones, (1 * z) * 1 + 1 * b - bit
    for bit the value a kind-3 pass of the engine forms (as tests/nrelu_twin.pre_activation); e and c of every group come from
    the oracle's pinned softmax row, orc_softmax_prefix at I = K; mean = e / S and t = u * S are single float32 NumPy operations;
    the uniforms are orc.uniform(seed, site, call, J * V, idx0 = row0 * V) read at every K-th column; the state is
    (c[k] > t) && !(c[k-1] > t);
  * the hidden pass: act2 with kind 0;
  * the update: orc_rbm_raw_grads on a hand-filled work struct, then orc_rbm_apply through OracleRBM; the free energy is
    OracleRBM.free_energy.
Nothing under oracle/ is involved beyond the calls named above.
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from tests.clamp_twin import SITE_H, SITE_V, act2

SITE_H0 = 2                  # csrc/bm_rbm.hip: the positive phase's site (and bm_rbm_sample_h's)
f32 = np.float32

_prefix_fn = None


def _prefix():
    """orc_softmax_prefix as a function object of its own (tests/multinomial_probes.prefix sets other argtypes on the library's)"""
    global _prefix_fn
    if _prefix_fn is None:
        proto = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
        _prefix_fn = proto(('orc_softmax_prefix', orc.lib()))
    return _prefix_fn


def group_prefix(L, K):
    """(e, c) [J][V] of the logits L [J][V]: per group of K columns e[k] = exp_neg(min(mx - l[k], 80)) and its sequential
    prefix sums c"""
    L = np.ascontiguousarray(L, f32)
    assert L.ndim == 2 and K >= 1 and L.shape[1] % K == 0, (L.shape, K)
    e, c = np.zeros_like(L), np.zeros_like(L)
    f, lp, ep, cp, step = _prefix(), L.ctypes.data, e.ctypes.data, c.ctypes.data, 4 * K
    for off in range(0, 4 * L.size, step):
        f(lp + off, K, ep + off, cp + off)
    return e, c


def softmax_groups(L, K, sample, u=None):
    """(means, states) [J][V] of the logits L; u [J][G]: the uniform of every group; sample = 0: states = means"""
    J, V = L.shape
    G = V // K
    e, c = group_prefix(L, K)
    e3, c3 = e.reshape(J, G, K), c.reshape(J, G, K)
    S = c3[:, :, K - 1:K]
    m = (e3 / S).astype(f32)
    if not sample:
        return m.reshape(J, V), m.reshape(J, V).copy()
    t = (np.asarray(u, f32).reshape(J, G, 1) * S).astype(f32)
    cp = np.concatenate([np.zeros((J, G, 1), f32), c3[:, :, :-1]], axis=2)
    s = ((c3 > t) & ~(cp > t)).astype(f32)
    return m.reshape(J, V), s.reshape(J, V)


def logits(h, W, vb):
    """l = h W^T + vb [J][V] as the engine's kind-3 pass rounds it"""
    Wt = np.ascontiguousarray(np.asarray(W, f32).T)
    l, _ = act2(h, Wt, None, None, vb, np.ones(Wt.shape[1], f32), 1.0, 1, 0, 0, 0, 0, 0)
    return l


def group_uniforms(seed, site, call, row0, J, V, K):
    """the uniform at flat index (row0 + j) * V + g K: the layer's per-element stream read at every group's first unit"""
    return orc.uniform(int(seed), int(site), int(call), J * V, idx0=int(row0) * V).reshape(J, V)[:, ::K]


def visible_pass(h, W, vb, K, sample, seed, site, call, row0=0):
    """(means, states) of the visible layer given h [J][H]"""
    l = logits(h, W, vb)
    J, V = l.shape
    u = group_uniforms(seed, site, call, row0, J, V, K) if sample else None
    return softmax_groups(l, K, sample, u)


def sample_v_from_h(p, Hs, K, seed, call=0, row0=0):
    """bm_rbm_sample_v_from_h of a handle with softmax visible units"""
    return visible_pass(Hs, p['W'], p['vb'], K, 1, seed, SITE_V, call, row0)


def one_hot(C_, K):
    C_ = np.asarray(C_)
    return (C_[:, :, None] == np.arange(K)[None, None, :]).astype(f32).reshape(len(C_), -1)


class SoftmaxVRBM(object):
    """CPU twin of one bm_rbm handle after bm_rbm_set_visible_groups(K): `rbm` is an oracle.OracleRBM that holds the variables
    and makes the update; the chain is restated here"""

    def __init__(self, p0, K, seed, l2=1e-4, sample_v_states=False, sample_h_states=True, sparsity_target=0.1, sparsity_cost=0.,
                 sparsity_damping=0.9):
        V, H = p0['W'].shape
        assert V % K == 0
        self.V, self.H, self.K = V, H, int(K)
        self.rbm = orc.OracleRBM(V, H, l2=l2, sample_v_states=sample_v_states, sample_h_states=sample_h_states,
                                 sparsity_target=sparsity_target, sparsity_cost=sparsity_cost, sparsity_damping=sparsity_damping)
        for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means'):
            if n in p0:
                self.rbm.p[n][...] = p0[n]
        self.seed, self.call, self.row0, self.l2 = int(seed), 0, 0, l2
        self.sample_v, self.sample_h = int(bool(sample_v_states)), int(bool(sample_h_states))

    @property
    def p(self):
        return self.rbm.p

    def set_seed(self, seed):
        self.seed, self.call = int(seed), 0

    def _up(self, v, sample, site):
        return act2(v, self.p['W'], None, None, self.p['hb'], None, 1.0, 0, sample, self.seed, site, self.call, self.row0)

    def _down(self, h, sample, site):
        return visible_pass(h, self.p['W'], self.p['vb'], self.K, sample, self.seed, site, self.call, self.row0)

    def chain(self, X, k):
        Xin = np.ascontiguousarray(X, f32)
        h0m, h0s = self._up(Xin, 1, SITE_H0)
        hstate = h0s if self.sample_h else h0m
        vm = vs = hm = None
        for t in range(k):
            vm, vs = self._down(hstate, self.sample_v, SITE_V + 16 * t)
            hm, hs = self._up(vs, self.sample_h, SITE_H + 16 * t)
            hstate = hs
        return dict(Xin=Xin, h0m=h0m, h0s=h0s, vm=vm, vs=vs, hm=hm)

    def train_step(self, X, lr, mom, k):
        ch = self.chain(X, k)
        B = len(ch['Xin'])
        Xin, h0m, vs, hm = (np.ascontiguousarray(ch[n], f32) for n in ('Xin', 'h0m', 'vs', 'hm'))
        z = np.zeros((B, max(self.V, self.H)), f32)                    # (h0s, vm, hs: not read by the raw sums)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        w = orc.RbmWork(ptr(Xin), ptr(h0m), ptr(z), ptr(z), ptr(vs), ptr(hm), ptr(z))
        raw = np.zeros(self.V * self.H + self.V + 2 * self.H, f32)
        orc.lib().orc_rbm_raw_grads(C.byref(self.rbm.cfg), C.byref(w), B, raw)
        self.rbm.apply(raw, float(B), lr, mom)
        self.call += 1
        return ch

    def train_epoch(self, X, batch, lr, mom, k):
        for s in range(0, len(X), batch):
            self.train_step(X[s:s + batch], lr, mom, k)

    def transform(self, X, k):
        hm = self.chain(X, k)['hm']
        self.call += 1
        return hm

    def free_energy(self, X):
        """mean F(x) over the rows of X"""
        return float(self.rbm.free_energy(X))

    def metrics(self, X, k):
        """(msre, l2_loss, free energy) of the chain from X, in float64"""
        ch = self.chain(X, k)
        self.call += 1
        d = ch['Xin'].astype(np.float64) - ch['vm'].astype(np.float64)
        return float((d * d).mean()), float(self.l2 * 0.5 * (self.p['W'].astype(np.float64) ** 2).sum()), self.free_energy(X)

    def gibbs(self, Hs, n_steps, keep=None):
        """bm_rbm_gibbs: n_steps of v ~ p(v|h), h ~ p(h|v) from the hidden states; keep(t, v): called with every step's v"""
        h = np.ascontiguousarray(Hs, f32)
        v = None
        for t in range(n_steps):
            _, v = self._down(h, self.sample_v, SITE_V + 16 * t)
            _, h = self._up(v, self.sample_h, SITE_H + 16 * t)
            if keep is not None:
                keep(t, v)
        self.call += 1
        return h, v

    def state(self):
        return {n: self.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}


# ---- shared cases of tests/test_softmax_v.py and tests/test_softmax_v_gpu.py
def small_model(seed=11, G=3, K=3, H=3):
    """weights N(0, 1), biases N(0, 0.5^2) of a model small enough to enumerate"""
    rng = np.random.RandomState(seed)
    return dict(W=rng.randn(G * K, H).astype(f32), vb=(0.5 * rng.randn(G * K)).astype(f32), hb=(0.5 * rng.randn(H)).astype(f32))


def all_visible_states(G, K):
    """[K^G][G] every category vector, [K^G][G K] one-hot"""
    cats = np.stack(np.meshgrid(*[np.arange(K)] * G, indexing='ij'), axis=-1).reshape(-1, G)
    return cats, one_hot(cats, K)


def free_energy64(p, X):
    """F(v) = -v.vb - sum_j softplus((v W + hb)_j) per row, in float64"""
    W, vb, hb = (np.asarray(p[n], np.float64) for n in ('W', 'vb', 'hb'))
    X = np.asarray(X, np.float64)
    return -X.dot(vb) - np.logaddexp(0.0, X.dot(W) + hb).sum(axis=1)


def log_z_visible(p, G, K):
    """log Z by enumerating the K^G visible states through the free energy"""
    _, X = all_visible_states(G, K)
    return float(np.logaddexp.reduce(-free_energy64(p, X)))


def log_z_hidden(p, G, K):
    """log Z by enumerating the 2^H hidden states, the groups summed analytically:
    Z = sum_h exp(h.hb) prod_g sum_k exp((W h + vb)_{gK+k})"""
    W, vb, hb = (np.asarray(p[n], np.float64) for n in ('W', 'vb', 'hb'))
    H = W.shape[1]
    terms = []
    for ch in range(1 << H):
        h = np.array([(ch >> b) & 1 for b in range(H)], np.float64)
        l = (W.dot(h) + vb).reshape(G, K)
        terms.append(h.dot(hb) + np.logaddexp.reduce(l, axis=1).sum())
    return float(np.logaddexp.reduce(terms))


def planted_data(n, seed, G=4, K=3, noise=0.1):
    """categories [n][G]: every group a copy of one latent category, replaced by a uniform other category with probability
    `noise`"""
    rng = np.random.RandomState(seed)
    z = rng.randint(0, K, n)
    C_ = np.repeat(z[:, None], G, axis=1)
    flip = rng.uniform(size=C_.shape) < noise
    other = (C_ + rng.randint(1, K, C_.shape)) % K
    return np.where(flip, other, C_)


def shuffled_groups(C_, seed):
    """the same categories with every group's column permuted independently over the rows: the marginals stay, the copies go"""
    rng = np.random.RandomState(seed)
    return np.stack([C_[rng.permutation(len(C_)), g] for g in range(C_.shape[1])], axis=1)


def group_marginals(X, G, K):
    return np.asarray(X, np.float64).reshape(len(X), G, K).mean(axis=0)
