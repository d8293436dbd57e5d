"""CPU twin of an RBM with replicated softmax visible units (bm_rbm_set_replicated_softmax; csrc/bm_rsm.h), for
the tests.

Built from what exists, in the style of tests/softmax_v_twin.py:
  * the DB pre-activation.  Row j of the hidden pass is tests/clamp_twin.act2 on that row alone with kind 0, mult = bmult = 1 and
    the bias vector fl(D_j * hb) (one float32 NumPy product per unit) at row offset row0 + j: t = 1 * z + 1 * fl(D_j hb_i) - the
    two rounded steps of the DB flavour - then the oracle's sigmoid and its draw at flat index (row0 + j) * H + i;
  * the visible pass.  The logits l = h W^T + vb are softmax_v_twin.logits (a kind-3 pass); e[i] = exp_neg(min(mx - l[i], 80))
    comes from the oracle's pinned softmax row (orc_softmax_prefix at I = V, whose own sequential prefix sums are NOT used);
    the prefix sums follow THE PREFIX ORDER, restated in prefix_order(); mean = fl(D * fl(e / S)); draw d of global row r reads
    the uniform at flat index r * max_length + d of the pass's stream, t = fl(u * S), and lands on the smallest i with c[i] > t
    (c is non-decreasing, so a bisection and np.searchsorted(side='right') agree), clamped to V - 1;
  * the update: orc_rbm_raw_grads on a hand-filled work struct, the hidden-bias sums replaced by the length-weighted ones
    (weighted_bias_sums: rows in ascending order), then orc_rbm_apply through OracleRBM.
Nothing under oracle/ is involved beyond the calls named above.
"""
import ctypes as C
from math import lgamma

import numpy as np

from oracle import oracle as orc
from tests.clamp_twin import SITE_H, SITE_V, act2
from tests.multinomial_probes import prefix as _seq_prefix
from tests.softmax_v_twin import SITE_H0, logits

f32 = np.float32
RUN, BLOCK = 16, 256          # the levels of the prefix order: runs of 16 units, blocks of 16 runs
MAX_V = 16384


def lengths(X):
    """D[j] = sum_i X[j][i]: integers below 2^24, exact in float32 in any order"""
    return np.asarray(X, np.float64).sum(axis=1).astype(f32)


def softmax_e(l):
    """e[i] = exp_neg(min(max(l) - l[i], 80)) of one row of logits"""
    return _seq_prefix(np.ascontiguousarray(l, f32))[0]


def prefix_order(e):
    """c [V] of e [V] in THE PREFIX ORDER (csrc/bm_rsm.h), a function of V alone; e is padded with zeros to whole blocks:
      level 0  within each aligned run of 16 units: r_k = r_{k-1} + e_k sequentially
      level 1  within each aligned block of 16 runs with totals T_q = r_15: O_0 = 0, O_q = O_{q-1} + T_{q-1} sequentially;
               local[q][k] = O_q + r_k
      level 2  over the blocks in ascending order: base_0 = 0, base_b = base_{b-1} + local_{b-1}[15][15];
               c = base_b + local_b[q][k]
    np.cumsum along an axis of a float32 array accumulates sequentially in float32"""
    e = np.ascontiguousarray(e, f32)
    V = len(e)
    nb = (V + BLOCK - 1) // BLOCK
    p = np.zeros(nb * BLOCK, f32)
    p[:V] = e
    r = np.cumsum(p.reshape(nb, BLOCK // RUN, RUN), axis=2, dtype=f32)
    T = r[:, :, RUN - 1]
    incl = np.cumsum(T, axis=1, dtype=f32)                    # O_q + T_q
    O = np.concatenate([np.zeros((nb, 1), f32), incl[:, :-1]], axis=1)
    local = (O[:, :, None] + r).astype(f32)
    tot = local[:, -1, -1]
    base = np.concatenate([np.zeros(1, f32), np.cumsum(tot, dtype=f32)[:-1]]) if nb > 1 else np.zeros(1, f32)
    # (np.cumsum(tot) IS base_b + tot_b step by step: base_{b+1} = base_b + tot_b)
    return (base[:, None, None] + local).astype(f32).reshape(-1)[:V]


def level_boundaries(vmax=MAX_V):
    """the widths at which the prefix order takes another path: every run and block edge's neighbourhood that tests can afford -
    the first edges of each level and the last block edge, each +- 1"""
    edges = [RUN, 2 * RUN, BLOCK, 2 * BLOCK, 16 * BLOCK, 17 * BLOCK, vmax - BLOCK, vmax]
    out = sorted({v for e in edges for v in (e - 1, e, e + 1) if 2 <= v <= vmax})
    return out


def softmax_counts(L, D, sample, seed, site, call, row0, max_length):
    """(means, states) [J][V] of the logits L [J][V] and the lengths D [J]: multinomial_counts_kernel"""
    L = np.ascontiguousarray(L, f32)
    J, V = L.shape
    D = np.asarray(D, f32)
    means, states = np.zeros_like(L), np.zeros_like(L)
    for j in range(J):
        e = softmax_e(L[j])
        c = prefix_order(e)
        S = c[V - 1]
        means[j] = (D[j] * (e / S).astype(f32)).astype(f32)
        if not sample:
            states[j] = means[j]
            continue
        n = int(D[j])
        u = orc.uniform(int(seed), int(site), int(call), n, idx0=(int(row0) + j) * int(max_length))
        t = (u * S).astype(f32)
        cat = np.minimum(np.searchsorted(c, t, side='right'), V - 1)
        states[j] = np.bincount(cat, minlength=V).astype(f32)
    return means, states


def db_up(v, W, hb, D, sample, seed, site, call, row0=0):
    """(means, states) [J][H] of the hidden layer given count rows v [J][V] with lengths D [J]: the DB flavour, row by row"""
    v = np.ascontiguousarray(v, f32)
    hb = np.asarray(hb, f32)
    m, s = [], []
    for j in range(len(v)):
        bj = (f32(D[j]) * hb).astype(f32)                      # __fmul_rn(row_bmult[j], bias[i])
        mj, sj = act2(v[j:j + 1], W, None, None, bj, None, 1.0, 0, sample, seed, site, call, int(row0) + j)
        m.append(mj[0]); s.append(sj[0])
    return np.stack(m), np.stack(s)


def visible_pass(h, W, vb, D, sample, seed, site, call, row0, max_length):
    return softmax_counts(logits(h, W, vb), D, sample, seed, site, call, row0, max_length)


def weighted_bias_sums(D, h0, hk):
    """s[h] = sum_b fl(D_b * fl(h0[b][h] - hk[b][h])), rows in ascending order, every step rounded to float32"""
    h0, hk = np.asarray(h0, f32), np.asarray(hk, f32)
    s = np.zeros(h0.shape[1], f32)
    for b in range(len(h0)):
        s = (s + (f32(D[b]) * (h0[b] - hk[b]).astype(f32)).astype(f32)).astype(f32)
    return s


class RsmRBM(object):
    """CPU twin of one bm_rbm handle after bm_rbm_set_replicated_softmax(max_length): `rbm` is an oracle.OracleRBM that holds the
    variables and applies the update; the chain is restated here"""

    def __init__(self, p0, max_length, seed, l2=1e-4, sample_v_states=False, sample_h_states=True):
        V, H = p0['W'].shape
        self.V, self.H, self.max_length = V, H, int(max_length)
        self.rbm = orc.OracleRBM(V, H, l2=l2, sample_v_states=sample_v_states, sample_h_states=sample_h_states)
        for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means'):
            if n in p0:
                self.rbm.p[n][...] = p0[n]
        self.seed, self.call, self.row0, self.l2 = int(seed), 0, 0, l2
        self.draw_v, self.draw_h = int(bool(sample_v_states)), int(bool(sample_h_states))

    @property
    def p(self):
        return self.rbm.p

    def set_seed(self, seed):
        self.seed, self.call = int(seed), 0

    def _up(self, v, D, sample, site):
        return db_up(v, self.p['W'], self.p['hb'], D, sample, self.seed, site, self.call, self.row0)

    def _down(self, h, D, sample, site):
        return visible_pass(h, self.p['W'], self.p['vb'], D, sample, self.seed, site, self.call, self.row0, self.max_length)

    def chain(self, X, k):
        """the lengths come from the batch, once; every pass of the chain keeps them"""
        Xin = np.ascontiguousarray(X, f32)
        D = lengths(Xin)
        h0m, h0s = self._up(Xin, D, 1, SITE_H0)
        hstate = h0s if self.draw_h else h0m
        vm = vs = hm = None
        for t in range(k):
            vm, vs = self._down(hstate, D, self.draw_v, SITE_V + 16 * t)
            hm, hs = self._up(vs, D, self.draw_h, SITE_H + 16 * t)
            hstate = hs
        return dict(Xin=Xin, D=D, h0m=h0m, h0s=h0s, vm=vm, vs=vs, hm=hm)

    def train_step(self, X, lr, mom, k):
        ch = self.chain(X, k)
        B = len(ch['Xin'])
        Xin, h0m, vs, hm = (np.ascontiguousarray(ch[n], f32) for n in ('Xin', 'h0m', 'vs', 'hm'))
        z = np.zeros((B, max(self.V, self.H)), f32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        w = orc.RbmWork(ptr(Xin), ptr(h0m), ptr(z), ptr(z), ptr(vs), ptr(hm), ptr(z))
        raw = np.zeros(self.V * self.H + self.V + 2 * self.H, f32)
        orc.lib().orc_rbm_raw_grads(C.byref(self.rbm.cfg), C.byref(w), B, raw)
        o = self.V * self.H + self.V
        raw[o:o + self.H] = weighted_bias_sums(ch['D'], h0m, hm)      # sum_b D_b (h0_b - hk_b) in place of the plain column sums
        self.rbm.apply(raw, float(B), lr, mom)
        self.call += 1
        return ch

    def transform(self, X, k):
        hm = self.chain(X, k)['hm']
        self.call += 1
        return hm

    def sample_h(self, X):
        """bm_rbm_sample_h: (means, states), the lengths from the input rows"""
        X = np.ascontiguousarray(X, f32)
        out = self._up(X, lengths(X), 1, SITE_H0)
        self.call += 1
        return out

    def sample_v_from_h(self, Hs, D):
        """bm_rbm_sample_v_from_h: (means, states) with the caller's lengths"""
        out = self._down(np.ascontiguousarray(Hs, f32), D, 1, SITE_V)
        self.call += 1
        return out

    def gibbs(self, Hs, D, n_steps, keep=None):
        """bm_rbm_gibbs with the caller's lengths: n_steps of v ~ p(v|h), h ~ p(h|v) from the hidden states"""
        h = np.ascontiguousarray(Hs, f32)
        v = None
        for t in range(n_steps):
            _, v = self._down(h, D, self.draw_v, SITE_V + 16 * t)
            _, h = self._up(v, D, self.draw_h, SITE_H + 16 * t)
            if keep is not None:
                keep(t, v)
        self.call += 1
        return h, v

    def sample_v(self, V0, D, n_steps, keep=None):
        """ReplicatedSoftmaxRBM.sample_v on one slice: sample_h, then n_steps of (sample_v_from_h, sample_h), both layers drawn"""
        _, h = self.sample_h(V0)
        v = None
        for t in range(n_steps):
            _, v = self.sample_v_from_h(h, D)
            _, h = self.sample_h(v)
            if keep is not None:
                keep(t, v)
        return v

    def state(self):
        return {n: self.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}


# ---- float64 helpers
def free_energy64(p, X):
    """F(v) = -v.vb - sum_j softplus(D hb_j + (v W)_j) per row, in float64"""
    W, vb, hb = (np.asarray(p[n], np.float64) for n in ('W', 'vb', 'hb'))
    X = np.asarray(X, np.float64)
    D = X.sum(axis=1, keepdims=True)
    return -X.dot(vb) - np.logaddexp(0.0, X.dot(W) + D * hb).sum(axis=1)


def count_vectors(V, D):
    """every count vector of length D over V words, [C(D+V-1, V-1)][V] float64, and the log of its multinomial coefficient
    D! / prod_i v_i!"""
    out = []

    def rec(prefix, left, slots):
        if slots == 1:
            out.append(prefix + [left])
            return
        for n in range(left, -1, -1):
            rec(prefix + [n], left - n, slots - 1)
    rec([], int(D), int(V))
    X = np.array(out, np.float64)
    logc = np.array([lgamma(D + 1) - sum(lgamma(n + 1) for n in row) for row in out])
    return X, logc


def log_z_visible(p, D):
    """log Z_D = log sum_v (D! / prod v_i!) exp(-F(v)) over the count vectors of length D"""
    X, logc = count_vectors(p['W'].shape[0], D)
    return float(np.logaddexp.reduce(logc - free_energy64(p, X)))


def log_z_hidden(p, D):
    """log Z_D over the 2^H hidden states, the counts summed by the multinomial theorem:
    Z_D = sum_h exp(D h.hb) (sum_i exp(vb_i + (W h)_i))^D"""
    W, vb, hb = (np.asarray(p[n], np.float64) for n in ('W', 'vb', 'hb'))
    H = W.shape[1]
    terms = []
    for ch in range(1 << H):
        h = np.array([(ch >> b) & 1 for b in range(H)], np.float64)
        terms.append(D * h.dot(hb) + D * np.logaddexp.reduce(vb + W.dot(h)))
    return float(np.logaddexp.reduce(terms))


def exact_pv(p, D):
    """(X, p(v)) over the count vectors of length D"""
    X, logc = count_vectors(p['W'].shape[0], D)
    lp = logc - free_energy64(p, X)
    return X, np.exp(lp - np.logaddexp.reduce(lp))


# ---- shared cases of tests/test_rsm.py and tests/test_rsm_gpu.py
def small_model(seed=23, V=4, H=2):
    """weights N(0, 1), biases N(0, 0.5^2) / N(0, 0.25^2) of a model small enough to enumerate"""
    rng = np.random.RandomState(seed)
    return dict(W=rng.randn(V, H).astype(f32), vb=(0.5 * rng.randn(V)).astype(f32), hb=(0.25 * rng.randn(H)).astype(f32))


def cell_index(X, states):
    """the row of X (all count vectors) that every state row equals"""
    key = {tuple(int(n) for n in row): i for i, row in enumerate(X)}
    return np.array([key[tuple(int(n) for n in row)] for row in states])


def chi_square_z(counts, probs):
    """z = (chi2 - dof) / sqrt(2 dof) of cell counts against their exact probabilities"""
    n = counts.sum()
    ex = n * probs
    assert ex.min() >= 5.0, ex.min()
    chi2 = float(((counts - ex) ** 2 / ex).sum())
    dof = len(probs) - 1
    return (chi2 - dof) / np.sqrt(2.0 * dof), ex.min()


def planted_corpus(n, seed, V=24, D_lo=10, D_hi=30):
    """a two-topic corpus: every document draws its D in [D_lo, D_hi] tokens from one of two topics, each putting 90 % of its
    mass on its own half of the vocabulary -> (count rows [n][V] float32, topics [n])"""
    rng = np.random.RandomState(seed)
    half = V // 2
    topics = rng.randint(0, 2, n)
    X = np.zeros((n, V), f32)
    for b in range(n):
        pw = np.full(V, 0.1 / half)
        pw[topics[b] * half:(topics[b] + 1) * half] = 0.9 / half
        X[b] = rng.multinomial(rng.randint(D_lo, D_hi + 1), pw)
    return X, topics


def shuffled_vocabulary(X, seed):
    """the same documents with every row's counts permuted over the vocabulary independently: the lengths stay, the topics go"""
    rng = np.random.RandomState(seed)
    return np.stack([row[rng.permutation(len(row))] for row in X]).astype(f32)
