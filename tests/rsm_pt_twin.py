"""CPU twin of parallel tempering and the tempered negative phase over replicated softmax visible units (bm_rbm_rsm_pt_init /
_sweep / _read, bm_rbm_rsm_train_step_pt / _train_epoch_pt), for the tests.

Built from what exists: the ensemble is tests/pt_twin.Ensemble (its swap step and counters are this model's unchanged) with
  * the prop-up, the DB + RT pass in its pinned float32 arithmetic: the raw z = v W is tests/clamp_twin.act2 with kind 1, a unit
    sigma, a zero bias and mult = 1 (the value a raw pass leaves); t = fl(z + fl(D_j hb)), x = fl(beta_j t) in NumPy float32; the
    sigmoid and the draw at flat index (row0 + j) H + i are the oracle's own, reached through act2 with an identity contraction
    (1 * x + 0 = x exactly); the slot partials are pt_twin.slot_partials of h * t with the UNTEMPERED t;
  * the prop-down: softmax_pt_twin.tempered_logits, l = fl(fl(beta_j z) + fl(beta_j vb)), then tests/rsm_twin.softmax_counts (THE
    PREFIX ORDER, draw d of global row r at r max_length + d);
  * the visible half of the swap energy: v.vb in double by the three levels of the prefix order, as a float32 pair (hi, lo) in
    TWO slots, which the swap adds in double like any other slots;
  * the start: D_c tokens uniform over the vocabulary - the count sampler on zero logits at site 11.
The update is tests/rsm_twin's with the two-length hidden-bias sums.  Nothing under oracle/ is involved beyond the calls named.
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from tests import pt_train_twin as PT
from tests import pt_twin as T
from tests import rsm_twin as rt
from tests.clamp_twin import SITE_H, SITE_V, act2
from tests.softmax_pt_twin import NEAR_TIE, ladder, tempered_logits

f32, f64 = np.float32, np.float64
SITE_H0 = PT.SITE_H0
CHUNK = 256


def raw_z(Q, Pk):
    """z = Q Pk as a raw pass of the engine leaves it: (1 * z) * 1 + 0"""
    I = Pk.shape[1]
    return act2(Q, Pk, None, None, np.zeros(I, f32), np.ones(I, f32), 1.0, 1, 0, 0, 0, 0, 0)[0]


def bernoulli_of(x, sample, seed, site, call, row0):
    """(sigmoid(x), its draws) [J][I] with the oracle's sigmoid and uniforms (flat index (row0 + j) I + i): act2 over an identity
    contraction, 256 rows at a time"""
    x = np.ascontiguousarray(x, f32)
    J, I = x.shape
    m, s = np.zeros_like(x), np.zeros_like(x)
    zero = np.zeros(I, f32)
    for j0 in range(0, J, CHUNK):
        n = min(CHUNK, J - j0)
        m[j0:j0 + n], s[j0:j0 + n] = act2(np.eye(n, dtype=f32), x[j0:j0 + n], None, None, zero, None, 1.0, 0, sample, seed, site, call,
                                          int(row0) + j0)
    return m, s


def db_rt_up(v, W, hb, D, mult, sample, seed, site, call, row0):
    """(means, states, t) of the DB + RT pass: t = fl(z + fl(D_j hb)), x = fl(mult_j t)"""
    z = raw_z(v, W)
    t = (z + (np.asarray(D, f32)[:, None] * np.asarray(hb, f32)[None, :]).astype(f32)).astype(f32)
    x = (np.asarray(mult, f32)[:, None] * t).astype(f32)
    m, s = bernoulli_of(x, sample, seed, site, call, row0)
    return m, s, t


def vb_pair(v, vb):
    """[rows][2] float32 (hi, lo) of sum_i double(v_i) double(vb_i) in the double three-level order of the count kernel"""
    v = np.ascontiguousarray(v, f32)
    rows, V = v.shape
    nb = (V + rt.BLOCK - 1) // rt.BLOCK
    p = np.zeros((rows, nb * rt.BLOCK), f64)
    p[:, :V] = v.astype(f64) * np.asarray(vb, f32).astype(f64)[None, :]
    r = np.cumsum(p.reshape(rows, nb, rt.BLOCK // rt.RUN, rt.RUN), axis=3)[..., -1]          # level 0: sequential within a run
    b = np.cumsum(r, axis=2)[..., -1]                                                         # level 1: the runs of a block
    s = np.cumsum(b, axis=1)[:, -1]                                                           # level 2: the blocks
    hi = s.astype(f32)
    lo = (s - hi.astype(f64)).astype(f32)
    return np.stack([hi, lo], axis=1)


def uniform_start(seed, call, row0, D, V, max_length):
    """[rows][V] count rows: D_j tokens uniform over the vocabulary, the count sampler on zero logits at site 11"""
    return rt.softmax_counts(np.zeros((len(D), V), f32), D, 1, seed, T.SITE_PT_V0, call, row0, max_length)[1]


def two_length_bias_sums(D, Dn, h0, hk):
    """s[h] = sum_b fl(fl(D_b h0[b][h]) - fl(Dn_b hk[b][h])), rows in ascending order from 0, every step rounded to float32"""
    h0, hk = np.asarray(h0, f32), np.asarray(hk, f32)
    s = np.zeros(h0.shape[1], f32)
    for b in range(len(h0)):
        s = (s + ((f32(D[b]) * h0[b]).astype(f32) - (f32(Dn[b]) * hk[b]).astype(f32)).astype(f32)).astype(f32)
    return s


def two_length_bias_sums64(D, Dn, h0, hk):
    D, Dn, h0, hk = (np.asarray(a, f64) for a in (D, Dn, h0, hk))
    return (D[:, None] * h0 - Dn[:, None] * hk).sum(axis=0)


class Ensemble(PT.TrainEnsemble):
    """pt_twin.Ensemble over count rows: chain c has the length lengths[c], shared by its R replicas"""

    def __init__(self, p, lengths, betas, seed, max_length, call=0, chain0=0, V0=None):
        V = np.asarray(p['W']).shape[0]
        R = len(np.asarray(betas).ravel())
        self.max_length = int(max_length)
        self.chain_len = np.asarray(lengths, f32).ravel()
        self.len = np.repeat(self.chain_len, R)
        M = len(self.chain_len)
        V0_rows = None
        if V0 is None:
            V0_rows = uniform_start(seed, call, int(chain0) * R, self.len, V, self.max_length)
        else:
            assert np.all(np.asarray(V0, f64).sum(axis=1) == self.chain_len)
        T.Ensemble.__init__(self, p, M, betas, seed, call=call, chain0=chain0, V0=V0, V0_rows=V0_rows)
        self.rescore()

    def rescore(self):
        """rsm_pt_rescore_kernel: the pair of v.vb of the stored counts under the vb of now"""
        self.part_v = vb_pair(self.v, self.vb)

    def sweep(self, n_steps, call=0):
        row0 = self.chain0 * self.R
        for t in range(n_steps):
            _, self.h, tt = db_rt_up(self.v, self.W, self.hb, self.len, self.mult, 1, self.seed, SITE_H + 16 * t, call, row0)
            self.part_h = T.slot_partials(self.h * tt)
            if self.R > 1:
                self._swap(t, call)
            l = tempered_logits(self.h, self.Wt, self.vb, self.mult)
            self.v = self._counts(l, SITE_V + 16 * t, call, row0)
            self.part_v = vb_pair(self.v, self.vb)
            self.step += 1

    def _counts(self, l, site, call, row0):
        """the counts of the logits l [rows][V]: multinomial_counts_kernel's draws"""
        return rt.softmax_counts(l, self.len, 1, self.seed, site, call, row0, self.max_length)[1]

    def near_ties(self):
        return int(np.sum(np.asarray(self.margins) < NEAR_TIE))


def snapshot(e):
    """everything the GPU tests compare of an ensemble, as copies (part_h: None before the first prop-up)"""
    return dict(v=e.v.copy(), h=e.h.copy(), part_v=e.part_v.T.copy(), part_h=None if e.part_h is None else e.part_h.T.copy(),
                mult=e.mult.copy(), idx=e.idx.copy(), swaps=e.cnt.copy(), len=e.len.copy())


def plain_chain(p, V0, D, n_steps, seed, max_length, call=0, row0=0):
    """(v, h) after n_steps of h ~ p(h|v), v ~ p(v|h) from V0: the single-temperature chain of tests/rsm_twin, both layers sampled"""
    v = np.ascontiguousarray(V0, f32)
    h = None
    for t in range(n_steps):
        _, h = rt.db_up(v, p['W'], p['hb'], D, 1, seed, SITE_H + 16 * t, call, row0)
        _, v = rt.visible_pass(h, p['W'], p['vb'], D, 1, seed, SITE_V + 16 * t, call, row0, max_length)
    return v, h


class TemperedRsmRBM(object):
    """CPU twin of one bm_rbm handle with the unit that trains through bm_rbm_rsm_train_step_pt"""

    def __init__(self, p, lengths, betas, seed, max_length, call=0, **cfg):
        V, H = p['W'].shape
        self.rbm = orc.OracleRBM(V, H, **cfg)
        for n in ('W', 'vb', 'hb'):
            self.rbm.p[n][...] = p[n]
        self.seed, self.call = int(seed), int(call)
        self.ens = Ensemble(self.rbm.p, lengths, betas, self.seed, max_length, call=self.call)

    @property
    def p(self):
        return self.rbm.p

    def train_step(self, X, lr, momentum, k):
        X = np.ascontiguousarray(X, f32)
        B, p, e = len(X), self.rbm.p, self.ens
        assert 1 <= B <= e.M and k >= 1
        e.set_params(p)
        e.rescore()                                                             # 1.
        D = rt.lengths(X)
        h0m = rt.db_up(X, p['W'], p['hb'], D, 0, self.seed, SITE_H0, self.call)[0]          # 2.
        e.sweep(k, call=self.call)                                              # 3.
        vs = np.ascontiguousarray(e.read()[0][:B])                              # 4.
        Dn = e.chain_len[:B]
        hm = rt.db_up(vs, p['W'], p['hb'], Dn, 0, self.seed, SITE_H, self.call)[0]          # 5.
        z = np.zeros((B, max(e.V, e.H)), f32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        h0m, hm = np.ascontiguousarray(h0m, f32), np.ascontiguousarray(hm, f32)
        w = orc.RbmWork(ptr(X), ptr(h0m), ptr(z), ptr(z), ptr(vs), ptr(hm), ptr(z))
        raw = np.zeros(e.V * e.H + e.V + 2 * e.H, f32)
        orc.lib().orc_rbm_raw_grads(C.byref(self.rbm.cfg), C.byref(w), B, raw)  # 6.
        o = e.V * e.H + e.V
        raw[o:o + e.H] = two_length_bias_sums(D, Dn, h0m, hm)
        self.rbm.apply(raw, float(B), lr, momentum)
        self.call += 1                                                          # 7.
        self.rbm.call = self.call

    def train_epoch(self, X, batch, lr, momentum, k):
        for s in range(0, len(X), batch):
            self.train_step(X[s:s + batch], lr, momentum, k)

    def state(self):
        out = {n: self.rbm.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}
        out.update(snapshot(self.ens))
        return out


# ---- ground truth by enumeration
def exact_joint(p, D, beta=1.0):
    """(X [C][V] count vectors of length D, Hs [2^H][H], P [C][2^H]): p_beta(v, h) ~ (D!/prod v_i!) exp(beta (v W h + v.vb + D h.hb))"""
    W, vb, hb = (np.asarray(p[n], f64) for n in ('W', 'vb', 'hb'))
    X, logc = rt.count_vectors(W.shape[0], D)
    H = W.shape[1]
    Hs = ((np.arange(1 << H)[:, None] >> np.arange(H)[None, :]) & 1).astype(f64)
    logp = logc[:, None] + beta * (X.dot(vb)[:, None] + D * Hs.dot(hb)[None, :] + X.dot(W).dot(Hs.T))
    P = np.exp(logp - logp.max())
    return X, Hs, P / P.sum()


def exact_pv_beta(p, D, beta):
    X, _, P = exact_joint(p, D, beta)
    return X, P.sum(axis=1)


def exact_vh(p, D):
    """E[v_i h_j] under p(v, h) at length D, [V][H]"""
    X, Hs, P = exact_joint(p, D)
    return X.T.dot(P).dot(Hs)


def two_topic_model(V=4, H=2, w=4.0, tilt=0.3):
    """Two well-separated topics over a vocabulary of two halves: hidden unit 0 stands for topic A (the first half), hidden unit
    1 for topic B.  W[i][0] = +w, W[i][1] = -w on the first half and the reverse on the second; hb = 0; vb tilts topic B"""
    half = V // 2
    W = np.zeros((V, H), f32)
    W[:half, 0], W[:half, 1] = w, -w
    W[half:, 0], W[half:, 1] = -w, w
    vb = np.zeros(V, f32)
    vb[half:] = tilt
    return dict(W=W, vb=vb, hb=np.zeros(H, f32))


def topic_mass(p, D):
    """exact P(more than half of the D tokens lie in the second half of the vocabulary)"""
    X, pv = rt.exact_pv(p, D)
    half = X.shape[1] // 2
    return float(pv[X[:, half:].sum(axis=1) > D / 2.0].sum())


# ---- shared cases of tests/test_rsm_pt.py and tests/test_rsm_pt_gpu.py
def make_params(V, H, seed=7, std=0.5):
    return dict(W=(orc.normal(4711, seed, 0, V * H) * f32(std)).reshape(V, H), vb=orc.normal(4711, seed + 1, 0, V) * f32(0.5),
                hb=orc.normal(4711, seed + 2, 0, H) * f32(0.05))


def chain_lengths(M, max_length, seed=1):
    """M lengths in [1, max_length], mixed, D = 1 and D = max_length among them where M allows it"""
    D = 1 + np.minimum((orc.uniform(4711, 70 + seed, 0, M) * max_length).astype(np.int64), max_length - 1)
    if M >= 2:
        D[0] = 1
        D[-1] = max_length
    return D.astype(f32)


MAX_LENGTH = 24
# (V, H, M, R): every V, every H and every (M, R) at least once - the marginals, not the cross product - and V = 4097 (the
# four-runs-per-thread count kernel) with every H and every (M, R); all of them are compared bit for bit
SWEEP_CASES = [(2, 16, 3, 4), (16, 17, 33, 2), (17, 40, 1, 1), (256, 16, 3, 4), (257, 17, 33, 2), (4096, 40, 3, 4), (4097, 16, 3, 4),
               (17, 16, 1, 1), (256, 40, 33, 2), (4097, 17, 33, 2), (4097, 40, 1, 1), (4096, 17, 33, 2)]
SWEEP_SEED, SWEEP_CALL, SWEEP_CHAIN0 = 9300, 0, 11
TRAIN_CASES = [(17, 16, 6, 3), (257, 40, 9, 2)]
TRAIN_SEED = 9400


def case_id(c):
    return 'x'.join(str(x) for x in c)


def sweep_lengths(M, chain0):
    """the lengths of the chains [chain0, chain0 + M) of one long list: a slice of chains keeps its chains' lengths"""
    L = chain_lengths(64, MAX_LENGTH)
    L[1::5], L[3::5] = 1, MAX_LENGTH               # (D = 1 and D = max_length inside every window of three chains at chain0 = 11)
    return L[chain0:chain0 + M].copy()


def sweep_twin(c, seed=SWEEP_SEED, call=SWEEP_CALL, chain0=SWEEP_CHAIN0, V0=None, lengths=None):
    """(the twin, its snapshots at the start, after a sweep of 2 steps at call `call` and after one of 2 more at `call + 1`)"""
    V, H, M, R = c
    D = sweep_lengths(M, chain0) if lengths is None else lengths
    e = Ensemble(make_params(V, H), D, ladder(R), seed, MAX_LENGTH, call=call, chain0=chain0, V0=V0)
    snaps = [snapshot(e)]
    e.sweep(2, call=call)
    snaps.append(snapshot(e))
    e.sweep(2, call=call + 1)
    snaps.append(snapshot(e))
    return e, snaps


def train_batches(V, n, seed, max_length=MAX_LENGTH):
    """count rows [n][V] of mixed lengths from the pinned stream"""
    D = chain_lengths(n, max_length, seed=seed + 5)
    return rt.softmax_counts(np.zeros((n, V), f32), D, 1, 4711, 90 + seed, 0, 0, max_length)[1]
