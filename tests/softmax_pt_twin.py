"""CPU twin of parallel tempering and the tempered negative phase over softmax visible units (bm_rbm_groups_pt_init / _sweep /
_read, bm_rbm_groups_train_step_pt / _train_epoch_pt), for the tests.

Built from what exists: the ensemble is tests/pt_twin.Ensemble (its prop-up, its swap step, its slot partials and counters are
this model's unchanged) with two parts replaced:
  * the prop-down: the raw z = h W^T is tests/clamp_twin.act2 with kind 1, sigma = ones, a zero bias and mult = 1 - (1 * z) * 1 + 0,
    the value a raw pass of the engine leaves; the logits are the pinned float32 arithmetic l = fl(fl(beta_j z) + fl(beta_j vb)), two
    NumPy float32 multiplies and one add with the row's own temperature; means, uniforms and the one-hot draw are
    tests/softmax_v_twin.softmax_groups / group_uniforms (the oracle's pinned softmax prefix);
  * the start: one uniform category per group by the same rule with zero logits (e = 1, c[k] = k + 1, S = K, the first k with
    c[k] > u K), u at flat index (row0 + row) V + g K of site 11.
The update is tests/pt_train_twin's: orc_rbm_raw_grads on a hand-filled work struct, then orc_rbm_apply.
"""
import numpy as np

from oracle import oracle as orc
from tests import pt_train_twin as PT
from tests import pt_twin as T
from tests import softmax_v_twin as SV
from tests.clamp_twin import SITE_H, act2

f32 = np.float32
SITE_H0 = PT.SITE_H0
NEAR_TIE = 1e-9                       # a swap draw this close to its threshold may go the other way on the device


def categorical_start(seed, call, row0, rows, V, K):
    """[rows][V] one-hot: the start of softmax_pt_init_kernel without a V0"""
    u = SV.group_uniforms(seed, T.SITE_PT_V0, call, row0, rows, V, K)                    # [rows][G]
    t = (u * f32(K)).astype(f32)[:, :, None]
    c = np.arange(1, K + 1, dtype=f32)[None, None, :]
    s = ((c > t) & ~((c - f32(1)) > t)).astype(f32)
    return s.reshape(rows, V)


def tempered_logits(h, Wt, vb, mult):
    """l [J][V] = fl(fl(beta_j z) + fl(beta_j vb)), z = h W^T as a raw pass leaves it, beta_j = mult[j]"""
    V = Wt.shape[1]
    z, _ = act2(h, Wt, None, None, np.zeros(V, f32), np.ones(V, f32), 1.0, 1, 0, 0, 0, 0, 0)
    b = np.ascontiguousarray(mult, f32)[:, None]
    bz = (b * z).astype(f32)
    bb = (b * np.ascontiguousarray(vb, f32)[None, :]).astype(f32)
    return (bz + bb).astype(f32)


class Ensemble(PT.TrainEnsemble):
    """pt_twin.Ensemble over one-hot groups of K (with pt_train_twin's set_params / rescore)"""

    def __init__(self, p, K, n_chains, betas, seed, call=0, chain0=0, V0=None, V0_rows=None):
        V = np.asarray(p['W']).shape[0]
        R = len(np.asarray(betas).ravel())
        assert V % K == 0
        self.K = int(K)
        if V0 is None and V0_rows is None:
            V0_rows = categorical_start(seed, call, int(chain0) * R, int(n_chains) * R, V, self.K)
        T.Ensemble.__init__(self, p, n_chains, betas, seed, call=call, chain0=chain0, V0=V0, V0_rows=V0_rows)

    def _tempered(self, Q, Pk, bias, site, call):
        if Pk is not self.Wt:                    # the prop-up: the Bernoulli row-tempered pass, unchanged
            return T.Ensemble._tempered(self, Q, Pk, bias, site, call)
        l = tempered_logits(Q, Pk, bias, self.mult)
        u = SV.group_uniforms(self.seed, site, call, self.chain0 * self.R, l.shape[0], self.V, self.K)
        return SV.softmax_groups(l, self.K, 1, u)[1]

    def near_ties(self):
        """the swap draws of every sweep so far that lie within NEAR_TIE of their threshold"""
        return int(np.sum(np.asarray(self.margins) < NEAR_TIE))


def plain_chain(p, K, V0, n_steps, seed, call=0, row0=0):
    """(v, h) after n_steps of h ~ p(h|v), v ~ p(v|h) from V0: the single-temperature chain of tests/softmax_v_twin, both layers
    sampled (sites SITE_H + 16 t, SITE_V + 16 t)"""
    v = np.ascontiguousarray(V0, f32)
    h = None
    for t in range(n_steps):
        _, h = act2(v, p['W'], None, None, p['hb'], None, 1.0, 0, 1, seed, SITE_H + 16 * t, call, row0)
        _, v = SV.visible_pass(h, p['W'], p['vb'], K, 1, seed, SV.SITE_V + 16 * t, call, row0)
    return v, h


class TemperedCategoricalRBM(PT.TemperedRBM):
    """CPU twin of one bm_rbm handle with visible groups that trains through bm_rbm_groups_train_step_pt"""

    def __init__(self, p, K, n_chains, betas, seed, call=0, **cfg):
        V, H = p['W'].shape
        self.rbm = orc.OracleRBM(V, H, **cfg)
        for n in ('W', 'vb', 'hb'):
            self.rbm.p[n][...] = p[n]
        self.seed, self.call, self.K = int(seed), int(call), int(K)
        self.ens = Ensemble(self.rbm.p, K, n_chains, betas, seed=self.seed, call=self.call)

    def state(self):
        """the variables, the momentum buffers and the ensemble's snapshot"""
        out = {n: self.rbm.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}
        out.update(snapshot(self.ens))
        return out


# ---- ground truth by enumeration
def exact_tempered_joint(p, G, K, beta):
    """(X [K^G][V] one-hot, Hs [2^H][H], P [K^G][2^H]): p_beta(v, h) ~ exp(beta (v.vb + h.hb + v W h)) in float64"""
    W, vb, hb = (np.asarray(p[n], np.float64) for n in ('W', 'vb', 'hb'))
    _, X = SV.all_visible_states(G, K)
    X = X.astype(np.float64)
    H = W.shape[1]
    Hs = ((np.arange(1 << H)[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
    logp = beta * (X.dot(vb)[:, None] + Hs.dot(hb)[None, :] + X.dot(W).dot(Hs.T))
    P = np.exp(logp - logp.max())
    return X, Hs, P / P.sum()


def exact_vh(p, G, K):
    """E[v_i h_j] under p(v, h), [V][H]"""
    X, Hs, P = exact_tempered_joint(p, G, K, 1.0)
    return X.T.dot(P).dot(Hs)


def two_mode_model(G=3, K=3, H=4, w=4.0, tilt=0.15):
    """Two well-separated modes that differ in every group: category 0 everywhere with h = 0, category 1 everywhere with h = 1.
    W[gK + 1][:] = w, W[gK][:] = 0 and hb = -w G / 2 make the hidden units follow the number of groups at category 1; vb[gK] =
    w H / 2 balances the two modes, vb[gK + 1] = tilt makes the second one the heavier; the other categories sit at -3"""
    V = G * K
    W, vb = np.zeros((V, H), f32), np.full(V, -3.0, f32)
    for g in range(G):
        W[g * K + 1, :] = w
        vb[g * K] = w * H / 2
        vb[g * K + 1] = tilt
    return dict(W=W, vb=vb, hb=np.full(H, -w * G / 2, f32))


def mode_mass(p, G, K, cat, least):
    """exact P(at least `least` of the G groups are at category `cat`)"""
    X, _, P = exact_tempered_joint(p, G, K, 1.0)
    n = X.reshape(len(X), G, K)[:, :, cat].sum(axis=1)
    return float(P.sum(axis=1)[n >= least].sum())


# ---- shared cases of tests/test_softmax_pt.py and tests/test_softmax_pt_gpu.py
def make_params(G, K, H, seed=7, std=0.5):
    V = G * K
    return dict(W=(orc.normal(4711, seed, 0, V * H) * f32(std)).reshape(V, H), vb=orc.normal(4711, seed + 1, 0, V) * f32(0.5),
                hb=orc.normal(4711, seed + 2, 0, H) * f32(0.5))


def ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(f32)


FUSED_SHAPES = [(5, 4), (3, 16), (9, 8), (34, 2)]
GENERIC_SHAPES = [(4, 3), (3, 5)]
HIDDEN = [8, 24, 40]
ENSEMBLES = [(5, 3), (33, 4), (7, 1)]
# (G, K, H, M, R): every shape, every H and every (M, R) at least once; all of them are compared bit for bit
SWEEP_CASES = [(5, 4, 8, 5, 3), (5, 4, 24, 33, 4), (5, 4, 40, 7, 1), (3, 16, 24, 5, 3), (9, 8, 40, 33, 4), (34, 2, 8, 7, 1),
               (34, 2, 24, 5, 3), (4, 3, 8, 33, 4), (4, 3, 40, 5, 3), (3, 5, 24, 5, 3), (3, 5, 8, 7, 1), (3, 16, 8, 33, 4)]
SWEEP_SEED, SWEEP_CALL, SWEEP_CHAIN0 = 9100, 0, 11      # (bm_rbm_seed resets the call counter: the sweeps are calls 0 and 1)
TRAIN_CASES = [(5, 4, 24, 6, 3), (9, 8, 40, 9, 4), (3, 5, 8, 6, 3)]        # fused, fused across a column tile, generic
TRAIN_SEED = 9200


def case_id(c):
    return 'x'.join(str(x) for x in c)


def snapshot(e):
    """everything the GPU tests compare of an ensemble, as copies (part_h: None before the first prop-up)"""
    return dict(v=e.v.copy(), h=e.h.copy(), part_v=e.part_v.T.copy(), part_h=None if e.part_h is None else e.part_h.T.copy(),
                mult=e.mult.copy(), idx=e.idx.copy(), swaps=e.cnt.copy())


def sweep_twin(c, seed=SWEEP_SEED, call=SWEEP_CALL, chain0=SWEEP_CHAIN0, V0=None, M=None):
    """(the twin, its snapshots at the start, after a sweep of 3 steps at call `call` and after one of 2 more at `call + 1`)"""
    G, K, H, M_, R = c
    e = Ensemble(make_params(G, K, H), K, M_ if M is None else M, ladder(R), seed, call=call, chain0=chain0, V0=V0)
    snaps = [snapshot(e)]
    e.sweep(3, call=call)
    snaps.append(snapshot(e))
    e.sweep(2, call=call + 1)
    snaps.append(snapshot(e))
    return e, snaps


def train_batches(G, K, n, seed):
    """one-hot rows [n][G K] with uniform categories from the pinned stream"""
    cats = np.minimum((orc.uniform(4711, 50 + seed, 0, n * G).reshape(n, G) * K).astype(np.int64), K - 1)
    return SV.one_hot(cats, K)
