"""CPU twin of the parallel-tempering sweeps (bm_rbm_pt_init / _sweep / _read), for the tests.

States come from the oracle library's activation stage (orc_act2 through tests/clamp_twin.act2: what act_kernel computes),
called once per distinct temperature with mult = bmult = beta and the engine's seed / site / call / row0 - only the rows that
are at that temperature are kept.  The untempered pre-activations z + b come from one more call with kind = 2, mult = 1 and a
unit sigma (its `means` are float32(z * 1 + b)).  The slot partials are restated in NumPy float32 in the order of DESIGN.md 3.4
(quads of 4 columns left to right, then (q0 + q1) + (q2 + q3) per 16-column slot), the swap uniforms come from
boltzmann_machines_amd/utils/philox.py, the acceptance rule is evaluated in float64.  Nothing under oracle/ is involved beyond
those calls.
"""
import numpy as np

from boltzmann_machines_amd.utils import philox
from tests.clamp_twin import SITE_H, SITE_V, act2

SITE_PT_SWAP, SITE_PT_V0 = 10, 11      # csrc/bm_rbm.hip


def slot_partials(P):
    """P [rows][I] float32 terms -> [rows][ceil(I/16)] float32 slot sums in the epilogue's order"""
    P = np.ascontiguousarray(P, np.float32)
    rows, I = P.shape
    ns = (I + 15) // 16
    X = np.zeros((rows, ns * 16), np.float32)
    X[:, :I] = P
    X = X.reshape(rows, ns, 4, 4)
    q = ((X[..., 0] + X[..., 1]) + X[..., 2]) + X[..., 3]
    return ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])).astype(np.float32)


def slot_sum(part, s=None):
    """[rows][nslot] float32 -> [rows] float64, the slots added in ascending order (onto the running sums `s`, if given)"""
    s = np.zeros(part.shape[0], np.float64) if s is None else s
    for q in range(part.shape[1]):
        s = s + part[:, q].astype(np.float64)
    return s


class Ensemble(object):
    """M chains x R replicas, chain-major rows (row c R + r is slot r of chain c)"""

    def __init__(self, p, n_chains, betas, seed, call=0, chain0=0, V0=None, V0_rows=None):
        """p: dict W [V][H], vb, hb.  V0 [M][V]: every chain's replicas start there; V0_rows [M R][V] (twin only): every row
        its own start; neither: v_0 ~ Ber(1/2) at site 11 of `call`"""
        self.W = np.ascontiguousarray(p['W'], np.float32)
        self.Wt = np.ascontiguousarray(self.W.T)
        self.vb, self.hb = np.ascontiguousarray(p['vb'], np.float32), np.ascontiguousarray(p['hb'], np.float32)
        self.V, self.H = self.W.shape
        self.betas = np.ascontiguousarray(betas, np.float32).ravel()
        self.M, self.R, self.seed, self.chain0 = int(n_chains), len(self.betas), int(seed), int(chain0)
        rows = self.M * self.R
        if V0_rows is not None:
            v = np.ascontiguousarray(V0_rows, np.float32).copy()
        elif V0 is not None:
            v = np.repeat(np.ascontiguousarray(V0, np.float32), self.R, axis=0)
        else:
            u = philox.uniform(seed, SITE_PT_V0, call, rows * self.V, idx0=self.chain0 * self.R * self.V)
            v = (u < np.float32(0.5)).astype(np.float32).reshape(rows, self.V)
        assert v.shape == (rows, self.V)
        self.v, self.h = v, np.zeros((rows, self.H), np.float32)
        self.mult = np.tile(self.betas, self.M)
        self.idx = np.tile(np.arange(self.R, dtype=np.int32), self.M)
        self.part_v = slot_partials(v * self.vb[None, :])
        self.part_h = None
        self.cnt = np.zeros((2, max(self.R - 1, 0)), np.int64)
        self.step = 0
        self.margins = []                      # |u - exp(delta)| of every swap draw

    def _tempered(self, Q, Pk, bias, site, call):
        """states of one pass, every row at its own temperature"""
        out = np.zeros((Q.shape[0], Pk.shape[1]), np.float32)
        for b in np.unique(self.mult):
            _, s = act2(Q, Pk, None, None, bias, None, float(b), 0, 1, self.seed, site, call, self.chain0 * self.R)
            rows = self.mult == b
            out[rows] = s[rows]
        return out

    def _swap(self, t, call):
        M, R = self.M, self.R
        parity = self.step & 1
        E = -slot_sum(self.part_h, slot_sum(self.part_v))          # one running sum per row: the v.vb slots, then the h slots
        u = philox.uniform(self.seed, SITE_PT_SWAP + 16 * t, call, M * (R - 1), idx0=self.chain0 * (R - 1)).reshape(M, R - 1)
        idx = self.idx.reshape(M, R)
        base = np.arange(M) * R
        for p in range(parity, R - 1, 2):
            ra, rb = base + np.argmax(idx == p, axis=1), base + np.argmax(idx == p + 1, axis=1)
            ba, bb = self.mult[ra].copy(), self.mult[rb].copy()
            delta = (ba.astype(np.float64) - bb.astype(np.float64)) * (E[ra] - E[rb])
            with np.errstate(over='ignore'):
                ex = np.exp(delta)
            up = u[:, p].astype(np.float64)
            accept = (delta >= 0.0) | (up < ex)
            self.margins.extend(np.abs(up - ex).tolist())
            self.cnt[0, p] += M
            self.cnt[1, p] += int(accept.sum())
            a, b = ra[accept], rb[accept]
            self.mult[a], self.mult[b] = bb[accept], ba[accept]
            self.idx[a], self.idx[b] = p + 1, p

    def sweep(self, n_steps, call=0):
        """bm_rbm_pt_sweep: per step t the tempered prop-up, the swap of parity (global step) & 1, the tempered prop-down"""
        ones = np.ones(self.H, np.float32)
        row0 = self.chain0 * self.R
        for t in range(n_steps):
            self.h = self._tempered(self.v, self.W, self.hb, SITE_H + 16 * t, call)
            zb, _ = act2(self.v, self.W, None, None, self.hb, ones, 1.0, 2, 0, self.seed, SITE_H + 16 * t, call, row0)
            self.part_h = slot_partials(self.h * zb)
            if self.R > 1:
                self._swap(t, call)
            self.v = self._tempered(self.h, self.Wt, self.vb, SITE_V + 16 * t, call)
            self.part_v = slot_partials(self.v * self.vb[None, :])
            self.step += 1

    def read(self):
        """(V [M][V], H [M][H]) of the beta = 1 rows"""
        rows = np.arange(self.M) * self.R + np.argmax(self.idx.reshape(self.M, self.R) == self.R - 1, axis=1)
        return self.v[rows].copy(), self.h[rows].copy()


def exact_tempered_visible(W, vb, hb, beta):
    """p_beta(v) of a small Bernoulli RBM for all 2^V visible states (state code: bit i = v_i), hidden layer summed out"""
    W, vb, hb = (np.asarray(a, np.float64) for a in (W, vb, hb))
    V = W.shape[0]
    codes = np.arange(1 << V)
    vs = ((codes[:, None] >> np.arange(V)[None, :]) & 1).astype(np.float64)
    logp = beta * vs.dot(vb) + np.logaddexp(0.0, beta * (vs.dot(W) + hb[None, :])).sum(axis=1)
    pr = np.exp(logp - logp.max())
    return vs, pr / pr.sum()
