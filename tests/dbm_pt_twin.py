"""CPU twin of the DBM's parallel-tempering sweeps (bm_dbm_pt_init / _sweep / _read), for the tests.

Built from the pieces of the RBM's twin: states come from the oracle library's activation stage through tests/clamp_twin.act2
(orc_act2: two K segments chained onto one accumulator, below first - what act_kernel computes), called once per distinct
temperature with mult = bmult = beta and the engine's seed / site / call / row0, only the rows at that temperature kept; the
untempered pre-activation z + b of the h1 pass comes from one more call with kind = 2, mult = 1 and a unit sigma; the slot
partials and their ascending sums are tests/pt_twin.slot_partials / slot_sum; the swap uniforms come from
boltzmann_machines_amd/utils/philox.py and the acceptance rule is evaluated in float64.

One step t, in the order of the engine's Gibbs sweep with every layer sampled:
    h1 <- (v, OLD h2)     site h + 16 t        leaves part_h1 = slots of h1 . (v W0 + h2 W1^T + b1)
    swap                  site swap + 16 t     E = -(sum part_v, then sum part_h2, then sum part_h1)
    h2 <- h1 (L = 2)      site h + 1 + 16 t    leaves part_h2 = slots of h2 . b2
    v  <- h1              site v + 16 t        leaves part_v  = slots of v . vb
"""
import numpy as np

from boltzmann_machines_amd.utils import philox
from tests.clamp_twin import SITE_DBM_H, SITE_DBM_V, act2
from tests.pt_twin import slot_partials, slot_sum

SITE_DBM_PT_SWAP, SITE_DBM_PT_START = 14, 15      # csrc/bm_dbm.hip
DBM_SITES = dict(h=SITE_DBM_H, v=SITE_DBM_V, swap=SITE_DBM_PT_SWAP, start=SITE_DBM_PT_START)


class Refused(NotImplementedError):
    pass


def check_model(n_layers, v_unit=0, h_units=None, literal=False):
    """the refusals of bm_dbm_pt_init, with the engine's reasons"""
    if v_unit != 0:
        raise Refused('Gaussian visible units are not supported')
    if any(int(u) != 0 for u in (h_units or [])):
        raise Refused('a Multinomial hidden layer is not supported')
    if n_layers > 2:
        raise Refused('%d hidden layers are not supported (at most 2): a pass reads the OLD layer above, so no point of the '
                      'sweep has every interaction term of one consistent state in the partials' % n_layers)
    if literal:
        raise Refused('literal-sigmoid mode: the row-tempered kernels have no literal flavour')


def check_ladder(betas):
    b = np.asarray(betas, np.float32).ravel()
    if len(b) < 1 or b[-1] != 1. or b[0] <= 0. or np.any(np.diff(b) <= 0.):
        raise ValueError('betas must increase strictly inside (0, 1] and end at 1')
    return b


class Ensemble(object):
    """M chains x R replicas, chain-major rows (row c R + r is slot r of chain c)"""

    def __init__(self, p, n_chains, betas, seed, call=0, chain0=0, V0=None, V0_rows=None, H2_rows=None, sites=None):
        """p: dict W (list of [n_l][n_{l+1}], one or two), vb, hb (list).  V0 [M][V]: every chain's replicas start there;
        V0_rows [M R][V] / H2_rows [M R][n2] (twin only): every row its own start; else v_0 ~ Ber(1/2) at the start site of
        `call`, h2_0 ~ Ber(1/2) at start site + 16.  sites: the RNG sites (default: the DBM's)"""
        self.W = [np.ascontiguousarray(w, np.float32) for w in p['W']]
        self.L = len(self.W)
        check_model(self.L)
        self.Wt = [np.ascontiguousarray(w.T) for w in self.W]
        self.vb = np.ascontiguousarray(p['vb'], np.float32)
        self.hb = [np.ascontiguousarray(b, np.float32) for b in p['hb']]
        self.n = [self.W[0].shape[0]] + [w.shape[1] for w in self.W]
        self.betas = check_ladder(betas)
        self.sites = dict(DBM_SITES, **(sites or {}))
        self.M, self.R, self.seed, self.chain0 = int(n_chains), len(self.betas), int(seed), int(chain0)
        rows, V = self.M * self.R, self.n[0]
        row0 = self.chain0 * self.R
        if V0_rows is not None:
            v = np.ascontiguousarray(V0_rows, np.float32).copy()
        elif V0 is not None:
            v = np.repeat(np.ascontiguousarray(V0, np.float32), self.R, axis=0)
        else:
            u = philox.uniform(seed, self.sites['start'], call, rows * V, idx0=row0 * V)
            v = (u < np.float32(0.5)).astype(np.float32).reshape(rows, V)
        assert v.shape == (rows, V)
        self.v = v
        self.h = [np.zeros((rows, n), np.float32) for n in self.n[1:]]
        self.part_v = slot_partials(v * self.vb[None, :])
        self.part_h2 = np.zeros((rows, 0), np.float32)
        if self.L == 2:
            n2 = self.n[2]
            if H2_rows is not None:
                h2 = np.ascontiguousarray(H2_rows, np.float32).copy()
            else:
                u = philox.uniform(seed, self.sites['start'] + 16, call, rows * n2, idx0=row0 * n2)
                h2 = (u < np.float32(0.5)).astype(np.float32).reshape(rows, n2)
            assert h2.shape == (rows, n2)
            self.h[1] = h2
            self.part_h2 = slot_partials(h2 * self.hb[1][None, :])
        self.part_h1 = None
        self.mult = np.tile(self.betas, self.M)
        self.idx = np.tile(np.arange(self.R, dtype=np.int32), self.M)
        self.cnt = np.zeros((2, max(self.R - 1, 0)), np.int64)
        self.step = 0
        self.margins = []                      # |u - exp(delta)| of every swap draw

    def _tempered(self, Q1, P1, Q2, P2, bias, site, call):
        """states of one pass, every row at its own temperature"""
        out = np.zeros((Q1.shape[0], P1.shape[1]), np.float32)
        for b in np.unique(self.mult):
            _, s = act2(Q1, P1, Q2, P2, bias, None, float(b), 0, 1, self.seed, site, call, self.chain0 * self.R)
            rows = self.mult == b
            out[rows] = s[rows]
        return out

    def _swap(self, t, call):
        M, R = self.M, self.R
        parity = self.step & 1
        E = -slot_sum(self.part_h1, slot_sum(self.part_h2, slot_sum(self.part_v)))     # one running sum per row: v.vb, h2.b2, h1
        u = philox.uniform(self.seed, self.sites['swap'] + 16 * t, call, M * (R - 1), idx0=self.chain0 * (R - 1)).reshape(M, R - 1)
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
        """bm_dbm_pt_sweep"""
        S = self.sites
        ones = np.ones(self.n[1], np.float32)
        row0 = self.chain0 * self.R
        two = self.L == 2
        for t in range(n_steps):
            Q2, P2 = (self.h[1], self.Wt[1]) if two else (None, None)
            self.h[0] = self._tempered(self.v, self.W[0], Q2, P2, self.hb[0], S['h'] + 16 * t, call)
            zb, _ = act2(self.v, self.W[0], Q2, P2, self.hb[0], ones, 1.0, 2, 0, self.seed, S['h'] + 16 * t, call, row0)
            self.part_h1 = slot_partials(self.h[0] * zb)
            if self.R > 1:
                self._swap(t, call)
            if two:
                self.h[1] = self._tempered(self.h[0], self.W[1], None, None, self.hb[1], S['h'] + 1 + 16 * t, call)
                self.part_h2 = slot_partials(self.h[1] * self.hb[1][None, :])
            self.v = self._tempered(self.h[0], self.Wt[0], None, None, self.vb, S['v'] + 16 * t, call)
            self.part_v = slot_partials(self.v * self.vb[None, :])
            self.step += 1

    def beta1_rows(self):
        return np.arange(self.M) * self.R + np.argmax(self.idx.reshape(self.M, self.R) == self.R - 1, axis=1)

    def read(self):
        """(V [M][V], [H1 [M][n1], H2 [M][n2]]) of the beta = 1 rows"""
        rows = self.beta1_rows()
        return self.v[rows].copy(), [h[rows].copy() for h in self.h]


def exact_tempered_joint(W, vb, hb, beta):
    """p_beta(v, h2) of a small v-h1-h2 Bernoulli DBM, h1 summed out, in float64: (vs [2^V][V], h2s [2^n2][n2], P [2^V][2^n2]);
    state code: bit i = unit i"""
    W0, W1 = (np.asarray(w, np.float64) for w in W)
    vb, b1, b2 = np.asarray(vb, np.float64), np.asarray(hb[0], np.float64), np.asarray(hb[1], np.float64)
    V, n2 = W0.shape[0], W1.shape[1]
    vs = ((np.arange(1 << V)[:, None] >> np.arange(V)[None, :]) & 1).astype(np.float64)
    h2s = ((np.arange(1 << n2)[:, None] >> np.arange(n2)[None, :]) & 1).astype(np.float64)
    z = vs.dot(W0)[:, None, :] + h2s.dot(W1.T)[None, :, :] + b1[None, None, :]
    logp = beta * vs.dot(vb)[:, None] + beta * h2s.dot(b2)[None, :] + np.logaddexp(0.0, beta * z).sum(axis=2)
    P = np.exp(logp - logp.max())
    return vs, h2s, P / P.sum()
