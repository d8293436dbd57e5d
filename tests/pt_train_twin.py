"""CPU twin of the tempered negative phase (bm_rbm_train_step_pt / _train_epoch_pt), for the tests.

Built from what exists: the ensemble is tests/pt_twin.Ensemble with the re-scoring of the v.vb slot partials added, the two
means-only prop-ups are tests/clamp_twin.act2 (sample = 0), and the update is the oracle's own: orc_rbm_raw_grads on a
hand-filled RbmWork (Xin = the batch, h0m = its hidden means, vs = the beta = 1 rows of the chains [0, B), hm = their hidden
means), then orc_rbm_apply.  Nothing under oracle/ is involved beyond those calls.
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from tests import pt_twin as T
from tests.clamp_twin import SITE_H, act2

SITE_H0 = 2                            # csrc/bm_rbm.hip: the positive phase's site


class TrainEnsemble(T.Ensemble):
    """Ensemble whose parameters move between the sweeps"""

    def set_params(self, p):
        self.W = np.ascontiguousarray(p['W'], np.float32)
        self.Wt = np.ascontiguousarray(self.W.T)
        self.vb, self.hb = np.ascontiguousarray(p['vb'], np.float32), np.ascontiguousarray(p['hb'], np.float32)

    def rescore(self):
        """pt_rescore_kernel: the v.vb slot partials of the stored states under the vb of now"""
        self.part_v = T.slot_partials(self.v * self.vb[None, :])


def hidden_means(p, v, seed=0, site=SITE_H, call=0):
    """E[h | v] of every row (no draw: seed, site and call are not read)"""
    return act2(v, p['W'], None, None, p['hb'], None, 1.0, 0, 0, seed, site, call, 0)[0]


class TemperedRBM(object):
    """CPU twin of one bm_rbm handle that trains through bm_rbm_train_step_pt: `rbm` is an oracle.OracleRBM (its parameters,
    momentum buffers and q_means are the handle's), `ens` the ensemble bm_rbm_pt_init built at call `call` of `seed`"""

    def __init__(self, p, n_chains, betas, seed, call=0, **cfg):
        V, H = p['W'].shape
        self.rbm = orc.OracleRBM(V, H, **cfg)
        for n in ('W', 'vb', 'hb'):
            self.rbm.p[n][...] = p[n]
        self.seed, self.call = int(seed), int(call)
        self.ens = TrainEnsemble(self.rbm.p, n_chains, betas, seed=self.seed, call=self.call)

    @property
    def p(self):
        return self.rbm.p

    def train_step(self, X, lr, momentum, k):
        X = np.ascontiguousarray(X, np.float32)
        B, p, e = len(X), self.rbm.p, self.ens
        assert 1 <= B <= e.M and k >= 1
        e.set_params(p)
        e.rescore()                                                             # 1.
        h0m = hidden_means(p, X, self.seed, SITE_H0, self.call)                # 2.
        e.sweep(k, call=self.call)                                              # 3.
        vs = np.ascontiguousarray(e.read()[0][:B])                              # 4.
        hm = hidden_means(p, vs, self.seed, SITE_H, self.call)                 # 5.
        z = np.zeros((B, max(e.V, e.H)), np.float32)                            # (h0s, vm, hs: not read by the raw sums)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        w = orc.RbmWork(ptr(X), ptr(h0m), ptr(z), ptr(z), ptr(vs), ptr(hm), ptr(z))
        raw = np.zeros(e.V * e.H + e.V + 2 * e.H, np.float32)
        orc.lib().orc_rbm_raw_grads(C.byref(self.rbm.cfg), C.byref(w), B, raw)  # 6.
        self.rbm.apply(raw, float(B), lr, momentum)
        self.call += 1                                                          # 7.
        self.rbm.call = self.call

    def train_epoch(self, X, batch, lr, momentum, k):
        for s in range(0, len(X), batch):
            self.train_step(X[s:s + batch], lr, momentum, k)

    def state(self):
        """everything the GPU tests compare, as copies"""
        e = self.ens
        out = {n: self.rbm.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}
        out.update(ens_v=e.v.copy(), ens_h=e.h.copy(), idx=e.idx.copy(), swaps=e.cnt.copy())
        return out


def exact_vh(W, vb, hb):
    """E[v_i h_j] under p(v, h) of a small Bernoulli RBM, [V][H], by enumeration of the visible states"""
    vs, pr = T.exact_tempered_visible(W, vb, hb, 1.0)
    hbar = 1.0 / (1.0 + np.exp(-(vs.dot(np.asarray(W, np.float64)) + np.asarray(hb, np.float64)[None, :])))
    return (vs * pr[:, None]).T.dot(hbar)
