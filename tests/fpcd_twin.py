"""CPU twin of fast-weights PCD (bm_rbm_set_fast_weights + bm_rbm_train_step_pt), for the tests.

tests/pt_train_twin.TemperedRBM with a fast parameter set beside the regular one.  The ensemble (rescore, tempered steps, swap
energies) and the negative means run under the effective set W + W_fast, vb + vb_fast, hb + hb_fast; the positive phase and
the regular update are the parent's.  The fast update is restated in NumPy float32 from the same raw sums with the engine's
roundings: g0 = raw / B (one float32 division), fast <- decay * fast + rate * g0 (two rounded products, one rounded sum),
effective = regular_new + fast (one rounded sum).
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from tests import pt_train_twin as P
from tests.clamp_twin import SITE_H

NAMES = ('W', 'vb', 'hb')


class FastTemperedRBM(P.TemperedRBM):
    def __init__(self, p, n_chains, betas, seed, call=0, fast_learning_rate=0.0, fast_decay=0.95, **cfg):
        super(FastTemperedRBM, self).__init__(p, n_chains, betas, seed, call=call, **cfg)
        self.set_fast_weights(fast_learning_rate, fast_decay)
        self.zero_fast()

    def set_fast_weights(self, fast_learning_rate, fast_decay):
        self.fast_lr, self.fast_decay = np.float32(fast_learning_rate), np.float32(fast_decay)

    def zero_fast(self):
        self.fast = {n: np.zeros_like(self.rbm.p[n], dtype=np.float32) for n in NAMES}

    def effective(self):
        """W_eff, vb_eff, hb_eff: one float32 addition per element"""
        return {n: (self.rbm.p[n] + self.fast[n]).astype(np.float32) for n in NAMES}

    def train_step(self, X, lr, momentum, k):
        X = np.ascontiguousarray(X, np.float32)
        B, p, e = len(X), self.rbm.p, self.ens
        assert 1 <= B <= e.M and k >= 1
        V, H = e.V, e.H
        pe = self.effective()
        e.set_params(pe)
        e.rescore()                                                             # 1. under vb_eff
        h0m = P.hidden_means(p, X, self.seed, P.SITE_H0, self.call)             # 2. the regular set
        e.sweep(k, call=self.call)                                              # 3. the effective set
        vs = np.ascontiguousarray(e.read()[0][:B])                              # 4.
        hm = P.hidden_means(pe, vs, self.seed, SITE_H, self.call)               # 5. the effective set
        z = np.zeros((B, max(V, H)), np.float32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        w = orc.RbmWork(ptr(X), ptr(h0m), ptr(z), ptr(z), ptr(vs), ptr(hm), ptr(z))
        raw = np.zeros(V * H + V + 2 * H, np.float32)
        orc.lib().orc_rbm_raw_grads(C.byref(self.rbm.cfg), C.byref(w), B, raw)  # 6. the regular update, exactly the parent's
        self.rbm.apply(raw, float(B), lr, momentum)
        N = np.float32(B)                                                       # ... and the fast one from the same raw sums
        g0 = dict(W=raw[:V * H].reshape(V, H) / N, vb=raw[V * H:V * H + V] / N, hb=raw[V * H + V:V * H + V + H] / N)
        for n in NAMES:
            assert g0[n].dtype == np.float32
            self.fast[n] = (self.fast_decay * self.fast[n] + self.fast_lr * g0[n]).astype(np.float32)
        self.last = dict(X=X, h0m=h0m, vs=vs, hm=hm, raw=raw, eff=pe)
        self.call += 1                                                          # 7.
        self.rbm.call = self.call

    def cd_step(self, X, lr, momentum, k):
        """a plain CD update of the regular model between two fast-weights updates (bm_rbm_train_step)"""
        self.rbm.seed, self.rbm.call = self.seed, self.call
        self.rbm.train_step(X, lr, momentum, k)
        self.call = self.rbm.call

    def state(self):
        out = super(FastTemperedRBM, self).state()
        eff = self.effective()
        for n in NAMES:
            out[n + '_fast'] = self.fast[n].copy()
            out[n + '_eff'] = eff[n]
        return out
