"""CPU twin of the DBM's tempered negative phase (bm_dbm_train_step_pt), for the tests.

Built from what exists: the ensemble is tests/dbm_pt_twin.Ensemble with parameters that move between the sweeps and the
re-scoring of the v.vb and h2.b2 slot partials added; the update is the oracle's own.  Per update, in the engine's order:
    set_params, rescore                     the partials under the biases of now
    ens.sweep(k, call)                      k tempered steps of every row at the handle's call
    p['v'], p['h'], p['h_1'] <- ens.read()  the beta = 1 rows of the chains [0, n_particles)
    oracle.train_step(X, lr, mom, 0, ...)   with k = 0 the oracle runs the mean-field, NO particle sweep, the msre and
                                            dbm_apply_update, and advances its call once
(the mean-field draws nothing and reads no particle, so its place before or behind the sweeps does not show).  Nothing under
oracle/ is involved beyond OracleDBM.
"""
import numpy as np

from oracle import oracle as orc
from tests import dbm_pt_twin as T
from tests.pt_twin import slot_partials


def sfx(i):
    return '' if i == 0 else '_%d' % i


class TrainEnsemble(T.Ensemble):
    """Ensemble whose parameters move between the sweeps"""

    def set_params(self, p):
        """p: dict W (list), vb, hb (list) - as Ensemble's constructor"""
        self.W = [np.ascontiguousarray(w, np.float32).copy() for w in p['W']]
        self.Wt = [np.ascontiguousarray(w.T) for w in self.W]
        self.vb = np.ascontiguousarray(p['vb'], np.float32).copy()
        self.hb = [np.ascontiguousarray(b, np.float32).copy() for b in p['hb']]

    def rescore(self):
        """pt_rescore_kernel: the v.vb and h2.b2 slot partials of the stored states under the biases of now"""
        self.part_v = slot_partials(self.v * self.vb[None, :])
        if self.L == 2:
            self.part_h2 = slot_partials(self.h[1] * self.hb[1][None, :])


class TemperedDBM(object):
    """CPU twin of one bm_dbm handle that trains through bm_dbm_train_step_pt: `oracle` is an oracle.OracleDBM (parameters,
    momentum buffers, running means, mu and the dense particles are the handle's), `ens` the ensemble bm_dbm_pt_init built at
    call `call` of `seed`.  ens_kw: V0 / V0_rows / H2_rows of the ensemble's start"""

    def __init__(self, p, n_particles, batch_size, n_chains, betas, seed, call=0, ens_kw=None, **cfg):
        n = [np.asarray(p['W'][0]).shape[0]] + [np.asarray(w).shape[1] for w in p['W']]
        T.check_model(len(n) - 1, literal=bool(cfg.get('sigmoid_literal', False)))
        if int(n_chains) < int(n_particles):
            raise ValueError('the ensemble has %d chains, fewer than n_particles = %d' % (n_chains, n_particles))
        self.oracle = orc.OracleDBM(n[0], n[1:], n_particles=n_particles, batch_size=batch_size, **cfg)
        self.L, self.M = len(n) - 1, int(n_particles)
        for i in range(self.L):
            self.oracle.p['W' + sfx(i)][...] = p['W'][i]
            self.oracle.p['hb' + sfx(i)][...] = p['hb'][i]
        self.oracle.p['vb'][...] = p['vb']
        self.oracle.set_seed(seed)
        self.oracle.call = int(call)
        self.seed = int(seed)
        self.ens = TrainEnsemble(self.params(), n_chains, betas, seed=self.seed, call=int(call), **(ens_kw or {}))

    @property
    def call(self):
        return self.oracle.call

    @property
    def p(self):
        return self.oracle.p

    def params(self):
        q = self.oracle.p
        return dict(W=[q['W' + sfx(i)] for i in range(self.L)], vb=q['vb'], hb=[q['hb' + sfx(i)] for i in range(self.L)])

    def pt_sweep(self, k):
        """bm_dbm_pt_sweep on the handle: the parameters of now, no re-scoring, the call advances once"""
        self.ens.set_params(self.params())
        self.ens.sweep(k, call=self.oracle.call)
        self.oracle.call += 1

    def train_step(self, X, lr, momentum, k, want_msre=False):
        assert k >= 1
        e, q = self.ens, self.oracle.p
        e.set_params(self.params())
        e.rescore()                                                             # 1.
        e.sweep(k, call=self.oracle.call)                                       # 3.
        v, H = e.read()                                                         # 4.
        q['v'][...] = v[:self.M]
        for i in range(self.L):
            q['h' + sfx(i)][...] = H[i][:self.M]
        return self.oracle.train_step(X, lr, momentum, 0, want_msre)            # 2., 5., 6., 7.

    NAMES = ('W', 'dW', 'hb', 'dhb', 'q_means', 'mu_means', 'mu', 'h')

    def names(self):
        return ['vb', 'dvb', 'v'] + [b + sfx(i) for i in range(self.L) for b in self.NAMES]

    def state(self):
        """everything the GPU tests compare, as copies: the handle's variables, the ensemble's beta = 1 rows, the ladder index
        of every row, the swap counters"""
        out = {nm: self.oracle.p[nm].copy() for nm in self.names()}
        v, H = self.ens.read()
        out.update(ens_V=v, idx=self.ens.idx.astype(np.int32).copy(), swaps=self.ens.cnt.copy())
        for i, h in enumerate(H):
            out['ens_H%d' % (i + 1)] = h
        return out


def exact_tempered_moments(W, vb, hb, beta=1.0):
    """(E[v_i h1_j] [V][n1], E[h1_j h2_k] [n1][n2]) under p_beta(v, h1, h2) of a small v-h1-h2 Bernoulli DBM, in float64:
    dbm_pt_twin.exact_tempered_joint extended to h1 - p_beta(v, h2) by enumeration, E[h1_j | v, h2] = sigmoid(beta z_j)"""
    vs, h2s, P = T.exact_tempered_joint(W, vb, hb, beta)
    W0, W1 = (np.asarray(w, np.float64) for w in W)
    z = vs.dot(W0)[:, None, :] + h2s.dot(W1.T)[None, :, :] + np.asarray(hb[0], np.float64)[None, None, :]
    h1 = 1.0 / (1.0 + np.exp(-beta * z))                                        # [2^V][2^n2][n1]
    PH = P[:, :, None] * h1
    return np.einsum('vi,vkj->ij', vs, PH), np.einsum('vkj,km->jm', PH, h2s)
