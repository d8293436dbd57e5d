"""CPU twin of an RBM with noisy rectified-linear hidden units (BM_UNIT_NRELU), for the tests.

Built from what exists, in the style of tests/class_joint_twin.py:
  * the hidden pass: the pre-activation t is tests/clamp_twin.act2 with kind 1 and sigma = ones, (1 * z) * 1 + 1 * b - bit for bit
    the value a kind-3 pass of the engine forms; the mean is the rectified t (a comparison: +0 for t <= 0, -0 and NaN); the state is
    max(0, t + n * sqrt(sigmoid(t))) with orc_sigmoid element by element, np.sqrt in float32, the normal draws of orc_normal at flat
    index (row0 + j) * I + i, and the multiply and the add as two float32 NumPy operations (each rounded once, nothing fused);
  * the visible pass: act2;
  * the update: orc_rbm_raw_grads on a hand-filled work struct, then orc_rbm_apply through OracleRBM.
Signed zeros.  A unit whose mean is +0 for the whole batch in both phases: the engine's last prop-up stores -m = -0 for it and its
kernels ADD that operand (outer products: fma(-0, v, acc); column sums: h0 + (-0)), the oracle SUBTRACTS +0 (fma(+0, -v, acc);
h0 - 0).  Every accumulator of either starts at +0 and x + (-0) == x - (+0) == x for every x including +0, so both leave +0: the
same bits.  Nothing under oracle/ is involved beyond the calls named above.
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from tests.clamp_twin import SITE_H, SITE_V, act2

SITE_H0 = 2                  # csrc/bm_rbm.hip: the positive phase's site (and bm_rbm_sample_h's)
f32 = np.float32


def sigmoid32(t):
    """orc_sigmoid element by element (one call per distinct bit pattern)"""
    t = np.ascontiguousarray(t, f32)
    bits, inv = np.unique(t.view(np.uint32).ravel(), return_inverse=True)
    f = orc.lib().orc_sigmoid
    vals = np.array([f(float(x)) for x in bits.view(f32)], f32)
    return vals[inv].reshape(t.shape)


def rectify(x):
    x = np.asarray(x, f32)
    with np.errstate(invalid='ignore'):
        return np.where(x > f32(0), x, f32(0)).astype(f32)


def state_from(t, n):
    """s = max(0, t + n * sqrt(sigmoid(t))), every step one float32 operation"""
    t, n = np.asarray(t, f32), np.asarray(n, f32)
    sd = np.sqrt(sigmoid32(t)).astype(f32)
    u = (t + (n * sd).astype(f32)).astype(f32)
    return rectify(u), u


def pre_activation(v, W, hb):
    """t = v W + hb [J][I] as the engine's kind-3 pass rounds it"""
    W = np.ascontiguousarray(W, f32)
    t, _ = act2(v, W, None, None, hb, np.ones(W.shape[1], f32), 1.0, 1, 0, 0, 0, 0, 0)
    return t


def normals(seed, site, call, row0, J, I):
    return orc.normal(int(seed), int(site), int(call), J * I, idx0=int(row0) * I).reshape(J, I)


def hidden_pass(v, W, hb, sample, seed, site, call, row0=0):
    """(means, states) of the hidden layer given v [J][V]; sample = 0: states = means"""
    t = pre_activation(v, W, hb)
    m = rectify(t)
    if not sample:
        return m, m.copy()
    s, _ = state_from(t, normals(seed, site, call, row0, t.shape[0], t.shape[1]))
    return m, s


def sample_h(p, X, seed, call=0, row0=0):
    """bm_rbm_sample_h of an NReLU handle"""
    return hidden_pass(X, p['W'], p['hb'], 1, seed, SITE_H0, call, row0)


class NReLURBM(object):
    """CPU twin of one bm_rbm handle with h_unit = BM_UNIT_NRELU: `rbm` is an oracle.OracleRBM that holds the variables and makes
    the update; the chain is restated here"""

    def __init__(self, p0, seed, v_unit=0, l2=1e-4, sample_v_states=False, sample_h_states=True):
        V, H = p0['W'].shape
        self.V, self.H, self.v_unit = V, H, int(v_unit)
        self.rbm = orc.OracleRBM(V, H, v_unit=v_unit, l2=l2, sample_v_states=sample_v_states, sample_h_states=sample_h_states)
        for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means', 'sigma'):
            if n in p0:
                self.rbm.p[n][...] = p0[n]
        self.seed, self.call, self.row0, self.l2 = int(seed), 0, 0, l2
        self.sample_v, self.sample_h = int(bool(sample_v_states)), int(bool(sample_h_states))

    @property
    def p(self):
        return self.rbm.p

    def set_seed(self, seed):
        self.seed, self.call = int(seed), 0

    def _xin(self, X):
        X = np.ascontiguousarray(X, f32)
        if self.v_unit == 1:
            X = np.ascontiguousarray((X / self.p['sigma'][None, :]).astype(f32))
        return X

    def _up(self, v, sample, site):
        return hidden_pass(v, self.p['W'], self.p['hb'], sample, self.seed, site, self.call, self.row0)

    def _down(self, h, site):
        Wt = np.ascontiguousarray(self.p['W'].T)
        return act2(h, Wt, None, None, self.p['vb'], self.p['sigma'], 1.0, self.v_unit, self.sample_v, self.seed, site, self.call,
                    self.row0)

    def chain(self, X, k):
        Xin = self._xin(X)
        h0m, h0s = self._up(Xin, 1, SITE_H0)
        hstate = h0s if self.sample_h else h0m
        vm = vs = hm = None
        for t in range(k):
            vm, vs = self._down(hstate, SITE_V + 16 * t)
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

    def metrics(self, X, k):
        """(msre, l2_loss) of the chain from X, in float64"""
        ch = self.chain(X, k)
        self.call += 1
        d = ch['Xin'].astype(np.float64) - ch['vm'].astype(np.float64)
        return float((d * d).mean()), float(self.l2 * 0.5 * (self.p['W'].astype(np.float64) ** 2).sum())

    def gibbs(self, Hs, n_steps):
        h = np.ascontiguousarray(Hs, f32)
        v = None
        for t in range(n_steps):
            _, v = self._down(h, SITE_V + 16 * t)
            _, h = self._up(v, self.sample_h, SITE_H + 16 * t)
        self.call += 1
        return h, v

    def state(self):
        return {n: self.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}
