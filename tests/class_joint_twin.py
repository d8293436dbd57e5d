"""CPU twin of the joint training of a classification RBM (bm_rbm_class_joint_train_step / _epoch, bm_rbm_class_gibbs;
DESIGN.md 3.19), for the tests.

Built from what exists: the class-bias prop-up is tests/clamp_twin.act2 once per distinct class with the bias float32(hb + U[c])
(the rows of that class kept: draws go by position, so this is the CB pass bit for bit - the pattern of pt_twin._tempered); the
W / hb / vb update is the oracle's own (orc_rbm_raw_grads on a hand-filled RbmWork, then orc_rbm_apply through OracleRBM); the
class draw and the U / yb update are NumPy in the kernels' stated orders.  Nothing under oracle/ is involved beyond those calls.
"""
import ctypes as C

import numpy as np

from boltzmann_machines_amd.utils import philox
from oracle import oracle as orc
from tests.clamp_twin import SITE_H, SITE_V, act2

SITE_H0 = 2                  # csrc/bm_rbm.hip: the positive phase's site
SITE_CLASS_Y = 12            # ... the class draw's (one uniform per row, + 16 t)
SITE_CLASS_V0 = 13           # ... the Ber(1/2) start of bm_rbm_class_gibbs
f32 = np.float32


def cb_pass(p, v, y, sample, seed, site, call, row0=0):
    """E[h | v, y] and its draw: row j takes the bias float32(hb + U[y_j]); a label outside [0, C) the plain bias"""
    v = np.ascontiguousarray(v, f32)
    C_ = p['U'].shape[0]
    means, states = np.zeros((len(v), p['W'].shape[1]), f32), np.zeros((len(v), p['W'].shape[1]), f32)
    y = np.asarray(y)
    valid = (y >= 0) & (y < C_)
    for c in [-1] + sorted(set(int(t) for t in y[valid])):
        rows = ~valid if c < 0 else (valid & (y == c))
        if not rows.any():
            continue
        bias = p['hb'] if c < 0 else (p['hb'].astype(f32) + p['U'][c].astype(f32)).astype(f32)
        m, s = act2(v, p['W'], None, None, bias, None, 1.0, 0, sample, seed, site, call, row0)
        means[rows], states[rows] = m[rows], s[rows]
    return means, states


def class_draw(p, h, seed, site, call, row0=0, margins=None):
    """y ~ p(y | h), class_draw_kernel's order.  logit_c = yb_c + sum_i h_i U[c][i] in double: lane l of 64 adds the products of
    i = l, l + 64, ... in ascending order, the 64 partial sums meet in a butterfly (offsets 32, 16, .., 1), yb_c is added last;
    maximum, sum of exp(logit - max) and the prefix sums over the classes in ascending order, in double; one float32 uniform
    per row at flat index row0 + j; y = the lowest c with u * total < prefix_c, C - 1 if none.  margins (a list): every draw's
    min_c |u * total - prefix_c| / total is appended"""
    h64, U64, yb64 = np.asarray(h, f32).astype(np.float64), p['U'].astype(np.float64), p['yb'].astype(np.float64)
    B, H = h64.shape
    C_ = U64.shape[0]
    u = philox.uniform(seed, site, call, B, idx0=row0).astype(np.float64)
    lanes = np.arange(64)
    y = np.zeros(B, np.int32)
    for j in range(B):
        part = np.zeros((C_, 64))
        for i0 in range(0, H, 64):
            n = min(64, H - i0)
            part[:, :n] = part[:, :n] + h64[j, i0:i0 + n][None, :] * U64[:, i0:i0 + n]
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[:, lanes ^ off]
        logit = yb64 + part[:, 0]
        mx = logit[0]
        for c in range(1, C_):
            mx = logit[c] if logit[c] > mx else mx
        total = 0.0
        for c in range(C_):
            total = total + np.exp(logit[c] - mx)
        pre, got, thr, marg = 0.0, C_ - 1, u[j] * total, np.inf
        found = False
        for c in range(C_):
            pre = pre + np.exp(logit[c] - mx)
            if c < C_ - 1:                               # (the last prefix decides nothing: C - 1 is taken either way)
                marg = min(marg, abs(thr - pre) / total)
            if not found and thr < pre:
                got, found = c, True
        y[j] = got
        if margins is not None:
            margins.append(marg)
    return y


def chain(p, X, y, k, seed, call, row0=0, sample_v=False, sample_h=True, margins=None):
    """the CD-k chain on (x, y): dict(h0m, vk, yk, hk) - plus every step's (v, y, h means)"""
    h0m, h0s = cb_pass(p, X, y, 1, seed, SITE_H0, call, row0)
    hstate = h0s if sample_h else h0m
    Wt = np.ascontiguousarray(p['W'].T)
    steps = []
    for t in range(k):
        vm, vs = act2(hstate, Wt, None, None, p['vb'], None, 1.0, 0, int(sample_v), seed, SITE_V + 16 * t, call, row0)
        v = vs if sample_v else vm
        yk = class_draw(p, hstate, seed, SITE_CLASS_Y + 16 * t, call, row0, margins)
        hm, hs = cb_pass(p, v, yk, int(sample_h), seed, SITE_H + 16 * t, call, row0)
        hstate = hs if sample_h else hm
        steps.append((v, yk, hm))
    v, yk, hm = steps[-1]
    return dict(h0m=h0m, vk=v, yk=yk, hk=hm, steps=steps)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def sigmoid32(x):
    x = np.asarray(x, f32)
    e = np.exp(-np.abs(x)).astype(f32)
    return np.where(x >= 0, f32(1) / (f32(1) + e), e / (f32(1) + e)).astype(f32)


def head_sums(C_, y, yk, h0m, hk, gamma=0.0, coef=None, T=None, U=None):
    """the raw sums of class_joint_update_kernel, float32 in its order: for U[c][i] wave w of 4 takes the rows w, w + 4, ... in
    ascending order - per row + h0m where y == c, - hk where yk == c, then fma(gamma * coef, sigmoid(t + U[c][i]), .) - and the
    four partial sums meet as (s0 + s1) + (s2 + s3); for yb[c] lane l of 64 takes the rows l, l + 64, ... and the 64 sums meet
    in a butterfly (offsets 32 .. 1).  A row whose label is outside [0, C) is out of every sum"""
    B, H = h0m.shape
    ok = (np.asarray(y) >= 0) & (np.asarray(y) < C_)
    g = f32(gamma)
    sU, syb = np.zeros((C_, H), f32), np.zeros(C_, f32)
    lanes = np.arange(64)
    for c in range(C_):
        part = np.zeros((4, H), f32)
        for w in range(4):
            s = np.zeros(H, f32)
            for j in range(w, B, 4):
                if not ok[j]:
                    continue
                if y[j] == c:
                    s = (s + h0m[j]).astype(f32)
                if yk[j] == c:
                    s = (s - hk[j]).astype(f32)
                if gamma > 0:
                    s = _fma((g * coef[j, c]).astype(f32), sigmoid32((T[j] + U[c]).astype(f32)), s)
            part[w] = s
        sU[c] = ((part[0] + part[1]).astype(f32) + (part[2] + part[3]).astype(f32)).astype(f32)
        lane = np.zeros(64, f32)
        for j in range(B):
            if not ok[j]:
                continue
            d = f32(float(y[j] == c) - float(yk[j] == c))
            lane[j % 64] = f32(lane[j % 64] + d)
            if gamma > 0:
                lane[j % 64] = _fma(g, coef[j, c], lane[j % 64])
        for off in (32, 16, 8, 4, 2, 1):
            lane = (lane + lane[lanes ^ off]).astype(f32)
        syb[c] = lane[0]
    return sU, syb


def apply_head(p, sU, syb, B, lr, mom, l2):
    """apply_w_update on U (l2, momentum, learning rate), the bias rule on yb; float32, one rounding per operation"""
    lr, mom, l2, n = f32(lr), f32(mom), f32(l2), f32(B)
    g = ((sU / n).astype(f32) - (l2 * p['U']).astype(f32)).astype(f32)
    g = (g - f32(0)).astype(f32)
    p['dU'] = (lr * ((mom * p['dU']).astype(f32) + g).astype(f32)).astype(f32)
    p['U'] = (p['U'] + p['dU']).astype(f32)
    gb = (syb / n).astype(f32)
    p['dyb'] = (lr * ((mom * p['dyb']).astype(f32) + gb).astype(f32)).astype(f32)
    p['yb'] = (p['yb'] + p['dyb']).astype(f32)


def disc_parts(p, X, y):
    """float32 restatement of the discriminative launches 1-3: t = x W + hb, coef, g = pos + negm"""
    from tests import np_reference_class as R
    pf = R.cast(p, f32)
    L, z = R.forward(pf, X, f32)
    C_ = p['U'].shape[0]
    P = np.exp(L).astype(f32)
    S = sigmoid32(z[:, None, :] + pf['U'][None, :, :])
    coef = ((np.arange(C_)[None, :] == np.asarray(y)[:, None]).astype(f32) - P).astype(f32)
    pos = S[np.arange(len(X)), y, :]
    negm = -(P[:, :, None] * S).sum(axis=1, dtype=f32)
    return z.astype(f32), coef, (pos + negm).astype(f32), L


class JointRBM(object):
    """CPU twin of one bm_rbm handle with a class head that trains through bm_rbm_class_joint_train_step: `rbm` is an
    oracle.OracleRBM (W, hb, vb, their momentum buffers and q_means), `head` holds U, yb, dU, dyb"""

    def __init__(self, p0, seed, l2, sample_v_states=False, sample_h_states=True):
        V, H = p0['W'].shape
        self.rbm = orc.OracleRBM(V, H, l2=l2, sample_v_states=sample_v_states, sample_h_states=sample_h_states)
        for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb'):
            if n in p0:
                self.rbm.p[n][...] = p0[n]
        self.head = {n: np.array(p0[n], f32) for n in ('U', 'yb', 'dU', 'dyb')}
        self.seed, self.call, self.l2 = int(seed), 0, l2
        self.sample_v, self.sample_h = bool(sample_v_states), bool(sample_h_states)
        self.margins = []
        self.last = None

    def params(self):
        p = dict(self.rbm.p)
        p.update(self.head)
        return p

    def train_step(self, X, y, k, lr, mom, gamma=0.0, row0=0):
        X = np.ascontiguousarray(X, f32)
        B, p = len(X), self.params()
        C_ = p['U'].shape[0]
        T = coef = g = None
        if gamma > 0:
            T, coef, g, _ = disc_parts(p, X, y)
        ch = chain(p, X, y, k, self.seed, self.call, row0, self.sample_v, self.sample_h, self.margins)
        self.last = ch
        sU, syb = head_sums(C_, y, ch['yk'], ch['h0m'], ch['hk'], gamma, coef, T, p['U'])
        apply_head(self.head, sU, syb, B, lr, mom, self.l2)
        h0m = ch['h0m'] if gamma <= 0 else _fma(f32(gamma), g, ch['h0m'])
        h0m, vk, hk = (np.ascontiguousarray(a, f32) for a in (h0m, ch['vk'], ch['hk']))
        z = np.zeros((B, max(X.shape[1], h0m.shape[1])), f32)          # (h0s, vm, hs: not read by the raw sums)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        w = orc.RbmWork(ptr(X), ptr(h0m), ptr(z), ptr(z), ptr(vk), ptr(hk), ptr(z))
        raw = np.zeros(X.shape[1] * h0m.shape[1] + X.shape[1] + 2 * h0m.shape[1], f32)
        orc.lib().orc_rbm_raw_grads(C.byref(self.rbm.cfg), C.byref(w), B, raw)
        self.rbm.apply(raw, float(B), lr, mom)
        self.call += 1
        self.rbm.call = self.call

    def train_epoch(self, X, y, batch, k, lr, mom, gamma=0.0):
        for s in range(0, len(X), batch):
            self.train_step(X[s:s + batch], y[s:s + batch], k, lr, mom, gamma)

    def state(self):
        out = {n: self.rbm.p[n].copy() for n in ('W', 'hb', 'vb', 'dW', 'dhb', 'dvb')}
        out.update({n: self.head[n].copy() for n in ('U', 'yb', 'dU', 'dyb')})
        return out

    def log_proba(self, X):
        from tests import np_reference_class as R
        return R.forward(R.cast(self.params(), np.float64), X, np.float64)[0]


def class_gibbs(p, V0, y, n_steps, seed, call=0, row0=0):
    """bm_rbm_class_gibbs: v_0 from the caller or Ber(1/2) (u < 0.5 at SITE_CLASS_V0, flat index (row0 + j) V + i); per step the
    CB prop-up with y clamped, then the visible pass, both sampled.  Returns (v, v means of the last step)"""
    B, V = len(y), p['W'].shape[0]
    if V0 is None:
        V0 = (philox.uniform(seed, SITE_CLASS_V0, call, B * V, idx0=row0 * V) < f32(0.5)).astype(f32).reshape(B, V)
    v, vm = np.ascontiguousarray(V0, f32), None
    Wt = np.ascontiguousarray(p['W'].T)
    for t in range(n_steps):
        _, h = cb_pass(p, v, y, 1, seed, SITE_H + 16 * t, call, row0)
        vm, v = act2(h, Wt, None, None, p['vb'], None, 1.0, 0, 1, seed, SITE_V + 16 * t, call, row0)
    return v, vm


def exact_v_given_class(W, vb, hb, U, yb):
    """E[v_i | y = c] [C][V] of a small classification RBM, by enumeration of the visible states (the hidden layer summed out)"""
    W, vb, hb, U = (np.asarray(a, np.float64) for a in (W, vb, hb, U))
    V = W.shape[0]
    vs = np.array([[(n >> b) & 1 for b in range(V)] for n in range(1 << V)], np.float64)
    out = np.zeros((U.shape[0], V))
    for c in range(U.shape[0]):
        z = vs.dot(W) + hb[None, :] + U[c][None, :]
        lw = vs.dot(vb) + (np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))).sum(axis=1)
        pr = np.exp(lw - lw.max())
        pr /= pr.sum()
        out[c] = pr.dot(vs)
    return out
