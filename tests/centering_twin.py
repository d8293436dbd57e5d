"""float32 twin of the centred RBM update in the engine's documented order, for the tests.

The raw outer products and the plain column sums come from the oracle's orc_rbm_raw_grads on a hand-filled RbmWork, as
tests/pt_train_twin.py takes them; everything else is NumPy float32, one rounding per operation, in the order of the engine's
kernels:
  column sums      sequential over the rows (the oracle's canonical column sum)
  row scalars      per row 64 lane-strided partial sums (columns lane, lane + 64, ...; product and sum rounded separately),
                   then the xor butterfly 32, 16, ... 1
  bias corrections ONE fma chain over the rows in ascending order per column and phase (the MFMA chain with the row weight as
                   the second operand); r = pos / N - neg / M
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc

f32 = np.float32


def fma32(a, b, c):
    """fmaf(a, b, c) elementwise, correctly rounded: the product of two float32 is exact in float64, the float64 sum is
    turned into round-to-odd with the exact error of the addition (TwoSum), and rounding THAT to float32 is the single
    rounding of the exact a * b + c (53 >= 2 * 24 + 2 bits)."""
    a, b, c = (np.asarray(x, f32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) == 1
    nxt = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & ~odd, nxt, s).astype(f32)


def colsum_seq(A):
    out = np.zeros(A.shape[1], f32)
    for row in np.asarray(A, f32):
        out = out + row
    return out


def rowscal(X, o):
    """a_b = sum_c (x_bc - o_c) o_c in cen_rowscal_kernel's order"""
    X, o = np.asarray(X, f32), np.asarray(o, f32)
    rows, cols = X.shape
    s = np.zeros((rows, 64), f32)
    for c0 in range(0, cols, 64):
        n = min(64, cols - c0)
        s[:, :n] = s[:, :n] + (X[:, c0:c0 + n] - o[None, c0:c0 + n]) * o[None, c0:c0 + n]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ off]
    return np.ascontiguousarray(s[:, 0])


def wcolsum(X, o, w):
    """sum_b (x_bc - o_c) w_b as one fma chain over the rows"""
    X, o, w = np.asarray(X, f32), np.asarray(o, f32), np.asarray(w, f32)
    acc = np.zeros(X.shape[1], f32)
    for b in range(len(X)):
        acc = fma32(X[b] - o, np.full(X.shape[1], w[b], f32), acc)
    return acc


def ema(o, nu, s, N):
    nu, N = f32(nu), f32(N)
    return (f32(1.0) - nu) * np.asarray(o, f32) + nu * (np.asarray(s, f32) / N)


def raw_grads(rbm, X, h0m, vs, hm):
    """orc_rbm_raw_grads on a hand-filled RbmWork: [X^T h0 - v^T h_k | sum(X - v) | sum(h0 - h_k) | sum(h_k)]"""
    V, H, B = rbm.V, rbm.H, len(X)
    arrs = [np.ascontiguousarray(a, f32) for a in (X, h0m, vs, hm)]
    z = np.zeros((B, max(V, H)), f32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    w = orc.RbmWork(ptr(arrs[0]), ptr(arrs[1]), ptr(z), ptr(z), ptr(arrs[2]), ptr(arrs[3]), ptr(z))
    raw = np.zeros(V * H + V + 2 * H, f32)
    orc.lib().orc_rbm_raw_grads(C.byref(rbm.cfg), C.byref(w), B, raw)
    return raw


def centred_apply(rbm, off, nu, X, h0m, vs, hm, lr, momentum):
    """the centred update of an oracle.OracleRBM's variables in place; off = [o_v, o_h] (replaced), nu = (nu_v, nu_h)"""
    p, V, H = rbm.p, rbm.V, rbm.H
    X, h0m, vs, hm = (np.ascontiguousarray(a, f32) for a in (X, h0m, vs, hm))
    N, lr, mom = f32(len(X)), f32(lr), f32(momentum)
    raw = raw_grads(rbm, X, h0m, vs, hm)
    rawW, sv, sh, sq = raw[:V * H].reshape(V, H), raw[V * H:V * H + V], raw[V * H + V:V * H + V + H], raw[V * H + V + H:]
    # 1. offsets, plain bias gradients
    off[0] = ema(off[0], nu[0], colsum_seq(X), N)
    off[1] = ema(off[1], nu[1], colsum_seq(h0m), N)
    ov, oh = off
    gv, gh = sv / N, sh / N
    # 2. row scalars
    aX, av, ah0, ahk = rowscal(X, ov), rowscal(vs, ov), rowscal(h0m, oh), rowscal(hm, oh)
    z = f32(0.0)
    # 3. bias corrections and the bias update
    rv = wcolsum(X, ov, z + ah0) / N - wcolsum(vs, ov, z + ahk) / N
    rh = wcolsum(h0m, oh, aX + z) / N - wcolsum(hm, oh, av + z) / N
    c = rbm.cfg
    d = lr * (mom * p['dvb'] + (gv - rv))
    p['dvb'][...] = d
    p['vb'][...] = p['vb'] + d
    qn = f32(c.sp_damping) * p['q_means'] + (f32(1.0) - f32(c.sp_damping)) * sq
    p['q_means'][...] = qn
    pen = f32(c.sp_cost) * (qn - f32(c.sp_target))
    g = (gh - rh) - pen
    d = lr * (mom * p['dhb'] + g)
    p['dhb'][...] = d
    p['hb'][...] = p['hb'] + d
    # 4. centred weight update
    g = rawW / N
    g = g - (ov[:, None] * gh[None, :] + gv[:, None] * oh[None, :])
    g = g - f32(c.l2) * p['W']
    g = g - pen[None, :]
    d = lr * (mom * p['dW'] + g)
    p['dW'][...] = d
    p['W'][...] = p['W'] + d


class CentredRBM(object):
    """CPU twin of a bm_rbm handle with centering on that trains through bm_rbm_train_step"""

    def __init__(self, params, nu, offsets, seed=0, **cfg):
        V, H = params['W'].shape
        self.rbm = orc.OracleRBM(V, H, **cfg)
        for n in ('W', 'vb', 'hb'):
            self.rbm.p[n][...] = params[n]
        self.rbm.set_seed(seed)
        self.nu = tuple(nu)
        self.off = [np.array(o, f32) for o in offsets]

    def train_step(self, X, lr, momentum, k):
        self.rbm.chain(X, k)
        w = self.rbm.work
        centred_apply(self.rbm, self.off, self.nu, w['Xin'], w['h0m'], w['vs'], w['hm'], lr, momentum)
        self.rbm.call += 1

    def state(self):
        out = {n: self.rbm.p[n].copy() for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')}
        out.update(ov=self.off[0].copy(), oh=self.off[1].copy())
        return out


def tempered_centred_rbm(params, n_chains, betas, seed, nu, offsets, **cfg):
    """tests/pt_train_twin.TemperedRBM with the centred apply in place of orc_rbm_apply (bm_rbm_train_step_pt with centering on)"""
    from tests import pt_train_twin as P

    class TemperedCentredRBM(P.TemperedRBM):
        def train_step(self, X, lr, momentum, k):
            X = np.ascontiguousarray(X, f32)
            B, p, e = len(X), self.rbm.p, self.ens
            assert 1 <= B <= e.M and k >= 1
            e.set_params(p)
            e.rescore()
            h0m = P.hidden_means(p, X, self.seed, P.SITE_H0, self.call)
            e.sweep(k, call=self.call)
            vs = np.ascontiguousarray(e.read()[0][:B])
            hm = P.hidden_means(p, vs, self.seed, P.SITE_H, self.call)
            centred_apply(self.rbm, self.off, self.nu, X, h0m, vs, hm, lr, momentum)
            self.call += 1
            self.rbm.call = self.call

        def state(self):
            out = P.TemperedRBM.state(self)
            out.update(ov=self.off[0].copy(), oh=self.off[1].copy())
            return out

    t = TemperedCentredRBM(params, n_chains, betas, seed, **cfg)
    t.nu, t.off = tuple(nu), [np.array(o, f32) for o in offsets]
    return t


# ---- the case of the flip-invariance test through BernoulliRBM.fit() (tests/test_centering.py measures, test_centering_gpu.py asserts)
FIT = dict(V=37, H=29, rows=40, batch=10, epochs=2, lr=0.05, mom=0.5, nu=0.1)
# what this twin shows on the case: flip_gap(fit_twin(p, X), fit_twin(flip_params(p), 1 - X)) = 7.15e-07, measured on the CPU
# (tests/test_centering.py::test_fit_flip_deviation_of_the_twins keeps the figure honest)
FIT_TWIN_DEVIATION = 7.2e-7


def fit_case():
    SEED = 20241020
    V, H = FIT['V'], FIT['H']
    p = dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H) * f32(0.3), vb=orc.normal(SEED, 2, 0, V) * f32(0.3),
             hb=orc.normal(SEED, 3, 0, H) * f32(0.3))
    X = (orc.uniform(SEED, 6, 0, FIT['rows'] * V) < 0.35).astype(f32).reshape(FIT['rows'], V)
    return p, X


def flip_params(p):
    """the same RBM for the data coded as 1 - v, rounded to float32 once"""
    W64 = p['W'].astype(np.float64)
    return dict(W=-p['W'], vb=-p['vb'], hb=(p['hb'].astype(np.float64) + W64.sum(0)).astype(f32))


def flip_gap(a, b):
    """max abs distance of state b (trained on 1 - X from the flipped start) from the flip of state a; a, b: dicts with W, vb,
    hb, ov, oh"""
    f = flip_params(a)
    return max(np.abs(f['W'] - b['W']).max(), np.abs(f['vb'] - b['vb']).max(), np.abs(f['hb'].astype(np.float64) - b['hb']).max(),
               np.abs((1 - a['ov'].astype(np.float64)) - b['ov']).max(), np.abs(a['oh'] - b['oh']).max())


def fit_twin(p, X):
    """what BernoulliRBM.fit does to the case with all sampling off and l2 = 0: sequential batches, default offsets"""
    o = [X.astype(np.float64).mean(0).astype(f32), np.full(FIT['H'], 0.5, f32)]
    t = CentredRBM(p, (FIT['nu'], FIT['nu']), o, seed=1, sample_v_states=False, sample_h_states=False, l2=0.)
    for _ in range(FIT['epochs']):
        for r in range(0, FIT['rows'], FIT['batch']):
            t.train_step(X[r:r + FIT['batch']], FIT['lr'], FIT['mom'], 1)
    return t.state()
