"""CPU twin of the clamped sweeps (bm_rbm_gibbs_clamped, bm_dbm_sample_v_clamped), for the tests.

The sweeps are restated as loops of the oracle library's one activation stage (orc_act / orc_act2, oracle/bm_oracle.c:
what act_kernel computes), called with the engine's seed / site / call / row0 arguments; the blend
`v = where(mask, clamp, v)` is done on the host between the calls.  Nothing under oracle/ is involved beyond those calls.
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc

SITE_V, SITE_H = 3, 4                  # csrc/bm_rng.h: the RBM's Gibbs sites
SITE_DBM_H, SITE_DBM_V = 8, 12         # ... the DBM's (hidden layer i: SITE_DBM_H + i)

_vp = C.c_void_p
_ACT2_ARGS = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, C.c_float, C.c_float, C.c_int, C.c_int,
              _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64]


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def act2(Q1, P1k, Q2, P2k, bias, sigma, mult, kind, sample, seed, site, call, row0):
    """one activation stage: Q1 [J][K1] x P1k [K1][I] (+ Q2 [J][K2] x P2k [K2][I]) -> (means, states), both [J][I]"""
    f = orc.lib().orc_act2
    f.argtypes = _ACT2_ARGS
    f.restype = None
    Q1, P1k = np.ascontiguousarray(Q1, np.float32), np.ascontiguousarray(P1k, np.float32)
    J, K1 = Q1.shape
    I = P1k.shape[1]
    K2 = 0
    if Q2 is not None:
        Q2, P2k = np.ascontiguousarray(Q2, np.float32), np.ascontiguousarray(P2k, np.float32)
        K2 = Q2.shape[1]
    bias = np.ascontiguousarray(bias, np.float32)
    sigma = None if sigma is None else np.ascontiguousarray(sigma, np.float32)
    means, states = np.zeros((J, I), np.float32), np.zeros((J, I), np.float32)
    f(_p(Q1), K1, _p(P1k), _p(Q2), K2, _p(P2k if K2 else None), I, J, _p(bias), _p(sigma), mult, mult, int(kind), int(sample),
      _p(means), _p(states), int(seed), int(site), int(call), int(row0))
    return means, states


def blend(mask, clamp, v):
    return np.where(np.asarray(mask) != 0, clamp, v).astype(np.float32)


def rbm_gibbs_clamped(p, V0, clamp, mask, n_steps, seed, call=0, row0=0, v_unit=0, dbm_first=False, dbm_last=False,
                      clamped=True):
    """p: dict W [V][H], vb, hb, sigma.  Returns (V, H, Vmean) after n_steps of h ~ p(h|v), v ~ p(v|h) with the blend
    after every visible pass (and on V0 first); clamped=False: the same loop without any blend."""
    W = np.ascontiguousarray(p['W'], np.float32)
    Wt = np.ascontiguousarray(W.T)
    up, down = 1.0 + float(dbm_first), 1.0 + float(dbm_last)
    v = np.ascontiguousarray(V0, np.float32).copy()
    if clamped:
        v = blend(mask, clamp, v)
    h = vm = None
    for t in range(n_steps):
        _, h = act2(v, W, None, None, p['hb'], None, up, 0, 1, seed, SITE_H + 16 * t, call, row0)
        vm, v = act2(h, Wt, None, None, p['vb'], p['sigma'], down, v_unit, 1, seed, SITE_V + 16 * t, call, row0)
        if clamped:
            vm, v = blend(mask, clamp, vm), blend(mask, clamp, v)
    return v, h, vm


def _dbm_sweep(W, hb, vb, sigma, v_unit, sample_v, sample_h, vin, Hin, sample, t, seed, call, row0, clamp, mask):
    """`_make_gibbs_step` in orc's dbm_sweep order: bottom-up, NEW below / OLD above, then the visible layer (clamped)"""
    L = len(W)
    Hout = []
    for i in range(L):
        below = vin if i == 0 else Hout[i - 1]
        above, Wt = (Hin[i + 1], np.ascontiguousarray(W[i + 1].T)) if i + 1 < L else (None, None)
        smp = int(bool(sample and sample_h[i]))
        m, s = act2(below, W[i], above, Wt, hb[i], None, 1.0, 0, smp, seed, SITE_DBM_H + i + 16 * t, call, row0)
        Hout.append(s)
    smp = int(bool(sample and sample_v))
    _, v = act2(Hout[0], np.ascontiguousarray(W[0].T), None, None, vb, sigma, 1.0, v_unit, smp, seed, SITE_DBM_V + 16 * t,
                call, row0)
    if mask is not None:
        v = blend(mask, clamp, v)
    return v, Hout


def dbm_sample_v_clamped(W, hb, vb, sigma, v, H, k, seed, call=0, prow0=0, clamp=None, mask=None, v_unit=0,
                         sample_v=True, sample_h=None):
    """orc_dbm_sample_v's order of passes: k sampled sweeps (the particles), then k mean sweeps whose v is assigned.
    W: list of [n_l][n_{l+1}], hb: list, v [M][V], H: list of [M][n].  Returns (v_result, particles_v, particles_H);
    mask None: the unclamped call."""
    sample_h = sample_h or [True] * len(W)
    v = np.ascontiguousarray(v, np.float32).copy()
    H = [np.ascontiguousarray(h, np.float32).copy() for h in H]
    if mask is not None:
        v = blend(mask, clamp, v)
    for t in range(k):
        v, H = _dbm_sweep(W, hb, vb, sigma, v_unit, sample_v, sample_h, v, H, True, t, seed, call, prow0, clamp, mask)
    vm, Hm = v, H
    for t in range(k):
        vm, Hm = _dbm_sweep(W, hb, vb, sigma, v_unit, sample_v, sample_h, vm, Hm, False, k + t, seed, call, prow0, clamp, mask)
    return vm, v, H


def exact_conditional(W, vb, hb, x, observed):
    """p(v_i = 1 | v_observed) of a small Bernoulli RBM for the free units i, by enumeration of every (v_free, h)"""
    W, vb, hb = (np.asarray(a, np.float64) for a in (W, vb, hb))
    V, H = W.shape
    free = [i for i in range(V) if not observed[i]]
    num, den = np.zeros(len(free)), 0.0
    for cf in range(1 << len(free)):
        v = np.asarray(x, np.float64).copy()
        for b, i in enumerate(free):
            v[i] = (cf >> b) & 1
        for ch in range(1 << H):
            h = np.array([(ch >> b) & 1 for b in range(H)], np.float64)
            w = np.exp(v.dot(vb) + h.dot(hb) + v.dot(W).dot(h))
            den += w
            num += w * v[free]
    return free, num / den
