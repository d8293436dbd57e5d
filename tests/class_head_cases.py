"""The cases shared by tests/test_class_head.py (CPU) and tests/test_class_head_gpu.py: shapes, inputs drawn through the oracle's
Philox streams, and the float64 reference / float32 twin trajectories (tests/np_reference_class.py) with the tolerances they give.
Nothing here touches the engine."""
import functools

import numpy as np

from oracle import oracle as orc
from tests import np_reference_class as R

SEED = 818181
L2, LR, MOM, UPDATES = 1e-3, 0.05, 0.9, 3
# (V, H, C, B): ragged last slot of 11 columns, I % 8 != 0, several slots | aligned vector paths, power-of-two batch |
# I % 4 != 0 generic path, J no multiple of 16, smallest C | more than one tile in both directions for every geometry
SHAPES = [(70, 75, 10, 17), (64, 128, 3, 16), (37, 29, 2, 33), (100, 200, 10, 70)]
FACTOR = 10.0          # tolerance = FACTOR x the float32 twin's own deviation from float64 (the convention of the centring tests)


def params(V, H, C):
    """float32 start: scale-0.3 random parameters, zero momentum buffers"""
    n = lambda site, k: orc.normal(SEED, site, 0, k) * np.float32(0.3)
    p = dict(W=n(1, V * H).reshape(V, H), hb=n(2, H), vb=n(3, V), U=n(4, C * H).reshape(C, H), yb=n(5, C))
    for k in ('W', 'hb', 'vb', 'U', 'yb'):
        p['d' + k] = np.zeros_like(p[k])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in p.items()}


def data(n, V, C):
    X = (orc.uniform(SEED, 6, 0, n * V) < 0.4).astype(np.float32).reshape(n, V)
    y = np.minimum((orc.uniform(SEED, 7, 0, n) * C).astype(np.int32), C - 1)
    return X, y


@functools.lru_cache(maxsize=None)
def case(V, H, C, B):
    """dict(p0, X, y, ref=[state after update u], twin=[...], out2=[reference (mean log p, accuracy) before update u], out2_twin,
    logp_ref, logp_tol: the forward pass of the start on the first batch).  Computed once, shared, never modified."""
    p0 = params(V, H, C)
    X, y = data(UPDATES * B, V, C)
    ref, twin, out2, out2_twin = [], [], [], []
    pr, pt = R.cast(p0, np.float64), R.cast(p0, np.float32)
    for u in range(UPDATES):
        Xb, yb = X[u * B:(u + 1) * B], y[u * B:(u + 1) * B]
        pr, o = R.step(pr, Xb, yb, np.float32(LR), np.float32(MOM), np.float32(L2), np.float64)
        pt, ot = R.step(pt, Xb, yb, LR, MOM, L2, np.float32)
        ref.append(pr); twin.append(pt); out2.append(o); out2_twin.append(ot)
    logp_ref, _ = R.forward(R.cast(p0, np.float64), X[:B], np.float64)
    logp_twin, _ = R.forward(R.cast(p0, np.float32), X[:B], np.float32)
    assert logp_twin.dtype == np.float32 and twin[-1]['W'].dtype == np.float32
    return dict(p0=p0, X=X, y=y, ref=ref, twin=twin, out2=out2, out2_twin=out2_twin, logp_ref=logp_ref, logp_twin_dev=R.max_dev(logp_twin, logp_ref),
                logp_tol=FACTOR * R.max_dev(logp_twin, logp_ref))


def top_two_gap(logp):
    s = np.sort(np.asarray(logp, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


# ---- the learning problem of the public-class test: 4 random binary prototypes in 64 dimensions, 256 rows, every bit flipped
# with probability 0.15; H = 32, U and W of scale 0.1; lr 0.5, momentum 0.5, l2 1e-3, batch 32, 10 epochs
LEARN = dict(V=64, H=32, C=4, N=256, flip=0.15, scale=0.1, lr=0.5, mom=0.5, l2=1e-3, batch=32, epochs=10)


@functools.lru_cache(maxsize=None)
def learning_case():
    c = LEARN
    proto = (orc.uniform(SEED, 11, 0, c['C'] * c['V']) < 0.5).astype(np.float32).reshape(c['C'], c['V'])
    y = np.minimum((orc.uniform(SEED, 12, 0, c['N']) * c['C']).astype(np.int32), c['C'] - 1)
    flips = orc.uniform(SEED, 13, 0, c['N'] * c['V']).reshape(c['N'], c['V']) < c['flip']
    X = np.abs(proto[y] - flips.astype(np.float32)).astype(np.float32)
    W = np.ascontiguousarray(orc.normal(SEED, 14, 0, c['V'] * c['H']).reshape(c['V'], c['H']) * np.float32(c['scale']), dtype=np.float32)
    U = np.ascontiguousarray(orc.normal(SEED, 15, 0, c['C'] * c['H']).reshape(c['C'], c['H']) * np.float32(c['scale']), dtype=np.float32)
    p0 = dict(W=W, hb=np.zeros(c['H'], np.float32), vb=np.zeros(c['V'], np.float32), U=U, yb=np.zeros(c['C'], np.float32))
    for k in ('W', 'hb', 'vb', 'U', 'yb'):
        p0['d' + k] = np.zeros_like(p0[k])
    out = {}
    for name, dt in (('ref', np.float64), ('twin', np.float32)):
        p = R.cast(p0, dt)
        for _ in range(c['epochs']):
            p, _ = R.epoch(p, X, y, c['batch'], np.float32(c['lr']), np.float32(c['mom']), np.float32(c['l2']), dt)
        L, _ = R.forward(p, X, dt)
        out[name] = (float(L[np.arange(c['N']), y].astype(np.float64).mean()), float((L.argmax(axis=1) == y).mean()))
    return dict(X=X, y=y, p0=p0, ref=out['ref'], twin=out['twin'], tol=FACTOR * abs(out['twin'][0] - out['ref'][0]))
