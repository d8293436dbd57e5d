"""The cases shared by tests/test_stack_finetune.py (CPU) and tests/test_stack_finetune_gpu.py: shapes, inputs drawn through
utils.philox, and the float64 reference / float32 twin results (tests/np_reference_stack.py) with the bounds they give.  Nothing
here touches the engine."""
import functools

import numpy as np

from boltzmann_machines_amd.utils import philox
from tests import np_reference_stack as S

SEED = 212121
FACTOR = 10.0          # bound = FACTOR x the float32 twin's own deviation from float64 (the rule of the class-head tests)
# name -> (V, hidden widths (the last one is the top's), C, B, N)
#   S1: partial quads, partial 16-column slots, a short last batch (10, 10, 5)
#   S2: the backward passes chained through two layers, every width and the batch across a 64 boundary
#   S3: the aligned vector-store paths
STACKS = dict(S1=(33, (17, 20), 3, 10, 25), S2=(70, (130, 66, 36), 10, 67, 67), S3=(64, (128, 64), 2, 64, 64))
GRAD_LR = 0.25                       # test 1: one step, momentum 0, l2 0
LR, MOM, L2, UPDATES = 0.1, 0.5, 1e-3, 3      # test 2: three consecutive steps (every layer the same lr and l2)


def _normal(site, n, scale):
    return (philox.normal(SEED, site, 0, n) * np.float32(scale)).astype(np.float32)


def _bias(site, n):
    return (philox.uniform(SEED, site, 0, n) * np.float32(2) - np.float32(1)).astype(np.float32)


def params(V, widths, C):
    """float32 start: weights N(0, 0.3^2), biases in +-1, zero momentum buffers"""
    sizes = (V,) + tuple(widths)
    layers = []
    for i in range(len(widths)):
        v, h = sizes[i], sizes[i + 1]
        l = dict(W=_normal(10 * i + 1, v * h, 0.3).reshape(v, h), hb=_bias(10 * i + 2, h), vb=_bias(10 * i + 3, v))
        layers.append(l)
    H = widths[-1]
    layers[-1].update(U=_normal(91, C * H, 0.3).reshape(C, H), yb=_bias(92, C))
    for l in layers:
        for k in list(l):
            l['d' + k] = np.zeros_like(l[k])
    layers = [{k: np.ascontiguousarray(v, dtype=np.float32) for k, v in l.items()} for l in layers]
    return dict(layers=layers[:-1], top=layers[-1])


def data(n, V, C):
    """grey levels in [0, 1] (a_l is never binary either) and labels"""
    X = philox.uniform(SEED, 95, 0, n * V).astype(np.float32).reshape(n, V)
    y = np.minimum((philox.uniform(SEED, 96, 0, n) * C).astype(np.int32), C - 1)
    return X, y


def grad_like(before, after, lr):
    """(P_after - P_before) / lr per trained tensor, in float64 - the quantity test 1 compares, formed the same way from the
    engine's and from the twin's float32 parameters"""
    b, a = S.tensors(before), S.tensors(after)
    return {k: (np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)) / float(lr) for k in b}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(p0, X, y, D, lrs, l2s; grad_ref / grad_twin / grad_tol per tensor for the first batch; ref / twin / stale: the states
    after each of UPDATES steps on batch 0; logp_ref, logp_tol).  Computed once, shared, never modified."""
    V, widths, C, B, N = STACKS[name]
    p0 = params(V, widths, C)
    X, y = data(max(N, B), V, C)
    D = len(widths) - 1
    Xb, yb = X[:B], y[:B]
    # test 1: momentum 0, l2 0
    zeros, glr = [0.0] * (D + 1), [GRAD_LR] * (D + 1)
    lg, tg, _ = S.gradients(S.cast(p0, np.float64), Xb, yb, np.float64)
    grad_ref = {}
    for i, g in enumerate(lg):
        grad_ref['W%d' % (i + 1)], grad_ref['hb%d' % (i + 1)] = g['W'], g['hb']
    for k in ('W', 'hb', 'U', 'yb'):
        grad_ref[k] = tg[k]
    twin1, _ = S.step(p0, Xb, yb, glr, 0.0, zeros, np.float32)
    grad_twin = grad_like(p0, twin1, GRAD_LR)
    grad_tol = {k: FACTOR * S.max_dev(grad_twin[k], grad_ref[k]) for k in grad_ref}
    # test 2: three steps on the same batch with momentum and l2
    lrs, l2s = [LR] * (D + 1), [L2] * (D + 1)
    ref, twin, stale = [], [], []
    pr, pt, ps = S.cast(p0, np.float64), S.cast(p0, np.float32), S.cast(p0, np.float32)
    for u in range(UPDATES):
        pr, _ = S.step(pr, Xb, yb, [np.float32(v) for v in lrs], np.float32(MOM), [np.float32(v) for v in l2s], np.float64)
        pt, _ = S.step(pt, Xb, yb, lrs, MOM, l2s, np.float32)
        ps, _ = S.step(ps, Xb, yb, lrs, MOM, l2s, np.float32, stale=True)
        ref.append(pr); twin.append(pt); stale.append(ps)
    assert twin[-1]['top']['W'].dtype == np.float32
    logp_ref = S.log_proba(S.cast(p0, np.float64), X, np.float64)
    logp_twin = S.log_proba(S.cast(p0, np.float32), X, np.float32)
    return dict(p0=p0, X=X, y=y, D=D, B=B, N=N, C=C, V=V, widths=widths, glr=glr, lrs=lrs, l2s=l2s, grad_ref=grad_ref,
                grad_twin=grad_twin, grad_tol=grad_tol, ref=ref, twin=twin, stale=stale, logp_ref=logp_ref,
                logp_tol=FACTOR * S.max_dev(logp_twin, logp_ref))


# ---- the learning problem of the public-class test: 16-12-10, C = 3, 60 rows - three well-separated prototype patterns (disjoint
# blocks of set bits: any two differ in 10 or 11 of the 16 bits) plus 10 % bit noise.  (With blocks that shared a bit and lr 0.5
# the float64 reference reached 0.83 in five epochs: the separation and the learning rate were enlarged, nothing else)
TOY = dict(V=16, widths=(12, 10), C=3, N=60, flip=0.10, scale=0.3, lr=1.0, mom=0.5, l2=1e-4, batch=10, epochs=5)


@functools.lru_cache(maxsize=None)
def toy_case():
    c = TOY
    proto = np.zeros((c['C'], c['V']), np.float32)
    proto[0, :5], proto[1, 5:11], proto[2, 11:] = 1, 1, 1
    y = (np.arange(c['N']) % c['C']).astype(np.int32)
    flips = philox.uniform(SEED, 97, 0, c['N'] * c['V']).reshape(c['N'], c['V']) < c['flip']
    X = np.abs(proto[y] - flips.astype(np.float32)).astype(np.float32)
    p0 = params(c['V'], c['widths'], c['C'])
    for l in p0['layers'] + [p0['top']]:
        for k in ('hb', 'vb') + (('yb',) if 'yb' in l else ()):
            l[k] = np.zeros_like(l[k])
    D = len(c['widths']) - 1
    lrs, l2s = [c['lr']] * (D + 1), [c['l2']] * (D + 1)
    out = {}
    for name, dt in (('ref', np.float64), ('twin', np.float32)):
        p = S.cast(p0, dt)
        start = S.mean_log_proba(p, X, y, dt)
        for _ in range(c['epochs']):
            p, _ = S.epoch(p, X, y, c['batch'], lrs, c['mom'], l2s, dt)
        L = S.log_proba(p, X, dt)
        out[name] = (start, float(L[np.arange(c['N']), y].astype(np.float64).mean()), float((L.argmax(axis=1) == y).mean()))
    return dict(X=X, y=y, p0=p0, lrs=lrs, ref=out['ref'], twin=out['twin'])
