"""The cases shared by tests/test_class_joint.py (CPU) and tests/test_class_joint_gpu.py: the shapes, start
parameters and hyper-parameters of tests/class_head_cases.py, labels that cover every class, and the CPU twin's trajectories
(tests/class_joint_twin.py).  Nothing here touches the engine."""
import functools

import numpy as np

from oracle import oracle as orc
from tests import class_head_cases as H
from tests import class_joint_twin as T

SEED = 272727                  # the engine seed of every case (bm_rbm_seed)
SHAPES, L2, LR, MOM, UPDATES, FACTOR = H.SHAPES, H.L2, H.LR, H.MOM, H.UPDATES, H.FACTOR
GAMMA = 0.5                    # the hybrid case's discriminative weight
MIN_MARGIN = 1e-9              # no class draw of any case may sit closer to a prefix sum than this, relative to the total
NAMES = ('W', 'hb', 'vb', 'U', 'yb', 'dW', 'dhb', 'dvb', 'dU', 'dyb')


@functools.lru_cache(maxsize=None)
def inputs(V, H_, C, B):
    """dict(p0, X [UPDATES * B][V], y): class_head_cases' parameters and data; the first C labels of every batch are 0 .. C - 1"""
    p0 = H.params(V, H_, C)
    X, y = H.data(UPDATES * B, V, C)
    y = y.copy()
    for u in range(UPDATES):
        y[u * B:u * B + C] = np.arange(C)
    return dict(p0=p0, X=X, y=np.ascontiguousarray(y, np.int32))


@functools.lru_cache(maxsize=None)
def trajectory(V, H_, C, B, k=1, gamma=0.0, updates=UPDATES):
    """the twin's run of `updates` updates from the case's start: dict(states=[state after update u], chains=[the chain of update
    u: h0m, vk, yk, hk, steps], margins=[every class draw's relative margin]).  Computed once, shared, never modified"""
    c = inputs(V, H_, C, B)
    tw = T.JointRBM(c['p0'], SEED, L2)
    states, chains = [], []
    for u in range(updates):
        tw.train_step(c['X'][u * B:(u + 1) * B], c['y'][u * B:(u + 1) * B], k, LR, MOM, gamma)
        states.append(tw.state())
        chains.append(tw.last)
    return dict(states=states, chains=chains, margins=list(tw.margins))


# ---- the enumerable model of the sampling test: V = 6, H = 4, C = 3, parameters of scale 1
SMALL = dict(V=6, H=4, C=3, chains=4096, steps=200, seed=515151)


@functools.lru_cache(maxsize=None)
def small_model():
    c = SMALL
    n = lambda site, k: orc.normal(SEED, site, 0, k)
    p = dict(W=n(21, c['V'] * c['H']).reshape(c['V'], c['H']), hb=n(22, c['H']) * np.float32(0.5), vb=n(23, c['V']) * np.float32(0.5),
             U=n(24, c['C'] * c['H']).reshape(c['C'], c['H']) * np.float32(1.5), yb=n(25, c['C']) * np.float32(0.5))
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    return dict(p=p, exact=T.exact_v_given_class(p['W'], p['vb'], p['hb'], p['U'], p['yb']))


# ---- the learning problem of the public-class test: two prototype patterns per class, 5 % flips, V = 64, C = 4
LEARN = dict(V=64, H=32, C=4, N=256, flip=0.05, scale=0.1, lr=0.2, mom=0.5, l2=1e-3, batch=32, epochs=5, k=1, gamma=0.0, seed=1337,
             threshold=0.9)


@functools.lru_cache(maxsize=None)
def learning_data():
    c = LEARN
    proto = (orc.uniform(SEED, 31, 0, 2 * c['C'] * c['V']) < 0.5).astype(np.float32).reshape(c['C'], 2, c['V'])
    y = (np.arange(c['N']) % c['C']).astype(np.int32)
    which = (orc.uniform(SEED, 32, 0, c['N']) < 0.5).astype(np.int64)
    flips = orc.uniform(SEED, 33, 0, c['N'] * c['V']).reshape(c['N'], c['V']) < c['flip']
    X = np.abs(proto[y, which] - flips.astype(np.float32)).astype(np.float32)
    W = np.ascontiguousarray(orc.normal(SEED, 34, 0, c['V'] * c['H']).reshape(c['V'], c['H']) * np.float32(c['scale']), dtype=np.float32)
    U = np.ascontiguousarray(orc.normal(SEED, 35, 0, c['C'] * c['H']).reshape(c['C'], c['H']) * np.float32(c['scale']), dtype=np.float32)
    return dict(X=X, y=y, W=W, U=U)
