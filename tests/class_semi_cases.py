"""The cases shared by tests/test_class_semi.py (CPU) and tests/test_class_semi_gpu.py: the shapes and
hyper-parameters of tests/class_head_cases.py plus one shape with more classes than a wave has lanes, the CPU twin's trajectories
(tests/class_semi_twin.py) and the learning problem of the public-class test.  Nothing here touches the engine."""
import functools

import numpy as np

from oracle import oracle as orc
from tests import class_head_cases as H
from tests import class_joint_cases as K
from tests import class_semi_twin as T

SEED = 272727                  # the engine seed of every case (the first seed tried: every margin below holds with it)
WIDE = (20, 24, 70, 9)         # more classes than a wave has lanes
SHAPES = list(H.SHAPES) + [WIDE]
L2, LR, MOM, UPDATES, FACTOR = H.L2, H.LR, H.MOM, H.UPDATES, H.FACTOR
Y0_MARGIN = 1e-6               # no posterior draw may sit closer to a prefix sum than this, relative to the total
MIN_MARGIN = K.MIN_MARGIN      # ... and no class draw of the chain closer than this
NAMES = K.NAMES


@functools.lru_cache(maxsize=None)
def inputs(V, H_, C, B):
    """dict(p0, X [UPDATES * B][V]): class_head_cases' parameters and data.  The wide shape's class biases rise with the class
    (yb_c = 3 c / C on top of the random start), so that the posterior's mass - and with it the draws - reach the classes >= 64"""
    p0 = dict(H.params(V, H_, C))
    if C > 64:
        p0['yb'] = np.ascontiguousarray(p0['yb'] + np.float32(3.0) * np.arange(C, dtype=np.float32) / np.float32(C), np.float32)
    X, _ = H.data(UPDATES * B, V, C)
    return dict(p0=p0, X=X)


@functools.lru_cache(maxsize=None)
def chain(V, H_, C, B, k=1, sample_h=True):
    """the twin's chain of the case's first batch at call 0, with dict(margins, y0_margins)"""
    c = inputs(V, H_, C, B)
    m, m0 = [], []
    ch = T.unsup_chain(c['p0'], c['X'][:B], k, SEED, 0, sample_h=sample_h, margins=m, y0_margins=m0)
    return dict(ch, margins=m, y0_margins=m0)


@functools.lru_cache(maxsize=None)
def trajectory(V, H_, C, B, k=1, updates=UPDATES):
    """the twin's run of `updates` unlabelled updates from the case's start: dict(states, chains, out2, margins, y0_margins).
    Computed once, shared, never modified"""
    c = inputs(V, H_, C, B)
    tw = T.SemiRBM(c['p0'], SEED, L2)
    states, chains, out2 = [], [], []
    for u in range(updates):
        out2.append(tw.unsup_step(c['X'][u * B:(u + 1) * B], k, LR, MOM))
        states.append(tw.state())
        chains.append(tw.last_unsup)
    return dict(states=states, chains=chains, out2=out2, margins=list(tw.margins), y0_margins=list(tw.y0_margins))


# ---- the learning problem of the public-class test, modelled on class_joint_cases.LEARN: two prototype patterns per class,
# V = 64, C = 4; few labelled rows, many unlabelled ones, held-out rows for the accuracy
LEARN = dict(V=64, H=32, C=4, N=32, Nu=512, Nval=512, flip=0.2, scale=0.1, lr=0.1, mom=0.5, l2=1e-3, batch=32, epochs=100, k=1, gamma=0.0,
             beta=1.0, seed=1337, gain=0.05, tol=0.05)


@functools.lru_cache(maxsize=None)
def learning_data():
    c = LEARN
    n = c['N'] + c['Nu'] + c['Nval']
    proto = (orc.uniform(SEED, 41, 0, 2 * c['C'] * c['V']) < 0.5).astype(np.float32).reshape(c['C'], 2, c['V'])
    y = (np.arange(n) % c['C']).astype(np.int32)
    which = (orc.uniform(SEED, 42, 0, n) < 0.5).astype(np.int64)
    flips = orc.uniform(SEED, 43, 0, n * c['V']).reshape(n, c['V']) < c['flip']
    X = np.abs(proto[y, which] - flips.astype(np.float32)).astype(np.float32)
    W = np.ascontiguousarray(orc.normal(SEED, 44, 0, c['V'] * c['H']).reshape(c['V'], c['H']) * np.float32(c['scale']), dtype=np.float32)
    U = np.ascontiguousarray(orc.normal(SEED, 45, 0, c['C'] * c['H']).reshape(c['C'], c['H']) * np.float32(c['scale']), dtype=np.float32)
    a, b = c['N'], c['N'] + c['Nu']
    return dict(X=X[:a], y=y[:a], Xu=X[a:b], Xval=X[b:], yval=y[b:], W=W, U=U)


@functools.lru_cache(maxsize=None)
def learning_twin(beta, seed=None):
    """the twin's held-out accuracy after the schedule of LEARN with unlabelled_weight = beta, as fit_semi_supervised runs it:
    one engine seed for the call (None: learning_seed()), the slice cursor carried from epoch to epoch"""
    c, d = LEARN, learning_data()
    p0 = dict(W=d['W'], hb=np.zeros(c['H'], np.float32), vb=np.zeros(c['V'], np.float32), U=d['U'], yb=np.zeros(c['C'], np.float32))
    for n in ('W', 'hb', 'vb', 'U', 'yb'):
        p0['d' + n] = np.zeros_like(p0[n])
    tw = T.SemiRBM(p0, learning_seed() if seed is None else int(seed), c['l2'])
    u = 0
    for _ in range(c['epochs']):
        u = tw.semi_epoch(d['X'], d['y'], d['Xu'], u, c['batch'], c['k'], c['lr'], c['mom'], c['gamma'], beta)
    return float((tw.log_proba(d['Xval']).argmax(axis=1) == d['yval']).mean())


def learning_seed():
    """what make_random_seed() of a fresh model with random_seed = LEARN['seed'] returns first (base.SeedMixin)"""
    from boltzmann_machines_amd.utils.rng import RNG
    return int(RNG(seed=LEARN['seed']).randint(2 ** 31 - 1))
