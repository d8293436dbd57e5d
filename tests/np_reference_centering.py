"""float64 NumPy restatement of the centred update, two ways.

Layers x_0 = v, x_1 .. x_L; W[l] connects l and l + 1 (l = 0 .. L - 1); b[l] is the bias of layer l (b[0] = vb).  The RBM is
L = 1.  `pos` / `neg` are lists of the layers' rows in the positive (N rows) and negative (M rows) phase.

  update_standard   the form the engine implements: everything in standard parameters, the centred weight gradient as the
                    plain one minus a rank-2 term, the bias gradients corrected by r_l.
  update_explicit   Melchior, Fischer & Wiskott 2016, Algorithm 1: the model held in CENTRED parameters (W, b~), the biases
                    re-parameterised when the offsets move so that the model is unchanged, plain gradient steps on the
                    centred energy, converted back to standard parameters for the comparison.

The two agree (to float64 round-off) for plain gradient steps: momentum 0, l2 0, no sparsity - momentum and l2 act on
different parameterisations in the two forms, and the engine's definition is update_standard.
"""
import numpy as np


def sigm(x):
    return 1.0 / (1.0 + np.exp(-x))


class State(object):
    """parameters, momentum buffers, sparsity accumulators and offsets of a stack of layer sizes n"""

    def __init__(self, n, rng=None, scale=0.1):
        self.n = list(n)
        L = len(n) - 1
        rng = rng or np.random.RandomState(0)
        self.W = [scale * rng.randn(n[l], n[l + 1]) for l in range(L)]
        self.b = [scale * rng.randn(n[l]) for l in range(L + 1)]
        self.dW = [np.zeros_like(w) for w in self.W]
        self.db = [np.zeros_like(b) for b in self.b]
        self.q = [np.zeros(n[l]) for l in range(L + 1)]         # q_means (index 0 unused)
        self.mm = [np.zeros(n[l]) for l in range(L + 1)]        # mu_means of the DBM (index 0 unused)
        self.o = [np.zeros(n[l]) for l in range(L + 1)]

    def copy(self):
        import copy
        return copy.deepcopy(self)

    def astype(self, dtype):
        """a copy with every array in `dtype`: with float32 arrays (and float32 phases) every function of this file computes in
        float32, NumPy's order - the float32 restatement the DBM's flip test takes its tolerance from"""
        t = self.copy()
        for name in ('W', 'b', 'dW', 'db', 'q', 'mm', 'o'):
            setattr(t, name, [np.asarray(a, dtype) for a in getattr(t, name)])
        return t


def flip(s):
    """the same model for the data coded as 1 - v: W_0 -> -W_0, vb -> -vb, hb_0 -> hb_0 + W_0^T 1, o_v -> 1 - o_v (the
    momentum buffers follow the same linear map)"""
    t = s.copy()
    t.W[0] = -s.W[0]
    t.b[0] = -s.b[0]
    t.b[1] = s.b[1] + s.W[0].sum(0)
    t.dW[0] = -s.dW[0]
    t.db[0] = -s.db[0]
    t.db[1] = s.db[1] + s.dW[0].sum(0)
    t.o[0] = 1.0 - s.o[0]
    return t


def flip_gap(s, t):
    """how far t is from flip(s): max abs difference per variable"""
    f = flip(s)
    out = {}
    for l in range(len(s.W)):
        out['W%d' % l] = np.abs(f.W[l] - t.W[l]).max()
    for l in range(len(s.b)):
        out['b%d' % l] = np.abs(f.b[l] - t.b[l]).max()
        out['o%d' % l] = np.abs(f.o[l] - t.o[l]).max()
    return out


def penalties(s, pos, neg, kind, cost, target, damping):
    """the engines' sparsity terms per layer (None where cost is 0).  kind 'rbm': q <- d q + (1 - d) colSUM(h_k),
    pen = cost (q - target) (base_rbm.py:457-460).  kind 'dbm': the reference's scalar-index quirk (dbm.py:582-589): layer i's
    accumulators move towards the column sum of UNIT i of the negative / positive rows, broadcast; pen = cost (q - t) + cost (mm - t)"""
    L = len(s.W)
    pen = [None] * (L + 1)
    for l in range(1, L + 1):
        c = cost[l - 1] if hasattr(cost, '__iter__') else cost
        t = target[l - 1] if hasattr(target, '__iter__') else target
        if kind == 'rbm':
            s.q[l] = damping * s.q[l] + (1.0 - damping) * neg[l].sum(0)
            pen[l] = c * (s.q[l] - t)
        else:
            i = l - 1
            s.q[l] = damping * s.q[l] + (1.0 - damping) * neg[l].sum(0)[i]
            s.mm[l] = damping * s.mm[l] + (1.0 - damping) * pos[l].sum(0)[i]
            pen[l] = c * (s.q[l] - t) + c * (s.mm[l] - t)
    return pen


def update_standard(s, pos, neg, nu, lr, mom=0.0, l2=0.0, centred=True, sparsity=None, max_norm=np.inf):
    """one update in place.  nu: one sliding factor per layer.  sparsity: None or dict(kind, cost, target, damping).
    centred=False: the plain update (the offsets are not touched)."""
    L = len(s.W)
    N, M = float(len(pos[0])), float(len(neg[0]))
    if centred:
        for l in range(L + 1):                                                      # 1. offsets
            s.o[l] = (1.0 - nu[l]) * s.o[l] + nu[l] * pos[l].mean(0)
    o = s.o if centred else [np.zeros_like(x) for x in s.o]
    g = [pos[l].sum(0) / N - neg[l].sum(0) / M for l in range(L + 1)]               # 2. plain bias gradients
    pen = penalties(s, pos, neg, **sparsity) if sparsity else [None] * (L + 1)
    dWs = []
    for l in range(L):                                                              # 3. centred weight gradients
        dWs.append(pos[l].T.dot(pos[l + 1]) / N - neg[l].T.dot(neg[l + 1]) / M
                   - np.outer(o[l], g[l + 1]) - np.outer(g[l], o[l + 1]))
    a_pos = [(pos[l] - o[l]).dot(o[l]) for l in range(L + 1)]                       # 4. row scalars, bias corrections
    a_neg = [(neg[l] - o[l]).dot(o[l]) for l in range(L + 1)]
    for l in range(L + 1):
        wp, wn = np.zeros(int(N), pos[0].dtype), np.zeros(int(M), neg[0].dtype)
        if l > 0:
            wp, wn = wp + a_pos[l - 1], wn + a_neg[l - 1]
        if l < L:
            wp, wn = wp + a_pos[l + 1], wn + a_neg[l + 1]
        r = (pos[l] - o[l]).T.dot(wp) / N - (neg[l] - o[l]).T.dot(wn) / M
        gb = g[l] - r
        if pen[l] is not None:
            gb = gb - pen[l]
        s.db[l] = lr * (mom * s.db[l] + gb)
        s.b[l] = s.b[l] + s.db[l]
    for l in range(L):
        gw = dWs[l] - l2 * s.W[l]
        if pen[l + 1] is not None:
            gw = gw - pen[l + 1][None, :]
        s.dW[l] = lr * (mom * s.dW[l] + gw)
        s.W[l] = s.W[l] + s.dW[l]
        if np.isfinite(max_norm):                                                   # dbm.py:603-607
            nrm = np.sqrt((s.W[l] ** 2).sum(0))
            s.W[l] = s.W[l] * (np.minimum(nrm, max_norm) / np.maximum(nrm, 1e-8))[None, :]
    return s


def centred_biases(s, o):
    """b~_l = b_l + W_{l-1}^T o_{l-1} + W_l o_{l+1}: the biases of the centred energy that is the same model"""
    L = len(s.W)
    out = []
    for l in range(L + 1):
        bt = s.b[l].copy()
        if l > 0:
            bt = bt + s.W[l - 1].T.dot(o[l - 1])
        if l < L:
            bt = bt + s.W[l].dot(o[l + 1])
        out.append(bt)
    return out


def update_explicit(s, pos, neg, nu, lr):
    """Melchior et al. 2016, Algorithm 1, one plain gradient step (no momentum, no l2), in place on the standard-parameter
    state: convert to centred parameters under the old offsets, move the offsets and re-parameterise the biases so that the
    model stays the same, step on the centred gradients, convert back."""
    L = len(s.W)
    bt = centred_biases(s, s.o)                                   # centred biases under the old offsets
    o_new = [(1.0 - nu[l]) * s.o[l] + nu[l] * pos[l].mean(0) for l in range(L + 1)]
    for l in range(L + 1):                                        # re-parameterisation: b~ += W^T (o' - o) (+ the layer above)
        if l > 0:
            bt[l] = bt[l] + s.W[l - 1].T.dot(o_new[l - 1] - s.o[l - 1])
        if l < L:
            bt[l] = bt[l] + s.W[l].dot(o_new[l + 1] - s.o[l + 1])
    s.o = o_new
    cp = [pos[l] - s.o[l] for l in range(L + 1)]
    cn = [neg[l] - s.o[l] for l in range(L + 1)]
    N, M = float(len(pos[0])), float(len(neg[0]))
    for l in range(L + 1):                                        # centred bias gradient: <x_l>_pos - <x_l>_neg
        bt[l] = bt[l] + lr * (cp[l].sum(0) / N - cn[l].sum(0) / M)
    for l in range(L):                                            # centred weight gradient
        s.W[l] = s.W[l] + lr * (cp[l].T.dot(cp[l + 1]) / N - cn[l].T.dot(cn[l + 1]) / M)
    for l in range(L + 1):                                        # back to standard parameters under the new W
        b = bt[l].copy()
        if l > 0:
            b = b - s.W[l - 1].T.dot(s.o[l - 1])
        if l < L:
            b = b - s.W[l].dot(s.o[l + 1])
        s.b[l] = b
    return s


# ---- phases (means only: no sampling anywhere, so a run is a deterministic function of its inputs)
def rbm_phases(s, X, k=1):
    """CD-k with means everywhere: pos = [X, h0], neg = [v_k, h_k]"""
    h0 = sigm(X.dot(s.W[0]) + s.b[1])
    h = h0
    for _ in range(k):
        v = sigm(h.dot(s.W[0].T) + s.b[0])
        h = sigm(v.dot(s.W[0]) + s.b[1])
    return [X, h0], [v, h]


def dbm_layer_mean(s, below, above, l):
    z = s.b[l].copy()[None, :]
    if below is not None:
        z = z + below.dot(s.W[l - 1])
    if above is not None:
        z = z + above.dot(s.W[l].T)
    return sigm(z)


def dbm_phases(s, X, particles, n_mf=5, k=1):
    """fixed number of mean-field sweeps on X (mu started at 0.5, layers in ascending order) and k mean sweeps on the
    particles (hidden layers in ascending order, then the visible layer); returns pos, neg and the new particles"""
    L = len(s.W)
    mu = [X] + [np.full((len(X), s.n[l]), 0.5, X.dtype) for l in range(1, L + 1)]
    for _ in range(n_mf):
        for l in range(1, L + 1):
            mu[l] = dbm_layer_mean(s, mu[l - 1], mu[l + 1] if l < L else None, l)
    p = [x.copy() for x in particles]
    for _ in range(k):
        for l in range(1, L + 1):
            p[l] = dbm_layer_mean(s, p[l - 1], p[l + 1] if l < L else None, l)
        p[0] = dbm_layer_mean(s, None, p[1], 0)
    return mu, p, p


# ---- the case of the flip-invariance tests through DBM.fit() (tests/test_centering.py measures, tests/test_centering_gpu.py asserts)
FIT_N = (16, 12, 8)
FIT_ROWS, FIT_BATCH, FIT_EPOCHS, FIT_LR, FIT_MOM, FIT_NU, FIT_MF = 20, 10, 2, 0.05, 0.5, 0.1, 5
# what this file, run in float32, shows on the case: max flip_gap of the run on X and the run on 1 - X from the flipped start
# = 2.38e-07, measured on the CPU (tests/test_centering.py::test_fit_flip_deviation_of_the_twins keeps the figure honest)
FIT_F32_DEVIATION = 2.4e-7


def fit_case():
    """float32 start of the case: State (offsets at the defaults of fit: data mean, 0.5), X, particles"""
    rng = np.random.RandomState(20241020)
    n = FIT_N
    X = (rng.rand(FIT_ROWS, n[0]) < 0.35).astype(np.float32)
    s = State(list(n), rng, scale=0.3).astype(np.float32)
    s.o = [X.astype(np.float64).mean(0).astype(np.float32)] + [np.full(m, 0.5, np.float32) for m in n[1:]]
    particles = [rng.rand(FIT_BATCH, m).astype(np.float32) for m in n]
    return s, X, particles


def fit_run(s, X, particles, dtype):
    """FIT_EPOCHS epochs of sequential batches, persistent particles, means only, in `dtype`"""
    s = s.astype(dtype)
    X, particles = X.astype(dtype), [p.astype(dtype) for p in particles]
    for _ in range(FIT_EPOCHS):
        for r in range(0, FIT_ROWS, FIT_BATCH):
            pos, neg, particles = dbm_phases(s, X[r:r + FIT_BATCH], particles, n_mf=FIT_MF, k=1)
            update_standard(s, pos, neg, [FIT_NU] * len(s.n), FIT_LR, mom=FIT_MOM)
    return s
