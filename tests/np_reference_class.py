"""NumPy restatement of the class head of a Bernoulli RBM (include/bm355.h: bm_rbm_set_classes, bm_rbm_class_*).

    z_i        = (x W)_i + hb_i
    s_c        = yb_c + sum_i softplus(z_i + U[c][i])
    log p(c|x) = s_c - logsumexp_c' s_c'

and the exact gradient of the batch mean of log p(t|x), which the update ascends:

    coef[j][c] = 1[c == t_j] - p(c|x_j),   S[j][c][i] = sigmoid(z_ji + U[c][i])
    g  = S[j][t_j][i] - sum_c p(c|x_j) S[j][c][i]
    dW = X^T g / B,  dhb = colmean(g),  dvb = 0,  dU[c][i] = sum_j coef[j][c] S[j][c][i] / B,  dyb[c] = colmean(coef[:, c])

with the update rules of the CD update: W and U  g -= l2 w; d = lr (mom d + g); w += d;  the biases  d = lr (mom d + g); b += d.

Every function takes `dt`: np.float64 is the reference; np.float32 is the "twin" - float32 GEMM, float32 epilogue, the same
update rule - which exists only to size tolerances (how far honest float32 arithmetic lands from float64 on the same inputs).
"""
import numpy as np

NAMES = ('W', 'hb', 'vb', 'U', 'yb', 'dW', 'dhb', 'dvb', 'dU', 'dyb')


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def cast(params, dt):
    return {k: np.array(v, dtype=dt) for k, v in params.items()}


def forward(p, X, dt=np.float64):
    """log p(c|x) [B, C] and the pre-activations z [B, H], all arithmetic in `dt`"""
    X = np.asarray(X, dtype=dt)
    z = X.dot(p['W'].astype(dt)) + p['hb'].astype(dt)
    s = p['yb'].astype(dt)[None, :] + softplus(z[:, None, :] + p['U'].astype(dt)[None, :, :]).sum(axis=2, dtype=dt)
    m = s.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(axis=1, keepdims=True, dtype=dt))
    return (s - lse).astype(dt), z


def mean_log_proba(p, X, y, dt=np.float64):
    L, _ = forward(p, X, dt)
    return float(L[np.arange(len(y)), y].astype(np.float64).mean())


def gradients(p, X, y, dt=np.float64, keep=None):
    """the ascent direction of the batch mean of log p(t|x): dict(W, hb, vb, U, yb), and the forward pass's (mean log p(t|x),
    accuracy).  keep [B] bool (or None): rows with False contribute nothing to any sum - the divisor stays B"""
    X = np.asarray(X, dtype=dt)
    B, C = len(X), p['U'].shape[0]
    keep = np.ones(B, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    t = np.where(keep, y, 0)
    L, z = forward(p, X, dt)
    P = np.exp(L)
    S = sigmoid(z[:, None, :] + p['U'].astype(dt)[None, :, :])           # [B, C, H]
    coef = ((np.arange(C)[None, :] == t[:, None]).astype(dt) - P) * keep[:, None].astype(dt)
    g = (S[np.arange(B), t, :] - (P[:, :, None] * S).sum(axis=1, dtype=dt)) * keep[:, None].astype(dt)
    n = dt(B)
    grads = dict(W=X.T.dot(g) / n, hb=g.sum(axis=0, dtype=dt) / n, vb=np.zeros(X.shape[1], dtype=dt),
                 U=(coef[:, :, None] * S).sum(axis=0, dtype=dt) / n, yb=coef.sum(axis=0, dtype=dt) / n)
    lp = L[np.arange(B), t].astype(np.float64) * keep
    hit = (L.argmax(axis=1) == t) & keep
    return grads, (float(lp.sum() / B), float(hit.sum() / float(B)))


def step(p, X, y, lr, mom, l2, dt=np.float64, keep=None):
    """one update in place of a copy: returns (new params, (mean log p(t|x), accuracy) of the forward pass before it)"""
    p = cast(p, dt)
    g, out2 = gradients(p, X, y, dt, keep)
    lr, mom, l2 = dt(lr), dt(mom), dt(l2)
    for w in ('W', 'U'):
        gw = g[w] - l2 * p[w]
        p['d' + w] = lr * (mom * p['d' + w] + gw)
        p[w] = p[w] + p['d' + w]
    for b in ('hb', 'vb', 'yb'):
        p['d' + b] = lr * (mom * p['d' + b] + g[b])
        p[b] = p[b] + p['d' + b]
    return p, out2


def epoch(p, X, y, batch, lr, mom, l2, dt=np.float64):
    """consecutive batches of `batch` rows (a short last one); (params, (mean log p, accuracy) over the rows, each batch's
    taken before its update)"""
    N, lp, acc = len(X), 0.0, 0.0
    for s in range(0, N, batch):
        Xb, yb = X[s:s + batch], y[s:s + batch]
        p, (l, a) = step(p, Xb, yb, lr, mom, l2, dt)
        lp += l * len(Xb)
        acc += a * len(Xb)
    return p, (lp / N, acc / N)


def max_dev(a, b):
    """max |a - b| over the entries, in float64"""
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))
