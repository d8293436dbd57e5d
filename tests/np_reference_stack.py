"""NumPy restatement of fine-tuning a stack of sigmoid layers below a class head (include/bm355.h:
bm_rbm_class_stack_*, bm_rbm_backprop_down, bm_rbm_delta_update).

    a_0 = x,   a_l = sigmoid(a_{l-1} W_l + hb_l)   (l = 1..D)
    log p(c|x) = the class head's posterior (tests/np_reference_class.py) of the top RBM on the input a_D

and the exact gradient of the batch mean of log p(t|x), with g = S[., t, .] - sum_c p(c|x) S[., c, .] of the top:

    delta_D = (g W_top^T)             * a_D * (1 - a_D)
    delta_l = (delta_{l+1} W_{l+1}^T) * a_l * (1 - a_l)
    dW_l = a_{l-1}^T delta_l / B,  dhb_l = colmean(delta_l),  dvb_l = 0;   the top: the class head's gradients on the input a_D

A stack is dict(layers=[dict(W, hb, vb, dW, dhb, dvb), ...] bottom first, top=dict(W, hb, vb, U, yb, dW, ...)).  Every function
takes `dt`: np.float64 is the reference; np.float32 is the twin, which restates the engine's association of the derivative,
(z * a) * (1 - a) with every step rounded once, and exists only to size tolerances.
"""
import numpy as np

from tests import np_reference_class as R

LAYER_NAMES = ('W', 'hb', 'vb', 'dW', 'dhb', 'dvb')
max_dev = R.max_dev


def cast(stack, dt):
    return dict(layers=[R.cast(l, dt) for l in stack['layers']], top=R.cast(stack['top'], dt))


def activations(stack, X, dt=np.float64):
    """[a_0 .. a_D], all arithmetic in `dt`"""
    a = [np.asarray(X, dtype=dt)]
    for l in stack['layers']:
        a.append(R.sigmoid(a[-1].dot(l['W'].astype(dt)) + l['hb'].astype(dt)).astype(dt))
    return a


def log_proba(stack, X, dt=np.float64):
    return R.forward(stack['top'], activations(stack, X, dt)[-1], dt)[0]


def mean_log_proba(stack, X, y, dt=np.float64):
    L = log_proba(stack, X, dt)
    return float(L[np.arange(len(y)), y].astype(np.float64).mean())


def sigmoid_derivative(z, a, dt):
    """z * a * (1 - a) in the association the BP flavour of act_kernel states: (z * a) * (1 - a), three rounded steps"""
    z, a = np.asarray(z, dtype=dt), np.asarray(a, dtype=dt)
    return ((z * a) * (dt(1) - a)).astype(dt)


def top_g(top, A, y, dt, keep):
    """g [B, H_top] of the class head on the input A (rows with keep == False: zeros)"""
    B = len(A)
    t = np.where(keep, y, 0)
    L, z = R.forward(top, A, dt)
    P = np.exp(L)
    S = R.sigmoid(z[:, None, :] + top['U'].astype(dt)[None, :, :])
    return ((S[np.arange(B), t, :] - (P[:, :, None] * S).sum(axis=1, dtype=dt)) * keep[:, None].astype(dt)).astype(dt)


def backward(weights_above, g, acts, dt):
    """[delta_1 .. delta_D] from g of the top; weights_above[l] is the W the pass into layer l + 1 (1-based) reads: W_{l+2}, the
    top's for the last"""
    deltas, d = [None] * (len(acts) - 1), g
    for l in range(len(acts) - 2, -1, -1):
        d = sigmoid_derivative(d.dot(weights_above[l].astype(dt).T), acts[l + 1], dt)
        deltas[l] = d
    return deltas


def layer_gradients(a_in, delta, dt):
    n = dt(len(a_in))
    return dict(W=a_in.T.dot(delta) / n, hb=delta.sum(axis=0, dtype=dt) / n, vb=np.zeros(a_in.shape[1], dtype=dt))


def gradients(stack, X, y, dt=np.float64, keep=None):
    """the ascent direction of the batch mean of log p(t|x): ([dict(W, hb, vb) per layer below], dict(W, hb, vb, U, yb) of the top,
    (mean log p(t|x), accuracy) of the forward pass).  keep as in np_reference_class.gradients"""
    keep = np.ones(len(X), dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    acts = activations(stack, X, dt)
    gtop, out2 = R.gradients(stack['top'], acts[-1], y, dt, keep)
    g = top_g(stack['top'], acts[-1], y, dt, keep)
    above = [l['W'] for l in stack['layers'][1:]] + [stack['top']['W']]
    deltas = backward(above, g, acts, dt)
    return [layer_gradients(acts[l], deltas[l], dt) for l in range(len(deltas))], gtop, out2


def apply_layer(l, g, lr, mom, l2, dt):
    """the update rules of the CD update on one layer, in place: W takes l2, the biases the plain rule"""
    lr, mom, l2 = dt(lr), dt(mom), dt(l2)
    l['dW'] = lr * (mom * l['dW'] + (g['W'] - l2 * l['W']))
    l['W'] = l['W'] + l['dW']
    for b in ('hb', 'vb'):
        l['d' + b] = lr * (mom * l['d' + b] + g[b])
        l[b] = l[b] + l['d' + b]


def step(stack, X, y, lrs, mom, l2s, dt=np.float64, keep=None, stale=False):
    """one update of a copy: (new stack, out2 of the forward pass before it).  lrs, l2s: one value per layer, the top's last.
    stale=True is the WRONG order - every layer is updated before the backward pass through it, so the passes read updated
    weights - kept to show that the stale-weight test can tell the two apart"""
    s = cast(stack, dt)
    D = len(s['layers'])
    keep = np.ones(len(X), dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    acts = activations(s, X, dt)
    g = top_g(s['top'], acts[-1], y, dt, keep)
    if not stale:
        above = [np.array(l['W']) for l in s['layers'][1:]] + [np.array(s['top']['W'])]
        deltas = backward(above, g, acts, dt)
    s['top'], out2 = R.step(s['top'], acts[-1], y, lrs[D], mom, l2s[D], dt, keep)
    d = g
    for l in range(D - 1, -1, -1):
        if stale:
            w = s['layers'][l + 1]['W'] if l + 1 < D else s['top']['W']          # already updated
            d = sigmoid_derivative(d.dot(w.astype(dt).T), acts[l + 1], dt)
        else:
            d = deltas[l]
        apply_layer(s['layers'][l], layer_gradients(acts[l], d, dt), lrs[l], mom, l2s[l], dt)
    return s, out2


def epoch(stack, X, y, batch, lrs, mom, l2s, dt=np.float64):
    """consecutive batches of `batch` rows (a short last one): (stack, (mean log p, accuracy) over the rows, each batch's taken
    before its update)"""
    N, lp, acc = len(X), 0.0, 0.0
    for r in range(0, N, batch):
        stack, (l, a) = step(stack, X[r:r + batch], y[r:r + batch], lrs, mom, l2s, dt)
        n = len(X[r:r + batch])
        lp, acc = lp + l * n, acc + a * n
    return stack, (lp / N, acc / N)


def tensors(stack, names=('W', 'hb')):
    """the trained tensors by name: W1, hb1, ... of the layers below, W, hb, U, yb of the top"""
    out = {}
    for i, l in enumerate(stack['layers']):
        for n in names:
            out['%s%d' % (n, i + 1)] = l[n]
    for n in tuple(names) + ('U', 'yb'):
        out[n] = stack['top'][n]
    return out
