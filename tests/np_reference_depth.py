"""AIS log Z and the ELBO for binary DBMs of any depth: a float64 NumPy restatement (extends tests/np_reference.py,
whose NumpyDBM handles the 2-layer AIS of reference dbm.py:650-759), and exact ground truth by enumeration.

Depth d = 0 is the visible layer, depth d = i + 1 the hidden layer i; W_d connects depths d and d + 1.  The AIS chain x
is the odd-depth layers {h1, h3}; the even-depth layers {v, h2, h4} are conditionally independent given x and summed
out analytically:
    log p*_beta(x) = beta sum_{odd d} b_d.x_d + sum_{even d} sum_i softplus(beta a_{d,i}),
a_d = s_{d-1} W_{d-1} + s_{d+1} W_d^T + b_d (the neighbours that exist).  One transition step draws the even-depth
layers in ascending depth given x, then the odd-depth layers in ascending depth given them.  RNG: the pinned Philox
stream of DbmEngine - site 12 for v, 8 + i for hidden layer i, counter word site + 16 t, call = beta step, global
chain index as row offset; x_0 ~ Ber(1/2) of the j-th odd-depth layer from site 13 + 16 j, call 0."""
import numpy as np

from boltzmann_machines_amd.utils import philox
from tests.np_reference import NumpyDBM, _sfx, sigmoid, softplus


def _W(P, d):
    return P['W' + _sfx(d)]


def _b(P, d):
    return P['vb'] if d == 0 else P['hb' + _sfx(d - 1)]


def _widths(P, L):
    return [_W(P, 0).shape[0]] + [_W(P, d).shape[1] for d in range(L)]


def _pre(P, L, d, S):
    """a_d without beta: the input from the neighbours of depth d in S (dict depth -> states) plus the bias"""
    a = _b(P, d)
    if d > 0:
        a = a + S[d - 1].dot(_W(P, d - 1))
    if d < L:
        a = a + S[d + 1].dot(_W(P, d).T)
    return a


def log_p_star(P, L, x, beta=1.):
    """log p*_beta(x) of the odd-depth states x (dict depth -> [R][n_d])"""
    R = len(next(iter(x.values())))
    lp = np.zeros(R)
    for d in range(1, L + 1, 2):
        lp = lp + x[d].dot(_b(P, d)) * beta
    for d in range(0, L + 1, 2):
        lp = lp + np.sum(softplus(_pre(P, L, d, x) * beta), axis=1)
    return lp


def _bits(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)


def _odd_configs(P, L):
    """every configuration of the odd-depth layers: dict depth -> [2^(sum n_odd)][n_d]"""
    n = _widths(P, L)
    odd = list(range(1, L + 1, 2))
    allb = _bits(sum(n[d] for d in odd))
    x, c = {}, 0
    for d in odd:
        x[d] = allb[:, c:c + n[d]]
        c += n[d]
    return x


def _lse(a, axis=None):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def exact_log_Z(P, L):
    """log Z by enumeration of the odd-depth layers, the even-depth layers summed analytically (float64)"""
    return float(_lse(log_p_star(P, L, _odd_configs(P, L))))


def exact_log_p(P, L, X):
    """log p(v) per row of X: the hidden odd-depth layers enumerated given v, the hidden even-depth layers summed
    analytically, minus exact_log_Z"""
    x = _odd_configs(P, L)
    X = np.asarray(X, dtype=np.float64)
    out = np.empty(len(X))
    for r, v in enumerate(X):
        lp = x[1].dot(v.dot(_W(P, 0)))
        for d in range(1, L + 1, 2):
            lp = lp + x[d].dot(_b(P, d))
        for d in range(2, L + 1, 2):
            lp = lp + np.sum(softplus(_pre(P, L, d, x)), axis=1)
        out[r] = v.dot(P['vb']) + _lse(lp)
    return out - exact_log_Z(P, L)


def brute_log_Z(P, L):
    """log Z by enumeration of every unit (tiny models only): -E = sum_d b_d.s_d + sum_d s_d W_d s_{d+1}"""
    n = _widths(P, L)
    allb = _bits(sum(n))
    S, c = [], 0
    for w in n:
        S.append(allb[:, c:c + w])
        c += w
    negE = sum(S[d].dot(_b(P, d)) for d in range(L + 1))
    negE = negE + sum(np.sum(S[d].dot(_W(P, d)) * S[d + 1], axis=1) for d in range(L))
    return float(_lse(negE))


class DepthDBM(NumpyDBM):
    """NumpyDBM with AIS and the ELBO at any depth (the same P dict and RNG conventions)"""

    def _site(self, d):
        return 12 if d == 0 else 8 + d - 1

    def _sampled(self, d):
        return self.smp_v if d == 0 else self.smp_h[d - 1]

    def log_p_x(self, x, beta):
        return log_p_star(self.P, self.L, x, beta)

    def ais_next(self, x, beta, k, seed, step, chain0):
        """k transition steps T_beta: even depths given x, then odd depths given the new even depths"""
        L, P = self.L, self.P
        x = dict(x)
        for t in range(k):
            S = dict(x)
            for d in range(0, L + 1, 2):
                m = sigmoid(beta * (_pre(P, L, d, S) - _b(P, d)) + beta * _b(P, d))
                S[d] = self._draw(m, self._site(d), t, seed, step, chain0) if self._sampled(d) else m
            for d in range(1, L + 1, 2):
                m = sigmoid(beta * (_pre(P, L, d, S) - _b(P, d)) + beta * _b(P, d))
                x[d] = self._draw(m, self._site(d), t, seed, step, chain0) if self._sampled(d) else m
        return x

    def ais(self, n_betas, n_runs, k, seed, chain0=0):
        """the 2-layer loop of NumpyDBM.ais (:696-736) over the odd-depth state; beta accumulates in float32"""
        R = np.float32
        L, n = self.L, _widths(self.P, self.L)
        x = {}
        for j, d in enumerate(range(1, L + 1, 2)):
            u = philox.uniform(seed, 13 + 16 * j, 0, n_runs * n[d], idx0=chain0 * n[d]).reshape(n_runs, n[d])
            x[d] = (u < R(0.5)).astype(np.float64)
        db = R(1.0) / R(n_betas)
        x = self.ais_next(x, float(db), k, seed, 0, chain0)
        log_Z = -self.log_p_x(x, 0.)
        beta, step = db, 1
        while beta < R(1.) - db + R(1e-5):
            log_Z = log_Z + self.log_p_x(x, float(beta))
            x = self.ais_next(x, float(R(beta + db)), k, seed, step, chain0)
            log_Z = log_Z - self.log_p_x(x, float(beta))
            beta = R(beta + db)
            step += 1
        log_Z = log_Z + self.log_p_x(x, 1.)
        return log_Z + sum(n) * float(np.log(np.float32(2.)))

    def log_proba(self, X):
        """ELBO per row (log Z not subtracted): sum_l sum((mu_{l-1} W_l) * mu_l) + X.vb + sum_l mu_l.hb_l + entropies"""
        X = np.asarray(X, dtype=np.float64)
        self.mean_field(X)
        mu = [self.P['mu' + _sfx(i)] for i in range(self.L)]
        below = [X] + mu[:-1]
        mE = sum(np.sum(below[i].dot(self.W(i)) * mu[i], axis=1) for i in range(self.L))
        mE = mE + X.dot(self.P['vb']) + sum(mu[i].dot(self.hb(i)) for i in range(self.L))
        S = 0.
        for m in mu:
            s = np.clip(m, 1e-7, 1. - 1e-7)
            S = S + np.sum(-s * np.log(s) - (1. - s) * np.log(1. - s), axis=1)
        self.call += 1
        return mE + S
