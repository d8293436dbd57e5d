"""CPU twin of the semi-supervised training of a classification RBM (bm_rbm_class_unsup_train_step / _chain,
bm_rbm_class_semi_train_epoch), for the tests.

Built from tests/class_joint_twin.py: its cb_pass and chain run the CD-k chain on (x, y0), its apply_head and the oracle's update
move the parameters; p(y|x) and t = x W + hb are tests/np_reference_class.forward in float32.  The posterior draw, the marginal
hidden means and the U / yb sums of an unlabelled batch are NumPy in the kernels' stated orders.
"""
import ctypes as C

import numpy as np

from boltzmann_machines_amd.utils import philox
from oracle import oracle as orc
from tests import class_joint_twin as J
from tests import np_reference_class as R

SITE_CLASS_Y0 = 14           # csrc/bm_rbm.hip: the start class of the unlabelled chain (one uniform per row, step 0)
f32 = np.float32


def posterior(p, X):
    """(prob [B][C] = float32(exp(log p(c|x))), t [B][H] = x W + hb): np_reference_class.forward with the precisions of the CR
    pass and class_row_kernel - t, every softplus and the partial sums of the 16-column slots in float32, the sum of the slots,
    the logsumexp and exp in double, prob rounded to float32 once.  (np_reference_class.forward in float32 throughout carries
    the whole sum over the hidden units in float32 and is ~1e-5 off in prob: more than the posterior draw's margin allows for)"""
    pf = R.cast(p, f32)
    z = (np.asarray(X, f32).dot(pf['W']) + pf['hb']).astype(f32)
    sp = R.softplus((z[:, None, :] + pf['U'][None, :, :]).astype(f32)).astype(f32)
    H = sp.shape[2]
    sp = np.concatenate([sp, np.zeros(sp.shape[:2] + ((-H) % 16,), f32)], axis=2).reshape(sp.shape[0], sp.shape[1], -1, 16)
    slot = np.zeros(sp.shape[:3], f32)
    for i in range(16):
        slot = (slot + sp[..., i]).astype(f32)
    s = pf['yb'].astype(np.float64)[None, :] + slot.astype(np.float64).sum(axis=2)
    m = s.max(axis=1, keepdims=True)
    L = s - (m + np.log(np.exp(s - m).sum(axis=1, keepdims=True)))
    return np.exp(L).astype(f32), z


def posterior_draw(prob, seed, call, row0=0, margins=None):
    """class_posterior_kernel: per row the prob values widened to double; total and the prefix sums over the classes in ascending
    order; one float32 uniform at flat index row0 + j of SITE_CLASS_Y0; y0 = the lowest c with u * total < prefix_c, C - 1 if
    none; entropy = -sum_c p_c log p_c in double, ascending, zero p_c contributing 0, rounded to float once; max_c p_c.
    margins (a list): every draw's min_c |u * total - prefix_c| / total is appended.  Returns (y0, entropy, confidence)"""
    P = np.asarray(prob, f32).astype(np.float64)
    B, C_ = P.shape
    u = philox.uniform(seed, SITE_CLASS_Y0, call, B, idx0=row0).astype(np.float64)
    y0, ent, conf = np.zeros(B, np.int32), np.zeros(B, f32), np.zeros(B, f32)
    for j in range(B):
        total = 0.0
        for c in range(C_):
            total = total + P[j, c]
        thr, pre, got, found, marg, e, mx = u[j] * total, 0.0, C_ - 1, False, np.inf, 0.0, P[j, 0]
        for c in range(C_):
            pre = pre + P[j, c]
            if c < C_ - 1:
                marg = min(marg, abs(thr - pre) / total)
            if not found and thr < pre:
                got, found = c, True
            if P[j, c] > 0:
                e = e - P[j, c] * np.log(P[j, c])
            mx = P[j, c] if P[j, c] > mx else mx
        y0[j], ent[j], conf[j] = got, f32(e), f32(mx)
        if margins is not None:
            margins.append(marg)
    return y0, ent, conf


def marginal(prob, T, U):
    """class_marginal_kernel: em = E[h | x] with y summed out, the classes in ascending order, fma(p_c, sigmoid(t + U[c]), em)"""
    em = np.zeros_like(T, dtype=f32)
    for c in range(U.shape[0]):
        em = J._fma(prob[:, c][:, None], J.sigmoid32((T + U[c][None, :]).astype(f32)), em)
    return em


def unsup_sums(prob, T, U, yk, hk):
    """the raw sums of class_unsup_update_kernel, float32 in its order: for U[c][i] wave w of 4 takes the rows w, w + 4, ... in
    ascending order - per row fma(p_jc, sigmoid(t_ji + U[c][i]), .), then - hk_ji where yk_j == c - and the four partial sums
    meet as (s0 + s1) + (s2 + s3); for yb[c] lane l of 64 takes the rows l, l + 64, ... adding p_jc - 1[yk_j == c], and the 64
    sums meet in a butterfly (offsets 32 .. 1)"""
    B, H = T.shape
    C_ = U.shape[0]
    sU, syb = np.zeros((C_, H), f32), np.zeros(C_, f32)
    lanes = np.arange(64)
    for c in range(C_):
        S = J.sigmoid32((T + U[c][None, :]).astype(f32))
        part = np.zeros((4, H), f32)
        for w in range(4):
            s = np.zeros(H, f32)
            for j in range(w, B, 4):
                s = J._fma(prob[j, c], S[j], s)
                if yk[j] == c:
                    s = (s - hk[j]).astype(f32)
            part[w] = s
        sU[c] = ((part[0] + part[1]).astype(f32) + (part[2] + part[3]).astype(f32)).astype(f32)
        lane = np.zeros(64, f32)
        for j in range(B):
            lane[j % 64] = f32(lane[j % 64] + f32(prob[j, c] - f32(yk[j] == c)))
        for off in (32, 16, 8, 4, 2, 1):
            lane = (lane + lane[lanes ^ off]).astype(f32)
        syb[c] = lane[0]
    return sU, syb


def unsup_chain(p, X, k, seed, call, row0=0, sample_v=False, sample_h=True, margins=None, y0_margins=None):
    """bm_rbm_class_unsup_chain: dict(prob, T, y0, entropy, confidence, em, h0s, vk, yk, hk)"""
    X = np.ascontiguousarray(X, f32)
    prob, T = posterior(p, X)
    y0, ent, conf = posterior_draw(prob, seed, call, row0, y0_margins)
    ch = J.chain(p, X, y0, k, seed, call, row0, sample_v, sample_h, margins)
    _, h0s = J.cb_pass(p, X, y0, 1, seed, J.SITE_H0, call, row0)
    return dict(prob=prob, T=T, y0=y0, entropy=ent, confidence=conf, em=marginal(prob, T, p['U']), h0s=h0s, vk=ch['vk'], yk=ch['yk'],
                hk=ch['hk'])


class SemiRBM(J.JointRBM):
    """JointRBM plus the unlabelled update and the interleaved epoch"""

    def __init__(self, *a, **kw):
        super(SemiRBM, self).__init__(*a, **kw)
        self.y0_margins = []
        self.last_unsup = None

    def unsup_step(self, X, k, lr, mom, row0=0):
        """one update on unlabelled rows; returns (mean posterior entropy, mean max_c p(c|x)) of the forward pass before it"""
        X = np.ascontiguousarray(X, f32)
        B, p = len(X), self.params()
        ch = unsup_chain(p, X, k, self.seed, self.call, row0, self.sample_v, self.sample_h, self.margins, self.y0_margins)
        self.last_unsup = ch
        sU, syb = unsup_sums(ch['prob'], ch['T'], p['U'], ch['yk'], ch['hk'])
        J.apply_head(self.head, sU, syb, B, lr, mom, self.l2)
        em, vk, hk = (np.ascontiguousarray(a, f32) for a in (ch['em'], ch['vk'], ch['hk']))
        z = np.zeros((B, max(X.shape[1], em.shape[1])), f32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        w = orc.RbmWork(ptr(X), ptr(em), ptr(z), ptr(z), ptr(vk), ptr(hk), ptr(z))
        raw = np.zeros(X.shape[1] * em.shape[1] + X.shape[1] + 2 * em.shape[1], f32)
        orc.lib().orc_rbm_raw_grads(C.byref(self.rbm.cfg), C.byref(w), B, raw)
        self.rbm.apply(raw, float(B), lr, mom)
        self.call += 1
        self.rbm.call = self.call
        return float(ch['entropy'].astype(np.float64).mean()), float(ch['confidence'].astype(np.float64).mean())

    def semi_epoch(self, X, y, Xu, u_slice, batch, k, lr, mom, gamma=0.0, unl_weight=1.0):
        """bm_rbm_class_semi_train_epoch: per labelled batch the joint update, then one unlabelled update with
        float32(lr * unl_weight) on the next slice of Xu (cyclic).  Returns the slice cursor after the epoch"""
        lr_u = float(f32(f32(lr) * f32(unl_weight)))
        n_slices = 0 if Xu is None else (len(Xu) + batch - 1) // batch
        u = u_slice
        for s in range(0, len(X), batch):
            self.train_step(X[s:s + batch], y[s:s + batch], k, lr, mom, gamma)
            if unl_weight > 0:
                self.unsup_step(Xu[u * batch:(u + 1) * batch], k, lr_u, mom)
                u = (u + 1) % n_slices
        return u


def positive_stats64(p, X):
    """float64: (X^T em, colsum em, sum_j p_jc S_jci [C][H], sum_j p_jc [C]) and em itself - the gradient of
    sum_j (x_j . vb + logsumexp_c s_c(x_j)) in W, hb, U, yb (its gradient in vb is colsum X)"""
    p = R.cast(p, np.float64)
    X = np.asarray(X, np.float64)
    L, z = R.forward(p, X, np.float64)
    P = np.exp(L)
    S = R.sigmoid(z[:, None, :] + p['U'][None, :, :])
    em = (P[:, :, None] * S).sum(axis=1)
    return dict(W=X.T.dot(em), hb=em.sum(axis=0), U=(P[:, :, None] * S).sum(axis=0), yb=P.sum(axis=0), vb=X.sum(axis=0)), em


def log_px_unnorm64(p, X):
    """float64: sum_j (x_j . vb + logsumexp_c s_c(x_j)) = sum_j log sum_y p*(x_j, y), the unnormalised log-probability"""
    p = R.cast(p, np.float64)
    X = np.asarray(X, np.float64)
    z = X.dot(p['W']) + p['hb']
    s = p['yb'][None, :] + R.softplus(z[:, None, :] + p['U'][None, :, :]).sum(axis=2)
    m = s.max(axis=1, keepdims=True)
    return float((X.dot(p['vb']) + m[:, 0] + np.log(np.exp(s - m).sum(axis=1))).sum())


def float64_unsup_update(p0, X, ch, lr, mom, l2):
    """the unlabelled update in float64 on given chain states (vk, yk, hk): exact positive phase, the update rules of the twin"""
    p = R.cast(p0, np.float64)
    B, C_ = len(X), p['U'].shape[0]
    pos, _ = positive_stats64(p, X)
    X64, vk, hk = (np.asarray(a, np.float64) for a in (X, ch['vk'], ch['hk']))
    Yk = np.eye(C_)[ch['yk']]
    g = dict(W=(pos['W'] - vk.T.dot(hk)) / B, hb=(pos['hb'] - hk.sum(axis=0)) / B, vb=(X64 - vk).mean(axis=0),
             U=(pos['U'] - Yk.T.dot(hk)) / B, yb=(pos['yb'] - Yk.sum(axis=0)) / B)
    lr, mom, l2 = (np.float64(f32(v)) for v in (lr, mom, l2))
    for w in ('W', 'U'):
        p['d' + w] = lr * (mom * p['d' + w] + (g[w] - l2 * p[w]))
        p[w] = p[w] + p['d' + w]
    for b in ('hb', 'vb', 'yb'):
        p['d' + b] = lr * (mom * p['d' + b] + g[b])
        p[b] = p[b] + p['d' + b]
    return p
