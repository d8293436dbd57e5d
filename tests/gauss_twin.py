"""CPU twin of a Gaussian-visible RBM as ONE joint model (bm_rbm_gauss_ais, bm_rbm_gauss_free_energy_rows, bm_rbm_gauss_pt_*;
csrc/bm_gauss.h), for the tests, and ground truth by enumeration of the hidden layer.

    u = x / sigma,  c = fl32(vb / sigma):   E(u, h) = 1/2 |u - c|^2 - u W h - hb.h
    h | u ~ Ber(sigmoid(u W + hb)),   u | h ~ N(c + W h, I),   x = sigma u

Built from what exists, in the style of tests/pt_twin.py and tests/nrelu_twin.py:
  * contractions and Bernoulli draws are tests/clamp_twin.act2 (orc_act2: what act_kernel computes), called with the engine's seed /
    site / call / row0; a tempered prop-up is one call per distinct temperature with mult = bmult = beta (pt_twin's rule);
  * m = z + c is its call with kind 2, mult 1 and a unit sigma: (1 * z) * 1 + 1 * c, one rounded add; the raw beta z of an AIS
    transition is the same call with mult = beta and a zero bias;
  * normals are orc.normal at the flat index (row0 + j) * V + i;
  * every other step is ONE float32 NumPy operation (c + n sd, m + n sd, u - c, -0.5 d, (-0.5 d) d, a + beta_k d, u sigma, x / sigma);
  * slot partials are pt_twin.slot_partials, the swap is pt_twin.Ensemble's own;
  * AIS scores are float64 re-scorings of the float32 states (the engine's are double sums of float32 partials).
The ensemble exposes every replica row, not only the beta = 1 rows.  Nothing under oracle/ is involved beyond the calls named above.
"""
import numpy as np

from oracle import oracle as orc
from tests import pt_twin
from tests.clamp_twin import SITE_H, SITE_V, act2
from tests.np_reference import softplus

SITE_AIS_V0, SITE_AIS_V, SITE_AIS_H = 7, 8, 9            # csrc/bm_rbm.hip
SITE_PT_V0 = pt_twin.SITE_PT_V0
f32, f64 = np.float32, np.float64


def params(p):
    """(W, hb, c, sigma) float32, c = fl32(vb / sigma)"""
    W = np.ascontiguousarray(p['W'], f32)
    sigma = np.ascontiguousarray(p.get('sigma', np.ones(W.shape[0], f32)), f32)
    vb, hb = np.ascontiguousarray(p['vb'], f32), np.ascontiguousarray(p['hb'], f32)
    return W, hb, (vb / sigma).astype(f32), sigma


def scale_in(X, sigma):
    return (np.asarray(X, f32) / np.asarray(sigma, f32)).astype(f32)


def scale_out(U, sigma):
    return (np.asarray(U, f32) * np.asarray(sigma, f32)).astype(f32)


def normals(seed, site, call, row0, J, I):
    return orc.normal(int(seed), int(site), int(call), J * I, idx0=int(row0) * I).reshape(J, I)


def ladder_sd(betas):
    """sd[r] = float32(1 / sqrt(double(beta_r)))"""
    return (1.0 / np.sqrt(np.asarray(betas, f32).astype(f64))).astype(f32)


def sq_terms(u, c):
    """-1/2 (u - c)^2 in three rounded steps: d = u - c, e = -0.5 d, e d"""
    d = (np.asarray(u, f32) - c).astype(f32)
    return ((f32(-0.5) * d).astype(f32) * d).astype(f32)


# ---- AIS
def base_mean(X, sigma):
    """a = mean(X / sigma) as GaussianRBM.ais_log_Z(X_base=X) hands it to the engine"""
    return scale_in(X, sigma).astype(f64).mean(axis=0).astype(f32)


def betas32(n_betas):
    return np.linspace(0., 1., n_betas).astype(f32)


def log_Z0(p, a=None):
    W, hb, c, sigma = params(p)
    V, H = W.shape
    a = np.zeros(V) if a is None else np.asarray(a, f32).astype(f64)
    c = c.astype(f64)
    return 0.5 * V * np.log(2. * np.pi) + H * np.log(2.) + np.sum(np.log(sigma.astype(f64))) + 0.5 * (a.dot(a) - c.dot(c))


def ais(p, n_betas, n_runs, k, seed, chain0=0, a=None):
    """-> (values [n_runs] float64, u [n_runs][V], h [n_runs][H]: the float32 chain states behind the last transition)"""
    W, hb, c, sigma = params(p)
    Wt = np.ascontiguousarray(W.T)
    V, H = W.shape
    R = int(n_runs)
    a32 = np.zeros(V, f32) if a is None else np.ascontiguousarray(a, f32)
    d32 = (c - a32).astype(f32)                                    # rbm_ais_prep_kernel: dvec = c - a
    b32 = betas32(n_betas)
    W64, hb64, d64 = W.astype(f64), hb.astype(f64), d32.astype(f64)
    zeros, ones = np.zeros(V, f32), np.ones(V, f32)
    u = (a32 + normals(seed, SITE_AIS_V0, 0, chain0, R, V)).astype(f32)
    h = np.zeros((R, H), f32)
    logw = np.zeros(R)
    for step in range(1, n_betas):
        ba, bb = b32[step - 1], b32[step]
        z = u.astype(f64).dot(W64) + hb64
        logw += f64(f32(bb - ba)) * u.astype(f64).dot(d64) + np.sum(softplus(f64(bb) * z) - softplus(f64(ba) * z), axis=1)
        if step == n_betas - 1:
            break
        table = (a32 + (bb * d32).astype(f32)).astype(f32)         # rbm_ais_prep_kernel: a + beta_k (c - a), two rounded steps
        for t in range(k):
            _, h = act2(u, W, None, None, hb, None, float(bb), 0, 1, seed, SITE_AIS_H + 16 * t, step, chain0)
            bz, _ = act2(h, Wt, None, None, zeros, ones, float(bb), 2, 0, 0, 0, 0, 0)          # fl(beta z)
            m = (bz + table).astype(f32)
            u = (normals(seed, SITE_AIS_V + 16 * t, step, chain0, R, V) + m).astype(f32)
    return logw + log_Z0(p, a32), u, h


def log_mean_and_se(values):
    """(log_mean_exp, its delta-method standard error std(w) / (mean(w) sqrt(n)), w = exp(values))"""
    x = np.asarray(values, f64)
    w = np.exp(x - x.max())
    return float(x.max() + np.log(w.mean())), float(w.std(ddof=1) / (w.mean() * np.sqrt(len(w))))


# ---- parallel tempering
class Ensemble(pt_twin.Ensemble):
    """M chains x R replicas over u, chain-major rows; _swap and the counters are pt_twin.Ensemble's, with part_v = the slots of
    -1/2 (u - c)^2 and part_h = the slots of h.(u W + hb)"""

    def __init__(self, p, n_chains, betas, seed, call=0, chain0=0, V0=None):
        """V0 [M][V] in data units: every chain's replicas start at fl32(V0 / sigma); None: u_0 = c + n sd_r at site 11 of `call`"""
        self.W, self.hb, self.c, self.sigma = params(p)
        self.Wt = np.ascontiguousarray(self.W.T)
        self.V, self.H = self.W.shape
        self.betas = np.ascontiguousarray(betas, f32).ravel()
        self.sd = ladder_sd(self.betas)
        self.M, self.R, self.seed, self.chain0 = int(n_chains), len(self.betas), int(seed), int(chain0)
        rows = self.M * self.R
        self.mult = np.tile(self.betas, self.M)
        self.idx = np.tile(np.arange(self.R, dtype=np.int32), self.M)
        if V0 is not None:
            v = np.repeat(scale_in(V0, self.sigma), self.R, axis=0)
        else:
            n = normals(seed, SITE_PT_V0, call, self.chain0 * self.R, rows, self.V)
            v = (self.c + (n * self.sd[self.idx][:, None]).astype(f32)).astype(f32)
        assert v.shape == (rows, self.V)
        self.v, self.h = v, np.zeros((rows, self.H), f32)
        self.part_v = pt_twin.slot_partials(sq_terms(v, self.c))
        self.part_h = None
        self.cnt = np.zeros((2, max(self.R - 1, 0)), np.int64)
        self.step = 0
        self.margins = []

    def sweep(self, n_steps, call=0):
        """bm_rbm_gauss_pt_sweep: per step t the tempered prop-up, the swap of parity (global step) & 1, the prop-down around the
        untempered mean with the row's standard deviation"""
        ones_h, ones_v = np.ones(self.H, f32), np.ones(self.V, f32)
        row0 = self.chain0 * self.R
        rows = self.M * self.R
        for t in range(n_steps):
            self.h = self._tempered(self.v, self.W, self.hb, SITE_H + 16 * t, call)
            zb, _ = act2(self.v, self.W, None, None, self.hb, ones_h, 1.0, 2, 0, self.seed, SITE_H + 16 * t, call, row0)
            self.part_h = pt_twin.slot_partials(self.h * zb)
            if self.R > 1:
                self._swap(t, call)
            m, _ = act2(self.h, self.Wt, None, None, self.c, ones_v, 1.0, 2, 0, self.seed, SITE_V + 16 * t, call, row0)
            n = normals(self.seed, SITE_V + 16 * t, call, row0, rows, self.V)
            self.v = (m + (n * self.sd[self.idx][:, None]).astype(f32)).astype(f32)
            self.part_v = pt_twin.slot_partials(sq_terms(self.v, self.c))
            self.step += 1

    def read(self):
        """(X [M][V] in data units, H [M][H]) of the beta = 1 rows"""
        rows = np.arange(self.M) * self.R + np.argmax(self.idx.reshape(self.M, self.R) == self.R - 1, axis=1)
        return scale_out(self.v[rows], self.sigma), self.h[rows].copy()

    def state(self):
        """the whole ensemble under the names of RbmGaussPt.pt_state"""
        return dict(v=self.v, h=self.h, part_v=np.ascontiguousarray(self.part_v.T), part_h=np.ascontiguousarray(self.part_h.T),
                    mult=self.mult, idx=self.idx, swaps=self.cnt)


def plain_chain(p, V0, n_steps, seed, call=0, row0=0):
    """n_steps of h ~ p(h|u), u ~ N(c + W h, I) from u_0 = fl32(V0 / sigma), with no ensemble around it -> (X, H)"""
    W, hb, c, sigma = params(p)
    Wt = np.ascontiguousarray(W.T)
    ones = np.ones(W.shape[0], f32)
    u = scale_in(V0, sigma)
    h = None
    for t in range(n_steps):
        _, h = act2(u, W, None, None, hb, None, 1.0, 0, 1, seed, SITE_H + 16 * t, call, row0)
        m, _ = act2(h, Wt, None, None, c, ones, 1.0, 2, 0, 0, 0, 0, 0)
        u = (m + normals(seed, SITE_V + 16 * t, call, row0, u.shape[0], u.shape[1])).astype(f32)
    return scale_out(u, sigma), h


# ---- float64 statements and ground truth by enumeration of h
def _bits(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(f64)


def _lse(x):
    m = np.max(x)
    return float(m + np.log(np.sum(np.exp(x - m))))


def free_energy64(p, X):
    """F(x / sigma) = 1/2 |u - c|^2 - sum_j softplus((u W + hb)_j), u = fl32(x / sigma), everything behind u and c in float64"""
    W, hb, c, sigma = params(p)
    u = scale_in(X, sigma).astype(f64)
    return 0.5 * np.sum((u - c.astype(f64)) ** 2, axis=1) - np.sum(softplus(u.dot(W.astype(f64)) + hb.astype(f64)), axis=1)


def _hidden_terms(p):
    """(h [2^H][H], W h [2^H][V], t_h = hb.h + c.(W h) + 1/2 |W h|^2)"""
    W, hb, c, _ = params(p)
    h = _bits(W.shape[1])
    Wh = h.dot(W.astype(f64).T)
    return h, Wh, h.dot(hb.astype(f64)) + Wh.dot(c.astype(f64)) + 0.5 * np.sum(Wh * Wh, axis=1)


def exact_log_Z(p, data_units=True):
    """log Z~ = (V/2) log 2 pi + logsumexp_h t_h over u; + sum_i log sigma_i over x"""
    W, _, _, sigma = params(p)
    lz = 0.5 * W.shape[0] * np.log(2. * np.pi) + _lse(_hidden_terms(p)[2])
    return lz + (float(np.sum(np.log(sigma.astype(f64)))) if data_units else 0.0)


def exact_tempered(p, beta):
    """under p_beta ~ exp(-beta E): (p_beta(h) [2^H], E[u] [V], Cov[u] [V][V], the fourth central moments of u [V])"""
    W, _, c, _ = params(p)
    h, Wh, t = _hidden_terms(p)
    lp = beta * t
    ph = np.exp(lp - _lse(lp))
    mu_h = c.astype(f64)[None, :] + Wh                                 # the mean of u given h
    mean = ph.dot(mu_h)
    dev = mu_h - mean[None, :]
    cov = np.eye(W.shape[0]) / beta + (dev * ph[:, None]).T.dot(dev)
    m4 = ph.dot(dev ** 4 + 6. * dev ** 2 / beta + 3. / beta ** 2)      # a mixture of normals of variance 1 / beta
    return ph, mean, cov, m4


# ---- shared cases of tests/test_gauss_joint.py and tests/test_gauss_joint_gpu.py
def make_params(V, H, std=0.3, seed=3):
    """float32 W ~ N(0, std^2), vb, hb ~ U(-0.5, 0.5), sigma ~ U(0.5, 1.5) (none equal to 1) from NumPy's generator"""
    rng = np.random.RandomState(seed)
    return dict(W=(std * rng.randn(V, H)).astype(f32), vb=rng.uniform(-0.5, 0.5, V).astype(f32), hb=rng.uniform(-0.5, 0.5, H).astype(f32),
                sigma=rng.uniform(0.5, 1.5, V).astype(f32))


def data(N, V, seed, sigma=None):
    """real-valued rows around two centres, in data units"""
    rng = np.random.RandomState(seed)
    X = rng.randn(N, V) + np.where(rng.rand(N, 1) < 0.5, 1.0, -0.5)
    return (X * (1.0 if sigma is None else np.asarray(sigma, f64))).astype(f32)


def bimodal_params(w=8.0, p1=0.3, sigma=(0.5, 2.0)):
    """V = 2, H = 1: the modes u = c (h = 0) and u = c + W (h = 1), |W| = w sqrt(2) standard deviations apart, p(h = 1) = p1:
    hb = logit(p1) - c.W - 1/2 |W|^2"""
    W = np.array([[w], [w]], f32)
    sigma = np.array(sigma, f32)
    vb = np.array([0.25, -0.5], f32)
    c = (vb / sigma).astype(f64)
    hb = np.log(p1 / (1. - p1)) - c.dot(W[:, 0].astype(f64)) - 0.5 * float(np.sum(W.astype(f64) ** 2))
    return dict(W=W, vb=vb, hb=np.array([hb], f32), sigma=sigma)


def mode_of(p, X):
    """0 / 1: which of the two modes of a bimodal_params model a row of X (data units) is nearer to"""
    W, _, c, sigma = params(p)
    u = scale_in(X, sigma).astype(f64)
    w = W[:, 0].astype(f64)
    return ((u - c.astype(f64)).dot(w) > 0.5 * w.dot(w)).astype(np.int64)
