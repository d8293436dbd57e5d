"""Point sets, one-hot operands and high-precision references that probe the epilogue functions of csrc/bm_numerics.h
element by element THROUGH THE PUBLIC ABI (tests/test_epilogue_numerics.py without a GPU, tests/test_epilogue_numerics_gpu.py
on one).  No GPU call in here.

The probe: if one operand of a contraction is one-hot, the contraction passes the other operand through exactly
(1 * w + 0 * ... is exact in float32, whatever the order of the chain), so a propagation pass returns the epilogue function
of chosen bit patterns:

  * `RbmEngine.gibbs(Hd = onehot(H), Vd, B = H, 1)` / `OracleRBM.gibbs(onehot(H), 1)` with sample_v_states = False: the
    prop-down leaves the MEANS in V, V[j][i] = act(W[i][j] + vb[i]) - sigmoid for Bernoulli visible units, the linear form
    W[i][j] * sigma[i] + vb[i] for Gaussian ones.  (This is the public call both test files use; OracleRBM.gibbs returns
    (H, V).)
  * `RbmEngine.free_energy_rows(onehot(V), V)` of a V x 1 model with vb = hb = 0: F(row j) = -softplus(W[j]).

The point sets hold no inf and no NaN: 0 * inf inside the contraction is not something the specification defines."""
import numpy as np

LN2 = np.log(np.longdouble(2))
CLAMP = 80.0                      # bm_numerics.h: sigmoid and softplus clamp |x| here
SIGMOID_RTOL = 3e-7               # the bounds tests/test_oracle.py::test_sigmoid_spec_accuracy asserts on its grid
SIGMOID_ATOL_BEYOND = 1e-34


def neighbours(x, k=2):
    """float32(x) with its k float32 neighbours on each side, ascending"""
    c = np.float32(x)
    out, lo, hi = [c], c, c
    for _ in range(k):
        lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32)
        hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
        out = [lo] + out + [hi]
    return np.array(out, dtype=np.float32)


def tie_points(ns=range(116)):
    """the float32 nearest to (n + 1/2) ln 2 with two neighbours on each side, both signs: the ties of rintf(a log2 e),
    where the Cody-Waite reduction of exp_neg changes n"""
    pos = np.concatenate([neighbours(np.float32((np.longdouble(n) + np.longdouble(0.5)) * LN2)) for n in ns])
    return np.concatenate([pos, -pos])


def sigmoid_specials():
    s = [np.float32([0.0, -0.0, 1e-40, -1e-40, 1e-8, -1e-8])]
    for x in (17.32, 17.33, 17.34, 88.3762626647949, 88.72, 103.97, 1e10, 1.7e38):
        s.append(np.float32([x, -x]))                               # 17.33: the result starts to round to 1.0f
    s += [neighbours(80.0), -neighbours(80.0)]
    return np.concatenate(s)


def softplus_specials():
    extra = [f(neighbours(x)) for x in (20.0, 40.0, 79.0) for f in (np.positive, np.negative)]
    return np.concatenate([sigmoid_specials()] + extra)


def _fill(n, rng):
    """n values: half +- log-uniform magnitudes in [2^-30, 181], half uniform in [-90, 90]"""
    nl = n // 2
    mag = np.exp(rng.uniform(np.log(2.0 ** -30), np.log(181.0), nl))
    sign = np.where(rng.randint(0, 2, nl) == 1, 1.0, -1.0)
    return np.concatenate([mag * sign, rng.uniform(-90.0, 90.0, n - nl)]).astype(np.float32)


def point_set(n, specials, seed):
    """n float32 values: every entry of `specials`, the rest from _fill, in an order shuffled by RandomState(seed) (so that
    the special points do not all sit in the first tile)"""
    rng = np.random.RandomState(seed)
    specials = np.asarray(specials, dtype=np.float32)
    assert len(specials) <= n
    x = np.concatenate([specials, _fill(n - len(specials), rng)]).astype(np.float32)
    assert np.all(np.isfinite(x))
    return x[rng.permutation(n)]


def sigmoid_points():
    """[128][128] float32: sigmoid_specials(), the ties for n = 0 .. 115, the random rest"""
    return point_set(128 * 128, np.concatenate([sigmoid_specials(), tie_points()]), 0).reshape(128, 128)


def softplus_points():
    """[16][256] float32: the recipe of sigmoid_points() plus +-20, +-40, +-79 with their neighbours"""
    return point_set(16 * 256, np.concatenate([softplus_specials(), tie_points()]), 0).reshape(16, 256)


def bias_points(n=128, seed=1):
    """a second, small point set (a bias vector): the specials and every eighth tie (the centre point, both signs)"""
    return point_set(n, np.concatenate([sigmoid_specials(), tie_points(range(0, 116, 8))[2::5]]), seed)


def saturated_points():
    """[128][128] float32 with |x| in [20, 80] only: the special points inside that range, +- log-uniform and uniform
    magnitudes (part e: sampling where the sigmoid has rounded to 1.0f or is tiny and positive)"""
    sp = np.concatenate([softplus_specials(), tie_points()])
    sp = sp[(np.abs(sp) >= 20.0) & (np.abs(sp) <= 80.0)]
    n = 128 * 128 - len(sp)
    rng = np.random.RandomState(2)
    mag = np.concatenate([np.exp(rng.uniform(np.log(20.0), np.log(80.0), n // 2)), rng.uniform(20.0, 80.0, n - n // 2)])
    mag = np.clip(mag.astype(np.float32), np.float32(20.0), np.float32(80.0))
    x = np.concatenate([sp, mag * np.where(rng.randint(0, 2, n) == 1, 1.0, -1.0).astype(np.float32)]).astype(np.float32)
    return x[rng.permutation(len(x))].reshape(128, 128)


def onehot(n):
    return np.eye(n, dtype=np.float32)


def sigmoid64(x):
    """1 / (1 + exp(-x)) of the float32 / float64 values x, evaluated in long double without cancellation -> float64"""
    x = np.asarray(x).astype(np.longdouble)
    e = np.exp(-np.abs(x))
    return (np.where(x >= 0, 1.0, e) / (1.0 + e)).astype(np.float64)


def softplus64(x):
    """max(x, 0) + log1p(exp(-|x|)) in long double -> float64"""
    x = np.asarray(x).astype(np.longdouble)
    return (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))).astype(np.float64)


def closed_form_log_Z(vb, hb):
    """log Z of an RBM with W = 0: the units are independent, Z = prod (1 + e^b)"""
    return float(np.sum(softplus64(vb)) + np.sum(softplus64(hb)))


# ---- AIS at saturated biases (W = 0, base_bias = vb): every chain's value is closed_form_log_Z whatever it samples
AIS_VB = np.linspace(-8., 8., 16).astype(np.float32)
AIS_HB = {'saturated': np.linspace(-40., 40., 64).astype(np.float32),
          'sparse': np.random.RandomState(4).uniform(-12., -4., 64).astype(np.float32)}       # the sparse-unit regime


def dbm_zero_weight_params(V=12, nh=(8, 6), h1_bias=0.0):
    """float32 parameters of a V-h1-h2 DBM with zero weights and biases in +-20 on the layers AIS sums out analytically
    (v and h2: the softplus terms).  h1_bias = 0 (default): the biases of the sampled chain layer h1 are ZERO - with the
    uniform base of the DBM's AIS a non-zero h1 bias enters the log-weight through the sampled states (beta b.x), and the
    value would no longer be the same for every chain.  h1_bias = 20: h1 biases in +-20 as well (the estimate is then a
    random variable; log Z stays the closed form)."""
    P = {'vb': np.linspace(-20., 20., V).astype(np.float32),
         'hb': np.linspace(-h1_bias, h1_bias, nh[0]).astype(np.float32),
         'hb_1': np.linspace(20., -20., nh[1]).astype(np.float32),
         'W': np.zeros((V, nh[0]), dtype=np.float32), 'W_1': np.zeros((nh[0], nh[1]), dtype=np.float32)}
    return P


def ulp32(exact):
    """the float32 spacing at |exact| (float64 in, float64 out): the unit the softplus budget is counted in"""
    return np.spacing(np.abs(np.asarray(exact, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def check_sigmoid_bounds(x, s, what='sigmoid'):
    """the float64 bounds of the pinned sigmoid over the float32 points x -> (max relative error for |x| <= 80, max
    absolute error beyond); asserts them, the exact 0.5 at +-0 and the denormals, and monotonicity over the sorted points"""
    x = np.asarray(x, dtype=np.float32).ravel()
    s = np.asarray(s, dtype=np.float32).ravel()
    exact = sigmoid64(x)
    core = np.abs(x) <= CLAMP
    rel = np.abs(s[core].astype(np.float64) - exact[core]) / exact[core]
    beyond = np.abs(s[~core].astype(np.float64) - exact[~core])
    worst = int(np.argmax(rel))
    print('%s: max rel err %.3e (x = %r) over %d points with |x| <= 80, max abs err beyond %.3e'
          % (what, rel[worst], float(x[core][worst]), int(core.sum()), float(beyond.max()) if beyond.size else 0.0))
    assert rel.max() < SIGMOID_RTOL, (what, float(x[core][worst]), float(rel[worst]))
    assert beyond.size == 0 or beyond.max() < SIGMOID_ATOL_BEYOND, (what, float(beyond.max()))
    tiny = np.abs(x) < 1e-38
    assert tiny.sum() >= 4 and np.all(s[tiny] == np.float32(0.5)), (what, x[tiny], s[tiny])
    order = np.argsort(x, kind='stable')
    d = np.diff(s[order])
    assert np.all(d >= 0), '%s decreases between x = %r and %r' % (
        what, float(x[order][int(np.argmin(d))]), float(x[order][int(np.argmin(d)) + 1]))
    return float(rel.max()), float(beyond.max()) if beyond.size else 0.0


def orc_sigmoid_of(x):
    """orc_sigmoid elementwise (the C oracle's scalar entry point), same shape, float32"""
    from oracle import oracle as orc
    f = orc.lib().orc_sigmoid
    x = np.asarray(x, dtype=np.float32)
    return np.array([f(float(v)) for v in x.ravel()], dtype=np.float32).reshape(x.shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
