"""Point sets, structured weights, a NumPy twin of `split3` (csrc/bm_bf3.h) and float64 references that probe the fast-binary
contraction - three bf16 planes on the bf16 matrix cores - THROUGH THE PUBLIC ABI (tests/test_fast_binary_exact.py without a
GPU, tests/test_fast_binary_exact_gpu.py on one).  No GPU call in here.

The observation route: a one-layer stack `DbmEngine(V, [n], sample_v_states=False)` with `set_fast_binary(True,
everywhere=True)`; one particle sweep (k = 1) first samples h = sample(v . W + hb) on the fp32 path (the particles a call
starts from have no bf16 shadow) and then computes v = act(W h + vb) from the planes W3[0] and the shadow of that h - the strip
kernel act_bf3_kernel.  `get('v')` / `get('h')` return that v and exactly the h it was computed from: with Gaussian visibles,
sigma = 1 and vb = 0, v is the fp32 accumulator itself; with Bernoulli visibles v = sigmoid_hw(acc + vb).

The sweep is run through `DbmEngine.metrics(X, 1)`: the same mean-field + particle sweeps as `train_step`, without the parameter
update.  (A `train_step` with lr = 0 does NOT leave W unchanged: the reference's max-norm step rescales every column as
(W * min(norm, max_norm)) / max(norm, 1e-8) whatever max_norm is - two roundings with max_norm = inf, and NaN where the column
norm overflows, as it does for the 2^100 probe weights; tests/test_fast_binary_exact.py shows it on the oracle.)

hb = +40 on chosen units and -40 elsewhere with the particles v = 0 pins h (sigmoid(40) rounds to 1.0f, sigmoid(-40) is 4e-18);
the references are nevertheless computed from the h READ BACK."""
import numpy as np

from tests import numerics_probes as npb

U = 2.0 ** -24                       # unit round-off of float32

# ---- the tolerance of the float64 comparisons: |v - ref64| <= C (m + 2) 2^-24 S, m active units in the row, S = sum |w| h.
# C = 1: first-order bound for correctly rounded fp32 additions in any order; C = 2 covers truncating additions.  The accumulation
# inside v_mfma_f32_16x16x32_bf16 is not documented: C_MEASURED is max |err| / ((m + 2) 2^-24 S) over every pinned-sparse and
# dense case on an MI355X (printed by the tests), C twice that, rounded up.  C > 4 would not be explained by
# addition rounding: a finding, not a tolerance to widen.
C_MEASURED = 0.1450                  # dense 5 x 7 x 3; pinned-sparse: 0.1148; the same figures in every geometry
C = 1
assert C <= 4

# ---- sigmoid_hw: relative error <= (|t| + 2 A) 2^-24.  |t| 2^-24: the rounded product t * log2(e) in front of v_exp_f32;
# A 2^-24: v_exp_f32, the add, v_rcp_f32 - measured on an MI355X as max (rel err / 2^-24 - |t|) over sigmoid_hw_points(): 8.196
# at t = -45 (it also absorbs the representation error of float32(log2 e), 0.22 |t| 2^-24), 1.797 over the points with |t| <= 1
A_MEASURED = 8.196
T_ONE = 17.33                        # from here on the result is exactly 1.0f
T_TINY = -87.0                       # below: absolute tolerance 2^-126 (a flush to zero is acceptable)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------ the split
def split3_np(w):
    """split3() of csrc/bm_bf3.h on float32 arrays -> (hi, mid, lo) as float32 values whose low 16 bits are zero: truncate to
    the top 16 bits, subtract (exact), twice; the last remainder is truncated as well (it has at most 8 significant bits for
    every w whose last bit is a normal number)"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    top = np.uint32(0xffff0000)
    hi = from_bits(bits(w) & top)
    r1 = (w - hi).astype(np.float32)
    mid = from_bits(bits(r1) & top)
    r2 = (r1 - mid).astype(np.float32)
    lo = from_bits(bits(r2) & top)
    return hi, mid, lo


def is_bf16(x):
    """at most 8 significant bits and float32's exponent range: the low 16 bits of the float32 pattern are zero"""
    return (bits(x) & np.uint32(0xffff)) == 0


# ------------------------------------------------------------------ point sets
E_MIN, E_MAX = -100, 100             # exponents of the pass-through points (denormal and near-denormal bf16 operands: not
                                     # established for the matrix cores anywhere in this project, DESIGN.md 3.9 - out of scope)


def in_range(x):
    """+0 and every float32 with 2^E_MIN <= |x| < 2^(E_MAX + 1).  (-0 is left out: 0 + (-0) * 1 = +0 in any arithmetic.)"""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x.astype(np.float64))
    return ((a >= 2.0 ** E_MIN) & (a < 2.0 ** (E_MAX + 1))) | (bits(x) == 0)


def low_bit_patterns():
    """float32 over both signs, exponents 2^-100 .. 2^100 in steps of 10 and ALL patterns of the low and of the middle
    significand byte (= the lo and the mid plane), each against a zero, a full and a varying other byte; the top 7 bits vary"""
    rng = np.random.RandomState(7)
    byte = np.arange(256, dtype=np.uint32)
    lows, mids = [], []
    for other in (np.zeros(256, np.uint32), np.full(256, 0xff, np.uint32), rng.randint(0, 256, 256).astype(np.uint32)):
        lows += [byte, other]
        mids += [other, byte]
    low, mid = np.concatenate(lows), np.concatenate(mids)
    n = len(low)
    top7 = rng.randint(0, 128, n).astype(np.uint32)
    top7[::5] = 0
    top7[1::5] = 0x7f
    exps = np.arange(E_MIN, E_MAX + 1, 10)
    out = []
    for sign in (0, 1):
        e = exps[(np.arange(n) + sign * 7) % len(exps)].astype(np.int64) + 127
        out.append(from_bits((np.uint32(sign) << 31) | (e.astype(np.uint32) << 23) | (top7 << 16) | (mid << 8) | low))
    x = np.concatenate(out)
    return x[rng.permutation(len(x))]


def pass_through_points():
    """1-D float32: +0, powers of two at both ends of the range, low_bit_patterns() and every point of
    numerics_probes.sigmoid_points() that is in range"""
    sp = npb.sigmoid_points().ravel()
    ends = np.float32([0.0, 2.0 ** E_MIN, -2.0 ** E_MIN, 2.0 ** E_MAX, -2.0 ** E_MAX])
    top = from_bits(np.uint32([0x7fffff | ((E_MAX + 127) << 23), 0x80000000 | 0x7fffff | ((E_MAX + 127) << 23)]))
    x = np.concatenate([ends, top, low_bit_patterns(), sp[in_range(sp)]]).astype(np.float32)
    assert np.all(in_range(x))
    return x


def chunks(x, size):
    """x in rows of `size` (the last one filled up from the front)"""
    n = -(-len(x) // size) * size
    return np.resize(x, n).reshape(-1, size)


PASS_SHAPES = [(100, 72, 17), (100, 70, 17)]        # nk % 8 == 0: vector build of split3_body; 70: scalar build, tail zeroing


def pass_k0(n):
    return [0, 7, 8, 63, 64, n - 1]


def filler(V, n, seed):
    """non-zero weights for the columns a pinned h multiplies by zero: a wrong column or row would show"""
    return (np.random.RandomState(seed).standard_normal((V, n)) * 0.1 + 3.0).astype(np.float32)


def pinned_hb(n, active):
    hb = np.full(n, -40.0, dtype=np.float32)
    hb[list(active)] = 40.0
    return hb


# ------------------------------------------------------------------ structured weights, pinned-sparse cases
def structured_weights(V, n, scale, seed):
    """positive float32 in [0.5, 1) times the power of two `scale`: low significand byte 0xFF, middle byte in 0x80 .. 0xBF,
    top 7 bits random.  split3() cuts by SIGNIFICANT bits, not by bytes: with bit 15 set the mid plane is exactly the middle
    byte, so by truncation every lo plane entry is positive and maximal (255 units of the last place) and every mid entry
    positive: a lost or shifted plane is a coherent error, the same sign in every term.  (With bit 15 clear the mid plane would
    reach into the low byte and leave a smaller lo.)"""
    rng = np.random.RandomState(seed)
    top7 = rng.randint(0, 128, (V, n)).astype(np.uint32)
    mid = rng.randint(0x80, 0xc0, (V, n)).astype(np.uint32)
    w = from_bits((np.uint32(126) << 23) | (top7 << 16) | (mid << 8) | np.uint32(0xff))
    assert np.all((w >= 0.5) & (w < 1.0))
    m, e = np.frexp(scale)
    assert m == 0.5
    return (w * np.float32(scale)).astype(np.float32)


SPARSE_REQUIRED = (0, 63, 64, 127, 255, 256)        # and n - 1


def sparse_active(n):
    """12 active units (at most 16 allowed): chunk edges of the 64-k ring, the last unit, a few inside"""
    a = sorted(set(SPARSE_REQUIRED + (n - 1, 1, 31, 128, 191, 200)))
    assert len(a) == 12 and a[-1] == n - 1
    return a


# (V, n, M, scale): n = 264 / 521 are 5 / 9 chunks of 64 k - the 4-slot ring wraps
SPARSE_CASES = [(V, n, M, 2.0 ** -4 if n == 264 else 8.0) for n in (264, 521) for V in (33, 128) for M in (1, 65)]


def sparse_weights(V, n, scale):
    return structured_weights(V, n, scale, seed=1000 + V + n)


def pinned_h(n, active, M):
    h = np.zeros((M, n), dtype=np.float32)
    h[:, list(active)] = 1.0
    return h


# ------------------------------------------------------------------ references
def ref64(W, h):
    """v[r][i] = sum_k W[i][k] h[r][k] in float64 (n <= 521 terms: 2^-53 n relative, nothing next to 2^-24)"""
    return h.astype(np.float64) @ W.astype(np.float64).T


def bound(W, h, c=None):
    """C (m + 2) 2^-24 S per element, m = active units of the row, S = sum_k |w_ik| h_rk"""
    m = np.count_nonzero(h, axis=1).astype(np.float64)
    S = np.abs(h.astype(np.float64)) @ np.abs(W.astype(np.float64)).T
    return (C if c is None else c) * (m[:, None] + 2.0) * U * S


def err_ratio(v, W, h):
    """max |v - ref64| / ((m + 2) 2^-24 S): what C is measured as (0 where S == 0 and the value is exact)"""
    err = np.abs(v.astype(np.float64) - ref64(W, h))
    b = bound(W, h, 1.0)
    assert np.all(err[b == 0] == 0)
    return float(np.max(err[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0


def fault_signatures(W, h):
    """|v_fault - v| in float64 for three plane faults -> dict of [M][V] arrays:
      lo_dropped / mid_dropped: the plane contributes nothing;
      swapped: the low and the middle significand byte change places (lo * 2^8 + mid * 2^-8: each plane at the other's
               weight.  Feeding the two planes to the matrix cores in the other ORDER is no fault: the sum commutes)."""
    hi, mid, lo = [p.astype(np.float64) for p in split3_np(W)]
    h64 = h.astype(np.float64)
    good = h64 @ (hi + mid + lo).T
    return {'lo_dropped': np.abs(h64 @ (hi + mid).T - good),
            'mid_dropped': np.abs(h64 @ (hi + lo).T - good),
            'swapped': np.abs(h64 @ (hi + lo * 256.0 + mid / 256.0).T - good)}


# ------------------------------------------------------------------ dense cases
# (V, n, M); the last one is the strip case: on 256 CUs 80 tile columns over 32 strips in geometry 4 and 40 over 32 in
# geometries 2 and 8 - uneven multi-tile strips, the next tile prefetched under the epilogue - in every geometry
DENSE_CASES = [(1, 1, 1), (5, 7, 3), (33, 65, 17), (64, 64, 64), (100, 200, 37), (128, 264, 65), (512, 136, 2560)]
DENSE_DISTINCT = (128, 264, 65)      # here the fast v must also differ from the default path's bits somewhere


def dense_inputs(V, n, M):
    """(W, hb, v0): normal weights with std 0.1, small biases, normal starting particles - h is sampled freely"""
    rng = np.random.RandomState(31 * V + 7 * n + M)
    W = (rng.standard_normal((V, n)) * 0.1).astype(np.float32)
    hb = (rng.uniform(-0.2, 0.2, n)).astype(np.float32)
    v0 = rng.standard_normal((M, V)).astype(np.float32)
    return W, hb, v0


# ------------------------------------------------------------------ sigmoid_hw
def sigmoid_hw_points():
    """1-D float32: numerics_probes.bias_points() and grids over [-100, 100] and [-1, 1]"""
    return np.concatenate([npb.bias_points(), np.linspace(-100.0, 100.0, 2001), np.linspace(-1.0, 1.0, 513),
                           np.float32([T_ONE, T_TINY, -87.3, -87.33, -87.34, -88.0])]).astype(np.float32)


def sigmoid_hw_excess(t, got):
    """per point with t > T_TINY: rel err / 2^-24 - |t| against the float64 sigmoid of the float32 argument (what A bounds)"""
    t = np.asarray(t, dtype=np.float32)
    core = t > np.float32(T_TINY)
    exact = npb.sigmoid64(t[core])
    rel = np.abs(got[core].astype(np.float64) - exact) / exact
    return rel / U - np.abs(t[core].astype(np.float64))


def check_sigmoid_hw(t, got, what):
    """the bounds of sigmoid_hw over the float32 arguments t -> the measured A of these points"""
    t = np.asarray(t, dtype=np.float32).ravel()
    got = np.asarray(got, dtype=np.float32).ravel()
    assert not np.any(np.isnan(got)), what
    assert np.all((got >= 0.0) & (got <= 1.0)), what
    assert np.all(got[t >= np.float32(T_ONE)] == np.float32(1.0)), (what, got[t >= np.float32(T_ONE)].min())
    tiny = t <= np.float32(T_TINY)
    assert tiny.sum() >= 4
    abs_err = np.abs(got[tiny].astype(np.float64) - npb.sigmoid64(t[tiny]))
    ex = sigmoid_hw_excess(t, got)
    tc = t[~tiny]
    worst = int(np.argmax(ex))
    unit = np.abs(tc) <= 1.0
    print('%s: A = max(rel err / 2^-24 - |t|) = %.3f at t = %r over %d points with t > %g (%.3f over the %d with |t| <= 1); '
          'max abs err %.3e over the %d points below'
          % (what, ex[worst], float(tc[worst]), len(tc), T_TINY, float(ex[unit].max()), int(unit.sum()), float(abs_err.max()),
             int(tiny.sum())))
    assert abs_err.max() <= 2.0 ** -126, (what, float(abs_err.max()))
    assert ex.max() <= 2.0 * A_MEASURED, '%s: rel err %.3f x 2^-24 beyond |t| x 2^-24 at t = %r (allowed: %.3f)' % (
        what, ex[worst], float(tc[worst]), 2.0 * A_MEASURED)
    return float(max(ex.max(), 0.0))
