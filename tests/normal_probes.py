"""Float64 references, edge-word search and placement for the Normal sampler (`box_muller` of csrc/bm_rng.h; oracle:
`box_muller_pair` of oracle/bm_oracle.c).  tests/test_normal_sampler.py uses them without a GPU,
tests/test_normal_sampler_gpu.py on one.  No GPU call in here.

A Normal draw is a function of ONE PAIR of Philox words: elements 4b + 2p and 4b + 2p + 1 of a stream take the words
2p and 2p + 1 of block b; the first word gives u1 (radius), the second u2 (angle); the even element is sin, the odd one
cos.  Every branch of the definition is decided by the 23-bit mantissa of one of the two words (`TARGETS`), and a word with
a given mantissa has probability 2^-23 per pair - so the tests SEARCH the stream for the first pair that holds each edge
word (`find_words`) and place a small tensor around it with a row offset (`rows_for`).

The probe on the device: an RbmEngine with Gaussian visible units, sample_v_states = True and W = 0.  The prop-down of
`gibbs(Hd, Vd, B, n_steps)` then leaves V[j][i] = n * sigma[i] + vb[i] with n the draw of site 3 + 16 (n_steps - 1),
call 0 (after `seed`), flat index (row0 + j) * V + i."""
import numpy as np

M23 = 0x7fffff
EPS = np.float32(1.0e-7)                        # box_muller: u1 = max(u, 1e-7f)
R_MAX = 5.678                                   # sqrt(-2 ln 1e-7f) = 5.6777, rounded up
# A draw against the real-number Box-Muller of the same words, derived: the angle error of (sin, cos) scaled by the
# largest radius, the error of the radius (one float32 ulp at r_max, |sin|, |cos| <= 1), the half ulp of the product
# (|n| < 8: ulp 2^-21).  The bounds of the three terms are what test_exhaustive_sweep asserts.
LOG_RTOL = 2.0 ** -22
SINCOS_ATOL = 2.0 ** -23
R_ATOL = 2.0 ** -21
DRAW_ATOL = R_MAX * SINCOS_ATOL + R_ATOL + 2.0 ** -22           # 1.39e-6

SITE_V = 3                                      # the visible draws of RbmEngine.gibbs: site 3 + 16 t
SITE_DBM_V = 12                                 # the visible draws of a DBM sweep: site 12 + 16 t
SEED = 5

# (which word of the pair, mantissa): what it hits
FIRST = (0, 1, 2, 0x7fffff, 0x7ffffe,           # the clamp, the first unclamped values, the smallest r
         0x400000, 0x3fffff, 0x200000,          # binade boundaries of u1
         0x5a8279, 0x5a827a, 0x5a827b)          # the m > sqrt 2 split of the log in the top binade
SECOND = (0, 1, 0x7fffff,                       # angle 0 and the wrap
          0x200000, 0x400000, 0x600000,         # quadrant boundaries
          0x100000, 0x100001, 0x300000, 0x300001, 0x500000, 0x500001, 0x700000, 0x700001,   # f = 0.5, the first folded value
          0x0fffff, 0x1fffff)                   # just below a fold, just below a quadrant boundary
TARGETS = tuple((0, m) for m in FIRST) + tuple((1, m) for m in SECOND)
CLAMP, ANGLE0, FOLD = (0, 0), (1, 0), (1, 0x100000)       # FOLD: f = 0.5 exactly, where `f > 0.5f` and `f >= 0.5f` give different bits


def unit(x):
    """TF Uint32ToFloat of the words x: (x & 0x7fffff) / 2^23, exact in float32"""
    return ((np.asarray(x, dtype=np.uint32) & np.uint32(M23)).astype(np.float64) / 2.0 ** 23).astype(np.float32)


def box_muller64(x0, x1):
    """the real-number Box-Muller of the word pairs (x0, x1), evaluated in long double -> dict of float64 arrays:
    n0, n1 (the two draws), log64 = ln u1, r64 = sqrt(-2 ln u1), sin64, cos64 = (sin, cos)(2 pi u2);
    u = (x & 0x7fffff) / 2^23 exactly, u1 = max(u, float32(1e-7))"""
    ld = np.longdouble
    u1 = np.maximum(unit(x0), EPS).astype(ld)
    u2 = unit(x1).astype(ld)
    lg = np.log(u1)
    r = np.sqrt(ld(-2) * lg)
    a = (ld(8) * np.arctan(ld(1))) * u2            # 2 pi u2, pi in long double (no reduction of our own: absolute error ~1e-18)
    sn, cs = np.sin(a), np.cos(a)
    f8 = np.float64
    return dict(n0=(sn * r).astype(f8), n1=(cs * r).astype(f8), log64=lg.astype(f8), r64=r.astype(f8),
                sin64=sn.astype(f8), cos64=cs.astype(f8))


def normal64(seed, site, call, n, idx0=0):
    """float64 reference of orc.normal(seed, site, call, n, idx0): box_muller64 of the stream's own words"""
    from oracle import oracle as orc
    b0, b1 = idx0 // 4, (idx0 + n + 3) // 4
    w = orc.philox_words(seed, site, call, b0, b1 - b0).reshape(-1, 2)
    ref = box_muller64(w[:, 0], w[:, 1])
    return np.stack([ref['n0'], ref['n1']], axis=1).reshape(-1)[idx0 - 4 * b0: idx0 - 4 * b0 + n]


_found = {}


def find_words(seed, site, call, targets=TARGETS, limit=2 ** 26, chunk=2 ** 20):
    """{(word, mantissa): flat element index of the first pair (its even element) whose first (word = 0) or second
    (word = 1) Philox word has that 23-bit mantissa}, scanning the elements below `limit` in chunks of `chunk` blocks.
    EVERY target must be found (an AssertionError otherwise).  Cached per (seed, site, call, targets)."""
    from oracle import oracle as orc
    key = (seed, site, call, tuple(targets), limit)
    if key in _found:
        return dict(_found[key])
    want = [np.array(sorted(m for w, m in targets if w == k), dtype=np.uint32) for k in (0, 1)]
    out = {}
    for b0 in range(0, limit // 4, chunk):
        nb = min(chunk, limit // 4 - b0)
        mant = orc.philox_words(seed, site, call, b0, nb).reshape(-1, 2) & np.uint32(M23)        # rows = pairs
        for k in (0, 1):
            hit = np.flatnonzero(np.isin(mant[:, k], want[k]))
            for p in hit:
                out.setdefault((k, int(mant[p, k])), 4 * b0 + 2 * int(p))
        if len(out) == len(targets):
            break
    missing = [t for t in targets if t not in out]
    assert not missing, 'no pair below element %d holds the words %r' % (limit, missing)
    _found[key] = dict(out)
    return out


def rows_for(idx, V):
    """(row0, B) of a [B][V] tensor that holds the pair at flat element idx (and, V odd, a pair that straddles a row
    end next to it): the row of idx is the middle one of three"""
    return idx // V - 1, 3


def pair_words(seed, site, call, idx):
    """the two Philox words behind elements idx, idx + 1 (idx even)"""
    from oracle import oracle as orc
    w = orc.philox_words(seed, site, call, idx // 4, 1)[0]
    return int(w[idx % 4]), int(w[idx % 4 + 1])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), '%s: %d / %d elements differ bitwise, first at %r: %r against %r' % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def assert_draws(got, seed, site, n_elems, idx0, what):
    """the three assertions every device (or twin) tensor of raw draws meets: equal to orc.normal at the same stream
    position by value (n * 1 + 0 turns a -0 into +0), and within DRAW_ATOL of the float64 Box-Muller of the same words
    -> the largest error against float64"""
    from oracle import oracle as orc
    got = np.asarray(got, dtype=np.float32).reshape(-1)
    assert got.size == n_elems
    want = orc.normal(seed, site, 0, n_elems, idx0=idx0)
    bad = got != want
    assert not bad.any(), '%s: %d / %d elements differ from orc.normal, first at %d: %r against %r' % (
        what, int(bad.sum()), bad.size, int(np.flatnonzero(bad)[0]), got[bad][0], want[bad][0])
    err = np.abs(got.astype(np.float64) - normal64(seed, site, 0, n_elems, idx0=idx0))
    worst = int(np.argmax(err))
    assert err[worst] < DRAW_ATOL, '%s: %.3e from the float64 Box-Muller at element %d (bound %.3e)' % (
        what, err[worst], worst, DRAW_ATOL)
    return float(err[worst])


def check_clamp_pair(Vs, seed, site, idx, row0):
    """the pair at flat element idx of the [B][V] draws Vs (row offset row0) is the clamp word's: r(1e-7f) times the
    (sin, cos) of its angle word, predicted from the two component functions - the largest |n| a draw can have is in the
    tensor, and nothing in the tensor is larger"""
    from oracle import oracle as orc
    x0, x1 = pair_words(seed, site, 0, idx)
    assert x0 & M23 == 0
    r = np.sqrt(np.float32(-2.0) * orc.pin_log_unit(np.float32([1e-7])))[0]
    sn, cs = orc.pin_sincos_2pi(unit([x1]))
    want = np.float32([sn[0] * r, cs[0] * r])
    V = Vs.shape[1]
    got = np.asarray(Vs).reshape(-1)[idx - row0 * V: idx - row0 * V + 2]
    assert np.array_equal(got, want), (got, want)
    assert np.abs(Vs).max() == np.abs(want).max() and 5.6777 * 0.7071 < np.abs(want).max() < R_MAX


def twin_gibbs(V, B, row0, n_steps=1, seed=SEED, H=16, v_unit=1, sigma=None, vb=None, Hs=None):
    """the last V of OracleRBM.gibbs on the probe model (W = 0) at row offset row0"""
    from oracle import oracle as orc
    t = orc.OracleRBM(V, H, v_unit=v_unit, sample_v_states=True)
    if sigma is not None:
        t.p['sigma'][...] = sigma
    if vb is not None:
        t.p['vb'][...] = vb
    t.set_seed(seed)
    t.row0 = int(row0)
    return t.gibbs(np.zeros((B, H), dtype=np.float32) if Hs is None else Hs, n_steps)[1]


# ---- the cases both test files build the same way
BULK = ((1024, 2048), (1024, 2047))             # one aligned launch, one whose rows start at every word of a block
BULK_ROW0 = 977                                  # an odd offset: the bulk is not block-aligned by accident
CARRY = ((12, 1431655765 - 1), (16, 2 ** 30 - 1))
# (V, row0): row0 + 1 starts at flat element 2^34 - 4 (V = 12: 3 * 1431655765 = 2^32 - 1, so the row's first eight elements
# are the blocks 2^32 - 1 and 2^32 - the low counter word carries into the high one) and at 2^34 exactly (V = 16)
CHAIN_SHAPE = (256, 192, 512)                    # V, H, B of the chained probe: 8 row blocks of 64, K >= 192 both ways
CHAIN_STEPS = 3                                  # six passes: the default rule chains them (csrc/bm_chain.h)
CHAIN_TARGETS = (CLAMP, (1, 0x100000))
DBM_HIDDEN = (16, 18)                            # x-major W (K % 4 == 0: geometries with MI = 1) and k-major W^T (MI = 2 too)


def two_roundings_case(V=128, B=64, row0=3):
    """(sigma, vb, n, want, fused): want = float32(float32(n * sigma) + vb), fused = the same through one rounding"""
    from oracle import oracle as orc
    from tests import numerics_probes as npb
    sigma = np.linspace(0.5, 1.5, V).astype(np.float32)
    vb = npb.bias_points(V)
    n = orc.normal(SEED, SITE_V, 0, B * V, idx0=row0 * V).reshape(B, V)
    want = ((n * sigma[None, :]).astype(np.float32) + vb[None, :]).astype(np.float32)
    fused = (n.astype(np.float64) * sigma[None, :].astype(np.float64) + vb[None, :].astype(np.float64)).astype(np.float32)
    return sigma, vb, n, want, fused


def dbm_case(V):
    """(sigma, vb) of the DBM probe: a non-unit sigma, biases of both signs"""
    return np.linspace(0.5, 1.5, V).astype(np.float32), np.linspace(-1.0, 1.0, V).astype(np.float32)


def dbm_twin(V, H, particle0, seed=SEED):
    """OracleDBM of the probe (zero weights, M = N = 3) after sample_v(2): its v_new holds the SAMPLED visible layer of
    sweep 0 (site 12) - sample_v itself returns the means of its last mean sweep, here vb"""
    from oracle import oracle as orc
    t = orc.OracleDBM(V, [H], v_unit=1, n_particles=3, batch_size=3)
    sigma, vb = dbm_case(V)
    t.p['sigma'][...] = sigma
    t.p['vb'][...] = vb
    t.set_seed(seed)
    t.prow0 = int(particle0)
    v = t.sample_v(2)
    return t, v


def check_dbm_draws(v_new, V, particle0, what, seed=SEED):
    """v_new [3][V] of the DBM probe against float64: box_muller64 * sigma + vb within DRAW_ATOL * max(sigma) plus one
    float32 ulp of the result (the rounding of the product and of the sum)"""
    sigma, vb = dbm_case(V)
    ref = normal64(seed, SITE_DBM_V, 0, 3 * V, idx0=particle0 * V).reshape(3, V) * sigma[None, :].astype(np.float64) + vb[None, :]
    err = np.abs(np.asarray(v_new, dtype=np.float64) - ref)
    bound = DRAW_ATOL * float(sigma.max()) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.all(err < bound), '%s: %.3e from float64 at %r (bound %.3e)' % (
        what, err.max(), tuple(np.argwhere(err >= bound)[0]), float(bound[err >= bound][0]))
    return float((err / bound).max())
