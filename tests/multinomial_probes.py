"""Logit sets, float64 references, derived bounds and exact count checks that probe the Multinomial layer (softmax +
categorical counts, one wave per row) at its edges THROUGH THE PUBLIC ABI (tests/test_multinomial_edges.py on the oracle
without a GPU, tests/test_multinomial_edges_gpu.py on the device).  No GPU call in here.

The probe.  The logits of a row must be known bit patterns:

  * W = 0: the prop-up gives 0 + hb exactly, so the logit vector goes into `hb` and every row of a call has the same logits;
    the rows differ only in their draws (draw d of row r reads uniform (row0 + r) * M + d).  Means come back through
    `transform(X, rows, 1)`, counts through `gibbs(H, V, rows, 1)`, which leaves the hidden states in H.  This is the
    construction both test files use.
  * a one-hot X with hb = 0 gives row r the logits W[r, :] in the FIRST prop-up only (h0).  No public call returns h0:
    `transform` returns the means after a Gibbs step, whose visible input is sigmoid(h0 W^T + vb) and not one-hot any more
    (tests/test_multinomial_edges.py::test_what_the_probes_return shows both facts on the oracle).  Distinct logits per row
    are therefore covered by the DBM case with real weights only.
  * the float64 ABI (bm_rbm64_*) has transform and no gibbs: the device's float64 means are probed, its float64 counts
    are not reachable (the oracle's are: OracleRBM64.work['hs']).

Families (all finite: the specification defines nothing for inf / NaN), per width I:
  a normal, std 3                      b all equal                  c uniform, spread 2.5 x the clamp (beyond it)
  d one unit at +30, the rest at -30 (hot unit first / last / middle)
  e two units tied at the maximum, the rest 1.125 x the clamp below
  f "absorbed": l[0] = 0, the rest so low that e[i] is below half an ulp of 1 (-17.5 in float32, -37.5 in float64), and
    the same reversed (small terms first: they are NOT absorbed)
  g ramps over [-20, 0], ascending and descending

The bound on the means (derived, not tuned).  For an entry with d = mx - l[i] <= clamp the relative error of mean / M
against the float64 softmax is at most ((I - 1) + d) * eps + const: (I - 1) eps for the sequential sum of positive terms, d eps
for the rounding of mx - l[i] itself, const for exp_neg, the division, the product and the conversion of M (1e-6 in float32,
where tests/test_oracle.py holds the sigmoid to 3e-7; 1e-15 in float64).  Beyond the clamp the bound is absolute:
mean / M <= e^-clamp (1.81e-35 in float32) and not below the exact value.

Counts (exact): whole, non-negative, every row sums to M; a unit with c[i] == c[i-1] (the prefix sums of the oracle,
orc_softmax_prefix) can never be drawn and has count 0; I = 1 gives M; family d at M <= 100 puts every draw on the hot unit
(the exact mass of the rest is (I - 1) e^-60 < 1e-22).

Chi-square: per row, the cells with expectation M p >= 5 plus one lumped rest cell if that reaches 5; chi2 and dof summed
over the rows of a case; z = (chi2 - dof) / sqrt(2 dof), |z| <= 4 wherever dof >= 10.  dof is a property of the case, not
of the code under test: a row with one cell (M = 1, family d, family f, a flat row wider than M / 5) has dof 0 whatever is
drawn, and widths 1 and 2 have at most 8 at 8 rows.  So "at most one case in ten below dof 10" is asserted over the cases
that CAN carry a test, fixed here before any run: families a, b and g at M >= 20000 and I >= 7, family b only while
M / I >= 5 (Tally.assert_statistical_leg); every other case with dof >= 10 is tested all the same."""
import ctypes as C

import numpy as np

WIDTHS = (1, 2, 7, 63, 64, 65, 1000, 4097, 8191, 8192)
WIDTHS64 = (1, 2, 63, 64, 65, 1000)                     # + the float64 limit the device reports
N_SAMPLES = (1, 100, 20000)
ROWS = 8
Z_CAP = 4.0
LD = np.longdouble


class Prec(object):
    def __init__(self, dtype, eps, clamp, const, low):
        self.dtype, self.eps, self.clamp, self.const, self.low = dtype, eps, clamp, const, low
        self.scale = clamp / 80.0
        self.beyond = float(np.exp(LD(-clamp)) * (1 + LD(3) * eps + LD(const)))   # e^-clamp / S, S >= 1: 1.81e-35 in float32
        self.name = np.dtype(dtype).name


F32 = Prec(np.float32, 2.0 ** -24, 80.0, 1e-6, -17.5)
F64 = Prec(np.float64, 2.0 ** -53, 700.0, 1e-15, -37.5)
assert F32.beyond <= 1.81e-35


def logit_sets(I, prec=F32):
    """[(name, [I] logits of prec.dtype)], identical vectors (small I) once"""
    rng = np.random.RandomState(1000 + I)
    s = prec.scale
    out = [('a_normal', rng.normal(0.0, 3.0, I)), ('b_equal', np.full(I, -3.75)),
           ('c_uniform', rng.uniform(-100.0 * s, 100.0 * s, I))]
    for nm, hot in (('first', 0), ('last', I - 1), ('middle', I // 2)):
        l = np.full(I, -30.0); l[hot] = 30.0
        out.append(('d_hot_' + nm, l))
    l = np.full(I, 2.5 - 90.0 * s); l[I // 3] = 2.5; l[I - 1] = 2.5
    out.append(('e_tied', l))
    l = np.full(I, prec.low); l[0] = 0.0
    out += [('f_absorbed', l), ('f_absorbed_reversed', l[::-1].copy())]
    out += [('g_ramp_up', np.linspace(-20.0, 0.0, I)), ('g_ramp_down', np.linspace(0.0, -20.0, I))]
    seen, uniq = set(), []
    for nm, l in out:
        l = np.ascontiguousarray(l, dtype=prec.dtype)
        assert l.shape == (I,) and np.all(np.isfinite(l))
        if l.tobytes() not in seen:
            seen.add(l.tobytes()); uniq.append((nm, l))
    return uniq


def hot_unit(name, I):
    return {'d_hot_first': 0, 'd_hot_last': I - 1, 'd_hot_middle': I // 2}.get(name)


def softmax64(l):
    """softmax of the float32 / float64 logits l in long double -> float64"""
    x = np.asarray(l).astype(LD)
    e = np.exp(x - x.max())
    return (e / e.sum()).astype(np.float64)


def prefix(l, prec=F32):
    """(e, c) of the oracle's softmax row: e[i] = exp_neg(min(mx - l[i], clamp)), c = its sequential prefix sums"""
    from oracle import oracle as orc
    l = np.ascontiguousarray(l, dtype=prec.dtype)
    ptr = np.ctypeslib.ndpointer(dtype=prec.dtype, flags='C_CONTIGUOUS')
    f = getattr(orc.lib(), 'orc_softmax_prefix' if prec is F32 else 'orc_softmax_prefix_d')
    f.argtypes, f.restype = [ptr, C.c_int, ptr, ptr], None
    e, c = np.zeros_like(l), np.zeros_like(l)
    f(l, len(l), e, c)
    return e, c


def undrawable(l, prec=F32):
    """mask of the units no draw can land on: t < c[i] and t >= c[i-1] has no solution when c[i] == c[i-1]"""
    _, c = prefix(l, prec)
    m = np.zeros(len(c), dtype=bool)
    m[1:] = c[1:] == c[:-1]
    return m


def absorbed_mass(l, prec=F32):
    """exact probability mass of the undrawable units; asserts the bound (I - 1) eps: an absorbed e[i] is below half an ulp of
    the running sum, so below eps S, and p[i] = e[i] / S"""
    mass = float(np.sum(softmax64(l).astype(LD)[undrawable(l, prec)]))
    assert mass <= (len(l) - 1) * prec.eps, (mass, len(l))
    return mass


def check_means(l, means, M, prec=F32, what=''):
    """means [rows][I] or [I] of rows that all have the logits l, against M * softmax64(l) -> the largest error / bound"""
    l = np.ascontiguousarray(l, dtype=prec.dtype)
    I = len(l)
    means = np.asarray(means)
    assert means.dtype == prec.dtype and means.shape[-1] == I, (means.dtype, means.shape)
    got = means.reshape(-1, I).astype(np.float64) / float(M)
    p = softmax64(l)
    d = (l.astype(LD).max() - l.astype(LD)).astype(np.float64)
    core = d <= prec.clamp
    bound = ((I - 1) + d[core]) * prec.eps + prec.const
    rel = np.abs(got[:, core] - p[core]) / p[core]
    ratio = float(np.max(rel / bound))
    worst = float(np.max(rel))
    beyond = got[:, ~core]
    print('%s %s I=%d M=%d: max rel err %.3e = %.3f of the bound over %d entries, %d beyond the clamp (max %.3e)'
          % (what, prec.name, I, M, worst, ratio, int(core.sum()), int((~core).sum()), float(beyond.max()) if beyond.size else 0.0))
    assert np.all(np.isfinite(got)), what
    assert ratio <= 1.0, (what, I, M, worst, ratio)
    if beyond.size:
        assert np.all(beyond <= prec.beyond), (what, float(beyond.max()))
        assert np.all(beyond >= p[~core]), (what, float(np.min(beyond - p[~core])))
    return ratio


def check_counts(l, counts, M, prec=F32, name='', what=''):
    """the exact properties of the counts [rows][I] of rows that all have the logits l"""
    I = len(l)
    c = np.asarray(counts).reshape(-1, I).astype(np.float64)
    assert np.all(c >= 0) and np.all(c == np.round(c)), (what, 'counts are not non-negative whole numbers')
    assert np.all(c.sum(axis=1) == M), (what, 'row sums', c.sum(axis=1), M)
    dead = undrawable(l, prec)
    assert np.all(c[:, dead] == 0), (what, 'a unit with c[i] == c[i-1] was drawn', int(dead.sum()))
    if I == 1:
        assert np.all(c == M), what
    hot = hot_unit(name, I)
    if hot is not None and M <= 100:
        assert (I - 1) * float(np.exp(LD(-60))) < 1e-22
        assert np.all(c[:, hot] == M), (what, 'a draw left the hot unit')


def chi_square(l, counts, M):
    """-> (z, dof) of the counts [rows][I] against M * softmax64(l); (0.0, 0) where no row has two cells"""
    I = len(l)
    c = np.asarray(counts).reshape(-1, I).astype(np.float64)
    ex = float(M) * softmax64(l)
    cells = ex >= 5.0
    rest_ex = float(M) - float(ex[cells].sum())
    rest = rest_ex >= 5.0
    ncell = int(cells.sum()) + int(rest)
    if ncell < 2:
        return 0.0, 0
    chi2 = float(np.sum((c[:, cells] - ex[cells]) ** 2 / ex[cells]))
    if rest:
        chi2 += float(np.sum((c[:, ~cells].sum(axis=1) - rest_ex) ** 2 / rest_ex))
    dof = c.shape[0] * (ncell - 1)
    return (chi2 - dof) / np.sqrt(2.0 * dof), dof


def carries_a_test(name, I, M):
    """the cases that can reach dof >= 10 at ROWS rows, decided from the families alone (module docstring)"""
    return M >= 20000 and I >= 7 and name[0] in 'abg' and (name[0] != 'b' or M / float(I) >= 5.0)


class Tally(object):
    """collects the chi-square of every case of a test and asserts the cap and that the statistical leg is not empty"""

    def __init__(self):
        self.rows = []

    def add(self, l, counts, M, prec, name, what):
        check_counts(l, counts, M, prec, name, what)
        z, dof = chi_square(l, counts, M)
        self.rows.append((what, name, len(l), M, z, dof))
        print('%s %s I=%d M=%d: chi-square z = %+.2f at dof %d' % (what, prec.name, len(l), M, z, dof))
        if dof >= 10:
            assert abs(z) <= Z_CAP, (what, name, len(l), M, z, dof)
        return z, dof

    def assert_statistical_leg(self):
        can = [r for r in self.rows if carries_a_test(r[1], r[2], r[3])]
        low = [r for r in can if r[5] < 10]
        tested = [r for r in self.rows if r[5] >= 10]
        print('chi-square: %d of %d cases tested (dof >= 10), max |z| %.2f; %d of the %d cases that can carry a test have dof < 10'
              % (len(tested), len(self.rows), max([abs(r[4]) for r in tested] or [0.0]), len(low), len(can)))
        assert len(low) * 10 <= len(can), low
        return tested


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bits(got, want, what):
    bad = bits(got) != bits(want)
    assert got.shape == want.shape and not bad.any(), '%s: %d / %d elements differ bitwise, first at %r: %r against %r' % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


# ---- the probe on the oracle twins (the device side of the same calls lives in tests/test_multinomial_edges_gpu.py)
V_PROBE = 3


def probe_x(rows, dtype=np.float32):
    """any visible input: with W = 0 it cannot reach the logits"""
    return ((np.arange(rows * V_PROBE).reshape(rows, V_PROBE) % 2) == 0).astype(dtype)


def twin_rbm(I, M, l, prec=F32, seed=7, row0=0, sample_h_states=True):
    from oracle import oracle as orc
    t = (orc.OracleRBM if prec is F32 else orc.OracleRBM64)(V_PROBE, I, h_unit=2, n_samples=M, sample_h_states=sample_h_states)
    t.p['hb'][...] = l
    t.set_seed(seed)
    t.row0 = int(row0)
    return t


def twin_means(t, rows=ROWS):
    """transform(X, 1): the means of the last prop-up"""
    return t.transform(probe_x(rows, t.p['hb'].dtype), 1)


def twin_counts(t, rows=ROWS):
    """float32: gibbs(H, 1) -> the hidden states; float64 (no gibbs entry): the hidden states of the same chain call"""
    if t.p['hb'].dtype == np.float32:
        return t.gibbs(np.zeros((rows, t.H), dtype=np.float32), 1)[0]
    t.chain(probe_x(rows, np.float64), 1)
    t.call += 1
    return t.work['hs'].copy()


def dbm_layers(widths, prec=F32):
    """a V_PROBE - widths stack with Multinomial layers first and last (Bernoulli between), zero weights and the logits of
    families c and a in the biases -> (h_units, n_samples, {name: value})"""
    L = len(widths)
    hu = [2 if i in (0, L - 1) else 0 for i in range(L)]
    ns = [(100 if i == 0 else 7) if hu[i] else 0 for i in range(L)]
    P = {}
    for i, w in enumerate(widths):
        fam = dict(logit_sets(w, prec))
        P['hb' + ('' if i == 0 else '_%d' % i)] = fam['c_uniform'] if i == 0 else fam['a_normal']
    return hu, ns, P
