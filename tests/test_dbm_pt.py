"""Parallel tempering of a DBM, checked on the CPU twin alone (tests/dbm_pt_twin.py: the tempered sweep as
loops of the oracle's two-segment activation stage, the swap step in NumPy float64).  The twin is the reference of the GPU tests
(test_dbm_pt_gpu.py), so it is itself checked here: against exact enumeration of a 5-4-3 DBM (the transition leaves the target
where it is, and mixes between modes a single-temperature sweep does not leave), against the plain sweep of tests/clamp_twin.py
at one temperature, and against the RBM's twin at one hidden layer."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import clamp_twin
from tests import dbm_pt_twin as T
from tests import pt_twin

SEED = 20241018
NV, N1, N2 = 5, 4, 3


def _exact_rows(p, betas, M, site):
    """([M R][V], [M R][n2]): row c R + r drawn exactly from p_{beta_r}(v, h2) (inverse CDF over the 2^(V + n2) states, one
    uniform per row; h1 is the first thing a step draws)"""
    R = len(betas)
    u = orc.uniform(SEED, site, 0, M * R).reshape(M, R).astype(np.float64)
    v, h2 = np.zeros((M, R, NV), np.float32), np.zeros((M, R, N2), np.float32)
    for r, b in enumerate(betas):
        vs, h2s, P = T.exact_tempered_joint(p['W'], p['vb'], p['hb'], float(b))
        code = np.minimum(np.searchsorted(np.cumsum(P.ravel()), u[:, r], side='right'), P.size - 1)
        v[:, r], h2[:, r] = vs[code // P.shape[1]], h2s[code % P.shape[1]]
    return v.reshape(M * R, NV), h2.reshape(M * R, N2)


def test_transition_leaves_the_target_invariant():
    """Detailed balance, by a LARGE-SAMPLE ESTIMATE: 5-4-3 DBM (2^12 states, enumerated in float64) with N(0, 1) weights,
    R = 3, betas (0.3, 0.6, 1).  20 000 independent chains start in the exact product distribution prod_r p_{beta_r}(v, h2);
    four steps of (h1, swap, h2, v) follow - both swap parities twice.  The beta = 1 rows must still be distributed as the exact
    p_1(v): every one of the 32 visible patterns' frequencies within 5 binomial standard deviations, 5 sqrt(p (1 - p) / M),
    + 2 / M for the patterns whose expected count is of order one (the rarest has 4.4: there the binomial is Poisson-like and
    5 sigma alone is not a 5 sigma bound) - the convention of tests/test_pt.py.  The start has the same bound, and so have the
    hot marginals after the steps."""
    p = dict(W=[orc.normal(SEED, 1, 0, NV * N1).reshape(NV, N1), orc.normal(SEED, 2, 0, N1 * N2).reshape(N1, N2)],
             vb=orc.normal(SEED, 3, 0, NV) * np.float32(0.5),
             hb=[orc.normal(SEED, 4, 0, N1) * np.float32(0.5), orc.normal(SEED, 5, 0, N2) * np.float32(0.5)])
    betas = np.array([0.3, 0.6, 1.0], np.float32)
    M = 20000
    v0, h20 = _exact_rows(p, betas, M, 6)
    e = T.Ensemble(p, M, betas, seed=SEED, V0_rows=v0, H2_rows=h20)
    weights = (1 << np.arange(NV))

    def exact_v(b):
        return T.exact_tempered_joint(p['W'], p['vb'], p['hb'], float(b))[2].sum(axis=1)

    def freq(v):
        return np.bincount(v.astype(np.int64).dot(weights), minlength=1 << NV) / float(M)
    exact = exact_v(1.0)
    bound = 5.0 * np.sqrt(exact * (1.0 - exact) / M) + 2.0 / M
    start = freq(e.read()[0])
    assert np.all(np.abs(start - exact) <= bound)
    e.sweep(4)
    assert np.all(e.cnt[0] == [2 * M, 2 * M]) and np.all(e.cnt[1] > 0) and np.all(e.cnt[1] < e.cnt[0])
    assert np.array_equal(np.sort(e.idx.reshape(M, 3), axis=1), np.tile(np.arange(3), (M, 1)))     # a permutation per chain
    assert np.array_equal(e.mult, betas[e.idx])
    end = freq(e.read()[0])
    print('max |freq - exact| / bound: start %.3f, after 4 steps %.3f' % (np.max(np.abs(start - exact) / bound),
                                                                          np.max(np.abs(end - exact) / bound)))
    assert np.all(np.abs(end - exact) <= bound)
    for r, b in enumerate(betas[:-1]):
        ex = exact_v(b)
        rows = np.arange(M) * 3 + np.argmax(e.idx.reshape(M, 3) == r, axis=1)
        assert np.all(np.abs(freq(e.v[rows]) - ex) <= 5.0 * np.sqrt(ex * (1.0 - ex) / M) + 2.0 / M)


MV, M1, M2 = 6, 4, 3


def _two_mode_model():
    """all weights w = 3 in both layers, every bias minus half the weight that reaches the unit (vb = -w n1 / 2 + 0.15,
    b1 = -w (V + n2) / 2, b2 = -w n1 / 2): in +-1 spins a ferromagnet, the modes are all units 0 and all units 1, the tilt
    0.15 on vb makes the second one the heavier (so the exact answer is not 1/2 by symmetry)"""
    w = 3.0
    return dict(W=[np.full((MV, M1), w, np.float32), np.full((M1, M2), w, np.float32)],
                vb=np.full(MV, -w * M1 / 2 + 0.15, np.float32),
                hb=[np.full(M1, -w * (MV + M2) / 2, np.float32), np.full(M2, -w * M1 / 2, np.float32)])


def _other_mode_fraction(R, steps=240, M=512):
    p = _two_mode_model()
    e = T.Ensemble(p, M, np.linspace(0., 1., R + 1)[1:].astype(np.float32), seed=SEED,
                   V0_rows=np.zeros((M * R, MV), np.float32), H2_rows=np.zeros((M * R, M2), np.float32))
    e.sweep(steps)
    return float((e.read()[0].sum(axis=1) >= 4).mean())


def test_tempering_mixes_between_modes_and_a_single_temperature_does_not():
    """6-4-3 DBM with two well-separated modes (`_two_mode_model`), M = 512 independent chains, all started in the mode
    v = h2 = 0, 240 steps of burn-in (the deeper stack relaxes more slowly than the 6 x 4 RBM of tests/test_pt.py: the tempered
    fraction is 0.527 after 60 steps, 0.625 after 120, 0.701 after 240 - approaching the exact mass, as invariance says it
    must); "in the other mode" = at least 4 of the 6 visible units on.  Exact by enumeration: P(sum v >= 4) = 0.7100.
    Margin: 5 binomial standard deviations, 5 sqrt(p (1 - p) / 512) = 0.1003.
    Observed on the twin: R = 6 (betas 1/6 .. 1): 0.7012 (inside, 0.009 off); R = 1, the same call: 0.0000 (misses the bound by
    0.61 - no chain has left its mode; this is what shows the test has power)."""
    p = _two_mode_model()
    vs, _, P = T.exact_tempered_joint(p['W'], p['vb'], p['hb'], 1.0)
    exact = float(P.sum(axis=1)[vs.sum(axis=1) >= 4].sum())
    margin = 5.0 * np.sqrt(exact * (1.0 - exact) / 512)
    tempered, single = _other_mode_fraction(6), _other_mode_fraction(1)
    print('exact %.4f, margin %.4f, R = 6: %.4f, R = 1: %.4f' % (exact, margin, tempered, single))
    assert abs(exact - 0.7100) < 1e-4
    assert abs(tempered - exact) <= margin
    assert abs(single - exact) > margin


def _random_model(n, site0=1):
    return dict(W=[orc.normal(SEED, site0 + i, 0, n[i] * n[i + 1]).reshape(n[i], n[i + 1]) for i in range(len(n) - 1)],
                vb=orc.normal(SEED, site0 + 10, 0, n[0]) * np.float32(0.5),
                hb=[orc.normal(SEED, site0 + 11 + i, 0, n[i + 1]) * np.float32(0.5) for i in range(len(n) - 1)])


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_one_temperature_is_the_plain_sweep():
    """R = 1, betas = (1,): the twin is clamp_twin._dbm_sweep with all layers sampled and no clamp, bit for bit, and no swap
    is drawn"""
    n = [37, 20, 11]
    p = _random_model(n)
    M = 9
    V0 = (orc.uniform(SEED, 30, 0, M * n[0]) < 0.5).astype(np.float32).reshape(M, n[0])
    e = T.Ensemble(p, M, [1.0], seed=SEED, call=2, V0=V0)
    h20 = e.h[1].copy()
    e.sweep(3, call=2)
    v, H = V0, [None, h20]
    for t in range(3):
        v, H = clamp_twin._dbm_sweep(p['W'], p['hb'], p['vb'], None, 0, True, [True, True], v, H, True, t, SEED, 2, 0, None, None)
    gv, gh = e.read()
    assert _same(gv, v) and _same(gh[0], H[0]) and _same(gh[1], H[1])
    assert not e.margins and e.cnt.size == 0


def test_one_hidden_layer_is_the_rbm_twin():
    """L = 1 with the RBM's sites: pt_twin.Ensemble on the same parameters, bit for bit - states, ladder indices, counters and
    every swap margin, over two calls, from a random start"""
    V, H, R, M = 37, 22, 4, 7
    p = _random_model([V, H])
    betas = np.linspace(0., 1., R + 1)[1:].astype(np.float32)
    d = T.Ensemble(p, M, betas, seed=SEED, chain0=2,
                   sites=dict(h=clamp_twin.SITE_H, v=clamp_twin.SITE_V, swap=pt_twin.SITE_PT_SWAP, start=pt_twin.SITE_PT_V0))
    r = pt_twin.Ensemble(dict(W=p['W'][0], vb=p['vb'], hb=p['hb'][0]), M, betas, seed=SEED, chain0=2)
    assert _same(d.v, r.v)
    for call, n in enumerate((3, 4)):
        d.sweep(n, call=call)
        r.sweep(n, call=call)
        assert _same(d.v, r.v) and _same(d.h[0], r.h) and _same(d.mult, r.mult)
        assert np.array_equal(d.idx, r.idx) and np.array_equal(d.cnt, r.cnt)
    assert d.margins == r.margins and 0 < d.cnt[1].sum() < d.cnt[0].sum()
    # the DBM's own sites (8 / 12 / 14 / 15) give other draws
    own = T.Ensemble(p, M, betas, seed=SEED, chain0=2)
    assert (own.sites['h'], own.sites['v'], own.sites['swap'], own.sites['start']) == (8, 12, 14, 15)
    assert not _same(own.v, r.v)


def test_no_swap_draw_of_the_gpu_fixtures_is_a_near_tie():
    """the swap compares a float32 uniform with a double exp(): device and host may differ in its last place, so the seeds of
    the bit-for-bit GPU cases are chosen such that no draw lies within 1e-9 of its threshold (and acceptance is neither 0 nor 1)"""
    from tests import test_dbm_pt_gpu as G
    for n, R, M in G.SHAPES:
        for kw in (dict(), dict(with_v0=True)):
            want, margin = G.twin_run(n, R, M, (G.STEPS, G.STEPS), **kw)
            assert margin >= 1e-9, (n, kw, margin)
            att, acc = want[-1]['swaps']
            assert np.all(att > 0) and 0 < acc.sum() < att.sum()
    n, R, M = G.SHAPES[0]
    assert G.twin_run(n, R, 3, (G.STEPS,), chain0=2)[1] >= 1e-9
    assert G.twin_run(n[:2], R, M, (G.STEPS, G.STEPS))[1] >= 1e-9
    assert G.twin_run(n[:2], R, M, (G.STEPS, G.STEPS), rbm_sites=True)[1] >= 1e-9
    assert G.twin_run(n, R, M, (3, 2))[1] >= 1e-9
    assert G.twin_run(G.FULL, 4, 8, (2,))[1] >= 1e-9


def test_refusals():
    with pytest.raises(NotImplementedError, match='Gaussian'):
        T.check_model(2, v_unit=1)
    with pytest.raises(NotImplementedError, match='Multinomial'):
        T.check_model(2, h_units=[0, 2])
    with pytest.raises(NotImplementedError, match='OLD layer above'):
        T.check_model(3)
    with pytest.raises(NotImplementedError, match='OLD layer above'):
        T.Ensemble(_random_model([6, 5, 4, 3]), 2, [1.0], seed=SEED)
    with pytest.raises(NotImplementedError, match='literal'):
        T.check_model(2, literal=True)
    for bad in ([0.5, 0.5, 1.0], [0.6, 0.4, 1.0], [0.0, 1.0], [-0.5, 1.0], [0.5, 0.9], [0.5, 1.5], [1.0, 1.0], []):
        with pytest.raises(ValueError, match='betas'):
            T.Ensemble(_random_model([6, 5, 4]), 2, bad, seed=SEED)


def test_abi_surface():
    from boltzmann_machines_amd import DBM, _ffi
    from boltzmann_machines_amd.engine import DbmEngine, DbmEngine64
    assert [len(_ffi.SIGNATURES[n]) for n in ('bm_dbm_pt_init', 'bm_dbm_pt_sweep', 'bm_dbm_pt_read')] == [6, 2, 6]
    assert all(callable(getattr(DbmEngine, n, None)) for n in ('pt_init', 'pt_sweep', 'pt_read'))
    for n in ('pt_init', 'pt_sweep', 'pt_read'):
        with pytest.raises(NotImplementedError, match='float64'):
            getattr(DbmEngine64, n)(None)
    assert callable(getattr(DBM, 'sample_v_tempered', None))
    header = open(_ffi.__file__.replace('boltzmann_machines_amd/_ffi.py', 'include/bm355.h')).read()
    assert all(('int %s(' % n) in header for n in ('bm_dbm_pt_init', 'bm_dbm_pt_sweep', 'bm_dbm_pt_read'))
    assert 'bm_dbm64_pt' not in header
