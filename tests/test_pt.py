"""Parallel tempering, checked on the CPU twin alone (tests/pt_twin.py: the tempered sweeps as loops of the oracle's activation
stage, the swap step in NumPy float64).  The twin is the reference of the GPU tests (test_pt_gpu.py), so it is itself checked
here against exact enumeration of a model small enough for that: the transition leaves the target distribution where it is,
and it mixes between modes a single Gibbs chain does not leave."""
import numpy as np

from oracle import oracle as orc
from tests import pt_twin as T

V, H, SEED = 6, 4, 20241018


def _exact_rows(p, betas, M, site):
    """[M R][V]: row c R + r drawn exactly from p_{beta_r}(v) (inverse CDF over the 2^V states, one uniform per row)"""
    R = len(betas)
    u = orc.uniform(SEED, site, 0, M * R).reshape(M, R).astype(np.float64)
    rows = np.zeros((M, R, V), np.float32)
    for r, b in enumerate(betas):
        vs, pr = T.exact_tempered_visible(p['W'], p['vb'], p['hb'], float(b))
        code = np.minimum(np.searchsorted(np.cumsum(pr), u[:, r], side='right'), len(pr) - 1)
        rows[:, r] = vs[code]
    return rows.reshape(M * R, V)


def test_transition_leaves_the_target_invariant():
    """Detailed balance, by a LARGE-SAMPLE ESTIMATE (not by enumerating the joint): 6 x 4 RBM with N(0, 1) weights, R = 3,
    betas (0.3, 0.6, 1).  20 000 independent chains start in the exact product distribution prod_r p_{beta_r}(v) (every row
    drawn by inverse CDF from the enumerated p_beta); four steps of (up, swap, down) follow - both swap parities twice, the
    pair that holds beta = 1 is the odd one.  The beta = 1 rows must still be distributed as the exact p_1(v): every one of
    the 64 state frequencies within 5 binomial standard deviations, 5 sqrt(p (1 - p) / M), + 2 / M for the states whose
    expected count is of order one (there the binomial is Poisson-like and 5 sigma alone is not a 5 sigma bound).  The
    start has the same bound, so a twin whose swap rule favoured either side would show as a drift between the two."""
    p = dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H), vb=orc.normal(SEED, 2, 0, V) * np.float32(0.5),
             hb=orc.normal(SEED, 3, 0, H) * np.float32(0.5))
    betas = np.array([0.3, 0.6, 1.0], np.float32)
    M = 20000
    e = T.Ensemble(p, M, betas, seed=SEED, V0_rows=_exact_rows(p, betas, M, 4))
    vs, exact = T.exact_tempered_visible(p['W'], p['vb'], p['hb'], 1.0)
    bound = 5.0 * np.sqrt(exact * (1.0 - exact) / M) + 2.0 / M
    weights = (1 << np.arange(V))

    def freq(v):
        return np.bincount(v.astype(np.int64).dot(weights), minlength=1 << V) / float(M)
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
    # the hot marginals stay where they are as well
    for r, b in enumerate(betas[:-1]):
        _, ex = T.exact_tempered_visible(p['W'], p['vb'], p['hb'], float(b))
        rows = np.arange(M) * 3 + np.argmax(e.idx.reshape(M, 3) == r, axis=1)
        assert np.all(np.abs(freq(e.v[rows]) - ex) <= 5.0 * np.sqrt(ex * (1.0 - ex) / M) + 2.0 / M)


def _two_mode_model():
    """all weights w = 3, vb = -w H / 2 + 0.15, hb = -w V / 2: in +-1 spins a ferromagnet, the modes are v = h = 0 and
    v = h = 1, the tilt 0.15 on vb makes the second one the heavier (so the exact answer is not 1/2 by symmetry)"""
    w = 3.0
    return dict(W=np.full((V, H), w, np.float32), vb=np.full(V, -w * H / 2 + 0.15, np.float32),
                hb=np.full(H, -w * V / 2, np.float32))


def _other_mode_fraction(R, steps=60, M=512):
    p = _two_mode_model()
    e = T.Ensemble(p, M, np.linspace(0., 1., R + 1)[1:].astype(np.float32), seed=SEED, V0=np.zeros((M, V), np.float32))
    e.sweep(steps)
    return float((e.read()[0].sum(axis=1) >= 4).mean())


def test_tempering_mixes_between_modes_and_a_single_chain_does_not():
    """6 x 4 RBM with two well-separated modes (`_two_mode_model`), M = 512 independent chains, all started in the mode
    v = 0, 60 steps of burn-in; "in the other mode" = at least 4 of the 6 visible units on.  Exact by enumeration:
    P(sum v >= 4) = 0.7100.  Margin: 5 binomial standard deviations, 5 sqrt(p (1 - p) / 512) = 0.1003.
    Observed on the twin: R = 6 (betas 1/6 .. 1): 0.6582 (inside, 0.052 off); R = 1, the same call: 0.0000 (misses the bound by
    0.61 - no chain has left its mode; this is what shows the test has power)."""
    p = _two_mode_model()
    vs, pr = T.exact_tempered_visible(p['W'], p['vb'], p['hb'], 1.0)
    exact = float(pr[vs.sum(axis=1) >= 4].sum())
    margin = 5.0 * np.sqrt(exact * (1.0 - exact) / 512)
    tempered, single = _other_mode_fraction(6), _other_mode_fraction(1)
    print('exact %.4f, margin %.4f, R = 6: %.4f, R = 1: %.4f' % (exact, margin, tempered, single))
    assert abs(exact - 0.7100) < 1e-4
    assert abs(tempered - exact) <= margin
    assert abs(single - exact) > margin


def test_one_temperature_is_the_plain_gibbs_loop():
    """R = 1, betas = (1,): the twin is clamp_twin's unclamped loop bit for bit, and no swap is drawn"""
    from tests import clamp_twin
    p = dict(W=orc.normal(SEED, 1, 0, 37 * 22).reshape(37, 22), vb=orc.normal(SEED, 2, 0, 37) * np.float32(0.5),
             hb=orc.normal(SEED, 3, 0, 22) * np.float32(0.5), sigma=np.ones(37, np.float32))
    V0 = (orc.uniform(SEED, 5, 0, 9 * 37) < 0.5).astype(np.float32).reshape(9, 37)
    e = T.Ensemble(p, 9, [1.0], seed=SEED, V0=V0)
    e.sweep(3, call=2)
    v, h, _ = clamp_twin.rbm_gibbs_clamped(p, V0, None, None, 3, seed=SEED, call=2, clamped=False)
    assert np.array_equal(e.read()[0].view(np.uint32), v.view(np.uint32)) and np.array_equal(e.read()[1].view(np.uint32), h.view(np.uint32))
    assert not e.margins and e.cnt.size == 0


def test_slot_partials_restate_the_epilogue_order():
    """a sum the order matters for: the slot of 16 terms is ((x0+x1)+x2)+x3 per quad, then (q0+q1)+(q2+q3); ragged tails are
    short quads"""
    x = (orc.normal(SEED, 9, 0, 3 * 37) * np.float32(1e3)).reshape(3, 37)
    got = T.slot_partials(x)
    assert got.shape == (3, 3)
    f = np.float32
    for r in range(3):
        for s in range(3):
            q = []
            for g in range(4):
                acc = f(0)
                for c in range(s * 16 + 4 * g, min(s * 16 + 4 * g + 4, 37)):
                    acc = f(acc + x[r, c])
                q.append(acc)
            assert got[r, s] == f(f(q[0] + q[1]) + f(q[2] + q[3]))


def test_abi_surface():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
    from boltzmann_machines_amd import BernoulliRBM
    assert [len(_ffi.SIGNATURES[n]) for n in ('bm_rbm_pt_init', 'bm_rbm_pt_sweep', 'bm_rbm_pt_read')] == [6, 2, 5]
    assert all(callable(getattr(RbmEngine, n, None)) for n in ('pt_init', 'pt_sweep', 'pt_read'))
    assert not hasattr(RbmEngine64, 'pt_init')
    assert callable(getattr(BernoulliRBM, 'sample_v', None))
