"""Parallel tempering and the tempered negative phase over softmax visible units, checked on the CPU twin alone
(tests/softmax_pt_twin.py) and, for the public checks, on the Python layer without a device.  The twin is the reference of the GPU
tests (test_softmax_pt_gpu.py), so it is itself checked here against exact enumeration of models small enough for that."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import softmax_pt_twin as S
from tests import softmax_v_twin as SV

SEED = 20261021
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the twin against enumeration
def test_transition_leaves_the_product_distribution_invariant():
    """2 groups x 3 categories x 3 hidden units (9 x 8 joint states, enumerated in float64), N(0, 1) weights, R = 3, betas (0.3,
    0.6, 1).  20 000 independent chains start in the exact product distribution prod_r p_{beta_r}(v) (every row drawn by inverse
    CDF from the enumerated marginal); four steps of (up, swap, down) follow - both swap parities twice.  The (v, h) pairs of the
    beta = 1 rows - h ~ p(h | v_old), v ~ p(v | h) - must then be distributed as the exact joint p_1(v, h).  The statistic and its
    significance are test_pt.py's: every one of the 72 state frequencies within 5 binomial standard deviations,
    5 sqrt(p (1 - p) / M), + 2 / M for the states whose expected count is of order one; and, over the same 72 cells, Pearson's
    chi-square (71 degrees of freedom) below its quantile at the same 5 sigma (Wilson-Hilferty: 71 (1 - 2/639 + 5 sqrt(2/639))^3
    = 147.7).  The hot marginals stay where they are as well."""
    G, K, H, M = 2, 3, 3, 20000
    p = dict(W=orc.normal(SEED, 1, 0, G * K * H).reshape(G * K, H), vb=orc.normal(SEED, 2, 0, G * K) * f32(0.5),
             hb=orc.normal(SEED, 3, 0, H) * f32(0.5))
    betas = np.array([0.3, 0.6, 1.0], f32)
    R = len(betas)
    u = orc.uniform(SEED, 4, 0, M * R).reshape(M, R).astype(np.float64)
    rows = np.zeros((M, R, G * K), f32)
    marg = []
    for r, b in enumerate(betas):
        X, Hs, P = S.exact_tempered_joint(p, G, K, float(b))
        pv = P.sum(axis=1)
        marg.append(pv)
        rows[:, r] = X[np.minimum(np.searchsorted(np.cumsum(pv), u[:, r], side='right'), len(pv) - 1)]
    e = S.Ensemble(p, K, M, betas, seed=SEED, V0_rows=rows.reshape(M * R, G * K))
    X, Hs, exact = S.exact_tempered_joint(p, G, K, 1.0)

    def vcode(v):
        c = v.reshape(len(v), G, K).argmax(axis=2)
        return (c * (K ** np.arange(G - 1, -1, -1))[None, :]).sum(axis=1)          # the row of all_visible_states ('ij' order)
    assert np.array_equal(SV.all_visible_states(G, K)[1][vcode(rows[:, 0])], rows[:, 0])

    def bound(ex):
        return 5.0 * np.sqrt(ex * (1.0 - ex) / M) + 2.0 / M
    start = np.bincount(vcode(e.read()[0]), minlength=K ** G) / float(M)
    assert np.all(np.abs(start - marg[2]) <= bound(marg[2]))
    e.sweep(4)
    assert np.all(e.cnt[0] == [2 * M, 2 * M]) and np.all(e.cnt[1] > 0) and np.all(e.cnt[1] < e.cnt[0])
    assert np.array_equal(np.sort(e.idx.reshape(M, R), axis=1), np.tile(np.arange(R), (M, 1)))        # a permutation per chain
    assert np.array_equal(e.mult, betas[e.idx])
    v, h = e.read()
    assert np.all(v.reshape(M, G, K).sum(axis=2) == 1) and np.all((v == 0) | (v == 1))
    hcode = h.astype(np.int64).dot(1 << np.arange(H))
    freq = np.bincount(vcode(v) * (1 << H) + hcode, minlength=K ** G * (1 << H)).reshape(K ** G, 1 << H) / float(M)
    chi2 = float(M * np.sum((freq - exact) ** 2 / exact))
    chi2_bound = 71.0 * (1.0 - 2.0 / 639.0 + 5.0 * np.sqrt(2.0 / 639.0)) ** 3
    print('max |freq - exact| / bound: %.3f; chi-square %.1f (71 dof, bound %.1f)' % (np.max(np.abs(freq - exact) / bound(exact)), chi2, chi2_bound))
    assert np.all(np.abs(freq - exact) <= bound(exact))
    assert chi2 < chi2_bound
    for r in range(R - 1):
        rws = np.arange(M) * R + np.argmax(e.idx.reshape(M, R) == r, axis=1)
        fr = np.bincount(vcode(e.v[rws]), minlength=K ** G) / float(M)
        assert np.all(np.abs(fr - marg[r]) <= bound(marg[r]))


G2, K2 = 3, 3                          # the two-mode model of this file: 3 groups of 3, 4 hidden units


def _second_mode_fraction(R, steps=60, M=512):
    p = S.two_mode_model(G2, K2)
    V0 = SV.one_hot(np.zeros((M, G2), np.int64), K2)            # every chain in the first mode: category 0 everywhere
    e = S.Ensemble(p, K2, M, S.ladder(R), seed=SEED, V0=V0)
    e.sweep(steps)
    return float((e.read()[0].reshape(M, G2, K2)[:, :, 1].sum(axis=1) >= 2).mean()), e.near_ties()


def test_tempering_mixes_between_modes_and_a_single_chain_does_not():
    """softmax_pt_twin.two_mode_model at 3 groups x 3 categories x 4 hidden units: the modes are (category 0 everywhere, h = 0) and
    (category 1 everywhere, h = 1) - they differ in every group - the second the heavier.  M = 512 independent chains, all started
    in the first mode, 60 steps; "in the second mode" = at least 2 of the 3 groups at category 1.  Exact mass by enumeration
    against the fraction of the beta = 1 rows; margin: 5 binomial standard deviations.  R = 6 (betas 1/6 .. 1) must lie inside,
    the single-temperature twin chains (R = 1, the same call) outside: they do not reach the second mode."""
    p = S.two_mode_model(G2, K2)
    exact = S.mode_mass(p, G2, K2, 1, 2)
    margin = 5.0 * np.sqrt(exact * (1.0 - exact) / 512)
    (tempered, _), (single, _) = _second_mode_fraction(6), _second_mode_fraction(1)
    print('exact %.4f, margin %.4f, R = 6: %.4f, R = 1: %.4f' % (exact, margin, tempered, single))
    assert 0.5 < exact < 0.9
    assert abs(tempered - exact) <= margin
    assert abs(single - exact) > margin and single < 0.05


def test_one_temperature_is_the_plain_softmax_chain():
    """R = 1, betas = (1,) from a V0: the twin is the plain softmax twin chain bit for bit (1 * z + 1 * b is z + b), and no swap is
    drawn"""
    G, K, H, M = 7, 5, 22, 9
    p = S.make_params(G, K, H)
    V0 = S.train_batches(G, K, M, 3)
    e = S.Ensemble(p, K, M, [1.0], seed=SEED, V0=V0)
    e.sweep(3, call=2)
    v, h = S.plain_chain(p, K, V0, 3, SEED, call=2)
    assert np.array_equal(bits(e.read()[0]), bits(v)) and np.array_equal(bits(e.read()[1]), bits(h))
    assert not e.margins and e.cnt.size == 0


def test_random_start_is_one_hot_and_uniform():
    G, K = 40, 5
    v = S.categorical_start(SEED, 0, 7, 500, G * K, K)
    assert np.all(v.reshape(500, G, K).sum(axis=2) == 1) and np.all((v == 0) | (v == 1))
    share = v.reshape(-1, K).mean(axis=0)
    assert np.all(np.abs(share - 1.0 / K) <= 5.0 * np.sqrt(0.2 * 0.8 / (500 * G)))
    # rows [3, 10) of a start at row0 = 7 are the start at row0 = 10
    assert np.array_equal(v[3:10], S.categorical_start(SEED, 0, 10, 7, G * K, K))


def test_no_swap_draw_of_a_bit_for_bit_case_is_a_near_tie():
    """Every case the GPU tests compare bit for bit (softmax_pt_twin.SWEEP_CASES, the chain slices and the training cases): the
    number of swap draws within 1e-9 of their threshold - where the device's exp may decide the other way - is 0"""
    ties = 0
    for c in S.SWEEP_CASES:
        e, snaps = S.sweep_twin(c)
        G, K, H, M, R = c
        start = snaps[0]['v']
        assert np.all(start.reshape(M * R, G, K).sum(axis=2) == 1)
        assert e.step == 5 and (R == 1 or e.cnt[0].sum() > 0)
        ties += e.near_ties()
    for c in ((5, 4, 8, 5, 3), (3, 5, 24, 5, 3)):           # the chain slices: 7 chains at chain0 = 4 hold the 3 at chain0 = 6
        ties += S.sweep_twin(c, chain0=4, M=7)[0].near_ties()
    for c in S.TRAIN_CASES:                                 # three updates, the short last batch, lr = 0
        G, K, H, M, R = c
        for lr, steps in ((0.05, (4, 4, 4)), (0.05, (4, 4, 2)), (0.0, (4, 4))):
            t = S.TemperedCategoricalRBM(S.make_params(G, K, H), K, M, S.ladder(R), S.TRAIN_SEED, l2=1e-3)
            X, s = S.train_batches(G, K, sum(steps), 1), 0
            for B in steps:
                t.train_step(X[s:s + B], lr, 0.5, 2)
                s += B
            ties += t.ens.near_ties()
    print('near ties: %d' % ties)
    assert ties == 0


def test_chain_slices_are_the_small_ensemble():
    c = (5, 4, 8, 5, 3)
    whole, _ = S.sweep_twin(c, chain0=4, M=7)
    part, _ = S.sweep_twin(c, chain0=6, M=3)
    R = c[4]
    for n in ('v', 'h', 'part_v', 'part_h', 'mult', 'idx'):
        assert np.array_equal(getattr(whole, n)[2 * R:5 * R], getattr(part, n)), n


# ------------------------------------------------------------------------------------------------ training
def test_zero_learning_rate_is_a_sweep():
    G, K, H, R, M, B, k = 5, 4, 24, 4, 9, 7, 2
    p = S.make_params(G, K, H)
    t = S.TemperedCategoricalRBM(p, K, M, S.ladder(R), SEED, l2=1e-3)
    X = S.train_batches(G, K, 2 * B, 2)
    for i in range(2):
        t.train_step(X[B * i:B * i + B], 0.0, 0.9, k)
    e = S.Ensemble(p, K, M, S.ladder(R), seed=SEED)
    e.sweep(k, call=0)
    e.sweep(k, call=1)
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(t.p[n]), bits(p[n])), n
    assert np.array_equal(bits(t.ens.v), bits(e.v)) and np.array_equal(bits(t.ens.h), bits(e.h))
    assert np.array_equal(t.ens.idx, e.idx) and np.array_equal(t.ens.cnt, e.cnt) and t.ens.step == e.step == 2 * k
    assert np.array_equal(bits(t.ens.part_v), bits(e.part_v))
    assert t.call == 2 and 0 < e.cnt[1].sum() < e.cnt[0].sum()


def test_rescore_with_unchanged_vb_is_the_identity():
    G, K, H, R, M = 7, 5, 22, 4, 9
    p = S.make_params(G, K, H)
    e = S.Ensemble(p, K, M, S.ladder(R), seed=SEED)
    for sweep in (0, 3):
        if sweep:
            e.sweep(sweep)
        before = e.part_v.copy()
        e.rescore()
        assert np.array_equal(bits(e.part_v), bits(before))
    e.set_params(dict(p, vb=p['vb'] + f32(0.25)))
    e.rescore()
    assert not np.array_equal(bits(e.part_v), bits(before))


def test_tempered_negative_statistic_is_unbiased_where_cd1_is_not():
    """The two-mode model again.  The negative statistic of the update, S_ij = mean_c v_ci hbar_cj over the M = 4096 beta = 1 rows
    (hbar = E[h | v]), against E[v_i h_j] by enumeration.  Bound, entry by entry: 5 binomial standard deviations,
    5 sqrt(E (1 - E) / M) - v_i hbar_j lies in [0, 1], so its variance is at most that of a Bernoulli variable of the same mean, and
    the chains are independent.  Tempered leg: R = 6, random start, 100 steps.  CD-1 leg: the same number of chains started in the
    first mode, one step h ~ p(h|v), v ~ p(v|h): it misses in the entries of the second mode."""
    from tests import pt_train_twin as PT
    M, R = 4096, 6
    p = S.two_mode_model(G2, K2)
    exact = S.exact_vh(p, G2, K2)
    bound = 5.0 * np.sqrt(exact * (1.0 - exact) / M)

    def statistic(v):
        return v.T.astype(np.float64).dot(PT.hidden_means(p, v).astype(np.float64)) / M
    e = S.Ensemble(p, K2, M, S.ladder(R), seed=SEED)
    e.sweep(100)
    tempered = statistic(e.read()[0])
    v, _ = S.plain_chain(p, K2, SV.one_hot(np.zeros((M, G2), np.int64), K2), 1, SEED)
    cd1 = statistic(v)
    second = np.arange(G2) * K2 + 1                        # the units of category 1
    print('exact (second mode) %.4f, bound %.4f, tempered max dev / bound %.3f, CD-1 min dev / bound (second mode) %.1f'
          % (exact[second].max(), bound[second].max(), np.max(np.abs(tempered - exact) / bound),
             np.min(np.abs(cd1 - exact)[second] / bound[second])))
    assert np.all(np.abs(tempered - exact) <= bound)
    assert np.all(np.abs(cd1 - exact)[second] > bound[second])


def test_twin_update_moves_towards_the_tempered_statistic():
    """one update of the twin, restated in NumPy float64 for a batch shorter than the ensemble, momentum 0, no l2"""
    from tests import pt_train_twin as PT
    G, K, H, R, M, B = 4, 4, 16, 3, 9, 5
    p = S.make_params(G, K, H)
    X = S.train_batches(G, K, B, 4)
    t = S.TemperedCategoricalRBM(p, K, M, S.ladder(R), SEED, l2=0.0)
    t.train_step(X, 0.1, 0.0, 1)
    e = S.Ensemble(p, K, M, S.ladder(R), seed=SEED)
    e.sweep(1, call=0)
    vs = e.read()[0][:B]
    pos, neg = X.T.dot(PT.hidden_means(p, X)), vs.T.dot(PT.hidden_means(p, vs))
    want = p['W'].astype(np.float64) + 0.1 * (pos.astype(np.float64) - neg) / B
    assert np.max(np.abs(t.p['W'] - want)) < 1e-5
    assert np.max(np.abs(t.p['vb'] - (p['vb'] + 0.1 * (X.sum(0) - vs.sum(0)) / B))) < 1e-5


# ------------------------------------------------------------------------------------------------ no device needed
def test_abi_surface():
    from boltzmann_machines_amd import _ffi, CategoricalRBM
    from boltzmann_machines_amd.engine import RbmEngine, RbmGroupsPt
    names = ('bm_rbm_groups_pt_init', 'bm_rbm_groups_pt_sweep', 'bm_rbm_groups_pt_read', 'bm_rbm_groups_train_step_pt',
             'bm_rbm_groups_train_epoch_pt')
    assert [len(_ffi.SIGNATURES[n]) for n in names] == [6, 2, 5, 6, 7]
    assert RbmGroupsPt._pt_prefix == 'bm_rbm_groups' and isinstance(RbmEngine.groups_pt, property)
    assert all(callable(getattr(RbmGroupsPt, n, None)) for n in ('pt_init', 'pt_sweep', 'pt_read', 'train_step_pt', 'train_epoch_pt'))
    assert all(callable(getattr(CategoricalRBM, n, None)) for n in ('sample_v_tempered', 'set_group_tempering', 'tempering_stats'))
    import os
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'bm355.h')).read()
    assert all('int %s(' % n in header for n in names)


def test_public_checks_without_a_device(tmp_path, monkeypatch):
    import boltzmann_machines_amd as bm
    monkeypatch.delenv('BM355_DATA_PARALLEL', raising=False)
    kw = dict(n_groups=3, n_categories=4, n_hidden=8, batch_size=5, verbose=False, model_path=str(tmp_path / 'm') + '/')
    m = bm.CategoricalRBM(**kw)
    made = []
    monkeypatch.setattr(bm.CategoricalRBM, '_ensure_engine', lambda self: made.append(1))       # no check below may reach the engine
    good = SV.one_hot(np.zeros((6, 3), np.int64), 4)
    # sample_v_tempered: counts, ladder, shape and one-hot completeness of V_init
    for bad in (dict(n_samples=0), dict(n_gibbs_steps=0), dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.5, 0.9]), dict(n_temperatures=0),
                dict(V_init=good[:5]), dict(V_init=good[:, :8]), dict(V_init=2 * good), dict(V_init=np.ones_like(good))):
        with pytest.raises(ValueError):
            m.sample_v_tempered(**dict(dict(n_samples=6, n_gibbs_steps=2), **bad))
    empty = good.copy()
    empty[2, 4:8] = 0
    with pytest.raises(ValueError, match='group 1 of row 2'):
        m.sample_v_tempered(6, 2, V_init=empty)
    # set_group_tempering
    with pytest.raises(ValueError, match='softmax visible units'):
        bm.CategoricalRBM(missing_values=True, **kw).set_group_tempering()
    for bad in (dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.5, 0.9]), dict(n_temperatures=0), dict(n_chains=4)):
        with pytest.raises(ValueError):
            m.set_group_tempering(**bad)
    assert m._neg_phase is None
    assert m.set_group_tempering(n_temperatures=4) is m
    betas, n_chains = m._neg_phase
    assert np.array_equal(f32(betas), np.linspace(0., 1., 5)[1:].astype(f32)) and n_chains == 5
    assert m.set_group_tempering(betas=[0.25, 1.0], n_chains=9)._neg_phase == ((0.25, 1.0), 9)
    assert not any('neg' in k or 'temper' in k for k in m.get_params())
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        m.tempering_stats()
    # n_chains < batch_size after set_params: refused when fit checks the setting again
    m.set_params(batch_size=12)
    with pytest.raises(ValueError, match='n_chains'):
        m._check_tempered_fit()
    m.set_params(batch_size=5)
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(NotImplementedError, match='BM355_DATA_PARALLEL'):
        m.set_group_tempering()
    monkeypatch.delenv('BM355_DATA_PARALLEL')
    assert m.set_group_tempering(False)._neg_phase is None
    # the Bernoulli entry stays refused for this unit, and 'cd' stays accepted
    with pytest.raises(ValueError, match='the tempered sweep has no softmax pass'):
        m.set_negative_phase('tempered')
    assert m.set_negative_phase('cd') is m and m._neg_phase is None
    assert not made
