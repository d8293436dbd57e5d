"""Parallel tempering and the tempered negative phase over replicated softmax visible units, checked on the CPU twin
alone (tests/rsm_pt_twin.py) and, for the public checks, on the Python layer without a device.  The twin is the reference of the GPU
tests (test_rsm_pt_gpu.py), so it is itself checked here against exact enumeration of models small enough for that.

The statistical tests run thousands of rows: there the twin's count draw - a Python loop over rows - is replaced by the same
sampler vectorised over rows (the pinned uniforms of the same positions, a NumPy softmax and NumPy prefix sums); every other step,
the swap included, is the twin's own."""
import functools

import numpy as np
import pytest

from boltzmann_machines_amd.utils import philox
from tests import multinomial_probes as P
from tests import rsm_pt_twin as S
from tests import rsm_twin as rt

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


class FastEnsemble(S.Ensemble):
    """the twin with the count draw vectorised over rows: draw d of global row r reads position r * max_length + d"""

    def _counts(self, l, site, call, row0):
        rows, V = l.shape
        ML = self.max_length
        e = np.exp(l.astype(np.float64) - l.max(axis=1, keepdims=True))
        c = np.cumsum(e, axis=1)
        U = philox.uniform(self.seed, site, call, rows * ML, idx0=row0 * ML).reshape(rows, ML).astype(np.float64)
        out = np.zeros((rows, V), f32)
        for d in range(ML):
            live = self.len > d
            cat = np.minimum((c <= (U[:, d] * c[:, -1])[:, None]).sum(axis=1), V - 1)
            np.add.at(out, (np.nonzero(live)[0], cat[live]), 1.0)
        return out


# ------------------------------------------------------------------------------------------------ the twin against enumeration
@functools.lru_cache(maxsize=None)
def invariance_run():
    """V = 4, H = 2, chains of D = 2 and D = 3 side by side, R = 3, 20 000 chains, 12 steps from the all-on-word-0 start"""
    p = rt.small_model()
    M = 20000
    D = np.where(np.arange(M) % 2 == 0, 2, 3).astype(f32)
    V0 = np.zeros((M, 4), f32)
    V0[:, 0] = D
    e = FastEnsemble(p, D, S.ladder(3), 515, 3, V0=V0)
    e.sweep(12)
    return p, D, e


def test_tempered_chains_sample_the_model_at_every_length():
    """the beta = 1 counts of each length against exact_pv, chi_square_z within the cap tests/test_rsm.py uses for the plain chain; the
    same statistic on the beta_0 replicas exceeds the cap - the test has power"""
    p, D, e = invariance_run()
    v1 = e.read()[0]
    hot = e.v[e.idx == 0]
    assert np.array_equal(e.v.sum(axis=1), e.len)
    for length in (2, 3):
        X, pv = rt.exact_pv(p, length)
        rows = D == length
        z, exmin = rt.chi_square_z(np.bincount(rt.cell_index(X, v1[rows]), minlength=len(X)).astype(np.float64), pv)
        zh, _ = rt.chi_square_z(np.bincount(rt.cell_index(X, hot[rows]), minlength=len(X)).astype(np.float64), pv)
        print('D = %d: z = %+.2f at beta = 1 (smallest expected cell %.1f), z = %+.2f at beta_0' % (length, z, exmin, zh))
        assert abs(z) <= P.Z_CAP
        assert abs(zh) > P.Z_CAP
    # the hot replicas sample THEIR distribution: p_beta with the untempered coefficient
    X, pb = S.exact_pv_beta(p, 3, float(S.ladder(3)[0]))
    zb, _ = rt.chi_square_z(np.bincount(rt.cell_index(X, hot[D == 3]), minlength=len(X)).astype(np.float64), pb)
    assert abs(zb) <= P.Z_CAP, zb
    assert np.all(e.cnt[0] > 0) and np.all(e.cnt[1] > 0)


def test_the_unmodified_twin_samples_the_model():
    """the same check on S.Ensemble ITSELF - the pinned count draw of rt.softmax_counts: the oracle's e, the prefix order, the
    bisection - at a size its Python loop over rows affords: 2000 chains of D = 3, R = 3, 10 steps"""
    p = rt.small_model()
    M = 2000
    D = np.full(M, 3, f32)
    V0 = np.zeros((M, 4), f32)
    V0[:, 0] = 3
    e = S.Ensemble(p, D, S.ladder(3), 818, 3, V0=V0)
    e.sweep(10)
    X, pv = rt.exact_pv(p, 3)
    z, exmin = rt.chi_square_z(np.bincount(rt.cell_index(X, e.read()[0]), minlength=len(X)).astype(np.float64), pv)
    zh, _ = rt.chi_square_z(np.bincount(rt.cell_index(X, e.v[e.idx == 0]), minlength=len(X)).astype(np.float64), pv)
    print('unmodified twin: z = %+.2f at beta = 1 (smallest expected cell %.1f), z = %+.2f at beta_0' % (z, exmin, zh))
    assert abs(z) <= P.Z_CAP and abs(zh) > P.Z_CAP


# The ladder: the two topics are coupled through beta w D = 24 beta, so the bottom rung sits where that coupling is about one (0.05:
# a hot replica crosses in a step or two) and every rung roughly doubles beta.  120 steps: the mass that has not yet left the start
# topic decays geometrically with the round trips of a four-rung ladder (a few steps each).
TOPIC_D, TOPIC_M, TOPIC_STEPS = 6, 4096, 120
TOPIC_LADDER = (0.05, 0.2, 0.45, 1.0)


@functools.lru_cache(maxsize=None)
def topic_run(ladder):
    p = S.two_topic_model()
    D = np.full(TOPIC_M, TOPIC_D, f32)
    V0 = np.zeros((TOPIC_M, 4), f32)
    V0[:, 0] = TOPIC_D                                  # every chain starts inside topic A
    e = FastEnsemble(p, D, np.array(ladder, f32), 616, TOPIC_D, V0=V0)
    e.sweep(TOPIC_STEPS)
    return p, e


def in_topic_b(v):
    return v[:, 2:].sum(axis=1) > TOPIC_D / 2.0


def test_tempering_mixes_between_topics_and_a_single_chain_does_not():
    """a planted two-topic model: the single-temperature chain (R = 1: the plain `sample_v` twin, bit for bit - see below) stays in
    its start topic; the tempered mass of the other topic lies within 5 binomial standard deviations of the enumerated mass"""
    p, plain = topic_run((1.0,))
    assert in_topic_b(plain.read()[0]).sum() == 0
    p, e = topic_run(TOPIC_LADDER)
    want = S.topic_mass(p, TOPIC_D)
    got = in_topic_b(e.read()[0]).mean()
    sd = np.sqrt(want * (1 - want) / TOPIC_M)
    print('mass of topic B: %.4f tempered, %.4f exact, sd %.4f' % (got, want, sd))
    assert 0.5 < want < 0.99
    assert abs(got - want) <= 5 * sd


def test_tempered_negative_statistic_is_unbiased_where_cd1_is_not():
    """E[v_i h_j] from the 4096 tempered chains of the two-topic run lies within 5 standard deviations of the enumerated value in
    every entry; CD-1 from documents of topic A misses it"""
    p, e = topic_run(TOPIC_LADDER)
    want = S.exact_vh(p, TOPIC_D)
    D = np.full(TOPIC_M, TOPIC_D, f32)
    vs = e.read()[0]
    hm = rt.db_up(vs, p['W'], p['hb'], D, 0, 0, 0, 0)[0].astype(np.float64)
    got = (vs.astype(np.float64)[:, :, None] * hm[:, None, :]).mean(axis=0)
    # the standard deviation of one sample's v_i E[h_j | v] under the MODEL, by enumeration (the sample's own is degenerate in the
    # entries that only rare count vectors feed)
    X, pv = rt.exact_pv(p, TOPIC_D)
    hbar = 1.0 / (1.0 + np.exp(-(X.dot(p['W'].astype(np.float64)) + TOPIC_D * p['hb'].astype(np.float64))))
    x = X[:, :, None] * hbar[:, None, :]
    mean = (pv[:, None, None] * x).sum(axis=0)
    assert np.allclose(mean, want, rtol=1e-9, atol=1e-12)
    sd = np.sqrt(np.maximum((pv[:, None, None] * x * x).sum(axis=0) - mean * mean, 0.0) / TOPIC_M)
    assert np.all(np.abs(got - want) <= 5 * sd + 1e-9), np.abs(got - want) / (sd + 1e-12)
    Xa = np.zeros((TOPIC_M, 4), f32)
    Xa[:, 0], Xa[:, 1] = TOPIC_D // 2, TOPIC_D - TOPIC_D // 2
    v1, h1 = S.plain_chain(p, Xa[:256], D[:256], 1, 717, TOPIC_D)
    hm1 = rt.db_up(v1, p['W'], p['hb'], D[:256], 0, 0, 0, 0)[0].astype(np.float64)
    cd = (v1.astype(np.float64)[:, :, None] * hm1[:, None, :]).mean(axis=0)
    assert np.max(np.abs(cd - want)) > 1.0


# ------------------------------------------------------------------------------------------------ the twin against itself
def test_one_temperature_is_the_plain_chain():
    for V, H, M in ((17, 16, 5), (257, 40, 4)):
        p = S.make_params(V, H)
        D = S.chain_lengths(M, S.MAX_LENGTH, seed=3)
        V0 = S.uniform_start(5, 0, 0, D, V, S.MAX_LENGTH)
        e = S.Ensemble(p, D, [1.0], 77, S.MAX_LENGTH, V0=V0)
        e.sweep(3)
        v, h = S.plain_chain(p, V0, D, 3, 77, S.MAX_LENGTH)
        assert np.array_equal(bits(e.v), bits(v)) and np.array_equal(bits(e.h), bits(h))
        assert e.cnt.size == 0


def test_uniform_start_and_pair():
    D = S.chain_lengths(40, S.MAX_LENGTH)
    v = S.uniform_start(3, 0, 5, D, 300, S.MAX_LENGTH)
    assert np.array_equal(v.sum(axis=1), D) and np.all(v >= 0)
    vb = S.make_params(300, 4)['vb']
    pair = S.vb_pair(v, vb).astype(np.float64)
    exact = v.astype(np.float64).dot(vb.astype(np.float64))
    assert np.all(np.abs(pair.sum(axis=1) - exact) <= 1e-12 * np.maximum(1.0, np.abs(exact)))
    assert np.array_equal(bits(pair[:, 0]), bits(exact.astype(f32)))


def test_no_swap_draw_of_a_bit_for_bit_case_is_a_near_tie():
    """asserted on the twin first: no swap uniform within 1e-9 of its threshold in any case the GPU tests compare bit for bit"""
    for c in S.SWEEP_CASES + [(257, 17, 7, 4)]:
        for chain0, M in ((S.SWEEP_CHAIN0, None),) if c[2] != 7 else ((4, 7), (7, 3)):
            e = S.sweep_twin(c if M is None else (c[0], c[1], M, c[3]), chain0=chain0)[0]
            assert e.near_ties() == 0, (c, chain0)
            assert np.array_equal(e.v.sum(axis=1), e.len)
    for c in S.TRAIN_CASES:
        V, H, M, R = c
        t = S.TemperedRsmRBM(S.make_params(V, H), S.chain_lengths(M, S.MAX_LENGTH, seed=2), S.ladder(R), S.TRAIN_SEED, S.MAX_LENGTH, l2=1e-3)
        X = S.train_batches(V, 12, 1)
        for s in range(0, 12, 4):
            t.train_step(X[s:s + 4], 0.05, 0.5, 2)
        assert t.ens.near_ties() == 0, c


def test_chain_slices_are_the_small_ensemble():
    c = (257, 17, 7, 4)
    whole = S.sweep_twin(c, chain0=4)[1]
    part = S.sweep_twin((257, 17, 3, 4), chain0=7)[1]
    for a, b in zip(whole, part):
        for k in ('v', 'h', 'mult', 'idx', 'len'):
            assert np.array_equal(a[k][12:24], b[k]), k


# ------------------------------------------------------------------------------------------------ training
def test_zero_learning_rate_is_a_sweep_and_the_rescore_is_the_identity():
    V, H, M, R = S.TRAIN_CASES[0]
    p, D = S.make_params(V, H), S.chain_lengths(M, S.MAX_LENGTH, seed=2)
    t = S.TemperedRsmRBM(p, D, S.ladder(R), S.TRAIN_SEED, S.MAX_LENGTH, l2=1e-3)
    e = S.Ensemble(p, D, S.ladder(R), S.TRAIN_SEED, S.MAX_LENGTH)
    X = S.train_batches(V, 8, 1)
    for n in range(2):
        before = t.ens.part_v.copy()
        t.ens.rescore()
        assert np.array_equal(bits(t.ens.part_v), bits(before))
        t.train_step(X[4 * n:4 * n + 4], 0.0, 0.5, 2)
        e.sweep(2, call=n)
        for k, w in S.snapshot(e).items():
            assert np.array_equal(t.state()[k], w), (n, k)
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(t.p[n]), bits(p[n]))


def test_two_length_bias_sums_against_float64():
    """every term is two rounded products and one rounded difference, |term error| <= 3 u max(D) (|h| <= 1), and row b adds one
    rounding of a partial sum bounded by b max(D): |s - s64| <= u max(D) (3 B + B (B + 1) / 2), u = 2^-24"""
    rng = np.random.RandomState(5)
    for B in (1, 7, 64, 130):
        D, Dn = rng.randint(1, 1000, B).astype(f32), rng.randint(1, 1000, B).astype(f32)
        h0, hk = rng.uniform(size=(B, 9)).astype(f32), rng.uniform(size=(B, 9)).astype(f32)
        s = S.two_length_bias_sums(D, Dn, h0, hk)
        bound = 2.0 ** -24 * max(D.max(), Dn.max()) * (3 * B + B * (B + 1) / 2.0)
        assert np.all(np.abs(s.astype(np.float64) - S.two_length_bias_sums64(D, Dn, h0, hk)) <= bound)
    # equal lengths: not the CD kernel's bits in general (D (h0 - hk) rounds once), but the same number to the bound
    assert np.allclose(S.two_length_bias_sums(D, D, h0, hk), rt.weighted_bias_sums(D, h0, hk), rtol=0, atol=2 * bound)


# ------------------------------------------------------------------------------------------------ host logic
def test_abi_surface():
    from boltzmann_machines_amd import _ffi, ReplicatedSoftmaxRBM
    from boltzmann_machines_amd.engine import RbmEngine, RbmRsmPt
    names = ('bm_rbm_rsm_pt_init', 'bm_rbm_rsm_pt_sweep', 'bm_rbm_rsm_pt_read', 'bm_rbm_rsm_train_step_pt', 'bm_rbm_rsm_train_epoch_pt')
    assert [len(_ffi.SIGNATURES[n]) for n in names] == [7, 2, 5, 6, 7]
    assert len(_ffi.SIGNATURES['bm_debug_rsm_up']) == 8 and callable(getattr(RbmEngine, 'debug_rsm_up', None))
    assert RbmRsmPt._pt_prefix == 'bm_rbm_rsm' and isinstance(RbmEngine.rsm_pt, property)
    assert all(callable(getattr(RbmRsmPt, n, None)) for n in ('pt_init', 'pt_sweep', 'pt_read', 'train_step_pt', 'train_epoch_pt'))
    assert all(callable(getattr(ReplicatedSoftmaxRBM, n, None)) for n in ('sample_v_tempered', 'set_count_tempering', 'tempering_stats'))
    import os
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'bm355.h')).read()
    assert all('int %s(' % n in header for n in names)


class StubLib(object):
    """records the C-ABI calls of an RbmRsmPt view"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_view_checks_on_a_stub_engine():
    from boltzmann_machines_amd.engine import RbmRsmPt

    class Eng(object):
        lib, V, H, _h = StubLib(), 6, 3, 1234
    view = RbmRsmPt(Eng())
    with pytest.raises(ValueError, match='document lengths'):
        view.pt_init(3, [0.5, 1.0])
    with pytest.raises(ValueError, match='2 lengths for 3 chains'):
        view.pt_init(3, [0.5, 1.0], lengths=[4, 5])
    view.train_lengths = np.array([4, 5, 6], f32)
    view.pt_init(3, [0.5, 1.0], chain0=2)
    name, args = Eng.lib.calls[-1]
    assert name == 'bm_rbm_rsm_pt_init' and args[0] == 1234 and args[1:3] == (3, 2) and args[5] is None and args[6] == 2
    assert view._pt_shape == (3, 2) and view._pt_train_key is None
    view.pt_sweep(4)
    assert Eng.lib.calls[-1] == ('bm_rbm_rsm_pt_sweep', (1234, 4))
    swaps, idx = view.pt_read()
    assert Eng.lib.calls[-1][0] == 'bm_rbm_rsm_pt_read' and swaps.shape == (2, 1) and idx.shape == (3, 2)
    with pytest.raises(TypeError):
        view.pt_read(None, None, None)


def test_public_checks_without_a_device(tmp_path, monkeypatch):
    import boltzmann_machines_amd as bm
    monkeypatch.delenv('BM355_DATA_PARALLEL', raising=False)
    kw = dict(n_visible=6, n_hidden=4, max_length=9, batch_size=5, verbose=False, model_path=str(tmp_path / 'm') + '/')
    m = bm.ReplicatedSoftmaxRBM(**kw)
    made = []
    monkeypatch.setattr(bm.ReplicatedSoftmaxRBM, '_ensure_engine', lambda self: made.append(1))   # no check below may reach the engine
    good = np.zeros((4, 6), f32)
    good[:, 1] = 3
    for bad in (dict(n_samples=0), dict(n_gibbs_steps=0), dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.5, 0.9]), dict(n_temperatures=0),
                dict(lengths=0), dict(lengths=10), dict(lengths=2.5), dict(lengths=[3, 3, 3]), dict(lengths=[[3, 3], [3, 3]]),
                dict(V_init=good[:3]), dict(V_init=good[:, :5]), dict(V_init=2 * good), dict(V_init=good - 4), dict(V_init=good + 0.5)):
        with pytest.raises(ValueError):
            m.sample_v_tempered(**dict(dict(n_samples=4, lengths=3, n_gibbs_steps=2), **bad))
    # set_count_tempering
    for bad in (dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.5, 0.9]), dict(n_temperatures=0), dict(n_chains=4), dict(chain_lengths=[3, 3]),
                dict(chain_lengths=3), dict(chain_lengths=[1, 2, 3, 4, 10]), dict(chain_lengths=[1, 2, 3, 4, 0])):
        with pytest.raises(ValueError):
            m.set_count_tempering(**bad)
        assert m._neg_phase is None
    assert m.set_count_tempering(n_temperatures=4) is m
    betas, n_chains = m._neg_phase
    assert np.array_equal(f32(betas), np.linspace(0., 1., 5)[1:].astype(f32)) and n_chains == 5
    with pytest.raises(RuntimeError, match='no chain lengths'):
        m._train_chain_lengths()
    m._fit_lengths = np.array([2, 7, 4])
    assert m._train_chain_lengths() == (2, 7, 4, 2, 7)                     # the first n_chains rows' lengths, cycled
    m.set_count_tempering(betas=[0.25, 1.0], n_chains=6, chain_lengths=[1, 2, 3, 4, 5, 9])
    assert m._neg_phase == ((0.25, 1.0), 6) and m._train_chain_lengths() == (1, 2, 3, 4, 5, 9)
    assert not any('neg' in k or 'temper' in k or 'chain' in k for k in m.get_params())
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        m.tempering_stats()
    m.set_params(batch_size=12)
    with pytest.raises(ValueError, match='n_chains'):
        m._check_tempered_fit()
    m.set_params(batch_size=5)
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(ValueError, match='BM355_DATA_PARALLEL'):
        m.set_count_tempering()
    monkeypatch.delenv('BM355_DATA_PARALLEL')
    assert m.set_count_tempering(False)._neg_phase is None
    # the Bernoulli entry stays refused for this unit, and 'cd' stays accepted
    with pytest.raises(ValueError, match='the tempered sweep has no count sampler'):
        m.set_negative_phase('tempered')
    assert m.set_negative_phase('cd') is m and m._neg_phase is None
    assert not made
