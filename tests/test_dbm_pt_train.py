"""The DBM's tempered negative phase, checked on the CPU twin alone (tests/dbm_pt_train_twin.py: the ensemble
of tests/dbm_pt_twin.py with moving parameters and the re-scoring, the oracle's own update).  The twin is the reference of the
GPU tests (test_dbm_pt_train_gpu.py), so it is itself checked here: an update with lr = 0 is a plain tempered sweep, the
re-scoring is an identity under unchanged biases, and the handed-over rows carry the exact negative statistics of a two-mode
model where single-temperature particles do not."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import dbm_pt_train_twin as P
from tests import dbm_pt_twin as T

SEED = 20241018


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _random_model(n, site0=1):
    return dict(W=[orc.normal(SEED, site0 + i, 0, n[i] * n[i + 1]).reshape(n[i], n[i + 1]) * np.float32(0.5) for i in range(len(n) - 1)],
                vb=orc.normal(SEED, site0 + 10, 0, n[0]) * np.float32(0.5),
                hb=[orc.normal(SEED, site0 + 11 + i, 0, n[i + 1]) * np.float32(0.5) for i in range(len(n) - 1)])


def _data(N, V, s=0):
    return (orc.uniform(SEED, 40 + s, 0, N * V) < 0.4).astype(np.float32).reshape(N, V)


@pytest.mark.parametrize('n', [(37, 20, 11), (37, 20)])
def test_update_with_zero_learning_rate_is_a_plain_sweep(n):
    """lr = 0, momentum, l2, sparsity and a finite max_norm on: after one train_step(k) the ensemble (all rows of all layers,
    temperatures, ladder indices, counters, partials) equals tests/dbm_pt_twin.Ensemble.sweep(k) from the same start, bit for
    bit; rescore() rewrites the bits that are there, before and after the update; vb and every hb keep their bits (d = lr * (..)
    = 0).  W is NOT compared: the max-norm pass rescales every column as (w * n) / n whatever max_norm is, which may move w in
    its last place even at lr = 0 - the reason the ensemble is compared after ONE update, whose sweeps precede it."""
    M, B, R, k = 5, 6, 3, 3
    p = _random_model(n)
    betas = np.linspace(0., 1., R + 1)[1:].astype(np.float32)
    L = len(n) - 1
    cfg = dict(max_mf_updates=5, mf_tol=1e-5, l2=1e-3, max_norm=1.5, sparsity_cost=[0.05, 0.02][:L], sparsity_target=[0.2, 0.1][:L])
    t = P.TemperedDBM(p, M, B, M + 2, betas, SEED, call=1, **cfg)
    plain = T.Ensemble(p, M + 2, betas, seed=SEED, call=1)
    e = t.ens
    pv, ph2 = e.part_v.copy(), e.part_h2.copy()
    e.rescore()
    assert same(pv, e.part_v) and same(ph2, e.part_h2)
    n_mf, msre = t.train_step(_data(B, n[0]), 0.0, 0.5, k, want_msre=True)
    assert 1 <= n_mf <= 5 and 0.0 < msre < 1.0 and t.call == 2
    plain.sweep(k, call=1)
    assert same(e.v, plain.v) and all(same(a, b) for a, b in zip(e.h, plain.h))
    assert same(e.mult, plain.mult) and np.array_equal(e.idx, plain.idx) and np.array_equal(e.cnt, plain.cnt)
    assert same(e.part_v, plain.part_v) and same(e.part_h1, plain.part_h1) and same(e.part_h2, plain.part_h2)
    assert e.margins == plain.margins and 0 < e.cnt[1].sum() < e.cnt[0].sum()
    pv, ph2 = e.part_v.copy(), e.part_h2.copy()
    e.set_params(t.params())
    e.rescore()
    assert same(pv, e.part_v) and same(ph2, e.part_h2)
    assert same(t.p['vb'], p['vb']) and all(same(t.p['hb' + P.sfx(i)], p['hb'][i]) for i in range(L))
    # the hand-over: the dense particles are the beta = 1 rows of the first M of the M + 2 chains
    v, H = e.read()
    assert same(t.p['v'], v[:M]) and all(same(t.p['h' + P.sfx(i)], H[i][:M]) for i in range(L))
    assert np.all(t.p['dvb'] == 0) and all(np.all(t.p['dW' + P.sfx(i)] == 0) for i in range(L))


def test_rescore_follows_moved_biases():
    """lr > 0: the update moves vb and b2, so the stored partials are stale until the next update's rescore() - which then
    equals the partials formed from scratch"""
    n, M, B, R = (37, 20, 11), 5, 6, 3
    t = P.TemperedDBM(_random_model(n), M, B, M, np.linspace(0., 1., R + 1)[1:].astype(np.float32), SEED, max_mf_updates=3)
    t.train_step(_data(B, n[0]), 0.05, 0.5, 2)
    e = t.ens
    stale_v, stale_h2 = e.part_v.copy(), e.part_h2.copy()
    e.set_params(t.params())
    e.rescore()
    assert not same(stale_v, e.part_v) and not same(stale_h2, e.part_h2)
    from tests.pt_twin import slot_partials
    assert same(e.part_v, slot_partials(e.v * t.p['vb'][None, :])) and same(e.part_h2, slot_partials(e.h[1] * t.p['hb_1'][None, :]))


MV, M1, M2 = 6, 4, 3
STEPS, CHAINS = 240, 512


def _two_mode_model():
    """tests/test_dbm_pt.py's, restated: all weights w = 3 in both layers, every bias minus half the weight that reaches the
    unit (vb = -w n1 / 2 + 0.15, b1 = -w (V + n2) / 2, b2 = -w n1 / 2): in +-1 spins a ferromagnet, the modes are all units 0
    and all units 1, the tilt 0.15 on vb makes the second one the heavier"""
    w = 3.0
    return dict(W=[np.full((MV, M1), w, np.float32), np.full((M1, M2), w, np.float32)],
                vb=np.full(MV, -w * M1 / 2 + 0.15, np.float32),
                hb=[np.full(M1, -w * (MV + M2) / 2, np.float32), np.full(M2, -w * M1 / 2, np.float32)])


def _negative_statistics(R):
    """(mean v_i h1_j [V][n1], mean h1_j h2_k [n1][n2]) over the dense particles ONE update with lr = 0 hands over: 512
    chains x R temperatures, all rows started in the mode v = h2 = 0, STEPS tempered steps under fixed parameters"""
    p = _two_mode_model()
    t = P.TemperedDBM(p, CHAINS, 4, CHAINS, np.linspace(0., 1., R + 1)[1:].astype(np.float32), SEED, max_mf_updates=1,
                      ens_kw=dict(V0_rows=np.zeros((CHAINS * R, MV), np.float32), H2_rows=np.zeros((CHAINS * R, M2), np.float32)))
    t.train_step(np.zeros((4, MV), np.float32), 0.0, 0.0, STEPS)
    v, h1, h2 = (t.p[k].astype(np.float64) for k in ('v', 'h', 'h_1'))
    assert v.shape == (CHAINS, MV) and h1.shape == (CHAINS, M1) and h2.shape == (CHAINS, M2)
    return v.T.dot(h1) / CHAINS, h1.T.dot(h2) / CHAINS


def test_handed_over_rows_carry_the_exact_negative_statistics():
    """Power.  6-4-3 two-mode DBM, 512 chains, all started in the mode v = h2 = 0, one update of 240 tempered steps with lr = 0
    (fixed parameters); the negative statistics mean(v_i h1_j) (24 entries) and mean(h1_j h2_k) (12 entries) over the
    handed-over rows against the enumerated expectations (exact_tempered_moments, float64).  Bound per entry: 5 binomial standard
    deviations of a mean of 512 independent Bernoulli(p) products, 5 sqrt(p (1 - p) / 512) - a condition, not a fit.
    Exact: E[v_i h1_j] and E[h1_j h2_k] lie in 0.7083 .. 0.7085 (the model is symmetric in the units of a layer); bound 0.1004.
    Observed on the twin: R = 6 (betas 1/6 .. 1): entries 0.6992 .. 0.7012, the worst at 0.090 of its bound; R = 1, the same
    call: every entry 0.0000, 7.06 times the bound away in ALL 36 entries - no particle has left its mode: the statistics a
    single-temperature PCD phase would feed the update."""
    p = _two_mode_model()
    Evh, Ehh = P.exact_tempered_moments(p['W'], p['vb'], p['hb'])
    exact = np.concatenate([Evh.ravel(), Ehh.ravel()])
    bound = 5.0 * np.sqrt(exact * (1.0 - exact) / CHAINS)
    got = {R: np.concatenate([a.ravel() for a in _negative_statistics(R)]) for R in (6, 1)}
    for R in (6, 1):
        print('R = %d: exact %.4f .. %.4f, bound %.4f .. %.4f, observed %.4f .. %.4f, worst |diff| / bound %.3f'
              % (R, exact.min(), exact.max(), bound.min(), bound.max(), got[R].min(), got[R].max(),
                 np.max(np.abs(got[R] - exact) / bound)))
    assert exact.size == 36 and np.all((exact > 0.5) & (exact < 0.9))
    assert np.all(np.abs(got[6] - exact) <= bound)
    assert np.any(np.abs(got[1] - exact) > bound)


def test_exact_moments_against_brute_force():
    """exact_tempered_moments on a random 3-3-2 model against the sum over all 2^8 joint states"""
    n = (3, 3, 2)
    p = _random_model(n, site0=50)
    W0, W1 = (np.asarray(w, np.float64) for w in p['W'])
    vb, b1, b2 = (np.asarray(b, np.float64) for b in (p['vb'], p['hb'][0], p['hb'][1]))
    Z, Evh, Ehh = 0.0, np.zeros((3, 3)), np.zeros((3, 2))
    for code in range(1 << 8):
        s = np.array([(code >> i) & 1 for i in range(8)], np.float64)
        v, h1, h2 = s[:3], s[3:6], s[6:]
        w = np.exp(v.dot(vb) + h1.dot(b1) + h2.dot(b2) + v.dot(W0).dot(h1) + h1.dot(W1).dot(h2))
        Z += w
        Evh += w * np.outer(v, h1)
        Ehh += w * np.outer(h1, h2)
    a, b = P.exact_tempered_moments(p['W'], p['vb'], p['hb'])
    np.testing.assert_allclose(a, Evh / Z, rtol=1e-12)
    np.testing.assert_allclose(b, Ehh / Z, rtol=1e-12)


def _bare_dbm(**kw):
    """a DBM that has no engine yet (the refusals come before one is built), its layer description filled in by hand"""
    from boltzmann_machines_amd import DBM
    d = DBM(rbms=None, n_particles=5, batch_size=5, **kw)
    d.n_layers_, d.n_visible_, d.n_hiddens_, d.h_units_ = 2, 12, [8, 6], [0, 0]
    return d


def test_refusals():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import DbmEngine64
    d = _bare_dbm()
    assert d.set_negative_phase('tempered', n_temperatures=3) is d
    assert d._neg_phase == ((np.float32(1 / 3.), np.float32(2 / 3.), 1.0), 5)
    assert d.set_negative_phase('tempered', betas=[0.25, 1.0], n_chains=9)._neg_phase == ((0.25, 1.0), 9)
    assert d.set_negative_phase('cd')._neg_phase is None
    with pytest.raises(ValueError, match='n_chains. must be >= n_particles'):
        d.set_negative_phase('tempered', n_chains=4)
    with pytest.raises(ValueError, match='betas'):
        d.set_negative_phase('tempered', betas=[0.5, 0.4, 1.0])
    with pytest.raises(ValueError, match='n_temperatures'):
        d.set_negative_phase('tempered', n_temperatures=0)
    with pytest.raises(ValueError, match='kind'):
        d.set_negative_phase('pcd')
    assert d._neg_phase is None
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        d.tempering_stats()
    d.n_layers_, d.n_hiddens_, d.h_units_ = 3, [8, 6, 4], [0, 0, 0]
    with pytest.raises(NotImplementedError, match='OLD layer above'):
        d.set_negative_phase('tempered')
    d = _bare_dbm()
    d.v_unit_ = _ffi.UNIT_GAUSSIAN
    with pytest.raises(NotImplementedError, match='Gaussian'):
        d.set_negative_phase('tempered')
    d = _bare_dbm()
    d.h_units_ = [0, _ffi.UNIT_MULTINOMIAL]
    with pytest.raises(NotImplementedError, match='Multinomial'):
        d.set_negative_phase('tempered')
    d = _bare_dbm()
    d.set_mean_field_arithmetic('reference')
    with pytest.raises(NotImplementedError, match='literal'):
        d.set_negative_phase('tempered')
    d = _bare_dbm()
    d._dp = object()
    with pytest.raises(NotImplementedError, match='data parallelism'):
        d.set_negative_phase('tempered')
    d = _bare_dbm(dtype='float64')
    with pytest.raises(NotImplementedError, match='float64'):
        d.set_negative_phase('tempered')
    with pytest.raises(NotImplementedError, match='float64'):
        DbmEngine64.train_step_pt(None, None, 0.1, 0.5, 1)
    # what changed behind set_negative_phase is refused when the fit starts
    d = _bare_dbm().set_negative_phase('tempered', n_temperatures=3)
    d.n_particles = 6
    with pytest.raises(ValueError, match='n_chains. must be >= n_particles'):
        d._check_tempered_fit()
    # the twin's own
    with pytest.raises(ValueError, match='fewer than n_particles'):
        P.TemperedDBM(_random_model((6, 5, 4)), 5, 4, 4, [1.0], SEED)
    with pytest.raises(NotImplementedError, match='OLD layer above'):
        P.TemperedDBM(_random_model((6, 5, 4, 3)), 2, 2, 2, [1.0], SEED)
    with pytest.raises(NotImplementedError, match='literal'):
        P.TemperedDBM(_random_model((6, 5, 4)), 2, 2, 2, [1.0], SEED, sigmoid_literal=True)


def test_no_swap_draw_of_the_gpu_fixtures_is_a_near_tie():
    """the seeds of the bit-for-bit GPU cases are such that no swap draw lies within 1e-9 of its threshold, and acceptance is
    neither 0 nor 1 (the full-size case: attempts only)"""
    from tests import test_dbm_pt_train_gpu as G
    for case in range(len(G.CASES)):
        G.decisive_twin(case)
    G.decisive_full()
    G.decisive_between_sweeps()
    G.decisive_public()


def test_abi_surface():
    from boltzmann_machines_amd import DBM, _ffi
    from boltzmann_machines_amd.engine import DbmEngine, DbmEngine64
    assert len(_ffi.SIGNATURES['bm_dbm_train_step_pt']) == 7 == len(_ffi.SIGNATURES['bm_dbm_train_step'])
    assert callable(getattr(DbmEngine, 'train_step_pt', None))
    with pytest.raises(NotImplementedError, match='float64'):
        DbmEngine64.train_step_pt(None)
    assert callable(getattr(DBM, 'set_negative_phase', None)) and callable(getattr(DBM, 'tempering_stats', None))
    header = open(_ffi.__file__.replace('boltzmann_machines_amd/_ffi.py', 'include/bm355.h')).read()
    decl = header[header.index('int bm_dbm_train_step_pt('):]
    decl = decl[:decl.index(';')]
    assert decl.count(',') + 1 == 7
    assert 'bm_dbm64_train_step_pt' not in header
