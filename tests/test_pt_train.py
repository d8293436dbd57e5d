"""The tempered negative phase, checked on the CPU twin alone (tests/pt_train_twin.py) and, for the public
refusals, on the Python layer without a device.  The twin is the reference of the GPU tests (test_pt_train_gpu.py)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import pt_train_twin as P
from tests import pt_twin as T
from tests.clamp_twin import SITE_H, SITE_V, act2
from tests.test_pt import _two_mode_model

SEED = 20241018


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _params(V, H):
    return dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H), vb=orc.normal(SEED, 2, 0, V) * np.float32(0.5),
                hb=orc.normal(SEED, 3, 0, H) * np.float32(0.5))


def _batch(B, V):
    return (orc.uniform(SEED, 6, 0, B * V) < 0.4).astype(np.float32).reshape(B, V)


def test_zero_learning_rate_is_a_sweep():
    """lr = 0: W, vb, hb stay where they are bit for bit (their increments are lr * (...) = 0) and the ensemble is the one two
    plain `Ensemble.sweep` calls of the same k, calls and seed leave - re-scoring included"""
    V, H, R, M, B, k = 37, 29, 5, 9, 7, 2
    p = _params(V, H)
    betas = np.linspace(0., 1., R + 1)[1:].astype(np.float32)
    t = P.TemperedRBM(p, M, betas, SEED, l2=1e-3)
    for _ in range(2):
        t.train_step(_batch(B, V), 0.0, 0.9, k)
    e = T.Ensemble(p, M, betas, seed=SEED)
    e.sweep(k, call=0)
    e.sweep(k, call=1)
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(t.p[n]), bits(p[n])), n
    assert np.array_equal(bits(t.ens.v), bits(e.v)) and np.array_equal(bits(t.ens.h), bits(e.h))
    assert np.array_equal(t.ens.idx, e.idx) and np.array_equal(t.ens.cnt, e.cnt) and t.ens.step == e.step == 2 * k
    assert np.array_equal(bits(t.ens.part_v), bits(e.part_v))
    assert t.call == 2 and 0 < e.cnt[1].sum() < e.cnt[0].sum()


def test_rescore_with_unchanged_vb_is_the_identity():
    """after the start and after a sweep (partials left by the prop-down); with another vb it is not"""
    V, H, R, M = 37, 29, 5, 9
    p = _params(V, H)
    e = P.TrainEnsemble(p, M, np.linspace(0., 1., R + 1)[1:].astype(np.float32), seed=SEED)
    for sweep in (0, 3):
        if sweep:
            e.sweep(sweep)
        before = e.part_v.copy()
        e.rescore()
        assert np.array_equal(bits(e.part_v), bits(before))
    e.set_params(dict(p, vb=p['vb'] + np.float32(0.25)))
    e.rescore()
    assert not np.array_equal(bits(e.part_v), bits(before))


def test_tempered_negative_statistic_is_unbiased_where_cd1_is_not():
    """6 x 4 RBM with two well-separated modes (test_pt._two_mode_model: v = h = 0 and v = h = 1, the second the heavier).  The
    negative statistic of the update, S_ij = mean_c v_ci hbar_cj over the M = 4096 beta = 1 rows (hbar = E[h | v]), against
    E[v_i h_j] by enumeration (0.7084 in every entry).
    Bound, entry by entry: 5 binomial standard deviations, 5 sqrt(E (1 - E) / M) = 0.0355 - v_i hbar_j lies in [0, 1], so its
    variance is at most that of a Bernoulli variable of the same mean, and the chains are independent.
    Tempered leg: R = 6 (betas 1/6 .. 1), random start, 100 steps of burn-in (the hot replicas cross between the modes within
    a few steps; a state needs of the order of R^2 = 36 swap steps to diffuse down the ladder).  Observed: max |S - E| = 0.0120
    (0.34 bounds).
    CD-1 leg: the same number of chains started at the mode v = 0, one step h ~ p(h|v), v ~ p(v|h) - where CD starts when the
    data sit in that mode.  Observed: S = 6e-6 in every entry, 19.9 bounds off: no chain leaves its mode."""
    V, H, M, R = 6, 4, 4096, 6
    p = _two_mode_model()
    exact = P.exact_vh(p['W'], p['vb'], p['hb'])
    bound = 5.0 * np.sqrt(exact * (1.0 - exact) / M)

    def statistic(v):
        return v.T.astype(np.float64).dot(P.hidden_means(p, v).astype(np.float64)) / M
    e = P.TrainEnsemble(p, M, np.linspace(0., 1., R + 1)[1:].astype(np.float32), seed=SEED)
    e.sweep(100)
    tempered = statistic(e.read()[0])
    _, h = act2(np.zeros((M, V), np.float32), p['W'], None, None, p['hb'], None, 1.0, 0, 1, SEED, SITE_H, 0, 0)
    _, v = act2(h, np.ascontiguousarray(p['W'].T), None, None, p['vb'], None, 1.0, 0, 1, SEED, SITE_V, 0, 0)
    cd1 = statistic(v)
    print('exact %.4f, bound %.4f, tempered max dev %.4f, CD-1 min dev %.4f' % (exact.max(), bound.max(), np.max(np.abs(tempered - exact)),
                                                                               np.min(np.abs(cd1 - exact))))
    assert np.all(np.abs(exact - 0.7084) < 1e-4)
    assert np.all(np.abs(tempered - exact) <= bound)
    assert np.all(np.abs(cd1 - exact) > bound)


def test_twin_update_moves_towards_the_tempered_statistic():
    """one update of the twin is the oracle's CD update with the ensemble's beta = 1 rows in place of the chain's: restated here
    in NumPy float64 for a batch shorter than the ensemble, momentum 0, no l2 (the slice [0, B) and the sign are what could go
    wrong)"""
    V, H, R, M, B = 16, 16, 3, 9, 5
    p = _params(V, H)
    betas = np.linspace(0., 1., R + 1)[1:].astype(np.float32)
    X = _batch(B, V)
    t = P.TemperedRBM(p, M, betas, SEED, l2=0.0)
    t.train_step(X, 0.1, 0.0, 1)
    e = T.Ensemble(p, M, betas, seed=SEED)
    e.sweep(1, call=0)
    vs = e.read()[0][:B]
    pos, neg = X.T.dot(P.hidden_means(p, X)), vs.T.dot(P.hidden_means(p, vs))
    want = p['W'].astype(np.float64) + 0.1 * (pos.astype(np.float64) - neg) / B
    assert np.max(np.abs(t.p['W'] - want)) < 1e-5
    assert np.max(np.abs(t.p['vb'] - (p['vb'] + 0.1 * (X.sum(0) - vs.sum(0)) / B))) < 1e-5


# ------------------------------------------------------------------------------------------------ no device needed
def test_abi_surface():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
    from boltzmann_machines_amd import BernoulliRBM
    assert [len(_ffi.SIGNATURES[n]) for n in ('bm_rbm_train_step_pt', 'bm_rbm_train_epoch_pt')] == [6, 7]
    assert all(callable(getattr(RbmEngine, n, None)) for n in ('train_step_pt', 'train_epoch_pt'))
    assert not hasattr(RbmEngine64, 'train_step_pt')
    assert callable(getattr(BernoulliRBM, 'set_negative_phase', None)) and callable(getattr(BernoulliRBM, 'tempering_stats', None))


def test_public_refusals_without_a_device(tmp_path, monkeypatch):
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM, MultinomialRBM
    monkeypatch.delenv('BM355_DATA_PARALLEL', raising=False)
    kw = dict(n_visible=12, n_hidden=8, batch_size=5, verbose=False, model_path=str(tmp_path / 'm') + '/')
    for model, word in ((GaussianRBM(**kw), 'Gaussian'), (MultinomialRBM(n_samples=3, **kw), 'Multinomial'),
                        (BernoulliRBM(dtype='float64', **kw), 'float64'), (BernoulliRBM(dbm_first=True, **kw), 'dbm_first'),
                        (BernoulliRBM(dbm_last=True, **kw), 'dbm_first'), (BernoulliRBM(dropout=0.9, **kw), 'dropout')):
        with pytest.raises(NotImplementedError, match=word):
            model.set_negative_phase('tempered')
        assert model.set_negative_phase('cd') is model            # the default is always there
    r = BernoulliRBM(**kw)
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(NotImplementedError, match='BM355_DATA_PARALLEL'):
        r.set_negative_phase('tempered')
    monkeypatch.delenv('BM355_DATA_PARALLEL')
    for bad in (dict(kind='pcd'), dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.5, 0.9]), dict(n_temperatures=0), dict(n_chains=4)):
        with pytest.raises(ValueError):
            r.set_negative_phase(**dict(dict(kind='tempered'), **bad))
    assert r._neg_phase is None
    assert r.set_negative_phase('tempered', n_temperatures=4) is r
    betas, n_chains = r._neg_phase
    assert np.array_equal(np.float32(betas), np.linspace(0., 1., 5)[1:].astype(np.float32)) and n_chains == 5
    assert r.set_negative_phase('tempered', betas=[0.25, 1.0], n_chains=9)._neg_phase == ((0.25, 1.0), 9)
    # the setting is no parameter: params.json keeps the reference's schema
    assert not any('neg' in k or 'temper' in k for k in r.get_params())
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        r.tempering_stats()
    assert r.set_negative_phase('cd')._neg_phase is None
