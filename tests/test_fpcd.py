"""Fast-weights PCD, checked on the CPU twin alone (tests/fpcd_twin.py) and, for the ABI surface and the public
refusals, on the Python layer without a device.  The twin is the reference of the GPU tests (test_fpcd_gpu.py)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import fpcd_twin as F
from tests import pt_train_twin as P
from tests.test_pt import _two_mode_model

SEED = 20250307
STATE = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means', 'ens_v', 'ens_h', 'idx', 'swaps')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _params(V, H):
    return dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H) * np.float32(0.5), vb=orc.normal(SEED, 2, 0, V) * np.float32(0.3),
                hb=orc.normal(SEED, 3, 0, H) * np.float32(0.3))


def _batch(n, V):
    return (orc.uniform(SEED, 6, 0, n * V) < 0.4).astype(np.float32).reshape(n, V)


def _ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(np.float32)


V, H, R, M, B, K = 37, 29, 3, 9, 7, 2
CFG = dict(l2=1e-3, sparsity_cost=0.1, sparsity_target=0.2)


def test_rate_zero_is_the_plain_tempered_update():
    """fast_learning_rate = 0: three updates equal TemperedRBM bit for bit - parameters, momentum, q_means, ensemble, ladder
    indices, swap counters - and the fast set stays all zero"""
    X = _batch(3 * B, V)
    plain = P.TemperedRBM(_params(V, H), M, _ladder(R), SEED, **CFG)
    fast = F.FastTemperedRBM(_params(V, H), M, _ladder(R), SEED, fast_learning_rate=0.0, fast_decay=0.95, **CFG)
    for u in range(3):
        plain.train_step(X[u * B:(u + 1) * B], 0.05, 0.9, K)
        fast.train_step(X[u * B:(u + 1) * B], 0.05, 0.9, K)
        a, b = plain.state(), fast.state()
        for n in STATE:
            assert np.array_equal(a[n].view(np.uint32) if a[n].dtype == np.float32 else a[n],
                                  b[n].view(np.uint32) if b[n].dtype == np.float32 else b[n]), (u, n)
        assert all(not np.any(fast.fast[n]) for n in F.NAMES)
    assert 0 < plain.ens.cnt[1].sum() < plain.ens.cnt[0].sum()


def test_first_update_with_a_positive_rate():
    """while the fast set is zero the effective set is the regular one: the first update's regular parameters are the plain
    twin's, W_fast = float32(rate) * float32(raw / B) element for element; from the second update on the ensembles differ"""
    X = _batch(2 * B, V)
    rate = 0.25
    plain = P.TemperedRBM(_params(V, H), M, _ladder(R), SEED, **CFG)
    fast = F.FastTemperedRBM(_params(V, H), M, _ladder(R), SEED, fast_learning_rate=rate, fast_decay=0.95, **CFG)
    plain.train_step(X[:B], 0.05, 0.9, K)
    fast.train_step(X[:B], 0.05, 0.9, K)
    a, b = plain.state(), fast.state()
    for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means', 'ens_v', 'ens_h'):
        assert same(a[n], b[n]), n
    raw = fast.last['raw']
    g0 = (raw[:V * H].reshape(V, H) / np.float32(B)).astype(np.float32)
    assert same(fast.fast['W'], np.float32(rate) * g0) and np.any(fast.fast['W'])
    assert same(fast.fast['vb'], np.float32(rate) * (raw[V * H:V * H + V] / np.float32(B)))
    assert same(b['W_eff'], b['W'] + fast.fast['W']) and not same(b['W_eff'], b['W'])
    plain.train_step(X[B:], 0.05, 0.9, K)
    fast.train_step(X[B:], 0.05, 0.9, K)
    assert not same(plain.ens.v, fast.ens.v)
    assert not same(plain.p['W'], fast.p['W'])


def _sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-z))


def test_the_negative_phase_reads_the_effective_set():
    """third update, its negative statistic v-^T E[h|v-] / B restated in float64 NumPy from (W_eff, hb_eff) and from (W, hb):
    the twin's raw sums (positive statistic in float64 from its own h0 means, minus the raw sums) agree with the first to 1e-5
    relative - the project's parity bound - and differ from the second by more than 100 times that (rate 0.5: after two updates
    the fast weights are of the order of 0.05)"""
    X = _batch(3 * B, V)
    t = F.FastTemperedRBM(_params(V, H), M, _ladder(R), SEED, fast_learning_rate=0.5, fast_decay=0.95, l2=1e-3)
    for u in range(2):
        t.train_step(X[u * B:(u + 1) * B], 0.05, 0.9, K)
    reg = {n: t.p[n].astype(np.float64) for n in F.NAMES}
    t.train_step(X[2 * B:], 0.05, 0.9, K)
    L = t.last
    vs, eff = L['vs'].astype(np.float64), {n: L['eff'][n].astype(np.float64) for n in F.NAMES}
    twin = (L['X'].astype(np.float64).T.dot(L['h0m'].astype(np.float64)) - L['raw'][:V * H].reshape(V, H).astype(np.float64)) / B
    from_eff = vs.T.dot(_sigmoid64(vs.dot(eff['W']) + eff['hb'])) / B
    from_reg = vs.T.dot(_sigmoid64(vs.dot(reg['W']) + reg['hb'])) / B
    rel = lambda a, b: np.max(np.abs(a - b)) / np.max(np.abs(b))
    print('relative distance of the twin: to the effective set %.3g, to the regular set %.3g' % (rel(twin, from_eff), rel(twin, from_reg)))
    assert rel(twin, from_eff) <= 1e-5
    assert rel(twin, from_reg) > 1e-3
    # the positive phase reads the regular set: the h0 means are those of (W, hb)
    h0 = _sigmoid64(L['X'].astype(np.float64).dot(reg['W']) + reg['hb'])
    assert np.max(np.abs(L['h0m'] - h0)) <= 1e-5 < np.max(np.abs(h0 - _sigmoid64(L['X'].astype(np.float64).dot(eff['W']) + eff['hb'])))


def _hop(rate):
    p = _two_mode_model()
    Vm, Hm = p['W'].shape
    Mh, Bh = 512, 64
    t = F.FastTemperedRBM(p, Mh, _ladder(1), SEED, fast_learning_rate=rate, fast_decay=0.95)
    t.ens = P.TrainEnsemble(t.rbm.p, Mh, _ladder(1), seed=SEED, call=0, V0=np.zeros((Mh, Vm), np.float32))
    ones = (orc.uniform(SEED, 8, 0, 60 * Bh) < 0.7).astype(np.float32)
    X = np.repeat(ones[:, None], Vm, axis=1)
    for u in range(60):
        t.train_step(X[u * Bh:(u + 1) * Bh], 0.0, 0.0, 1)
    for n in F.NAMES:
        assert same(t.p[n], p[n]), n
    return float((t.ens.read()[0].sum(axis=1) >= 4).mean())


def test_fast_weights_push_the_chains_out_of_their_mode():
    """6 x 4 two-mode model (test_pt._two_mode_model), R = 1, 512 chains started in the light mode v = 0, data rows all ones
    with probability 0.7 else all zeros, batch 64, k = 1, learning_rate = 0 (W, vb, hb keep their bits), 60 updates.  Fraction of
    chains with sum(v) >= 4: at least 0.4 with fast_learning_rate = 0.3, fast_decay = 0.95; at most 0.02 with rate 0.
    A float64 probe gave 0.67 - 0.74 and 0.00; the twin gives 0.664 and 0.000."""
    with_fast, without = _hop(0.3), _hop(0.0)
    print('fraction in the other mode: %.3f with fast weights, %.3f without' % (with_fast, without))
    assert with_fast >= 0.4
    assert without <= 0.02


# ------------------------------------------------------------------------------------------------ no device needed
def test_abi_surface():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
    from boltzmann_machines_amd import BernoulliRBM
    assert len(_ffi.SIGNATURES['bm_rbm_set_fast_weights']) == 4
    assert callable(getattr(RbmEngine, 'set_fast_weights', None)) and not hasattr(RbmEngine64, 'set_fast_weights')
    assert callable(getattr(BernoulliRBM, 'fast_weights', None))


def test_public_refusals_without_a_device(tmp_path, monkeypatch):
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM, MultinomialRBM
    monkeypatch.delenv('BM355_DATA_PARALLEL', raising=False)
    kw = dict(n_visible=12, n_hidden=8, batch_size=5, verbose=False, model_path=str(tmp_path / 'm') + '/')
    fw = dict(fast_learning_rate=0.1)
    for model, word in ((GaussianRBM(**kw), 'Gaussian'), (MultinomialRBM(n_samples=3, **kw), 'Multinomial'),
                        (BernoulliRBM(dtype='float64', **kw), 'float64'), (BernoulliRBM(dbm_first=True, **kw), 'dbm_first'),
                        (BernoulliRBM(dropout=0.9, **kw), 'dropout')):
        with pytest.raises(NotImplementedError, match=word):
            model.set_negative_phase('tempered', n_temperatures=1, **fw)
        assert model._fast_weights is None
    r = BernoulliRBM(**kw)
    with pytest.raises(ValueError, match='tempered'):
        r.set_negative_phase('cd', **fw)
    with pytest.raises(ValueError, match='tempered'):
        r.set_negative_phase(**fw)
    for bad in (dict(fast_learning_rate=-0.1), dict(fast_learning_rate=float('nan')), dict(fast_learning_rate=float('inf')),
                dict(fast_learning_rate=0.1, fast_decay=1.0), dict(fast_learning_rate=0.1, fast_decay=-0.01),
                dict(fast_learning_rate=0.1, fast_decay=float('nan'))):
        with pytest.raises(ValueError, match='fast_'):
            r.set_negative_phase('tempered', n_temperatures=1, **bad)
    assert r._neg_phase is None and r._fast_weights is None
    with pytest.raises(RuntimeError, match='no fast weights'):
        r.fast_weights()
    assert r.set_negative_phase('tempered', n_temperatures=1, fast_learning_rate=0.3, fast_decay=0.9) is r
    assert r._neg_phase == ((1.0,), 5) and len(r._neg_phase) == 2            # still the 2-tuple
    assert r._fast_weights == (0.3, 0.9)
    with pytest.raises(RuntimeError, match='no fast weights'):               # nothing trained yet
        r.fast_weights()
    # centring and fast weights: refused whichever comes second
    with pytest.raises(NotImplementedError, match='fast weights'):
        r.set_centering(True)
    assert r.set_centering(False) is r
    assert r.set_negative_phase('tempered', n_temperatures=3)._fast_weights is None      # the defaults switch it off again
    r.set_centering(True)
    with pytest.raises(NotImplementedError, match='centering'):
        r.set_negative_phase('tempered', n_temperatures=3, **fw)
    assert r._fast_weights is None and r._neg_phase is not None
    assert r.set_negative_phase('tempered', n_temperatures=3, fast_learning_rate=0.0) is r     # rate 0 asks for nothing
    r.set_centering(False)
    r.set_negative_phase('tempered', n_temperatures=2, **fw)
    # the setting is no parameter: params.json keeps the reference's schema
    assert not any('fast' in k or 'neg' in k or 'temper' in k for k in r.get_params())
    assert r.set_negative_phase('cd')._fast_weights is None
