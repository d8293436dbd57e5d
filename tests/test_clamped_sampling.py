"""Conditional sampling, checked on the CPU twin alone (tests/clamp_twin.py: the clamped sweeps as a loop of the oracle's
activation stage with the blend on the host).  The twin is the reference of the GPU tests (test_clamped_sampling_gpu.py), so
it is itself checked here against the exact conditional of a model small enough to enumerate."""
import numpy as np

from oracle import oracle as orc
from tests import clamp_twin as T

V, H, ROWS, STEPS, SEED = 6, 4, 4096, 50, 20240611


def _model():
    W = orc.normal(SEED, 1, 0, V * H).reshape(V, H)                     # N(0, 1) weights
    vb = orc.normal(SEED, 2, 0, V) * np.float32(0.5)
    hb = orc.normal(SEED, 3, 0, H) * np.float32(0.5)
    return dict(W=W, vb=vb, hb=hb, sigma=np.ones(V, np.float32))


def test_marginals_match_the_exact_conditional():
    """6 x 4 Bernoulli RBM, 3 visibles clamped, 4096 independent rows x 50 sweeps: the empirical marginals of the 3 free
    visibles against p(v_i = 1 | v_observed) from the enumeration of all 2^3 2^4 (v_free, h).  Bound: 4 binomial standard
    errors of 4096 draws, 4 sqrt(p (1 - p) / 4096) <= 0.032."""
    p = _model()
    observed = np.array([1, 0, 1, 0, 0, 1], bool)
    x = np.array([1, 0, 0, 0, 0, 1], np.float32)
    free, exact = T.exact_conditional(p['W'], p['vb'], p['hb'], x, observed)
    assert free == [1, 3, 4]
    V0 = (orc.uniform(SEED, 4, 0, ROWS * V) < 0.5).astype(np.float32).reshape(ROWS, V)
    clamp = np.tile(x, (ROWS, 1))
    mask = np.tile(observed.astype(np.float32), (ROWS, 1))
    v, h, vm = T.rbm_gibbs_clamped(p, V0, clamp, mask, STEPS, seed=SEED)
    assert np.array_equal(v[:, observed], clamp[:, observed]) and np.array_equal(vm[:, observed], clamp[:, observed])
    emp = v[:, free].mean(axis=0)
    bound = 4.0 * np.sqrt(exact * (1.0 - exact) / ROWS)
    print('exact', exact, 'empirical', emp, 'bound', bound)
    assert np.all(bound <= 0.032)
    assert np.all(np.abs(emp - exact) <= bound)


def test_all_ones_mask_returns_x_and_all_zero_mask_is_the_plain_loop():
    p = _model()
    B = 37
    V0 = (orc.uniform(SEED, 5, 0, B * V) < 0.5).astype(np.float32).reshape(B, V)
    X = orc.uniform(SEED, 6, 0, B * V).reshape(B, V)                      # grey levels
    v, _, vm = T.rbm_gibbs_clamped(p, V0, X, np.ones((B, V), np.float32), 3, seed=SEED)
    assert np.array_equal(v.view(np.uint32), X.view(np.uint32)) and np.array_equal(vm.view(np.uint32), X.view(np.uint32))
    a = T.rbm_gibbs_clamped(p, V0, X, np.zeros((B, V), np.float32), 3, seed=SEED)
    b = T.rbm_gibbs_clamped(p, V0, None, None, 3, seed=SEED, clamped=False)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # and the plain loop is the oracle's own sampling sweep shifted by half a step: h of sweep 0 from V0, then OracleRBM.gibbs
    twin = orc.OracleRBM(V, H, sample_v_states=True, sample_h_states=True)
    for n in ('W', 'vb', 'hb'):
        twin.p[n][...] = p[n]
    twin.set_seed(SEED)
    _, h0 = T.act2(V0, p['W'], None, None, p['hb'], None, 1.0, 0, 1, SEED, T.SITE_H, 0, 0)
    _, v1 = twin.gibbs(h0, 1)
    c = T.rbm_gibbs_clamped(p, V0, None, None, 1, seed=SEED, clamped=False)
    assert np.array_equal(c[0].view(np.uint32), v1.view(np.uint32))
