"""-m gpu: AIS log Z of a Bernoulli RBM and its exact log-likelihood (RbmEngine.ais / free_energy_rows,
BernoulliRBM.log_Z / log_proba) - chain-by-chain parity with the float64 NumPy twin (tests/np_reference_rbm_ais.py),
ground truth by enumeration, determinism and the slice property, the full 784 x 1024 shape, and the public API.

The chain-by-chain cases are the twin module's CHAIN_CASES / FULL_CASE: tests/test_rbm_ais.py shows that the twin meets no
near-tie in any of them, so no chain is excluded from a comparison here."""
import numpy as np
import pytest

from boltzmann_machines_amd.utils import philox
from tests import np_reference_rbm_ais as ra

pytestmark = pytest.mark.gpu

RTOL = 1e-5            # the project's parity bar


def make_engine(P, max_batch=10, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = P['W'].shape
    kw.setdefault('sample_v_states', True)
    eng = RbmEngine(V, H, max_batch=max_batch, **kw)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, P[n])
    return eng


def assert_chains(got, case_values, ties):
    """every chain without a recorded near-tie at rtol 1e-5; at most a quarter may be excluded (the chosen inputs: none)"""
    keep = ties == 0
    assert np.sum(~keep) * 4 <= len(keep), ties
    for j in np.flatnonzero(keep):
        print('chain %d: engine %.9g twin %.9g rel %.2e' % (j, got[j], case_values[j], abs(got[j] - case_values[j]) / abs(case_values[j])))
    np.testing.assert_allclose(got[keep], case_values[keep], rtol=RTOL)


def bracket(values, exact):
    est, sem = ra.sem_of(values)
    print('estimate %.6f exact %.6f sem %.4g' % (est, exact, sem))
    assert abs(est - exact) < max(0.02, 4 * sem), (est, exact, sem)


@pytest.mark.parametrize('case', ra.CHAIN_CASES, ids=lambda c: '%dx%d-k%d-%s' % (c[0], c[1], c[6], c[9]))
def test_ais_chain_by_chain(gpu_lib, case):
    V, H, pseed, std, n_betas, n_runs, k, seed, chain0, base = case
    assert chain0 != 0 and n_runs % 16 != 0
    P = ra.make_params(V, H, std=std, seed=pseed)
    a = ra.base_of(base, V)
    want, ties = ra.ais(P, n_betas, n_runs, k, seed, chain0, a)
    # (n_runs > max_batch: the chain workspaces are the run's own)
    eng = make_engine(P, max_batch=4)
    got = eng.ais(n_betas, n_runs, k, seed, chain0=chain0, base_bias=a)
    assert_chains(got, want, ties)
    eng.close()
    # sample_v_states = False, sample_h_states = False: AIS samples both layers whatever the flags say
    eng = make_engine(P, sample_v_states=False, sample_h_states=False)
    flagged = eng.ais(n_betas, n_runs, k, seed, chain0=chain0, base_bias=a)
    assert np.array_equal(flagged.view(np.uint32), got.view(np.uint32))
    eng.close()


@pytest.mark.parametrize('shape', [(20, 12), (33, 17), (784, 1024)])
def test_free_energy_rows(gpu_lib, shape):
    from boltzmann_machines_amd.engine import as_device
    V, H = shape
    P = ra.make_params(V, H, std=0.1, seed=4)
    N, B = 45, 10
    X = ra.data(N, V, 3)
    eng = make_engine(P, max_batch=B)        # no dropout
    Xd = as_device(X)
    got = eng.free_energy_rows(Xd, N)        # more rows than max_batch
    np.testing.assert_allclose(got, ra.free_energy_rows(P, X), rtol=RTOL)
    part = eng.free_energy_rows(Xd, 7, row=13)
    assert np.array_equal(part.view(np.uint32), got[13:20].view(np.uint32))
    for start in (0, 10, 40):
        n = min(B, N - start)
        mean = eng.free_energy(Xd, n, row=start)
        np.testing.assert_allclose(np.mean(got[start:start + n].astype(np.float64)), mean, rtol=RTOL)
    eng.close()


def _model_samples(P, n, sweeps=200, seed=5):
    """approximate samples of the model (NumPy block Gibbs): the data a base-rate reference is computed from"""
    rng = np.random.RandomState(seed)
    W, vb, hb = (np.asarray(P[k], dtype=np.float64) for k in ('W', 'vb', 'hb'))
    v = (rng.rand(n, W.shape[0]) < 0.5).astype(np.float64)
    for _ in range(sweeps):
        h = (rng.rand(n, W.shape[1]) < ra.sigmoid(v.dot(W) + hb)).astype(np.float64)
        v = (rng.rand(n, W.shape[0]) < ra.sigmoid(h.dot(W.T) + vb)).astype(np.float64)
    return v.astype(np.float32)


def test_ground_truth(gpu_lib, tmp_path):
    """the 10 x 8 model with weights N(0, 0.5^2): AIS (5000 betas, 512 chains) brackets the enumerated log Z under the uniform
    base and under the base rates of samples of the model; log_proba with the exact log Z is the exact log p"""
    from boltzmann_machines_amd import BernoulliRBM
    P = ra.make_params(10, 8, std=0.5, seed=7)
    exact = ra.exact_log_Z(P)
    eng = make_engine(P)
    bracket(eng.ais(5000, 512, 1, 777), exact)
    bracket(eng.ais(5000, 512, 1, 778, base_bias=ra.base_rate_bias(_model_samples(P, 500))), exact)
    eng.close()
    m = BernoulliRBM(n_visible=10, n_hidden=8, W_init=P['W'], vb_init=P['vb'], hb_init=P['hb'], batch_size=7, verbose=False,
                     random_seed=1, model_path=str(tmp_path / 'gt') + '/')
    m.init()
    X = ra.data(30, 10, 5, p=0.4)
    lp = m.log_proba(X, exact)
    want = ra.exact_log_p(P, X)
    print('max |log_proba - exact log p| = %.3g' % np.max(np.abs(lp - want)))
    np.testing.assert_allclose(lp, want, rtol=0, atol=1e-4)


def test_determinism_slices_and_fast_binary(gpu_lib):
    P = ra.make_params(20, 12, std=0.3)
    a = ra.base_of('vector', 20)
    eng = make_engine(P)
    r1 = eng.ais(30, 300, 1, 11, base_bias=a)
    r2 = eng.ais(30, 300, 1, 11, base_bias=a)
    assert np.all(np.isfinite(r1))
    assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32))
    c = eng.ais(30, 100, 1, 11, chain0=150, base_bias=a)
    assert np.array_equal(c.view(np.uint32), r1[150:250].view(np.uint32))
    eng.set_fast_binary(True, everywhere=True)
    fast = eng.ais(30, 300, 1, 11, base_bias=a)
    assert np.array_equal(fast.view(np.uint32), r1.view(np.uint32))
    eng.close()


# ---- the full shape: 784 x 1024, weights N(0, 0.1^2)
def test_full_shape_chain_by_chain(gpu_lib):
    V, H, pseed, std, n_betas, n_runs, k, seed, chain0, base = ra.FULL_CASE
    assert (V, H) == (784, 1024) and chain0 >= 1000
    P = ra.make_params(V, H, std=std, seed=pseed)
    a = ra.base_of(base, V)
    want, ties = ra.ais(P, n_betas, n_runs, k, seed, chain0, a)
    eng = make_engine(P)
    assert_chains(eng.ais(n_betas, n_runs, k, seed, chain0=chain0, base_bias=a), want, ties)
    eng.close()


def test_full_shape_long_run_against_twin(gpu_lib):
    """1000 betas x 64 chains: over 10^8 draws a float64 twin cannot be held chain by chain (forks at near-ties are expected);
    the two 64-chain estimates agree within 4 combined standard errors"""
    V, H, pseed, std = ra.FULL_CASE[:4]
    P = ra.make_params(V, H, std=std, seed=pseed)
    a = ra.base_of('data', V)
    eng = make_engine(P)
    g1 = eng.ais(1000, 64, 1, 4243, base_bias=a)
    g2 = eng.ais(1000, 64, 1, 4243, base_bias=a)
    eng.close()
    assert np.all(np.isfinite(g1))
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    want, ties = ra.ais(P, 1000, 64, 1, 4243, 0, a)
    est_g, sem_g = ra.sem_of(g1)
    est_t, sem_t = ra.sem_of(want)
    print('engine %.6f (sem %.4g) twin %.6f (sem %.4g), %d near-ties in the twin, %d chains equal at 1e-5'
          % (est_g, sem_g, est_t, sem_t, ties.sum(), np.sum(np.isclose(g1, want, rtol=RTOL, atol=0))))
    assert abs(est_g - est_t) < 4 * np.sqrt(sem_g ** 2 + sem_t ** 2), (est_g, sem_g, est_t, sem_t)


def test_full_shape_many_chains_slices(gpu_lib):
    P = ra.make_params(784, 1024, std=0.1, seed=5)
    eng = make_engine(P)
    big = eng.ais(4, 20000, 1, 606)
    assert np.all(np.isfinite(big))
    for c0, n in ((7000, 100), (19667, 333)):
        w = eng.ais(4, n, 1, 606, chain0=c0)
        assert np.array_equal(w.view(np.uint32), big[c0:c0 + n].view(np.uint32)), (c0, n)
    eng.close()


# ---- the public API
AV, AH, AN, BS = 16, 12, 20, 10
AX = (philox.uniform(2468, 200, 0, AN * AV) < 0.3).astype(np.float32).reshape(AN, AV)


def test_public_api(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM
    m = BernoulliRBM(n_visible=AV, n_hidden=AH, max_epoch=1, batch_size=BS, random_seed=11, verbose=False,
                     model_path=str(tmp_path / 'api') + '/').fit(AX)
    params = m.get_tf_params(scope='weights')
    state = m._rng.get_state()
    H0 = m.transform(AX)

    m._rng.set_state(state)
    lz, (lo, hi), vals = m.log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1)
    assert vals.shape == (32,) and np.all(np.isfinite(vals))
    assert np.isfinite(lz) and lo <= lz <= hi
    assert abs(lz - (AV + AH) * np.log(2)) < 10.0                        # small weights: near the uniform value
    lzb, (lob, hib), valsb = m.log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1, X_base=AX)
    assert np.all(np.isfinite(valsb)) and lob <= lzb <= hib and abs(lzb - lz) < 1.0
    lzv = m.log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1, X_base=ra.base_rate_bias(AX))[0]
    assert abs(lzv - lz) < 1.0
    before = m._rng.get_state()
    lp = m.log_proba(AX, lz)
    assert lp.shape == (AN,) and np.all(np.isfinite(lp)) and np.all(lp < 0)
    assert m._rng.get_state() == before                                  # log_proba draws nothing
    after = m.get_tf_params(scope='weights')
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(after[n].view(np.uint32), params[n].view(np.uint32)), n
    m._rng.set_state(state)
    H1 = m.transform(AX)                                                 # the same host seed stream: the same bits
    assert np.array_equal(H1.view(np.uint32), H0.view(np.uint32))

    m2 = BernoulliRBM.load_model(m._model_dirpath)
    lp2 = m2.log_proba(AX, lz)
    assert np.array_equal(lp2, lp)
    lz2 = m2.log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1)[0]
    assert abs(lz2 - lz) < 1.0


def test_refusals(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM, MultinomialRBM, _ffi
    from boltzmann_machines_amd.engine import RbmEngine, as_device
    kw = dict(n_visible=AV, n_hidden=AH, max_epoch=1, batch_size=BS, random_seed=3, verbose=False)
    for tag, cls, extra, word in (('g', GaussianRBM, {}, 'Gaussian'), ('m', MultinomialRBM, dict(n_samples=5), 'Multinomial'),
                                  ('d', BernoulliRBM, dict(dtype='float64'), 'float64'),
                                  ('f', BernoulliRBM, dict(dbm_first=True), 'dbm_first'),
                                  ('l', BernoulliRBM, dict(dbm_last=True), 'dbm_last')):
        m = cls(model_path=str(tmp_path / tag) + '/', **dict(kw, **extra)).fit(AX)
        with pytest.raises(NotImplementedError, match=word):
            m.log_Z(n_betas=5, n_runs=4)
        with pytest.raises(NotImplementedError, match=word):
            m.log_proba(AX, 0.)
    # ... and the library itself refuses the handles
    Xd = as_device(AX)
    for ekw, word in ((dict(v_unit=_ffi.UNIT_GAUSSIAN), 'Gaussian'), (dict(h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=5), 'Multinomial'),
                      (dict(dbm_first=True), 'dbm_first'), (dict(dbm_last=True), 'dbm_first')):
        eng = RbmEngine(AV, AH, **ekw)
        with pytest.raises(_ffi.Bm355Error, match=word):
            eng.ais(5, 4, 1, 1)
        with pytest.raises(_ffi.Bm355Error, match=word):
            eng.free_energy_rows(Xd, 4)
        eng.close()
    eng = RbmEngine(AV, AH)
    with pytest.raises(_ffi.Bm355Error, match='bad AIS arguments'):
        eng.ais(1, 4, 1, 1)
    eng.close()
