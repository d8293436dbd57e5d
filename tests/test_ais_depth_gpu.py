"""-m gpu: AIS log Z and the ELBO of binary DBMs at depths 1, 3 and 4 (the odd-depth layers are the AIS chain, the
even-depth layers are summed out; tests/np_reference_depth.py) - chain-by-chain parity with the float64 NumPy
restatement, ground truth by enumeration, determinism and chain sharding, the accumulation modes, and the public
DBM API end to end."""
import numpy as np
import pytest

from boltzmann_machines_amd.utils import log_mean_exp, log_std_exp, philox
from tests import np_reference_depth as rd

pytestmark = pytest.mark.gpu


def make_pair(V, nh, N=10, M=10, std=0.1, seed=3, **kw):
    """a DbmEngine and its float64 NumPy twin with identical parameters"""
    from boltzmann_machines_amd.engine import DbmEngine
    eng = DbmEngine(V, nh, n_particles=M, batch_size=N, **kw)
    n = [V] + list(nh)
    P = {}
    for i in range(len(nh)):
        s = rd._sfx(i)
        W = (philox.normal(2468, seed + i, 0, n[i] * n[i + 1]) * np.float32(std)).reshape(n[i], n[i + 1])
        hb = (philox.uniform(2468, seed + 10 + i, 0, n[i + 1]) - np.float32(0.5)) * np.float32(0.4)
        eng.set('W' + s, W); eng.set('hb' + s, hb)
        P['W' + s], P['hb' + s] = W.astype(np.float64), hb.astype(np.float64)
        P['mu' + s] = np.zeros((N, n[i + 1]))
    vb = (philox.uniform(2468, seed + 30, 0, V) - np.float32(0.5)) * np.float32(0.4)
    eng.set('vb', vb)
    P['vb'] = vb.astype(np.float64)
    twin = rd.DepthDBM(P, len(nh), N, M, sample_v=kw.get('sample_v_states', True), sample_h=kw.get('sample_h_states'),
                       max_mf=kw.get('max_mf_updates', 10), mf_tol=kw.get('mf_tol', 1e-7))
    return eng, twin


def data(N, V, s):
    return (philox.uniform(2468, 99 + s, 0, N * V) < 0.25).astype(np.float32).reshape(N, V)


def bracket(vals, exact):
    vals = vals.astype(np.float64)
    est = log_mean_exp(vals)
    sem = np.exp(log_std_exp(vals) - est) / np.sqrt(len(vals))
    assert abs(est - exact) < max(0.02, 4 * sem), (est, exact, sem)


NH = {1: [12], 3: [12, 16, 10], 4: [12, 16, 10, 8]}


@pytest.mark.parametrize('L', [1, 3, 4])
@pytest.mark.parametrize('k', [1, 2])
def test_ais_and_log_proba_chain_by_chain(gpu_lib, L, k):
    from boltzmann_machines_amd.engine import as_device
    V, N = 20, 10
    eng, twin = make_pair(V, NH[L], N=N, max_mf_updates=8, mf_tol=1e-6)
    g = eng.ais(n_betas=25, n_runs=37, k=k, seed=2222, chain0=5)
    c = twin.ais(n_betas=25, n_runs=37, k=k, seed=2222, chain0=5)
    np.testing.assert_allclose(g, c, rtol=1e-5, err_msg='%d near-ties among the draws of the NumPy chains' % twin.ties)
    X = data(N, V, 2)
    np.testing.assert_allclose(eng.log_proba(as_device(X)), twin.log_proba(X), rtol=1e-5)
    eng.close()


@pytest.mark.parametrize('L', [1, 3])
def test_ais_with_unsampled_layers(gpu_lib, L):
    """sample_v_states=False and (L = 3) an unsampled hidden layer: those layers pass their means"""
    sh = [True] if L == 1 else [True, False, True]
    eng, twin = make_pair(20, NH[L], sample_v_states=False, sample_h_states=sh)
    g = eng.ais(n_betas=25, n_runs=37, k=2, seed=77, chain0=11)
    c = twin.ais(n_betas=25, n_runs=37, k=2, seed=77, chain0=11)
    np.testing.assert_allclose(g, c, rtol=1e-5, err_msg='%d near-ties among the draws of the NumPy chains' % twin.ties)
    eng.close()


GT = {1: (10, [8]), 3: (8, [6, 5, 4]), 4: (6, [5, 4, 4, 4])}      # (the engine: hidden layer i has more than i units)


@pytest.mark.parametrize('L', [1, 3, 4])
def test_ais_brackets_exact_log_Z_and_elbo_bounds(gpu_lib, L):
    """non-trivial small models (weights N(0, 0.5^2)): the AIS estimate (5000 betas, 512 chains) brackets the log Z
    enumerated over the odd-depth layers; the ELBO is exact at L = 1 and a lower bound at L = 3, 4"""
    from boltzmann_machines_amd.engine import as_device
    V, nh = GT[L]
    N = 16
    eng, twin = make_pair(V, nh, N=N, std=0.5, seed=7, max_mf_updates=30, mf_tol=1e-7)
    exact = rd.exact_log_Z(twin.P, L)
    bracket(eng.ais(n_betas=5000, n_runs=512, k=1, seed=777), exact)
    eng.log_proba(as_device(data(N, V, 4)))            # a different batch first: the mean-field loop starts from its mu
    X = data(N, V, 5)
    elbo = eng.log_proba(as_device(X)).astype(np.float64) - exact
    lp = rd.exact_log_p(twin.P, L, X)
    if L == 1:
        np.testing.assert_allclose(elbo, lp, rtol=0, atol=1e-4)
    else:
        assert np.all(elbo <= lp + 1e-4), elbo - lp
    eng.close()


def test_determinism_slices_and_sharded_direct_at_three_layers(gpu_lib):
    from boltzmann_machines_amd import parallel
    eng, _ = make_pair(20, NH[3], std=0.3)
    a = eng.ais(n_betas=30, n_runs=300, k=1, seed=11)
    b = eng.ais(n_betas=30, n_runs=300, k=1, seed=11)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = eng.ais(n_betas=30, n_runs=100, k=1, seed=11, chain0=150)
    assert np.array_equal(c.view(np.uint32), a[150:250].view(np.uint32))
    eng.close()
    # world 1 over the direct exchange, a registered buffer shorter than the number of chains: several windows
    eng, _ = make_pair(6, [4, 4, 4], N=2, M=2, std=0.3)
    xchg = parallel.DirectExchange(eng, 0, 1)
    n = eng.device_view('grad').shape[0]
    R = 2 * n + 5
    got = eng.ais_sharded_direct(xchg, 6, R, 1, 99)
    ref = eng.ais(6, R, 1, 99)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    xchg.close(); eng.close()


@pytest.mark.parametrize('L', [1, 3])
def test_accumulation_modes(gpu_lib, L):
    """literal float32 accumulation: the same chains, another sum (1e-5); fast-binary at depth != 2 runs the fp32 path
    (bm355.h): the default's values bit for bit"""
    eng, twin = make_pair(20, NH[L], std=0.3)
    d64 = eng.ais(n_betas=200, n_runs=64, k=1, seed=5, chain0=3)
    eng.set_ais_literal(True)
    lit = eng.ais(n_betas=200, n_runs=64, k=1, seed=5, chain0=3)
    np.testing.assert_allclose(lit, d64, rtol=1e-5)
    eng.set_ais_literal(False)
    eng.set_fast_binary(True)
    fast = eng.ais(n_betas=200, n_runs=64, k=1, seed=5, chain0=3)
    assert np.all(np.isfinite(fast))
    assert np.array_equal(fast.view(np.uint32), d64.view(np.uint32))
    eng.set_fast_binary(False)
    np.testing.assert_allclose(d64, twin.ais(n_betas=200, n_runs=64, k=1, seed=5, chain0=3), rtol=1e-5,
                               err_msg='%d near-ties among the draws of the NumPy chains' % twin.ties)
    eng.close()


# ---- the public API
AV, AN, BS = 16, 20, 10
AX = (philox.uniform(2468, 200, 0, AN * AV) < 0.3).astype(np.float32).reshape(AN, AV)


def _rbm(tmp, tag, nv, nh, X, seed, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    return BernoulliRBM(n_visible=nv, n_hidden=nh, max_epoch=1, batch_size=BS, random_seed=seed, verbose=False,
                        model_path=str(tmp / tag) + '/', **kw).fit(X)


def _dbm(tmp, tag, rbms, **kw):
    from boltzmann_machines_amd import DBM
    cfg = dict(rbms=rbms, n_particles=BS, n_gibbs_steps=2, max_mf_updates=5, mf_tol=1e-5, learning_rate=0.01, max_epoch=1,
               batch_size=BS, random_seed=1337, verbose=False, model_path=str(tmp / tag) + '/')
    cfg.update(kw)
    return DBM(**cfg)


def _check_log_Z_and_proba(d, n_units):
    lz, (lo, hi), vals = d.log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1)
    assert vals.shape == (32,) and np.all(np.isfinite(vals))
    assert np.isfinite(lz) and lo <= lz <= hi
    assert abs(lz - n_units * np.log(2)) < 10.0                          # small weights: near the uniform value
    lp = d.log_proba(AX, lz)
    assert lp.shape == (AN,) and np.all(np.isfinite(lp)) and np.all(lp < 0)
    return lz


def test_public_api_three_layers_and_one_layer(gpu_lib, tmp_path):
    from boltzmann_machines_amd import DBM
    r1 = _rbm(tmp_path, 'r1', AV, 12, AX, 11, dbm_first=True)
    Q1 = r1.transform(AX)
    r2 = _rbm(tmp_path, 'r2', 12, 10, Q1, 12)
    r3 = _rbm(tmp_path, 'r3', 10, 8, r2.transform(Q1), 13, dbm_last=True)
    d = _dbm(tmp_path, 'd3', [r1, r2, r3]).fit(AX)
    assert d.n_layers_ == 3
    lz = _check_log_Z_and_proba(d, AV + 12 + 10 + 8)
    d2 = DBM.load_model(d._model_dirpath)
    assert d2.n_layers_ == 3
    lz2 = _check_log_Z_and_proba(d2, AV + 12 + 10 + 8)
    assert abs(lz2 - lz) < 1.0
    # one layer: the DBM of one RBM (its own composition rule: the hidden bias is halved, see DBM.log_Z)
    r = _rbm(tmp_path, 'r0', AV, 12, AX, 21)
    d0 = _dbm(tmp_path, 'd0', [r])
    d0.init()
    np.testing.assert_allclose(d0.get_tf_params('weights')['hb'], 0.5 * r.get_tf_params('weights')['hb'])
    d1 = _dbm(tmp_path, 'd1', [r]).fit(AX)
    assert d1.n_layers_ == 1
    _check_log_Z_and_proba(d1, AV + 12)


def test_refusals_unchanged(gpu_lib, tmp_path):
    """float64 DBMs keep the 2-layer AIS / ELBO: a 3-layer float64 DBM builds and trains, and refuses both"""
    f64 = dict(dtype='float64')
    r1 = _rbm(tmp_path, 'f1', AV, 8, AX, 31, dbm_first=True, **f64)
    Q1 = r1.transform(AX)
    r2 = _rbm(tmp_path, 'f2', 8, 6, Q1, 32, **f64)
    r3 = _rbm(tmp_path, 'f3', 6, 4, r2.transform(Q1), 33, dbm_last=True, **f64)
    d = _dbm(tmp_path, 'f64', [r1, r2, r3], dtype='float64').fit(AX)
    assert np.all(np.isfinite(d.get_tf_params('weights')['W_2']))
    with pytest.raises(AssertionError):
        d.log_Z(n_betas=5, n_runs=4)
    with pytest.raises(AssertionError):
        d.log_proba(AX, 0.)
