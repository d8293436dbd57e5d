"""-m gpu: AIS log Z of softmax visible units and the log-likelihood of incomplete rows (RbmEngine.groups_ais,
CategoricalRBM.ais_log_Z / ais_log_Z_rows / log_proba) - chain-by-chain parity with the float64 NumPy twin
(tests/softmax_ais_twin.py) on both softmax routes, the routes and every tile geometry bit for bit, determinism, slices and what
a run leaves untouched, ground truth by enumeration, the full width, the public API and the refusals.

The chain-by-chain cases are the twin module's CHAIN_CASES / FULL_CASES: tests/test_softmax_ais.py shows that the twin meets no
near-tie in any of them, so no chain is excluded from a comparison here."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import softmax_ais_twin as st

pytestmark = pytest.mark.gpu

RTOL = 1e-5            # the project's parity bar
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_engine(P, K, max_batch=10, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = P['W'].shape
    eng = RbmEngine(V, H, max_batch=max_batch, v_groups=K, **kw)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, P[n])
    return eng


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_chains(got, want, ties):
    """every chain without a recorded near-tie at rtol 1e-5; at most a quarter may be excluded (the chosen inputs: none)"""
    keep = ties == 0
    assert np.sum(~keep) * 4 <= len(keep), ties
    for j in np.flatnonzero(keep):
        print('chain %d: engine %.9g twin %.9g rel %.2e' % (j, got[j], want[j], abs(got[j] - want[j]) / abs(want[j])))
    np.testing.assert_allclose(got[keep], want[keep], rtol=RTOL)


def bracket(values, exact):
    ok, est, sem = st.bracketed(values, exact)
    print('estimate %.6f exact %.6f sem %.4g' % (est, exact, sem))
    assert ok, (est, exact, sem)


def run_case(c, max_batch=4):
    G, K, H, pseed, std, n_betas, n_runs, k, seed, chain0 = c[:10]
    P, a, obs = st.case_inputs(c)
    eng = make_engine(P, K, max_batch=max_batch)          # n_runs > max_batch: the chain workspaces are the run's own
    got = eng.groups_ais(n_betas, n_runs, k, seed, chain0=chain0, base_bias=a, observed=obs)
    eng.close()
    return got


# ---- 1. chain by chain against the twin
@pytest.mark.parametrize('case', st.CHAIN_CASES, ids=st.case_id)
def test_chain_by_chain(gpu_lib, case):
    assert case[9] != 0 and case[6] % 16 != 0 and case[6] > 4
    want, ties = st.run_case(case)
    assert_chains(run_case(case), want, ties)


@pytest.mark.parametrize('case', st.FULL_CASES, ids=st.case_id)
def test_full_width_chain_by_chain(gpu_lib, case):
    assert case[2] == 1024 and case[9] >= 1000
    want, ties = st.run_case(case)
    assert_chains(run_case(case, max_batch=10), want, ties)


# ---- 2. the fused flavour against the generic triple, and in every geometry
FUSED_CASES = [c for c in st.CHAIN_CASES if c[:3] in st.FUSED_SHAPES]


def fused_digests():
    """one digest per fused chain-by-chain case of the values bm_rbm_groups_ais returns"""
    return [hashlib.sha1(bits(run_case(c)).tobytes()).hexdigest() for c in FUSED_CASES]


GEOMETRIES = ('8', '4', '1', '3', '108', '104', '101', '103', '208', '6', '5', '7', '9')      # what launch_act_as accepts
CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_softmax_ais_gpu as G
print('SOFTMAX_AIS_DIGEST', ' '.join(G.fused_digests()))
'''


def test_routes_and_every_geometry_give_the_same_bits(gpu_lib):
    """the fused cases in fresh child processes (BM355_DEBUG is read once per process): one under sm_fused=0 - the logits pass,
    softmax_groups_kernel and the row-dot kernel - and one per forced act_geo, each under its own time limit; the first failure
    ends the test (as tests/test_softmax_v_gpu.py)"""
    assert len(FUSED_CASES) == 9
    want = fused_digests()
    for dbg in ('sm_fused=0',) + tuple('act_geo=' + g for g in GEOMETRIES):
        env = dict(os.environ, BM355_DEBUG=dbg)
        r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'SOFTMAX_AIS_DIGEST' in r.stdout, '%s: %s' % (dbg, r.stdout[-2000:] + r.stderr[-4000:])
        got = r.stdout.split('SOFTMAX_AIS_DIGEST', 1)[1].split()
        assert got == want, '%s: cases %r differ from the default run' % (dbg, [st.case_id(c) for c, g, w in zip(FUSED_CASES, got, want) if g != w])


# ---- 3. determinism, slices, what a run leaves untouched
@pytest.mark.parametrize('shape', [(6, 4, 12), (7, 5, 17)], ids=['fused', 'generic'])
def test_determinism_slices_and_patterns(gpu_lib, shape):
    G, K, H = shape
    P = st.make_params(G, K, H, std=0.3)
    a = st.base_of('vector', G, K)
    obs = st.observed_of((0, G - 1), G)
    eng = make_engine(P, K)
    for o in (None, obs):
        r1 = eng.groups_ais(30, 300, 1, 11, base_bias=a, observed=o)
        r2 = eng.groups_ais(30, 300, 1, 11, base_bias=a, observed=o)
        assert np.all(np.isfinite(r1))
        assert np.array_equal(bits(r1), bits(r2))
        c = eng.groups_ais(30, 100, 1, 11, chain0=150, base_bias=a, observed=o)
        assert np.array_equal(bits(c), bits(r1[150:250]))
    full = eng.groups_ais(30, 100, 2, 12, chain0=3, base_bias=a, observed=np.ones(G, bool))
    none = eng.groups_ais(30, 100, 2, 12, chain0=3, base_bias=a)
    assert np.array_equal(bits(full), bits(none))
    assert not np.array_equal(bits(none), bits(eng.groups_ais(30, 100, 2, 12, chain0=3, base_bias=a, observed=obs)))
    eng.close()


@pytest.mark.parametrize('K,G,H,B', [(4, 33, 24, 37), (5, 13, 24, 37)], ids=['fused', 'generic'])
def test_a_run_leaves_the_handle_as_it_was(gpu_lib, K, G, H, B):
    """parameters, momentum buffers, the call counter (three updates against the training twin, bit for bit, behind the run) and
    groups_scores are what they were; bm_rbm_groups_set_missing is not looked at"""
    from boltzmann_machines_amd.engine import as_device
    from tests import test_softmax_v_gpu as SV
    eng, twin = SV.pair(K, G, H, B, 3)
    X = SV.categories(B, G, K, 2)
    SV.three_updates(eng, twin, X, 1, what='before')
    before = {n: eng.get(n).copy() for n in SV.STATE}
    scores = eng.groups_scores(as_device(X), B)
    obs = st.observed_of((0, G - 1), G)
    v1 = eng.groups_ais(10, 50, 2, 5, chain0=9, observed=obs)
    eng.groups_set_missing(True)
    v2 = eng.groups_ais(10, 50, 2, 5, chain0=9, observed=obs)
    eng.groups_set_missing(False)
    assert np.array_equal(bits(v1), bits(v2))
    for n in SV.STATE:
        assert np.array_equal(bits(eng.get(n)), bits(before[n])), n
    assert np.array_equal(eng.groups_scores(as_device(X), B), scores)
    SV.three_updates(eng, twin, X, 1, what='behind the AIS run')
    eng.close()


# ---- 4. ground truth
GT = (4, 3, 8)
GT_PATTERN = np.array([True, False, True, True])


def _model_samples(P, K, n, sweeps=200, seed=5):
    """approximate samples of the model (NumPy block Gibbs): the data a base-rate reference is computed from"""
    rng = np.random.RandomState(seed)
    W, vb, hb = (np.asarray(P[k], dtype=np.float64) for k in ('W', 'vb', 'hb'))
    G = W.shape[0] // K
    v = st.one_hot(rng.randint(0, K, (n, G)), K).astype(np.float64)
    for _ in range(sweeps):
        h = (rng.rand(n, W.shape[1]) < st.sigmoid(v.dot(W) + hb)).astype(np.float64)
        l3 = (h.dot(W.T) + vb).reshape(n, G, K)
        c = np.cumsum(np.exp(l3 - l3.max(axis=2, keepdims=True)), axis=2)
        cat = (rng.rand(n, G, 1) * c[:, :, -1:] >= c).sum(axis=2)
        v = st.one_hot(np.minimum(cat, K - 1), K).astype(np.float64)
    return v.astype(f32)


def test_ground_truth(gpu_lib, tmp_path):
    """the 4 x 3 x 8 model with weights N(0, 0.5^2): AIS (5000 betas, 512 chains) brackets the enumerated log Z under the uniform
    base, under the base rates of samples of the model, and for a pattern; log_proba with the exact log Z is the exact log p - over
    all 81 states, and for incomplete rows with their pattern's log Z"""
    from boltzmann_machines_amd import CategoricalRBM
    G, K, H = GT
    P = st.make_params(G, K, H, std=0.5, seed=7)
    exact = st.exact_log_Z(P, K)
    eng = make_engine(P, K)
    bracket(eng.groups_ais(5000, 512, 1, 777), exact)
    bracket(eng.groups_ais(5000, 512, 1, 778, base_bias=st.base_group_logits(_model_samples(P, K, 500), G, K)), exact)
    bracket(eng.groups_ais(5000, 512, 1, 779, observed=GT_PATTERN), st.exact_log_Z(P, K, GT_PATTERN))
    eng.close()
    m = CategoricalRBM(G, K, H, W_init=P['W'], vb_init=P['vb'], hb_init=P['hb'], batch_size=7, verbose=False, random_seed=1,
                       model_path=str(tmp_path / 'gt') + '/', v_shape=(G, K)).init()
    X = st.all_states(G, K)
    lp = m.log_proba(X, exact)
    print('sum of p over the %d states: %.6f' % (len(X), np.exp(lp).sum()))
    assert len(X) == 81 and abs(np.exp(lp).sum() - 1.0) < 1e-3
    Xi = st.data(30, G, K, 5, p_missing=0.4)
    patterns, index = m.observed_patterns(Xi)
    assert len(patterns) > 2
    logz = np.array([st.exact_log_Z(P, K, p) for p in patterns])[index]
    lpi, want = m.log_proba(Xi, logz), st.exact_log_p(P, K, Xi)
    print('max |log_proba - exact log p| over incomplete rows = %.3g' % np.max(np.abs(lpi - want)))
    np.testing.assert_allclose(lpi, want, rtol=0, atol=1e-4)


# ---- 5. the public API
AG, AK, AH, AN, BS = 5, 4, 12, 24, 8


def test_public_api(gpu_lib, tmp_path):
    from boltzmann_machines_amd import CategoricalRBM
    AX = st.data(AN, AG, AK, 3, p_missing=0.25)
    m = CategoricalRBM(AG, AK, AH, max_epoch=1, batch_size=BS, random_seed=11, verbose=False, missing_values=True,
                       model_path=str(tmp_path / 'api') + '/', v_shape=(AG, AK)).fit(AX)
    params = m.get_tf_params(scope='weights')
    state = m._rng.get_state()
    lz, (lo, hi), vals = m.ais_log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1)
    assert vals.shape == (32,) and np.all(np.isfinite(vals))
    assert np.isfinite(lz) and lo <= lz <= hi
    assert abs(lz - (AH * np.log(2) + AG * np.log(AK))) < 10.0            # small weights: near the uniform value
    m._rng.set_state(state)
    again = m.ais_log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1)[2]      # the same host seed state: the same bits
    assert np.array_equal(bits(again), bits(vals))
    lzb, (lob, hib), valsb = m.ais_log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1, X_base=AX)
    assert np.all(np.isfinite(valsb)) and lob <= lzb <= hib and abs(lzb - lz) < 1.0
    obs = np.array([True, False, True, True, False])
    lzo, (loo, hio), _ = m.ais_log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1, X_base=AX, observed=obs)
    assert loo <= lzo <= hio and abs(lzo - (AH * np.log(2) + 3 * np.log(AK))) < 10.0
    # the log-likelihood of incomplete rows: one run per distinct pattern
    patterns, index = m.observed_patterns(AX)
    logz = m.ais_log_Z_rows(AX, n_betas=100, n_runs=32, n_gibbs_steps=1, X_base=AX)
    assert logz.shape == (AN,) and np.all(np.isfinite(logz))
    for p in range(len(patterns)):
        assert len(set(logz[index == p])) == 1
    lp = m.log_proba(AX, logz)
    assert lp.shape == (AN,) and np.all(np.isfinite(lp)) and np.all(lp < 0)
    after = m.get_tf_params(scope='weights')
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(after[n]), bits(params[n])), n
    m2 = CategoricalRBM.load_model(m._model_dirpath)
    assert m2.missing_values is True
    assert np.array_equal(m2.log_proba(AX, logz), lp)
    lz2 = m2.ais_log_Z(n_betas=100, n_runs=32, n_gibbs_steps=1)[0]
    assert abs(lz2 - lz) < 1.0
    with pytest.raises(ValueError) as e:
        m.log_Z()
    assert 'softmax visible units' in str(e.value) and 'log_Z' in str(e.value)


# ---- 6. refusals
def test_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    lib = gpu_lib
    G, K, H = 4, 3, 8
    P = st.make_params(G, K, H)
    out = np.zeros(8, f32)
    op = out.ctypes.data_as(C.c_void_p)
    # a handle without groups: the message names visible groups, the handle still runs its own AIS
    plain = RbmEngine(G * K, H)
    assert lib.bm_rbm_groups_ais(plain._h, 4, 4, 1, None, None, 1, 0, op) != 0
    assert 'visible groups' in lib.bm_last_error().decode()
    assert np.all(np.isfinite(plain.ais(4, 4, 1, 1)))
    plain.close()
    eng = make_engine(P, K)
    good = eng.groups_ais(5, 8, 1, 3)
    assert lib.bm_rbm_ais(eng._h, 4, 4, 1, None, 1, 0, op) != 0                      # bm_rbm_ais still refuses a grouped handle
    assert 'softmax visible' in lib.bm_last_error().decode()
    with pytest.raises(_ffi.Bm355Error, match='bad AIS arguments'):
        eng.groups_ais(1, 4, 1, 1)
    with pytest.raises(_ffi.Bm355Error, match='bad AIS arguments'):
        eng.groups_ais(4, 0, 1, 1)
    with pytest.raises(_ffi.Bm355Error, match='bad AIS arguments'):
        eng.groups_ais(4, 4, 0, 1)
    with pytest.raises(_ffi.Bm355Error, match='observes none'):
        eng.groups_ais(4, 4, 1, 1, observed=np.zeros(G, bool))
    with pytest.raises(ValueError):
        eng.groups_ais(4, 4, 1, 1, observed=np.ones(G + 1, bool))
    with pytest.raises(ValueError):
        eng.groups_ais(4, 4, 1, 1, base_bias=np.zeros(G * K + 1, f32))
    assert np.array_equal(bits(eng.groups_ais(5, 8, 1, 3)), bits(good))              # the handle stays usable
    eng.close()
