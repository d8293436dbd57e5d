"""AIS log Z per document length, log-likelihood and perplexity of replicated softmax visible units without a GPU:
the twin (tests/rsm_ais_twin.py) against enumeration, its exact cases, its slice property, the absence of near-ties in every case
the GPU test compares chain by chain, and the host logic of the Python class.  tests/test_rsm_ais_gpu.py holds the engine to the
same twin."""
import re
from math import lgamma

import numpy as np
import pytest

from tests import rsm_ais_twin as A
from tests import rsm_twin as T

f32, f64 = np.float32, np.float64

# ---- 1. the twin against enumeration
# |log_mean - exact| <= 3 s per length, s the delta-method standard error of log_mean_exp from the run's own values, the seeds fixed.
# n_betas is the smallest of the ladder 100 / 300 / 1000 at which every case below holds on the CPU: 100.  Observed ratios
# |log_mean - exact| / s at n_betas = 100, (V, H) x D = (1, 3, 40):  (4, 2): 0.73, 0.70, 0.97;  (17, 5): 0.70, 1.51, 1.05;
# (300, 10): 1.01, 0.73, 0.62  (at 300: the largest is 1.78, at 1000: 2.74 - s shrinks with the ladder, the ratio does not).
# tests/test_rsm_ais_gpu.py runs the (300, 10) case through ReplicatedSoftmaxRBM.ais_log_Z at the same n_betas and criterion.
GT_N_BETAS, GT_N_RUNS, GT_K, GT_LENGTHS = 100, 60, 1, (1, 3, 40)
GT_SHAPES = [(4, 2, 11), (17, 5, 12), (300, 10, 13)]            # (V, H, param seed); weights N(0, 0.5^2)


def gt_params(V, H, pseed):
    return A.make_params(V, H, std=0.5, seed=pseed)


def gt_ratios(P, values):
    """per length (|log_mean - exact| / s, log_mean, exact, s) of values [L][n_runs]"""
    out = []
    for l, D in enumerate(GT_LENGTHS):
        est, s = A.log_mean_and_se(values[l])
        exact = A.exact_log_Z(P, D)
        out.append((abs(est - exact) / s, est, exact, s))
    return out


@pytest.mark.parametrize('V,H,pseed', GT_SHAPES)
def test_twin_against_enumeration(V, H, pseed):
    P = gt_params(V, H, pseed)
    lengths = np.repeat(GT_LENGTHS, GT_N_RUNS)                  # the three lengths mixed in one run
    values, _ = A.ais(P, lengths, GT_N_BETAS, GT_K, 900 + pseed, max_length=40)
    for (ratio, est, exact, s), D in zip(gt_ratios(P, values.reshape(len(GT_LENGTHS), GT_N_RUNS)), GT_LENGTHS):
        print('V=%d H=%d D=%d: log_mean %.6f exact %.6f s %.3g ratio %.2f' % (V, H, D, est, exact, s, ratio))
        assert ratio <= 3.0, (V, H, D, est, exact, s)


def test_exact_log_Z_agrees_with_both_enumerations():
    """the hidden-side enumeration against rsm_twin's, and against the sum over the count vectors"""
    P = T.small_model()
    for D in (1, 3, 6):
        assert abs(A.exact_log_Z(P, D) - T.log_z_hidden(P, D)) < 1e-12
        assert abs(A.exact_log_Z(P, D) - T.log_z_visible(P, D)) < 1e-10


# ---- 2. two exact cases
def test_flat_model_is_exact():
    """W = 0, hb = 0, a = vb: every importance weight is 1 - values == H log 2 + D logsumexp(vb) to double round-off"""
    V, H = 17, 5
    P = A.make_params(V, H, seed=21)
    P['W'][...] = 0
    P['hb'][...] = 0
    lengths = np.array([1, 3, 40, 40, 7, 1], f64)
    values, _ = A.ais(P, lengths, 30, 2, 77, chain0=3, base_logits=P['vb'], max_length=40)
    vb = P['vb'].astype(f64)
    want = H * np.log(2.) + lengths * (vb.max() + np.log(np.exp(vb - vb.max()).sum()))
    np.testing.assert_allclose(values, want, rtol=1e-14, atol=0)


def test_two_betas_is_one_score():
    """n_betas = 2: one score of v_0 and no transition - value = v_0.dvec + sum_j [softplus(t_j) - log 2] + log Z_0(D)"""
    V, H, ml = 17, 5, 12
    P = A.make_params(V, H, std=0.4, seed=22)
    a = A.peaked_base(V, 2)
    lengths = np.array([1, 12, 5, 7], f64)
    values, ties = A.ais(P, lengths, 2, 3, 88, chain0=6, base_logits=a, max_length=ml)
    v0 = A._draw_counts(np.tile(a, (4, 1)), lengths, 88, A.SITE_V0, 0, 0, 6, ml, np.zeros(4, np.int64))
    assert np.array_equal(v0.sum(axis=1), lengths)
    d = (P['vb'] - a).astype(f32).astype(f64)
    t = v0.dot(P['W'].astype(f64)) + lengths[:, None] * P['hb'].astype(f64)
    want = v0.dot(d) + np.sum(np.logaddexp(0., t) - np.log(2.), axis=1) + A.log_Z0(P, lengths, a)
    np.testing.assert_allclose(values, want, rtol=1e-13, atol=0)


# ---- 3. the slice property
def test_twin_slices():
    """rows [0, R) in one call == rows [0, r1) at chain0 = c and rows [r1, R) at chain0 = c + r1, for an odd r1"""
    V, H, ml = 17, 5, 9
    P = A.make_params(V, H, std=0.3, seed=23)
    lengths = np.array(A._ladder(11, ml), f64)
    whole, _ = A.ais(P, lengths, 6, 2, 99, chain0=4, base_logits=A.peaked_base(V, 3), max_length=ml)
    head, _ = A.ais(P, lengths[:5], 6, 2, 99, chain0=4, base_logits=A.peaked_base(V, 3), max_length=ml)
    tail, _ = A.ais(P, lengths[5:], 6, 2, 99, chain0=9, base_logits=A.peaked_base(V, 3), max_length=ml)
    assert np.array_equal(whole, np.concatenate([head, tail]))


# ---- 4. no near-ties in the cases the GPU test compares chain by chain (a condition, not a measurement)
@pytest.mark.parametrize('case', A.CHAIN_CASES, ids=A.case_id)
def test_chain_cases_meet_no_near_tie(case):
    values, ties = A.run_case(case)
    assert np.all(np.isfinite(values)) and len(values) == len(case[3])
    assert ties.sum() == 0, 'near-ties per chain: %r' % (ties,)


def test_chain_cases_cover_the_boundaries():
    """what DESIGN.md 3.28 lists: run, block and kernel-instantiation edges of V, softplus slots of H, the score kernel's 32 chains
    per workgroup, both Gibbs depths, both bases, n_betas = 2, lengths 1 and max_length in every mixed run"""
    C = A.CHAIN_CASES
    assert {2, 16, 17, 256, 257, 4096, 4097} <= {c[0] for c in C} and {16, 17, 40} <= {c[1] for c in C}
    assert {1, 32, 33} <= {len(c[3]) for c in C} and {1, 2} <= {c[5] for c in C} and {None, 'peaked'} <= {c[8] for c in C}
    assert 2 in {c[4] for c in C} and max(c[4] for c in C) <= 30 and max(len(c[3]) for c in C) <= 70
    for c in C:
        assert 1 <= min(c[3]) and max(c[3]) <= c[2]
        if len(c[3]) > 1:
            assert 1 in c[3] and c[2] in c[3]


# ---- 5. the Python class: log-likelihood and perplexity with the engine's free energy replaced by float64
def _no_engine(monkeypatch):
    """any attempt to build an engine fails the test (as tests/test_rsm.py)"""
    from boltzmann_machines_amd import rbm as rbm_mod

    def boom(*a, **k):
        raise AssertionError('an engine call was made')
    monkeypatch.setattr(rbm_mod, 'RbmEngine', boom)
    monkeypatch.setattr(rbm_mod, 'RbmEngine64', boom)


def _model(tmp_path, V=4, H=2, ml=40, **kw):
    import boltzmann_machines_amd as bm
    return bm.ReplicatedSoftmaxRBM(V, H, ml, batch_size=4, model_path=str(tmp_path) + '/m/', verbose=False, **kw)


def _with_free_energy(monkeypatch, m, P):
    monkeypatch.setattr(m, 'free_energy', lambda X: T.free_energy64(P, X))


def test_perplexity_of_a_flat_model_is_the_unigram_perplexity(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    V, H = 24, 3
    m = _model(tmp_path, V, H)
    P = A.make_params(V, H, seed=31)
    P['W'][...] = 0
    P['hb'][...] = 0
    _with_free_energy(monkeypatch, m, P)
    X, _ = T.planted_corpus(40, 5, V=V)
    D = X.sum(axis=1).astype(f64)
    vb = P['vb'].astype(f64)
    lse = vb.max() + np.log(np.exp(vb - vb.max()).sum())
    log_q = vb - lse
    want = np.exp(-np.mean(X.astype(f64).dot(log_q) / D))
    got = m.perplexity(X, H * np.log(2.) + D * lse)
    assert abs(got - want) <= 1e-12 * want, (got, want)
    assert m._engine is None


def test_coefficient_and_normalisation(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    P = T.small_model()
    m = _model(tmp_path)
    _with_free_energy(monkeypatch, m, P)
    X, logc = T.count_vectors(4, 3)
    lz = np.full(len(X), A.exact_log_Z(P, 3))
    unordered, ordered = m.log_likelihood(X, lz), m.log_likelihood(X, lz, ordered=True)
    assert unordered.dtype == f64 and unordered.shape == (len(X),)
    np.testing.assert_allclose(unordered - ordered, logc, rtol=0, atol=1e-13)
    np.testing.assert_allclose(logc, [lgamma(4.) - sum(lgamma(n + 1.) for n in row) for row in X], rtol=0, atol=1e-13)
    assert abs(np.exp(unordered).sum() - 1.0) < 1e-12
    # one token sequence per count vector weighs D!/prod v_i! sequences: the ordered probabilities sum to one over the sequences
    assert abs(np.sum(np.exp(ordered + logc)) - 1.0) < 1e-12
    with pytest.raises(ValueError):
        m.log_likelihood(X, lz[:-1])
    assert m._engine is None


# ---- 6. host logic
class _StubEngine(object):
    """records the calls of RbmEngine.rsm_ais and returns the chain's length plus a thousandth of its global index"""

    def __init__(self):
        self.calls = []

    def rsm_ais(self, n_betas, lengths, k, seed, chain0=0, base_logits=None):
        lengths = np.asarray(lengths)
        self.calls.append(dict(n_betas=n_betas, lengths=lengths.copy(), k=k, seed=seed, chain0=chain0, base_logits=base_logits))
        return (lengths + 1e-3 * (chain0 + np.arange(len(lengths)))).astype(f32)


def _stubbed(monkeypatch, m):
    stub = _StubEngine()
    m.initialized_ = True
    monkeypatch.setattr(m, '_ensure_engine', lambda: None)
    monkeypatch.setattr(m, '_on_device', lambda: stub)
    monkeypatch.setattr(m, '_seed_engine', lambda seed: None)
    monkeypatch.setattr(m, '_join_save', lambda: None)
    return stub


def test_base_logits(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    X = np.array([[2, 0, 1, 0], [0, 0, 4, 0], [1, 1, 1, 1]], f32)
    a = m._base_logits(X)
    assert a.dtype == f32 and a.shape == (4,)
    np.testing.assert_array_equal(a, np.log((np.array([3., 1., 6., 1.]) + 1.) / (11. + 4.)).astype(f32))
    np.testing.assert_array_equal(a, A.unigram_base(X))
    assert abs(np.exp(a.astype(f64)).sum() - 1.0) < 1e-6
    assert m._base_logits(None) is None
    np.testing.assert_array_equal(m._base_logits(np.arange(4.)), np.arange(4, dtype=f32))
    for bad in (np.zeros(3), np.zeros((2, 3)), np.array([0., np.inf, 0., 0.]), np.array([[1, 0.5, 0, 0]])):
        with pytest.raises(ValueError):
            m._base_logits(bad)
    assert m._engine is None


def test_return_shapes_and_chain_indices(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    stub = _stubbed(monkeypatch, m)
    log_mean, (lo, hi), values = m.ais_log_Z([3, 40, 3], n_betas=7, n_runs=5, n_gibbs_steps=2)
    assert log_mean.shape == lo.shape == hi.shape == (3,) and values.shape == (3, 5)
    assert len(stub.calls) == 1
    c = stub.calls[0]
    assert (c['n_betas'], c['k'], c['chain0'], c['base_logits']) == (7, 2, 0, None) and c['seed'] is not None
    np.testing.assert_array_equal(c['lengths'], np.repeat([3, 40, 3], 5))      # chain index = position in the flattened [L, n_runs]
    assert np.all(lo <= log_mean) and np.all(log_mean <= hi)
    from boltzmann_machines_amd.utils import log_mean_exp
    for l in range(3):
        assert log_mean[l] == log_mean_exp(values[l])
    s_mean, (s_lo, s_hi), s_values = m.ais_log_Z(np.int64(40), n_runs=4)
    assert np.ndim(s_mean) == 0 and np.ndim(s_lo) == 0 and np.ndim(s_hi) == 0 and s_values.shape == (4,)
    assert stub.calls[1]['n_betas'] == 100 and stub.calls[1]['k'] == 5 and stub.calls[1]['seed'] != c['seed']
    # more chains than one engine call takes: chunks through chain0, invisible in the values
    monkeypatch.setattr(m, '_AIS_MAX_ROWS', 4)
    n0 = len(stub.calls)
    _, _, chunked = m.ais_log_Z([3, 40, 3], n_runs=3)
    assert [cc['chain0'] for cc in stub.calls[n0:]] == [0, 4, 8] and len({cc['seed'] for cc in stub.calls[n0:]}) == 1
    np.testing.assert_array_equal(chunked.reshape(-1), (np.repeat([3, 40, 3], 3) + 1e-3 * np.arange(9)).astype(f32))


def test_ais_log_Z_rows_groups_by_length(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    stub = _stubbed(monkeypatch, m)
    X = np.array([[2, 0, 1, 0], [0, 0, 4, 0], [1, 1, 1, 0], [0, 7, 0, 0], [0, 0, 0, 3]], f32)       # lengths 3, 4, 3, 7, 3
    rows = m.ais_log_Z_rows(X, n_betas=5, n_runs=2, X_base=X)
    assert len(stub.calls) == 1                                    # ONE run for the three distinct lengths
    np.testing.assert_array_equal(stub.calls[0]['lengths'], np.repeat([3, 4, 7], 2))
    np.testing.assert_array_equal(stub.calls[0]['base_logits'], A.unigram_base(X))
    assert rows.dtype == f64 and rows.shape == (5,)
    assert rows[0] == rows[2] == rows[4] and len({rows[0], rows[1], rows[3]}) == 3
    assert abs(rows[1] - 4.0) < 0.01 and abs(rows[3] - 7.0) < 0.01
    assert m.ais_log_Z_rows(np.zeros((0, 4), f32)).shape == (0,) and len(stub.calls) == 1
    with pytest.raises(ValueError):
        m.ais_log_Z_rows(X, lengths=[3])


def test_argument_errors_come_before_the_engine(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    X = np.array([[2, 0, 1, 0], [0, 0, 4, 0]], f32)
    for kw in (dict(n_betas=1), dict(n_runs=0), dict(n_gibbs_steps=0), dict(X_base=np.zeros(3)), dict(X_base=np.zeros((2, 5)))):
        with pytest.raises(ValueError):
            m.ais_log_Z(3, **kw)
        with pytest.raises(ValueError):
            m.ais_log_Z_rows(X, **kw)
    for bad in (0, 41, 2.5, -1, [3, 0], [[3, 4]], [], np.nan, 'x', [3, 41], None):
        with pytest.raises(ValueError) as e:
            m.ais_log_Z(bad)
        assert 'lengths' in str(e.value) and 'max_length' in str(e.value)
    for bad in (np.array([[1, 0.5, 0, 0]]), np.zeros((1, 4)), np.array([[41, 0, 0, 0]]), np.zeros((2, 3))):
        for f in (m.ais_log_Z_rows, lambda B: m.log_likelihood(B, np.zeros(len(B))), lambda B: m.perplexity(B, np.zeros(len(B)))):
            with pytest.raises(ValueError):
                f(bad)
    with pytest.raises(ValueError):
        m.perplexity(np.zeros((0, 4)), np.zeros(0))
    assert m._engine is None


def test_refusals_name_the_new_methods(monkeypatch, tmp_path):
    _no_engine(monkeypatch)
    m = _model(tmp_path)
    for method, args, names in (('log_Z', (), ('ais_log_Z', 'ais_log_Z_rows')),
                                ('log_proba', (np.ones((1, 4)), 0.0), ('log_likelihood', 'perplexity', 'ais_log_Z_rows'))):
        with pytest.raises(ValueError) as e:
            getattr(m, method)(*args)
        msg = str(e.value)
        assert 'replicated softmax visible units' in msg and method in msg, msg
        for n in names:
            assert n in msg, msg
    # the docstring says which probability the perplexity uses
    assert 'SEQUENCE' in m.perplexity.__doc__ and 'ordered=True' in m.perplexity.__doc__
    assert m._engine is None


def test_header_declares_library_exports_and_ffi_binds():
    """the C-ABI surface of the entry: declared in the header with the arguments _ffi binds, exported by the library, wrapped by
    the engine"""
    import os
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'bm355.h')).read()
    mm = re.search(r'\bint\s+bm_rbm_rsm_ais\s*\(([^;]*?)\)\s*;', header, flags=re.S)
    assert mm, 'bm_rbm_rsm_ais is not declared in include/bm355.h'
    assert len(re.sub(r'/\*.*?\*/', '', mm.group(1), flags=re.S).split(',')) == 9 == len(_ffi.SIGNATURES['bm_rbm_rsm_ais'])
    assert 'bm_rbm_rsm_ais' in _ffi.exported_symbols()
    assert hasattr(_ffi.load(), 'bm_rbm_rsm_ais')
    assert callable(getattr(RbmEngine, 'rsm_ais', None))
