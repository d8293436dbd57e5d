"""-m gpu: AIS log Z per document length of replicated softmax visible units (RbmEngine.rsm_ais, bm_rbm_rsm_ais)
chain by chain against tests/rsm_ais_twin.py, its exact case, determinism, the slice property, what a run leaves untouched, ground
truth by enumeration through ReplicatedSoftmaxRBM.ais_log_Z, the class end to end, and the C-ABI refusals.

The chain-by-chain cases are rsm_ais_twin.CHAIN_CASES; tests/test_rsm_ais.py shows without a GPU that the twin meets no near-tie in
any of them, so every chain is compared."""
import ctypes as C

import numpy as np
import pytest

from tests import rsm_ais_twin as A
from tests import rsm_twin as T

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RTOL = 1e-5                     # the project's tolerance for AIS values
STATE = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')
PLANTED = dict(V=24, H=4, n_train=120, batch=20, lr=0.02, mom=0.5, epochs=3, max_length=30)      # tests/test_rsm.py's corpus


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def engine(P, max_length, B=8):
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = P['W'].shape
    eng = RbmEngine(V, H, max_batch=B, rsm_max_length=max_length)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, P[n])
    return eng


# ---- 1. chain by chain against the twin
@pytest.mark.parametrize('case', A.CHAIN_CASES, ids=A.case_id)
def test_chains_against_the_twin(gpu_lib, case):
    V, H, ml, lengths, n_betas, k, seed, chain0 = case[:8]
    P, a = A.case_inputs(case)
    want, ties = A.run_case(case)
    assert ties.sum() == 0
    eng = engine(P, ml)
    got = eng.rsm_ais(n_betas, lengths, k, seed, chain0=chain0, base_logits=a)
    eng.close()
    assert got.dtype == f32 and got.shape == (len(lengths),)
    err = np.abs(got.astype(f64) - want) / np.abs(want)
    print('%s: max relative error %.3e' % (A.case_id(case), err.max()))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


# ---- 2. the exact case
def test_flat_model_is_the_closed_form(gpu_lib):
    """W = 0, hb = 0, a = vb: dvec = 0 and t = 0, every score is exactly 0 - every chain equals H log 2 + D logsumexp(vb) within
    the float32 rounding of the value (half an ulp: 2^-24 relative)"""
    V, H, ml = 300, 17, 40
    P = A.make_params(V, H, seed=41)
    P['W'][...] = 0
    P['hb'][...] = 0
    lengths = np.array(A._ladder(33, ml), f64)
    eng = engine(P, ml)
    got = eng.rsm_ais(12, lengths, 2, 5, chain0=7, base_logits=P['vb'])
    eng.close()
    vb = P['vb'].astype(f64)
    want = H * np.log(2.) + lengths * (vb.max() + np.log(np.exp(vb - vb.max()).sum()))
    assert np.all(np.abs(got.astype(f64) - want) <= 2.0 ** -24 * np.abs(want) * (1 + 1e-9))


# ---- 3. determinism and the slice property
def test_determinism_and_slices(gpu_lib):
    V, H, ml = 257, 17, 25
    P = A.make_params(V, H, std=0.2, seed=42)
    a = A.peaked_base(V, 4)
    lengths = np.array(A._ladder(41, ml), f32)
    eng = engine(P, ml)
    r1 = eng.rsm_ais(9, lengths, 2, 11, chain0=100, base_logits=a)
    r2 = eng.rsm_ais(9, lengths, 2, 11, chain0=100, base_logits=a)
    assert np.array_equal(bits(r1), bits(r2))
    head = eng.rsm_ais(9, lengths[:13], 2, 11, chain0=100, base_logits=a)           # a split at an odd row
    tail = eng.rsm_ais(9, lengths[13:], 2, 11, chain0=113, base_logits=a)
    assert np.array_equal(bits(r1), bits(np.concatenate([head, tail])))
    other = eng.rsm_ais(9, lengths, 2, 12, chain0=100, base_logits=a)
    assert not np.array_equal(bits(r1), bits(other))
    eng.close()


# ---- 4. a run leaves the handle untouched
def test_a_run_leaves_the_handle_untouched(gpu_lib):
    """parameters and momenta; the call counter and the lengths of bm_rbm_set_row_lengths (the second sample_v_from_h of a seeded
    handle draws the same counts with and without a run in between, and needs no new lengths); the update that follows"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    V, H, ml, B = 40, 17, 20, 8
    P = A.make_params(V, H, std=0.3, seed=43)
    D = np.array([1, 20, 3, 7, 11, 2, 19, 5], f32)
    rng = np.random.RandomState(5)
    Hs = (rng.uniform(size=(B, H)) < 0.5).astype(f32)
    X = np.stack([np.bincount(rng.randint(0, V, int(d)), minlength=V) for d in D]).astype(f32)

    def run(with_ais):
        eng = engine(P, ml, B)
        eng.seed(77)
        eng.train_step(as_device(X), B, 0.05, 0.5, 1)                    # (momenta that are not zero)
        before = {n: eng.get(n) for n in STATE}
        Hd, Sd = as_device(Hs), DeviceArray((B, V), f32)
        eng.set_row_lengths(as_device(D), B)
        eng.sample_v_from_h(Hd, B, None, Sd)
        eng.sync()
        s1 = Sd.numpy()
        if with_ais:
            eng.rsm_ais(6, [20, 1, 5] * 4, 2, 3, chain0=1, base_logits=A.peaked_base(V, 5))
            for n in STATE:
                assert np.array_equal(bits(eng.get(n)), bits(before[n])), n
        eng.sample_v_from_h(Hd, B, None, Sd)
        eng.sync()
        s2 = Sd.numpy()
        eng.train_step(as_device(X), B, 0.05, 0.5, 1)
        out = (s1, s2, {n: eng.get(n) for n in STATE})
        eng.close()
        return out
    a1, a2, pa = run(True)
    b1, b2, pb = run(False)
    assert np.array_equal(bits(a1), bits(b1)) and np.array_equal(bits(a2), bits(b2))
    assert not np.array_equal(bits(a1), bits(a2))                        # (the call counter did advance between the two draws)
    assert np.array_equal(a2.sum(axis=1), D)
    for n in STATE:
        assert np.array_equal(bits(pa[n]), bits(pb[n])), 'the update after a run differs in ' + n


# ---- 5. ground truth, through the class
def test_ground_truth_through_the_class(gpu_lib, tmp_path):
    """V = 300, H = 10, three lengths in one run, at the n_betas and the criterion fixed on the CPU (tests/test_rsm_ais.py):
    |log_mean - exact| <= 3 s, s the delta-method standard error of the run's own values"""
    import boltzmann_machines_amd as bm
    from tests.test_rsm_ais import GT_K, GT_LENGTHS, GT_N_BETAS, GT_N_RUNS, GT_SHAPES, gt_params, gt_ratios
    V, H, pseed = GT_SHAPES[-1]
    assert (V, H) == (300, 10)
    P = gt_params(V, H, pseed)
    m = bm.ReplicatedSoftmaxRBM(n_visible=V, n_hidden=H, max_length=40, W_init=P['W'], vb_init=P['vb'], hb_init=P['hb'],
                                random_seed=4242, verbose=False, v_shape=(15, 20), model_path=str(tmp_path) + '/g/').init()
    log_mean, (lo, hi), values = m.ais_log_Z(list(GT_LENGTHS), n_betas=GT_N_BETAS, n_runs=GT_N_RUNS, n_gibbs_steps=GT_K)
    assert values.shape == (3, GT_N_RUNS) and log_mean.shape == (3,)
    for (ratio, est, exact, s), D, lm in zip(gt_ratios(P, values), GT_LENGTHS, log_mean):
        print('D=%d: log_mean %.6f exact %.6f s %.3g ratio %.2f' % (D, est, exact, s, ratio))
        # (log_mean is the helpers' float32 arithmetic on the float32 values, est the same mean in float64)
        assert abs(lm - est) <= 1e-6 * abs(est) and abs(lm - exact) <= 3.0 * s and ratio <= 3.0, (D, lm, est, exact, s)


# ---- 6. the class end to end
def test_class_end_to_end(gpu_lib, tmp_path):
    """a few updates on the planted two-topic corpus: the perplexity from AIS is finite and below the uniform model's V; a
    checkpoint round trip returns the same ais_log_Z values from the same seed"""
    import boltzmann_machines_amd as bm
    c = PLANTED
    X, _ = T.planted_corpus(c['n_train'], 1, c['V'])
    rng = np.random.RandomState(3)
    m = bm.ReplicatedSoftmaxRBM(n_visible=c['V'], n_hidden=c['H'], max_length=c['max_length'],
                                W_init=(0.01 * rng.randn(c['V'], c['H'])).astype(f32), vb_init=np.zeros(c['V'], f32),
                                hb_init=np.zeros(c['H'], f32), batch_size=c['batch'], learning_rate=c['lr'], momentum=c['mom'], l2=1e-4,
                                max_epoch=c['epochs'], random_seed=1337, verbose=False, save_after_each_epoch=False, v_shape=(4, 6),
                                model_path=str(tmp_path) + '/a/')
    m.fit(X)
    kw = dict(n_betas=30, n_runs=3, n_gibbs_steps=1, X_base=X)
    lz = m.ais_log_Z_rows(X, **kw)
    assert lz.shape == (len(X),) and np.all(np.isfinite(lz))
    ppl = m.perplexity(X, lz)
    print('perplexity %.3f (uniform: %d)' % (ppl, c['V']))
    assert np.isfinite(ppl) and ppl < c['V']
    ll = m.log_likelihood(X, lz)
    assert ll.shape == (len(X),) and np.all(np.isfinite(ll)) and np.all(ll < 0)
    a, b = bm.ReplicatedSoftmaxRBM.load_model(str(tmp_path) + '/a/'), bm.ReplicatedSoftmaxRBM.load_model(str(tmp_path) + '/a/')
    va, vb_ = a.ais_log_Z([3, 30, 11], **kw)[2], b.ais_log_Z([3, 30, 11], **kw)[2]
    assert va.shape == (3, 3) and np.array_equal(bits(va), bits(vb_))


# ---- 7. the C ABI
def test_c_abi_refusals(gpu_lib):
    from boltzmann_machines_amd.engine import RbmEngine
    lib = gpu_lib
    case = A.CHAIN_CASES[1]                                                # (the run that shows the handle usable is one of the cases)
    V, H, ml = case[:3]
    assert ml < 20
    P, a = A.case_inputs(case)
    out = np.zeros(64, f32)
    op = out.ctypes.data_as(C.c_void_p)

    def lp(x):
        return np.ascontiguousarray(x, f32).ctypes.data_as(C.c_void_p)

    def refused(rc, what):
        assert rc != 0, what + ' was accepted'
        msg = lib.bm_last_error().decode()
        assert 'bm_rbm_rsm_ais' in msg, '%s: %s' % (what, msg)
    good = np.array([1, ml, 5, 7], f32)
    plain = RbmEngine(V, H, max_batch=8)
    refused(lib.bm_rbm_rsm_ais(plain._h, 4, 4, 1, None, lp(good), 1, 0, op), 'a handle without replicated softmax')
    assert 'replicated softmax' in lib.bm_last_error().decode()
    assert plain.ais(4, 4, 1, 1).shape == (4,)                             # the handle is what it was
    plain.close()
    eng = engine(P, ml)
    h = eng._h
    for bad, what in (([1, 0, 5, 7], 'a length of 0'), ([1, ml + 1, 5, 7], 'a length above max_length'), ([1, 2.5, 5, 7], 'a fractional length'),
                      ([1, np.nan, 5, 7], 'a NaN length'), ([1, -3, 5, 7], 'a negative length')):
        keep = np.ascontiguousarray(bad, f32)
        refused(lib.bm_rbm_rsm_ais(h, 4, 4, 1, None, keep.ctypes.data_as(C.c_void_p), 1, 0, op), what)
    refused(lib.bm_rbm_rsm_ais(h, 1, 4, 1, None, lp(good), 1, 0, op), 'n_betas = 1')
    refused(lib.bm_rbm_rsm_ais(h, 4, 0, 1, None, lp(good), 1, 0, op), 'n_rows = 0')
    refused(lib.bm_rbm_rsm_ais(h, 4, 4, 0, None, lp(good), 1, 0, op), 'n_gibbs_steps = 0')
    refused(lib.bm_rbm_rsm_ais(h, 4, 4, 1, None, lp(good), 1, -1, op), 'chain0 = -1')
    refused(lib.bm_rbm_rsm_ais(h, 4, 4, 1, None, None, 1, 0, op), 'null lengths')
    refused(lib.bm_rbm_rsm_ais(h, 4, 4, 1, None, lp(good), 1, 0, None), 'null values')
    refused(lib.bm_rbm_rsm_ais(None, 4, 4, 1, None, lp(good), 1, 0, op), 'a null handle')
    assert lib.bm_rbm_ais(h, 4, 4, 1, None, 1, 0, op) != 0                 # bm_rbm_ais stays refused, and now names the entry
    msg = lib.bm_last_error().decode()
    assert 'replicated softmax' in msg and 'bm_rbm_ais' in msg and 'bm_rbm_rsm_ais' in msg, msg
    got = eng.rsm_ais(case[4], case[3], case[5], case[6], chain0=case[7], base_logits=a)      # the handle is usable
    np.testing.assert_allclose(got, A.run_case(case)[0], rtol=RTOL, atol=0)
    with pytest.raises(ValueError):
        eng.rsm_ais(5, good, 1, 3, base_logits=np.zeros(V + 1, f32))
    eng.close()
