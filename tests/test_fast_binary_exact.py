"""What the float64 tests of the fast-binary mode (tests/test_fast_binary_exact_gpu.py) rest on, without a GPU: the NumPy twin
of split3() is exact on every probe weight, the structured weights are what they claim to be, and the tolerance of the
pinned-sparse comparison - with the constant C recorded in tests/fast_binary_probes.py - cannot hide a lost or shifted plane."""
import numpy as np
import pytest

from tests import fast_binary_probes as fb


def all_probe_weights():
    ws = [fb.pass_through_points()]
    ws += [fb.sparse_weights(V, n, s).ravel() for V, n, M, s in fb.SPARSE_CASES]
    ws += [fb.dense_inputs(V, n, M)[0].ravel() for V, n, M in fb.DENSE_CASES]
    ws += [fb.filler(100, 72, 1).ravel(), fb.sigmoid_hw_points()[fb.in_range(fb.sigmoid_hw_points())]]
    return np.concatenate(ws)


def test_split_twin_is_exact_on_every_probe_weight():
    w = all_probe_weights()
    w = w[fb.in_range(w)]
    assert len(w) > 300000
    hi, mid, lo = fb.split3_np(w)
    for name, p in (('hi', hi), ('mid', mid), ('lo', lo)):
        assert np.all(fb.is_bf16(p)), name                    # at most 8 significant bits each
    s = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(s, w.astype(np.float64))
    assert np.array_equal(fb.bits(s.astype(np.float32)), fb.bits(w))
    # and the parts do not overlap: |mid| < one unit of hi's last place, |lo| < one of mid's
    nz = hi != 0
    assert np.all(np.abs(mid[nz]) < np.abs(hi[nz]) * 2.0 ** -7) and np.all(np.abs(lo[mid != 0]) < np.abs(mid[mid != 0]) * 2.0 ** -7)


def test_pass_through_points_cover_what_they_claim():
    x = fb.pass_through_points()
    b = fb.bits(x)
    e = ((b >> 23) & 0xff).astype(int) - 127
    nz = b != 0
    assert e[nz].min() == fb.E_MIN and e[nz].max() == fb.E_MAX and np.any(~nz)
    for sign in (0, 1):
        s = (b >> 31) == sign
        assert len(np.unique(b[s & nz] & 0xff)) == 256 and len(np.unique((b[s & nz] >> 8) & 0xff)) == 256      # every lo, every mid byte
        assert len(np.unique(e[s & nz])) >= 21
    from tests import numerics_probes as npb
    sp = npb.sigmoid_points().ravel()
    assert np.all(np.isin(fb.bits(sp[fb.in_range(sp)]), b)) and fb.in_range(sp).sum() > 16000
    for V, n, M in fb.PASS_SHAPES:                             # one chunk per k0 at least, every point in some chunk
        assert len(fb.chunks(x, V)) >= len(fb.pass_k0(n))
        assert np.all(np.isin(b, fb.bits(fb.chunks(x, V))))


@pytest.mark.parametrize('V,n,M,scale', fb.SPARSE_CASES)
def test_structured_weights(V, n, M, scale):
    W = fb.sparse_weights(V, n, scale)
    b = fb.bits(W)
    assert W.shape == (V, n) and np.all(W > 0)
    unscaled = W.astype(np.float64) / scale
    assert np.all((unscaled >= 0.5) & (unscaled < 1.0))
    assert np.all((b & 0xff) == 0xff) and np.all(((b >> 8) & 0xff) != 0)
    hi, mid, lo = fb.split3_np(W)
    ulp = scale * 2.0 ** -24                                   # the last place of a float32 in [0.5, 1) * scale
    assert np.all(lo.astype(np.float64) == 255 * ulp)          # positive and maximal
    assert np.array_equal(mid.astype(np.float64), ((b >> 8) & 0xff) * 256 * ulp) and np.all(mid > 0) and np.all(hi > 0)
    a = fb.sparse_active(n)
    assert len(a) <= 16 and set(fb.SPARSE_REQUIRED + (n - 1,)) <= set(a) and max(a) < n


@pytest.mark.parametrize('V,n,M,scale', fb.SPARSE_CASES)
def test_tolerance_cannot_hide_a_plane_fault(V, n, M, scale):
    """a condition on the inputs and on the recorded C, not a measurement: the largest tolerance of the pinned-sparse comparison
    is at most a quarter of the smallest fault signature over all elements.  With m active units the ratio is about
    2^8 / (C (m + 2)): 12 units keep it above 4 for every allowed C <= 4 whatever the weights are."""
    assert 1 <= fb.C <= 4
    W = fb.sparse_weights(V, n, scale)
    h = fb.pinned_h(n, fb.sparse_active(n), M)
    tol = fb.bound(W, h)
    assert tol.shape == (M, V) and np.all(tol > 0)
    for name, sig in fb.fault_signatures(W, h).items():
        assert sig.shape == (M, V)
        assert tol.max() <= sig.min() / 4.0, '%s: tolerance %.3e against a signature of %.3e (C = %d)' % (name, tol.max(), sig.min(), fb.C)
        assert np.all(fb.bound(W, h, 4) <= sig / 4.0), name    # and element by element at the largest C allowed


def test_recorded_constants_are_consistent():
    """C is twice the measured maximum, rounded up, at most 4; A keeps sigmoid_hw inside the 1e-6 the mode promises for |t| <= 1
    (bm_bf3.h): the condition (A + 1.5) 2^-24 < 1e-6"""
    assert fb.C_MEASURED > 0 and fb.C == max(1, int(np.ceil(2 * fb.C_MEASURED))) and fb.C <= 4
    assert fb.A_MEASURED > 0 and (fb.A_MEASURED + 1.5) * fb.U < 1e-6


def test_train_step_with_zero_rates_is_not_a_no_op_on_the_weights():
    """why the probes run `metrics` and not `train_step(lr = 0)`: the max-norm step of the reference's train op rescales W
    whatever max_norm is (oracle = device, bit for bit: tests/test_dbm_parity_gpu.py)"""
    from oracle import oracle as orc
    V, n, M, scale = fb.SPARSE_CASES[0]
    W = fb.sparse_weights(V, n, scale)
    twin = orc.OracleDBM(V, [n], n_particles=4, batch_size=4, sample_v_states=False, v_unit=1)
    twin.p['W'][...] = W
    twin.set_seed(1)
    twin.train_step(np.zeros((4, V), dtype=np.float32), 0.0, 0.0, 1)
    changed = int(np.sum(fb.bits(twin.p['W']) != fb.bits(W)))
    assert changed > 0
    np.testing.assert_allclose(twin.p['W'], W, rtol=3e-7)
