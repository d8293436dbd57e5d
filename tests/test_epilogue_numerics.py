"""The probe construction and the references of tests/numerics_probes.py, validated without a GPU.

The public call that returns the prop-down MEANS of chosen pre-activations is `OracleRBM.gibbs(H0, 1)` (device:
`RbmEngine.gibbs`) with sample_v_states = False: it returns (H, V) and V holds the means, V[j][i] = act(W[i][j] + vb[i])
for H0 = onehot.  tests/test_epilogue_numerics_gpu.py uses the same call on the engine."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import np_reference_rbm_ais as ra
from tests import numerics_probes as npb


def twin_means(W, vb=None, sigma=None, **kw):
    """V of one oracle gibbs step from H0 = onehot: the prop-down means [H][V]"""
    V, H = W.shape
    kw.setdefault('sample_v_states', False)
    kw.setdefault('sample_h_states', False)
    t = orc.OracleRBM(V, H, **kw)
    t.p['W'][...] = W
    if vb is not None:
        t.p['vb'][...] = vb
    if sigma is not None:
        t.p['sigma'][...] = sigma
    t.set_seed(5)
    return t.gibbs(npb.onehot(H), 1)[1]


def test_point_sets():
    for pts, shape, sp in ((npb.sigmoid_points(), (128, 128), npb.sigmoid_specials()),
                           (npb.softplus_points(), (16, 256), npb.softplus_specials())):
        assert pts.shape == shape and pts.dtype == np.float32 and np.all(np.isfinite(pts))
        have = set(npb.bits(pts).ravel().tolist())
        for s in (sp, npb.tie_points()):
            assert set(npb.bits(s).tolist()) <= have
        assert np.array_equal(npb.bits(pts), npb.bits(npb.sigmoid_points() if shape[0] == 128 else npb.softplus_points()))
        rest = np.abs(pts)
        assert rest.min() == 0 and np.sum((rest > 0) & (rest < 1e-6)) > 100 and np.sum((rest > 80) & (rest < 181)) > 100
    # the ties really straddle a change of n in the reduction
    t = npb.tie_points()[:5 * 116].reshape(116, 5)
    q = t.astype(np.longdouble) / npb.LN2 - np.arange(116)[:, None]
    assert np.all(q[:, 1] < 0.5) and np.all(q[:, 3] > 0.5) and np.all(np.diff(q, axis=1) > 0)
    assert np.all(np.abs(q[:, 2] - 0.5) <= np.minimum(0.5 - q[:, 1], q[:, 3] - 0.5))
    sat = npb.saturated_points()
    assert sat.shape == (128, 128) and np.abs(sat).min() >= 20 and np.abs(sat).max() <= 80
    assert set(npb.bits(npb.neighbours(80.0)[:3]).tolist()) <= set(npb.bits(sat).ravel().tolist())


def test_probe_passes_sigmoid_through_bit_for_bit():
    W = npb.sigmoid_points()
    V = twin_means(W)
    assert np.array_equal(npb.bits(V), npb.bits(npb.orc_sigmoid_of(W.T)))
    b = npb.bias_points()
    V = twin_means(np.zeros_like(W), vb=b)
    assert np.array_equal(npb.bits(V), npb.bits(np.tile(npb.orc_sigmoid_of(b), (128, 1))))


def test_probe_passes_linear_epilogue_through():
    W = npb.sigmoid_points()
    V = twin_means(W, v_unit=1)
    assert np.array_equal(V, W.T)                                   # (== : up to the sign of zero)
    nz = W.T != 0
    assert np.array_equal(npb.bits(V)[nz], npb.bits(W.T)[nz])       # denormals included
    sigma = np.linspace(0.5, 1.5, 128).astype(np.float32)
    vb = npb.bias_points(seed=3)
    want = ((W.T * sigma[None, :]).astype(np.float32) + vb[None, :]).astype(np.float32)      # two roundings
    assert np.array_equal(npb.bits(twin_means(W, vb=vb, sigma=sigma, v_unit=1)), npb.bits(want))


def test_oracle_sigmoid_meets_the_float64_bounds_on_the_probe_points():
    x = npb.sigmoid_points()
    npb.check_sigmoid_bounds(x, npb.orc_sigmoid_of(x), 'orc_sigmoid')
    x = np.concatenate([npb.softplus_points().ravel(), npb.bias_points(), npb.bias_points(seed=3)])
    npb.check_sigmoid_bounds(x, npb.orc_sigmoid_of(x), 'orc_sigmoid (second sets)')


def test_references():
    xs = np.float64([0., 1e-40, 1., 17.33, 80., 103.97, 800.])
    x = np.concatenate([-xs[::-1], xs])
    s, p = npb.sigmoid64(x), npb.softplus64(x)
    assert s[0] == 0. and s[-1] == 1. and np.all(s[5:9] == 0.5)
    lo = x[1:6]                                                                   # -103.97 .. -1: no cancellation in e / (1 + e)
    np.testing.assert_allclose(s[1:6], np.exp(lo) / (1. + np.exp(lo)), rtol=1e-15)
    np.testing.assert_allclose(s + s[::-1], 1., rtol=1e-15)
    np.testing.assert_allclose(p - p[::-1], x, rtol=1e-15, atol=1e-16)          # softplus(x) - softplus(-x) = x
    np.testing.assert_allclose(p[1:3], np.exp(x[1:3]), rtol=1e-15)                # log1p(e) = e far below
    assert p[6] == np.log(2.) and p[0] == 0. and p[-1] == 800.
    assert npb.closed_form_log_Z([0., 0.], [0.]) == pytest.approx(3 * np.log(2.), rel=1e-15)
    assert np.array_equal(npb.ulp32([1., 3., 1e-40]), [2. ** -23, 2. ** -22, 2. ** -149])


@pytest.mark.parametrize('regime', sorted(npb.AIS_HB))
@pytest.mark.parametrize('n_betas', [100, 1000])
def test_float64_ais_twin_telescopes_to_the_closed_form(regime, n_betas):
    """W = 0 and base_bias = vb: every chain's log-weight is sum_j softplus(hb_j) - H log 2 whatever it samples"""
    hb, vb = npb.AIS_HB[regime], npb.AIS_VB
    P = dict(W=np.zeros((16, 64), dtype=np.float32), vb=vb, hb=hb)
    vals, _ = ra.ais(P, n_betas, 16, 1, 31, base_bias=vb)
    np.testing.assert_allclose(vals, npb.closed_form_log_Z(vb, hb), rtol=1e-12, atol=0)


@pytest.mark.parametrize('h1_bias', [0.0, 20.0])
def test_dbm_enumeration_equals_the_closed_form(h1_bias):
    """the 12-8-6 stack of part d: the enumerator of tests/np_reference_depth.py against the sum of softplus(b) over all units"""
    from tests import np_reference_depth as rd
    P = npb.dbm_zero_weight_params(h1_bias=h1_bias)
    exact = rd.exact_log_Z({k: v.astype(np.float64) for k, v in P.items()}, 2)
    closed = npb.closed_form_log_Z(np.concatenate([P['vb'], P['hb_1']]), P['hb'])
    assert exact == pytest.approx(closed, rel=1e-12)
