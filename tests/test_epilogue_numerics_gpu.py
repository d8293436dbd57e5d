"""-m gpu: the scalar functions of csrc/bm_numerics.h and the linear Gaussian epilogue, evaluated ON THE DEVICE over the
whole input range, element by element, through the public ABI (the probes of tests/numerics_probes.py: a one-hot operand
makes a contraction pass the other operand through exactly).

  a. sigmoid (prop-down means of RbmEngine.gibbs): bit for bit against orc_sigmoid and the oracle twin, float64 bounds
  b. the linear epilogue x * sigma + b: two roundings, never a fused multiply-add; denormals pass the matrix cores
  c. the polynomial softplus (free_energy_rows): <= 4 float32 ulp of the exact value
  d. AIS score accumulation (softplus_hw, difference form) at saturated biases: W = 0 telescopes to a closed form
  e. sampling at saturation, default and fast-binary: identical bitmaps

The public call that returns the means is `gibbs` with sample_v_states = False (tests/test_epilogue_numerics.py checks the
same construction on the oracle without a GPU)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import numerics_probes as npb

pytestmark = pytest.mark.gpu

RTOL = 1e-5            # the project's parity bar (tests/test_rbm_ais_gpu.py: RTOL)
N = 128


def run_gibbs(W, vb=None, sigma=None, seed=5, fast=False, **kw):
    """one gibbs step from H0 = onehot on the engine and on its oracle twin -> (V_dev, H_dev, V_twin, H_twin)"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = W.shape
    kw.setdefault('sample_v_states', False)
    kw.setdefault('sample_h_states', False)
    eng = RbmEngine(V, H, max_batch=H, **kw)
    twin = orc.OracleRBM(V, H, **kw)
    vals = dict(W=W, vb=np.zeros(V, dtype=np.float32) if vb is None else vb, hb=np.zeros(H, dtype=np.float32))
    if sigma is not None:
        vals['sigma'] = sigma
    for name, val in vals.items():
        eng.set(name, val)
        twin.p[name][...] = val
    eng.seed(seed); twin.set_seed(seed)
    if fast:
        eng.set_fast_binary(True, everywhere=True)
    Hd, Vd = DeviceArray.from_numpy(npb.onehot(H)), DeviceArray((H, V))          # (a fresh identity for every call)
    eng.gibbs(Hd, Vd, H, 1)
    eng.sync()
    out = Vd.numpy(), Hd.numpy()
    eng.close()
    Ht, Vt = (None, None) if fast else twin.gibbs(npb.onehot(H), 1)
    return out + (Vt, Ht)


def assert_bits(got, want, what):
    bad = npb.bits(got) != npb.bits(want)
    assert not bad.any(), '%s: %d / %d elements differ bitwise, first at %r: %r against %r' % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


@pytest.fixture(scope='module')
def sig_ref():
    """the point set and orc_sigmoid of it, computed once"""
    W = npb.sigmoid_points()
    return W, npb.orc_sigmoid_of(W.T)


# ---- a. the default sigmoid through the prop-down
def test_sigmoid_bit_for_bit_and_float64_bounds(gpu_lib, sig_ref):
    W, want = sig_ref
    Vd, _, Vt, _ = run_gibbs(W)
    assert_bits(Vd, want, 'device sigmoid against orc_sigmoid')
    assert_bits(Vd, Vt, 'device prop-down against the oracle twin')
    npb.check_sigmoid_bounds(W.T, Vd, 'device sigmoid')


def test_sigmoid_of_the_bias_add(gpu_lib, sig_ref):
    W, _ = sig_ref
    b = npb.bias_points()
    Vd, _, Vt, _ = run_gibbs(np.zeros_like(W), vb=b)                              # x + b = 0 + b
    assert_bits(Vd, np.tile(npb.orc_sigmoid_of(b), (N, 1)), 'device sigmoid(0 + vb) against orc_sigmoid')
    assert_bits(Vd, Vt, 'device prop-down against the oracle twin')
    npb.check_sigmoid_bounds(b, Vd[0], 'device sigmoid(0 + vb)')
    Vd, _, Vt, _ = run_gibbs(W, vb=b)                                             # a rounded add in front of the sigmoid
    assert_bits(Vd, npb.orc_sigmoid_of((W.T + b[None, :]).astype(np.float32)), 'device sigmoid(x + vb) against orc_sigmoid')
    assert_bits(Vd, Vt, 'device prop-down against the oracle twin')


@pytest.mark.parametrize('flag', ['dbm_first', 'dbm_last'])
def test_sigmoid_with_a_doubled_pass(gpu_lib, sig_ref, flag):
    """dbm_first doubles the prop-up of the sweep, dbm_last the prop-down (sigmoid(2 x), 2 * 1.7e38 = inf included): the
    prop-down means against the oracle twin, bit for bit"""
    W, want = sig_ref
    Vd, _, Vt, _ = run_gibbs(W, **{flag: True})
    assert_bits(Vd, Vt, 'device prop-down (%s) against the oracle twin' % flag)
    if flag == 'dbm_first':
        assert_bits(Vd, want, 'device sigmoid (dbm_first) against orc_sigmoid')
    else:
        with np.errstate(over='ignore'):
            assert_bits(Vd, npb.orc_sigmoid_of(np.float32(2) * W.T), 'device sigmoid(2 x) against orc_sigmoid')


# ---- b. the linear epilogue and the pass-through of the contraction
def test_linear_epilogue_passes_the_operand_through(gpu_lib, sig_ref):
    from boltzmann_machines_amd import _ffi
    W, _ = sig_ref
    Vd, _, Vt, _ = run_gibbs(W, v_unit=_ffi.UNIT_GAUSSIAN)
    assert np.sum(np.abs(W) == np.float32(1e-40)) >= 2
    nz = W.T != 0
    assert np.array_equal(Vd, W.T), 'values differ (denormals flushed?): %r' % Vd[Vd != W.T][:4]
    assert_bits(Vd[nz], W.T[nz], 'pass-through of the non-zero values, denormals included')
    assert_bits(Vd, Vt, 'device linear epilogue against the oracle twin')


def test_linear_epilogue_is_two_roundings(gpu_lib, sig_ref):
    from boltzmann_machines_amd import _ffi
    W, _ = sig_ref
    sigma = np.linspace(0.5, 1.5, N).astype(np.float32)
    vb = npb.bias_points(seed=3)
    want = ((W.T * sigma[None, :]).astype(np.float32) + vb[None, :]).astype(np.float32)
    fused = (W.T.astype(np.float64) * sigma[None, :].astype(np.float64) + vb[None, :].astype(np.float64)).astype(np.float32)
    assert np.sum(npb.bits(want) != npb.bits(fused)) > 100                       # the points can tell a contracted fma
    Vd, _, Vt, _ = run_gibbs(W, vb=vb, sigma=sigma, v_unit=_ffi.UNIT_GAUSSIAN)
    assert_bits(Vd, want, 'device x * sigma + b against float32(float32(x * sigma) + b)')
    assert_bits(Vd, Vt, 'device linear epilogue against the oracle twin')


# ---- c. the polynomial softplus through the per-row free energy
def test_softplus_polynomial_within_4_ulp(gpu_lib):
    """budget from the operation count: two roundings in s = e / (2 + e), about one ulp for the series, one for 2 s p, one
    for the final add.  The measured maximum is printed (and quoted in DESIGN.md 5)."""
    from boltzmann_machines_amd.engine import RbmEngine, as_device
    P = npb.softplus_points()
    eng = RbmEngine(256, 1, max_batch=16)
    eng.set('vb', np.zeros(256, dtype=np.float32)); eng.set('hb', np.zeros(1, dtype=np.float32))
    Xd = as_device(npb.onehot(256))
    worst, worst_x, worst_abs = 0.0, None, 0.0
    for c in range(16):
        x = P[c]
        eng.set('W', x.reshape(256, 1))
        rows = eng.free_energy_rows(Xd, 256)
        got = -rows.astype(np.float64)
        exact = npb.softplus64(x)
        core = x >= -80.0
        ulps = np.abs(got[core] - exact[core]) / npb.ulp32(exact[core])
        below = np.abs(got[~core] - exact[~core])
        if ulps.max() > worst:
            worst, worst_x = float(ulps.max()), float(x[core][int(np.argmax(ulps))])
        worst_abs = max(worst_abs, float(below.max()) if below.size else 0.0)
        assert ulps.max() <= 4.0, 'column %d: %.2f ulp at x = %r' % (c, ulps.max(), float(x[core][int(np.argmax(ulps))]))
        assert below.size == 0 or below.max() < 2e-35, (c, float(below.max()))
        for r in (0, 112, 240):
            mean = eng.free_energy(Xd, 16, row=r)
            np.testing.assert_allclose(mean, np.mean(rows[r:r + 16].astype(np.float64)), rtol=RTOL)
    print('polynomial softplus on the device: max %.2f ulp (x = %r) over 4096 points with x >= -80, max abs err below %.3e'
          % (worst, worst_x, worst_abs))
    eng.close()


# ---- d. AIS score accumulation at saturated biases (softplus_hw, difference form)
@pytest.mark.parametrize('regime', sorted(npb.AIS_HB))
def test_rbm_ais_telescopes_to_the_closed_form(gpu_lib, regime):
    """W = 0, base_bias = vb: the value of every chain is sum softplus(vb) + sum softplus(hb), whatever it samples - the
    engine's answer is a deterministic measurement of the error accumulated over n_betas softplus_hw differences.
    Measured on an MI355X (worst relative deviation): see DESIGN.md 3.11."""
    from boltzmann_machines_amd.engine import RbmEngine
    vb, hb = npb.AIS_VB, npb.AIS_HB[regime]
    want = npb.closed_form_log_Z(vb, hb)
    eng = RbmEngine(16, 64)
    eng.set('W', np.zeros((16, 64), dtype=np.float32)); eng.set('vb', vb); eng.set('hb', hb)
    for n_betas in (100, 1000, 20000):
        got = eng.ais(n_betas, 16, 1, 31 + n_betas, base_bias=vb).astype(np.float64)
        print('RBM AIS %s, %5d betas: closed form %.9g, worst relative deviation %.3e, spread between chains %.3e'
              % (regime, n_betas, want, np.max(np.abs(got - want)) / abs(want), (got.max() - got.min()) / abs(want)))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
        np.testing.assert_allclose(got, got[0], rtol=RTOL, atol=0)
    eng.close()


def test_dbm_ais_telescopes_to_the_closed_form(gpu_lib):
    """the same construction on a 12-8-6 DBM (zero weights, biases in +-20 on the layers that are summed out); the closed
    form is the enumeration of tests/np_reference_depth.py"""
    from boltzmann_machines_amd.engine import DbmEngine
    from tests import np_reference_depth as rd
    P = npb.dbm_zero_weight_params()
    want = rd.exact_log_Z({k: v.astype(np.float64) for k, v in P.items()}, 2)
    assert want == pytest.approx(npb.closed_form_log_Z(np.concatenate([P['vb'], P['hb_1']]), P['hb']), rel=1e-12)
    eng = DbmEngine(12, [8, 6], n_particles=16, batch_size=16)
    for name, val in P.items():
        eng.set(name, val)
    for n_betas in (100, 1000, 20000):
        got = eng.ais(n_betas, 16, 1, 77 + n_betas).astype(np.float64)
        print('DBM AIS 12-8-6, %5d betas: exact %.9g, worst relative deviation %.3e, spread between chains %.3e'
              % (n_betas, want, np.max(np.abs(got - want)) / abs(want), (got.max() - got.min()) / abs(want)))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
        np.testing.assert_allclose(got, got[0], rtol=RTOL, atol=0)
    eng.close()


def test_dbm_ais_brackets_the_closed_form_with_saturated_chain_biases(gpu_lib):
    """biases in +-20 on EVERY layer of the 12-8-6 stack, the sampled h1 included: the beta b.h1 term of the score at
    saturation.  With the uniform base a chain's value now depends on its samples, so no per-chain closed form holds; the
    estimate of 64 chains x 20 000 betas must bracket the exact log Z by the project's rule max(0.02, 4 sem)
    (tests/test_ais_depth_gpu.py: bracket)."""
    from boltzmann_machines_amd.engine import DbmEngine
    from boltzmann_machines_amd.utils import log_mean_exp, log_std_exp
    P = npb.dbm_zero_weight_params(h1_bias=20.0)
    want = npb.closed_form_log_Z(np.concatenate([P['vb'], P['hb_1']]), P['hb'])
    eng = DbmEngine(12, [8, 6], n_particles=16, batch_size=16)
    for name, val in P.items():
        eng.set(name, val)
    vals = eng.ais(20000, 64, 1, 4711).astype(np.float64)
    eng.close()
    est = log_mean_exp(vals)
    sem = np.exp(log_std_exp(vals) - est) / np.sqrt(len(vals))
    print('DBM AIS 12-8-6, h1 biases in +-20: estimate %.6f exact %.6f sem %.4g, chains in [%.4f, %.4f]'
          % (est, want, sem, vals.min(), vals.max()))
    assert np.all(np.isfinite(vals))
    assert abs(est - want) < max(0.02, 4 * sem), (est, want, sem)


# ---- e. sampling at saturation, default and fast-binary
def test_sampling_at_saturation_default_and_fast_binary(gpu_lib):
    """What this can and cannot see: in the RBM fast-binary mode is legal only with both samplers on, so the RBM ABI never
    returns the means of sigmoid_hw - only the bitmap `u < p`.  (The DBM gates the mode per pass and only asks for sampled
    hidden layers: a one-layer DbmEngine with sample_v_states = False does return them, and
    tests/test_fast_binary_exact_gpu.py holds them to float64 there.)  Above 17.33 a sigmoid_hw that failed to round to 1.0f would lose draws
    with u close to 1 (seen here: all ones is asserted for both paths).  Below -20 a sigmoid_hw that flushed to zero would
    change a draw only where u == 0, which these ~8 000 draws meet with a probability of about 0.1 %: positivity down to -80 is
    NOT established by the bitmap equality, only that no draw decides differently.  That the fast path really ran (and the
    comparison is not the default path against itself) is shown by its own refusal: the same handle rejects hidden states
    that are not a bitmap, which only the fast-binary sweep checks."""
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    W = npb.saturated_points()
    kw = dict(sample_v_states=True, sample_h_states=True)
    Vd, Hd, Vt, Ht = run_gibbs(W, seed=11, **kw)
    assert set(np.unique(Vd)) <= {0.0, 1.0}
    assert_bits(Vd, Vt, 'visible bitmap against the oracle twin')
    assert_bits(Hd, Ht, 'hidden bitmap against the oracle twin')
    assert np.all(Vd[W.T >= 20.0] == 1.0)                         # sigmoid has rounded to 1.0f: u < 1 always
    print('%d of %d draws below -20 came out as 1' % (int(Vd[W.T <= -20.0].sum()), int((W.T <= -20.0).sum())))
    Vf = run_gibbs(W, seed=11, fast=True, **kw)[0]
    assert_bits(Vf, Vd, 'fast-binary visible bitmap against the default path (no draw excluded)')
    assert np.all(Vf[W.T >= 20.0] == 1.0)
    # the same configuration takes the fast-binary sweep: it alone refuses a non-bitmap H
    eng = RbmEngine(N, N, max_batch=N, **kw)
    eng.set('W', W); eng.set('vb', np.zeros(N, dtype=np.float32)); eng.set('hb', np.zeros(N, dtype=np.float32))
    eng.seed(11)
    half = np.full((N, N), 0.5, dtype=np.float32)
    Hh, Vh = DeviceArray.from_numpy(half), DeviceArray((N, N))
    eng.gibbs(Hh, Vh, N, 1)
    eng.sync()                                                     # default path: any H is legal
    eng.set_fast_binary(True, everywhere=True)
    Hh = DeviceArray.from_numpy(half)
    eng.gibbs(Hh, Vh, N, 1)
    with pytest.raises(_ffi.Bm355Error, match='bitmap'):
        eng.sync()
    eng.close()
