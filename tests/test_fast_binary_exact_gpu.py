"""-m gpu: the fast-binary contraction (csrc/bm_bf3.h: split3_kernel, act_bf3_kernel, the HWMATH epilogue) against float64,
element by element, through the public ABI.  The observation route, the point sets and the tolerances are those of
tests/fast_binary_probes.py (conditions on them: tests/test_fast_binary_exact.py):

  1. pass-through, bitwise: one pinned hidden unit k0 and Gaussian visibles return W[:, k0] - 0 + hi + mid + lo has no rounding
  2. pinned-sparse against float64: structured weights whose lo plane is maximal - a lost or shifted plane is >= 4 tolerances
  3. dense against float64, up to a shape whose strips are uneven and hold several tiles in every geometry
  4. the means of sigmoid_hw against float64
  5. 1 - 3 and the two-segment kernels with every bf16 tile geometry forced (BM355_DEBUG=bf3_geo, one child process each)

The check functions are plain functions: the tests call them with the launcher's own choice of geometry, the child processes
of 5 with a forced one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fast_binary_probes as fb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSSIAN, BERNOULLI = 1, 0
RATIOS = []                            # err / ((m + 2) 2^-24 S) of every float64 comparison of this process


def sweep(eng, W, hb, v0, vb=None):
    """one particle sweep on `eng` from the particles v0 -> (v, h): see tests/fast_binary_probes.py.  W is what the planes were
    built from: it must come back bitwise unchanged."""
    from boltzmann_machines_amd.engine import as_device
    V, n = W.shape
    eng.set('W', W); eng.set('hb', hb); eng.set('vb', np.zeros(V, dtype=np.float32) if vb is None else vb)
    eng.set('v', v0); eng.set('h', np.zeros((eng.M, n), dtype=np.float32))
    eng.metrics(as_device(np.zeros((eng.N, V), dtype=np.float32)), 1)
    v, h = eng.get('v'), eng.get('h')
    assert np.array_equal(fb.bits(eng.get('W')), fb.bits(W)), 'W changed under the sweep'
    assert set(np.unique(h)) <= {0.0, 1.0}
    return v, h


def engine(V, n, M, v_unit, fast, seed=5):
    from boltzmann_machines_amd.engine import DbmEngine
    eng = DbmEngine(V, [n], v_unit=v_unit, sample_v_states=False, n_particles=M, batch_size=4, max_mf_updates=1)
    eng.seed(seed)
    eng.set_fast_binary(fast, everywhere=True)
    return eng


def first_bad(bad, got, want):
    i = tuple(np.argwhere(bad)[0])
    return '%d / %d elements, first at %r: %r against %r' % (int(bad.sum()), bad.size, i, got[i], want[i])


# ---- 1. pass-through
def check_pass_through(V, n, M, k0):
    """every chunk of the point set whose index is k0's turn, as column k0 of W; the other columns hold non-zero filler"""
    turn = fb.pass_k0(n).index(k0)
    rows = fb.chunks(fb.pass_through_points(), V)[turn::len(fb.pass_k0(n))]
    hb, v0 = fb.pinned_hb(n, [k0]), np.zeros((M, V), dtype=np.float32)
    fast, default = engine(V, n, M, GAUSSIAN, True), engine(V, n, M, GAUSSIAN, False)
    W = fb.filler(V, n, k0)
    for pts in rows:
        W[:, k0] = pts
        v, h = sweep(fast, W, hb, v0)
        assert np.array_equal(h, fb.pinned_h(n, [k0], M)), 'h is not pinned to unit %d' % k0
        want = np.tile(pts, (M, 1))
        bad = fb.bits(v) != fb.bits(want)
        assert not bad.any(), 'fast-binary pass-through of W[:, %d]: %s' % (k0, first_bad(bad, v, want))
        vd, hd = sweep(default, W, hb, v0)
        assert np.array_equal(hd, h)
        bad = fb.bits(v) != fb.bits(vd)
        assert not bad.any(), 'fast-binary against the default path: %s' % first_bad(bad, v, vd)
    fast.close(); default.close()
    return len(rows) * V


@pytest.mark.parametrize('V,n,M,k0', [(V, n, M, k0) for V, n, M in fb.PASS_SHAPES for k0 in fb.pass_k0(n)])
def test_pass_through_is_bitwise(gpu_lib, V, n, M, k0):
    assert check_pass_through(V, n, M, k0) >= 3000


# ---- 2. and 3. against float64
def check_against_float64(W, hb, v0, what, required=(), max_active=None):
    V, n = W.shape
    M = v0.shape[0]
    eng = engine(V, n, M, GAUSSIAN, True)
    v, h = sweep(eng, W, hb, v0)
    eng.close()
    active = np.count_nonzero(h, axis=1)
    if max_active is not None:
        assert np.all(h[:, list(required)] == 1.0) and active.max() <= max_active, (what, active.max())
    ratio = fb.err_ratio(v, W, h)
    RATIOS.append(ratio)
    print('%s: max |err| / ((m + 2) 2^-24 S) = %.4f (m = %d .. %d active units per row)' % (what, ratio, active.min(), active.max()))
    err = np.abs(v.astype(np.float64) - fb.ref64(W, h))
    bad = err > fb.bound(W, h)
    assert not bad.any(), '%s, C = %d: %s' % (what, fb.C, first_bad(bad, v, fb.ref64(W, h)))
    return v, h


def check_sparse(V, n, M, scale):
    W, a = fb.sparse_weights(V, n, scale), fb.sparse_active(n)
    return check_against_float64(W, fb.pinned_hb(n, a), np.zeros((M, V), dtype=np.float32),
                                 'pinned-sparse %d x %d, %d particles' % (V, n, M), required=a, max_active=16)


@pytest.mark.parametrize('V,n,M,scale', fb.SPARSE_CASES)
def test_pinned_sparse_against_float64(gpu_lib, V, n, M, scale):
    check_sparse(V, n, M, scale)


def check_dense(V, n, M):
    W, hb, v0 = fb.dense_inputs(V, n, M)
    v, h = check_against_float64(W, hb, v0, 'dense %d x %d, %d particles' % (V, n, M))
    if (V, n, M) == fb.DENSE_DISTINCT:                 # the fast path ran: the default path's chain rounds elsewhere
        eng = engine(V, n, M, GAUSSIAN, False)
        vd, hd = sweep(eng, W, hb, v0)
        eng.close()
        assert np.array_equal(hd, h)                   # (h is sampled on the fp32 path in both modes)
        assert np.any(fb.bits(vd) != fb.bits(v)), 'fast-binary v is bit-identical to the default path: the bf16 kernel did not run'
    return v, h


@pytest.mark.parametrize('V,n,M', fb.DENSE_CASES)
def test_dense_against_float64(gpu_lib, V, n, M):
    v, h = check_dense(V, n, M)
    if n > 1:
        assert 0 < h.mean() < 1                        # sampled freely


# ---- 4. sigmoid_hw
def sigmoid_means(W, hb, vb, fast):
    V, n = W.shape
    eng = engine(V, n, 4, BERNOULLI, fast)
    v, h = sweep(eng, W, hb, np.zeros((4, V), dtype=np.float32), vb=vb)
    eng.close()
    return v, h


def test_sigmoid_hw_means_against_float64(gpu_lib):
    """W = 0: the argument is exactly vb_i; then one pinned unit with vb = 0: the argument is exactly W[i, k0] (test 1)"""
    t = fb.sigmoid_hw_points()
    V, n, k0 = len(t), 8, 3
    measured = []
    v, h = sigmoid_means(np.zeros((V, n), dtype=np.float32), np.zeros(n, dtype=np.float32), t, True)
    assert np.all(fb.bits(v) == fb.bits(v[0])[None, :])
    measured.append(fb.check_sigmoid_hw(t, v[0], 'sigmoid_hw(0 + vb)'))
    vd, _ = sigmoid_means(np.zeros((V, n), dtype=np.float32), np.zeros(n, dtype=np.float32), t, False)
    assert np.any(fb.bits(vd) != fb.bits(v)), 'the means equal the default sigmoid bit for bit: sigmoid_hw did not run'
    tw = t[fb.in_range(t)]
    W = fb.filler(len(tw), n, 2)
    W[:, k0] = tw
    v, h = sigmoid_means(W, fb.pinned_hb(n, [k0]), None, True)
    assert np.array_equal(h, fb.pinned_h(n, [k0], 4))
    assert np.all(fb.bits(v) == fb.bits(v[0])[None, :])
    measured.append(fb.check_sigmoid_hw(tw, v[0], 'sigmoid_hw(W[:, k0] + 0)'))
    vd, _ = sigmoid_means(W, fb.pinned_hb(n, [k0]), None, False)
    assert np.any(fb.bits(vd) != fb.bits(v))
    print('sigmoid_hw: measured A = %.3f (recorded: %.3f)' % (max(measured), fb.A_MEASURED))


# ---- 5. every bf16 geometry, forced
def check_two_segment():
    """the two-segment strip kernel (and the transposed planes W3t) feed samplers only: bitmaps against the default path under
    the bar of tests/test_fast_binary_gpu.py, unchanged"""
    from tests import test_fast_binary_gpu as F
    F.test_pcd_sweeps_match_the_default_path_up_to_ties(None, 70, [33, 9], 4, 17, {}, 2)
    F.test_pcd_sweeps_match_the_default_path_up_to_ties(None, 64, [128, 72], 4, 80, {}, 2)


def run_forced():
    """what a child process of test 5 runs (BM355_DEBUG is read once per process)"""
    for V, n, M in fb.PASS_SHAPES:
        for k0 in fb.pass_k0(n):
            check_pass_through(V, n, M, k0)
    for case in fb.SPARSE_CASES:
        check_sparse(*case)
    for case in fb.DENSE_CASES:
        check_dense(*case)
    check_two_segment()
    print('max ratio %.4f' % max(RATIOS))
    print('BF3_GEOMETRY_OK')


SCRIPT = 'import sys; sys.path.insert(0, %r); from tests import test_fast_binary_exact_gpu as T; T.run_forced()'


@pytest.mark.parametrize('geo', ['2', '4', '8'])
def test_forced_bf16_geometry(gpu_lib, geo):
    """2: 64 x 32 tiles, two workgroups per CU; 4: 64 x 64; 8: 128 x 32 with 8 waves (bm_launch.h launch_act_bf3_as)"""
    env = dict(os.environ, BM355_DEBUG='bf3_geo=' + geo)
    r = subprocess.run([sys.executable, '-c', SCRIPT % ROOT], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and 'BF3_GEOMETRY_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_measured_constant_is_the_recorded_one(gpu_lib):
    """the maximum over the float64 comparisons this process has run so far (the whole module: all of tests 2 and 3), against
    what fast_binary_probes.py and DESIGN.md 3.9 record"""
    if not RATIOS:
        check_dense(*fb.DENSE_DISTINCT)
    print('fast-binary contraction: measured C = max |err| / ((m + 2) 2^-24 S) = %.4f over %d cases (recorded: %.4f, asserted: %d)'
          % (max(RATIOS), len(RATIOS), fb.C_MEASURED, fb.C))
    assert max(RATIOS) <= fb.C
