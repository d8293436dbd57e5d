"""-m gpu: the float64 engine's own numerics against long double, at the edges where they can break.

sigmoid (exp_neg): a one-hidden-layer DbmEngine64 on one-hot rows with hb = 0 and one mean-field sweep.  Row r has its
single 1 in column r, so every pre-activation chain has ONE non-zero product, W[r][h] * 1: no rounding before the
sigmoid.  The initial pass (mult 2) leaves sigmoid(2 W[r][h]) in mu_new, the sweep sigmoid(W[r][h]) in mu.
softplus (free_energy_kernel): RbmEngine64.free_energy of row r of a device identity matrix with H = 1, vb = hb = 0 is
-softplus(W[r][0]).
max-norm (dmaxnorm_kernel): zero column, a column under the 1e-8 floor, a clipped column, with lr = 0."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import f64_lattice as lat

pytestmark = pytest.mark.gpu


def dev(a):
    from boltzmann_machines_amd._ffi import DeviceArray
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.float64), np.float64)


def _first_bad(got, want):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    return bad


def test_sigmoid_device_bit_equal_to_oracle_and_4ulp_of_long_double(gpu_lib):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import DbmEngine64
    L = orc.lib()
    orc.OracleRBM64(2, 2)                                   # registers the double signatures
    V = N = 64
    x = lat.sigmoid_probes()
    H = (x.size + V - 1) // V
    W = np.zeros(V * H)
    W[:x.size] = x
    W = W.reshape(V, H)
    eng = DbmEngine64(V, [H], n_particles=1, batch_size=N, max_mf_updates=1, mf_tol=1e-7)
    eng.set('W', W); eng.set('hb', 0.0); eng.set('mu', 0.0)
    out = DeviceArray((N, H), np.float64)
    assert eng.mean_field(dev(np.eye(V)), out=out) == 1
    eng.sync()
    for what, got, arg in (('sigmoid(w)', out.numpy(), W), ('sigmoid(2 w)', eng.get('mu_new'), 2.0 * W)):
        got, arg = got.reshape(-1), arg.reshape(-1)
        want = np.array([L.orc_sigmoid_d(float(v)) for v in arg])
        bad = _first_bad(got, want)
        assert bad.size == 0, '%s: %d / %d differ from orc_sigmoid_d, first at x = %r (n = rint(-|x| / ln 2) = %d): device %r, ' \
            'oracle %r' % (what, bad.size, got.size, float(arg[bad[0]]), int(np.rint(-min(abs(arg[bad[0]]), 700.) / np.log(2.))),
                           float(got[bad[0]]), float(want[bad[0]]))
        err = lat.ulp_error(got, lat.sigmoid_exact(arg))
        i = int(np.argmax(err))
        print('%s on the device: max %.3f ulp at x = %r over %d points' % (what, float(err[i]), float(arg[i]), got.size))
        assert float(err[i]) <= 4.0
    eng.close()


def test_softplus_device_against_long_double(gpu_lib):
    """the device uses the GPU math library's exp and log1p: not bit-equal to the host.  E = the error of the same formula
    under the host libm on these points (ulps of the exact value); the device may be 4 * max(E, 1): two library calls, each
    allowed about one ulp more than the host's.  Below the smallest normal: 2**-1022 absolute."""
    from boltzmann_machines_amd.engine import RbmEngine64
    x = lat.softplus_probes()
    n = x.size
    eng = RbmEngine64(n, 1, max_batch=1)
    eng.set('W', x.reshape(n, 1)); eng.set('vb', 0.0); eng.set('hb', 0.0)
    Xd = dev(np.eye(n))
    got = np.array([-eng.free_energy(Xd, 1, row=r) for r in range(n)])
    eng.close()
    exact = lat.softplus_exact(x)
    E = lat.softplus_host_error()
    normal = exact >= lat.TINY
    err = lat.ulp_error(got[normal], exact[normal])
    i = int(np.argmax(err))
    print('softplus: host libm E = %.3f ulp; device max %.3f ulp at x = %r over %d points; %d subnormal-range points, max abs '
          'error there %.3e' % (E, float(err[i]), float(x[normal][i]), int(normal.sum()), int((~normal).sum()),
                                float(np.max(np.abs(got[~normal].astype(np.longdouble) - exact[~normal])))))
    assert float(err[i]) <= 4.0 * max(E, 1.0)
    assert np.all(np.abs(got[~normal].astype(np.longdouble) - exact[~normal]) <= lat.TINY)


def test_max_norm_edges_f64(gpu_lib):
    """bit-exact to the oracle and within 2 ulp of the long-double W * min(n, c) / max(n, 1e-8)"""
    from boltzmann_machines_amd.engine import DbmEngine64
    V, nh, N, M = lat.MAXNORM_SHAPE
    eng = DbmEngine64(V, nh, n_particles=M, batch_size=N, max_norm=lat.MAXNORM_LIMIT)
    twin = orc.OracleDBM64(V, nh, n_particles=M, batch_size=N, max_norm=lat.MAXNORM_LIMIT)
    P = lat.maxnorm_edge_params()
    for nm, val in P.items():
        eng.set(nm, val); twin.p[nm][...] = val
    eng.seed(42); twin.set_seed(42)
    X = lat.dbm_data(N, V, 0)
    assert eng.train_step(dev(X), 0.0, 0.5, 1)[0] == twin.train_step(X, 0.0, 0.5, 1)[0]
    for nm, nn in (('W', 'W_norm'), ('W_1', 'W_norm_1')):
        g, gn = eng.get(nm), eng.get(nn)
        for what, a, b in ((nm, g, twin.p[nm]), (nn, gn, twin.p[nn])):
            bad = _first_bad(a.reshape(-1), b.reshape(-1))
            assert bad.size == 0, '%s: %d elements differ from the oracle, first at %d' % (what, bad.size, int(bad[0]))
        n, Wx = lat.maxnorm_exact(P[nm])
        assert gn[0] == 0.0 and float(np.max(lat.ulp_error(gn[1:], n[1:]))) <= 2.0
        nz = Wx != 0
        assert float(np.max(lat.ulp_error(g[nz], Wx[nz]))) <= 2.0
        assert np.all(g[:, 0] == 0.0)                                                   # 0 * 0 / 1e-8
        np.testing.assert_allclose(g[:, 1], 1e-10 * float(n[1]) / 1e-8, rtol=1e-15)     # the floor, not the norm
        np.testing.assert_allclose(float(np.sqrt(np.sum(g[:, 2].astype(np.longdouble) ** 2))), lat.MAXNORM_LIMIT, rtol=1e-15)
    eng.close()
