"""-m gpu: the float64 engine over the lattice of tests/f64_lattice.py, one case per row, BIT-EXACT against the float64
oracle (parameters, momenta, running means, mean-field mu, particle bitmaps, transform / reconstruction); metrics and free
energy (sums in a device order) at 1e-10 / 1e-12 like the parity files.  A mismatch names the first differing element, the
tile it belongs to and the branch labels of that launch from the path model."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import f64_lattice as lat

pytestmark = pytest.mark.gpu


def dev(a):
    from boltzmann_machines_amd._ffi import DeviceArray
    return DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.float64), np.float64)


def assert_bits(name, got, want, launch=None, bias=None):
    """bit equality; the message points at a branch: `launch` maps a 2-D element (row j, column i) to its tile"""
    bad = np.flatnonzero(got.reshape(-1).view(np.uint64) != want.reshape(-1).view(np.uint64))
    if bad.size == 0:
        return
    e = int(bad[0])
    where = ''
    if launch is not None and got.ndim == 2:
        j, i = divmod(e, got.shape[1])
        where = '; element [%d][%d]: %s' % (j, i, lat.locate(launch, j, i))
    elif bias is not None:
        where = '; column %d, bias job %d of %s' % (e, e // 16, sorted(bias))
    raise AssertionError('%s: %d / %d elements differ bitwise, first at flat index %d (got %r, oracle %r, max abs diff %.3e)%s'
                         % (name, bad.size, got.size, e, float(got.reshape(-1)[e]), float(want.reshape(-1)[e]),
                            float(np.max(np.abs(got - want))), where))


# ------------------------------------------------------------------------------------------------------------- RBM
@pytest.mark.parametrize('c', lat.RBM_LATTICE, ids=[c['id'] for c in lat.RBM_LATTICE])
def test_rbm_lattice_bit_exact_f64(gpu_lib, c):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine64
    V, H, B, k, row, rows = c['V'], c['H'], c['B'], c['k'], c['row'], c['rows']
    kw = dict(c['kw'])
    if c['gaussian']:
        kw['v_unit'] = 1                                     # means only: sample_v_states stays off
    eng = RbmEngine64(V, H, max_batch=B, **kw)
    twin = orc.OracleRBM64(V, H, **kw)
    for nm, val in lat.rbm_params(V, H).items():
        eng.set(nm, val); twin.p[nm][...] = val
    if c['gaussian']:
        eng.set('sigma', lat.rbm_sigma(V)); twin.p['sigma'][...] = lat.rbm_sigma(V)
    eng.seed(lat.RBM_SEED); twin.set_seed(lat.RBM_SEED)
    if row:
        eng.set_row_offset(row); twin.row0 = row
    launches = lat.rbm_launches(V, H, B, k)
    up, grad = launches[-2], launches[-1]
    bias = lat.bias_labels(V, H, B, fused=float(kw.get('sparsity_cost', 0.)) == 0.)
    lr = lat.RBM_LR_GAUSS if c['gaussian'] else lat.RBM_LR
    for s in range(2):
        X = lat.rbm_data(rows, V, s, c['gaussian'])         # the engine reads rows row .. row + B - 1 of the device array
        eng.train_step(dev(X), B, lr, lat.RBM_MOM, k, row=row)
        twin.train_step(X[row:row + B], lr, lat.RBM_MOM, k)
        for n in ('W', 'dW'):                                # W[v][h]: row j = v, column i = h of grad_kernel
            assert_bits('%s after step %d' % (n, s), eng.get(n), twin.p[n], launch=grad)
        for n in ('vb', 'hb', 'dvb', 'dhb', 'q_means'):
            assert_bits('%s after step %d' % (n, s), eng.get(n), twin.p[n], bias=bias)
    X = lat.rbm_data(rows, V, 9, c['gaussian'])
    Xd = dev(X)
    Hd = DeviceArray((B, H), np.float64)
    eng.transform(Xd, B, k, Hd, row=row)
    eng.sync()
    assert_bits('transform', Hd.numpy(), twin.transform(X[row:row + B], k), launch=up)
    np.testing.assert_allclose(eng.metrics(Xd, B, k, row=row), twin.metrics(X[row:row + B], k), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(eng.free_energy(Xd, B, row=row), twin.free_energy(X[row:row + B]), rtol=1e-12)
    eng.close()


# ------------------------------------------------------------------------------------------------------------- DBM
def _dbm_launch_of(name, launches):
    base, _, idx = name.partition('_')
    if not idx.isdigit():
        base, idx = name, '0'
    tag = {'W': 'outer_pos_', 'dW': 'outer_pos_', 'mu': 'mf_sweep_', 'h': 'particles_'}.get(base)
    want = 'particles_v' if name == 'v' else (tag + idx if tag else None)
    for l in launches:
        if l['name'] == want:
            return l
    return None


@pytest.mark.parametrize('c', lat.DBM_LATTICE, ids=[c['id'] for c in lat.DBM_LATTICE])
def test_dbm_lattice_bit_exact_f64(gpu_lib, c):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import DbmEngine64
    V, nh, N, M = c['V'], c['nh'], c['N'], c['M']
    kw = dict(c['kw'])
    if c['gaussian']:
        kw['v_unit'] = 1
    eng = DbmEngine64(V, nh, n_particles=M, batch_size=N, **kw)
    twin = orc.OracleDBM64(V, nh, n_particles=M, batch_size=N, **kw)
    for nm, val in lat.dbm_params(V, nh, M).items():
        eng.set(nm, val); twin.p[nm][...] = val
    if c['gaussian']:
        sig = np.linspace(0.6, 1.4, V)
        eng.set('sigma', sig); twin.p['sigma'][...] = sig
    eng.seed(42); twin.set_seed(42)
    row, rows = c['row'], c['rows']
    if row or c['particle0']:
        eng.set_row_offset(row, c['particle0']); twin.prow0 = c['particle0']
    launches = lat.dbm_launches(V, nh, N, M)
    lr = 1e-3 if c['gaussian'] else 0.05
    X = lat.dbm_data(rows, V, 0, c['gaussian'])             # the engine reads rows row .. row + N - 1 of the device array
    n1, m1 = eng.train_step(dev(X), lr, 0.5, 2, row=row, want_msre=True)
    n2, m2 = twin.train_step(X[row:row + N], lr, 0.5, 2, want_msre=True)
    assert n1 == n2, 'mean-field sweeps: device %d, oracle %d' % (n1, n2)
    cap = kw.get('max_mf_updates', 10)
    assert ('dbm:mf-exit-tol' in c['expect']) == (0 < n1 < cap) and ('dbm:mf-exit-cap' in c['expect']) == (n1 == cap), n1
    np.testing.assert_allclose(m1, m2, rtol=1e-10)
    names = lat.dbm_state_names(nh) + ['W_norm' + ('' if i == 0 else '_%d' % i) for i in range(len(nh))]
    for nm in names:
        assert_bits(nm, eng.get(nm), twin.p[nm], launch=_dbm_launch_of(nm, launches))
    X = lat.dbm_data(rows, V, 5, c['gaussian'])
    n1, m1 = eng.metrics(dev(X), 1, row=row)
    X = X[row:row + N]
    n2, m2 = twin.metrics(X, 1)
    assert n1 == n2
    np.testing.assert_allclose(m1, m2, rtol=1e-10)
    for nm in names:
        assert_bits(nm + ' after metrics', eng.get(nm), twin.p[nm], launch=_dbm_launch_of(nm, launches))
    R = DeviceArray((N, V), np.float64)
    eng.reconstruct(dev(lat.dbm_data(rows, V, 5, c['gaussian'])), R, row=row)
    eng.sync()
    assert_bits('reconstruct', R.numpy(), twin.reconstruct(X), launch=[l for l in launches if l['name'] == 'recon'][0])
    eng.close()
