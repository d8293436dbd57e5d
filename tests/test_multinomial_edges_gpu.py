"""-m gpu: the three device implementations of the Multinomial layer (softmax_multinomial_kernel in float32 - RBM and DBM -
and float64, mn_hhat_kernel in both widths) at the edges.  Every test asserts two things on the same device output: it is
bit-identical to the oracle twin, and it meets the float64 bounds and exact count checks of tests/multinomial_probes.py
directly (a mistake mirrored in kernel and oracle would pass the first alone).  tests/test_multinomial_edges.py is the
proof, without a GPU, that the oracle passes each of these assertions with the same sets and seeds.  8 rows everywhere; the
largest launch is 8 x 8192."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import multinomial_probes as mp

pytestmark = pytest.mark.gpu

SEED = 7
R = mp.ROWS


def limits():
    """what bm_rbm_multinomial_limit / bm_rbm64_multinomial_limit report (a query, no launch) -> {prec name: int64[4]}"""
    from boltzmann_machines_amd import _ffi
    lib = _ffi.load()
    out = {}
    for prec, fn in ((mp.F32, lib.bm_rbm_multinomial_limit), (mp.F64, lib.bm_rbm64_multinomial_limit)):
        q = (C.c_int64 * 4)()
        _ffi.check(fn(q))
        out[prec.name] = [int(x) for x in q]
    return out


class Probe(object):
    """a V_PROBE x I Multinomial RBM with W = 0 on the device: the logits of every row are hb"""

    def __init__(self, I, M, prec=mp.F32, sample_h_states=True):
        from boltzmann_machines_amd import _ffi
        from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
        self.I, self.M, self.prec, self.sample_h = I, M, prec, sample_h_states
        self.eng = (RbmEngine if prec is mp.F32 else RbmEngine64)(
            mp.V_PROBE, I, max_batch=R, h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=M, sample_h_states=sample_h_states)
        self.eng.set('W', np.zeros((mp.V_PROBE, I)))

    def twin(self, l, row0=0):
        return mp.twin_rbm(self.I, self.M, l, self.prec, SEED, row0, self.sample_h)

    def means(self, l):
        from boltzmann_machines_amd._ffi import DeviceArray
        dt = self.prec.dtype
        self.eng.set('hb', l); self.eng.seed(SEED)
        Xd, Hd = DeviceArray.from_numpy(mp.probe_x(R, dt), dt), DeviceArray((R, self.I), dt)
        self.eng.transform(Xd, R, 1, Hd)
        self.eng.sync()
        return Hd.numpy()

    def counts(self, l, row0=0):
        from boltzmann_machines_amd._ffi import DeviceArray
        self.eng.set('hb', l); self.eng.seed(SEED); self.eng.set_row_offset(row0)
        Hd, Vd = DeviceArray.from_numpy(np.zeros((R, self.I), dtype=np.float32)), DeviceArray((R, mp.V_PROBE))
        self.eng.gibbs(Hd, Vd, R, 1)
        self.eng.sync()
        return Hd.numpy()

    def close(self):
        self.eng.close()


# ---- RbmEngine (float32)
@pytest.mark.parametrize('I', mp.WIDTHS)
def test_rbm_means_every_width_and_family(gpu_lib, I):
    worst = 0.0
    for M in mp.N_SAMPLES:
        p = Probe(I, M)
        for name, l in mp.logit_sets(I):
            got = p.means(l)
            mp.assert_bits(got, mp.twin_means(p.twin(l)), 'device means against the twin, %s I=%d M=%d' % (name, I, M))
            worst = max(worst, mp.check_means(l, got, M, what='device ' + name))
        p.close()
    print('device float32 I=%d: largest error / bound %.3f' % (I, worst))


def test_rbm_counts_every_width_and_family(gpu_lib):
    tally = mp.Tally()
    for I in mp.WIDTHS:
        for M in mp.N_SAMPLES:
            p = Probe(I, M)
            for name, l in mp.logit_sets(I):
                got = p.counts(l)
                mp.assert_bits(got, mp.twin_counts(p.twin(l)), 'device counts against the twin, %s I=%d M=%d' % (name, I, M))
                tally.add(l, got, M, mp.F32, name, 'device ' + name)
            p.close()
    assert len(tally.assert_statistical_leg()) >= 30


def test_rbm_n_samples_far_above_the_width(gpu_lib):
    I, M = 64, 100000
    p, tally = Probe(I, M), mp.Tally()
    for name, l in mp.logit_sets(I):
        got = p.means(l)
        mp.assert_bits(got, mp.twin_means(p.twin(l)), 'device means against the twin, ' + name)
        mp.check_means(l, got, M, what='device ' + name)
        got = p.counts(l)
        mp.assert_bits(got, mp.twin_counts(p.twin(l)), 'device counts against the twin, ' + name)
        tally.add(l, got, M, mp.F32, name, 'device ' + name)
    p.close()
    assert len([r for r in tally.rows if r[5] >= 10]) >= 4


@pytest.mark.parametrize('I', [1, 65, 8192])
def test_rbm_states_equal_means_without_sampling(gpu_lib, I):
    p = Probe(I, 100, sample_h_states=False)
    for name, l in mp.logit_sets(I):
        h = p.counts(l)
        mp.assert_bits(h, p.means(l), 'device states against device means, ' + name)
        mp.assert_bits(h, mp.twin_counts(p.twin(l)), 'device states against the twin, ' + name)
        mp.check_means(l, h, 100, what='device states (no sampling) ' + name)
    p.close()


def test_rbm_draw_index_beyond_2_pow_33(gpu_lib):
    """(row0 + row) * M + d > 2^34: the high word of the Philox block counter is non-zero"""
    I, M = 65, 3
    l = dict(mp.logit_sets(I))['a_normal']
    p = Probe(I, M)
    far = p.counts(l, row0=2 ** 33)
    base = p.counts(l, row0=0)
    p.close()
    mp.assert_bits(far, mp.twin_counts(p.twin(l, row0=2 ** 33)), 'device counts at row offset 2^33 against the twin')
    mp.assert_bits(base, mp.twin_counts(p.twin(l)), 'device counts at row offset 0 against the twin')
    mp.check_counts(l, far, M, what='row offset 2^33')
    assert not np.array_equal(far, base), 'the row offset is dropped'


# ---- the width limit
def test_width_limit_is_what_the_runtime_allows(gpu_lib):
    """create accepts exactly the widths whose softmax row fits the dynamic LDS the runtime grants the kernel (measured on an
    MI355X, ROCm 7.2: 163840 bytes per workgroup without any opt-in, static 0 - DESIGN.md 5), capped at 8192"""
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import DbmEngine, RbmEngine, RbmEngine64
    lim = limits()
    for prec, E in ((mp.F32, RbmEngine), (mp.F64, RbmEngine64)):
        per_block, static, dyn, widest = lim[prec.name]
        print('%s: MaxSharedMemoryPerBlock %d, static LDS %d, dynamic LDS a launch may ask for %d -> n_hidden <= %d'
              % (prec.name, per_block, static, dyn, widest))
        size = 2 * np.dtype(prec.dtype).itemsize
        assert widest == min(8192, dyn // size) and widest * size <= dyn <= per_block - static
        assert widest >= 1
        kw = dict(max_batch=R, h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=3)
        E(mp.V_PROBE, widest, **kw).close()
        with pytest.raises(_ffi.Bm355Error, match='n_hidden %d > %d' % (widest + 1, widest)):
            E(mp.V_PROBE, widest + 1, **kw)
    widest = lim['float32'][3]
    kw = dict(n_particles=R, batch_size=R, h_units=[0, _ffi.UNIT_MULTINOMIAL], n_samples=[0, 3])
    DbmEngine(mp.V_PROBE, [4, widest], **kw).close()
    with pytest.raises(_ffi.Bm355Error, match='%d units > %d' % (widest + 1, widest)):
        DbmEngine(mp.V_PROBE, [4, widest + 1], **kw)


# ---- RbmEngine64
def widths64():
    return mp.WIDTHS64 + ('limit',)


@pytest.mark.parametrize('I', widths64())
def test_rbm64_means(gpu_lib, I):
    """float64 means, bit for bit and within the float64 bound; the widest row the create call accepts included (its 16
    bytes per unit are more than 64 KiB of dynamic LDS from 4097 units on).  The float64 ABI returns no hidden states: its
    counts are reached through the train step of test_hhat_and_the_stream_after_it only"""
    if I == 'limit':
        I = limits()['float64'][3]
    worst = 0.0
    for M in mp.N_SAMPLES:
        p = Probe(I, M, mp.F64)
        for name, l in mp.logit_sets(I, mp.F64):
            got = p.means(l)
            mp.assert_bits(got, mp.twin_means(p.twin(l)), 'device float64 means against the twin, %s I=%d M=%d' % (name, I, M))
            worst = max(worst, mp.check_means(l, got, M, mp.F64, 'device ' + name))
        p.close()
    print('device float64 I=%d: largest error / bound %.3f' % (I, worst))


# ---- mn_hhat_kernel, both widths
@pytest.mark.parametrize('prec', [mp.F32, mp.F64], ids=['float32', 'float64'])
@pytest.mark.parametrize('K', [1, 2, 8192])
@pytest.mark.parametrize('M', [1, 100000])
def test_hhat_and_the_stream_after_it(gpu_lib, prec, K, M):
    """free_energy draws h_hat ~ Multinomial(M, uniform over K) on the device: against the twin to the existing tolerance,
    and one more train step is still bit-identical (the stream advanced alike on both sides; the step's v pass consumes
    the sampled counts of the softmax kernel)"""
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine, RbmEngine64
    V, B, dt = 6, R, prec.dtype
    K = min(K, limits()[prec.name][3])
    kw = dict(h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=M, sample_v_states=True, sample_h_states=True)
    eng = (RbmEngine if prec is mp.F32 else RbmEngine64)(V, K, max_batch=B, **kw)
    twin = (orc.OracleRBM if prec is mp.F32 else orc.OracleRBM64)(V, K, **kw)
    W = (orc.normal(87654321, 3, 0, V * K) * np.float32(0.1)).reshape(V, K).astype(dt)
    hb = ((orc.uniform(87654321, 13, 0, K) - np.float32(0.5)) * np.float32(0.4)).astype(dt)
    for name, val in (('W', W), ('hb', hb)):
        eng.set(name, val); twin.p[name][...] = val
    eng.seed(SEED); twin.set_seed(SEED)
    X = (orc.uniform(87654321, 99, 0, B * V) < 0.4).astype(dt).reshape(B, V)
    Xd = DeviceArray.from_numpy(X, dt)
    fe, want = eng.free_energy(Xd, B), twin.free_energy(X)
    print('%s K=%d M=%d: free energy %.9g, twin %.9g' % (prec.name, K, M, fe, want))
    np.testing.assert_allclose(fe, want, rtol=2e-5 if prec is mp.F32 else 1e-12, atol=0)
    eng.train_step(Xd, B, 0.05, 0.5, 1)
    twin.train_step(X, 0.05, 0.5, 1)
    eng.sync()
    for name in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb'):
        mp.assert_bits(eng.get(name), twin.p[name], '%s after free_energy + train_step' % name)
    eng.close()


# ---- inside the DBM
def dbm_pair(widths, **kw):
    from boltzmann_machines_amd.engine import DbmEngine
    hu, ns, P = mp.dbm_layers(widths)
    kw = dict(n_particles=R, batch_size=R, h_units=hu, n_samples=ns, max_mf_updates=10, mf_tol=1e-7, **kw)
    eng, twin = DbmEngine(mp.V_PROBE, list(widths), **kw), orc.OracleDBM(mp.V_PROBE, list(widths), **kw)
    for name, val in P.items():
        eng.set(name, val); twin.p[name][...] = val
    eng.seed(SEED); twin.set_seed(SEED)
    return eng, twin, hu, ns, P


@pytest.mark.parametrize('widths', [(63, 64, 65), (65, 64, 63), (64, 65)], ids=str)
def test_dbm_layers_with_zero_weights(gpu_lib, widths):
    """Multinomial layers first and last at widths that are not their pitch; W = 0, so the means are the same in every
    sweep and the mean-field residual is exactly 0 (the kernel's atomicMax is skipped): same trip count, mu bit for bit and
    within the bound, h particles bit for bit and through the count checks"""
    from boltzmann_machines_amd.engine import as_device
    eng, twin, hu, ns, P = dbm_pair(widths)
    X = mp.probe_x(R)
    n_dev, n_twin = eng.mean_field(as_device(X)), twin.mean_field(X)
    assert n_dev == n_twin and 1 <= n_dev <= 2, (n_dev, n_twin)
    eng.sample_v(1); twin.sample_v(1)
    tally = mp.Tally()
    for i in range(len(widths)):
        sfx = '' if i == 0 else '_%d' % i
        mu, h = eng.get('mu' + sfx), eng.get('h' + sfx)
        mp.assert_bits(mu, twin.p['mu' + sfx], 'mu' + sfx)
        mp.assert_bits(h, twin.p['h' + sfx], 'h' + sfx)
        if hu[i]:
            mp.check_means(P['hb' + sfx], mu, ns[i], what='device DBM mu' + sfx)
            tally.add(P['hb' + sfx], h, ns[i], mp.F32, 'dbm', 'device DBM h' + sfx)
    mp.assert_bits(eng.get('v'), twin.p['v'], 'v')
    eng.close()


def test_dbm_real_weights_spread_beyond_the_clamp(gpu_lib):
    """the weights of tests/test_dbm_parity_gpu.py::make_pair scaled by 40: distinct logits per row, spread over more than 80
    within a row; mean-field, a train step and sample_v bit for bit, the counts whole and summing to n_samples"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    from tests.test_dbm_parity_gpu import assert_equal, data, make_pair
    V, nh, hu, ns, N = 20, [63, 16, 65], [2, 0, 2], [100, 0, 7], R
    eng, twin = make_pair(V, nh, N, N, max_mf_updates=5, mf_tol=1e-5, l2=1e-3, h_units=hu, n_samples=ns)
    for nm in ('W', 'W_1', 'W_2'):
        W = twin.p[nm] * np.float32(40)
        eng.set(nm, W); twin.p[nm][...] = W
    X = data(N, V, 0)
    logits = np.float32(2) * (X @ twin.p['W']) + twin.p['hb']         # the first pass of the mean-field (doubled weights)
    spread = float(np.max(logits.max(axis=1) - logits.min(axis=1)))
    assert spread > 80.0, spread
    eng.seed(SEED); twin.set_seed(SEED)
    names = ['vb', 'dvb', 'v']
    for i in range(3):
        names += [b + ('' if i == 0 else '_%d' % i) for b in ('W', 'dW', 'hb', 'dhb', 'q_means', 'mu_means', 'mu', 'h')]
    assert eng.mean_field(as_device(X)) == twin.mean_field(X)
    assert_equal(eng, twin, ['mu', 'mu_1', 'mu_2'])
    assert eng.train_step(as_device(X), 0.02, 0.5, 2)[0] == twin.train_step(X, 0.02, 0.5, 2)[0]
    assert_equal(eng, twin, names)
    Vd = DeviceArray((N, V))
    eng.sample_v(2, Vd)
    mp.assert_bits(Vd.numpy(), twin.sample_v(2), 'sample_v')
    for sfx, M in (('', 100), ('_2', 7)):
        h = eng.get('h' + sfx)
        assert np.all(h >= 0) and np.all(h == np.round(h)) and np.all(h.sum(axis=1) == M), sfx
        assert np.all(np.isfinite(eng.get('mu' + sfx)))
    eng.close()
