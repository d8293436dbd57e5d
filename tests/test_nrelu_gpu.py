"""Noisy rectified-linear hidden units (BM_UNIT_NRELU) on the GPU: every state-carrying result bit for bit against
the CPU twin (tests/nrelu_twin.py) - bm_rbm_sample_h, the value range of the epilogue, the update, the epoch loop, transform /
gibbs / metrics, the public classes - and the C-ABI refusals."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import nrelu_twin as T
from tests import numerics_probes as npb
from tests.clamp_twin import act2

pytestmark = pytest.mark.gpu
f32 = np.float32
SHAPES = [(12, 8, 16), (37, 23, 19), (100, 52, 37), (64, 96, 33), (784, 128, 100)]     # (37, 23, 19): generic RNG path, ragged tiles
STATE = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')


def bits_equal(g, c, what=''):
    g, c = np.ascontiguousarray(g, f32), np.ascontiguousarray(c, f32)
    bad = int(np.sum(g.view(np.uint32) != c.view(np.uint32)))
    assert bad == 0, '%s: %d / %d elements differ bitwise (max abs diff %.3e)' % (what, bad, g.size, float(np.nanmax(np.abs(g - c))))


def params(V, H, w_seed=1337, w_std=0.01, gaussian=False):
    p = dict(W=(orc.normal(87654321, w_seed, 0, V * H) * f32(w_std)).reshape(V, H).astype(f32),
             vb=((orc.uniform(87654321, w_seed + 1, 0, V) - f32(0.5)) * f32(0.2)).astype(f32),
             hb=((orc.uniform(87654321, w_seed + 2, 0, H) - f32(0.5)) * f32(0.2)).astype(f32))
    if gaussian:
        p['sigma'] = np.linspace(0.5, 1.5, V).astype(f32)
    return p


def data(B, V, seed, gaussian=False):
    if gaussian:
        return orc.normal(87654321, 43 + seed, 0, B * V).reshape(B, V)
    return (orc.uniform(87654321, 42 + seed, 0, B * V).reshape(B, V) < 0.1307).astype(f32)


def engine(p, B, v_unit=0, h_unit=3, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = p['W'].shape
    eng = RbmEngine(V, H, v_unit=v_unit, max_batch=B, h_unit=h_unit, **kw)
    for n, a in p.items():
        eng.set(n, a)
    return eng


def pair(V, H, B, seed, gaussian=False, p=None, **kw):
    p = p or params(V, H, gaussian=gaussian)
    eng = engine(p, B, v_unit=int(gaussian), **kw)
    twin = T.NReLURBM(p, seed, v_unit=int(gaussian), l2=kw.get('l2', 1e-4), sample_v_states=kw.get('sample_v_states', False),
                      sample_h_states=kw.get('sample_h_states', True))
    eng.seed(seed)
    return eng, twin


def state_equal(eng, twin, what=''):
    for n in STATE:
        bits_equal(eng.get(n), twin.p[n], '%s %s' % (what, n))


def run_sample_h(eng, X, seed, row0, means=True, states=True):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    B = len(X)
    Md = DeviceArray((B, eng.H), f32) if means else None
    Sd = DeviceArray((B, eng.H), f32) if states else None
    eng.seed(seed)
    eng.set_row_offset(row0)
    eng.sample_h(as_device(X), B, Md, Sd)
    eng.sync()
    eng.set_row_offset(0)
    return (Md.numpy() if means else None), (Sd.numpy() if states else None)


# ---- 1. bm_rbm_sample_h
@pytest.mark.parametrize('V,H,B', SHAPES)
def test_sample_h(gpu_lib, V, H, B):
    p = params(V, H, w_std=0.2)
    X = data(B, V, 3, gaussian=True)
    eng = engine(p, B)
    for row0 in (0, 1000):
        gm, gs = run_sample_h(eng, X, 7, row0)
        cm, cs = T.sample_h(p, X, 7, 0, row0)
        bits_equal(gm, cm, 'means row0=%d' % row0)
        bits_equal(gs, cs, 'states row0=%d' % row0)
    assert (cs > 0).mean() > 0.2 and (cs == 0).mean() > 0.2               # both branches of the rectifier are exercised
    _, gs = run_sample_h(eng, X, 7, 1000, means=False)                    # either output may be null
    bits_equal(gs, cs, 'states alone')
    gm, _ = run_sample_h(eng, X, 7, 1000, states=False)
    bits_equal(gm, cm, 'means alone')
    eng.close()


@pytest.mark.parametrize('h_unit,kind', [(0, 0), (2, 16 + 20)])
def test_sample_h_other_units(gpu_lib, h_unit, kind):
    """bm_rbm_sample_h on a Bernoulli and on a Multinomial handle against act2"""
    V, H, B = 37, 23, 19
    p = params(V, H, w_std=0.2)
    X = data(B, V, 4)
    eng = engine(p, B, h_unit=h_unit, n_samples=20)
    for row0 in (0, 1000):
        cm, cs = act2(X, p['W'], None, None, p['hb'], None, 1.0, kind, 1, 9, T.SITE_H0, 0, row0)
        gm, gs = run_sample_h(eng, X, 9, row0)
        bits_equal(gm, cm, 'means')
        bits_equal(gs, cs, 'states')
        _, gs = run_sample_h(eng, X, 9, row0, means=False)
        bits_equal(gs, cs, 'states alone')
    eng.close()


def sample_h_digests():
    """one digest per shape of the means and states bm_rbm_sample_h returns (row0 = 1000)"""
    out = []
    for V, H, B in SHAPES:
        eng = engine(params(V, H, w_std=0.2), B)
        gm, gs = run_sample_h(eng, data(B, V, 3, gaussian=True), 7, 1000)
        eng.close()
        out.append(hashlib.sha1(gm.tobytes() + gs.tobytes()).hexdigest())
    return out


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ('8', '4', '1', '3', '108', '104', '101', '103', '208', '6', '5', '7', '9')      # what launch_act_as accepts
CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_nrelu_gpu as G
print('NRELU_DIGEST', ' '.join(G.sample_h_digests()))
'''


def test_every_geometry_holds_the_twins_bits(gpu_lib):
    """one fresh child per act_kernel geometry (BM355_DEBUG is read once per process, as tests/test_class_joint_gpu.py does it),
    each under its own time limit; the first failure ends the test.  The shapes cover both operand layouts of the prop-up (W^T
    x-major where V % 4 == 0, W k-major otherwise) and both RNG paths"""
    want = []
    for V, H, B in SHAPES:
        cm, cs = T.sample_h(params(V, H, w_std=0.2), data(B, V, 3, gaussian=True), 7, 0, 1000)
        want.append(hashlib.sha1(cm.tobytes() + cs.tobytes()).hexdigest())
    assert sample_h_digests() == want
    for geo in GEOMETRIES:
        env = dict(os.environ, BM355_DEBUG='act_geo=' + geo)
        r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'NRELU_DIGEST' in r.stdout, 'act_geo=%s: %s' % (geo, r.stdout[-2000:] + r.stderr[-4000:])
        got = r.stdout.split('NRELU_DIGEST', 1)[1].split()
        assert got == want, 'act_geo=%s: shapes %r differ from the twin' % (geo, [s for s, g, w in zip(SHAPES, got, want) if g != w])


# ---- 2. value range: every output is one probed t (one-hot input), over denormals, -0 and large |t|
def test_value_range(gpu_lib):
    W = npb.sigmoid_points()
    p = dict(W=W, vb=np.zeros(128, f32), hb=np.zeros(128, f32))
    eng = engine(p, 128)
    X = npb.onehot(128)
    gm, gs = run_sample_h(eng, X, 21, 0)
    cm, cs = T.sample_h(p, X, 21, 0, 0)
    bits_equal(gm, cm, 'means')
    bits_equal(gs, cs, 'states')
    bits_equal(gm, T.rectify(W), 'the mean is the rectified point')
    eng.close()


# ---- 3. train_step: three updates, every variable after each
def three_updates(eng, twin, X, k, lr=0.01, mom=0.9, what=''):
    from boltzmann_machines_amd.engine import as_device
    Xd = as_device(X)
    for s in range(3):
        eng.train_step(Xd, len(X), lr, mom, k)
        twin.train_step(X, lr, mom, k)
        state_equal(eng, twin, '%s update %d' % (what, s))


@pytest.mark.parametrize('gaussian', [False, True])
@pytest.mark.parametrize('sample_v', [False, True])
@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('V,H,B', SHAPES)
def test_train_step(gpu_lib, V, H, B, k, sample_v, gaussian):
    eng, twin = pair(V, H, B, 3, gaussian=gaussian, sample_v_states=sample_v, l2=1e-3)
    three_updates(eng, twin, data(B, V, 5, gaussian), k, lr=1e-3 if gaussian else 0.01)
    eng.close()


def test_train_step_zero_units(gpu_lib):
    """hb = -20 on a third of the hidden units: those units are exactly zero for the whole batch in both phases, so the last
    prop-up stores -0 for them (the signed-zero case of tests/nrelu_twin.py)"""
    V, H, B = 64, 96, 33
    p = params(V, H)
    p['hb'][::3] = -20.0
    eng, twin = pair(V, H, B, 3, p=p)
    X = data(B, V, 6)
    ch = twin.chain(X, 1)
    assert np.all(ch['h0m'][:, ::3] == 0) and np.all(ch['hm'][:, ::3] == 0) and np.any(ch['hm'] > 0)
    three_updates(eng, twin, X, 1)
    eng.close()


def test_train_step_mean_field_hidden(gpu_lib):
    V, H, B = 37, 23, 19
    eng, twin = pair(V, H, B, 3, sample_h_states=False)
    three_updates(eng, twin, data(B, V, 7), 2)
    eng.close()


# ---- 4. train_epoch = the loop of train_step calls
def test_train_epoch(gpu_lib):
    from boltzmann_machines_amd.engine import as_device
    V, H, B = 37, 23, 19
    N = 2 * B + 7
    X = data(N, V, 8)
    eng, twin = pair(V, H, B, 5)
    loop, _ = pair(V, H, B, 5)
    Xd = as_device(X)
    eng.train_epoch(Xd, N, B, 0.01, 0.9, 1)
    for s in range(0, N, B):
        loop.train_step(Xd, min(B, N - s), 0.01, 0.9, 1, row=s)
    twin.train_epoch(X, B, 0.01, 0.9, 1)
    for n in STATE:
        bits_equal(eng.get(n), loop.get(n), 'epoch against loop: ' + n)
    state_equal(eng, twin, 'epoch against twin')
    eng.close(); loop.close()


# ---- 5. transform, gibbs, metrics
@pytest.mark.parametrize('gaussian', [False, True])
def test_transform_gibbs_metrics(gpu_lib, gaussian):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    V, H, B = 100, 52, 37
    eng, twin = pair(V, H, B, 11, gaussian=gaussian, sample_v_states=True)
    X = data(B, V, 9, gaussian)
    Xd = as_device(X)
    Hd = DeviceArray((B, H), f32)
    eng.transform(Xd, B, 2, Hd)
    bits_equal(Hd.numpy(), twin.transform(X, 2), 'transform')
    H0 = T.rectify(orc.normal(1, 2, 3, B * H).reshape(B, H))
    Hd, Vd = as_device(H0), DeviceArray((B, V), f32)
    eng.gibbs(Hd, Vd, B, 2)
    ch, cv = twin.gibbs(H0, 2)
    bits_equal(Hd.numpy(), ch, 'gibbs h')
    bits_equal(Vd.numpy(), cv, 'gibbs v')
    out = eng.metrics(Xd, B, 1)
    msre, l2 = twin.metrics(X, 1)
    np.testing.assert_allclose([out[0], out[2]], [msre, l2], rtol=1e-5)
    assert np.isnan(out[1]) and np.isnan(out[3])
    # train_step_metrics (blocking and asynchronous) leaves the parameters train_step leaves
    out = eng.train_step_metrics(Xd, B, 0.01, 0.9, 1)
    assert np.isnan(out[1]) and np.isnan(out[3]) and np.isfinite(out[0]) and np.isfinite(out[2])
    twin.train_step(X, 0.01, 0.9, 1)
    state_equal(eng, twin, 'train_step_metrics')
    eng.train_step_metrics_async(Xd, B, 0.01, 0.9, 1)
    twin.train_step(X, 0.01, 0.9, 1)
    got = eng.collect_metrics()
    assert got.shape == (1, 4) and np.isnan(got[0, 1]) and np.isnan(got[0, 3]) and np.isfinite(got[0, 0])
    state_equal(eng, twin, 'train_step_metrics_async')
    eng.close()


# ---- 6. the public classes
@pytest.mark.parametrize('cls_name', ['ReLURBM', 'GaussianReLURBM'])
def test_public_classes(gpu_lib, cls_name, tmp_path):
    """fit() for 2 epochs at 36 x 20, batch 16 (a short last batch), against the twin driven with the seeds fit() draws from the
    model's host stream (one per call) and its schedule; checkpoint, load_model, transform; a fit resumed from disk against the
    one continued in the same process (and both against the twin); sample_h over two batch sizes"""
    import boltzmann_machines_amd as bm
    from boltzmann_machines_amd.utils import RNG
    cls = getattr(bm, cls_name)
    gaussian = cls_name == 'GaussianReLURBM'
    V, H, N, bs, lr, mom = 36, 20, 40, 16, 0.005, 0.5
    X = data(N, V, 10, gaussian)
    p0 = params(V, H, gaussian=gaussian)
    kw = dict(n_visible=V, n_hidden=H, W_init=p0['W'], vb_init=p0['vb'], hb_init=p0['hb'], batch_size=bs, learning_rate=lr,
              momentum=mom, l2=1e-3, max_epoch=2, random_seed=1337, verbose=False, v_shape=(6, 6))
    if gaussian:
        kw['sigma'] = p0['sigma']
    path = lambda n: str(tmp_path) + '/%s/' % n
    host = RNG(seed=1337)
    s1, s2 = host.randint(2 ** 31 - 1), host.randint(2 ** 31 - 1)       # the seeds of the first and of the second fit() call

    def against_twin(model, twin, what):
        w, acc = model.get_tf_params(scope='weights'), model.get_tf_params(scope='grads_accumulators')
        for n in ('W', 'vb', 'hb'):
            bits_equal(w[n], twin.p[n], '%s %s' % (what, n))
        for n in ('dW', 'dvb', 'dhb'):
            bits_equal(acc[n], twin.p[n], '%s %s' % (what, n))

    twin = T.NReLURBM(p0, s1, v_unit=int(gaussian), l2=1e-3)
    for _ in range(2):
        twin.train_epoch(X, bs, lr, mom, 1)
    a = cls(model_path=path('a'), **kw).fit(X)
    b = cls(model_path=path('b'), **kw).fit(X)
    against_twin(a, twin, 'fit')
    # save, load_model, transform equal
    loaded = cls.load_model(path('b'))
    assert loaded.epoch_ == 2
    against_twin(loaded, twin, 'load_model')
    h_loaded, h_again = loaded.transform(X), cls.load_model(path('b')).transform(X)
    bits_equal(h_loaded, h_again, 'transform of two loads')
    assert h_loaded.shape == (N, H) and np.all(h_loaded >= 0) and np.any(h_loaded > 0)
    # two more epochs: continued in the same process (a), resumed from the checkpoint on disk (b)
    twin.set_seed(s2)
    for _ in range(2):
        twin.train_epoch(X, bs, lr, mom, 1)
    a.set_params(max_epoch=4).fit(X)
    resumed = cls.load_model(path('b'))
    resumed.set_params(max_epoch=4).fit(X)
    assert a.epoch_ == 4 and resumed.epoch_ == 4
    against_twin(a, twin, 'continued fit')
    against_twin(resumed, twin, 'resumed fit')
    # sample_h does not depend on batch_size
    m16 = cls(model_path=path('s16'), **kw).init()
    m7 = cls(model_path=path('s7'), **dict(kw, batch_size=7)).init()
    s16, mean16 = m16.sample_h(X, return_means=True)
    s7, mean7 = m7.sample_h(X, return_means=True)
    bits_equal(s16, s7, 'sample_h states over batch sizes')
    bits_equal(mean16, mean7, 'sample_h means over batch sizes')
    cm, cs = T.sample_h(p0, X, s1, 0, 0)
    bits_equal(s16, cs, 'sample_h states against the twin')
    bits_equal(mean16, cm, 'sample_h means against the twin')


# ---- 7. the C-ABI refusals
def test_c_abi_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine, as_device
    V, H, B = 12, 8, 16
    lib = gpu_lib

    def refused(rc, what):
        assert rc != 0, what + ' was accepted'
        msg = lib.bm_last_error().decode()
        assert 'NReLU' in msg, '%s: %s' % (what, msg)

    for bad in (dict(dbm_first=True), dict(dbm_last=True), dict(sparsity_cost=0.1), dict(dropout=0.8)):
        with pytest.raises(_ffi.Bm355Error) as e:
            RbmEngine(V, H, max_batch=B, h_unit=_ffi.UNIT_NRELU, **bad)
        assert 'NReLU' in str(e.value), (bad, str(e.value))
    cfg = _ffi.RbmConfig(V, H, 0, 0, 1, 0, 0, B, 1e-4, 0.1, 0., 0.9, -1.0, _ffi.UNIT_NRELU, 0)
    h64, hyper = C.c_void_p(), (C.c_double * 5)(1e-4, 0.1, 0., 0.9, -1.0)
    refused(lib.bm_rbm64_create(C.byref(cfg), hyper, C.byref(h64)), 'bm_rbm64_create')

    eng, twin = pair(V, H, B, 3)
    X = data(B, V, 2)
    Xd = as_device(X)
    D = DeviceArray((4 * B, max(V, H)), f32)                # a device buffer for every pointer argument of a refused call
    hostf = np.zeros(4 * B * max(V, H), f32)
    hp = hostf.ctypes.data_as(C.c_void_p)
    fp = hostf.ctypes.data_as(C.POINTER(C.c_float))
    lr3 = (C.c_float * 3)(0.01, 0.01, 0.01)
    h, d = eng._h, D.ptr
    one = (C.c_void_p * 1)(h)
    out = C.c_void_p()
    calls = [
        ('bm_rbm_free_energy', lambda: lib.bm_rbm_free_energy(h, d, B, fp)),
        ('bm_rbm_free_energy_rows', lambda: lib.bm_rbm_free_energy_rows(h, d, B, hp)),
        ('bm_rbm_ais', lambda: lib.bm_rbm_ais(h, 4, 4, 1, None, 1, 0, hp)),
        ('bm_rbm_pt_init', lambda: lib.bm_rbm_pt_init(h, B, 2, hp, None, 0)),
        ('bm_rbm_pt_sweep', lambda: lib.bm_rbm_pt_sweep(h, 1)),
        ('bm_rbm_pt_read', lambda: lib.bm_rbm_pt_read(h, d, None, None, None)),
        ('bm_rbm_train_step_pt', lambda: lib.bm_rbm_train_step_pt(h, d, B, 0.01, 0.9, 1)),
        ('bm_rbm_train_epoch_pt', lambda: lib.bm_rbm_train_epoch_pt(h, d, B, B, 0.01, 0.9, 1)),
        ('bm_rbm_set_fast_weights', lambda: lib.bm_rbm_set_fast_weights(h, 1, 0.01, 0.95)),
        ('bm_rbm_set_centering', lambda: lib.bm_rbm_set_centering(h, 1, 0.01, 0.01)),
        ('bm_rbm_set_classes', lambda: lib.bm_rbm_set_classes(h, 3)),
        ('bm_rbm_class_log_proba', lambda: lib.bm_rbm_class_log_proba(h, d, B, hp)),
        ('bm_rbm_class_train_step', lambda: lib.bm_rbm_class_train_step(h, d, d, B, 0.01, 0.9, None)),
        ('bm_rbm_class_train_epoch', lambda: lib.bm_rbm_class_train_epoch(h, d, d, B, B, 0.01, 0.9, None)),
        ('bm_rbm_class_joint_train_step', lambda: lib.bm_rbm_class_joint_train_step(h, d, d, B, 1, 0.01, 0.9, 0.0, None)),
        ('bm_rbm_class_joint_train_epoch', lambda: lib.bm_rbm_class_joint_train_epoch(h, d, d, B, B, 1, 0.01, 0.9, 0.0, None)),
        ('bm_rbm_class_joint_chain', lambda: lib.bm_rbm_class_joint_chain(h, d, d, B, 1, hp, hp, hp, hp, hp)),
        ('bm_rbm_class_unsup_train_step', lambda: lib.bm_rbm_class_unsup_train_step(h, d, B, 1, 0.01, 0.9, None)),
        ('bm_rbm_class_unsup_chain', lambda: lib.bm_rbm_class_unsup_chain(h, d, B, 1, hp, hp, hp, hp, hp, hp)),
        ('bm_rbm_class_semi_train_epoch', lambda: lib.bm_rbm_class_semi_train_epoch(h, d, d, B, d, B, 0, B, 1, 0.01, 0.9, 0.0, 1.0, None)),
        ('bm_rbm_class_gibbs', lambda: lib.bm_rbm_class_gibbs(h, d, d, B, 1, d, None)),
        ('bm_rbm_gibbs_clamped', lambda: lib.bm_rbm_gibbs_clamped(h, d, d, None, B, 1, d, d)),
        ('bm_rbm_grad_step', lambda: lib.bm_rbm_grad_step(h, d, B, 1)),
        ('bm_rbm_apply_step', lambda: lib.bm_rbm_apply_step(h, B, 0.01, 0.9)),
        ('bm_rbm_set_grad_slot', lambda: lib.bm_rbm_set_grad_slot(h, 1)),
        ('bm_rbm_xchg_create', lambda: lib.bm_rbm_xchg_create(h, 0, 1, C.byref(out))),
        ('bm_rbm_backprop_down', lambda: lib.bm_rbm_backprop_down(h, d, B, None, V, d, V)),
        ('bm_rbm_delta_update', lambda: lib.bm_rbm_delta_update(h, d, d, B, 0.01, 0.9)),
        ('bm_rbm_class_stack_train_step', lambda: lib.bm_rbm_class_stack_train_step(h, None, 0, d, d, B, lr3, 0.9, None)),
        ('bm_rbm_class_stack_train_epoch', lambda: lib.bm_rbm_class_stack_train_epoch(h, None, 0, d, d, B, B, lr3, 0.9, None)),
        ('bm_rbm_class_stack_log_proba', lambda: lib.bm_rbm_class_stack_log_proba(h, None, 0, d, B, hp)),
        ('bm_rbm_stack_transform', lambda: lib.bm_rbm_stack_transform(one, 1, d, B, d)),
    ]
    for what, f in calls:
        refused(f(), what)
    assert lib.bm_rbm_set_fast_binary(h, 2) == 0             # accepted: the handle keeps running fp32
    # the handle is still usable: an update matches the twin
    three_updates(eng, twin, X, 1, what='after the refusals')
    eng.close()
