"""Centred training on the CPU: the float64 reference against itself (two parameterisations, flip
invariance), the float32 twin of the engine's order against the reference, and the surface that needs no device."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import centering_twin as T
from tests import np_reference_centering as R

SEED = 20241019


def _binary(rng, rows, cols, p=0.35):
    return (rng.rand(rows, cols) < p).astype(np.float64)


def _max_gap(a, b):
    return max(max(np.abs(x - y).max() for x, y in zip(a.W, b.W)), max(np.abs(x - y).max() for x, y in zip(a.b, b.b)),
               max(np.abs(x - y).max() for x, y in zip(a.o, b.o)))


def _rbm_run(s, X, n_updates, nu, lr, **kw):
    for _ in range(n_updates):
        pos, neg = R.rbm_phases(s, X)
        R.update_standard(s, pos, neg, nu, lr, **kw)
    return s


def _dbm_run(s, X, particles, n_updates, nu, lr, **kw):
    for _ in range(n_updates):
        pos, neg, particles = R.dbm_phases(s, X, particles, n_mf=5, k=1)
        R.update_standard(s, pos, neg, nu, lr, **kw)
    return s


# ---- 1. the two forms of the reference
def test_reference_two_ways_rbm():
    rng = np.random.RandomState(1)
    X = _binary(rng, 12, 7)
    a = R.State([7, 5], rng)
    a.o = [X.mean(0), np.full(5, 0.5)]
    b = a.copy()
    nu = [0.1, 0.2]
    for _ in range(5):
        pos, neg = R.rbm_phases(a, X)
        R.update_standard(a, pos, neg, nu, 0.1)
        pos, neg = R.rbm_phases(b, X)
        R.update_explicit(b, pos, neg, nu, 0.1)
    assert _max_gap(a, b) <= 1e-12


def test_reference_two_ways_dbm():
    rng = np.random.RandomState(2)
    n = [7, 5, 4, 3]
    X = _binary(rng, 6, 7)
    a = R.State(n, rng)
    a.o = [X.mean(0)] + [np.full(m, 0.5) for m in n[1:]]
    b = a.copy()
    pa = [rng.rand(5, m) for m in n]
    pb = [x.copy() for x in pa]
    nu = [0.1, 0.05, 0.2, 0.1]
    for _ in range(4):
        pos, neg, pa = R.dbm_phases(a, X, pa)
        R.update_standard(a, pos, neg, nu, 0.1)
        pos, neg, pb = R.dbm_phases(b, X, pb)
        R.update_explicit(b, pos, neg, nu, 0.1)
    assert _max_gap(a, b) <= 1e-12


# ---- 2. flip invariance (means only; momentum on, l2 and sparsity off: those two act on W alone and break the symmetry)
@pytest.mark.parametrize('centred', [True, False])
def test_flip_invariance_rbm(centred):
    rng = np.random.RandomState(3)
    X = _binary(rng, 12, 7)
    s = R.State([7, 5], rng, scale=0.5)
    s.o = [X.mean(0), np.full(5, 0.5)]
    t = R.flip(s)
    _rbm_run(s, X, 5, [0.1, 0.1], 0.1, mom=0.5, centred=centred)
    _rbm_run(t, 1.0 - X, 5, [0.1, 0.1], 0.1, mom=0.5, centred=centred)
    gap = R.flip_gap(s, t)
    worst = max(v for k, v in gap.items() if centred or not k.startswith('o'))
    if centred:
        assert worst <= 1e-12, gap
    else:
        assert worst >= 1e-3, gap


@pytest.mark.parametrize('centred', [True, False])
def test_flip_invariance_dbm(centred):
    rng = np.random.RandomState(4)
    n = [7, 5, 4, 3]
    X = _binary(rng, 6, 7)
    s = R.State(n, rng, scale=0.5)
    s.o = [X.mean(0)] + [np.full(m, 0.5) for m in n[1:]]
    t = R.flip(s)
    p = [rng.rand(5, m) for m in n]
    q = [1.0 - p[0]] + [x.copy() for x in p[1:]]
    nu = [0.1] * 4
    _dbm_run(s, X, p, 4, nu, 0.1, mom=0.5, centred=centred)
    _dbm_run(t, 1.0 - X, q, 4, nu, 0.1, mom=0.5, centred=centred)
    gap = R.flip_gap(s, t)
    worst = max(v for k, v in gap.items() if centred or not k.startswith('o'))
    if centred:
        assert worst <= 1e-12, gap
    else:
        assert worst >= 1e-3, gap


# ---- 3. the float32 twin
def test_fma32_is_fmaf():
    libm = C.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
    libm.fmaf.restype, libm.fmaf.argtypes = C.c_float, [C.c_float] * 3
    rng = np.random.RandomState(5)
    a = (rng.randn(4000) * np.exp(rng.randn(4000) * 4)).astype(np.float32)
    b = (rng.randn(4000) * np.exp(rng.randn(4000) * 4)).astype(np.float32)
    c = (-a * b * (1 + rng.randn(4000).astype(np.float32) * np.float32(1e-6))).astype(np.float32)      # heavy cancellation
    c[::3] = (rng.randn(len(c[::3])) * 10).astype(np.float32)
    # ties of the float32 rounding that only the sticky bit decides: a * b = 1 + 2^-24 exactly, c = +-2^-60
    a[:2], b[:2], c[:2] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12) , [2.0 ** -60, -2.0 ** -60]
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    got = T.fma32(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _params32(V, H):
    return dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H) * np.float32(0.3), vb=orc.normal(SEED, 2, 0, V) * np.float32(0.5),
                hb=orc.normal(SEED, 3, 0, H) * np.float32(0.5))


def _batch32(B, V, site=6):
    return (orc.uniform(SEED, site, 0, B * V) < 0.4).astype(np.float32).reshape(B, V)


def twin_and_reference(V, H, B, n_updates=3, nu=(0.1, 0.1), lr=0.05, mom=0.5, l2=1e-4):
    """the float32 twin and the float64 reference from the same float32 start, all sampling off; returns (twin state, State)"""
    p, X = _params32(V, H), _batch32(B, V)
    o = [X.astype(np.float64).mean(0).astype(np.float32), np.full(H, 0.5, np.float32)]
    tw = T.CentredRBM(p, nu, o, seed=SEED, sample_v_states=False, sample_h_states=False, l2=l2)
    s = R.State([V, H])
    s.W, s.b = [p['W'].astype(np.float64)], [p['vb'].astype(np.float64), p['hb'].astype(np.float64)]
    s.o = [x.astype(np.float64) for x in o]
    for _ in range(n_updates):
        tw.train_step(X, lr, mom, 1)
        pos, neg = R.rbm_phases(s, X.astype(np.float64))
        R.update_standard(s, pos, neg, [float(np.float32(x)) for x in nu], float(np.float32(lr)), mom=float(np.float32(mom)),
                          l2=float(np.float32(l2)))
    return tw.state(), s


@pytest.mark.parametrize('V,H,B', [(7, 5, 12), (70, 75, 17), (37, 29, 33)])
def test_twin_against_reference(V, H, B):
    """rtol 1e-5 (the project's parity bound), atol 1e-6 * max|param|, after 3 updates"""
    got, s = twin_and_reference(V, H, B)
    for name, want in (('W', s.W[0]), ('vb', s.b[0]), ('hb', s.b[1]), ('ov', s.o[0]), ('oh', s.o[1])):
        np.testing.assert_allclose(got[name], want, rtol=1e-5, atol=1e-6 * np.abs(want).max(), err_msg=name)


def test_twin_zero_offsets_is_the_oracle():
    """o = 0, nu = 0: the centred twin is orc_rbm_train_step bit for bit (what the GPU tests assert of the engine)"""
    V, H, B = 37, 29, 33
    p, X = _params32(V, H), _batch32(B, V)
    tw = T.CentredRBM(p, (0., 0.), [np.zeros(V), np.zeros(H)], seed=SEED, sparsity_cost=0.1)
    ref = orc.OracleRBM(V, H, sparsity_cost=0.1)
    for n in ('W', 'vb', 'hb'):
        ref.p[n][...] = p[n]
    ref.set_seed(SEED)
    for _ in range(3):
        tw.train_step(X, 0.05, 0.5, 1)
        ref.train_step(X, 0.05, 0.5, 1)
    got = tw.state()
    for n in ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means'):
        assert np.array_equal(got[n].view(np.uint32), ref.p[n].view(np.uint32)), n
    assert not got['ov'].any() and not got['oh'].any()


def test_fit_flip_deviation_of_the_twins():
    """the float32 deviations the GPU's flip tests through fit() take their tolerance from (ten times these): the recorded
    figures are what the twins show now, not a loose bound"""
    p, X = T.fit_case()
    dev = T.flip_gap(T.fit_twin(p, X), T.fit_twin(T.flip_params(p), 1 - X))
    assert T.FIT_TWIN_DEVIATION / 2 <= dev <= T.FIT_TWIN_DEVIATION, dev
    s, X, P = R.fit_case()
    a = R.fit_run(s, X, P, np.float32)
    b = R.fit_run(R.flip(s), 1 - X, [1 - P[0]] + P[1:], np.float32)
    dev = max(R.flip_gap(a, b).values())
    assert a.W[0].dtype == np.float32 and R.FIT_F32_DEVIATION / 2 <= dev <= R.FIT_F32_DEVIATION, dev
    # ... and without centering the same runs are far apart
    a, b = s.copy(), R.flip(s)
    for st, Xs, Ps in ((a, X, P), (b, 1 - X, [1 - P[0]] + P[1:])):
        pos, neg, _ = R.dbm_phases(st, Xs[:R.FIT_BATCH], Ps, n_mf=R.FIT_MF)
        R.update_standard(st, pos, neg, [0.1] * 3, 0.5, centred=False)
    assert max(v for k, v in R.flip_gap(a, b).items() if not k.startswith('o')) >= 1e-3


# ---- 4. surface
def test_abi_surface():
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import DbmEngine, DbmEngine64, RbmEngine, RbmEngine64
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'bm355.h')).read()
    assert 'int bm_rbm_set_centering(bm_rbm *h, int32_t on, float nu_v, float nu_h);' in header
    assert 'int bm_dbm_set_centering(bm_dbm *h, int32_t on, const float *nu' in header
    assert len(_ffi.SIGNATURES['bm_rbm_set_centering']) == 4 and len(_ffi.SIGNATURES['bm_dbm_set_centering']) == 3
    assert callable(RbmEngine.set_centering) and callable(DbmEngine.set_centering)
    assert not hasattr(RbmEngine64, 'set_centering')
    with pytest.raises(NotImplementedError, match='float64'):
        DbmEngine64.set_centering(None, True)


def _bare_dbm(**kw):
    from boltzmann_machines_amd import DBM
    d = DBM(rbms=None, n_particles=5, batch_size=5, **kw)
    d.n_layers_, d.n_visible_, d.n_hiddens_, d.h_units_ = 2, 12, [8, 6], [0, 0]
    return d


def test_public_refusals(monkeypatch):
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM, MultinomialRBM, _ffi
    with pytest.raises(NotImplementedError, match='Gaussian'):
        GaussianRBM(n_visible=6, n_hidden=4).set_centering()
    with pytest.raises(NotImplementedError, match='Multinomial'):
        MultinomialRBM(n_visible=6, n_hidden=4).set_centering()
    with pytest.raises(NotImplementedError, match='float64'):
        BernoulliRBM(n_visible=6, n_hidden=4, dtype='float64').set_centering()
    with pytest.raises(NotImplementedError, match='dbm_first'):
        BernoulliRBM(n_visible=6, n_hidden=4, dbm_first=True).set_centering()
    with pytest.raises(NotImplementedError, match='dbm_first'):
        BernoulliRBM(n_visible=6, n_hidden=4, dbm_last=True).set_centering()
    with pytest.raises(NotImplementedError, match='dropout'):
        BernoulliRBM(n_visible=6, n_hidden=4, dropout=0.8).set_centering()
    m = BernoulliRBM(n_visible=6, n_hidden=4)
    m._dp = object()
    with pytest.raises(NotImplementedError, match='data parallelism'):
        m.set_centering()
    d = _bare_dbm()
    d.v_unit_ = _ffi.UNIT_GAUSSIAN
    with pytest.raises(NotImplementedError, match='Gaussian'):
        d.set_centering()
    d = _bare_dbm()
    d.h_units_ = [0, _ffi.UNIT_MULTINOMIAL]
    with pytest.raises(NotImplementedError, match='Multinomial'):
        d.set_centering()
    with pytest.raises(NotImplementedError, match='float64'):
        _bare_dbm(dtype='float64').set_centering()
    d = _bare_dbm()
    d._dp = object()
    with pytest.raises(NotImplementedError, match='data parallelism'):
        d.set_centering()
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(NotImplementedError, match='BM355_DATA_PARALLEL'):
        BernoulliRBM(n_visible=6, n_hidden=4).set_centering()
    with pytest.raises(NotImplementedError, match='BM355_DATA_PARALLEL'):
        _bare_dbm().set_centering()


def test_setting_is_not_a_parameter():
    from boltzmann_machines_amd import BernoulliRBM
    m = BernoulliRBM(n_visible=6, n_hidden=4)
    before = m.get_params()
    assert m.centering_offsets() is None and m._centering_variables() == {}
    assert m.set_centering(nu_v=0.2, offset_h=0.25) is m
    after = m.get_params()
    assert sorted(before) == sorted(after) and all(np.array_equal(before[k], after[k]) for k in before)
    off = m.centering_offsets()
    assert off[0] is None and np.array_equal(off[1], np.full(4, 0.25, np.float32))
    assert sorted(m._centering_variables()) == ['centering_nu', 'centering_oh']
    assert m.set_centering(False).centering_offsets() is None and m._centering_variables() == {}
    with pytest.raises(ValueError, match='sliding factors'):
        m.set_centering(nu_v=1.5)
    d = _bare_dbm()
    before = d.get_params()
    assert d.set_centering(nu=[0.1, 0.2, 0.3]) is d and d._centering['nu'] == [0.1, 0.2, 0.3]
    assert sorted(before) == sorted(d.get_params())
    assert len(d.set_centering(nu=0.05).centering_offsets()) == 3
    with pytest.raises(ValueError, match='sliding factors'):
        d.set_centering(nu=[0.1, 0.2])


class _FakeEngine(object):
    """records what the Python layer asks of an engine"""

    def __init__(self):
        self.vars, self.calls = {}, []

    def set(self, name, value):
        self.vars[name] = np.array(value, np.float32)

    def get(self, name):
        return self.vars[name]

    def set_centering(self, on, *nu):
        self.calls.append(bool(on))

    def close(self):
        pass


def _write_checkpoint(model, extra):
    """the three files of a checkpoint without a device: params.json as _save_model writes it, model.npz from `extra`"""
    import json
    params = model._serialize(dict(model.get_params(deep=False)))
    params['__class_name__'] = model.__class__.__name__
    os.makedirs(model._model_dirpath, exist_ok=True)
    with open(model._params_filepath, 'w') as f:
        f.write(json.dumps(params, **model.json_params))
    np.savez(model._model_filepath + '.npz', **extra)


def test_load_then_set_centering_is_not_undone(tmp_path):
    """load_model restores the mode ONCE: what the caller sets between load_model and the first engine build stands"""
    from boltzmann_machines_amd import BernoulliRBM
    V, H = 6, 4
    m = BernoulliRBM(n_visible=V, n_hidden=H, model_path=str(tmp_path / 'm') + '/', verbose=False)
    ov, oh = np.linspace(0.1, 0.6, V).astype(np.float32), np.full(H, 0.25, np.float32)
    _write_checkpoint(m, dict(W=np.zeros((V, H), np.float32), vb=np.zeros(V, np.float32), hb=np.zeros(H, np.float32),
                              centering_nu=np.float32([0.2, 0.3]), centering_ov=ov, centering_oh=oh))

    def build(model):               # what _ensure_engine does, on a fake engine
        model._engine = _FakeEngine()
        model._apply_centering()
        model._upload_variables(model._pending_vars)
        return model._engine
    a = BernoulliRBM.load_model(str(tmp_path / 'm') + '/')
    assert a._centering['nu'] == [float(np.float32(0.2)), float(np.float32(0.3))]
    assert np.array_equal(a.centering_offsets()[0], ov) and np.array_equal(a.centering_offsets()[1], oh)
    assert not [k for k in a._pending_vars if k.startswith('centering')]
    eng = build(a)
    assert eng.calls == [True] and np.array_equal(eng.vars['ov'], ov) and np.array_equal(eng.vars['oh'], oh)
    assert sorted(a._centering_variables()) == ['centering_nu', 'centering_oh', 'centering_ov']
    # switched off after the load: stays off, nothing centred is written
    b = BernoulliRBM.load_model(str(tmp_path / 'm') + '/').set_centering(False)
    eng = build(b)
    assert eng.calls == [] and 'ov' not in eng.vars and b.centering_offsets() is None and b._centering_variables() == {}
    # another nu and other offsets after the load: they stand
    c = BernoulliRBM.load_model(str(tmp_path / 'm') + '/').set_centering(nu_v=0.5, nu_h=0.5, offset_v=0.75)
    eng = build(c)
    assert c._centering['nu'] == [0.5, 0.5] and np.array_equal(eng.vars['ov'], np.full(V, 0.75, np.float32)) and 'oh' not in eng.vars
    # a rebuild after set_params: the offsets go back to the host first, centering_offsets() needs no engine
    d = BernoulliRBM.load_model(str(tmp_path / 'm') + '/')
    build(d)
    d._centering_detach()
    d._engine = None
    assert np.array_equal(d.centering_offsets()[0], ov) and np.array_equal(d.centering_offsets()[1], oh)
    assert build(d).calls == [True] and np.array_equal(d._engine.vars['oh'], oh)


def test_switching_off_never_raises():
    from boltzmann_machines_amd import GaussianRBM
    assert GaussianRBM(n_visible=6, n_hidden=4).set_centering(False).centering_offsets() is None
    d = _bare_dbm(dtype='float64')
    assert d.set_centering(False) is d
    d = _bare_dbm()
    d.n_layers_ = None                       # (a DBM without layers yet)
    assert d.set_centering(False) is d
