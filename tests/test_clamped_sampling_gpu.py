"""-m gpu: conditional sampling (block-Gibbs with clamped visible units) - the CL flavour of act_kernel,
bm_rbm_gibbs_clamped, bm_dbm_sample_v_clamped and `sample_v_given` of the model classes.

The engine is compared BIT FOR BIT (view(uint32)) with the CPU twin of tests/clamp_twin.py (the oracle's activation stage in
a loop, the blend on the host).  Shapes are the smallest at which the epilogue can go wrong: I % 4 != 0 (the generic draw
path, scalar clamp loads, a ragged pitch), more than one 16-row block with ragged columns, and one multi-tile shape with a
tuned geometry and x-major operands; 8 sweeps lie above the chained launch's threshold of 6 passes."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import clamp_twin as T

pytestmark = pytest.mark.gpu

SEED = 424242
SHAPES = [(20, 12, 5), (33, 17, 7), (100, 72, 37), (784, 1024, 40)]
GREY = np.array([0.0, 1.0, 0.25, 0.75], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rbm_params(V, H, gaussian=False):
    p = dict(W=(orc.normal(SEED, 1, 0, V * H) * np.float32(0.1)).reshape(V, H),
             vb=(orc.uniform(SEED, 2, 0, V) - np.float32(0.5)) * np.float32(0.6),
             hb=(orc.uniform(SEED, 3, 0, H) - np.float32(0.5)) * np.float32(0.6),
             sigma=np.ones(V, np.float32))
    if gaussian:
        p['sigma'] = np.float32(0.5) + orc.uniform(SEED, 4, 0, V)           # a non-unit sigma vector
    return p


def rbm_engine(V, H, B, p, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    eng = RbmEngine(V, H, max_batch=B, **kw)
    for n in ('W', 'vb', 'hb', 'sigma'):
        eng.set(n, p[n])
    eng.seed(SEED)
    return eng


def masks(B, V):
    """random 50 %, all zero, all one, one row fully clamped while the others are free"""
    one_row = np.zeros((B, V), np.float32)
    one_row[B // 2] = 1
    return dict(half=(orc.uniform(SEED, 5, 0, B * V) < 0.5).astype(np.float32).reshape(B, V),
                zero=np.zeros((B, V), np.float32), one=np.ones((B, V), np.float32), row=one_row)


def start_and_clamp(B, V, gaussian=False):
    V0 = (orc.uniform(SEED, 6, 0, B * V) < 0.5).astype(np.float32).reshape(B, V)
    if gaussian:
        return V0, orc.normal(SEED, 7, 0, B * V).reshape(B, V) * np.float32(1.5)
    return V0, GREY[(orc.uniform(SEED, 7, 0, B * V) * 4).astype(np.int64) % 4].reshape(B, V)    # {0, 1} and grey levels


def run_engine(eng, V0, clamp, mask, n_steps, B=None, row=0):
    from boltzmann_machines_amd._ffi import DeviceArray
    B = B or len(V0)
    H = eng.H
    Vd, Cd, Md = DeviceArray.from_numpy(V0), DeviceArray.from_numpy(clamp), DeviceArray.from_numpy(mask)
    Hd, Pd = DeviceArray((len(V0), H)), DeviceArray(V0.shape)
    eng.gibbs_clamped(Vd, Hd, B, n_steps, Cd, Md, Pd, row=row)
    eng.sync()
    return Vd.numpy(), Hd.numpy(), Pd.numpy()


def check_against_twin(eng, p, V0, clamp, mask, n_steps, what, **twin_kw):
    got = run_engine(eng, V0, clamp, mask, n_steps)
    eng.seed(SEED)                                            # (the call advanced the counter: back to call 0)
    want = T.rbm_gibbs_clamped(p, V0, clamp, mask, n_steps, seed=SEED, **twin_kw)
    for name, g, w in zip(('V', 'H', 'Vmean'), got, want):
        assert same(g, w), '%s: %s differs from the twin in %d entries' % (what, name, int(np.sum(bits(g) != bits(w))))
    m = mask != 0
    assert same(got[0][m], clamp[m]) and same(got[2][m], clamp[m]), '%s: clamped entries are not the clamp values' % what
    return got


@pytest.mark.parametrize('n_steps', [1, 3, 8])
@pytest.mark.parametrize('V,H,B', SHAPES)
def test_rbm_engine_matches_twin(gpu_lib, V, H, B, n_steps):
    p = rbm_params(V, H)
    eng = rbm_engine(V, H, B, p)
    V0, clamp = start_and_clamp(B, V)
    for name, mask in masks(B, V).items():
        got = check_against_twin(eng, p, V0, clamp, mask, n_steps, '%dx%dx%d, %d steps, mask %s' % (V, H, B, n_steps, name))
        if name == 'zero':                                    # ... equals the loop without any blend
            plain = T.rbm_gibbs_clamped(p, V0, None, None, n_steps, seed=SEED, clamped=False)
            assert all(same(g, w) for g, w in zip(got, plain))
        if name == 'one':
            assert same(got[0], clamp) and same(got[2], clamp)
    eng.close()


@pytest.mark.parametrize('V,H,B', [(33, 17, 7), (100, 72, 37)])
def test_gaussian_visible_units(gpu_lib, V, H, B):
    p = rbm_params(V, H, gaussian=True)
    eng = rbm_engine(V, H, B, p, v_unit=1)
    V0, clamp = start_and_clamp(B, V, gaussian=True)
    for name, mask in masks(B, V).items():
        check_against_twin(eng, p, V0, clamp, mask, 3, 'gaussian %dx%dx%d, mask %s' % (V, H, B, name), v_unit=1)
    eng.close()


def test_dbm_first_handle(gpu_lib):
    V, H, B = 20, 12, 5
    p = rbm_params(V, H)
    eng = rbm_engine(V, H, B, p, dbm_first=True)
    V0, clamp = start_and_clamp(B, V)
    check_against_twin(eng, p, V0, clamp, masks(B, V)['half'], 3, 'dbm_first', dbm_first=True)
    eng.close()


def test_sample_flags_do_not_apply(gpu_lib):
    """both layers are sampled whatever the handle's sample_*_states say"""
    V, H, B = 33, 17, 7
    p = rbm_params(V, H)
    eng = rbm_engine(V, H, B, p, sample_v_states=False, sample_h_states=False)
    V0, clamp = start_and_clamp(B, V)
    check_against_twin(eng, p, V0, clamp, masks(B, V)['half'], 2, 'sample flags off')
    eng.close()


@pytest.mark.parametrize('V,H,B', [(100, 72, 37), (784, 1024, 40)])
def test_same_bits_in_fast_binary_mode_and_on_a_second_call(gpu_lib, V, H, B):
    p = rbm_params(V, H)
    V0, clamp = start_and_clamp(B, V)
    mask = masks(B, V)['half']
    eng = rbm_engine(V, H, B, p)
    first = run_engine(eng, V0, clamp, mask, 8)
    eng.seed(SEED)
    again = run_engine(eng, V0, clamp, mask, 8)
    eng.seed(SEED)
    eng.set_fast_binary(True, everywhere=True)
    fast = run_engine(eng, V0, clamp, mask, 8)
    for a, b, c in zip(first, again, fast):
        assert same(a, b) and same(a, c)
    eng.close()


def test_row_slices_reproduce_the_whole(gpu_lib):
    """the slice property: rows [r0, r1) run alone with set_row_offset(r0) are rows [r0, r1) of the whole"""
    V, H, B = 100, 72, 37
    p = rbm_params(V, H)
    V0, clamp = start_and_clamp(B, V)
    mask = masks(B, V)['half']
    eng = rbm_engine(V, H, B, p)
    whole = run_engine(eng, V0, clamp, mask, 3)
    for r0, r1 in ((0, 16), (16, 37), (5, 6)):
        eng.seed(SEED)
        eng.set_row_offset(r0)
        part = run_engine(eng, V0, clamp, mask, 3, B=r1 - r0, row=r0)
        for w, g in zip(whole, part):
            assert same(w[r0:r1], g[r0:r1])
    eng.close()


def test_rbm_refusals(gpu_lib):
    from boltzmann_machines_amd._ffi import Bm355Error, UNIT_MULTINOMIAL
    V, H, B = 20, 12, 5
    p = rbm_params(V, H)
    V0, clamp = start_and_clamp(B, V)
    mask = masks(B, V)['half']
    eng = rbm_engine(V, H, B, p)
    with pytest.raises(Bm355Error, match='max_batch'):
        run_engine(eng, np.tile(V0, (2, 1)), np.tile(clamp, (2, 1)), np.tile(mask, (2, 1)), 1)
    with pytest.raises(Bm355Error, match='max_batch'):
        run_engine(eng, V0, clamp, mask, 1, B=-1)
    with pytest.raises(Bm355Error, match='n_steps'):
        run_engine(eng, V0, clamp, mask, 0)
    eng.close()
    eng = rbm_engine(V, H, B, p, h_unit=UNIT_MULTINOMIAL, n_samples=3)
    with pytest.raises(Bm355Error, match='Multinomial'):
        run_engine(eng, V0, clamp, mask, 1)
    eng.close()
    from boltzmann_machines_amd.engine import RbmEngine64
    assert not hasattr(RbmEngine64, 'gibbs_clamped')


# ------------------------------------------------------------------------------------------------ DBM
DBM_SHAPES = [(20, [12, 16]), (33, [17, 9])]
M = 10


def dbm_state(V, nh, gaussian=False):
    n = [V] + nh
    W = [(orc.normal(SEED, 20 + i, 0, n[i] * n[i + 1]) * np.float32(0.2)).reshape(n[i], n[i + 1]) for i in range(len(nh))]
    hb = [(orc.uniform(SEED, 30 + i, 0, n[i + 1]) - np.float32(0.5)) * np.float32(0.6) for i in range(len(nh))]
    vb = (orc.uniform(SEED, 40, 0, V) - np.float32(0.5)) * np.float32(0.6)
    sigma = (np.float32(0.5) + orc.uniform(SEED, 41, 0, V)) if gaussian else np.ones(V, np.float32)
    v = (orc.uniform(SEED, 42, 0, M * V) < 0.5).astype(np.float32).reshape(M, V)
    Hs = [(orc.uniform(SEED, 50 + i, 0, M * n[i + 1]) < 0.5).astype(np.float32).reshape(M, n[i + 1]) for i in range(len(nh))]
    return W, hb, vb, sigma, v, Hs


def dbm_engine(V, nh, st, gaussian=False):
    from boltzmann_machines_amd.engine import DbmEngine
    W, hb, vb, sigma, v, Hs = st
    eng = DbmEngine(V, nh, v_unit=1 if gaussian else 0, n_particles=M, batch_size=M)
    sfx = lambda i: '' if i == 0 else '_%d' % i
    for i in range(len(nh)):
        eng.set('W' + sfx(i), W[i]); eng.set('hb' + sfx(i), hb[i]); eng.set('h' + sfx(i), Hs[i])
    eng.set('vb', vb); eng.set('sigma', sigma); eng.set('v', v)
    eng.seed(SEED)
    return eng


def dbm_run(eng, k, clamp=None, mask=None):
    from boltzmann_machines_amd._ffi import DeviceArray
    Vd = DeviceArray((M, eng.V))
    if mask is None:
        eng.sample_v(k, Vd)
    else:
        eng.sample_v_clamped(k, DeviceArray.from_numpy(clamp), DeviceArray.from_numpy(mask), Vd)
    eng.sync()
    sfx = lambda i: '' if i == 0 else '_%d' % i
    return Vd.numpy(), eng.get('v'), [eng.get('h' + sfx(i)) for i in range(eng.L)]


@pytest.mark.parametrize('k', [0, 1, 3])
@pytest.mark.parametrize('gaussian', [False, True])
@pytest.mark.parametrize('V,nh', DBM_SHAPES)
def test_dbm_matches_twin(gpu_lib, V, nh, gaussian, k):
    st = dbm_state(V, nh, gaussian)
    W, hb, vb, sigma, v, Hs = st
    _, clamp = start_and_clamp(M, V, gaussian)
    for name, mask in masks(M, V).items():
        eng = dbm_engine(V, nh, st, gaussian)
        got_v, got_pv, got_H = dbm_run(eng, k, clamp, mask)
        eng.close()
        want_v, want_pv, want_H = T.dbm_sample_v_clamped(W, hb, vb, sigma, v, Hs, k, SEED, clamp=clamp, mask=mask,
                                                         v_unit=1 if gaussian else 0)
        what = '%d-%s gaussian=%s k=%d mask %s' % (V, nh, gaussian, k, name)
        assert same(got_v, want_v), what + ': V'
        # (the particles' v takes the result of the mean sweeps: v <- v_means, dbm.py:646-647)
        assert same(got_pv, want_v), what + ': particle v'
        for g, w in zip(got_H, want_H):
            assert same(g, w), what + ': particle H'
        m = mask != 0
        assert same(got_v[m], clamp[m])
        if k == 0:                                            # no sweep runs: the clamp alone
            assert same(got_v, T.blend(mask, clamp, v))


@pytest.mark.parametrize('literal', [False, True])
@pytest.mark.parametrize('V,nh', DBM_SHAPES)
def test_dbm_zero_mask_is_sample_v(gpu_lib, V, nh, literal):
    """from the same state and seed; also with the literal sigmoid (the CL kernel of the parity tile) and in fast-binary mode"""
    st = dbm_state(V, nh)
    _, clamp = start_and_clamp(M, V)
    zero = np.zeros((M, V), np.float32)
    out = []
    for clamped, fast in ((False, False), (True, False), (True, True)):
        eng = dbm_engine(V, nh, st)
        eng.set_sigmoid_literal(literal)
        if fast and not literal:
            eng.set_fast_binary(True, everywhere=True)
        out.append(dbm_run(eng, 3, clamp, zero) if clamped else dbm_run(eng, 3))
        eng.close()
    for other in out[1:]:
        assert same(out[0][0], other[0]) and same(out[0][1], other[1])
        assert all(same(a, b) for a, b in zip(out[0][2], other[2]))


def test_dbm_refusals(gpu_lib):
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray, UNIT_MULTINOMIAL
    from boltzmann_machines_amd.engine import DbmEngine, DbmEngine64
    V, nh = 20, [12, 16]
    z = DeviceArray.from_numpy(np.zeros((M, V), np.float32))
    eng = DbmEngine(V, nh, n_particles=M, batch_size=M)
    with pytest.raises(Bm355Error, match='n_gibbs_steps'):
        eng.sample_v_clamped(-1, z, z)
    eng.close()
    eng = DbmEngine(V, nh, n_particles=M, batch_size=M, h_units=[0, UNIT_MULTINOMIAL], n_samples=[0, 3])
    with pytest.raises(Bm355Error, match='Multinomial'):
        eng.sample_v_clamped(1, z, z)
    eng.close()
    eng = DbmEngine64(V, nh, n_particles=M, batch_size=M)
    with pytest.raises(NotImplementedError):
        eng.sample_v_clamped(1, z, z)
    eng.close()


# ------------------------------------------------------------------------------------------------ public API
NV, NH, BS = 12, 8, 5
XTRAIN = (orc.uniform(SEED, 60, 0, 20 * NV) < 0.4).astype(np.float32).reshape(20, NV)


def weights(model):
    return dict(w=model.get_tf_params(scope='weights'), g=model.get_tf_params(scope='grads_accumulators'))


def assert_same_params(a, b):
    for s in a:
        assert set(a[s]) == set(b[s])
        for k in a[s]:
            assert np.array_equal(np.asarray(a[s][k]).view(np.uint32), np.asarray(b[s][k]).view(np.uint32)), (s, k)


def check_host_stream_and_state(model, call, transform_X):
    """the call draws exactly one seed from the host stream, changes no parameter, and `transform` behind it gives the
    bits it gives without it (host RNG state restored)"""
    rng = model._rng
    before = weights(model)
    st = rng.get_state()
    H1 = model.transform(transform_X)
    rng.set_state(st)
    out = call()
    after_call = model.make_random_seed()
    rng.set_state(st)
    model.make_random_seed()
    assert after_call == model.make_random_seed()
    assert_same_params(before, weights(model))
    rng.set_state(st)
    H2 = model.transform(transform_X)
    assert np.array_equal(H1.view(np.uint32), H2.view(np.uint32))
    rng.set_state(st)
    return out


@pytest.mark.parametrize('gaussian', [False, True])
def test_public_rbm(gpu_lib, tmp_path, gaussian):
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM
    kw = dict(n_visible=NV, n_hidden=NH, batch_size=BS, max_epoch=2, random_seed=1337, verbose=False,
              model_path=str(tmp_path / 'm') + '/')
    if gaussian:
        rbm = GaussianRBM(sigma=list(0.5 + 0.1 * np.arange(NV)), learning_rate=1e-3, **kw).fit(XTRAIN)
    else:
        rbm = BernoulliRBM(**kw).fit(XTRAIN)
    N = 13                                                     # > batch_size: three slices, the last one short
    X = XTRAIN[:N].copy()
    mask = (orc.uniform(SEED, 61, 0, N * NV) < 0.5).astype(np.float32).reshape(N, NV)
    V, Vm = check_host_stream_and_state(rbm, lambda: rbm.sample_v_given(X, mask, n_gibbs_steps=3, return_means=True), XTRAIN)
    assert V.shape == X.shape and Vm.shape == X.shape
    assert same(V[mask != 0], X[mask != 0]) and same(Vm[mask != 0], X[mask != 0])
    if not gaussian:
        assert set(np.unique(V)) <= {0.0, 1.0}
    # N > batch_size equals the concatenation of single-slice calls (every slice at its row offset, same seed)
    st = rbm._rng.get_state()
    eng = rbm._engine
    from boltzmann_machines_amd._ffi import DeviceArray
    Xin = X / np.asarray(rbm._sigma_vector(), np.float32)[None, :] if gaussian else X
    parts = []
    for r0 in range(0, N, BS):
        r1 = min(N, r0 + BS)
        seed = rbm.make_random_seed()
        rbm._rng.set_state(st)
        eng.seed(seed)
        eng.set_row_offset(r0)
        Vd, Hd = DeviceArray.from_numpy(Xin[r0:r1]), DeviceArray((r1 - r0, NH))
        eng.gibbs_clamped(Vd, Hd, r1 - r0, 3, DeviceArray.from_numpy(Xin[r0:r1]), DeviceArray.from_numpy(mask[r0:r1]))
        eng.sync()
        parts.append(Vd.numpy())
    eng.set_row_offset(0)
    free = mask == 0
    assert same(np.concatenate(parts)[free], V[free])
    # a [n_visible] mask is broadcast over the rows; n_gibbs_steps defaults to the model's
    row_mask = mask[0]
    Vb = rbm.sample_v_given(X, row_mask)
    rbm._rng.set_state(st)
    Vf = rbm.sample_v_given(X, np.tile(row_mask, (N, 1)), n_gibbs_steps=1)
    assert same(Vb, Vf)
    with pytest.raises(ValueError):
        rbm.sample_v_given(X, mask[:, :-1])
    with pytest.raises(ValueError):
        rbm.sample_v_given(X, mask, n_gibbs_steps=0)


def test_public_dbm(gpu_lib, tmp_path):
    from boltzmann_machines_amd import DBM, BernoulliRBM
    H2 = 6
    r1 = BernoulliRBM(n_visible=NV, n_hidden=NH, dbm_first=True, max_epoch=2, batch_size=BS, random_seed=11, verbose=False,
                      model_path=str(tmp_path / 'r1') + '/').fit(XTRAIN)
    r2 = BernoulliRBM(n_visible=NH, n_hidden=H2, dbm_last=True, max_epoch=2, batch_size=BS, random_seed=12, verbose=False,
                      model_path=str(tmp_path / 'r2') + '/').fit(r1.transform(XTRAIN))
    dbm = DBM(rbms=[r1, r2], n_particles=BS, n_gibbs_steps=2, max_mf_updates=5, mf_tol=1e-5, learning_rate=0.01, max_epoch=2,
              batch_size=BS, random_seed=1337, verbose=False, model_path=str(tmp_path / 'dbm') + '/').fit(XTRAIN)
    X = XTRAIN[:BS].copy()
    mask = (orc.uniform(SEED, 62, 0, BS * NV) < 0.5).astype(np.float32).reshape(BS, NV)
    particles = lambda: [dbm._engine.get(n) for n in ('v', 'v_new', 'h', 'h_new', 'h_1', 'h_new_1')]
    p0 = particles()
    V = check_host_stream_and_state(dbm, lambda: dbm.sample_v_given(X, mask, n_gibbs_steps=2), XTRAIN)
    assert V.shape == X.shape and same(V[mask != 0], X[mask != 0])
    assert np.all((V >= 0) & (V <= 1))
    assert all(same(a, b) for a, b in zip(p0, particles()))   # save_model=False: the persistent particles are untouched
    st = dbm._rng.get_state()
    Vb = dbm.sample_v_given(X, mask[0])                         # broadcast mask, the model's n_gibbs_steps (2)
    dbm._rng.set_state(st)
    Vf, Vm = dbm.sample_v_given(X, np.tile(mask[0], (BS, 1)), n_gibbs_steps=2, return_means=True)
    assert same(Vb, Vf) and same(Vf, Vm)
    with pytest.raises(ValueError):
        dbm.sample_v_given(XTRAIN[:BS + 1], mask)


def test_public_refusals(gpu_lib, tmp_path):
    from boltzmann_machines_amd import DBM, BernoulliRBM, MultinomialRBM
    kw = dict(n_visible=NV, n_hidden=NH, batch_size=BS, max_epoch=1, random_seed=1337, verbose=False)
    X, mask = XTRAIN[:BS], np.ones(NV)
    m = MultinomialRBM(n_samples=3, model_path=str(tmp_path / 'm') + '/', **kw).fit(XTRAIN)
    with pytest.raises(NotImplementedError, match='Multinomial'):
        m.sample_v_given(X, mask)
    r64 = BernoulliRBM(dtype='float64', model_path=str(tmp_path / 'f') + '/', **kw).fit(XTRAIN)
    with pytest.raises(NotImplementedError, match='float64'):
        r64.sample_v_given(X, mask)
    r1 = BernoulliRBM(dbm_first=True, model_path=str(tmp_path / 'a') + '/', **kw).fit(XTRAIN)
    r2 = MultinomialRBM(n_visible=NH, n_hidden=6, n_samples=3, dbm_last=True, batch_size=BS, max_epoch=1, random_seed=3,
                        verbose=False, model_path=str(tmp_path / 'b') + '/').fit(r1.transform(XTRAIN))
    dbm = DBM(rbms=[r1, r2], n_particles=BS, batch_size=BS, max_epoch=1, random_seed=5, verbose=False,
              model_path=str(tmp_path / 'd') + '/')
    dbm.init()
    with pytest.raises(NotImplementedError, match='Multinomial'):
        dbm.sample_v_given(X, mask)
    d64 = DBM(rbms=[r1, r2], n_particles=BS, batch_size=BS, max_epoch=1, random_seed=5, verbose=False, dtype='float64',
              model_path=str(tmp_path / 'e') + '/')
    with pytest.raises(NotImplementedError, match='float64'):         # (refused before anything is built)
        d64.sample_v_given(X, mask)
