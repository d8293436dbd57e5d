"""-m gpu: centred training - grad_kernel's centred flavour, cen_ema / rbm_cen_stats / cen_rowscal / cen_bias
kernels, bm_rbm_set_centering / bm_dbm_set_centering, BernoulliRBM / DBM.set_centering.

The shapes are chosen for the epilogue's edges: several 64 x 64 tiles in both directions, I % 8 != 0 (the scalar store path),
ldw % 4 == 0 with I % 8 == 0 (the vec8 path), a power-of-two and a non-power-of-two batch (the two division paths).
Bit-exact comparisons are view(uint32).  The DBM has no bit-exact twin: the oracle exports no raw DBM gradients, so its update
is checked against the float64 reference (tests/np_reference_centering.py) from the mu and particles the engine itself read."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import centering_twin as T
from tests import np_reference_centering as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 717171
LR, MOM, UPDATES = 0.05, 0.9, 3
RBM_NAMES = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')
# V, H, B, k, options
RBM_CASES = [(70, 75, 17, 1, {}), (64, 128, 16, 2, dict(sparsity_cost=0.1, sparsity_target=0.2)),
             (37, 29, 33, 1, dict(sample_v_states=True))]
# layers, N, M, options
DBM_CASES = [((70, 75, 33), 12, 10, {}), ((64, 64, 64), 16, 16, dict(max_norm=2.0, sparsity_cost=[0.05, 0.02], sparsity_target=[0.2, 0.1])),
             ((20, 12, 9, 7), 8, 8, {})]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what):
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), '%s: %s differs in %d of %d entries (max abs %.3g)' % (
            what, k, int(np.sum(bits(got[k]) != bits(want[k]))), want[k].size, float(np.abs(got[k] - want[k]).max()))


def rbm_params(V, H):
    return dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H) * np.float32(0.3),
                vb=(orc.uniform(SEED, 2, 0, V) - np.float32(0.5)) * np.float32(0.6),
                hb=(orc.uniform(SEED, 3, 0, H) - np.float32(0.5)) * np.float32(0.6))


def data(n, V, site=6):
    return (orc.uniform(SEED, site, 0, n * V) < 0.4).astype(np.float32).reshape(n, V)


def dev(a):
    from boltzmann_machines_amd._ffi import DeviceArray
    return DeviceArray.from_numpy(np.ascontiguousarray(a, np.float32))


def rbm_engine(V, H, max_batch, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    eng = RbmEngine(V, H, max_batch=max_batch, l2=1e-3, **kw)
    p = rbm_params(V, H)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, p[n])
    eng.seed(SEED)
    return eng


def rbm_state(eng, offsets=False):
    return {n: eng.get(n) for n in RBM_NAMES + (('ov', 'oh') if offsets else ())}


# ---- 1. zero offsets are the plain update
def check_rbm_zero(case, **over):
    V, H, B, k, opt = RBM_CASES[case]
    opt = dict(opt, **over)
    X = data(UPDATES * B, V)
    Xd = dev(X)
    plain, cen = rbm_engine(V, H, B, **opt), rbm_engine(V, H, B, **opt)
    cen.set_centering(True, 0.0, 0.0)
    for u in range(UPDATES):
        plain.train_step(Xd, B, LR, MOM, k, row=u * B)
        cen.train_step(Xd, B, LR, MOM, k, row=u * B)
        assert_same(rbm_state(cen), rbm_state(plain), 'RBM case %d, update %d, zero offsets against the plain update' % (case, u))
    assert not cen.get('ov').any() and not cen.get('oh').any()
    # ... and so are the metrics entry and the native epoch loop
    out_p = plain.train_step_metrics(Xd, B, LR, MOM, k)
    out_c = cen.train_step_metrics(Xd, B, LR, MOM, k)
    assert np.array_equal(bits(out_p), bits(out_c))
    plain.train_epoch(Xd, 2 * B, B, LR, MOM, k)
    cen.train_epoch(Xd, 2 * B, B, LR, MOM, k)
    assert_same(rbm_state(cen), rbm_state(plain), 'RBM case %d, metrics step + epoch' % case)


@pytest.mark.parametrize('case', range(len(RBM_CASES)))
def test_rbm_zero_offsets_are_the_plain_update(gpu_lib, case):
    check_rbm_zero(case)


def test_rbm_zero_offsets_sparsity_toggled(gpu_lib):
    """the 70 x 75 case with sparsity on, the 64 x 128 case with it off (the plain update then takes its one-launch form)"""
    check_rbm_zero(0, sparsity_cost=0.1, sparsity_target=0.2)
    check_rbm_zero(1, sparsity_cost=0.0)


def dbm_names(L):
    sfx = lambda i: '' if i == 0 else '_%d' % i
    out = ['vb', 'dvb', 'v']
    for i in range(L):
        out += [b + sfx(i) for b in ('W', 'dW', 'hb', 'dhb', 'q_means', 'mu_means', 'mu', 'h')]
    return out


def dbm_engine(case, **over):
    from boltzmann_machines_amd.engine import DbmEngine
    n, N, M, opt = DBM_CASES[case]
    opt = dict(opt, **over)
    L = len(n) - 1
    eng = DbmEngine(n[0], list(n[1:]), sample_v_states=True, n_particles=M, batch_size=N, max_mf_updates=6, mf_tol=1e-6,
                    l2=1e-3, **opt)
    eng.set('vb', (orc.uniform(SEED, 20, 0, n[0]) - np.float32(0.5)) * np.float32(0.4))
    eng.set('v', (orc.uniform(SEED, 21, 0, M * n[0]) < 0.5).astype(np.float32).reshape(M, n[0]))
    for i in range(L):
        s = '' if i == 0 else '_%d' % i
        eng.set('W' + s, orc.normal(SEED, 22 + i, 0, n[i] * n[i + 1]).reshape(n[i], n[i + 1]) * np.float32(0.3))
        eng.set('hb' + s, (orc.uniform(SEED, 26 + i, 0, n[i + 1]) - np.float32(0.5)) * np.float32(0.4))
        eng.set('h' + s, (orc.uniform(SEED, 30 + i, 0, M * n[i + 1]) < 0.5).astype(np.float32).reshape(M, n[i + 1]))
    eng.seed(SEED)
    return eng


def dbm_state(eng, L):
    return {k: eng.get(k) for k in dbm_names(L)}


def check_dbm_zero(case, updates=UPDATES + 2):
    """(five updates: from the fourth on the odd layers' outer products run on the second stream)"""
    n, N, M, _ = DBM_CASES[case]
    L = len(n) - 1
    Xd = dev(data(N, n[0]))
    plain, cen = dbm_engine(case), dbm_engine(case)
    cen.set_centering(True, 0.0)
    for u in range(updates):
        a = plain.train_step(Xd, LR, MOM, 2)
        b = cen.train_step(Xd, LR, MOM, 2)
        assert a[0] == b[0]
        assert_same(dbm_state(cen, L), dbm_state(plain, L), 'DBM case %d, update %d, zero offsets against the plain update' % (case, u))
    for name in ['ov'] + ['oh' + ('' if i == 0 else '_%d' % i) for i in range(L)]:
        assert not cen.get(name).any()


@pytest.mark.parametrize('case', range(len(DBM_CASES)))
def test_dbm_zero_offsets_are_the_plain_update(gpu_lib, case):
    check_dbm_zero(case)


# ---- 2. the RBM against the float32 twin, bit for bit
@functools.lru_cache(maxsize=None)
def rbm_twin_run(case):
    V, H, B, k, opt = RBM_CASES[case]
    X = data(UPDATES * B, V)
    o = [X[:B].astype(np.float64).mean(0).astype(np.float32), np.full(H, 0.5, np.float32)]
    t = T.CentredRBM(rbm_params(V, H), (0.1, 0.1), o, seed=SEED, l2=1e-3, **opt)
    out = []
    for u in range(UPDATES):
        t.train_step(X[u * B:(u + 1) * B], LR, MOM, k)
        out.append(t.state())
    return X, o, out


def check_rbm_twin(case):
    V, H, B, k, opt = RBM_CASES[case]
    X, o, want = rbm_twin_run(case)
    Xd = dev(X)
    eng = rbm_engine(V, H, B, **opt)
    eng.set_centering(True, 0.1, 0.1)
    eng.set('ov', o[0]); eng.set('oh', o[1])
    for u in range(UPDATES):
        eng.train_step(Xd, B, LR, MOM, k, row=u * B)
        assert_same(rbm_state(eng, offsets=True), want[u], 'RBM case %d, update %d against the twin' % (case, u))
    assert np.abs(want[-1]['ov'] - o[0]).max() > 1e-3           # the offsets moved


@pytest.mark.parametrize('case', range(len(RBM_CASES)))
def test_rbm_against_the_twin(gpu_lib, case):
    check_rbm_twin(case)


# ---- 3. the DBM update alone against the float64 reference
def check_dbm_update(case):
    """after every train_step the engine's mu and particles are what its update read: the expected new parameters follow from
    the previous ones in float64.  rtol 1e-5, atol 1e-6 * max|param|"""
    n, N, M, opt = DBM_CASES[case]
    L = len(n) - 1
    sfx = lambda i: '' if i == 0 else '_%d' % i
    X = data(N, n[0])
    Xd = dev(X)
    eng = dbm_engine(case)
    nu = [0.1, 0.2, 0.05, 0.1][:L + 1]
    eng.set_centering(True, nu)
    onames = ['ov'] + ['oh' + sfx(i) for i in range(L)]
    eng.set('ov', X.astype(np.float64).mean(0).astype(np.float32))
    for i in range(L):
        eng.set('oh' + sfx(i), np.float32(0.5))
    f64 = lambda a: np.asarray(a, np.float64)

    def read_state():
        s = R.State(list(n))
        s.W = [f64(eng.get('W' + sfx(i))) for i in range(L)]
        s.dW = [f64(eng.get('dW' + sfx(i))) for i in range(L)]
        s.b = [f64(eng.get('vb'))] + [f64(eng.get('hb' + sfx(i))) for i in range(L)]
        s.db = [f64(eng.get('dvb'))] + [f64(eng.get('dhb' + sfx(i))) for i in range(L)]
        s.q = [None] + [f64(eng.get('q_means' + sfx(i))) for i in range(L)]
        s.mm = [None] + [f64(eng.get('mu_means' + sfx(i))) for i in range(L)]
        s.o = [f64(eng.get(name)) for name in onames]
        return s
    # (the engine moves q_means / mu_means whether or not the sparsity cost is 0: the reference gets the terms in every case)
    sparsity = dict(kind='dbm', cost=[float(np.float32(c)) for c in opt.get('sparsity_cost', [0.] * L)],
                    target=[float(np.float32(c)) for c in opt.get('sparsity_target', [0.1] * L)], damping=float(np.float32(0.9)))
    for u in range(UPDATES):
        before = read_state()
        eng.train_step(Xd, LR, MOM, 2)
        pos = [f64(X)] + [f64(eng.get('mu' + sfx(i))) for i in range(L)]
        neg = [f64(eng.get('v'))] + [f64(eng.get('h' + sfx(i))) for i in range(L)]
        want = R.update_standard(before, pos, neg, [float(np.float32(x)) for x in nu], float(np.float32(LR)),
                                 mom=float(np.float32(MOM)), l2=float(np.float32(1e-3)), sparsity=sparsity,
                                 max_norm=opt.get('max_norm', np.inf))
        got = read_state()
        for name, g, w in ([('W' + sfx(i), got.W[i], want.W[i]) for i in range(L)] +
                           [('dW' + sfx(i), got.dW[i], want.dW[i]) for i in range(L)] +
                           [('b%d' % l, got.b[l], want.b[l]) for l in range(L + 1)] +
                           [('db%d' % l, got.db[l], want.db[l]) for l in range(L + 1)] +
                           [('q_means%d' % l, got.q[l], want.q[l]) for l in range(1, L + 1)] +
                           [('mu_means%d' % l, got.mm[l], want.mm[l]) for l in range(1, L + 1)] +
                           [('o%d' % l, got.o[l], want.o[l]) for l in range(L + 1)]):
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-6 * np.abs(w).max(),
                                       err_msg='DBM case %d, update %d: %s' % (case, u, name))


@pytest.mark.parametrize('case', range(len(DBM_CASES)))
def test_dbm_update_against_float64(gpu_lib, case):
    check_dbm_update(case)


# ---- 4. every instantiated centred geometry (and a forced one without a centred instantiation: the documented fall-back to 4)
@pytest.mark.parametrize('geo', ['4', '8', '108'])
def test_forced_geometry(gpu_lib, geo):
    code = ('import sys; sys.path.insert(0, %r)\n'
            'from tests import test_centering_gpu as G\n'
            'G.check_rbm_zero(0); G.check_rbm_twin(0); G.check_dbm_zero(0); G.check_dbm_update(0)\n'
            'print("CENTRED_GEOMETRY_OK")\n') % ROOT
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, BM355_DEBUG='grad_geo=' + geo), capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and 'CENTRED_GEOMETRY_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 5. centred and tempered together
def test_rbm_centred_and_tempered(gpu_lib):
    V, H, M, Rn, B, k = 37, 29, 24, 3, 17, 2
    betas = np.linspace(0., 1., Rn + 1)[1:].astype(np.float32)
    X = data(UPDATES * B, V)
    Xd = dev(X)
    # zero offsets: the plain tempered step
    plain, cen = rbm_engine(V, H, B), rbm_engine(V, H, B)
    cen.set_centering(True, 0.0, 0.0)
    for e in (plain, cen):
        e.pt_init(M, betas)
    for u in range(UPDATES):
        plain.train_step_pt(Xd, B, LR, MOM, k, row=u * B)
        cen.train_step_pt(Xd, B, LR, MOM, k, row=u * B)
    assert_same(rbm_state(cen), rbm_state(plain), 'tempered RBM, zero offsets')
    # the twin composed from pt_train_twin and the centred apply
    o = [X[:B].astype(np.float64).mean(0).astype(np.float32), np.full(H, 0.5, np.float32)]
    t = T.tempered_centred_rbm(rbm_params(V, H), M, betas, SEED, (0.1, 0.1), o, l2=1e-3)
    eng = rbm_engine(V, H, B)
    eng.set_centering(True, 0.1, 0.1)
    eng.set('ov', o[0]); eng.set('oh', o[1])
    eng.pt_init(M, betas)
    for u in range(UPDATES):
        t.train_step(X[u * B:(u + 1) * B], LR, MOM, k)
        eng.train_step_pt(Xd, B, LR, MOM, k, row=u * B)
    assert (min(t.ens.margins) if t.ens.margins else np.inf) >= 1e-9, 'a swap draw lies within 1e-9 of its threshold: choose another seed'
    want = t.state()
    assert_same(rbm_state(eng, offsets=True), {n: want[n] for n in RBM_NAMES + ('ov', 'oh')}, 'tempered RBM against the twin')


def test_dbm_centred_and_tempered(gpu_lib):
    from boltzmann_machines_amd.engine import DbmEngine
    n, N, M = (20, 12, 9), 8, 8
    betas = np.linspace(0., 1., 4)[1:].astype(np.float32)
    Xd = dev(data(N, n[0]))

    def make():
        eng = DbmEngine(n[0], list(n[1:]), sample_v_states=True, n_particles=M, batch_size=N, max_mf_updates=6, mf_tol=1e-6, l2=1e-3)
        eng.set('vb', (orc.uniform(SEED, 20, 0, n[0]) - np.float32(0.5)) * np.float32(0.4))
        for i in range(2):
            s = '' if i == 0 else '_%d' % i
            eng.set('W' + s, orc.normal(SEED, 22 + i, 0, n[i] * n[i + 1]).reshape(n[i], n[i + 1]) * np.float32(0.3))
        eng.seed(SEED)
        eng.pt_init(M, betas)
        return eng
    plain, cen = make(), make()
    cen.set_centering(True, 0.0)
    for u in range(UPDATES + 2):
        plain.train_step_pt(Xd, LR, MOM, 2)
        cen.train_step_pt(Xd, LR, MOM, 2)
    assert_same(dbm_state(cen, 2), dbm_state(plain, 2), 'tempered DBM, zero offsets')


# ---- 6. public API
def test_public_rbm(gpu_lib, tmp_path):
    from boltzmann_machines_amd import BernoulliRBM
    V, H, N, BS = 37, 29, 40, 10
    X = data(N, V)

    def model(tag, **kw):
        return BernoulliRBM(n_visible=V, n_hidden=H, batch_size=BS, max_epoch=2, learning_rate=0.05, momentum=0.5, l2=0.,
                            random_seed=77, verbose=False, model_path=str(tmp_path / tag) + '/', **kw)
    plain = model('plain').fit(X)
    keys = sorted(np.load(str(tmp_path / 'plain' / 'model.npz')).files)
    assert keys == sorted(['W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means', 'sigma'])          # nothing new for a never-centred model
    assert sorted(f for f in os.listdir(str(tmp_path / 'plain')) if os.path.isfile(str(tmp_path / 'plain' / f))) == \
        ['model.npz', 'params.json', 'random_state.json']
    m = model('a').set_centering(nu_v=0.1, nu_h=0.1)
    assert m.get_params().keys() == plain.get_params().keys()
    m.fit(X)
    o2 = m.centering_offsets()
    assert np.array_equal(np.load(str(tmp_path / 'a' / 'model.npz'))['centering_ov'], o2[0])
    assert np.abs(o2[1] - np.float32(0.5)).max() > 1e-4                                       # the hidden offsets moved
    assert not np.array_equal(m.get_tf_params('weights')['W'], plain.get_tf_params('weights')['W'])
    loaded = BernoulliRBM.load_model(str(tmp_path / 'a') + '/')
    assert [np.array_equal(a, b) for a, b in zip(loaded.centering_offsets(), o2)] == [True, True]
    m.set_params(max_epoch=3).fit(X)
    loaded.set_params(max_epoch=3).fit(X)
    for k in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(m.get_tf_params('weights')[k]), bits(loaded.get_tf_params('weights')[k])), k
    for a, b in zip(m.centering_offsets(), loaded.centering_offsets()):
        assert np.array_equal(bits(a), bits(b))
    # both negative phases
    t = model('t').set_centering().set_negative_phase('tempered', n_temperatures=3).fit(X)
    assert np.all(np.isfinite(t.get_tf_params('weights')['W']))


def test_public_dbm(gpu_lib, tmp_path):
    from boltzmann_machines_amd import DBM
    from tests.test_dbm_api_gpu import X, make_dbm
    plain, _ = make_dbm(tmp_path, 'p')
    plain.fit(X)
    assert not [k for k in np.load(plain._model_filepath + '.npz').files if k.startswith('centering')]
    d, _ = make_dbm(tmp_path, 'c')
    assert d.set_centering(nu=[0.1, 0.1, 0.05]) is d
    d.fit(X)
    o = d.centering_offsets()
    assert len(o) == 3 and np.abs(o[1] - np.float32(0.5)).max() > 1e-4
    z = np.load(d._model_filepath + '.npz')
    assert np.array_equal(z['centering_oh_1'], o[2]) and np.array_equal(z['centering_nu'], np.float32([0.1, 0.1, 0.05]))
    loaded = DBM.load_model(d._model_dirpath)
    assert all(np.array_equal(a, b) for a, b in zip(loaded.centering_offsets(), o))
    d.set_params(max_epoch=3).fit(X)
    loaded.set_params(max_epoch=3).fit(X)
    for k in ('W', 'W_1', 'vb', 'hb', 'hb_1'):
        assert np.array_equal(bits(d.get_tf_params('weights')[k]), bits(loaded.get_tf_params('weights')[k])), k
    for a, b in zip(d.centering_offsets(), loaded.centering_offsets()):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(d.get_tf_params('weights')['W'], plain.set_params(max_epoch=3).fit(X).get_tf_params('weights')['W'])


def test_flip_invariance_through_rbm_fit(gpu_lib, tmp_path):
    """BernoulliRBM.fit on X from theta and on 1 - X from the flipped theta, all sampling off, l2 = 0, offsets left at their
    defaults (data mean / 0.5 - so the default initialisation and the hand-over to the engine are part of what is tested): the
    two models stay flip-equivalent.  The float32 twin (tests/centering_twin.fit_twin) shows a deviation of 7.15e-07 on this case
    on the CPU (T.FIT_TWIN_DEVIATION = 7.2e-07, kept honest by tests/test_centering.py); the tolerance is ten times that,
    7.2e-06.  Without centering the same pair ends 1e-3 or more apart."""
    from boltzmann_machines_amd import BernoulliRBM
    F = T.FIT
    p, X = T.fit_case()

    def fit(tag, p, X, centred):
        m = BernoulliRBM(n_visible=F['V'], n_hidden=F['H'], W_init=p['W'], vb_init=p['vb'], hb_init=p['hb'], batch_size=F['batch'],
                         max_epoch=F['epochs'], learning_rate=F['lr'], momentum=F['mom'], l2=0., sample_v_states=False,
                         sample_h_states=False, random_seed=5, verbose=False, model_path=str(tmp_path / tag) + '/')
        if centred:
            m.set_centering(nu_v=F['nu'], nu_h=F['nu'])
        m.fit(X)
        w = m.get_tf_params('weights')
        o = m.centering_offsets() if centred else [np.zeros(F['V'], np.float32), np.zeros(F['H'], np.float32)]
        return dict(W=w['W'], vb=w['vb'], hb=w['hb'], ov=o[0], oh=o[1])
    a, b = fit('a', p, X, True), fit('b', T.flip_params(p), 1 - X, True)
    gap = T.flip_gap(a, b)
    print('flip gap through BernoulliRBM.fit: %.3g (tolerance %.3g)' % (gap, 10 * T.FIT_TWIN_DEVIATION))
    assert gap <= 10 * T.FIT_TWIN_DEVIATION, gap
    a, b = fit('c', p, X, False), fit('d', T.flip_params(p), 1 - X, False)
    b['ov'] = 1 - a['ov']                                   # (no offsets to compare)
    assert T.flip_gap(a, b) >= 1e-3


def test_flip_invariance_through_dbm_fit(gpu_lib, tmp_path):
    """DBM.fit on X from theta and on 1 - X from the flipped theta (particles v -> 1 - v), all sampling off, a fixed number of
    mean-field sweeps (mf_tol = 0), l2 = 0, no max-norm, no sparsity, default offsets.  No bit-exact float32 twin of the DBM
    exists (the oracle exports no raw DBM gradients); the float32 restatement is tests/np_reference_centering.py run in float32,
    which shows a deviation of 2.38e-07 on this case on the CPU (R.FIT_F32_DEVIATION = 2.4e-07, kept honest by
    tests/test_centering.py); the tolerance is ten times that, 2.4e-06."""
    from boltzmann_machines_amd import DBM, BernoulliRBM
    s, X, P = R.fit_case()
    n = R.FIT_N

    def fit(tag, s, X, P):
        kw = dict(max_epoch=1, batch_size=R.FIT_BATCH, verbose=False, random_seed=5)
        # RBMs that only carry the start: composed, the DBM's hb is 0.5 hb_1 + 0.5 vb_2 (dbm.py:287-290)
        r1 = BernoulliRBM(n_visible=n[0], n_hidden=n[1], W_init=s.W[0], vb_init=s.b[0], hb_init=2 * s.b[1].astype(np.float64),
                          dbm_first=True, model_path=str(tmp_path / (tag + 'r1')) + '/', **kw).init()
        r2 = BernoulliRBM(n_visible=n[1], n_hidden=n[2], W_init=s.W[1], vb_init=np.zeros(n[1], np.float32), hb_init=s.b[2],
                          dbm_last=True, model_path=str(tmp_path / (tag + 'r2')) + '/', **kw).init()
        d = DBM(rbms=[r1, r2], n_particles=R.FIT_BATCH, v_particle_init=P[0], h_particles_init=[P[1], P[2]], n_gibbs_steps=1,
                max_mf_updates=R.FIT_MF, mf_tol=0., learning_rate=R.FIT_LR, momentum=R.FIT_MOM, max_epoch=R.FIT_EPOCHS,
                batch_size=R.FIT_BATCH, l2=0., sample_v_states=False, sample_h_states=[False, False], random_seed=7,
                verbose=False, model_path=str(tmp_path / (tag + 'dbm')) + '/')
        d.set_centering(nu=R.FIT_NU).fit(X)
        w, out = d.get_tf_params('weights'), R.State(list(n))
        out.W, out.b, out.o = [w['W'], w['W_1']], [w['vb'], w['hb'], w['hb_1']], d.centering_offsets()
        out.dW, out.db = [np.zeros_like(x) for x in out.W], [np.zeros_like(x) for x in out.b]
        return out
    a = fit('a', s, X, P)
    b = fit('b', R.flip(s), 1 - X, [1 - P[0]] + P[1:])
    assert np.abs(a.W[0] - s.W[0]).max() > 1e-3                      # it trained
    gap = R.flip_gap(a, b)
    print('flip gap through DBM.fit: %s (tolerance %.3g)' % ({k: float(v) for k, v in gap.items()}, 10 * R.FIT_F32_DEVIATION))
    assert max(gap.values()) <= 10 * R.FIT_F32_DEVIATION, gap


# ---- 7. refusals at the library level
def test_library_refusals(gpu_lib):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import DbmEngine, RbmEngine
    for kw in (dict(v_unit=_ffi.UNIT_GAUSSIAN), dict(h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=5), dict(dbm_first=True),
               dict(dbm_last=True), dict(dropout=0.8)):
        eng = RbmEngine(12, 8, max_batch=4, **kw)
        with pytest.raises(_ffi.Bm355Error, match='centering'):
            eng.set_centering(True)
        eng.set_centering(False)
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        DbmEngine(12, [8, 6], v_unit=_ffi.UNIT_GAUSSIAN, n_particles=4, batch_size=4).set_centering(True)
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        DbmEngine(12, [8, 6], h_units=[0, _ffi.UNIT_MULTINOMIAL], n_samples=[0, 5], n_particles=4, batch_size=4).set_centering(True)
    Xd = dev(data(4, 12))
    eng = RbmEngine(12, 8, max_batch=4)
    eng.set_centering(True)
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        eng.grad_step(Xd, 4, 1)
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        eng.apply_step(4, 0.1, 0.5)
    eng.set_centering(False)
    eng.grad_step(Xd, 4, 1)
    eng.apply_step(4, 0.1, 0.5)
    d = DbmEngine(12, [8, 6], n_particles=4, batch_size=4)
    d.set_centering(True)
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        d.grad_step(Xd, 1)
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        d.apply_step(4, 4, 0.1, 0.5)
    # the exchange's fused applies: refused for the handle's mode before the exchange object is looked at
    eng.set_centering(True)
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        _ffi.check(gpu_lib.bm_rbm_exchange_apply_direct(eng._h, None, 4, 0.1, 0.5))
    with pytest.raises(_ffi.Bm355Error, match='centering'):
        _ffi.check(gpu_lib.bm_dbm_exchange_apply_direct(d._h, None, 4, 4, 0.1, 0.5))
    eng.set_centering(False)
    d.set_centering(False)
    for call in (lambda: gpu_lib.bm_rbm_exchange_apply_direct(eng._h, None, 4, 0.1, 0.5),
                 lambda: gpu_lib.bm_dbm_exchange_apply_direct(d._h, None, 4, 4, 0.1, 0.5)):
        with pytest.raises(_ffi.Bm355Error) as e:          # (centering off: the null exchange is what is wrong now)
            _ffi.check(call())
        assert 'centering' not in str(e.value)
