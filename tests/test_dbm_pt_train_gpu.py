"""-m gpu: the DBM's tempered negative phase - pt_rescore_kernel with two jobs, the three-matrix
pt_gather_kernel, bm_dbm_train_step_pt, DBM.set_negative_phase / tempering_stats.

The engine is compared BIT FOR BIT (view(uint32)) with the CPU twin of tests/dbm_pt_train_twin.py over FIVE consecutive updates
(the second stream of the update's tail switches on at the fourth): every parameter, momentum buffer, q_means, mu_means, mu,
the dense particles, the ensemble's beta = 1 states of all layers, the ladder index of EVERY row and the swap counters, the
mean-field trip count; msre to the 1e-5 relative of the existing parity tests.  Shapes ((V, n1, n2), batch, particles, R,
chains): (37, 20, 11) with 5 x 3 (ragged everywhere, fewer rows than a tile) and again with 7 chains for 5 particles (the
hand-over takes a prefix of the chains), (70, 65, 33) with 7 x 4 (both K segments cross BK with a remainder), (64, 64, 64) with
8 x 4 (the aligned paths), the one-layer stack (37, 20) (no h2 job in the re-scoring, two matrices in the gather).  k = 2, so
the swap parity alternates inside an update and continues across them.  The swap decision compares a uniform with a double
exp(): every case first asserts on the twin that NO draw lies within 1e-9 of its threshold, and then excludes nothing."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import dbm_pt_train_twin as P
from tests import test_dbm_pt_gpu as G

pytestmark = pytest.mark.gpu

SEED = G.SEED
CASES = [((37, 20, 11), 6, 5, 3, 5), ((37, 20, 11), 6, 5, 3, 7), ((70, 65, 33), 16, 7, 4, 7), ((64, 64, 64), 8, 8, 4, 8),
         ((37, 20), 6, 5, 3, 5)]                                                    # (V, n1, n2), batch, particles, R, chains
FULL_CASE = (G.FULL, 100, 100, 4, 100)
K, LR, MOM, UPDATES = 2, 0.05, 0.5, 5
bits, same, ladder, dbm_params = G.bits, G.same, G.ladder, G.dbm_params


def config(n):
    L = len(n) - 1
    return dict(max_mf_updates=5, mf_tol=1e-5, l2=1e-3, max_norm=1.5 if n[0] < 256 else 6.0,
                sparsity_target=[0.2, 0.1][:L], sparsity_cost=[1e-2, 5e-3][:L])


def data(rows, V, s=0):
    return (orc.uniform(SEED, 70 + s, 0, rows * V) < 0.3).astype(np.float32).reshape(rows, V)


def _engine(n, B, M, **kw):
    from boltzmann_machines_amd.engine import DbmEngine
    p = dbm_params(n)
    eng = DbmEngine(n[0], list(n[1:]), n_particles=M, batch_size=B, **kw)
    for i in range(len(n) - 1):
        eng.set('W' + P.sfx(i), p['W'][i])
        eng.set('hb' + P.sfx(i), p['hb'][i])
    eng.set('vb', p['vb'])
    eng.seed(SEED)
    return eng


def twin(n, B, M, R, chains, **kw):
    return P.TemperedDBM(dbm_params(n), M, B, chains, ladder(R), SEED, **kw)


def engine_state(eng, t, chains):
    """the engine's counterpart of TemperedDBM.state()"""
    from boltzmann_machines_amd._ffi import DeviceArray
    Vd = DeviceArray((chains, eng.V))
    Hd = [DeviceArray((chains, k)) for k in eng.n_hiddens]
    swaps, idx = eng.pt_read(Vd, *Hd)
    out = {nm: eng.get(nm) for nm in t.names()}
    out.update(ens_V=Vd.numpy(), idx=np.array(idx, np.int32).reshape(-1), swaps=np.array(swaps, np.int64))
    for i, h in enumerate(Hd):
        out['ens_H%d' % (i + 1)] = h.numpy()
    return out


def assert_same_state(got, want, what):
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        if k in ('idx', 'swaps'):
            continue
        assert same(got[k], want[k]), '%s: %s differs from the twin in %d of %d entries' % (
            what, k, int(np.sum(bits(got[k]) != bits(want[k]))), want[k].size)
    assert np.array_equal(got['idx'], want['idx']), '%s: ladder indices differ' % what
    assert np.array_equal(got['swaps'], want['swaps']), '%s: swap counters %s against %s' % (what, got['swaps'].tolist(), want['swaps'].tolist())


def assert_decisive(t, mixed=True):
    m = t.ens.margins
    assert (min(m) if m else np.inf) >= 1e-9, 'a swap draw of this case lies within 1e-9 of its threshold: choose another seed'
    att, acc = t.ens.cnt
    assert np.all(att > 0) and (not mixed or 0 < acc.sum() < att.sum())


@functools.lru_cache(maxsize=None)
def twin_run(case):
    """(state, n_mf, msre) after every one of the UPDATES updates of CASES[case] (computed once, shared, never modified), and
    the twin"""
    n, B, M, R, chains = CASES[case]
    t = twin(n, B, M, R, chains, **config(n))
    X = data(UPDATES * B, n[0])
    out = []
    for u in range(UPDATES):
        n_mf, msre = t.train_step(X[u * B:(u + 1) * B], LR, MOM, K, want_msre=True)
        out.append((t.state(), n_mf, msre))
    return out, t


def decisive_twin(case):
    out, t = twin_run(case)
    assert_decisive(t)
    return out


def engine_run(case):
    from boltzmann_machines_amd._ffi import DeviceArray
    n, B, M, R, chains = CASES[case]
    t = twin_run(case)[1]
    eng = _engine(n, B, M, **config(n))
    eng.pt_init(chains, ladder(R))
    Xd = DeviceArray.from_numpy(data(UPDATES * B, n[0]))
    out = []
    for u in range(UPDATES):
        n_mf, msre = eng.train_step_pt(Xd, LR, MOM, K, row=u * B, want_msre=True)
        out.append((engine_state(eng, t, chains), n_mf, msre))
    eng.close()
    return out


@pytest.mark.parametrize('case', range(len(CASES)))
def test_updates_match_the_twin(gpu_lib, case):
    """five consecutive updates with momentum, l2, the sparsity penalty and a finite max_norm"""
    want = decisive_twin(case)
    got = engine_run(case)
    for u, ((g, gn, gm), (w, wn, wm)) in enumerate(zip(got, want)):
        what = 'case %d, update %d' % (case, u)
        assert gn == wn, '%s: %d mean-field sweeps against %d' % (what, gn, wn)
        np.testing.assert_allclose(gm, wm, rtol=1e-5, err_msg=what)
        assert_same_state(g, w, what)
    assert not same(got[0][0]['W'], got[1][0]['W']) and not same(got[0][0]['vb'], got[1][0]['vb'])
    n, B, M, R, chains = CASES[case]
    g = got[-1][0]
    assert same(g['v'], g['ens_V'][:M]) and same(g['h'], g['ens_H1'][:M])          # the hand-over, on the device's own word


@functools.lru_cache(maxsize=None)
def twin_full():
    n, B, M, R, chains = FULL_CASE
    t = twin(n, B, M, R, chains, **config(n))
    X = data(2 * B, n[0], 1)
    res = [t.train_step(X[u * B:(u + 1) * B], LR, MOM, 1, want_msre=True) for u in range(2)]
    return t.state(), res, t


def decisive_full():
    state, res, t = twin_full()
    assert_decisive(t, mixed=False)
    return state, res, t


def test_full_size_two_updates(gpu_lib):
    """784-512-1024, batch 100, 100 particles, 100 chains x 4 temperatures, k = 1, two updates: the tuned geometries, the
    LDS-DMA loop and the x-major operands"""
    from boltzmann_machines_amd._ffi import DeviceArray
    want, res, t = decisive_full()
    n, B, M, R, chains = FULL_CASE
    eng = _engine(n, B, M, **config(n))
    eng.pt_init(chains, ladder(R))
    Xd = DeviceArray.from_numpy(data(2 * B, n[0], 1))
    for u in range(2):
        n_mf, msre = eng.train_step_pt(Xd, LR, MOM, 1, row=u * B, want_msre=True)
        assert n_mf == res[u][0]
        np.testing.assert_allclose(msre, res[u][1], rtol=1e-5)
    got = engine_state(eng, t, chains)
    eng.close()
    assert_same_state(got, want, '784-512-1024')


@functools.lru_cache(maxsize=None)
def twin_between_sweeps():
    n, B, M, R, chains = CASES[2]
    t = twin(n, B, M, R, chains, **config(n))
    t.pt_sweep(3)
    part = (t.ens.part_v.copy(), t.ens.part_h2.copy())
    t.train_step(data(B, n[0], 2), 0.0, MOM, 3)
    t.pt_sweep(3)
    return t.state(), part, t


def decisive_between_sweeps():
    state, part, t = twin_between_sweeps()
    assert_decisive(t)
    return state, part, t


def test_zero_learning_rate_update_between_two_sweeps(gpu_lib):
    """The re-scoring identity on the device: bm_dbm_pt_sweep(3), an update with lr = 0 and k = 3, bm_dbm_pt_sweep(3) leave the
    ensemble where the twin's three sweeps leave it (the twin's re-scoring is asserted to rewrite the same bits; vb and the hb
    keep their bits at lr = 0; the twin's last sweep follows the W of the oracle's update, which the max-norm rescale (w n) / n
    may move in its last place - W itself is compared too, against the oracle's).  Odd step counts: the parity runs through"""
    from boltzmann_machines_amd._ffi import DeviceArray
    want, part, t = decisive_between_sweeps()
    n, B, M, R, chains = CASES[2]
    p = dbm_params(n)
    # on the twin: a re-scoring of the state after the first sweep rewrites what is there
    chk = twin(n, B, M, R, chains, **config(n))
    chk.pt_sweep(3)
    chk.ens.rescore()
    assert same(chk.ens.part_v, part[0]) and same(chk.ens.part_h2, part[1])
    eng = _engine(n, B, M, **config(n))
    eng.pt_init(chains, ladder(R))
    eng.pt_sweep(3)
    eng.train_step_pt(DeviceArray.from_numpy(data(B, n[0], 2)), 0.0, MOM, 3)
    assert same(eng.get('vb'), p['vb']) and same(eng.get('hb'), p['hb'][0]) and same(eng.get('hb_1'), p['hb'][1])
    eng.pt_sweep(3)
    got = engine_state(eng, t, chains)
    eng.close()
    assert_same_state(got, want, 'sweep, lr = 0 update, sweep')
    assert want['swaps'][0].sum() > 0 and np.all(want['dvb'] == 0)


def test_other_entry_points_are_untouched(gpu_lib):
    """bm_dbm_sample_v, bm_dbm_train_step, bm_dbm_pt_init / _sweep / _read and bm_rbm_train_step_pt give the same bits whether
    or not a tempered update ran on the handle before them.  The update legitimately moves the variables (parameters, momentum
    buffers, running means, mu, the dense particles): they are set back through bm_dbm_set_param, so what could still differ is
    state behind the variables - the ensemble, the counters, the streams.  (On a build without the entry point the update is
    left out and the test compares the existing entry points with themselves.)"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import DbmEngine, RbmEngine
    n, B, M, R, chains = CASES[2]
    X = data(B, n[0], 3)
    names = ['vb', 'dvb', 'v', 'v_new'] + [b + P.sfx(i) for i in range(2)
                                            for b in ('W', 'dW', 'hb', 'dhb', 'q_means', 'mu_means', 'mu', 'mu_new', 'h', 'h_new')]
    init = dict(v=G.start(M, n[0]), h=(orc.uniform(SEED, 21, 0, M * n[1]) < 0.5).astype(np.float32).reshape(M, n[1]),
                h_1=(orc.uniform(SEED, 22, 0, M * n[2]) < 0.5).astype(np.float32).reshape(M, n[2]))
    results = []
    for tempered in (False, True):
        eng = _engine(n, B, M, **config(n))
        for k, v in init.items():
            eng.set(k, v)
        if tempered and hasattr(DbmEngine, 'train_step_pt'):
            before = {k: eng.get(k) for k in names}
            eng.pt_init(chains, ladder(R))
            for u in range(4):                     # (past the updates at which the second stream switches on)
                eng.train_step_pt(DeviceArray.from_numpy(X), LR, MOM, K)
            assert not same(before['W'], eng.get('W')) and not same(before['v'], eng.get('v'))
            for k, v in before.items():
                eng.set(k, v)
            eng.seed(SEED)
        Vd = DeviceArray((M, n[0]))
        eng.sample_v(2, Vd)
        eng.train_step(DeviceArray.from_numpy(X), LR, MOM, 1)
        eng.pt_init(chains, ladder(R))
        eng.pt_sweep(G.STEPS)
        snap = G.engine_read(eng, chains)
        results.append([Vd.numpy()] + [eng.get(k) for k in names] + [snap[k] for k in sorted(snap)])
        eng.close()
    for a, b in zip(*results):
        assert np.array_equal(np.asarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else a,
                              np.asarray(b).view(np.uint32) if np.asarray(b).dtype == np.float32 else b)
    # the RBM shares only the moved re-scoring kernel (and the generalised gather, under BM355_DEBUG=pt_sel=0): its tempered
    # update against ITS twin, one update of the first case of tests/test_pt_train_gpu.py
    from tests import test_pt_train_gpu as RG
    want = RG.decisive_twin(0)[0]
    V, H, Rr, Mr, Br, kr = RG.CASES[0]
    rbm = RG.rbm_engine(V, H, RG.rbm_params(V, H), Br, **RG.config(0))
    rbm.pt_init(Mr, RG.ladder(Rr))
    rbm.train_step_pt(DeviceArray.from_numpy(RG.data(RG.UPDATES * Br, V)), Br, RG.LR, RG.MOM, kr)
    got = RG.engine_state(rbm, Mr)
    rbm.close()
    RG.assert_same_state(got, want, 'bm_rbm_train_step_pt')


def test_entry_point_errors(gpu_lib):
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray, UNIT_GAUSSIAN, UNIT_MULTINOMIAL
    n = (20, 12, 9)
    Xd = DeviceArray.from_numpy(data(4, n[0]))
    eng = G.dbm_engine(n, dbm_params(n))                       # 4 particles, batch 4
    with pytest.raises(Bm355Error, match='no ensemble'):
        eng.train_step_pt(Xd, LR, MOM, 1)
    eng.pt_init(3, [0.5, 1.0])
    with pytest.raises(Bm355Error, match='fewer than n_particles'):
        eng.train_step_pt(Xd, LR, MOM, 1)
    eng.pt_init(4, [0.5, 1.0])
    with pytest.raises(Bm355Error, match='n_gibbs_steps'):
        eng.train_step_pt(Xd, LR, MOM, 0)
    before = eng.get('W')
    eng.train_step_pt(Xd, LR, MOM, 1)
    assert not same(before, eng.get('W'))
    eng.set_sigmoid_literal(True)
    with pytest.raises(Bm355Error, match='literal'):
        eng.train_step_pt(Xd, LR, MOM, 1)
    eng.set_sigmoid_literal(False)
    eng.set_mf_allreduce(lambda x: x)                            # what a data-parallel job attaches
    with pytest.raises(Bm355Error, match='not sharded over ranks'):
        eng.train_step_pt(Xd, LR, MOM, 1)
    eng.set_mf_allreduce(None)
    eng.train_step_pt(Xd, LR, MOM, 1)
    eng.close()
    # Gaussian / Multinomial / three-layer handles never get an ensemble: bm_dbm_pt_init refuses them (test_dbm_pt_gpu.py), and
    # without one the update names that
    for kw, nn in ((dict(v_unit=UNIT_GAUSSIAN), n), (dict(h_units=[0, UNIT_MULTINOMIAL], n_samples=[0, 3]), n), (dict(), (20, 12, 9, 7))):
        eng = G.dbm_engine(nn, dbm_params(nn), **kw)
        with pytest.raises(Bm355Error, match='no ensemble'):
            eng.train_step_pt(DeviceArray.from_numpy(data(4, nn[0])), LR, MOM, 1)
        eng.close()


# ------------------------------------------------------------------------------------------------ public API
def _oracle_of(dbm, variables, seed):
    """an OracleDBM in the state `variables` (engine names) of a two-layer public model, at call 0 of `seed`"""
    o = orc.OracleDBM(dbm.n_visible_, dbm.n_hiddens_, n_particles=dbm.n_particles, batch_size=dbm.batch_size,
                      max_mf_updates=dbm.max_mf_updates, mf_tol=dbm.mf_tol, l2=dbm.l2, max_norm=dbm.max_norm,
                      sparsity_target=dbm.sparsity_target, sparsity_cost=dbm.sparsity_cost, sparsity_damping=dbm.sparsity_damping)
    for k, v in variables.items():
        if k in o.p:
            o.p[k][...] = v
    o.set_seed(seed)
    return o


PUBLIC_R, PUBLIC_SEED = 3, 1337


@functools.lru_cache(maxsize=None)
def public_graph_seeds():
    """the seeds the model's host stream hands to init() (the AIS op seed drawn while the graph is built) and to the two
    fit() calls of test_public_tempered_fit - a function of random_seed = 1337 alone"""
    from boltzmann_machines_amd.utils import RNG
    r = RNG(seed=PUBLIC_SEED)
    draw = lambda: r.randint(2 ** 31 - 1)
    return draw(), draw(), draw()


@functools.lru_cache(maxsize=None)
def twin_public(init_items):
    """the twin of the tempered fit of test_public_tempered_fit from the model's initial variables (a tuple of (name, bytes,
    shape) so that the cache can key on it)"""
    variables = {k: np.frombuffer(b, np.float32).reshape(s).copy() for k, b, s in init_items}
    p = dict(W=[variables['W'], variables['W_1']], vb=variables['vb'], hb=[variables['hb'], variables['hb_1']])
    t = P.TemperedDBM(p, G.BS, G.BS, G.BS, ladder(PUBLIC_R), public_graph_seeds()[1], max_mf_updates=5, mf_tol=1e-5)
    for k, v in variables.items():
        if k in t.p:
            t.p[k][...] = v
    for s in range(0, len(G.XTRAIN), G.BS):
        t.train_step(G.XTRAIN[s:s + G.BS], 0.01, 0.9, 1)
    return t


def decisive_public():
    """(CPU) the near-tie guard of the public case needs the model's initial variables, which only a device run composes; the
    guard is asserted inside test_public_tempered_fit.  Here: the seeds are what the test will assume"""
    assert len(set(public_graph_seeds())) == 3


def test_public_tempered_fit(gpu_lib, tmp_path):
    from boltzmann_machines_amd import DBM
    dbm = G._fitted_dbm(tmp_path)
    assert dbm.set_negative_phase('tempered', n_temperatures=PUBLIC_R) is dbm
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        dbm.tempering_stats()
    dbm.init()
    names = [nm for nm, _ in dbm._var_names() if nm != 'sigma']
    init = {nm: dbm._engine.get(nm) for nm in names}
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        dbm.tempering_stats()
    dbm.fit(G.XTRAIN)
    assert dbm._graph_seed == public_graph_seeds()[1]
    t = twin_public(tuple((k, init[k].tobytes(), init[k].shape) for k in sorted(init)))
    assert_decisive(t, mixed=False)            # (a stack pre-trained for one epoch is nearly flat: every swap may be accepted)
    for nm in t.names():
        assert same(dbm._engine.get(nm), t.p[nm]), nm
    swaps, idx = dbm._engine.pt_read()
    assert np.array_equal(swaps, t.ens.cnt) and np.array_equal(idx.reshape(-1), t.ens.idx)
    assert np.array_equal(dbm.tempering_stats(), t.ens.cnt[1] / t.ens.cnt[0].astype(np.float64))
    assert np.all(t.ens.cnt[0] == [2 * G.BS, 2 * G.BS])                # 4 updates x 1 step: each parity twice
    # the checkpoint: the handed-over particles, the reference's variable set, no ensemble and no setting
    loaded = DBM.load_model(dbm._model_dirpath)
    assert sorted(loaded._pending_vars) == sorted(nm for nm, _ in dbm._var_names())
    for nm in ('v', 'h', 'h_1'):
        assert same(loaded._pending_vars[nm], t.p[nm]), nm
    assert loaded._neg_phase is None
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        loaded.tempering_stats()
    import json
    assert not any('neg' in k or 'temper' in k for k in json.load(open(dbm._params_filepath)))
    # sample_v() continues from the handed-over particles
    o = _oracle_of(dbm, {nm: dbm._engine.get(nm) for nm in names}, 0)
    st = dbm._rng.get_state()
    Pv = dbm.sample_v(n_gibbs_steps=2)
    dbm._rng.set_state(st)
    o.set_seed(dbm.make_random_seed())
    o.sample_v(2)
    assert same(Pv, o.p['v'])
    dbm._rng.set_state(st)
    # back to 'cd': a second epoch is the plain update, from the state the tempered epoch left (the oracle's own train_step)
    dbm.set_negative_phase('cd')
    dbm.max_epoch = 2
    o = _oracle_of(dbm, {nm: dbm._engine.get(nm) for nm in names}, public_graph_seeds()[2])
    dbm.fit(G.XTRAIN)
    assert dbm._graph_seed == public_graph_seeds()[2]
    for s in range(0, len(G.XTRAIN), G.BS):
        o.train_step(G.XTRAIN[s:s + G.BS], 0.01, 0.9, 1)
    for nm in t.names():
        assert same(dbm._engine.get(nm), o.p[nm]), nm
    with pytest.raises(ValueError, match='kind'):
        dbm.set_negative_phase('pt')
    # sample_v_tempered replaces the training ensemble
    dbm.sample_v_tempered(3, n_gibbs_steps=2, n_temperatures=2)
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        dbm.tempering_stats()


def test_public_default_is_untouched(gpu_lib, tmp_path):
    """set_negative_phase('tempered') followed by set_negative_phase('cd') trains the model that never left the default"""
    a = G._fitted_dbm(tmp_path, 'a').fit(G.XTRAIN)
    b = G._fitted_dbm(tmp_path, 'b').set_negative_phase('tempered', n_temperatures=4, n_chains=9).set_negative_phase('cd').fit(G.XTRAIN)
    for nm, _ in a._var_names():
        if nm != 'sigma':
            assert same(a._engine.get(nm), b._engine.get(nm)), nm


def test_public_refusals(gpu_lib, tmp_path):
    """on built models (the CPU test has them on bare ones): the errors surface as NotImplementedError / ValueError, at
    set_negative_phase and again when a fit starts"""
    d = G._fitted_dbm(tmp_path, 't', third=True)
    with pytest.raises(NotImplementedError, match='OLD layer above'):
        d.set_negative_phase('tempered')
    d = G._fitted_dbm(tmp_path, 'f', dtype='float64')
    with pytest.raises(NotImplementedError, match='float64'):
        d.set_negative_phase('tempered')
    d = G._fitted_dbm(tmp_path, 'l').set_negative_phase('tempered', n_temperatures=2)
    d.set_mean_field_arithmetic('reference')
    with pytest.raises(NotImplementedError, match='literal'):
        d.fit(G.XTRAIN)
    d = G._fitted_dbm(tmp_path, 'c')
    with pytest.raises(ValueError, match='n_chains'):
        d.set_negative_phase('tempered', n_chains=G.BS - 1)
