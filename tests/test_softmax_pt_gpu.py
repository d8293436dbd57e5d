"""-m gpu: parallel tempering and the tempered negative phase over softmax visible units - the SM + SA + RT flavour
of act_kernel, softmax_pt_init_kernel, the generic route's tempered groups kernel, bm_rbm_groups_pt_init / _sweep / _read,
bm_rbm_groups_train_step_pt / _train_epoch_pt, CategoricalRBM.sample_v_tempered / set_group_tempering.

The engine is compared BIT FOR BIT with the CPU twin of tests/softmax_pt_twin.py: the states of both layers, both partial arrays,
the rows' temperatures, the ladder indices and the swap counters of the WHOLE ensemble.  The cases are the twin module's
SWEEP_CASES / TRAIN_CASES: tests/test_softmax_pt.py shows that none of their swap draws lies within 1e-9 of its threshold (0 near
ties), so nothing is excluded.  BM355_DEBUG switches are read once per process: every run under one is a fresh child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import softmax_pt_twin as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENS = ('v', 'h', 'part_v', 'part_h', 'mult', 'idx', 'swaps')
NAMES = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')
LR, MOM, L2 = 0.05, 0.5, 1e-3


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def make_engine(p, K, max_batch=4, seed=None, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = p['W'].shape
    eng = RbmEngine(V, H, max_batch=max_batch, v_groups=K, **kw)          # (max_batch does not bound the ensemble)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, p[n])
    if seed is not None:
        eng.seed(seed)
    return eng


def assert_same_ensemble(got, want, what):
    for n in ENS:
        if want[n] is None:                         # (the h.(vW + hb) partials before the first prop-up: not written yet)
            continue
        if n in ('idx', 'swaps'):
            assert np.array_equal(got[n], want[n]), '%s: %s %s against %s' % (what, n, got[n].tolist(), want[n].tolist())
        else:
            assert got[n].shape == want[n].shape, (what, n, got[n].shape, want[n].shape)
            assert np.array_equal(got[n], want[n]), '%s: %s differs from the twin in %d entries' % (what, n, int(np.sum(got[n] != want[n])))


def one_hot_rows(v, G, K):
    return bool(np.all((v == 0) | (v == 1)) and np.all(v.reshape(len(v), G, K).sum(axis=2) == 1))


@functools.lru_cache(maxsize=None)
def twin_snaps(c, chain0=S.SWEEP_CHAIN0, M=None):
    """the twin's three snapshots of a case (computed once, shared, never modified)"""
    return S.sweep_twin(c, chain0=chain0, M=M)[1]


def engine_snaps(c, chain0=S.SWEEP_CHAIN0, M=None, eng=None):
    """bm_rbm_groups_pt_init at call 0 of SWEEP_SEED, then sweeps of 3 and of 2 steps; the whole ensemble after each"""
    G, K, H, M_, R = c
    M = M_ if M is None else M
    own = eng is None
    if own:
        eng = make_engine(S.make_params(G, K, H), K)
    eng.seed(S.SWEEP_SEED)
    pt = eng.groups_pt
    pt.pt_init(M, S.ladder(R), chain0=chain0)
    out = [pt.pt_state()]
    for n in (3, 2):
        pt.pt_sweep(n)
        out.append(pt.pt_state())
    if own:
        eng.close()
    return out


def check_sweep_case(c):
    G, K, H, M, R = c
    got, want = engine_snaps(c), twin_snaps(c)
    assert one_hot_rows(got[0]['v'], G, K)
    for n, (g, w) in enumerate(zip(got, want)):
        assert_same_ensemble(g, w, '%s, snapshot %d' % (S.case_id(c), n))
        assert one_hot_rows(g['v'], G, K)
        assert np.array_equal(np.sort(g['idx'].reshape(M, R), axis=1), np.tile(np.arange(R), (M, 1)))
        assert np.array_equal(g['mult'], S.ladder(R)[g['idx']])
    if R > 1:
        assert np.all(got[-1]['swaps'][0] > 0)


# ------------------------------------------------------------------------------------------------ sweeps
def test_the_cases_cover_the_table():
    assert {c[:2] for c in S.SWEEP_CASES} == set(S.FUSED_SHAPES + S.GENERIC_SHAPES)
    assert {c[2] for c in S.SWEEP_CASES} == set(S.HIDDEN) and {c[3:] for c in S.SWEEP_CASES} == set(S.ENSEMBLES)


@pytest.mark.parametrize('case', S.SWEEP_CASES, ids=S.case_id)
def test_engine_matches_twin(gpu_lib, case):
    """random start (every row one-hot per group, the twin's start), then two consecutive sweeps of 3 and 2 steps: call counter,
    parity continuation, a chain0 != 0"""
    check_sweep_case(case)


def test_one_temperature_from_v0_is_the_plain_chain(gpu_lib):
    """R = 1, betas = (1,) from a V0: the twin's plain softmax chain, on both routes' shapes"""
    from boltzmann_machines_amd._ffi import DeviceArray
    for G, K, H, M in ((5, 4, 24, 7), (3, 5, 8, 7)):
        p = S.make_params(G, K, H)
        V0 = S.train_batches(G, K, M, 3)
        eng = make_engine(p, K, seed=77)
        pt = eng.groups_pt
        pt.pt_init(M, [1.0], DeviceArray.from_numpy(V0))
        assert np.array_equal(pt.pt_state()['v'], V0)
        pt.pt_sweep(3)
        got = pt.pt_state()
        eng.close()
        v, h = S.plain_chain(p, K, V0, 3, 77)
        assert np.array_equal(got['v'], v) and np.array_equal(got['h'], h), (G, K)
        assert got['swaps'].size == 0


@pytest.mark.parametrize('case', [(5, 4, 8, 5, 3), (3, 5, 24, 5, 3)], ids=['fused', 'generic'])
def test_chain_slices_and_determinism(gpu_lib, case):
    """chains [2, 5) of an ensemble of 7 at chain0 = 4 are the ensemble of 3 at chain0 = 6; a second run gives the same bits; a start
    from V0 replicates the chain's row"""
    from boltzmann_machines_amd._ffi import DeviceArray
    G, K, H, _, R = case
    whole = engine_snaps(case, chain0=4, M=7)
    again = engine_snaps(case, chain0=4, M=7)
    part = engine_snaps(case, chain0=6, M=3)
    for n, (a, b, c, w) in enumerate(zip(whole, again, part, twin_snaps(case, chain0=4, M=7))):
        assert_same_ensemble(a, w, 'whole, snapshot %d' % n)
        for k in ('v', 'h', 'mult', 'idx'):
            if n == 0 and k == 'h':
                continue
            assert np.array_equal(a[k], b[k]), (n, k)
            assert np.array_equal(a[k][2 * R:5 * R], c[k]), (n, k)
        for k in ('part_v', 'part_h'):
            if n == 0 and k == 'part_h':
                continue
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k][:, 2 * R:5 * R], c[k]), (n, k)
        assert np.array_equal(a['swaps'], b['swaps'])
    eng = make_engine(S.make_params(G, K, H), K, seed=5)
    V0 = S.train_batches(G, K, 4, 9)
    eng.groups_pt.pt_init(4, S.ladder(R), DeviceArray.from_numpy(V0), chain0=3)
    st = eng.groups_pt.pt_state()
    eng.close()
    assert np.array_equal(st['v'], np.repeat(V0, R, axis=0))
    assert np.array_equal(st['part_v'], S.T.slot_partials(np.repeat(V0, R, axis=0) * S.make_params(G, K, H)['vb'][None, :]).T)


# ------------------------------------------------------------------------------------------------ training
@functools.lru_cache(maxsize=None)
def twin_updates(c, lr=LR, steps=(4, 4, 4)):
    """the twin's state after every update of a training case (batches of `steps` rows, k = 2)"""
    G, K, H, M, R = c
    t = S.TemperedCategoricalRBM(S.make_params(G, K, H), K, M, S.ladder(R), S.TRAIN_SEED, l2=L2)
    X = S.train_batches(G, K, sum(steps), 1)
    out, s = [], 0
    for B in steps:
        t.train_step(X[s:s + B], lr, MOM, 2)
        out.append(t.state())
        s += B
    return out


def engine_state(eng):
    out = {n: eng.get(n) for n in NAMES}
    out.update(eng.groups_pt.pt_state())
    return out


def assert_same_state(got, want, what):
    for n in NAMES:
        assert np.array_equal(bits(got[n]), bits(want[n])), '%s: %s differs from the twin in %d entries' % (what, n, int(np.sum(bits(got[n]) != bits(want[n]))))
    assert_same_ensemble(got, want, what)


def engine_updates(c, lr=LR, steps=(4, 4, 4), epoch=None):
    """pt_init at call 0 of TRAIN_SEED, then one groups_train_step_pt per entry of `steps` (epoch = batch: one
    groups_train_epoch_pt over all rows instead); the state after every update (epoch: after the last)"""
    from boltzmann_machines_amd.engine import as_device
    G, K, H, M, R = c
    eng = make_engine(S.make_params(G, K, H), K, max_batch=5, seed=S.TRAIN_SEED, l2=L2)
    pt = eng.groups_pt
    pt.pt_init(M, S.ladder(R))
    Xd = as_device(S.train_batches(G, K, sum(steps), 1))
    out, s = [], 0
    if epoch:
        pt.train_epoch_pt(Xd, sum(steps), epoch, lr, MOM, 2)
        out.append(engine_state(eng))
    else:
        for B in steps:
            pt.train_step_pt(Xd, B, lr, MOM, 2, row=s)
            out.append(engine_state(eng))
            s += B
    eng.close()
    return out


def check_train_case(c):
    for n, (g, w) in enumerate(zip(engine_updates(c), twin_updates(c))):
        assert_same_state(g, w, '%s, update %d' % (S.case_id(c), n))


@pytest.mark.parametrize('case', S.TRAIN_CASES, ids=S.case_id)
def test_updates_match_the_twin(gpu_lib, case):
    """three groups_train_step_pt updates: every parameter, every momentum buffer and the whole ensemble, bit for bit"""
    check_train_case(case)


@pytest.mark.parametrize('case', [S.TRAIN_CASES[0], S.TRAIN_CASES[2]], ids=['fused', 'generic'])
def test_zero_learning_rate_update_is_a_sweep(gpu_lib, case):
    """lr = 0: the parameters keep their bits, and two updates of k = 2 leave the ensemble two sweeps of 2 steps leave - the rescore
    in front of each rewrote the partials that were there"""
    G, K, H, M, R = case
    got = engine_updates(case, lr=0.0, steps=(4, 4))
    p = S.make_params(G, K, H)
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(got[-1][n]), bits(p[n])), n
    eng = make_engine(p, K, max_batch=5, seed=S.TRAIN_SEED, l2=L2)
    eng.groups_pt.pt_init(M, S.ladder(R))
    for n in range(2):
        eng.groups_pt.pt_sweep(2)
        assert_same_ensemble(eng.groups_pt.pt_state(), got[n], 'sweep %d against the lr = 0 update' % n)
    eng.close()
    assert_same_state(got[-1], twin_updates(case, lr=0.0, steps=(4, 4))[-1], 'lr = 0 against the twin')


@pytest.mark.parametrize('case', [S.TRAIN_CASES[0], S.TRAIN_CASES[2]], ids=['fused', 'generic'])
def test_native_loop_equals_single_steps(gpu_lib, case):
    """groups_train_epoch_pt over 10 rows in batches of 4: the steps of 4, 4 and 2 rows (a short last batch)"""
    steps = engine_updates(case, steps=(4, 4, 2))[-1]
    loop = engine_updates(case, steps=(4, 4, 2), epoch=4)[-1]
    assert_same_state(loop, steps, 'epoch against steps')
    assert_same_state(loop, twin_updates(case, steps=(4, 4, 2))[-1], 'epoch against the twin')


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import softmax_pt_twin as S
from tests import test_softmax_pt_gpu as G
for c in %(sweeps)r:
    G.check_sweep_case(c)
for c in %(trains)r:
    G.check_train_case(c)
print('SOFTMAX_PT_OK')
'''
SMALLEST = (5, 4, 8, 5, 3)
FUSED_SWEEPS = [c for c in S.SWEEP_CASES if c[:2] in S.FUSED_SHAPES][::2]
SWITCHES = [('sm_fused=0', FUSED_SWEEPS, [S.TRAIN_CASES[0]])] + \
           [('act_geo=' + g, [SMALLEST, (5, 4, 24, 33, 4)], [S.TRAIN_CASES[0]]) for g in ('8', '1', '3', '108', '101', '103')] + \
           [('pt_sel=0', [], list(S.TRAIN_CASES))]


@pytest.mark.parametrize('dbg,sweeps,trains', SWITCHES, ids=[s[0] for s in SWITCHES])
def test_routes_geometries_and_hand_over_give_the_same_bits(gpu_lib, dbg, sweeps, trains):
    """a fresh child process per switch: the fused shapes down the generic route (sm_fused=0), every geometry SM has under either
    staging at the smallest fused shape (act_geo), the gather launch in place of the hand-over in the pass (pt_sel=0) - each
    against the twin, so against the default run, bit for bit"""
    env = dict(os.environ, BM355_DEBUG=dbg)
    r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, sweeps=sweeps, trains=trains)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and 'SOFTMAX_PT_OK' in r.stdout, '%s: %s' % (dbg, r.stdout[-2000:] + r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ what a tempered call leaves untouched
@pytest.mark.parametrize('K,G,H,B', [(4, 33, 24, 37), (5, 13, 24, 37)], ids=['fused', 'generic'])
def test_a_tempered_call_leaves_the_handle_as_it_was(gpu_lib, K, G, H, B):
    """bm_rbm_train_step against its twin before and behind an init, a sweep and a read (the sweep consumes one call of the stream,
    nothing else), bm_rbm_groups_ais the same bits on both sides and its twin's values"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from tests import softmax_ais_twin as AT
    from tests import test_softmax_v_gpu as SV
    eng, twin = SV.pair(K, G, H, B, 3)
    X = SV.categories(B, G, K, 2)
    SV.three_updates(eng, twin, X, 1, what='before')
    before = {n: eng.get(n).copy() for n in SV.STATE}
    a1 = eng.groups_ais(10, 21, 2, 5, chain0=9)
    pt = eng.groups_pt
    pt.pt_init(6, S.ladder(3))
    pt.pt_sweep(3)
    Vd = DeviceArray((6, G * K), f32)
    swaps, idx = pt.pt_read(Vd)
    assert one_hot_rows(Vd.numpy(), G, K) and swaps.shape == (2, 2) and idx.shape == (6, 3)
    twin.call += 1
    for n in SV.STATE:
        assert np.array_equal(bits(eng.get(n)), bits(before[n])), n
    a2 = eng.groups_ais(10, 21, 2, 5, chain0=9)
    assert np.array_equal(bits(a1), bits(a2))
    want, ties = AT.ais({n: before[n] for n in ('W', 'vb', 'hb')}, K, 10, 21, 2, 5, chain0=9)
    keep = ties == 0
    assert np.sum(~keep) * 4 <= len(keep)
    np.testing.assert_allclose(a1[keep], want[keep], rtol=1e-5)
    SV.three_updates(eng, twin, X, 1, what='behind the tempered calls')
    eng.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_point_refusals(gpu_lib):
    """every refusal of the five entries, the handle still training afterwards; bm_rbm_set_visible_groups(0) discards the ensemble"""
    from boltzmann_machines_amd._ffi import Bm355Error
    from boltzmann_machines_amd.engine import RbmEngine, as_device
    G, K, H = 5, 4, 8
    p = S.make_params(G, K, H)
    Xd = as_device(S.train_batches(G, K, 8, 1))
    plain = RbmEngine(G * K, H, max_batch=6)
    calls = lambda pt: (lambda: pt.pt_init(5, [0.5, 1.0]), lambda: pt.pt_sweep(1), lambda: pt.pt_read(),
                        lambda: pt.train_step_pt(Xd, 4, LR, MOM, 1), lambda: pt.train_epoch_pt(Xd, 8, 4, LR, MOM, 1))
    for call in calls(plain.groups_pt):
        with pytest.raises(Bm355Error, match='needs a handle with visible groups'):
            call()
    plain.close()
    eng = make_engine(p, K, max_batch=6, seed=1)
    pt = eng.groups_pt
    pt._pt_shape = (5, 2)
    for call in calls(pt)[1:]:
        with pytest.raises(Bm355Error, match='no ensemble'):
            call()
    eng.groups_set_missing(True)
    for call in calls(pt):
        with pytest.raises(Bm355Error, match='bm_rbm_groups_set_missing'):
            call()
    eng.groups_set_missing(False)
    for M, betas in ((0, [0.5, 1.0]), (5, [0.5, 0.9]), (5, [0.6, 0.5, 1.0]), (5, [0.0, 1.0]), (5, [])):
        with pytest.raises(Bm355Error, match='beta|n_temps|ensemble'):
            pt.pt_init(M, betas)
    with pytest.raises(Bm355Error, match='chain0'):
        pt.pt_init(5, [0.5, 1.0], chain0=-1)
    pt.pt_init(5, [0.5, 1.0])
    for B in (0, 6, 7):                                          # min(max_batch = 6, n_chains = 5) = 5
        with pytest.raises(Bm355Error, match='batch'):
            pt.train_step_pt(Xd, B, LR, MOM, 1)
    with pytest.raises(Bm355Error, match='batch'):
        pt.train_epoch_pt(Xd, 8, 6, LR, MOM, 1)
    for call in (lambda: pt.pt_sweep(0), lambda: pt.train_step_pt(Xd, 4, LR, MOM, 0)):
        with pytest.raises(Bm355Error, match='>= 1'):
            call()
    # the Bernoulli entries keep refusing this handle
    for call in (lambda: eng.pt_init(5, [0.5, 1.0]), lambda: eng.pt_sweep(1), lambda: eng.train_step_pt(Xd, 4, LR, MOM, 1)):
        with pytest.raises(Bm355Error, match='softmax visible'):
            call()
    # the handle still trains, tempered and plain
    pt.train_step_pt(Xd, 5, LR, MOM, 1)
    pt.train_epoch_pt(Xd, 8, 5, LR, MOM, 1)
    eng.train_step(Xd, 6, LR, MOM, 1)
    eng.sync()
    assert all(np.all(np.isfinite(eng.get(n))) for n in NAMES)
    # groups off: the ensemble goes with them
    eng.set_visible_groups(0)
    with pytest.raises(Bm355Error, match='no ensemble'):
        eng.pt_sweep(1)
    eng.set_visible_groups(K)
    with pytest.raises(Bm355Error, match='no ensemble'):
        pt.pt_sweep(1)
    eng.close()


# ------------------------------------------------------------------------------------------------ public API
NG, NK, NH, BS, NROWS = 4, 4, 12, 10, 60
XTRAIN = S.train_batches(NG, NK, NROWS, 7)


def _model(tmp_path, name, **kw):
    from boltzmann_machines_amd import CategoricalRBM
    p = S.make_params(NG, NK, NH, std=0.1)
    base = dict(n_groups=NG, n_categories=NK, n_hidden=NH, batch_size=BS, max_epoch=2, random_seed=1337, verbose=False, n_gibbs_steps=2,
                learning_rate=0.01, momentum=0.9, l2=1e-4, W_init=p['W'], vb_init=p['vb'], hb_init=p['hb'], model_path=str(tmp_path / name) + '/')
    return CategoricalRBM(**dict(base, **kw))


def test_public_fit_matches_the_twin(gpu_lib, tmp_path):
    """fit() under set_group_tempering on 60 rows, two epochs of 6 updates, a metrics iteration every 10th (it consumes one call of
    the stream and changes nothing else), against the twin driven by the same host seed; tempering_stats equals the counters"""
    rbm = _model(tmp_path, 'a').set_group_tempering(n_temperatures=4, n_chains=BS + 3)
    seed1 = _model(tmp_path, 'seeds').make_random_seed()
    rbm.fit(XTRAIN)
    t = S.TemperedCategoricalRBM(S.make_params(NG, NK, NH, std=0.1), NK, BS + 3, S.ladder(4), seed1, l2=1e-4)
    it = 0
    for epoch in range(2):
        for s in range(0, NROWS, BS):
            it += 1
            if it % 10 == 0:
                t.call += 1                                  # bm_rbm_metrics
            t.train_step(XTRAIN[s:s + BS], 0.01, 0.9, 2)
    assert t.ens.near_ties() == 0, 'a swap draw lies within 1e-9 of its threshold: choose another seed'
    assert rbm.iter_ == it == 12
    assert_same_state(engine_state(rbm._engine), t.state(), 'fit')
    rates = rbm.tempering_stats()
    assert rates.shape == (3,) and np.all((rates >= 0) & (rates <= 1))
    assert np.array_equal(rates, t.ens.cnt[1] / np.maximum(t.ens.cnt[0], 1).astype(np.float64))
    from boltzmann_machines_amd import CategoricalRBM
    assert CategoricalRBM.load_model(str(tmp_path / 'a') + '/')._neg_phase is None
    # the sampler: one-hot rows, rates in [0, 1]; it replaces the training ensemble
    V, acc = rbm.sample_v_tempered(7, n_gibbs_steps=5, n_temperatures=3, return_stats=True)
    assert V.shape == (7, NG * NK) and one_hot_rows(V, NG, NK)
    assert acc.shape == (2,) and np.all((acc >= 0) & (acc <= 1))
    V0 = S.train_batches(NG, NK, 5, 2)
    assert np.array_equal(rbm.sample_v_tempered(5, n_gibbs_steps=1, betas=[1.0], V_init=V0).shape, V0.shape)
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        rbm.tempering_stats()
    with pytest.raises(ValueError, match='the tempered sweep has no softmax pass'):
        rbm.set_negative_phase('tempered')
    m = _model(tmp_path, 'm', missing_values=True).fit(XTRAIN[:20])
    with pytest.raises(ValueError, match='softmax visible units'):
        m.set_group_tempering()
    assert one_hot_rows(m.sample_v_tempered(3, n_gibbs_steps=2, n_temperatures=2), NG, NK)      # sampling: complete rows either way
