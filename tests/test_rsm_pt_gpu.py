"""-m gpu: parallel tempering and the tempered negative phase over replicated softmax visible units - the DB + RT
flavour of act_kernel, the PT flavour of multinomial_counts_kernel, rsm_pt_start_kernel, rsm_pt_rescore_kernel, the two-length
flavour of rsm_bias_kernel, bm_rbm_rsm_pt_init / _sweep / _read, bm_rbm_rsm_train_step_pt / _train_epoch_pt,
ReplicatedSoftmaxRBM.sample_v_tempered / set_count_tempering.

The engine is compared BIT FOR BIT with the CPU twin of tests/rsm_pt_twin.py: the states of both layers, both partial arrays (the
hi / lo pair of v.vb included), the rows' temperatures, lengths and ladder indices and the swap counters of the WHOLE ensemble.
The cases are the twin module's SWEEP_CASES / TRAIN_CASES: tests/test_rsm_pt.py shows that none of their swap draws lies within
1e-9 of its threshold (0 near ties), so nothing is excluded.  BM355_DEBUG switches are read once per process: every run under one
is a fresh child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rsm_pt_twin as S
from tests import rsm_twin as rt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENS = ('v', 'h', 'part_v', 'part_h', 'mult', 'len', 'idx', 'swaps')
NAMES = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')
LR, MOM, L2 = 0.05, 0.5, 1e-3
ML = S.MAX_LENGTH


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def make_engine(p, max_batch=4, seed=None, max_length=ML, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    V, H = p['W'].shape
    eng = RbmEngine(V, H, max_batch=max_batch, rsm_max_length=max_length, **kw)     # (max_batch does not bound the ensemble)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, p[n])
    if seed is not None:
        eng.seed(seed)
    return eng


def assert_same_ensemble(got, want, what):
    for n in ENS:
        if want[n] is None:                         # (the h.(vW + D hb) partials before the first prop-up: not written yet)
            continue
        if n in ('idx', 'swaps'):
            assert np.array_equal(got[n], want[n]), '%s: %s %s against %s' % (what, n, got[n].tolist(), want[n].tolist())
        else:
            assert got[n].shape == want[n].shape, (what, n, got[n].shape, want[n].shape)
            d = bits(got[n]) != bits(want[n])
            assert not d.any(), '%s: %s differs from the twin in %d entries' % (what, n, int(d.sum()))


@functools.lru_cache(maxsize=None)
def twin_snaps(c, chain0=S.SWEEP_CHAIN0, M=None):
    """the twin's three snapshots of a case (computed once, shared, never modified)"""
    V, H, M_, R = c
    M = M_ if M is None else M
    return S.sweep_twin((V, H, M, R), chain0=chain0, lengths=lengths_of(M, chain0))[1]


def lengths_of(M, chain0):
    """the lengths of the chains [chain0, chain0 + M) of one long list: a slice of chains keeps its chains' lengths"""
    return S.sweep_lengths(M, chain0)


def engine_snaps(c, chain0=S.SWEEP_CHAIN0, M=None, eng=None):
    """bm_rbm_rsm_pt_init at call 0 of SWEEP_SEED, then two sweeps of 2 steps; the whole ensemble after each"""
    V, H, M_, R = c
    M = M_ if M is None else M
    own = eng is None
    if own:
        eng = make_engine(S.make_params(V, H))
    eng.seed(S.SWEEP_SEED)
    pt = eng.rsm_pt
    pt.pt_init(M, S.ladder(R), chain0=chain0, lengths=lengths_of(M, chain0))
    out = [pt.pt_state()]
    for n in (2, 2):
        pt.pt_sweep(n)
        out.append(pt.pt_state())
    if own:
        eng.close()
    return out


def check_sweep_case(c):
    V, H, M, R = c
    got, want = engine_snaps(c), twin_snaps(c)
    for n, (g, w) in enumerate(zip(got, want)):
        assert_same_ensemble(g, w, '%s, snapshot %d' % (S.case_id(c), n))
        assert np.array_equal(g['v'].sum(axis=1), g['len']) and np.all(g['v'] >= 0) and np.all(g['v'] == np.trunc(g['v']))
        assert np.array_equal(np.sort(g['idx'].reshape(M, R), axis=1), np.tile(np.arange(R), (M, 1)))
        assert np.array_equal(g['mult'], S.ladder(R)[g['idx']])
    if R > 1:
        assert np.all(got[-1]['swaps'][0] > 0)


# ------------------------------------------------------------------------------------------------ sweeps
def test_the_cases_cover_the_table():
    assert {c[0] for c in S.SWEEP_CASES} == {2, 16, 17, 256, 257, 4096, 4097}
    assert {c[1] for c in S.SWEEP_CASES} == {16, 17, 40} and {c[2:] for c in S.SWEEP_CASES} == {(1, 1), (3, 4), (33, 2)}
    # the marginals, not the cross product; the RPT = 4 count kernel (V > 4096) meets every H and every (M, R)
    assert {c[1] for c in S.SWEEP_CASES if c[0] > 4096} == {16, 17, 40} and {c[2:] for c in S.SWEEP_CASES if c[0] > 4096} == {(1, 1), (3, 4), (33, 2)}
    D = lengths_of(33, S.SWEEP_CHAIN0)
    assert D.min() == 1 and D.max() == ML and len(np.unique(D)) > 5


@pytest.mark.parametrize('case', S.SWEEP_CASES, ids=S.case_id)
def test_engine_matches_twin(gpu_lib, case):
    """uniform start (the twin's), then two consecutive sweeps of 2 steps: call counter, parity continuation, a chain0 != 0, lengths
    mixed within every launch"""
    check_sweep_case(case)


def test_one_temperature_is_the_plain_chain_and_the_plain_prop_down(gpu_lib):
    """R = 1, betas = (1,) from a V0: the twin's plain chain (DB and the plain count sampler); the PT count kernel with every
    row_mult == 1 against bm_rbm_sample_v_from_h on the same H, lengths, seed, call and rows"""
    from boltzmann_machines_amd._ffi import DeviceArray
    for V, H, M in ((17, 16, 7), (257, 40, 7), (4097, 17, 3)):
        p = S.make_params(V, H)
        D = S.chain_lengths(M, ML, seed=3)
        V0 = S.uniform_start(5, 0, 0, D, V, ML)
        eng = make_engine(p, max_batch=8, seed=77)
        pt = eng.rsm_pt
        pt.pt_init(M, [1.0], DeviceArray.from_numpy(V0), lengths=D)
        st = pt.pt_state()
        assert np.array_equal(st['v'], V0) and np.array_equal(bits(st['part_v']), bits(S.vb_pair(V0, p['vb']).T))
        pt.pt_sweep(1)
        one = pt.pt_state()
        eng.seed(77)                                  # (call 0 again: the stream of the sweep)
        Hd, Dd, Sd = DeviceArray.from_numpy(one['h']), DeviceArray.from_numpy(D), DeviceArray((M, V), f32)
        eng.set_row_lengths(Dd, M)
        eng.sample_v_from_h(Hd, M, None, Sd)
        assert np.array_equal(Sd.numpy(), one['v']), (V, H)
        eng.seed(77)
        pt.pt_init(M, [1.0], DeviceArray.from_numpy(V0), lengths=D)
        pt.pt_sweep(3)
        got = pt.pt_state()
        eng.close()
        v, h = S.plain_chain(p, V0, D, 3, 77, ML)
        assert np.array_equal(got['v'], v) and np.array_equal(got['h'], h), (V, H)
        assert got['swaps'].size == 0


@pytest.mark.parametrize('V,H,J', [(17, 16, 7), (257, 40, 37), (4097, 17, 5)], ids=['17x16', '257x40', '4097x17'])
def test_row_tempered_prop_up_is_the_db_pass_at_a_uniform_beta(gpu_lib, V, H, J):
    """device against device, through the launch-level probe bm_debug_rsm_up: the DB + RT prop-up with every row_mult equal to one
    beta gives the bits of the existing DB pass at mult == bmult == beta (the pass of bm_rbm_rsm_ais) on the same rows, lengths, seed,
    call and site - at beta = 1 and at two betas below it; both equal the twin, the energy partials carry the untempered t, and at
    beta = 1 the states are those of the first prop-up of bm_rbm_rsm_pt_sweep and of the plain DB twin"""
    from boltzmann_machines_amd._ffi import DeviceArray
    p = S.make_params(V, H)
    D = S.sweep_lengths(J, 11)
    V0 = S.uniform_start(8, 0, 0, D, V, ML)
    eng = make_engine(p, seed=55)
    Vd, Dd = DeviceArray.from_numpy(V0), DeviceArray.from_numpy(D)
    ns = (H + 15) // 16
    one = None
    for beta in (1.0, 0.37, 0.05):
        Ha, Hb, Pd = DeviceArray((J, H), f32), DeviceArray((J, H), f32), DeviceArray((ns, J), f32)
        eng.debug_rsm_up(Vd, J, Dd, beta, True, Ha, Pd)
        eng.debug_rsm_up(Vd, J, Dd, beta, False, Hb)
        eng.sync()
        ha, hb, part = Ha.numpy(), Hb.numpy(), Pd.numpy()
        assert np.array_equal(bits(ha), bits(hb)), (beta, int(np.sum(ha != hb)))
        _, s, t = S.db_rt_up(V0, p['W'], p['hb'], D, np.full(J, beta, f32), 1, 55, S.SITE_H, 0, 0)
        assert np.array_equal(bits(ha), bits(s)), beta
        assert np.array_equal(bits(part), bits(S.T.slot_partials(s * t).T)), beta
        assert 0 < ha.sum() < ha.size
        if beta == 1.0:
            one = ha
            assert np.array_equal(bits(ha), bits(rt.db_up(V0, p['W'], p['hb'], D, 1, 55, S.SITE_H, 0)[1]))
    pt = eng.rsm_pt                                  # (the probe left the call counter where it was: call 0 of seed 55)
    pt.pt_init(J, [1.0], Vd, lengths=D)
    pt.pt_sweep(1)
    assert np.array_equal(bits(pt.pt_state()['h']), bits(one))
    eng.close()


def test_a_pending_length_flag_is_not_the_starts(gpu_lib):
    """the flag a bad training batch left in the handle and bm_rbm_sync has not reported yet neither fails a valid start nor is lost"""
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray
    from boltzmann_machines_amd.engine import as_device
    V, H = 17, 16
    D = S.sweep_lengths(3, 11)
    V0 = S.uniform_start(9, 0, 0, D, V, ML)
    eng = make_engine(S.make_params(V, H), seed=3)
    X = S.train_batches(V, 4, 1)
    X[1, 0] += ML                                      # a row longer than max_length
    eng.train_step(as_device(X), 4, 0.0, 0.0, 1)
    eng.rsm_pt.pt_init(3, S.ladder(2), DeviceArray.from_numpy(V0), lengths=D)
    with pytest.raises(Bm355Error, match='longer than max_length'):
        eng.sync()
    eng.sync()                                         # reported once
    eng.rsm_pt.pt_sweep(1)
    assert np.array_equal(eng.rsm_pt.pt_state()['v'].sum(axis=1), np.repeat(D, 2))
    eng.close()


def test_chain_slices_determinism_and_both_starts(gpu_lib):
    """chains [3, 6) of an ensemble of 7 at chain0 = 4 (split at an odd chain) are the ensemble of 3 at chain0 = 7; a second run gives
    the same bits; a start from V0 replicates the chain's row; a V0 whose sums disagree with the lengths is refused"""
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray
    case = (257, 17, 7, 4)
    V, H, _, R = case
    whole = engine_snaps(case, chain0=4, M=7)
    again = engine_snaps(case, chain0=4, M=7)
    part = engine_snaps(case, chain0=7, M=3)
    for n, (a, b, c, w) in enumerate(zip(whole, again, part, twin_snaps(case, chain0=4, M=7))):
        assert_same_ensemble(a, w, 'whole, snapshot %d' % n)
        for k in ('v', 'h', 'mult', 'idx', 'len', 'part_v'):
            if n == 0 and k == 'h':
                continue
            assert np.array_equal(bits(a[k]), bits(b[k])), (n, k)
            sl = a[k][..., 3 * R:6 * R] if k == 'part_v' else a[k][3 * R:6 * R]
            assert np.array_equal(bits(sl), bits(c[k])), (n, k)
    D = lengths_of(5, 0)
    V0 = S.uniform_start(9, 0, 0, D, V, ML)
    eng = make_engine(S.make_params(V, H), seed=3)
    pt = eng.rsm_pt
    pt.pt_init(5, S.ladder(R), DeviceArray.from_numpy(V0), lengths=D)
    st = pt.pt_state()
    assert np.array_equal(st['v'], np.repeat(V0, R, axis=0)) and np.array_equal(st['len'], np.repeat(D, R))
    e = S.Ensemble(S.make_params(V, H), D, S.ladder(R), 3, ML, V0=V0)
    assert np.array_equal(bits(st['part_v']), bits(e.part_v.T))
    bad = V0.copy()
    bad[2, 0] += 1.0
    with pytest.raises(Bm355Error, match='sum is not its chain'):
        pt.pt_init(5, S.ladder(R), DeviceArray.from_numpy(bad), lengths=D)
    with pytest.raises(Bm355Error, match='no ensemble'):
        pt.pt_sweep(1)
    pt.pt_init(5, S.ladder(R), DeviceArray.from_numpy(V0), lengths=D)      # the handle is usable
    pt.pt_sweep(1)
    e.sweep(1)
    assert_same_ensemble(pt.pt_state(), S.snapshot(e), 'behind a refused start')
    eng.close()


# ------------------------------------------------------------------------------------------------ updates
@functools.lru_cache(maxsize=None)
def twin_updates(c, lr=LR, steps=(4, 4, 4)):
    V, H, M, R = c
    t = S.TemperedRsmRBM(S.make_params(V, H), S.chain_lengths(M, ML, seed=2), S.ladder(R), S.TRAIN_SEED, ML, l2=L2)
    X = S.train_batches(V, sum(steps), 1)
    out, s = [], 0
    for B in steps:
        t.train_step(X[s:s + B], lr, MOM, 2)
        out.append(t.state())
        s += B
    assert t.ens.near_ties() == 0
    return out


def engine_state(eng):
    out = {n: eng.get(n) for n in NAMES}
    out.update(eng.rsm_pt.pt_state())
    return out


def assert_same_state(got, want, what):
    for n in NAMES:
        assert np.array_equal(bits(got[n]), bits(want[n])), '%s: %s differs from the twin in %d entries' % (what, n, int(np.sum(bits(got[n]) != bits(want[n]))))
    assert_same_ensemble(got, want, what)


def engine_updates(c, lr=LR, steps=(4, 4, 4), epoch=None):
    from boltzmann_machines_amd.engine import as_device
    V, H, M, R = c
    eng = make_engine(S.make_params(V, H), max_batch=5, seed=S.TRAIN_SEED, l2=L2)
    pt = eng.rsm_pt
    pt.pt_init(M, S.ladder(R), lengths=S.chain_lengths(M, ML, seed=2))
    Xd = as_device(S.train_batches(V, sum(steps), 1))
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
    """three rsm_train_step_pt updates: every parameter, every momentum buffer and the whole ensemble, bit for bit"""
    check_train_case(case)


def test_zero_learning_rate_update_is_a_sweep(gpu_lib):
    """lr = 0: the parameters keep their bits, and two updates of k = 2 leave the ensemble two sweeps of 2 steps leave - the rescore
    in front of each rewrote the bits that were there"""
    case = S.TRAIN_CASES[0]
    V, H, M, R = case
    got = engine_updates(case, lr=0.0, steps=(4, 4))
    p = S.make_params(V, H)
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(got[-1][n]), bits(p[n])), n
    eng = make_engine(p, max_batch=5, seed=S.TRAIN_SEED, l2=L2)
    eng.rsm_pt.pt_init(M, S.ladder(R), lengths=S.chain_lengths(M, ML, seed=2))
    for n in range(2):
        eng.rsm_pt.pt_sweep(2)
        assert_same_ensemble(eng.rsm_pt.pt_state(), got[n], 'sweep %d against the lr = 0 update' % n)
    eng.close()
    assert_same_state(got[-1], twin_updates(case, lr=0.0, steps=(4, 4))[-1], 'lr = 0 against the twin')


def test_native_loop_equals_single_steps(gpu_lib):
    """rsm_train_epoch_pt over 10 rows in batches of 4: the steps of 4, 4 and 2 rows (a short last batch)"""
    case = S.TRAIN_CASES[0]
    steps = engine_updates(case, steps=(4, 4, 2))[-1]
    loop = engine_updates(case, steps=(4, 4, 2), epoch=4)[-1]
    assert_same_state(loop, steps, 'epoch against steps')
    assert_same_state(loop, twin_updates(case, steps=(4, 4, 2))[-1], 'epoch against the twin')


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_rsm_pt_gpu as G
for c in %(sweeps)r:
    G.check_sweep_case(c)
for c in %(trains)r:
    G.check_train_case(c)
print('RSM_PT_OK')
'''
# every geometry code DB has (launch_act_as): both stagings of the four tiles, the 64 x 64 tiles, the BK = 32 tiles, half-wave DMA
GEOS = ('8', '4', '1', '3', '108', '104', '101', '103', '6', '9', '7', '208')
SWITCHES = [('act_geo=' + g, [(17, 40, 1, 1), (257, 17, 33, 2)], []) for g in GEOS] + [('pt_sel=0', [], list(S.TRAIN_CASES))]


@pytest.mark.parametrize('dbg,sweeps,trains', SWITCHES, ids=[s[0] for s in SWITCHES])
def test_geometries_and_hand_over_give_the_same_bits(gpu_lib, dbg, sweeps, trains):
    """a fresh child process per switch: every geometry DB has (act_geo), the gather launch in place of the hand-over in the count
    kernel (pt_sel=0) - each against the twin, so against the default run, bit for bit"""
    env = dict(os.environ, BM355_DEBUG=dbg)
    r = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, sweeps=sweeps, trains=trains)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and 'RSM_PT_OK' in r.stdout, '%s: %s' % (dbg, r.stdout[-2000:] + r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ what a tempered call leaves untouched
def test_a_tempered_call_leaves_the_handle_as_it_was(gpu_lib):
    """bm_rbm_gibbs, a CD update and bm_rbm_rsm_ais give the same bits before and behind an init, a sweep, a read and a tempered
    update at lr = 0 (each tempered call consumes one call of the stream, nothing else)"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import as_device
    V, H, B = 257, 17, 6
    p = S.make_params(V, H)
    X = S.train_batches(V, B, 4)
    D = rt.lengths(X)

    def probe(eng):
        eng.seed(41)
        a = eng.rsm_ais(6, D[:4], 2, 5, chain0=3)
        Vd, Hd, Dd = as_device(X), DeviceArray((B, H), f32), as_device(D)
        eng.set_row_lengths(Dd, B)
        eng.sample_h(Vd, B, None, Hd)
        eng.gibbs(Hd, Vd, B, 2)
        eng.train_step(as_device(X), B, LR, MOM, 1)
        eng.sync()
        return [a, Vd.numpy(), Hd.numpy()] + [eng.get(n) for n in NAMES]

    ref = make_engine(p, max_batch=B, l2=L2)
    want = probe(ref)
    ref.close()
    eng = make_engine(p, max_batch=B, l2=L2, seed=9)
    pt = eng.rsm_pt
    pt.pt_init(B, S.ladder(3), lengths=D)
    pt.pt_sweep(2)
    Vd = DeviceArray((B, V), f32)
    swaps, idx = pt.pt_read(Vd)
    assert np.array_equal(Vd.numpy().sum(axis=1), D) and swaps.shape == (2, 2) and idx.shape == (B, 3)
    pt.train_step_pt(as_device(X), B, 0.0, 0.0, 1)
    for n in ('W', 'vb', 'hb'):
        assert np.array_equal(bits(eng.get(n)), bits(p[n])), n
    for n in ('dW', 'dvb', 'dhb'):                     # (lr = 0 left zero momentum buffers, as the reference handle starts with)
        assert not eng.get(n).any(), n
    got = probe(eng)
    eng.close()
    for g, w in zip(got[:-1], want[:-1]):              # (q_means moved under the lr = 0 update: not compared)
        assert np.array_equal(bits(g), bits(w))


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_point_refusals(gpu_lib):
    """every refusal of the five entries, the handle still training afterwards; the rules of the handle's one ensemble"""
    from boltzmann_machines_amd._ffi import Bm355Error
    from boltzmann_machines_amd.engine import RbmEngine, as_device
    V, H = 17, 16
    p = S.make_params(V, H)
    Xd = as_device(S.train_batches(V, 8, 1))
    D5 = S.chain_lengths(5, ML)
    plain = RbmEngine(V, H, max_batch=6)
    calls = lambda pt: (lambda: pt.pt_init(5, [0.5, 1.0], lengths=D5), lambda: pt.pt_sweep(1), lambda: pt.pt_read(),
                        lambda: pt.train_step_pt(Xd, 4, LR, MOM, 1), lambda: pt.train_epoch_pt(Xd, 8, 4, LR, MOM, 1))
    plain.rsm_pt._pt_shape = (5, 2)
    for call in calls(plain.rsm_pt):
        with pytest.raises(Bm355Error, match='needs a handle with replicated softmax visible units'):
            call()
    # a handle that holds a Bernoulli ensemble does not take the unit
    plain.pt_init(5, [0.5, 1.0])
    with pytest.raises(Bm355Error, match='tempered ensemble'):
        plain.set_replicated_softmax(ML)
    plain.close()
    eng = make_engine(p, max_batch=6, seed=1)
    pt = eng.rsm_pt
    pt._pt_shape = (5, 2)
    for call in calls(pt)[1:]:
        with pytest.raises(Bm355Error, match='no ensemble'):
            call()
    for M, betas in ((0, [0.5, 1.0]), (5, [0.5, 0.9]), (5, [0.6, 0.5, 1.0]), (5, [0.0, 1.0]), (5, [])):
        with pytest.raises(Bm355Error, match='beta|n_temps|ensemble'):
            pt.pt_init(M, betas, lengths=D5[:M])
    with pytest.raises(Bm355Error, match='chain0'):
        pt.pt_init(5, [0.5, 1.0], chain0=-1, lengths=D5)
    for badlen in (0, ML + 1, 2.5):
        L = D5.copy()
        L[3] = badlen
        with pytest.raises(Bm355Error, match='no integer in'):
            pt.pt_init(5, [0.5, 1.0], lengths=L)
    pt.pt_init(5, [0.5, 1.0], lengths=D5)
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
        with pytest.raises(Bm355Error, match='replicated softmax'):
            call()
    # the handle still trains, tempered and plain
    pt.train_step_pt(Xd, 5, LR, MOM, 1)
    pt.train_epoch_pt(Xd, 8, 5, LR, MOM, 1)
    eng.train_step(Xd, 6, LR, MOM, 1)
    eng.sync()
    assert all(np.all(np.isfinite(eng.get(n))) for n in NAMES)
    # the unit off: the ensemble goes with it
    eng.set_replicated_softmax(0)
    with pytest.raises(Bm355Error, match='no ensemble'):
        eng.pt_sweep(1)
    eng.set_replicated_softmax(ML)
    with pytest.raises(Bm355Error, match='no ensemble'):
        pt.pt_sweep(1)
    eng.close()


# ------------------------------------------------------------------------------------------------ public API
NV, NH, BS, NROWS = 24, 12, 10, 60
XTRAIN = S.train_batches(NV, NROWS, 7)


def _model(tmp_path, name, **kw):
    from boltzmann_machines_amd import ReplicatedSoftmaxRBM
    p = S.make_params(NV, NH, std=0.1)
    base = dict(n_visible=NV, n_hidden=NH, max_length=ML, batch_size=BS, max_epoch=2, random_seed=1337, verbose=False, n_gibbs_steps=2,
                learning_rate=0.01, momentum=0.9, l2=1e-4, W_init=p['W'], vb_init=p['vb'], hb_init=p['hb'], model_path=str(tmp_path / name) + '/')
    return ReplicatedSoftmaxRBM(**dict(base, **kw))


def test_public_fit_matches_the_twin(gpu_lib, tmp_path):
    """fit() under set_count_tempering on 60 rows, two epochs of 6 updates, a metrics iteration every 10th (it consumes one call of
    the stream and changes nothing else), against the twin driven by the same host seed; the chains' lengths are those of the first
    n_chains rows of X; tempering_stats equals the counters; sample_v_tempered rows sum to their lengths"""
    rbm = _model(tmp_path, 'a').set_count_tempering(n_temperatures=4, n_chains=BS + 3)
    seed1 = _model(tmp_path, 'seeds').make_random_seed()
    rbm.fit(XTRAIN)
    Dc = rt.lengths(XTRAIN)[:BS + 3]
    t = S.TemperedRsmRBM(S.make_params(NV, NH, std=0.1), Dc, S.ladder(4), seed1, ML, l2=1e-4)
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
    from boltzmann_machines_amd import ReplicatedSoftmaxRBM
    assert ReplicatedSoftmaxRBM.load_model(str(tmp_path / 'a') + '/')._neg_phase is None
    # the sampler: count rows of the given lengths, rates in [0, 1]; it replaces the training ensemble
    Dq = np.array([1, 5, ML, 7, 7, 3, 12])
    Vs, acc = rbm.sample_v_tempered(7, Dq, n_gibbs_steps=5, n_temperatures=3, return_stats=True)
    assert Vs.shape == (7, NV) and np.array_equal(Vs.sum(axis=1), Dq) and np.all(Vs >= 0) and np.all(Vs == np.trunc(Vs))
    assert acc.shape == (2,) and np.all((acc >= 0) & (acc <= 1))
    V0 = XTRAIN[:5]
    out = rbm.sample_v_tempered(5, rt.lengths(V0).astype(np.int64), n_gibbs_steps=1, betas=[1.0], V_init=V0)
    assert np.array_equal(out.sum(axis=1), rt.lengths(V0))
    assert np.array_equal(rbm.sample_v_tempered(4, 9, n_gibbs_steps=2, n_temperatures=2).sum(axis=1), np.full(4, 9))
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        rbm.tempering_stats()
    with pytest.raises(ValueError, match='the tempered sweep has no count sampler'):
        rbm.set_negative_phase('tempered')
