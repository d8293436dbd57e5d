"""-m gpu: the tempered negative phase - pt_rescore_kernel, the hand-over option of the RT epilogue
(ActArgs::sel_out), bm_rbm_train_step_pt / _train_epoch_pt, BernoulliRBM.set_negative_phase / tempering_stats.

The engine is compared BIT FOR BIT (view(uint32)) with the CPU twin of tests/pt_train_twin.py.  Shapes (V, H, R, M, B, k):
37 x 29 with 24 chains x 5 temperatures, batch 17, k = 2 (120 rows: ragged slots in both directions, I % 4 != 0 on both sides, the
beta = 1 rows scatter inside and across row tiles, the batch is shorter than the ensemble); 16 x 16 with 33 x 3, batch 33, k = 3
(aligned 16-byte stores of the hand-over, an odd number of steps so the swap parity alternates between updates, sparsity
on); 64 x 48 with R = 1 (no swap launch: every row is handed over).  The ensemble is read through bm_rbm_pt_read: the
beta = 1 rows (v and the h it was drawn from), the ladder index of EVERY row and the swap counters - the hot rows' states enter
through the swap decisions (their energies) and their later visits to beta = 1.  The swap decision compares a uniform with a
double exp(): every case first asserts on the twin that no draw lies within 1e-9 of its threshold."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import pt_train_twin as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 515151
CASES = [(37, 29, 5, 24, 17, 2), (16, 16, 3, 33, 33, 3), (64, 48, 1, 16, 16, 1)]          # V, H, R, M, B, k
LR, MOM, UPDATES = 0.05, 0.9, 3
NAMES = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rbm_params(V, H):
    return dict(W=orc.normal(SEED, 1, 0, V * H).reshape(V, H) * np.float32(0.5),
                vb=(orc.uniform(SEED, 2, 0, V) - np.float32(0.5)) * np.float32(0.6),
                hb=(orc.uniform(SEED, 3, 0, H) - np.float32(0.5)) * np.float32(0.6))


def ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(np.float32)


def data(n, V):
    return (orc.uniform(SEED, 6, 0, n * V) < 0.4).astype(np.float32).reshape(n, V)


def config(case):
    return dict(l2=1e-3, sparsity_cost=0.1 if case == 1 else 0.0, sparsity_target=0.2)


def rbm_engine(V, H, p, max_batch, **kw):
    from boltzmann_machines_amd.engine import RbmEngine
    eng = RbmEngine(V, H, max_batch=max_batch, **kw)
    for n in ('W', 'vb', 'hb'):
        eng.set(n, p[n])
    eng.seed(SEED)
    return eng


def engine_state(eng, M):
    from boltzmann_machines_amd._ffi import DeviceArray
    Vd, Hd = DeviceArray((M, eng.V)), DeviceArray((M, eng.H))
    swaps, idx = eng.pt_read(Vd, Hd)
    out = {n: eng.get(n) for n in NAMES}
    out.update(V=Vd.numpy(), H=Hd.numpy(), idx=np.array(idx, np.int32).reshape(-1), swaps=np.array(swaps, np.int64))
    return out


def twin_state(t):
    s = t.state()
    v, h = t.ens.read()
    out = {n: s[n] for n in NAMES}
    out.update(V=v, H=h, idx=s['idx'].astype(np.int32), swaps=s['swaps'])
    return out


def assert_same_state(got, want, what):
    for k in NAMES + ('V', 'H'):
        assert same(got[k], want[k]), '%s: %s differs from the twin in %d entries' % (what, k, int(np.sum(bits(got[k]) != bits(want[k]))))
    assert np.array_equal(got['idx'], want['idx']), '%s: ladder indices differ' % what
    assert np.array_equal(got['swaps'], want['swaps']), '%s: swap counters %s against %s' % (what, got['swaps'].tolist(), want['swaps'].tolist())


@functools.lru_cache(maxsize=None)
def twin_run(case):
    """the states after every one of the UPDATES updates (computed once, shared, never modified) and the smallest tie margin"""
    V, H, R, M, B, k = CASES[case]
    t = P.TemperedRBM(rbm_params(V, H), M, ladder(R), SEED, **config(case))
    X = data(UPDATES * B, V)
    out = []
    for u in range(UPDATES):
        t.train_step(X[u * B:(u + 1) * B], LR, MOM, k)
        out.append(twin_state(t))
    return out, (min(t.ens.margins) if t.ens.margins else np.inf)


def decisive_twin(case):
    want, margin = twin_run(case)
    assert margin >= 1e-9, 'a swap draw of this case lies within 1e-9 of its threshold: choose another seed'
    if CASES[case][2] > 1:
        att, acc = want[-1]['swaps']
        assert np.all(att > 0) and 0 < acc.sum() < att.sum()
    return want


def engine_run(case):
    from boltzmann_machines_amd._ffi import DeviceArray
    V, H, R, M, B, k = CASES[case]
    eng = rbm_engine(V, H, rbm_params(V, H), B, **config(case))
    eng.pt_init(M, ladder(R))
    Xd = DeviceArray.from_numpy(data(UPDATES * B, V))
    out = []
    for u in range(UPDATES):
        eng.train_step_pt(Xd, B, LR, MOM, k, row=u * B)
        out.append(engine_state(eng, M))
    eng.close()
    return out


@pytest.mark.parametrize('case', range(len(CASES)))
def test_updates_match_the_twin(gpu_lib, case):
    """three consecutive updates with momentum and l2 (case 1: the sparsity penalty too): parameters, momentum buffers, q_means
    and the ensemble after every one"""
    want = decisive_twin(case)
    got = engine_run(case)
    for u, (g, w) in enumerate(zip(got, want)):
        assert_same_state(g, w, 'case %d, update %d' % (case, u))
    assert not same(got[0]['W'], got[1]['W'])


def test_rescore_is_the_identity_for_unchanged_parameters(gpu_lib):
    """pt_init + pt_sweep(k), then an update with lr = 0 (W, vb, hb keep their bits): the ensemble is where a second pt_sweep(k)
    leaves it"""
    from boltzmann_machines_amd._ffi import DeviceArray
    V, H, R, M, B, k = CASES[0]
    p = rbm_params(V, H)
    snaps = []
    for update in (True, False):
        eng = rbm_engine(V, H, p, B, l2=1e-3)
        eng.pt_init(M, ladder(R))
        eng.pt_sweep(k)
        if update:
            eng.train_step_pt(DeviceArray.from_numpy(data(B, V)), B, 0.0, MOM, k)
        else:
            eng.pt_sweep(k)
        snaps.append(engine_state(eng, M))
        eng.close()
    for n in ('V', 'H'):
        assert same(snaps[0][n], snaps[1][n]), n
    assert np.array_equal(snaps[0]['idx'], snaps[1]['idx']) and np.array_equal(snaps[0]['swaps'], snaps[1]['swaps'])
    assert 0 < snaps[0]['swaps'][1].sum()
    for n in ('W', 'vb', 'hb'):
        assert same(snaps[0][n], p[n]), n


SUB_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tests import test_pt_train_gpu as G
got = G.engine_run(0)[-1]
np.savez(%(out)r, **got)
print('PT_TRAIN_OK')
'''


def test_hand_over_variants_and_geometries_give_the_same_bits(gpu_lib, tmp_path):
    """case 0 with the hand-over in the epilogue (pt_sel=1, the default), as a gather launch (pt_sel=0) and under two forced
    act_geo values (64 x 32 with two quads per lane, 32 x 32): one subprocess each (the switches are read once per process);
    all equal the twin.  Nothing is started after a failure."""
    want = decisive_twin(0)[-1]
    for dbg in ('pt_sel=1', 'pt_sel=0', 'act_geo=4', 'act_geo=1'):
        out = str(tmp_path / (dbg.replace('=', '') + '.npz'))
        r = subprocess.run([sys.executable, '-c', SUB_SCRIPT % dict(root=ROOT, out=out)],
                           env=dict(os.environ, BM355_DEBUG=dbg), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and 'PT_TRAIN_OK' in r.stdout, dbg + ': ' + r.stdout[-2000:] + r.stderr[-4000:]
        assert_same_state(dict(np.load(out)), want, dbg)


def test_native_loop_equals_single_steps(gpu_lib):
    """train_epoch_pt over N = 2 batch + 5 rows (a short last batch) against three train_step_pt calls, and against the twin"""
    from boltzmann_machines_amd._ffi import DeviceArray
    V, H, R, M, B, k = CASES[0]
    N = 2 * B + 5
    X = data(N, V)
    states = []
    for native in (True, False):
        eng = rbm_engine(V, H, rbm_params(V, H), B, **config(0))
        eng.pt_init(M, ladder(R))
        Xd = DeviceArray.from_numpy(X)
        if native:
            eng.train_epoch_pt(Xd, N, B, LR, MOM, k)
        else:
            for s in range(0, N, B):
                eng.train_step_pt(Xd, min(B, N - s), LR, MOM, k, row=s)
        states.append(engine_state(eng, M))
        eng.close()
    t = P.TemperedRBM(rbm_params(V, H), M, ladder(R), SEED, **config(0))
    t.train_epoch(X, B, LR, MOM, k)
    assert min(t.ens.margins) >= 1e-9
    assert_same_state(states[0], states[1], 'native loop against single steps')
    assert_same_state(states[0], twin_state(t), 'native loop against the twin')


def test_existing_paths_are_untouched(gpu_lib):
    """a handle that made a tempered update (and then got its parameters and seed back) gives the bits of a fresh handle in
    bm_rbm_gibbs, bm_rbm_train_step and pt_init + pt_sweep + pt_read: the update leaves nothing behind in a workspace or flag
    those paths read"""
    from boltzmann_machines_amd._ffi import DeviceArray
    V, H, R, M, B, k = CASES[0]
    p = rbm_params(V, H)
    X = data(B, V)
    H0 = (orc.uniform(SEED, 7, 0, B * H) < 0.5).astype(np.float32).reshape(B, H)
    results = []
    for tempered in (False, True):
        eng = rbm_engine(V, H, p, B, sample_v_states=True, l2=1e-3)
        if tempered:
            eng.pt_init(M, ladder(R))
            eng.train_step_pt(DeviceArray.from_numpy(X), B, LR, MOM, k)
            for n in NAMES:
                eng.set(n, p[n] if n in p else 0.0)
            eng.seed(SEED)
        Hd, Vd = DeviceArray.from_numpy(H0), DeviceArray((B, V))
        eng.gibbs(Hd, Vd, B, 3)
        eng.train_step(DeviceArray.from_numpy(X), B, LR, MOM, 1)
        eng.pt_init(M, ladder(R))
        eng.pt_sweep(2)
        s = engine_state(eng, M)
        results.append([Hd.numpy(), Vd.numpy(), s['V'], s['H'], s['idx'].astype(np.float32), s['swaps'].astype(np.float32)] + [s[n] for n in NAMES])
        eng.close()
    for i, (a, b) in enumerate(zip(*results)):
        assert same(a, b), i


def test_entry_point_errors(gpu_lib):
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray
    V, H = 20, 12
    p = rbm_params(V, H)
    Xd = DeviceArray.from_numpy(data(8, V))
    eng = rbm_engine(V, H, p, 6)
    for call in (lambda: eng.train_step_pt(Xd, 4, LR, MOM, 1), lambda: eng.train_epoch_pt(Xd, 8, 4, LR, MOM, 1)):
        with pytest.raises(Bm355Error, match='pt_init first'):
            call()
    eng.pt_init(5, [0.5, 1.0])
    for B in (0, 6, 7):                                          # min(max_batch = 6, n_chains = 5) = 5
        with pytest.raises(Bm355Error, match='batch'):
            eng.train_step_pt(Xd, B, LR, MOM, 1)
    with pytest.raises(Bm355Error, match='batch'):
        eng.train_epoch_pt(Xd, 8, 6, LR, MOM, 1)
    eng.pt_init(8, [0.5, 1.0])                                   # min(6, 8) = 6
    with pytest.raises(Bm355Error, match='batch'):
        eng.train_step_pt(Xd, 7, LR, MOM, 1)
    for call in (lambda: eng.train_step_pt(Xd, 4, LR, MOM, 0), lambda: eng.train_epoch_pt(Xd, 8, 4, LR, MOM, 0)):
        with pytest.raises(Bm355Error, match='n_gibbs_steps'):
            call()
    for N, batch in ((0, 4), (8, 0)):
        with pytest.raises(Bm355Error, match='bad N'):
            eng.train_epoch_pt(Xd, N, batch, LR, MOM, 1)
    eng.train_step_pt(Xd, 6, LR, MOM, 1)
    eng.train_epoch_pt(Xd, 8, 6, LR, MOM, 1)
    eng.close()
    eng = rbm_engine(V, H, p, 6, dropout=0.8)
    eng.pt_init(6, [0.5, 1.0])
    for call in (lambda: eng.train_step_pt(Xd, 4, LR, MOM, 1), lambda: eng.train_epoch_pt(Xd, 8, 4, LR, MOM, 1)):
        with pytest.raises(Bm355Error, match='dropout'):
            call()
    eng.close()
    from boltzmann_machines_amd.engine import RbmEngine64
    assert not hasattr(RbmEngine64, 'train_step_pt')


# ------------------------------------------------------------------------------------------------ public API
NV, NH, BS, NROWS = 16, 12, 10, 200
XTRAIN = (orc.uniform(SEED, 60, 0, NROWS * NV) < 0.4).astype(np.float32).reshape(NROWS, NV)


def _model(tmp_path, name, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    p = rbm_params(NV, NH)
    base = dict(n_visible=NV, n_hidden=NH, batch_size=BS, max_epoch=2, random_seed=1337, verbose=False, n_gibbs_steps=2,
                W_init=p['W'], vb_init=p['vb'], hb_init=p['hb'], model_path=str(tmp_path / name) + '/')
    return BernoulliRBM(**dict(base, **kw))


def test_public_fit_matches_the_twin(gpu_lib, tmp_path):
    """fit() in tempered mode on 200 rows, two epochs of 20 updates, a metrics iteration every 10th (it consumes one call of
    the stream and changes nothing else), against the twin driven by the same host seed; tempering_stats; then
    set_negative_phase('cd') and one more epoch: the oracle's plain CD updates from where the tempered fit ended"""
    rbm = _model(tmp_path, 'a').set_negative_phase('tempered', n_temperatures=4, n_chains=BS + 3)
    seeds = _model(tmp_path, 'seeds')
    seed1, seed2 = seeds.make_random_seed(), seeds.make_random_seed()
    rbm.fit(XTRAIN)
    t = P.TemperedRBM(rbm_params(NV, NH), BS + 3, ladder(4), seed1, l2=1e-4)
    it = 0
    for epoch in range(2):
        for s in range(0, NROWS, BS):
            it += 1
            if it % 10 == 0:
                t.call += 1                                  # bm_rbm_metrics
            t.train_step(XTRAIN[s:s + BS], 0.01, 0.9, 2)
    assert min(t.ens.margins) >= 1e-9, 'a swap draw lies within 1e-9 of its threshold: choose another seed'
    assert rbm.iter_ == it == 40
    got = engine_state(rbm._engine, BS + 3)
    assert_same_state(got, twin_state(t), 'fit')
    rates = rbm.tempering_stats()
    assert rates.shape == (3,) and np.all((rates >= 0) & (rates <= 1))
    assert np.array_equal(rates, t.ens.cnt[1] / t.ens.cnt[0].astype(np.float64)) and np.all(t.ens.cnt[0] == 2 * 40 * (BS + 3) // 2)
    # the setting is not in the checkpoint: a loaded model trains with CD
    from boltzmann_machines_amd import BernoulliRBM
    assert BernoulliRBM.load_model(str(tmp_path / 'a') + '/')._neg_phase is None
    # back to CD: the oracle's plain updates
    o = orc.OracleRBM(NV, NH, sample_v_states=False, sample_h_states=True, l2=1e-4)
    for n in NAMES:
        o.p[n][...] = got[n]
    o.set_seed(seed2)
    rbm.set_negative_phase('cd')
    rbm.max_epoch = 3
    rbm.fit(XTRAIN)
    for s in range(0, NROWS, BS):
        o.train_step(XTRAIN[s:s + BS], 0.01, 0.9, 2)
    for n in NAMES:
        assert same(rbm._engine.get(n), o.p[n]), 'cd after tempered: ' + n


def test_public_refusals(gpu_lib, tmp_path, monkeypatch):
    """every NotImplementedError, at set_negative_phase and - for what can change afterwards - at fit"""
    from boltzmann_machines_amd import BernoulliRBM, GaussianRBM, MultinomialRBM
    monkeypatch.delenv('BM355_DATA_PARALLEL', raising=False)
    kw = dict(n_visible=NV, n_hidden=NH, batch_size=BS, max_epoch=1, random_seed=1337, verbose=False)
    X = XTRAIN[:20]
    g = GaussianRBM(learning_rate=1e-3, model_path=str(tmp_path / 'g') + '/', **kw).fit(X)
    m = MultinomialRBM(n_samples=3, model_path=str(tmp_path / 'm') + '/', **kw).fit(X)
    r64 = BernoulliRBM(dtype='float64', model_path=str(tmp_path / 'f') + '/', **kw).fit(X)
    first = BernoulliRBM(dbm_first=True, model_path=str(tmp_path / 'df') + '/', **kw).fit(X)
    last = BernoulliRBM(dbm_last=True, model_path=str(tmp_path / 'dl') + '/', **kw).fit(X)
    drop = BernoulliRBM(dropout=0.9, model_path=str(tmp_path / 'dr') + '/', **kw).fit(X)
    for model, word in ((g, 'Gaussian'), (m, 'Multinomial'), (r64, 'float64'), (first, 'dbm_first'), (last, 'dbm_first'), (drop, 'dropout')):
        with pytest.raises(NotImplementedError, match=word):
            model.set_negative_phase('tempered')
    r = BernoulliRBM(model_path=str(tmp_path / 'r') + '/', **kw).set_negative_phase('tempered', n_temperatures=3)
    with pytest.raises(RuntimeError, match='no tempered ensemble'):
        r.tempering_stats()
    r.set_params(dropout=0.9)                       # after the switch: refused at fit, before anything is trained
    with pytest.raises(NotImplementedError, match='dropout'):
        r.fit(X)
    r.set_params(dropout=None)
    monkeypatch.setenv('BM355_DATA_PARALLEL', '1')
    with pytest.raises(NotImplementedError, match='BM355_DATA_PARALLEL'):
        r.set_negative_phase('tempered')
    monkeypatch.delenv('BM355_DATA_PARALLEL')
    r.set_params(batch_size=BS + 1)                 # n_chains (= the old batch_size) < batch_size
    with pytest.raises(ValueError, match='n_chains'):
        r.fit(X)
