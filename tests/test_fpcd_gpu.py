"""-m gpu: fast-weights PCD - the fast-weights flavour of grad_kernel, the fast bias update, the refresh of the
effective copies, bm_rbm_set_fast_weights, BernoulliRBM.set_negative_phase(fast_learning_rate=...) / fast_weights().

The engine is compared BIT FOR BIT (view(uint32)) with the CPU twin of tests/fpcd_twin.py over three updates.  Shapes
(V, H, R, M, B, k): 37 x 29 with 24 x 5, batch 17, k = 2 (the ragged scalar epilogue, no W^T since V % 4 != 0, a batch shorter than
the ensemble); 16 x 16 with 33 x 3, batch 33, k = 3, sparsity on (the vec8 stores, the bias kernel first and a penalty in the
tiles, We^T kept, a swap parity that alternates between updates; rate 1e-3 and again the common rate); 64 x 48 with R = 1 (FPCD
proper: no swap launch, one full tile column); 132 x 72 with 12 x 2 (3 x 2 tiles, ragged last tiles both ways, W^T kept).  As in
test_pt_train_gpu.py every case first asserts on the twin that no swap draw lies within 1e-9 of its threshold."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fpcd_twin as F
from tests import pt_train_twin as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 626262
CASES = [(37, 29, 5, 24, 17, 2), (16, 16, 3, 33, 33, 3), (64, 48, 1, 16, 16, 1), (132, 72, 2, 12, 12, 1)]      # V, H, R, M, B, k
LR, MOM, UPDATES = 0.05, 0.9, 3
FAST_LR, FAST_DECAY = 0.05, 0.95
# what a run is: (case, fast_learning_rate); case 1 forms its own rounded values from its own small rate, and runs under the common one too
RUNS = [(0, FAST_LR), (1, 1e-3), (1, FAST_LR), (2, FAST_LR), (3, FAST_LR)]
NAMES = ('W', 'vb', 'hb', 'dW', 'dvb', 'dhb', 'q_means')
FAST_NAMES = ('W_fast', 'vb_fast', 'hb_fast', 'W_eff', 'vb_eff', 'hb_eff')


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


def engine_state(eng, M, fast=True):
    from boltzmann_machines_amd._ffi import DeviceArray
    Vd, Hd = DeviceArray((M, eng.V)), DeviceArray((M, eng.H))
    swaps, idx = eng.pt_read(Vd, Hd)
    out = {n: eng.get(n) for n in NAMES + (FAST_NAMES if fast else ())}
    out.update(V=Vd.numpy(), H=Hd.numpy(), idx=np.array(idx, np.int32).reshape(-1), swaps=np.array(swaps, np.int64))
    return out


def twin_state(t):
    s = t.state()
    v, h = t.ens.read()
    out = {n: s[n] for n in NAMES + (FAST_NAMES if isinstance(t, F.FastTemperedRBM) else ())}
    out.update(V=v, H=h, idx=s['idx'].astype(np.int32), swaps=s['swaps'])
    return out


def assert_same_state(got, want, what, fast=True):
    for k in NAMES + (FAST_NAMES if fast else ()) + ('V', 'H'):
        assert same(got[k], want[k]), '%s: %s differs in %d entries' % (what, k, int(np.sum(bits(got[k]) != bits(want[k]))))
    assert np.array_equal(got['idx'], want['idx']), '%s: ladder indices differ' % what
    assert np.array_equal(got['swaps'], want['swaps']), '%s: swap counters %s against %s' % (what, got['swaps'].tolist(), want['swaps'].tolist())


def make_twin(case, rate, decay=FAST_DECAY):
    V, H, R, M, B, k = CASES[case]
    return F.FastTemperedRBM(rbm_params(V, H), M, ladder(R), SEED, fast_learning_rate=rate, fast_decay=decay, **config(case))


@functools.lru_cache(maxsize=None)
def twin_run(case, rate):
    """the states after every one of the UPDATES updates (computed once, shared, never modified) and the smallest tie margin"""
    V, H, R, M, B, k = CASES[case]
    t = make_twin(case, rate)
    X = data(UPDATES * B, V)
    out = []
    for u in range(UPDATES):
        t.train_step(X[u * B:(u + 1) * B], LR, MOM, k)
        out.append(twin_state(t))
    return out, (min(t.ens.margins) if t.ens.margins else np.inf)


def decisive_twin(case, rate):
    want, margin = twin_run(case, rate)
    assert margin >= 1e-9, 'a swap draw of this case lies within 1e-9 of its threshold: choose another seed'
    if CASES[case][2] > 1:
        att, acc = want[-1]['swaps']
        assert np.all(att > 0) and 0 < acc.sum() < att.sum()
    return want


def engine_run(case, rate, decay=FAST_DECAY, mode=True):
    from boltzmann_machines_amd._ffi import DeviceArray
    V, H, R, M, B, k = CASES[case]
    eng = rbm_engine(V, H, rbm_params(V, H), B, **config(case))
    if mode:
        eng.set_fast_weights(True, rate, decay)
    eng.pt_init(M, ladder(R))
    Xd = DeviceArray.from_numpy(data(UPDATES * B, V))
    out = []
    for u in range(UPDATES):
        eng.train_step_pt(Xd, B, LR, MOM, k, row=u * B)
        out.append(engine_state(eng, M, fast=mode))
    eng.close()
    return out


@pytest.mark.parametrize('run', range(len(RUNS)))
def test_updates_match_the_twin(gpu_lib, run):
    """three consecutive updates with momentum and l2 (case 1: the sparsity penalty too): regular, fast and effective parameters,
    momentum buffers, q_means and the ensemble after every one"""
    case, rate = RUNS[run]
    want = decisive_twin(case, rate)
    got = engine_run(case, rate)
    for u, (g, w) in enumerate(zip(got, want)):
        assert_same_state(g, w, 'case %d, rate %g, update %d' % (case, rate, u))
    assert np.any(got[0]['W_fast']) and not same(got[0]['W_fast'], got[1]['W_fast'])
    assert not same(got[-1]['W_eff'], got[-1]['W'])


def test_rate_zero_and_mode_off_are_the_plain_update(gpu_lib):
    """the mode on with rate 0: bit-identical, ensemble included, to an engine with the mode off (the fast set stays zero, the
    effective set is the regular one); on -> off -> three plain tempered updates: identical to an engine that never had it"""
    case = 1
    V, H, R, M, B, k = CASES[case]
    plain = engine_run(case, 0.0, mode=False)
    zero = engine_run(case, 0.0, mode=True)
    for u in range(UPDATES):
        assert_same_state(zero[u], plain[u], 'rate 0, update %d' % u, fast=False)
        assert not np.any(zero[u]['W_fast']) and not np.any(zero[u]['vb_fast']) and not np.any(zero[u]['hb_fast'])
        assert same(zero[u]['W_eff'], zero[u]['W']) and same(zero[u]['hb_eff'], zero[u]['hb'])
    from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray
    eng = rbm_engine(V, H, rbm_params(V, H), B, **config(case))
    eng.set_fast_weights(True, FAST_LR, FAST_DECAY)
    eng.set_fast_weights(False)
    with pytest.raises(Bm355Error, match='W_fast'):
        eng.get('W_fast')
    eng.pt_init(M, ladder(R))
    Xd = DeviceArray.from_numpy(data(UPDATES * B, V))
    for u in range(UPDATES):
        eng.train_step_pt(Xd, B, LR, MOM, k, row=u * B)
    assert_same_state(engine_state(eng, M, fast=False), plain[-1], 'on -> off', fast=False)
    eng.close()


@pytest.mark.parametrize('what', ['set_W', 'cd_step'])
def test_stale_effective_copies_are_rebuilt(gpu_lib, what):
    """between the updates 1 and 2 the regular model is written by something else - set('W', ...) or one CD train_step: the
    engine equals a twin that does the same, and W_eff read right after the write is W + W_fast"""
    from boltzmann_machines_amd._ffi import DeviceArray
    case = 3
    V, H, R, M, B, k = CASES[case]
    X = data(UPDATES * B, V)
    W2 = rbm_params(V, H)['W'] * np.float32(0.75)
    t = make_twin(case, FAST_LR)
    eng = rbm_engine(V, H, rbm_params(V, H), B, **config(case))
    eng.set_fast_weights(True, FAST_LR, FAST_DECAY)
    eng.pt_init(M, ladder(R))
    Xd = DeviceArray.from_numpy(X)
    eng.train_step_pt(Xd, B, LR, MOM, k, row=0)
    t.train_step(X[:B], LR, MOM, k)
    if what == 'set_W':
        eng.set('W', W2)
        t.p['W'][...] = W2
    else:
        eng.train_step(Xd, B, LR, MOM, 1, row=B)
        t.cd_step(X[B:2 * B], LR, MOM, 1)
    assert same(eng.get('W'), t.p['W'])
    assert same(eng.get('W_eff'), eng.get('W') + eng.get('W_fast')) and same(eng.get('vb_eff'), eng.get('vb') + eng.get('vb_fast'))
    assert same(eng.get('hb_eff'), eng.get('hb') + eng.get('hb_fast'))
    for u in (1, 2):
        eng.train_step_pt(Xd, B, LR, MOM, k, row=u * B)
        t.train_step(X[u * B:(u + 1) * B], LR, MOM, k)
        assert_same_state(engine_state(eng, M), twin_state(t), '%s, update %d' % (what, u))
    assert min(t.ens.margins) >= 1e-9
    eng.close()


SUB_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tests import test_fpcd_gpu as G
for case in (0, 3):
    got = G.engine_run(case, G.FAST_LR)[-1]
    np.savez(%(out)r %% case, **got)
print('FPCD_OK')
'''


def test_geometries_and_hand_over_variants_give_the_same_bits(gpu_lib, tmp_path):
    """the cases 0 and 3 under the forced grad geometries (4 and 8 waves), two act geometries and both forms of the hand-over
    (pt_sel=0/1): one subprocess each (the switches are read once per process); all equal the twin.  Nothing is started after a
    failure."""
    want = {case: decisive_twin(case, FAST_LR)[-1] for case in (0, 3)}
    for dbg in ('grad_geo=4', 'grad_geo=8', 'act_geo=4', 'act_geo=1', 'pt_sel=0', 'pt_sel=1'):
        out = str(tmp_path / (dbg.replace('=', '') + '_%d.npz'))
        r = subprocess.run([sys.executable, '-c', SUB_SCRIPT % dict(root=ROOT, out=out)],
                           env=dict(os.environ, BM355_DEBUG=dbg), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and 'FPCD_OK' in r.stdout, dbg + ': ' + r.stdout[-2000:] + r.stderr[-4000:]
        for case in (0, 3):
            assert_same_state(dict(np.load(out % case)), want[case], '%s, case %d' % (dbg, case))


def test_native_loop_equals_single_steps(gpu_lib):
    """train_epoch_pt over N = 2 batch + 5 rows (a short last batch) against three train_step_pt calls, and against the twin"""
    from boltzmann_machines_amd._ffi import DeviceArray
    case = 0
    V, H, R, M, B, k = CASES[case]
    N = 2 * B + 5
    X = data(N, V)
    states = []
    for native in (True, False):
        eng = rbm_engine(V, H, rbm_params(V, H), B, **config(case))
        eng.set_fast_weights(True, FAST_LR, FAST_DECAY)
        eng.pt_init(M, ladder(R))
        Xd = DeviceArray.from_numpy(X)
        if native:
            eng.train_epoch_pt(Xd, N, B, LR, MOM, k)
        else:
            for s in range(0, N, B):
                eng.train_step_pt(Xd, min(B, N - s), LR, MOM, k, row=s)
        states.append(engine_state(eng, M))
        eng.close()
    t = make_twin(case, FAST_LR)
    t.train_epoch(X, B, LR, MOM, k)
    assert min(t.ens.margins) >= 1e-9
    assert_same_state(states[0], states[1], 'native loop against single steps')
    assert_same_state(states[0], twin_state(t), 'native loop against the twin')


# ------------------------------------------------------------------------------------------------ public API
NV, NH, BS, NROWS = 16, 12, 10, 60
XTRAIN = (orc.uniform(SEED, 60, 0, NROWS * NV) < 0.4).astype(np.float32).reshape(NROWS, NV)


def _model(tmp_path, name, **kw):
    from boltzmann_machines_amd import BernoulliRBM
    p = rbm_params(NV, NH)
    base = dict(n_visible=NV, n_hidden=NH, batch_size=BS, max_epoch=2, random_seed=1337, verbose=False, n_gibbs_steps=2,
                W_init=p['W'], vb_init=p['vb'], hb_init=p['hb'], model_path=str(tmp_path / name) + '/')
    return BernoulliRBM(**dict(base, **kw))


def test_public_fit_matches_the_twin(gpu_lib, tmp_path):
    """fit() with n_temperatures = 1 and fast weights on 60 rows, two epochs of 6 updates, a metrics iteration every 10th (it
    consumes one call of the stream), against the twin driven by the same host seed; fast_weights() is the engine's set;
    tempering_stats() still answers; a second fit() call starts from a zero fast set"""
    rbm = _model(tmp_path, 'a').set_negative_phase('tempered', n_temperatures=1, n_chains=BS + 3, fast_learning_rate=0.1, fast_decay=0.9)
    seeds = _model(tmp_path, 'seeds')
    seed1, seed2 = seeds.make_random_seed(), seeds.make_random_seed()
    rbm.fit(XTRAIN)
    t = F.FastTemperedRBM(rbm_params(NV, NH), BS + 3, ladder(1), seed1, fast_learning_rate=0.1, fast_decay=0.9, l2=1e-4)
    it = 0
    for epoch in range(2):
        for s in range(0, NROWS, BS):
            it += 1
            if it % 10 == 0:
                t.call += 1                                  # bm_rbm_metrics
            t.train_step(XTRAIN[s:s + BS], 0.01, 0.9, 2)
    assert rbm.iter_ == it == 12
    assert_same_state(engine_state(rbm._engine, BS + 3), twin_state(t), 'fit')
    fw = rbm.fast_weights()
    assert sorted(fw) == ['W', 'hb', 'vb'] and np.any(fw['W'])
    for n in F.NAMES:
        assert same(fw[n], rbm._engine.get(n + '_fast')) and same(fw[n], t.fast[n]), n
    assert rbm.tempering_stats().shape == (0,)
    # a second fit() call: a fresh ensemble under the next host seed and a ZERO fast set
    t2 = F.FastTemperedRBM({n: t.p[n] for n in F.NAMES}, BS + 3, ladder(1), seed2, fast_learning_rate=0.1, fast_decay=0.9, l2=1e-4)
    for n in ('dW', 'dvb', 'dhb', 'q_means'):
        t2.p[n][...] = t.p[n]
    rbm.max_epoch = 3
    rbm.fit(XTRAIN)
    for s in range(0, NROWS, BS):
        it += 1
        if it % 10 == 0:
            t2.call += 1
        t2.train_step(XTRAIN[s:s + BS], 0.01, 0.9, 2)
    assert_same_state(engine_state(rbm._engine, BS + 3), twin_state(t2), 'second fit')
    # switched off again: no fast set
    rbm.set_negative_phase('tempered', n_temperatures=1, n_chains=BS + 3)
    with pytest.raises(RuntimeError, match='no fast weights'):
        rbm.fast_weights()


def test_errors(gpu_lib, tmp_path):
    """centring in either order, bad scalars, a Gaussian / Multinomial / dropout handle"""
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd._ffi import Bm355Error
    V, H = 20, 12
    p = rbm_params(V, H)
    eng = rbm_engine(V, H, p, 6)
    for rate, decay in ((-0.1, 0.9), (float('nan'), 0.9), (float('inf'), 0.9), (0.1, 1.0), (0.1, -0.5), (0.1, float('nan'))):
        with pytest.raises(Bm355Error, match='fast'):
            eng.set_fast_weights(True, rate, decay)
    with pytest.raises(Bm355Error, match='unknown RBM variable'):      # nothing was switched on
        eng.get('W_fast')
    eng.set_centering(True, 0.01, 0.01)
    with pytest.raises(Bm355Error, match='centering'):
        eng.set_fast_weights(True, 0.1, 0.9)
    eng.set_centering(False)
    eng.set_fast_weights(True, 0.1, 0.9)
    with pytest.raises(Bm355Error, match='fast weights'):
        eng.set_centering(True, 0.01, 0.01)
    with pytest.raises(Bm355Error, match='get only'):
        eng.set('W_eff', 0.0)
    eng.set('W_fast', 0.25)
    assert same(eng.get('W_eff'), p['W'] + np.float32(0.25))
    eng.set_fast_weights(True, 0.2, 0.5)                                # on -> on: the scalars only
    assert same(eng.get('W_fast'), np.full((V, H), 0.25, np.float32))
    eng.close()
    from boltzmann_machines_amd.engine import RbmEngine
    for kw, word in ((dict(v_unit=_ffi.UNIT_GAUSSIAN), 'Gaussian'), (dict(h_unit=_ffi.UNIT_MULTINOMIAL, n_samples=3), 'Multinomial'),
                     (dict(dropout=0.8), 'dropout'), (dict(dbm_first=True), 'dbm_first')):
        e = RbmEngine(V, H, max_batch=6, **kw)
        with pytest.raises(Bm355Error, match=word):
            e.set_fast_weights(True, 0.1, 0.9)
        e.close()
    # the public layer: whichever is set second is refused
    r = _model(tmp_path, 'c').set_negative_phase('tempered', n_temperatures=1, fast_learning_rate=0.1)
    with pytest.raises(NotImplementedError, match='fast weights'):
        r.set_centering(True)
    r = _model(tmp_path, 'd').set_centering(True)
    with pytest.raises(NotImplementedError, match='centering'):
        r.set_negative_phase('tempered', n_temperatures=1, fast_learning_rate=0.1)
