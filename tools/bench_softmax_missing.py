#!/usr/bin/env python
"""The prices of incomplete rows, clamped groups and exact group conditionals at 784 x 1024, batch 512, K = 4
(196 groups):
  * one CD-1 update with bm_rbm_groups_set_missing on against the same update with the mode off, on the same complete one-hot
    rows - the mode adds the mask kernel and runs every prop-down in the SM + CL flavour;
  * one clamped Gibbs step (bm_rbm_groups_gibbs_clamped, half of the groups held) against an unclamped one (bm_rbm_gibbs);
  * bm_rbm_groups_scores of 512 rows: the whole call by the host clock (prop-up, group_scores_kernel, the copy of 512 x 784
    doubles, the synchronise) and the kernel alone by the handle's per-class event timing, beside the floor
        B V H x (instructions of one softplus_hw term + 3) / (VALU lanes x clock).
    One softplus_hw term is 7 VALU instructions (|x| * -log2(e), v_exp_f32, 1 + e, v_log_f32, * ln 2, max(x, 0), the add); + 3:
    the add that forms the argument, the conversion to double and the double add.  256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz.  The
    floor counts every instruction at full rate (the two transcendentals issue at a quarter of it) and no load, no address
    arithmetic and no select: it is a lower bound of the arithmetic alone, not a target.

One handle per leg, the legs of a pair alternating after a warm-up call each (launch tuning, code objects).  Update and sweep
times are HIP-event times on the engine's stream around calls that only enqueue.  No target and no assertion: the figures are the
record.  Prints a markdown report; --out writes it as well (meant for profiles/softmax_missing_bench.md).

    python tools/bench_softmax_missing.py [--runs 10] [--updates 48] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H, B, K, LR = 784, 1024, 512, 4, 0.01
SOFTPLUS_INSTR, LANES, CLOCK = 7, 256 * 4 * 16, 2.4e9


def one_hot_rows(n, seed):
    cats = np.random.RandomState(seed).randint(0, K, (n, V // K))
    return (cats[:, :, None] == np.arange(K)[None, None, :]).astype(np.float32).reshape(n, V)


def handle(W):
    from boltzmann_machines_amd.engine import RbmEngine
    e = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5, v_groups=K)
    e.set('W', W)
    e.seed(1)
    return e


def alternate(legs, runs):
    """{name: [ms] * runs}: legs = {name: (engine, enqueue)}, warmed up once each, then alternating"""
    for e, f in legs.values():
        f()
        e.sync()
    ms = {n: [] for n in legs}
    for _ in range(runs):
        for n, (e, f) in legs.items():
            e.timer_start()
            f()
            ms[n].append(e.timer_stop())
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--updates', type=int, default=48)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.utils import philox
    W = philox.tf_random_normal((V, H), 0.01, 1337)             # bench.py's weights
    n_rows, reps = 4 * B, args.updates // 4
    X = one_hot_rows(n_rows, K)
    Xd = DeviceArray.from_numpy(X)
    fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
    out = []

    # 1. the update, mode on against mode off
    on, off = handle(W), handle(W)
    on.groups_set_missing(True)
    ms = alternate({'off': (off, lambda: [off.train_epoch(Xd, n_rows, B, LR, 0.9, 1) for _ in range(reps)]),
                    'on': (on, lambda: [on.train_epoch(Xd, n_rows, B, LR, 0.9, 1) for _ in range(reps)])}, args.runs)
    us = {n: [1e3 * t / (4 * reps) for t in v] for n, v in ms.items()}
    out += ['| CD-1 update on complete rows | us per update (median, min - max) | ratio to mode off |', '|---|---|---|',
            '| mode off (SM prop-down) | %s | 1 |' % fmt(us['off']),
            '| mode on (mask kernel + SM + CL prop-down) | %s | %.3f |' % (fmt(us['on']), np.median(us['on']) / np.median(us['off'])), '']
    on.close(); off.close()

    # 2. one Gibbs step, clamped against unclamped
    a, b = handle(W), handle(W)
    steps = 16
    mask = np.repeat(np.random.RandomState(2).uniform(size=(B, V // K)) < 0.5, K, axis=1).astype(np.float32)
    Va, Ha, Ca, Ma = DeviceArray.from_numpy(X[:B]), DeviceArray((B, H), np.float32), DeviceArray.from_numpy(X[:B]), DeviceArray.from_numpy(mask)
    Vb = DeviceArray((B, V), np.float32)
    Hb = DeviceArray.from_numpy((np.random.RandomState(3).uniform(size=(B, H)) < 0.5).astype(np.float32))
    ms = alternate({'plain': (b, lambda: [b.gibbs(Hb, Vb, B, steps) for _ in range(reps)]),
                    'clamped': (a, lambda: [a.groups_gibbs_clamped(Va, Ha, B, steps, Ca, Ma) for _ in range(reps)])}, args.runs)
    us = {n: [1e3 * t / (steps * reps) for t in v] for n, v in ms.items()}
    out += ['| one Gibbs step (prop-down + prop-up, both sampled) | us per step (median, min - max) | ratio to unclamped |', '|---|---|---|',
            '| bm_rbm_gibbs | %s | 1 |' % fmt(us['plain']),
            '| bm_rbm_groups_gibbs_clamped, half of the groups held | %s | %.3f |'
            % (fmt(us['clamped']), np.median(us['clamped']) / np.median(us['plain'])), '']
    a.close(); b.close()

    # 3. the scores
    wall, up, kern = scores_leg(W, X, args.runs)
    floor = 1e6 * B * V * H * (SOFTPLUS_INSTR + 3) / (LANES * CLOCK)
    out += ['| bm_rbm_groups_scores, %d rows, 30 %% of the groups empty | us (median, min - max) |' % B, '|---|---|',
            '| whole call, host clock (prop-up, kernel, copy of %d x %d doubles, synchronise) | %s |' % (B, V, fmt(wall)),
            '| its prop-up alone, event pair | %s |' % fmt(up),
            '| group_scores_kernel alone, event pair | %s |' % fmt(kern),
            '| floor B V H x (%d + 3) / (%d lanes x %.1f GHz) | %.1f |' % (SOFTPLUS_INSTR, LANES, CLOCK / 1e9, floor),
            '| kernel / floor | %.2f |' % (np.median(kern) / floor), '',
            '%d runs per leg at %d x %d, batch %d, K = %d (%d groups); updates: %d per run, Gibbs steps: %d per run, the two legs of a pair '
            'alternating on one handle each, HIP-event times; bench.py\'s weights, one-hot rows.  The floor is the arithmetic of the '
            'softplus terms alone at full VALU rate (see the tool\'s header); no speed target is set.'
            % (args.runs, V, H, B, K, V // K, 4 * reps, steps * reps)]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


def scores_leg(W, X, runs):
    """(whole call by the host clock, the prop-up's event time, group_scores_kernel's event time), us, `runs` samples each"""
    from boltzmann_machines_amd._ffi import DeviceArray
    e = handle(W)
    Xg = X[:B].copy()
    Xg[np.repeat(np.random.RandomState(4).uniform(size=(B, V // K)) < 0.3, K, axis=1)] = 0.0
    Xgd = DeviceArray.from_numpy(Xg)
    e.groups_scores(Xgd, B)
    e.sync()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        e.groups_scores(Xgd, B)
        wall.append(1e6 * (time.perf_counter() - t0))
    e.profile(True)
    kern, up = [], []
    for _ in range(runs):
        t0 = e.kernel_times()
        e.groups_scores(Xgd, B)
        t1 = e.kernel_times()
        kern.append(1e3 * (t1['other'][0] - t0['other'][0]))
        up.append(1e3 * (t1['act_up'][0] - t0['act_up'][0]))
    e.profile(False)
    e.close()
    return wall, up, kern


if __name__ == '__main__':
    main()
