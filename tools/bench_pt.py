#!/usr/bin/env python
"""The price of a tempered sweep, at 784 x 1024 with R = 10 temperatures and M = 512 chains (5120 rows).

Three calls are timed in ONE run, alternating, --runs times each after a warm-up call (launch tuning, code objects):

  a. RbmEngine.pt_sweep: one step = a row-tempered prop-up, the swap launch, a row-tempered prop-down over all 5120 rows
  b. RbmEngine.gibbs at batch 512, the per-sweep time x 10: what R launches of a single-temperature chain would cost per
     step (the sweep this compares with runs as ONE chained launch where the shape allows it: csrc/bm_chain.h)
  c. RbmEngine.gibbs at batch 5120: one sweep over as many rows at one temperature, i.e. what the per-row temperature, the
     energy partials and the swap launch add

Times are HIP-event times on the engine's stream around `--steps` steps per call (the calls only enqueue).  Prints a markdown
report; --out writes it as well (meant for the measured section of profiles/pt_bench.md).

    python tools/bench_pt.py [--runs 7] [--steps 50] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

V, H, M, R = 784, 1024, 512, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    n = args.steps
    rng = np.random.RandomState(0)
    eng = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=M * R)
    eng.set('W', philox.tf_random_normal((V, H), 0.01, 1337))                # bench.py's weights
    eng.seed(1)
    betas = np.linspace(0., 1., R + 1)[1:].astype(np.float32)
    eng.pt_init(M, betas)
    Hs = DeviceArray.from_numpy((rng.rand(M, H) < 0.5).astype(np.float32))
    Vs = DeviceArray((M, V))
    Hl = DeviceArray.from_numpy((rng.rand(M * R, H) < 0.5).astype(np.float32))
    Vl = DeviceArray((M * R, V))
    calls = [('pt_sweep, %d chains x %d temperatures' % (M, R), lambda: eng.pt_sweep(n)),
             ('gibbs, batch %d' % M, lambda: eng.gibbs(Hs, Vs, M, n)),
             ('gibbs, batch %d' % (M * R), lambda: eng.gibbs(Hl, Vl, M * R, n))]
    for _, call in calls:                                                    # warm-up of every shape the timed window uses
        call()
    eng.sync()
    ms = [[] for _ in calls]
    for _ in range(args.runs):                                               # alternating: a drift of the box hits all three
        for k, (_, call) in enumerate(calls):
            eng.timer_start()
            call()
            ms[k].append(eng.timer_stop())
    chained = eng.chain_stats()
    swaps, _ = eng.pt_read()
    eng.close()

    us = [[1e3 * t / n for t in row] for row in ms]                          # per step
    med = lambda t: float(np.median(t))
    each = lambda t: ', '.join('%.1f' % x for x in t)
    spread = lambda t: (max(t) - min(t)) / med(t)
    pt, small, large = (med(u) for u in us)
    flops = 2 * 2.0 * M * R * V * H
    lines = [
        '## Measured (`tools/bench_pt.py`)',
        '',
        'One MI355X, one process; %d x %d, R = %d, M = %d; every call %d steps, one warm-up, then %d timed runs, the three calls'
        % (V, H, R, M, n, args.runs),
        'alternating; HIP-event time on the engine stream.',
        '',
        '| call | us per step (each run) | median us | (max - min) / median |',
        '|---|---|---|---|',
    ] + ['| `%s` | %s | %.1f | %.3f |' % (name, each(u), med(u), spread(u)) for (name, _), u in zip(calls, us)] + [
        '',
        '* tempered step / (10 x the batch-%d sweep) = %.1f / %.1f = %.3f' % (M, pt, R * small, pt / (R * small)),
        '* tempered step / one batch-%d sweep = %.1f / %.1f = %.3f: the price of the per-row temperature, the energy partials and'
        % (M * R, pt, large, pt / large),
        '  the swap launch, and of per-pass launches where the plain sweep is chained (%d chained launches were issued, chain'
        % chained[0],
        '  mode %d)' % chained[2],
        '* algorithmic rate of the tempered step: %.2f GFLOP per step (2 passes x 2 M R V H) -> %.1f TFLOP/s, %.3f of the'
        % (flops / 1e9, flops / (pt * 1e-6) / 1e12, flops / (pt * 1e-6) / 157.3e12),
        '  157.3 TFLOP/s fp32 matrix peak (a whole-call rate, not a kernel\'s share of peak)',
        '* swap acceptance per ladder pair over the run (zero-mean N(0, 0.01) weights: close to 1): '
        + ', '.join('%.2f' % (a / max(t, 1)) for t, a in zip(swaps[0], swaps[1])),
    ]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
