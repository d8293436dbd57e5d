#!/usr/bin/env python
"""The price of a tempered DBM step, at 784-512-1024 with M = 64 chains x R = 8 temperatures (512 rows).

Two calls are timed in ONE run, alternating, --runs times each after a warm-up call (launch tuning, code objects):

  a. DbmEngine.pt_sweep: one step = the two-segment row-tempered h1 pass, the swap launch, the row-tempered h2 and v passes
     over all 512 rows (four launches)
  b. DbmEngine.sample_v(k) with 512 particles, every layer sampled: k sampled sweeps and k mean sweeps of the same three
     passes at one temperature (plus two copies of v per call); the time per sweep is the call's time / 2k - the plain sweep
     of as many rows, i.e. what the per-row temperature, the energy partials and the swap launch add

Times are HIP-event times on the engine's stream around `--steps` steps per call.  Prints a markdown report; --out writes it
as well (meant for the measured section of profiles/dbm_pt_bench.md).

    python tools/bench_dbm_pt.py [--runs 7] [--steps 50] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

N = (784, 512, 1024)
M, R = 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd.engine import DbmEngine
    from boltzmann_machines_amd.utils import philox
    n = args.steps
    rows = M * R
    eng = DbmEngine(N[0], list(N[1:]), n_particles=rows, batch_size=rows)
    eng.set('W', philox.tf_random_normal((N[0], N[1]), 0.01, 1337))          # bench.py's scale of weights
    eng.set('W_1', philox.tf_random_normal((N[1], N[2]), 0.01, 1338))
    rng = np.random.RandomState(0)
    eng.set('v', (rng.rand(rows, N[0]) < 0.5).astype(np.float32))
    eng.set('h_1', (rng.rand(rows, N[2]) < 0.5).astype(np.float32))
    eng.seed(1)
    eng.pt_init(M, np.linspace(0., 1., R + 1)[1:].astype(np.float32))
    calls = [('pt_sweep, %d chains x %d temperatures' % (M, R), lambda: eng.pt_sweep(n), n),
             ('sample_v, %d particles (sampled + mean sweeps)' % rows, lambda: eng.sample_v(n // 2), 2 * (n // 2))]
    for _, call, _ in calls:                                                 # warm-up of every shape the timed window uses
        call()
    eng.sync()
    ms = [[] for _ in calls]
    for _ in range(args.runs):                                               # alternating: a drift of the box hits both
        for k, (_, call, _) in enumerate(calls):
            eng.timer_start()
            call()
            ms[k].append(eng.timer_stop())
    swaps, _ = eng.pt_read()
    eng.close()

    us = [[1e3 * t / cnt for t in row] for row, (_, _, cnt) in zip(ms, calls)]       # per step / per sweep
    med = lambda t: float(np.median(t))
    each = lambda t: ', '.join('%.1f' % x for x in t)
    spread = lambda t: (max(t) - min(t)) / med(t)
    pt, plain = (med(u) for u in us)
    flops = 2.0 * rows * (N[0] * N[1] + N[1] * N[2]) * 2
    lines = [
        '## Measured (`tools/bench_dbm_pt.py`)',
        '',
        'One MI355X, one process; %d-%d-%d, M = %d, R = %d (%d rows); every call %d steps / sweeps, one warm-up, then %d timed'
        % (N + (M, R, rows, n, args.runs)),
        'runs, the two calls alternating; HIP-event time on the engine stream.',
        '',
        '| call | us per step or sweep (each run) | median us | (max - min) / median |',
        '|---|---|---|---|',
    ] + ['| `%s` | %s | %.1f | %.3f |' % (name, each(u), med(u), spread(u)) for (name, _, _), u in zip(calls, us)] + [
        '',
        '* tempered step / plain sweep of %d rows = %.1f / %.1f = %.3f: the price of the per-row temperature, the energy partials'
        % (rows, pt, plain, pt / plain),
        '  and the swap launch (the plain figure averages sampled and mean sweeps and carries two copies of v per call)',
        '* algorithmic rate of the tempered step: %.2f GFLOP per step (v W0 and h1 W1 once up, once down) -> %.1f TFLOP/s'
        % (flops / 1e9, flops / (pt * 1e-6) / 1e12),
        '  (a whole-call rate of four small launches, not a kernel\'s share of peak)',
        '* swap acceptance per ladder pair over the run (zero-mean N(0, 0.01) weights): '
        + ', '.join('%.2f' % (a / max(t, 1)) for t, a in zip(swaps[0], swaps[1])),
    ]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
