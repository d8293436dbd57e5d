#!/usr/bin/env python
"""The price of clamping.  Two pairs, each timed --runs times after one warm-up call (launch tuning):

  * RbmEngine.gibbs_clamped against RbmEngine.gibbs at 784 x 1024 x 512, 10 sweeps, a 50 % mask.  The unclamped sweep runs
    as ONE chained launch (csrc/bm_chain.h) where the shape allows it; the clamped one as 20 per-pass launches + the initial
    blend, with 2 B V 4 bytes of extra reads per visible pass.
  * DbmEngine.sample_v_clamped against DbmEngine.sample_v at 784-512-1024, 512 particles, 5 sweeps.

Prints a markdown report (meant for profiles/clamped_bench.md).  Times are HIP-event times around the calls on the engine's
stream for the RBM pair (the calls only enqueue) and wall clock for the DBM pair (both calls end with a host wait).

    python tools/bench_clamped.py [--runs 5] [--sweeps 10] [--dbm-sweeps 5] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

V, H, B = 784, 1024, 512
DV, DH, DM = 784, [512, 1024], 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--sweeps', type=int, default=10)
    ap.add_argument('--dbm-sweeps', type=int, default=5)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import DbmEngine, RbmEngine
    from boltzmann_machines_amd.utils import philox
    n = args.sweeps
    rng = np.random.RandomState(0)
    W = philox.tf_random_normal((V, H), 0.01, 1337)                          # bench.py's weights
    eng = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B)
    eng.set('W', W)
    eng.seed(1)
    v0 = (rng.rand(B, V) < 0.5).astype(np.float32)
    h0 = (rng.rand(B, H) < 0.5).astype(np.float32)
    mask = (rng.rand(B, V) < 0.5).astype(np.float32)
    Vd, Hd = DeviceArray.from_numpy(v0), DeviceArray.from_numpy(h0)
    Cd, Md = DeviceArray.from_numpy(v0), DeviceArray.from_numpy(mask)

    def event_ms(call):
        call()                                                               # warm-up: launch tuning of the shapes
        eng.sync()
        out = []
        for _ in range(args.runs):
            eng.timer_start()
            call()
            out.append(eng.timer_stop())
        return out
    t_plain = event_ms(lambda: eng.gibbs(Hd, Vd, B, n))
    t_clamp = event_ms(lambda: eng.gibbs_clamped(Vd, Hd, B, n, Cd, Md))
    chained = eng.chain_stats()
    eng.close()

    dbm = DbmEngine(DV, DH, n_particles=DM, batch_size=DM)
    dbm.set('W', philox.tf_random_normal((DV, DH[0]), 0.01, 1337))
    dbm.set('W_1', philox.tf_random_normal((DH[0], DH[1]), 0.01, 1338))
    dbm.seed(1)
    dmask = (rng.rand(DM, DV) < 0.5).astype(np.float32)
    dval = (rng.rand(DM, DV) < 0.5).astype(np.float32)
    DCd, DMd = DeviceArray.from_numpy(dval), DeviceArray.from_numpy(dmask)

    def wall_ms(call):
        call()
        out = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            call()
            out.append(1e3 * (time.perf_counter() - t0))
        return out
    k = args.dbm_sweeps
    d_plain = wall_ms(lambda: dbm.sample_v(k))
    d_clamp = wall_ms(lambda: dbm.sample_v_clamped(k, DCd, DMd))
    dbm.close()

    med = lambda t: float(np.median(t))
    each = lambda t: ', '.join('%.3f' % x for x in t)
    spread = lambda t: (max(t) - min(t)) / med(t)
    lines = [
        '# The price of clamped sweeps (`tools/bench_clamped.py`)',
        '',
        'One MI355X, one session; each call: one warm-up, then %d timed runs.' % args.runs,
        '',
        '| call | ms per run (each) | median ms | (max - min) / median |',
        '|---|---|---|---|',
        '| `RbmEngine.gibbs`, %d x %d x %d, %d sweeps | %s | %.3f | %.3f |' % (V, H, B, n, each(t_plain), med(t_plain), spread(t_plain)),
        '| `RbmEngine.gibbs_clamped`, same, 50 %% mask | %s | %.3f | %.3f |' % (each(t_clamp), med(t_clamp), spread(t_clamp)),
        '| `DbmEngine.sample_v`, %d-%d-%d, M = %d, k = %d | %s | %.3f | %.3f |' % (DV, DH[0], DH[1], DM, k, each(d_plain), med(d_plain), spread(d_plain)),
        '| `DbmEngine.sample_v_clamped`, same, 50 %% mask | %s | %.3f | %.3f |' % (each(d_clamp), med(d_clamp), spread(d_clamp)),
        '',
        'RBM: clamped / unclamped = %.3f (medians; HIP-event time on the engine stream).  The unclamped sweeps issued %d chained'
        % (med(t_clamp) / med(t_plain), chained[0]),
        'launch(es) (chain mode %d); the clamped sweeps are %d per-pass launches and one blend, and read 2 B V 4 = %.1f MB more per'
        % (chained[2], 2 * n, 2 * B * V * 4 / 1e6),
        'visible pass.  DBM: clamped / unclamped = %.3f (medians; wall clock, both calls end with a host wait).'
        % (med(d_clamp) / med(d_plain)),
    ]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
