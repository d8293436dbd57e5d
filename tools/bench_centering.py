#!/usr/bin/env python
"""The price of the centred update against the plain one.

Two shapes, each in ONE process with the two engines alternating, after a warm-up call per engine (launch tuning, code
objects):

  rbm  784 x 1024, batch 512, CD-1:   bm_rbm_train_epoch, plain against centred (nu = 0.01)
  dbm  784-512-1024, 512 rows, 512 particles, PCD-1:   bm_dbm_train_step, plain against centred

Times are HIP-event times on the engine's stream around `--updates` updates per call (the calls only enqueue; the DBM's
mean-field loop control makes its own host round trips in both legs alike); `--runs` calls per engine, at least 2000 updates per
engine in all by default.  Prints a markdown report; --out writes it as well (meant for the measured section of
profiles/centering_bench.md).  The added launches are those of DESIGN.md 3.17's table.

    python tools/bench_centering.py [--runs 20] [--updates 100] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def alternate(calls, runs, n):
    """calls: [(name, engine, fn)]; returns {name: [us per update of every run]}"""
    for _, eng, call in calls:
        call()
        eng.sync()
    us = {name: [] for name, _, _ in calls}
    for _ in range(runs):
        for name, eng, call in calls:
            eng.timer_start()
            call()
            us[name].append(1e3 * eng.timer_stop() / n)
    return us


def rbm_leg(runs, n):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    V, H, B = 784, 1024, 512
    X = (philox.uniform(87654321, 42, 0, n * B * V).reshape(n * B, V) < 0.1307).astype(np.float32)      # bench.py's density
    Xd = DeviceArray.from_numpy(X)
    W = philox.tf_random_normal((V, H), 0.01, 1337)                                                      # bench.py's weights
    calls = []
    for name in ('plain', 'centred'):
        eng = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5)
        eng.set('W', W)
        eng.seed(1)
        if name == 'centred':
            eng.set_centering(True, 0.01, 0.01)
            eng.set('ov', X.mean(0)); eng.set('oh', np.float32(0.5))
        calls.append((name, eng, (lambda e: lambda: e.train_epoch(Xd, n * B, B, 0.05, 0.9, 1))(eng)))
    return alternate(calls, runs, n)


def dbm_leg(runs, n):
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import DbmEngine
    from boltzmann_machines_amd.utils import philox
    V, H1, H2, N = 784, 512, 1024, 512
    X = (philox.uniform(87654321, 42, 0, N * V).reshape(N, V) < 0.1307).astype(np.float32)
    Xd = DeviceArray.from_numpy(X)
    calls = []
    for name in ('plain', 'centred'):
        eng = DbmEngine(V, [H1, H2], sample_v_states=True, n_particles=N, batch_size=N, max_mf_updates=10, mf_tol=1e-7, l2=1e-5)
        eng.set('W', philox.tf_random_normal((V, H1), 0.01, 1337))
        eng.set('W_1', philox.tf_random_normal((H1, H2), 0.01, 1338))
        eng.seed(1)
        if name == 'centred':
            eng.set_centering(True, 0.01)
            eng.set('ov', X.mean(0)); eng.set('oh', np.float32(0.5)); eng.set('oh_1', np.float32(0.5))

        def call(e=eng):
            for _ in range(n):
                e.train_step(Xd, 0.01, 0.9, 1)
        calls.append((name, eng, call))
    return alternate(calls, runs, n)


def report(res, runs, n):
    out = ['| shape | plain us / update (median, min - max) | centred us / update (median, min - max) | difference (medians) | added launches |',
           '|---|---|---|---|---|']
    fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
    for shape, added in (('rbm 784 x 1024 x 512, CD-1', '3 (sparsity off)'), ('dbm 784-512-1024, 512 rows, 512 particles, PCD-1', '2')):
        us = res[shape.split()[0]]
        out.append('| %s | %s | %s | %+.1f | %s |' % (shape, fmt(us['plain']), fmt(us['centred']),
                                                    float(np.median(us['centred']) - np.median(us['plain'])), added))
    out.append('')
    out.append('%d runs of %d updates per engine and shape, alternating in one process per shape, HIP-event times.' % (runs, n))
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--updates', type=int, default=100)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    res = dict(rbm=rbm_leg(args.runs, args.updates), dbm=dbm_leg(args.runs, args.updates))
    text = report(res, args.runs, args.updates)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
