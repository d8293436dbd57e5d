#!/usr/bin/env python
"""The price of the class head: one discriminative update and one `predict` at 784 x 1024, batch 512.

C = 10 classes, and C = 2 for the floor of the class-rows epilogue; the plain CD-1 update of the same engine shape runs beside
them for scale.  ONE process, the legs alternating after a warm-up call each (launch tuning, code objects).  Times are HIP-event
times on the engine's stream around `--updates` calls that only enqueue (bm_rbm_class_train_epoch without out2;
bm_rbm_class_log_proba synchronises per call, so a predict is timed around its own calls, read-back of [B, C] included); `--runs`
samples per leg.  The per-kernel times come from bm_rbm_profile over `--updates` updates: the class update leaves the event
classes `colsum` and `bias` to class_hidden_kernel and class_head_update_kernel, `other` is class_row_kernel, `act_up` the
class-rows prop-up, `grad` the unchanged outer-product launch with its bias tail.  Prints a markdown report; --out writes it as
well (meant for profiles/class_head_bench.md).

    python tools/bench_class_head.py [--runs 20] [--updates 100] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H, B = 784, 1024, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--updates', type=int, default=100)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    n = args.updates
    X = (philox.uniform(87654321, 42, 0, n * B * V).reshape(n * B, V) < 0.1307).astype(np.float32)      # bench.py's density
    Xd = DeviceArray.from_numpy(X)
    W = philox.tf_random_normal((V, H), 0.01, 1337)                                                      # bench.py's weights
    rng = np.random.RandomState(7)
    legs = []
    for name, C_ in (('plain CD-1 update', 0), ('class update, C = 10', 10), ('class update, C = 2', 2)):
        eng = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5)
        eng.set('W', W)
        eng.seed(1)
        yd = None
        if C_:
            eng.set_classes(C_)
            eng.set('U', (rng.randn(C_, H) * 0.01).astype(np.float32))
            yd = DeviceArray.from_numpy(rng.randint(0, C_, n * B).astype(np.int32), np.int32)
            call = (lambda e, y: lambda: e.class_train_epoch(Xd, y, n * B, B, 0.05, 0.9, fetch=False))(eng, yd)
        else:
            call = (lambda e: lambda: e.train_epoch(Xd, n * B, B, 0.05, 0.9, 1))(eng)
        legs.append((name, C_, eng, yd, call))
    for _, _, eng, _, call in legs:
        call()
        eng.sync()
    us = {name: [] for name, _, _, _, _ in legs}
    pred = {name: [] for name, C_, _, _, _ in legs if C_}
    for _ in range(args.runs):
        for name, C_, eng, _, call in legs:
            eng.timer_start()
            call()
            us[name].append(1e3 * eng.timer_stop() / n)
            if C_:
                eng.timer_start()
                for i in range(8):
                    eng.class_log_proba(Xd, B, row=i * B)
                pred[name].append(1e3 * eng.timer_stop() / 8)
    fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
    out = ['| leg | us / update (median, min - max) | us / predict of 512 rows, read-back included (median, min - max) |', '|---|---|---|']
    for name, C_, _, _, _ in legs:
        out.append('| %s | %s | %s |' % (name, fmt(us[name]), fmt(pred[name]) if C_ else '-'))
    out += ['', '%d runs of %d updates per leg, alternating in one process, HIP-event times; 784 x 1024, batch 512.' % (args.runs, n), '',
            '| leg | act_up (class-rows prop-up) | other (class_row) | colsum (class_hidden) | bias (class_head_update) | grad (outer products + bias tail) |',
            '|---|---|---|---|---|---|']
    for name, C_, eng, yd, call in legs:
        if not C_:
            continue
        eng.profile(True)
        call()
        t = eng.kernel_times()
        eng.profile(False)
        out.append('| %s | %s |' % (name, ' | '.join('%.1f us x %d' % (1e3 * t[k][0] / max(t[k][1], 1), t[k][1])
                                                      for k in ('act_up', 'other', 'colsum', 'bias', 'grad'))))
    out += ['', 'Per-kernel: mean HIP-event time per launch over %d profiled updates (bm_rbm_profile: an event pair per launch, which keeps '
            'the launches from overlapping).' % n]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
