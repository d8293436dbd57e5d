#!/usr/bin/env python
"""The price of joint training: one CD-1 update on (x, y) at 784 x 1024, C = 10, batch 512 - generative
(discriminative_weight 0) and hybrid (1) - and class-conditional sampling, beside the plain CD-1 update of the SAME handle.

ONE process, ONE handle, the legs alternating after a warm-up call each (launch tuning, code objects).  Times are HIP-event
times on the engine's stream around `--updates` calls that only enqueue (the epoch entries without out2; `--steps` Gibbs steps
of bm_rbm_class_gibbs on 512 chains for the sampling leg); `--runs` samples per leg.  The ratios to the plain update are
recorded, not asserted.  Prints a markdown report; --out writes it as well (meant for profiles/class_joint_bench.md).

    python tools/bench_class_joint.py [--runs 20] [--updates 100] [--steps 100] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H, B, C_ = 784, 1024, 512, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--updates', type=int, default=100)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    n = args.updates
    X = (philox.uniform(87654321, 42, 0, n * B * V).reshape(n * B, V) < 0.1307).astype(np.float32)      # bench.py's density
    Xd = DeviceArray.from_numpy(X)
    rng = np.random.RandomState(7)
    yd = DeviceArray.from_numpy(rng.randint(0, C_, n * B).astype(np.int32), np.int32)
    eng = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5)
    eng.set('W', philox.tf_random_normal((V, H), 0.01, 1337))                                            # bench.py's weights
    eng.set_classes(C_)
    eng.set('U', (rng.randn(C_, H) * 0.01).astype(np.float32))
    eng.seed(1)
    out_v = DeviceArray((B, V), np.float32)
    legs = [('plain CD-1 update (bm_rbm_train_epoch)', n, lambda: eng.train_epoch(Xd, n * B, B, 0.01, 0.9, 1)),
            ('joint CD-1 update, discriminative_weight 0', n, lambda: eng.class_joint_train_epoch(Xd, yd, n * B, B, 1, 0.01, 0.9, 0.0, fetch=False)),
            ('joint CD-1 update, discriminative_weight 1', n, lambda: eng.class_joint_train_epoch(Xd, yd, n * B, B, 1, 0.01, 0.9, 1.0, fetch=False)),
            ('class-conditional Gibbs step, 512 chains (bm_rbm_class_gibbs)', args.steps, lambda: eng.class_gibbs(None, yd, B, args.steps, out_v))]
    for _, _, call in legs:
        call()
        eng.sync()
    us = {name: [] for name, _, _ in legs}
    for _ in range(args.runs):
        for name, per, call in legs:
            eng.timer_start()
            call()
            us[name].append(1e3 * eng.timer_stop() / per)
    base = float(np.median(us[legs[0][0]]))
    out = ['| leg | us / update or step (median, min - max) | ratio to the plain update |', '|---|---|---|']
    for name, _, _ in legs:
        v = us[name]
        out.append('| %s | %.1f (%.1f - %.1f) | %.2f |' % (name, float(np.median(v)), min(v), max(v), float(np.median(v)) / base))
    out += ['', '%d runs per leg of %d updates (%d Gibbs steps), alternating in one process on one handle, HIP-event times; 784 x 1024, C = 10, '
            'batch 512.  The plain update runs its chain as the handle runs it by default (one chained launch where the shape allows it); the '
            'joint update issues per-pass launches: the class-bias prop-up, the visible pass, class_draw_kernel, class_joint_update_kernel '
            'and the unchanged fused update - with discriminative_weight > 0 also launches 1 - 3 of the discriminative update and the '
            'elementwise mix.' % (args.runs, n, args.steps)]
    out += ['', '| leg | act_up (class-bias prop-ups; class-rows prop-up) | act_down | other (class_draw; class_row) | colsum (class_hidden) | '
            'bias (class_joint_update; class_mix) | grad (outer products + bias tail) |', '|---|---|---|---|---|---|---|']
    for name, _, call in legs[1:3]:
        eng.profile(True)
        call()
        t = eng.kernel_times()
        eng.profile(False)
        out.append('| %s | %s |' % (name, ' | '.join('%.1f us / update (%d timed scopes)' % (1e3 * t[k][0] / n, t[k][1] // n)
                                                      for k in ('act_up', 'act_down', 'other', 'colsum', 'bias', 'grad'))))
    out += ['', 'Per-kernel class: HIP-event time per update over %d profiled updates (bm_rbm_profile: an event pair per scope, which keeps the '
            'launches from overlapping).' % n]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
