#!/usr/bin/env python
"""The price of semi-supervised training: one update on unlabelled rows and one semi-supervised iteration (a
joint update plus an unlabelled one) at 784 x 1024, C = 10, batch 512, beside the joint CD-1 update of the SAME handle.

ONE process, ONE handle, the legs alternating after a warm-up call each (launch tuning, code objects).  Times are HIP-event
times on the engine's stream around `--updates` calls that only enqueue (the epoch entries without out4; the unlabelled leg is
a loop over bm_rbm_class_unsup_train_step without out2); `--runs` samples per leg.  The ratios to the joint update are recorded,
not asserted.  Prints a markdown report; --out writes it as well (meant for profiles/class_semi_bench.md).

    python tools/bench_class_semi.py [--runs 20] [--updates 100] [--out FILE]"""
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

    def unlabelled():
        for u in range(n):
            eng.class_unsup_train_step(Xd, B, 1, 0.01, 0.9, row=u * B, fetch=False)

    legs = [('joint CD-1 update (bm_rbm_class_joint_train_epoch)', lambda: eng.class_joint_train_epoch(Xd, yd, n * B, B, 1, 0.01, 0.9, 0.0, fetch=False)),
            ('unlabelled CD-1 update (bm_rbm_class_unsup_train_step)', unlabelled),
            ('semi-supervised iteration: joint + unlabelled update (bm_rbm_class_semi_train_epoch)',
             lambda: eng.class_semi_train_epoch(Xd, yd, n * B, Xd, n * B, 0, B, 1, 0.01, 0.9, 0.0, 1.0, fetch=False))]
    for _, call in legs:
        call()
        eng.sync()
    us = {name: [] for name, _ in legs}
    for _ in range(args.runs):
        for name, call in legs:
            eng.timer_start()
            call()
            us[name].append(1e3 * eng.timer_stop() / n)
    base = float(np.median(us[legs[0][0]]))
    out = ['| leg | us / update or iteration (median, min - max) | ratio to the joint update |', '|---|---|---|']
    for name, _ in legs:
        v = us[name]
        out.append('| %s | %.1f (%.1f - %.1f) | %.2f |' % (name, float(np.median(v)), min(v), max(v), float(np.median(v)) / base))
    out += ['', '%d runs per leg of %d updates, alternating in one process on one handle, HIP-event times; 784 x 1024, C = 10, batch 512.  '
            'The unlabelled update issues the class-rows prop-up with class_row_kernel, class_posterior_kernel, the joint chain '
            '(class-bias prop-up, visible pass, class_draw_kernel, class-bias prop-up), class_marginal_kernel, '
            'class_unsup_update_kernel and the unchanged fused update.' % (args.runs, n)]
    out += ['', '| leg | act_up (class-rows prop-up; class-bias prop-ups) | act_down | other (class_row; class_posterior; class_draw) | '
            'colsum (class_marginal) | bias (class_unsup_update) | grad (outer products + bias tail) |', '|---|---|---|---|---|---|---|']
    eng.profile(True)
    unlabelled()
    t = eng.kernel_times()
    eng.profile(False)
    out.append('| %s | %s |' % (legs[1][0], ' | '.join('%.1f us / update (%d timed scopes)' % (1e3 * t[k][0] / n, t[k][1] // n)
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
