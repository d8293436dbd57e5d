#!/usr/bin/env python
"""The price of fine-tuning a stack below the class head: one back-propagation update of 784-512-1024, C = 10,
batch 512 - one layer below the top - beside the same top handle's head-only update (`bm_rbm_class_train_step` on fixed
512-wide features).

ONE process, the two legs alternating after a warm-up call each (launch tuning, code objects).  Times are HIP-event times around
`--updates` calls that only enqueue (the epoch entries without out2), `--runs` samples per leg.  The stack's events sit on the
bottom layer's stream: an update starts there and its closing hand-over ends there, so the pair brackets every launch of every
handle.  The per-launch times come from bm_rbm_profile of each handle over `--updates` updates: of the top, `act_up` is the
class-rows prop-up, `other` class_row_kernel and stack_g_kernel together, `colsum` class_hidden_kernel, `act_down` the BP
pass, `bias` class_head_update_kernel, `grad` the outer-product launch with its bias tail; of the layer below, `act_up` is its
prop-up and `grad` its update (the zero fill of hneg in front of it is a memset, not an event class).  Prints a markdown report;
--out writes it as well (meant for profiles/stack_finetune_bench.md).

    python tools/bench_stack_finetune.py [--runs 20] [--updates 50] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H1, H2, C, B = 784, 512, 1024, 10, 512
CLASSES = ('act_up', 'other', 'colsum', 'act_down', 'bias', 'grad')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--updates', type=int, default=50)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine, StackEngine
    from boltzmann_machines_amd.utils import philox
    n = args.updates
    X = philox.uniform(87654321, 42, 0, n * B * V).reshape(n * B, V).astype(np.float32)
    F = philox.uniform(87654321, 43, 0, n * B * H1).reshape(n * B, H1).astype(np.float32)           # the head-only leg's features
    rng = np.random.RandomState(7)
    yd = DeviceArray.from_numpy(rng.randint(0, C, n * B).astype(np.int32), np.int32)
    Xd, Fd = DeviceArray.from_numpy(X), DeviceArray.from_numpy(F)

    def top():
        e = RbmEngine(H1, H2, max_batch=B, l2=1e-5)
        e.set('W', philox.tf_random_normal((H1, H2), 0.01, 1338))
        e.set_classes(C)
        e.set('U', (rng.randn(C, H2) * 0.01).astype(np.float32))
        return e

    low = RbmEngine(V, H1, max_batch=B, l2=1e-5)
    low.set('W', philox.tf_random_normal((V, H1), 0.01, 1337))
    stack, head = StackEngine([low, top()]), top()
    legs = [('stack update 784-512-1024', low, lambda: stack.train_epoch(Xd, yd, n * B, B, [0.01, 0.05], 0.9, fetch=False), stack.sync),
            ('head-only update 512-1024', head, lambda: head.class_train_epoch(Fd, yd, n * B, B, 0.05, 0.9, fetch=False), head.sync)]
    for _, _, call, sync in legs:
        call()
        sync()
    us = {name: [] for name, _, _, _ in legs}
    for _ in range(args.runs):
        for name, timer, call, sync in legs:
            timer.timer_start()
            call()
            us[name].append(1e3 * timer.timer_stop() / n)
            sync()
    fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
    out = ['| leg | us / update (median, min - max) |', '|---|---|']
    for name, _, _, _ in legs:
        out.append('| %s | %s |' % (name, fmt(us[name])))
    out += ['', '%d runs of %d updates per leg, alternating in one process, HIP-event times; C = %d, batch %d.' % (args.runs, n, C, B), '',
            '| handle | ' + ' | '.join(CLASSES) + ' |', '|---|' + '---|' * len(CLASSES)]
    rows = [('stack: layer below (784 x 512)', low, legs[0]), ('stack: top (512 x 1024)', stack.top, legs[0]),
            ('head-only: top (512 x 1024)', head, legs[1])]
    for e in (low, stack.top, head):
        e.profile(True)
    for _, _, call, sync in legs:
        call()
        sync()
    for label, e, _ in rows:
        t = e.kernel_times()
        out.append('| %s | %s |' % (label, ' | '.join('%.1f us / update, %d launches' % (1e3 * t[k][0] / n, t[k][1]) if t[k][1] else '-'
                                                       for k in CLASSES)))
    for e in (low, stack.top, head):
        e.profile(False)
    out += ['', 'Per handle and event class: the HIP-event time of the class summed over %d profiled updates, per update, and the number '
            'of launches in it (bm_rbm_profile: an event pair per launch, which keeps the launches from overlapping).  The zero operand of '
            'the layer update is a memset of %d rows per update; a single-product form of grad_kernel was not built, so there is no '
            'difference between the two to report.' % (n, B)]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
