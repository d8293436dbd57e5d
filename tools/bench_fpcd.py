#!/usr/bin/env python
"""The price of fast-weights PCD, at 784 x 1024, batch 512, k = 1, M = 512 chains, R in {1, 10} temperatures.

In ONE process, after a warm-up call of every case (launch tuning, code objects):

  a. an update with fast weights (bm_rbm_set_fast_weights on) against the plain tempered update, both through the native loop
     bm_rbm_train_epoch_pt, alternating, --runs times each; HIP-event time on the engine's stream around --updates updates
  b. the fast-weights flavour of grad_kernel against the plain one: bm_rbm_profile's per-class event times of the same updates
     (class `grad`; the per-pass events serialise the stream, so these are kernel times, not the update's)
  c. the refresh of the effective copies (fast_refresh_kernel + the transpose for We^T): profile class `other` of updates that
     each follow a device-side rewrite of vb, which leaves the copies stale

Prints a markdown report; --out writes it as well (meant for the measured section of profiles/fpcd_bench.md).

    python tools/bench_fpcd.py [--runs 7] [--updates 20] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H, B, M, K = 784, 1024, 512, 512, 1
TEMPS = (1, 10)
FAST_LR, FAST_DECAY = 0.05, 0.95


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=20)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    n = args.updates
    X = (philox.uniform(87654321, 42, 0, n * B * V).reshape(n * B, V) < 0.1307).astype(np.float32)      # bench.py's density
    Xd = DeviceArray.from_numpy(X)
    W = philox.tf_random_normal((V, H), 0.01, 1337)                                                      # bench.py's weights

    def engine(R, fast):
        eng = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5)
        eng.set('W', W)
        eng.seed(1)
        if fast:
            eng.set_fast_weights(True, FAST_LR, FAST_DECAY)
        eng.pt_init(M, np.linspace(0., 1., R + 1)[1:].astype(np.float32))
        return eng
    cases = [('%s, R = %d' % ('fast weights' if fast else 'plain', R), R, fast, engine(R, fast)) for R in TEMPS for fast in (False, True)]
    epoch = lambda e: e.train_epoch_pt(Xd, n * B, B, 0.05, 0.9, K)
    for _, _, _, eng in cases:
        epoch(eng)
        eng.sync()
    # a. whole updates
    us = {name: [] for name, _, _, _ in cases}
    for _ in range(args.runs):                                  # alternating: a drift of the box hits every case
        for name, _, _, eng in cases:
            eng.timer_start()
            epoch(eng)
            us[name].append(1e3 * eng.timer_stop() / n)
    # b. the grad launch alone
    grad = {}
    for name, _, _, eng in cases:
        eng.profile(True)
        epoch(eng)
        eng.sync()
        ms, cnt = eng.kernel_times()['grad']
        grad[name] = (1e3 * ms / max(cnt, 1), cnt)
        eng.profile(False)
    # c. the refresh
    refresh = {}
    vb = DeviceArray.from_numpy(np.zeros(V, np.float32))
    for name, R, fast, eng in cases:
        if not fast:
            continue
        eng.profile(True)
        for u in range(n):
            eng.set_from_device('vb', vb)                       # (stream order, no host wait: the effective copies are stale)
            eng.train_step_pt(Xd, B, 0.05, 0.9, K, row=u * B)
        eng.sync()
        ms, cnt = eng.kernel_times()['other']
        refresh[name] = (1e3 * ms / max(cnt, 1), cnt)
        eng.profile(False)
    for _, _, _, eng in cases:
        eng.close()

    med = lambda t: float(np.median(t))
    each = lambda t: ', '.join('%.1f' % x for x in t)
    spread = lambda t: (max(t) - min(t)) / med(t)
    lines = [
        '## Measured (`tools/bench_fpcd.py`)',
        '',
        'One MI355X; %d x %d, batch %d, k = %d, M = %d chains, fast_learning_rate %g, fast_decay %g; every call %d updates through'
        % (V, H, B, K, M, FAST_LR, FAST_DECAY, n),
        'the native loop, one warm-up, then %d timed runs, the cases alternating; HIP-event time on the engine stream.' % args.runs,
        '',
        '| case | us per update (each run) | median us | (max - min) / median |',
        '|---|---|---|---|',
    ] + ['| %s | %s | %.1f | %.3f |' % (name, each(us[name]), med(us[name]), spread(us[name])) for name, _, _, _ in cases] + ['']
    for R in TEMPS:
        a, b = med(us['fast weights, R = %d' % R]), med(us['plain, R = %d' % R])
        lines.append('* R = %d: update with fast weights %.1f us, plain tempered update %.1f us (%+.1f us, ratio %.3f)' % (R, a, b, a - b, a / b))
    lines += ['', '`grad_kernel` alone (profile class `grad`, event time per launch, %d launches each):' % n, '']
    for R in TEMPS:
        a, b = grad['fast weights, R = %d' % R], grad['plain, R = %d' % R]
        lines.append('* R = %d: fast-weights flavour %.1f us, plain %.1f us (%+.1f us, ratio %.3f)' % (R, a[0], b[0], a[0] - b[0], a[0] / b[0]))
    lines += ['', 'Refresh of the effective copies (profile class `other`: `fast_refresh_kernel` + `transpose_kernel`, event time per refresh):', '']
    for name in sorted(refresh):
        lines.append('* %s: %.1f us (%d refreshes)' % (name, refresh[name][0], refresh[name][1]))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
