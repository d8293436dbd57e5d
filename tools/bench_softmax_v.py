#!/usr/bin/env python
"""The price of softmax visible units: one CD-1 update at 784 x 1024, batch 512, for
  * the Bernoulli handle (bench.py's density),
  * K = 4 (196 groups): the SM flavour of the prop-down, one launch,
  * K = 7 (112 groups): the logits pass + softmax_groups_kernel, one more launch per prop-down,
  * K = 4 under BM355_DEBUG=sm_fused=0 (the generic pair at a fused width), in a fresh child process of its own - the switch is
    read once per process - beside a Bernoulli handle of that process,
the grouped handles on one-hot rows.

One handle per leg, the legs alternating after a warm-up call each (launch tuning, code objects).  Times are HIP-event times on
the engine's stream around `--updates` updates that only enqueue (bm_rbm_train_epoch); `--runs` samples per leg.  No target and no
assertion: the ratios to the Bernoulli update of the same build on the same box are the record.  Prints a markdown report; --out
writes it as well (meant for profiles/softmax_v_bench.md).

    python tools/bench_softmax_v.py [--runs 10] [--updates 48] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H, B, LR = 784, 1024, 512, 0.01


def measure(widths, runs, updates):
    """{leg: [us per update] * runs} for one handle per entry of `widths` (0: Bernoulli), alternating"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    n_rows = 4 * B                                              # the updates cycle over four batches
    W = philox.tf_random_normal((V, H), 0.01, 1337)             # bench.py's weights
    engs, data = {}, {}
    for K in widths:
        if K:
            cats = np.random.RandomState(K).randint(0, K, (n_rows, V // K))
            X = (cats[:, :, None] == np.arange(K)[None, None, :]).astype(np.float32).reshape(n_rows, V)
        else:
            X = (philox.uniform(87654321, 42, 0, n_rows * V).reshape(n_rows, V) < 0.1307).astype(np.float32)      # bench.py's density
        e = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5, v_groups=K)
        e.set('W', W)
        e.seed(1)
        engs[K], data[K] = e, DeviceArray.from_numpy(X)

    def update(K):
        for _ in range(updates // 4):
            engs[K].train_epoch(data[K], n_rows, B, LR, 0.9, 1)
    for K in widths:
        update(K)
        engs[K].sync()
    us = {K: [] for K in widths}
    for _ in range(runs):
        for K in widths:
            engs[K].timer_start()
            update(K)
            us[K].append(1e3 * engs[K].timer_stop() / (4 * (updates // 4)))
    for e in engs.values():
        e.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--updates', type=int, default=48)
    ap.add_argument('--out', default=None, help='write the report here as well')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:              # the sm_fused=0 leg: Bernoulli and K = 4 of THIS process
        us = measure([0, 4], args.runs, args.updates)
        print('SOFTMAX_V_CHILD ' + json.dumps({str(k): v for k, v in us.items()}))
        return
    us = measure([0, 4, 7], args.runs, args.updates)
    env = dict(os.environ, BM355_DEBUG='sm_fused=0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--runs', str(args.runs), '--updates', str(args.updates)],
                       env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 or 'SOFTMAX_V_CHILD' not in r.stdout:
        raise SystemExit('the sm_fused=0 child failed:\n' + r.stdout[-2000:] + r.stderr[-4000:])
    child = {int(k): v for k, v in json.loads(r.stdout.split('SOFTMAX_V_CHILD', 1)[1]).items()}
    fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
    ratio = lambda v, base: '%.3f' % (float(np.median(v)) / float(np.median(base)))
    out = ['| leg | process | us per CD-1 update (median, min - max) | ratio to the Bernoulli update of the same process |', '|---|---|---|---|',
           '| Bernoulli visible units | main | %s | 1 |' % fmt(us[0]),
           '| K = 4, fused (SM flavour) | main | %s | %s |' % (fmt(us[4]), ratio(us[4], us[0])),
           '| K = 7, generic (logits + softmax_groups_kernel) | main | %s | %s |' % (fmt(us[7]), ratio(us[7], us[0])),
           '| Bernoulli visible units | child, sm_fused=0 | %s | 1 |' % fmt(child[0]),
           '| K = 4, generic (sm_fused=0) | child, sm_fused=0 | %s | %s |' % (fmt(child[4]), ratio(child[4], child[0])),
           '', '%d runs per leg of %d updates at %d x %d, batch %d, the legs of a process alternating (one handle each), HIP-event times per '
           'update; one-hot rows for the grouped handles, bench.py\'s density for the Bernoulli one; visible and hidden states sampled.  The '
           'Bernoulli update runs its chain as the handle runs it by default (one chained launch where the shape allows it); a handle with '
           'softmax visible units issues per-pass launches.  No speed target is set.' % (args.runs, 4 * (args.updates // 4), V, H, B)]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
