#!/usr/bin/env python
"""The price of replicated softmax visible units.

(a) One CD-1 update at a vocabulary of 2000, 256 hidden units, batch 512, document lengths mixed over 20 - 400, against the
    Bernoulli update of the same shape (bench.py's density).  One handle per leg, the legs alternating after a warm-up call each
    (launch tuning, code objects).  Times are HIP-event times on the engine's stream around `--updates` updates that only enqueue
    (bm_rbm_train_epoch); `--runs` samples per leg.
(b) multinomial_counts_kernel alone against softmax_multinomial_kernel alone - the Multinomial hidden layer's kernel, the only other
    one that turns a row of logits into counts - on the same 512 rows of logits at V = 2000 and 8192, M = 210 (the mean length):
    tools/bench_rsm_kernel.hip, built here with hipcc when the binary is missing or older than its sources.

No target and no assertion: the numbers are the record.  Prints a markdown report; --out writes it as well (meant for
profiles/rsm_bench.md).

    python tools/bench_rsm.py [--runs 10] [--updates 48] [--reps 50] [--out FILE]"""
import argparse
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H, B, LR, D_LO, D_HI = 2000, 256, 512, 0.01, 20, 400
KERNEL_SRC = os.path.join(ROOT, 'tools', 'bench_rsm_kernel.hip')
KERNEL_BIN = os.path.join(ROOT, 'tools', 'bench_rsm_kernel')


def build_kernel_bench():
    csrc = os.path.join(ROOT, 'boltzmann_machines_amd', 'csrc')
    deps = [KERNEL_SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if os.path.exists(KERNEL_BIN) and os.path.getmtime(KERNEL_BIN) >= max(os.path.getmtime(d) for d in deps):
        return KERNEL_BIN
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-mllvm', '-amdgpu-mfma-vgpr-form',
                           '-I', csrc, '-I', os.path.join(ROOT, 'include'), KERNEL_SRC, '-o', KERNEL_BIN])
    return KERNEL_BIN


def measure_updates(runs, updates):
    """{leg: [us per update] * runs} for a Bernoulli and a replicated-softmax handle, alternating"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    n_rows = 4 * B                                              # the updates cycle over four batches
    W = philox.tf_random_normal((V, H), 0.01, 1337)
    rng = np.random.RandomState(7)
    lengths = rng.randint(D_LO, D_HI + 1, n_rows)
    zipf = 1.0 / np.arange(1, V + 1)
    counts = np.stack([rng.multinomial(d, zipf / zipf.sum()) for d in lengths]).astype(np.float32)
    bits = (philox.uniform(87654321, 42, 0, n_rows * V).reshape(n_rows, V) < 0.1307).astype(np.float32)      # bench.py's density
    engs, data = {}, {}
    for leg, X, kw in (('bernoulli', bits, {}), ('rsm', counts, dict(rsm_max_length=D_HI))):
        e = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5, **kw)
        e.set('W', W)
        e.seed(1)
        engs[leg], data[leg] = e, DeviceArray.from_numpy(X)

    def update(leg):
        for _ in range(updates // 4):
            engs[leg].train_epoch(data[leg], n_rows, B, LR, 0.9, 1)
    for leg in engs:
        update(leg)
        engs[leg].sync()
    us = {leg: [] for leg in engs}
    for _ in range(runs):
        for leg in engs:
            engs[leg].timer_start()
            update(leg)
            us[leg].append(1e3 * engs[leg].timer_stop() / (4 * (updates // 4)))
    for e in engs.values():
        e.sync()
        e.close()
    return us, float(lengths.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--updates', type=int, default=48)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    exe = build_kernel_bench()
    us, mean_len = measure_updates(args.runs, args.updates)
    fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
    out = ['## (a) one CD-1 update, %d x %d, batch %d' % (V, H, B), '',
           '| leg | us per CD-1 update (median, min - max) | ratio to the Bernoulli update |', '|---|---|---|',
           '| Bernoulli visible units | %s | 1 |' % fmt(us['bernoulli']),
           '| replicated softmax, lengths %d - %d (mean %.0f) | %s | %.3f |'
           % (D_LO, D_HI, mean_len, fmt(us['rsm']), float(np.median(us['rsm'])) / float(np.median(us['bernoulli']))),
           '', '%d runs per leg of %d updates, the legs alternating (one handle each), HIP-event times per update; Zipf-distributed word '
           'counts for the replicated-softmax handle, bench.py\'s density for the Bernoulli one; visible and hidden states sampled.  The '
           'Bernoulli update runs its chain as the handle runs it by default (one chained launch where the shape allows it); a '
           'replicated-softmax handle issues per-pass launches: row_lengths_kernel, three act_kernel passes, multinomial_counts_kernel, '
           'rsm_bias_kernel, grad_kernel.' % (args.runs, 4 * (args.updates // 4)), '',
           '## (b) multinomial_counts_kernel against softmax_multinomial_kernel, each alone', '',
           '| V | rows | M | softmax_multinomial_kernel us (median, min) | multinomial_counts_kernel, every length = M | '
           'multinomial_counts_kernel, lengths 20 .. 2 M - 20 | old / new (medians, equal lengths) |', '|---|---|---|---|---|---|---|']
    for v in (2000, 8192):
        r = subprocess.run([exe, str(v), str(B), '210', str(args.reps)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit('bench_rsm_kernel failed:\n' + r.stdout[-2000:] + r.stderr[-4000:])
        k = json.loads(r.stdout.strip().splitlines()[-1])
        out.append('| %d | %d | %d | %.1f, %.1f | %.1f, %.1f | %.1f, %.1f | %.2f |'
                   % (k['V'], k['J'], k['M'], k['old_us'][0], k['old_us'][1], k['new_equal_us'][0], k['new_equal_us'][1],
                      k['new_mixed_us'][0], k['new_mixed_us'][1], k['old_us'][0] / k['new_equal_us'][0]))
    out += ['', '%d launches per leg behind five warm ones, one HIP event pair per launch, the logits (N(0, 3^2)) restored in front of '
            'every launch; the legs alternate.  softmax_multinomial_kernel runs one wave per row and forms its prefix sums in lane 0; '
            'multinomial_counts_kernel runs four waves per row and forms them in the hierarchy of csrc/bm_rsm.h.' % args.reps]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
