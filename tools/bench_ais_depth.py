#!/usr/bin/env python
"""One full AIS run (DbmEngine.ais: 20 000 chains x 1000 betas, k = 1 - the configs[4] setting) at three depths:
784-512 (L = 1, the MNIST RBM as a one-layer DBM), 784-512-1024 (L = 2, the control: bench.py --config ais) and
784-512-1024-512 (L = 3).  One JSON line per model: ms per run (median of --runs after one warm-up run) and the
fraction of the fp32-MFMA roof, with flops per run = 4 k R n_betas sum_l n_l n_{l+1} (bench.py's formula at L = 2).

    python tools/bench_ais_depth.py [--runs 3] [--betas 1000] [--chains 20000] [--k 1] [--only L]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

PEAK_FP32_MFMA = 157.3          # TFLOP/s, MI355X (bench.py)
MODELS = {1: [784, 512], 2: [784, 512, 1024], 3: [784, 512, 1024, 512]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--betas', type=int, default=1000)
    ap.add_argument('--chains', type=int, default=20000)
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--only', type=int, default=0, help='one depth only (1, 2 or 3)')
    args = ap.parse_args()
    from boltzmann_machines_amd.engine import DbmEngine
    from boltzmann_machines_amd.utils import log_mean_exp, philox
    for L, n in sorted(MODELS.items()):
        if args.only and L != args.only:
            continue
        eng = DbmEngine(n[0], n[1:], n_particles=8, batch_size=8)
        for i in range(L):                       # bench.py's weights for the first two layers
            sfx = '' if i == 0 else '_%d' % i
            eng.set('W' + sfx, philox.tf_random_normal((n[i], n[i + 1]), 0.01, (1337, 1111, 2222)[i]))
        R, nb, k = args.chains, args.betas, args.k
        vals = eng.ais(nb, R, k, 2222)                                       # warm-up: launch tuning of the shapes
        times = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            vals = eng.ais(nb, R, k, 2222)                                   # one host synchronisation, at the end
            times.append(time.perf_counter() - t0)
        eng.close()
        ms = float(np.median(times)) * 1e3
        flops = 4.0 * k * R * nb * sum(n[l] * n[l + 1] for l in range(L))
        tf = flops / (ms * 1e-3) / 1e12
        print(json.dumps({'model': '-'.join(map(str, n)), 'n_layers': L, 'chains': R, 'betas': nb, 'k': k,
                          'ms_per_run': round(ms, 2), 'ms_runs': [round(t * 1e3, 2) for t in times],
                          'tflops': round(tf, 2), 'fraction_of_fp32_mfma_roof': round(tf / PEAK_FP32_MFMA, 3),
                          'log_Z': round(float(log_mean_exp(vals)), 4), 'finite': bool(np.all(np.isfinite(vals)))}),
              flush=True)


if __name__ == '__main__':
    main()
