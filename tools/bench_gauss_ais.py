#!/usr/bin/env python
"""RbmEngine.gauss_ais (bm_rbm_gauss_ais) beside RbmEngine.ais, the Bernoulli run that issues the same two GEMM
passes per beta step through the same host loop: 784 x 1024, `--chains` chains x `--betas` betas, k = 1, each timed --runs times
after one warm-up run (launch tuning of the shapes), the two engines alternating.  What differs per beta step is the epilogue of the
prop-down (a Box-Muller draw per output where the Bernoulli pass compares a uniform with a sigmoid) and the start kernel.  Prints a
markdown report (meant for profiles/gauss_ais_bench.md): the times, their ratio and the spread of the Bernoulli runs (the noise
floor).  No target and no assertion.  Without a GPU the report says that no run was made.

    python tools/bench_gauss_ais.py [--runs 3] [--betas 1000] [--chains 20000] [--k 1] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

V, H = 784, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--betas', type=int, default=1000)
    ap.add_argument('--chains', type=int, default=20000)
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import log_mean_exp, philox
    R, nb, k = args.chains, args.betas, args.k
    head = ('# Gaussian AIS against the Bernoulli AIS (`tools/bench_gauss_ais.py`)\n\n%d x %d, %d chains x %d betas, k = %d, one MI355X, one '
            'session.\n' % (V, H, R, nb, k))
    if _ffi.load().bm_device_count() <= 0:
        text = head + '\nNo GPU run of the tool has been made: nothing here has been measured and no speed is promised.\n'
    else:
        W = philox.tf_random_normal((V, H), 0.01, 1337)                          # bench.py's weights
        g = RbmEngine(V, H, v_unit=_ffi.UNIT_GAUSSIAN, sample_v_states=True, max_batch=8)
        g.set('W', W)
        g.set('sigma', (0.5 + philox.uniform(2468, 77, 0, V)).astype(np.float32))
        b = RbmEngine(V, H, sample_v_states=True, max_batch=8)
        b.set('W', W)
        legs = {'gauss': lambda: g.gauss_ais(nb, R, k, 2222), 'bern': lambda: b.ais(nb, R, k, 2222)}
        vals, t = {}, {n: [] for n in legs}
        for n, f in legs.items():
            f()                                              # warm-up: launch tuning of the shapes
        for _ in range(args.runs):
            for n, f in legs.items():
                t0 = time.perf_counter()
                vals[n] = f()                                # one host synchronisation, at the end
                t[n].append(time.perf_counter() - t0)
        g.close()
        b.close()
        m = {n: float(np.median(t[n])) for n in t}
        spread = (max(t['bern']) - min(t['bern'])) / m['bern']
        ms = lambda ts: ', '.join('%.2f' % (x * 1e3) for x in ts)
        lines = [head, 'Each engine: one warm-up run, then %d timed runs, the two alternating (wall clock around the call, one host '
                 'synchronisation at its end).' % args.runs, '',
                 '| engine | ms per run (each) | median ms | us per beta step | log Z estimate |', '|---|---|---|---|---|',
                 '| `RbmEngine.gauss_ais` (a = 0, sigma in [0.5, 1.5)) | %s | %.2f | %.1f | %.4f |'
                 % (ms(t['gauss']), m['gauss'] * 1e3, m['gauss'] * 1e6 / (nb - 1), float(log_mean_exp(vals['gauss']))),
                 '| `RbmEngine.ais` (uniform base) | %s | %.2f | %.1f | %.4f |'
                 % (ms(t['bern']), m['bern'] * 1e3, m['bern'] * 1e6 / (nb - 1), float(log_mean_exp(vals['bern']))), '',
                 'Ratio Gaussian / Bernoulli (medians): %.4f.  Spread of the Bernoulli runs, (max - min) / median - the noise floor: %.4f.'
                 % (m['gauss'] / m['bern'], spread),
                 'The two runs estimate different quantities (different models); with these weights both stay near their base values.  '
                 'No speed target is set.']
        text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
