#!/usr/bin/env python
"""RbmEngine.ais against the only existing code doing comparable work, DbmEngine(V, [H]).ais (the one-layer DBM run issues
the same two GEMM passes per beta step): 784 x 1024, 20 000 chains x 1000 betas, k = 1, each timed --runs times after one
warm-up run (launch tuning of the shapes).  Prints a markdown report (meant for profiles/rbm_ais_bench.md): the times, their
ratio, the spread of the DBM runs (the noise floor) and the achieved fraction of the fp32-MFMA roof with the flop count of
DESIGN.md 3.7, 4 k R n_betas V H per run.

    python tools/bench_rbm_ais.py [--runs 3] [--betas 1000] [--chains 20000] [--k 1] [--out FILE]
    BM355_DEBUG=act_geo=8 rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- \\
        python tools/bench_rbm_ais.py --trace-run --betas 50      # ONE RbmEngine.ais call, no tuning launches: the launch budget"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

PEAK_FP32_MFMA = 157.3          # TFLOP/s, MI355X (bench.py)
V, H = 784, 1024


def timed(f, runs):
    f()                                              # warm-up: launch tuning of the shapes
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        vals = f()                                   # one host synchronisation, at the end
        out.append(time.perf_counter() - t0)
    return out, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--betas', type=int, default=1000)
    ap.add_argument('--chains', type=int, default=20000)
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--out', default=None, help='write the report here as well')
    ap.add_argument('--trace-run', action='store_true', help='one RbmEngine.ais call and nothing else (for rocprofv3)')
    args = ap.parse_args()
    from boltzmann_machines_amd.engine import DbmEngine, RbmEngine
    from boltzmann_machines_amd.utils import log_mean_exp, philox
    R, nb, k = args.chains, args.betas, args.k
    W = philox.tf_random_normal((V, H), 0.01, 1337)                          # bench.py's weights
    rbm = RbmEngine(V, H, sample_v_states=True, max_batch=8)
    rbm.set('W', W)
    if args.trace_run:
        vals = rbm.ais(nb, R, k, 2222)
        rbm.close()
        print('one RbmEngine.ais call: %d chains x %d betas, k = %d, log Z %.4f' % (R, nb, k, float(log_mean_exp(vals))))
        return
    t_rbm, v_rbm = timed(lambda: rbm.ais(nb, R, k, 2222), args.runs)
    rbm.close()
    dbm = DbmEngine(V, [H], n_particles=8, batch_size=8)
    dbm.set('W', W)
    t_dbm, v_dbm = timed(lambda: dbm.ais(nb, R, k, 2222), args.runs)
    dbm.close()
    flops = 4.0 * k * R * nb * V * H
    frac = lambda t: flops / t / 1e12 / PEAK_FP32_MFMA
    m_rbm, m_dbm = float(np.median(t_rbm)), float(np.median(t_dbm))
    spread = (max(t_dbm) - min(t_dbm)) / m_dbm
    ms = lambda ts: ', '.join('%.2f' % (t * 1e3) for t in ts)
    lines = [
        '# RBM AIS against the one-layer DBM AIS (`tools/bench_rbm_ais.py`)',
        '',
        '%d x %d, %d chains x %d betas, k = %d, one MI355X, one session; each engine: one warm-up run, then %d timed runs'
        % (V, H, R, nb, k, args.runs),
        '(wall clock around the call, one host synchronisation at its end).',
        '',
        '| engine | ms per run (each) | median ms | fraction of the fp32-MFMA roof (median) | log Z estimate |',
        '|---|---|---|---|---|',
        '| `RbmEngine.ais` (uniform base) | %s | %.2f | %.3f | %.4f |' % (ms(t_rbm), m_rbm * 1e3, frac(m_rbm), float(log_mean_exp(v_rbm))),
        '| `DbmEngine(%d, [%d]).ais` | %s | %.2f | %.3f | %.4f |' % (V, H, ms(t_dbm), m_dbm * 1e3, frac(m_dbm), float(log_mean_exp(v_dbm))),
        '',
        'Ratio RBM / DBM (medians): %.4f.  Spread of the DBM runs, (max - min) / median - the noise floor: %.4f.' % (m_rbm / m_dbm, spread),
        'Flops per run: 4 k R n_betas V H = %.3e (DESIGN.md 3.7).  The two runs estimate different quantities (the DBM' % flops,
        'composition halves the hidden bias; with zero biases, as here, the distributions coincide).',
    ]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
