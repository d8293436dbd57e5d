#!/usr/bin/env python
"""The price of AIS per document length over replicated softmax visible units (bm_rbm_rsm_ais) beside the Bernoulli
AIS (bm_rbm_ais) of the same V, H, rows and betas, in one process on one box:
  * replicated softmax: `--lengths` distinct lengths spread over [--dmin, --dmax] x `--chains` chains each, ONE run - per beta step
    n_gibbs_steps tempered DB prop-ups, one score launch and n_gibbs_steps (logits pass, AIS flavour of multinomial_counts_kernel) pairs;
  * a Bernoulli RBM of the same size through RbmEngine.ais: n_gibbs_steps prop-ups, one score launch, n_gibbs_steps prop-downs.

A call is timed whole by the host clock: it uploads the base logits, the temperatures and the lengths, enqueues every launch and ends
in the download of the values behind a synchronise.  One handle per leg, the legs alternating after a warm-up call each (launch
tuning, code objects, workspaces).  A second pass with the handles' per-class event timing on gives the kernel time of a call by
class - prop-ups, prop-downs (the logits pass / the Bernoulli prop-down) and `other`, which in the replicated-softmax call is exactly
the count kernel (and the one fill of the start); the score launch is in no class.  Event pairs around every pass slow the host, so
the whole-call times come from the first pass only.  No target and no assertion: the figures are the record.  Prints a markdown
report; --out writes it as well (meant for profiles/rsm_ais_bench.md).

    python tools/bench_rsm_ais.py [--runs 5] [--betas 1000] [--lengths 100] [--chains 100] [--k 1] [--V 2000] [--H 256] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def handle(V, H, max_length):
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    e = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=512, rsm_max_length=max_length)
    e.set('W', philox.tf_random_normal((V, H), 0.01, 1337))             # bench.py's weights
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--betas', type=int, default=1000)
    ap.add_argument('--lengths', type=int, default=100)
    ap.add_argument('--chains', type=int, default=100)
    ap.add_argument('--dmin', type=int, default=10)
    ap.add_argument('--dmax', type=int, default=1000)
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--V', type=int, default=2000)
    ap.add_argument('--H', type=int, default=256)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    nb, k, V, H = args.betas, args.k, args.V, args.H
    D = np.repeat(np.round(np.linspace(args.dmin, args.dmax, args.lengths)), args.chains).astype(np.float32)
    R = len(D)
    legs = ('replicated softmax', 'Bernoulli')
    engines = {'replicated softmax': handle(V, H, args.dmax), 'Bernoulli': handle(V, H, 0)}
    call = {'replicated softmax': lambda: engines['replicated softmax'].rsm_ais(nb, D, k, 7),
            'Bernoulli': lambda: engines['Bernoulli'].ais(nb, R, k, 7)}
    for name in legs:                                     # warm-up: tuning, code objects, workspaces
        assert np.all(np.isfinite(call[name]()))
    wall = {name: [] for name in legs}
    for _ in range(args.runs):
        for name in legs:
            t0 = time.perf_counter()
            call[name]()                                  # (ends in the download of the values behind a synchronise)
            wall[name].append(1e3 * (time.perf_counter() - t0))
    cls = {name: [] for name in legs}
    for name in legs:
        e = engines[name]
        e.profile(True)
        for _ in range(2):
            t0 = e.kernel_times()
            call[name]()
            t1 = e.kernel_times()
            cls[name].append(tuple(t1[c][0] - t0[c][0] for c in ('act_up', 'act_down', 'other')))
        e.profile(False)
        e.close()
    fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
    base = float(np.median(wall['Bernoulli']))
    steps = nb - 1
    out = ['| AIS call, %d betas x %d rows, n_gibbs_steps = %d, V = %d, H = %d | launches per beta step | ms per call, host clock (median, '
           'min - max) | us per beta step | ratio to Bernoulli |' % (nb, R, k, V, H), '|---|---|---|---|---|']
    for name, n_launch in (('replicated softmax', '%d + 1 + %d = %d' % (k, 2 * k, 3 * k + 1)), ('Bernoulli', '%d + 1 + %d = %d' % (k, k, 2 * k + 1))):
        med = float(np.median(wall[name]))
        out.append('| %s | %s | %s | %.1f | %.3f |' % (name, n_launch, fmt(wall[name]), 1e3 * med / steps, med / base))
    out += ['', '| kernel time of a call by class, event pairs (ms, median) | prop-ups | prop-downs (logits pass / Bernoulli prop-down) | other '
            '(multinomial_counts_kernel, AIS flavour) |', '|---|---|---|---|']
    med_cls = {}
    for name in legs:
        med_cls[name] = tuple(float(np.median([c[i] for c in cls[name]])) for i in range(3))
        out.append('| %s | %.1f | %.1f | %.1f |' % ((name,) + med_cls[name]))
    cnt = med_cls['replicated softmax'][2]
    out += ['', 'The replicated-softmax run holds %d distinct lengths from %d to %d tokens (mean %.0f), %d chains each, in one call.  Its count '
            'kernel takes %.1f ms of kernel time per call: %.1f us per launch of %d workgroups (one per row), %.1f ns per row with the chip '
            'full of rows.  A row alone is bound by the latency of its chain of dependent steps (the prefix levels, the bisections; DESIGN.md '
            '3.27); with this many rows the workgroups that are resident together hide each other\'s latency.'
            % (args.lengths, args.dmin, args.dmax, float(D.mean()), args.chains, cnt, 1e3 * cnt / (steps * k), R, 1e6 * cnt / (steps * k * R)),
            '', '%d runs per leg, one handle per leg, the legs alternating after a warm-up call each; whole-call times by the host clock around '
            'calls that end in a synchronise, taken with the per-class event timing off; bench.py\'s weights, the uniform base.  No speed target is '
            'set.' % args.runs]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
