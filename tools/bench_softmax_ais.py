#!/usr/bin/env python
"""The price of AIS over softmax visible units (bm_rbm_groups_ais) beside the Bernoulli AIS (bm_rbm_ais) of the same
size, 1024 hidden units, in one process on one box:
  * 196 groups x 4 (V = 784): the fused route - per beta step n_gibbs_steps prop-ups, one score launch and n_gibbs_steps launches of
    the SM + SA flavour;
  * 157 groups x 5 (V = 785): the generic route - per beta step n_gibbs_steps prop-ups, one score launch, n_gibbs_steps logits
    passes, n_gibbs_steps launches of softmax_groups_kernel and one row-dot launch;
  * a Bernoulli RBM of 784 x 1024 through RbmEngine.ais: n_gibbs_steps prop-ups, one score launch, n_gibbs_steps prop-downs.

A call is timed whole by the host clock: it uploads the base logits and the temperatures, enqueues every launch and ends in the
download of the values behind a synchronise.  One handle per leg, the legs alternating after a warm-up call each (launch tuning,
code objects).  A second pass with the handles' per-class event timing on gives the kernel time of a call by class - prop-ups,
prop-downs (the fused pass, or the logits pass of the generic route) and `other`, which in these calls is exactly the generic
route's extra launches (softmax_groups_kernel and the row-dot kernel; the score launch is not in a class).  Event pairs around
every pass slow the host, so the whole-call times come from the first pass only.  No target and no assertion: the figures are the
record.  Prints a markdown report; --out writes it as well (meant for profiles/softmax_ais_bench.md).

    python tools/bench_softmax_ais.py [--runs 10] [--betas 1000] [--chains 512] [--k 1] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

H = 1024
LEGS = (('groups 196 x 4, fused route', 196, 4), ('groups 157 x 5, generic route', 157, 5), ('Bernoulli 784', 784, 0))


def handle(G, K, chains):
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    V = G * K if K else G
    e = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=min(chains, 512), v_groups=K)
    e.set('W', philox.tf_random_normal((V, H), 0.01, 1337))             # bench.py's weights
    return e


def launches(K, k):
    """launches per beta step (up, score, down)"""
    fused = K in (2, 4, 8, 16)
    return (k, 1, k if (K == 0 or fused) else 2 * k + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--betas', type=int, default=1000)
    ap.add_argument('--chains', type=int, default=512)
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    nb, R, k = args.betas, args.chains, args.k
    engines = {name: handle(G, K, R) for name, G, K in LEGS}
    call = {name: ((lambda e=engines[name]: e.groups_ais(nb, R, k, 7)) if K else (lambda e=engines[name]: e.ais(nb, R, k, 7)))
            for name, G, K in LEGS}
    for name in call:                                     # warm-up: tuning, code objects, workspaces
        assert np.all(np.isfinite(call[name]()))
    wall = {name: [] for name in call}
    for _ in range(args.runs):
        for name in call:
            t0 = time.perf_counter()
            call[name]()                                  # (ends in the download of the values behind a synchronise)
            wall[name].append(1e3 * (time.perf_counter() - t0))
    cls = {name: [] for name in call}
    for name, e in engines.items():
        e.profile(True)
        for _ in range(max(2, args.runs // 3)):
            t0 = e.kernel_times()
            call[name]()
            t1 = e.kernel_times()
            cls[name].append(tuple(t1[c][0] - t0[c][0] for c in ('act_up', 'act_down', 'other')))
        e.profile(False)
        e.close()
    fmt = lambda v: '%.2f (%.2f - %.2f)' % (float(np.median(v)), min(v), max(v))
    base = float(np.median(wall['Bernoulli 784']))
    steps = nb - 1
    out = ['| AIS call, %d betas x %d chains, n_gibbs_steps = %d, %d hidden | launches per beta step (up + score + down) | ms per call, host clock '
           '(median, min - max) | us per beta step | ratio to Bernoulli |' % (nb, R, k, H), '|---|---|---|---|---|']
    for name, G, K in LEGS:
        up, sc, dn = launches(K, k)
        med = float(np.median(wall[name]))
        out.append('| %s | %d + %d + %d = %d | %s | %.1f | %.3f |' % (name, up, sc, dn, up + sc + dn, fmt(wall[name]), 1e3 * med / steps, med / base))
    out += ['', '| kernel time of a call by class, event pairs (ms, median) | prop-ups | prop-downs (fused pass / logits pass) | other (softmax_groups_kernel + row-dot) |',
            '|---|---|---|---|']
    med_cls = {}
    for name, G, K in LEGS:
        med_cls[name] = tuple(float(np.median([c[i] for c in cls[name]])) for i in range(3))
        out.append('| %s | %.2f | %.2f | %.2f |' % ((name,) + med_cls[name]))
    f_name, g_name = LEGS[0][0], LEGS[1][0]
    gap = float(np.median(wall[g_name])) - float(np.median(wall[f_name]))
    extra = med_cls[g_name][2]
    out += ['', 'Generic minus fused, whole call: %.2f ms (%.1f us per beta step).  The generic route\'s extra launches (class `other`: %d per beta '
            'step) take %.2f ms of kernel time per call (%.1f us per beta step); its logits pass takes %.2f ms where the fused pass takes %.2f ms.'
            % (gap, 1e3 * gap / steps, k + 1, extra, 1e3 * extra / steps, med_cls[g_name][1], med_cls[f_name][1]),
            '', '%d runs per leg, one handle per leg, the legs alternating after a warm-up call each; whole-call times by the host clock around calls '
            'that end in a synchronise, taken with the per-class event timing off; bench.py\'s weights, the uniform base.  No speed target is set.'
            % args.runs]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
