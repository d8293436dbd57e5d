#!/usr/bin/env python
"""The price of parallel tempering over Gaussian visible units (bm_rbm_gauss_pt_sweep) at one shape - 784 visible, 1024
hidden units, an ensemble of `--chains` chains x `--temps` temperatures - two comparisons:
  1. a tempered step of this unit (RT prop-up, swap, the RT + GT prop-down) beside the Bernoulli tempered step (bm_rbm_pt_sweep of a
     784 x 1024 handle: RT prop-up, swap, RT prop-down) on the same number of rows;
  2. the fused prop-down (RT + GT: the row's standard deviation, the -1/2 (s - c)^2 partials from registers) beside the generic route
     (a raw pass and the row kernel) at the SAME shape: BM355_DEBUG=gt_fused=0 is read once per process, so this leg runs in a child
     process of its own.

A sweep is timed whole by the host clock around a synchronise (one handle per leg, a warm-up sweep each: launch tuning, code
objects), the legs of this process alternating; a second pass with the handle's per-class event timing on gives the kernel time of
a step by class - prop-ups, prop-downs (the fused pass, or the raw pass of the generic route) and `other`, which here is exactly the
generic route's row kernel (the swap launch is in no class).  No target and no assertion: the figures are the record.
Prints a markdown report; --out writes it as well (meant for profiles/gauss_pt_bench.md).  Without a GPU the report says that no
run was made.

    python tools/bench_gauss_pt.py [--runs 10] [--steps 50] [--chains 512] [--temps 10] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H = 784, 1024
FUSED, BERN, GENERIC = 'Gaussian 784, fused route', 'Bernoulli 784', 'Gaussian 784, generic route (gt_fused=0, own process)'


def ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(np.float32)


def handle(gaussian, rows):
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    e = RbmEngine(V, H, v_unit=_ffi.UNIT_GAUSSIAN if gaussian else _ffi.UNIT_BERNOULLI, sample_v_states=True, sample_h_states=True,
                  max_batch=64)
    e.set('W', philox.tf_random_normal((V, H), 0.01, 1337))             # bench.py's weights
    if gaussian:
        e.set('sigma', (0.5 + philox.uniform(2468, 77, 0, V)).astype(np.float32))
    e.seed(7)
    return e


def time_sweeps(legs, runs, steps):
    """{name: [us per step]} by the host clock, the legs alternating; {name: (up, down, other) us per step} by event pairs"""
    for e, pt in legs.values():
        pt.pt_sweep(steps)
        e.sync()
    wall = {n: [] for n in legs}
    for _ in range(runs):
        for n, (e, pt) in legs.items():
            t0 = time.perf_counter()
            pt.pt_sweep(steps)
            e.sync()
            wall[n].append(1e6 * (time.perf_counter() - t0) / steps)
    cls = {}
    for n, (e, pt) in legs.items():
        e.profile(True)
        rec = []
        for _ in range(max(2, runs // 3)):
            t0 = e.kernel_times()
            pt.pt_sweep(steps)
            e.sync()
            t1 = e.kernel_times()
            rec.append(tuple(1e3 * (t1[c][0] - t0[c][0]) / steps for c in ('act_up', 'act_down', 'other')))
        e.profile(False)
        cls[n] = tuple(float(np.median([r[i] for r in rec])) for i in range(3))
    return wall, cls


def generic_leg(args):
    """this process runs under BM355_DEBUG=gt_fused=0: the Gaussian handle takes the generic route"""
    e = handle(True, args.chains * args.temps)
    e.gauss_pt.pt_init(args.chains, ladder(args.temps))
    wall, cls = time_sweeps({'generic': (e, e.gauss_pt)}, args.runs, args.steps)
    print('GAUSS_PT_GENERIC ' + json.dumps(dict(wall=wall['generic'], cls=cls['generic'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--chains', type=int, default=512)
    ap.add_argument('--temps', type=int, default=10)
    ap.add_argument('--out', default=None, help='write the report here as well')
    ap.add_argument('--generic-leg', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.generic_leg:
        return generic_leg(args)
    from boltzmann_machines_amd import _ffi
    rows = args.chains * args.temps
    head = ('# Parallel tempering over Gaussian visible units: what a step costs\n\n`tools/bench_gauss_pt.py`: %d visible, %d hidden units, '
            '%d chains x %d temperatures = %d rows, %d steps per sweep.\n' % (V, H, args.chains, args.temps, rows, args.steps))
    if _ffi.load().bm_device_count() <= 0:
        text = head + '\nNo GPU run of the tool has been made: nothing here has been measured and no speed is promised.\n'
    else:
        eg, eb = handle(True, rows), handle(False, rows)
        eg.gauss_pt.pt_init(args.chains, ladder(args.temps))
        eb.pt_init(args.chains, ladder(args.temps))
        wall, cls = time_sweeps({FUSED: (eg, eg.gauss_pt), BERN: (eb, eb)}, args.runs, args.steps)
        eg.close()
        eb.close()
        env = dict(os.environ, BM355_DEBUG='gt_fused=0')
        cmd = [sys.executable, os.path.abspath(__file__), '--generic-leg', '--runs', str(args.runs), '--steps', str(args.steps),
               '--chains', str(args.chains), '--temps', str(args.temps)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0 or 'GAUSS_PT_GENERIC' not in r.stdout:
            raise SystemExit('the generic leg failed:\n' + r.stdout[-2000:] + r.stderr[-4000:])
        gen = json.loads(r.stdout.split('GAUSS_PT_GENERIC', 1)[1].strip().splitlines()[0])
        wall[GENERIC] = gen['wall']
        cls[GENERIC] = tuple(gen['cls'])
        fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
        base = float(np.median(wall[BERN]))
        out = [head, '| tempered step | us per step, host clock (median, min - max) | ratio to Bernoulli | kernel us per step: prop-up | prop-down '
               '(fused pass / raw pass) | other (row kernel) |', '|---|---|---|---|---|---|']
        for n in wall:
            out.append('| %s | %s | %.3f | %.1f | %.1f | %.1f |' % ((n, fmt(wall[n]), float(np.median(wall[n])) / base) + cls[n]))
        out += ['', '| prop-down on %d rows, kernel time by event pairs | us per launch |' % rows, '|---|---|',
                '| fused, RT + GT (row standard deviations, -1/2 (s - c)^2 partials from registers) | %.1f |' % cls[FUSED][1],
                '| Bernoulli RT prop-down (row temperatures, v.vb partials read back) | %.1f |' % cls[BERN][1],
                '| generic route: raw pass + row kernel | %.1f + %.1f = %.1f |' % (cls[GENERIC][1], cls[GENERIC][2], cls[GENERIC][1] + cls[GENERIC][2]),
                '', 'Fused / generic, whole step (medians): %.3f.' % (float(np.median(wall[FUSED])) / float(np.median(wall[GENERIC]))),
                '', '%d sweeps per leg after a warm-up sweep, the two in-process legs alternating; whole-sweep times by the host clock around a '
                'synchronise with the per-class event timing off, kernel times from a second pass with it on; bench.py\'s weights, sigma '
                'in [0.5, 1.5).  No speed target is set.' % args.runs]
        text = '\n'.join(out) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
