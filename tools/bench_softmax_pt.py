#!/usr/bin/env python
"""The price of parallel tempering over softmax visible units (bm_rbm_groups_pt_sweep) at one shape - 196 groups x 4
(V = 784), 1024 hidden units, an ensemble of `--chains` chains x `--temps` temperatures - three comparisons:
  1. a tempered step of this unit (RT prop-up, swap, the SM + SA + RT prop-down) beside the Bernoulli tempered step
     (bm_rbm_pt_sweep of a 784 x 1024 handle: RT prop-up, swap, RT prop-down) on the same number of rows;
  2. the fused prop-down (SM + SA + RT: a temperature per row, the v.vb partials) beside the plain SM pass (bm_rbm_sample_v_from_h)
     on the same number of rows;
  3. the fused prop-down beside the generic route (a raw pass, the tempered groups kernel, the row-dot kernel) at the SAME shape:
     BM355_DEBUG=sm_fused=0 is read once per process, so this leg runs in a child process of its own.

A sweep is timed whole by the host clock around a synchronise (one handle per leg, a warm-up sweep each: launch tuning, code
objects), the legs of this process alternating; a second pass with the handle's per-class event timing on gives the kernel time of
a step by class - prop-ups, prop-downs (the fused pass, or the raw pass of the generic route) and `other`, which here is exactly the
generic route's two extra launches (the swap launch is in no class).  No target and no assertion: the figures are the record.
Prints a markdown report; --out writes it as well (meant for profiles/softmax_pt_bench.md).  Without a GPU the report says that no
run was made.

    python tools/bench_softmax_pt.py [--runs 10] [--steps 50] [--chains 128] [--temps 8] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

G, K, H = 196, 4, 1024
V = G * K


def ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(np.float32)


def handle(groups, rows):
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    e = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=rows, v_groups=K if groups else 0)
    e.set('W', philox.tf_random_normal((V, H), 0.01, 1337))             # bench.py's weights
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


def plain_sm_pass(e, rows, runs, steps):
    """us per bm_rbm_sample_v_from_h call on `rows` rows (the plain SM pass), kernel time by event pairs"""
    from boltzmann_machines_amd._ffi import DeviceArray
    Hd = DeviceArray.from_numpy((np.random.RandomState(3).uniform(size=(rows, H)) < 0.5).astype(np.float32))
    Vd = DeviceArray((rows, V), np.float32)
    for _ in range(3):
        e.sample_v_from_h(Hd, rows, None, Vd)
    e.sync()
    e.profile(True)
    rec = []
    for _ in range(max(2, runs // 3)):
        t0 = e.kernel_times()
        for _ in range(steps):
            e.sample_v_from_h(Hd, rows, None, Vd)
        e.sync()
        t1 = e.kernel_times()
        rec.append(1e3 * (t1['act_down'][0] - t0['act_down'][0]) / steps)
    e.profile(False)
    return float(np.median(rec))


def generic_leg(args):
    """this process runs under BM355_DEBUG=sm_fused=0: the groups handle takes the generic route"""
    rows = args.chains * args.temps
    e = handle(True, rows)
    e.groups_pt.pt_init(args.chains, ladder(args.temps))
    wall, cls = time_sweeps({'generic': (e, e.groups_pt)}, args.runs, args.steps)
    print('SOFTMAX_PT_GENERIC ' + json.dumps(dict(wall=wall['generic'], cls=cls['generic'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--chains', type=int, default=128)
    ap.add_argument('--temps', type=int, default=8)
    ap.add_argument('--out', default=None, help='write the report here as well')
    ap.add_argument('--generic-leg', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.generic_leg:
        return generic_leg(args)
    from boltzmann_machines_amd import _ffi
    rows = args.chains * args.temps
    head = ('# Parallel tempering over softmax visible units: what a step costs\n\n`tools/bench_softmax_pt.py`: %d groups x %d (V = %d), %d hidden units, '
            '%d chains x %d temperatures = %d rows, %d steps per sweep.\n' % (G, K, V, H, args.chains, args.temps, rows, args.steps))
    if _ffi.load().bm_device_count() <= 0:
        text = head + '\nNo GPU run of the tool has been made: nothing here has been measured and no speed is promised.\n'
    else:
        eg, eb = handle(True, rows), handle(False, rows)
        eg.groups_pt.pt_init(args.chains, ladder(args.temps))
        eb.pt_init(args.chains, ladder(args.temps))
        wall, cls = time_sweeps({'groups 196 x 4, fused route': (eg, eg.groups_pt), 'Bernoulli 784': (eb, eb)}, args.runs, args.steps)
        sm = plain_sm_pass(eg, rows, args.runs, args.steps)
        eg.close()
        eb.close()
        env = dict(os.environ, BM355_DEBUG='sm_fused=0')
        cmd = [sys.executable, os.path.abspath(__file__), '--generic-leg', '--runs', str(args.runs), '--steps', str(args.steps),
               '--chains', str(args.chains), '--temps', str(args.temps)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0 or 'SOFTMAX_PT_GENERIC' not in r.stdout:
            raise SystemExit('the generic leg failed:\n' + r.stdout[-2000:] + r.stderr[-4000:])
        gen = json.loads(r.stdout.split('SOFTMAX_PT_GENERIC', 1)[1].strip().splitlines()[0])
        wall['groups 196 x 4, generic route (sm_fused=0, own process)'] = gen['wall']
        cls['groups 196 x 4, generic route (sm_fused=0, own process)'] = tuple(gen['cls'])
        fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)), min(v), max(v))
        base = float(np.median(wall['Bernoulli 784']))
        out = [head, '| tempered step | us per step, host clock (median, min - max) | ratio to Bernoulli | kernel us per step: prop-up | prop-down '
               '(fused pass / raw pass) | other (groups kernel + row-dot) |', '|---|---|---|---|---|---|']
        for n in wall:
            out.append('| %s | %s | %.3f | %.1f | %.1f | %.1f |' % ((n, fmt(wall[n]), float(np.median(wall[n])) / base) + cls[n]))
        f_dn = cls['groups 196 x 4, fused route'][1]
        g_cls = cls['groups 196 x 4, generic route (sm_fused=0, own process)']
        out += ['', '| prop-down on %d rows, kernel time by event pairs | us per launch |' % rows, '|---|---|',
                '| fused, SM + SA + RT (row temperatures, v.vb partials) | %.1f |' % f_dn,
                '| plain SM pass (bm_rbm_sample_v_from_h) | %.1f |' % sm,
                '| generic route: raw pass + groups kernel + row-dot | %.1f + %.1f = %.1f |' % (g_cls[1], g_cls[2], g_cls[1] + g_cls[2]),
                '', '%d sweeps per leg after a warm-up sweep, the two in-process legs alternating; whole-sweep times by the host clock around a '
                'synchronise with the per-class event timing off, kernel times from a second pass with it on; bench.py\'s weights.  '
                'No speed target is set.' % args.runs]
        text = '\n'.join(out) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
