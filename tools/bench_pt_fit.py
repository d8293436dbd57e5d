#!/usr/bin/env python
"""The price of an update with a tempered negative phase, at 784 x 1024, batch 512, k = 1, M = 512 chains.

Per update, in ONE process, alternating, --runs times each after a warm-up call (launch tuning, code objects):

  a. bm_rbm_train_step (CD-1), through the native loop bm_rbm_train_epoch
  b. bm_rbm_train_step_pt with R = 1, 5, 10 temperatures, through bm_rbm_train_epoch_pt

The hand-over switch BM355_DEBUG=pt_sel is read once per process, so the whole measurement runs twice, each in a fresh child
process: pt_sel=1 (the beta = 1 rows leave the last prop-down's epilogue) and pt_sel=0 (a gather launch).  The children run
one after the other; nothing is started after one that failed.  Times are HIP-event times on the engine's stream around
`--updates` updates per call (the calls only enqueue).  Prints a markdown report; --out writes it as well (meant for the
measured section of profiles/pt_fit_bench.md).

    python tools/bench_pt_fit.py [--runs 7] [--updates 20] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H, B, M, K = 784, 1024, 512, 512, 1
TEMPS = (1, 5, 10)


def leg(runs, n):
    """one process: {name: [us per update of every run]}"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    X = (philox.uniform(87654321, 42, 0, n * B * V).reshape(n * B, V) < 0.1307).astype(np.float32)      # bench.py's density
    Xd = DeviceArray.from_numpy(X)
    W = philox.tf_random_normal((V, H), 0.01, 1337)                                                      # bench.py's weights

    def engine():
        eng = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=B, l2=1e-5)
        eng.set('W', W)
        eng.seed(1)
        return eng
    plain = engine()
    calls = [('cd1', plain, lambda: plain.train_epoch(Xd, n * B, B, 0.05, 0.9, K))]
    for R in TEMPS:
        eng = engine()
        eng.pt_init(M, np.linspace(0., 1., R + 1)[1:].astype(np.float32))
        calls.append(('pt_R%d' % R, eng, (lambda e: lambda: e.train_epoch_pt(Xd, n * B, B, 0.05, 0.9, K))(eng)))
    for _, eng, call in calls:
        call()
        eng.sync()
    us = {name: [] for name, _, _ in calls}
    for _ in range(runs):                                       # alternating: a drift of the box hits every case
        for name, eng, call in calls:
            eng.timer_start()
            call()
            us[name].append(1e3 * eng.timer_stop() / n)
    for _, eng, _ in calls:
        eng.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=20)
    ap.add_argument('--out', default=None, help='write the report here as well')
    ap.add_argument('--leg', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        print('PT_FIT_LEG ' + json.dumps(leg(args.runs, args.updates)))
        return
    res = {}
    for sel in ('1', '0'):
        dbg = ','.join(x for x in (os.environ.get('BM355_DEBUG', ''), 'pt_sel=' + sel) if x)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', '--runs', str(args.runs), '--updates', str(args.updates)],
                           env=dict(os.environ, BM355_DEBUG=dbg), capture_output=True, text=True, timeout=420)
        line = [l for l in r.stdout.splitlines() if l.startswith('PT_FIT_LEG ')]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit('bench_pt_fit: the pt_sel=%s leg failed (exit %d)' % (sel, r.returncode))
        res[sel] = json.loads(line[0][len('PT_FIT_LEG '):])
    med = lambda t: float(np.median(t))
    each = lambda t: ', '.join('%.1f' % x for x in t)
    spread = lambda t: (max(t) - min(t)) / med(t)
    rows = [('`bm_rbm_train_step` (CD-1), pt_sel=%s process' % sel, res[sel]['cd1']) for sel in ('1', '0')]
    for R in TEMPS:
        for sel in ('1', '0'):
            rows.append(('`bm_rbm_train_step_pt`, R = %d, pt_sel=%s' % (R, sel), res[sel]['pt_R%d' % R]))
    cd = med(res['1']['cd1'] + res['0']['cd1'])
    lines = [
        '## Measured (`tools/bench_pt_fit.py`)',
        '',
        'One MI355X; %d x %d, batch %d, k = %d, M = %d chains; every call %d updates through the native loop, one warm-up, then'
        % (V, H, B, K, M, args.updates),
        '%d timed runs, the cases of a process alternating; HIP-event time on the engine stream; pt_sel=1 and pt_sel=0 in a' % args.runs,
        'process each, one after the other.',
        '',
        '| case | us per update (each run) | median us | (max - min) / median |',
        '|---|---|---|---|',
    ] + ['| %s | %s | %.1f | %.3f |' % (name, each(u), med(u), spread(u)) for name, u in rows] + ['']
    for R in TEMPS:
        a, b = med(res['1']['pt_R%d' % R]), med(res['0']['pt_R%d' % R])
        lines.append('* R = %d: hand-over in the epilogue %.1f us, gather launch %.1f us (%+.1f us, ratio %.3f); tempered / CD-1 = %.2f'
                     % (R, a, b, a - b, a / b, a / cd))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
