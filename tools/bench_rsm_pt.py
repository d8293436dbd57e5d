#!/usr/bin/env python
"""The price of parallel tempering over replicated softmax visible units (bm_rbm_rsm_pt_sweep) at one shape - a
vocabulary of 2000 words, 256 hidden units, an ensemble of `--chains` chains x `--temps` temperatures, documents of `--length`
tokens - three legs:
  1. a tempered step of this unit (the DB + RT prop-up, the swap, the raw pass and the PT count kernel);
  2. the Bernoulli tempered step (bm_rbm_pt_sweep of a 2000 x 256 handle: RT prop-up, swap, RT prop-down) on the same number of rows,
     as tools/bench_pt.py times it;
  3. `--temps` plain Gibbs steps of `--chains` rows of this unit (bm_rbm_gibbs: the logits pass, the plain count kernel, the DB
     prop-up) - the same number of row-steps without a ladder.

A sweep is timed whole by the host clock around a synchronise (one handle per leg, a warm-up sweep each: launch tuning, code
objects), the legs alternating; a second pass with the handle's per-class event timing on gives the kernel time of a step by class -
prop-ups, prop-downs (the raw or logits pass) and `other`, the count kernel (the swap launch is in no class).  No target and no
assertion: the figures are the record.  Prints a markdown report; --out writes it as well (meant for profiles/rsm_pt_bench.md).
Without a GPU the report says that no run was made.

    python tools/bench_rsm_pt.py [--runs 10] [--steps 20] [--chains 512] [--temps 10] [--length 200] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V, H = 2000, 256


def ladder(R):
    return np.linspace(0., 1., R + 1)[1:].astype(np.float32)


def handle(rsm, rows, length):
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    e = RbmEngine(V, H, sample_v_states=True, sample_h_states=True, max_batch=rows, rsm_max_length=length if rsm else 0)
    e.set('W', philox.tf_random_normal((V, H), 0.01, 1337))             # bench.py's weights
    e.seed(7)
    return e


def time_legs(legs, runs):
    """{name: [us per call]} by the host clock, the legs alternating; {name: (up, down, other) us per call} by event pairs"""
    for e, run in legs.values():
        run()
        e.sync()
    wall = {n: [] for n in legs}
    for _ in range(runs):
        for n, (e, run) in legs.items():
            t0 = time.perf_counter()
            run()
            e.sync()
            wall[n].append(1e6 * (time.perf_counter() - t0))
    cls = {}
    for n, (e, run) in legs.items():
        e.profile(True)
        rec = []
        for _ in range(max(2, runs // 3)):
            t0 = e.kernel_times()
            run()
            e.sync()
            t1 = e.kernel_times()
            rec.append(tuple(1e3 * (t1[c][0] - t0[c][0]) for c in ('act_up', 'act_down', 'other')))
        e.profile(False)
        cls[n] = tuple(float(np.median([r[i] for r in rec])) for i in range(3))
    return wall, cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--chains', type=int, default=512)
    ap.add_argument('--temps', type=int, default=10)
    ap.add_argument('--length', type=int, default=200)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd import _ffi
    M, R, S = args.chains, args.temps, args.steps
    rows = M * R
    head = ('# Parallel tempering over replicated softmax visible units: what a step costs\n\n`tools/bench_rsm_pt.py`: V = %d words, %d hidden '
            'units, %d chains x %d temperatures = %d rows, documents of %d tokens, %d steps per sweep.\n' % (V, H, M, R, rows, args.length, S))
    if _ffi.load().bm_device_count() <= 0:
        text = head + '\nNo GPU run of the tool has been made: nothing here has been measured and no speed is promised.\n'
    else:
        from boltzmann_machines_amd._ffi import DeviceArray
        er, eb, eg = handle(True, rows, args.length), handle(False, rows, 0), handle(True, M, args.length)
        er.rsm_pt.pt_init(M, ladder(R), lengths=np.full(M, args.length, np.float32))
        eb.pt_init(M, ladder(R))
        Dd = DeviceArray.from_numpy(np.full(M, args.length, np.float32))
        Hd = DeviceArray.from_numpy((np.random.RandomState(3).uniform(size=(M, H)) < 0.5).astype(np.float32))
        Vd = DeviceArray((M, V), np.float32)
        eg.set_row_lengths(Dd, M)
        names = ('replicated softmax, tempered', 'Bernoulli %d, tempered' % V, 'replicated softmax, %d plain Gibbs steps of %d rows' % (R, M))
        legs = {names[0]: (er, lambda: er.rsm_pt.pt_sweep(S)), names[1]: (eb, lambda: eb.pt_sweep(S)),
                names[2]: (eg, lambda: eg.gibbs(Hd, Vd, M, S * R))}
        wall, cls = time_legs(legs, args.runs)
        for e in (er, eb, eg):
            e.close()
        fmt = lambda v: '%.1f (%.1f - %.1f)' % (float(np.median(v)) / S, min(v) / S, max(v) / S)
        base = float(np.median(wall[names[0]]))
        out = [head, '| per tempered step (the third row: per %d plain steps) | us, host clock (median, min - max) | tempered RSM step / this | '
               'kernel us: prop-up | prop-down (raw or logits pass) | other (count kernel) |' % R, '|---|---|---|---|---|---|']
        for n in names:
            out.append('| %s | %s | %.3f | %.1f | %.1f | %.1f |' % ((n, fmt(wall[n]), base / float(np.median(wall[n]))) + tuple(c / S for c in cls[n])))
        out += ['', '%d sweeps per leg after a warm-up sweep, the legs alternating; whole-sweep times by the host clock around a synchronise with '
                'the per-class event timing off, kernel times from a second pass with it on; bench.py\'s weights.  No speed target is set.'
                % args.runs]
        text = '\n'.join(out) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
