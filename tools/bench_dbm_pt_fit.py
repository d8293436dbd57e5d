#!/usr/bin/env python
"""The price of a DBM update with a tempered negative phase, at 784-512-1024, batch 100, 100 particles,
max_mf_updates 50, k = 5 steps per update, 100 chains.

Per update, in ONE process, alternating, --runs times each after --warmup-calls warm-up calls (launch tuning, code objects, and
enough updates for the mean-field loop to reach the length it has in training):

  a. bm_dbm_train_step (the plain update: PCD-5 on the persistent particles, on the second stream under the mean-field loop)
  b. bm_dbm_mean_field alone, on the handle of (a) right behind its updates: the positive phase both updates share, under
     the parameters the training has reached (the loop's trip count grows from a few sweeps to its cap while the parameters
     leave their initial values, so a handle that does not train would time another loop; the executed sweeps are reported)
  c. for R = 1, 4, 10 temperatures: bm_dbm_train_step_pt, and bm_dbm_pt_sweep(5) alone (the tempered sweeps of 100 R rows)

so that "tempered - plain", "mean-field" and "sweeps" can be read side by side: if the sweeps are short against the mean-field
loop, running them under it (as the plain update runs its particle sweeps) could hide at most min(sweeps, mean-field).  Times
are HIP-event times on the engine's main stream around `--updates` calls (the calls only enqueue; the mean-field loop's
trip-count read is part of every update).  Every engine sees the same minibatches in the same order; the parameters move, as
in training.  Prints a markdown report; --out writes it as well (the measured section of profiles/dbm_pt_fit_bench.md).

    python tools/bench_dbm_pt_fit.py [--runs 7] [--updates 20] [--warmup-calls 4] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N_LAYERS = (784, 512, 1024)
B, M, MAX_MF, K = 100, 100, 50, 5
TEMPS = (1, 4, 10)
LR, MOM = 0.0005, 0.9


def measure(runs, n, warmup_calls):
    """({name: [us per call of every run]}, {name: [executed mean-field sweeps per update, mean of every run]})"""
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import DbmEngine
    from boltzmann_machines_amd.utils import philox
    V = N_LAYERS[0]
    X = (philox.uniform(87654321, 42, 0, n * B * V).reshape(n * B, V) < 0.1307).astype(np.float32)      # bench.py's density
    Xd = DeviceArray.from_numpy(X)
    W = [philox.tf_random_normal((N_LAYERS[i], N_LAYERS[i + 1]), 0.01, 1337 + i) for i in range(2)]

    def engine():
        eng = DbmEngine(V, list(N_LAYERS[1:]), n_particles=M, batch_size=B, max_mf_updates=MAX_MF, mf_tol=1e-7, l2=1e-7, max_norm=6.)
        eng.set('W', W[0])
        eng.set('W_1', W[1])
        eng.seed(1)
        return eng

    def each_batch(f):
        def run():
            return [f(u * B) for u in range(n)]
        return run
    plain = engine()
    calls = [('plain', plain, each_batch(lambda row: plain.train_step(Xd, LR, MOM, K, row=row)[0])),
             ('mean_field', plain, each_batch(lambda row: plain.mean_field(Xd, row=row)))]
    for R in TEMPS:
        betas = np.linspace(0., 1., R + 1)[1:].astype(np.float32)
        e1, e2 = engine(), engine()
        e1.pt_init(M, betas)
        e2.pt_init(M, betas)
        calls.append(('pt_R%d' % R, e1, each_batch((lambda e: lambda row: e.train_step_pt(Xd, LR, MOM, K, row=row)[0])(e1))))
        calls.append(('sweeps_R%d' % R, e2, each_batch((lambda e: lambda row: e.pt_sweep(K))(e2))))
    for _ in range(warmup_calls):                               # warm-up: every shape the timed window uses, and enough
        for _, eng, call in calls:                              # updates for the mean-field loop to reach its steady length
            call()
            eng.sync()
    us = {name: [] for name, _, _ in calls}
    nmf = {name: [] for name, _, _ in calls}
    for _ in range(runs):                                       # alternating: a drift of the box hits every case
        for name, eng, call in calls:
            eng.timer_start()
            got = call()
            us[name].append(1e3 * eng.timer_stop() / n)
            if got[0] is not None:
                nmf[name].append(float(np.mean(got)))
    for eng in set(e for _, e, _ in calls):
        eng.close()
    return us, nmf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=20)
    ap.add_argument('--warmup-calls', type=int, default=4)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    us, nmf = measure(args.runs, args.updates, args.warmup_calls)
    med = lambda t: float(np.median(t))
    each = lambda t: ', '.join('%.0f' % x for x in t)
    spread = lambda t: (max(t) - min(t)) / med(t)
    label = dict(plain='`bm_dbm_train_step` (plain, PCD-%d)' % K, mean_field='`bm_dbm_mean_field` alone')
    for R in TEMPS:
        label['pt_R%d' % R] = '`bm_dbm_train_step_pt`, R = %d' % R
        label['sweeps_R%d' % R] = '`bm_dbm_pt_sweep(%d)` alone, R = %d' % (K, R)
    order = ['plain', 'mean_field'] + [s % R for R in TEMPS for s in ('pt_R%d', 'sweeps_R%d')]
    lines = [
        '## Measured (`tools/bench_dbm_pt_fit.py`)',
        '',
        'One MI355X; %d-%d-%d, batch %d, %d particles, max_mf_updates %d, k = %d, %d chains; every call %d updates, %d warm-up calls,'
        % (N_LAYERS + (B, M, MAX_MF, K, M, args.updates, args.warmup_calls)),
        'then %d timed runs, the cases alternating in one process; HIP-event time on the engine stream.' % args.runs,
        '',
        '| case | us per update (each run) | median us | (max - min) / median | mean-field sweeps per update (median of the runs) |',
        '|---|---|---|---|---|',
    ] + ['| %s | %s | %.0f | %.3f | %s |' % (label[k], each(us[k]), med(us[k]), spread(us[k]), '%.1f' % med(nmf[k]) if nmf[k] else '-')
         for k in order] + ['']
    p, m = med(us['plain']), med(us['mean_field'])
    for R in TEMPS:
        t, s = med(us['pt_R%d' % R]), med(us['sweeps_R%d' % R])
        lines.append('* R = %d: tempered / plain = %.2f (%+.0f us); sweeps alone %.0f us, mean-field alone %.0f us: the most an overlap '
                     'of the two could hide is %.0f us = %.0f %% of the tempered update' % (R, t / p, t - p, s, m, min(s, m), 100. * min(s, m) / t))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
