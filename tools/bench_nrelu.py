#!/usr/bin/env python
"""The price of noisy rectified-linear hidden units: one CD-1 update at 784 x 1024, batch 512 (Bernoulli visible,
ReLURBM's handle) and at 3072 x 5000, batch 512 (Gaussian visible, GaussianReLURBM's handle), beside the Bernoulli-hidden update of
the same build at the same shape - and the hidden pass alone (bm_rbm_sample_h, means and states) for both units.

ONE process, two handles per shape (h_unit Bernoulli / NReLU), the legs alternating after a warm-up call each (launch tuning, code
objects).  Times are HIP-event times on the engine's stream around `--updates` updates that only enqueue (bm_rbm_train_epoch) or
`--passes` hidden passes; `--runs` samples per leg.  No target: the ratios NReLU / Bernoulli are recorded, not asserted.  Prints
a markdown report; --out writes it as well (meant for profiles/nrelu_bench.md).

    python tools/bench_nrelu.py [--runs 10] [--updates 50] [--passes 100] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SHAPES = [('784 x 1024, Bernoulli visible (ReLURBM)', 784, 1024, 512, 0, 0.01),
          ('3072 x 5000, Gaussian visible (GaussianReLURBM)', 3072, 5000, 512, 1, 1e-4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--updates', type=int, default=50)
    ap.add_argument('--passes', type=int, default=100)
    ap.add_argument('--out', default=None, help='write the report here as well')
    args = ap.parse_args()
    from boltzmann_machines_amd import _ffi
    from boltzmann_machines_amd._ffi import DeviceArray
    from boltzmann_machines_amd.engine import RbmEngine
    from boltzmann_machines_amd.utils import philox
    out = ['| shape | leg | Bernoulli hidden, us (median, min - max) | NReLU hidden, us (median, min - max) | NReLU / Bernoulli |',
           '|---|---|---|---|---|']
    for name, V, H, B, v_unit, lr in SHAPES:
        n_rows = 4 * B                                              # the updates cycle over four batches
        if v_unit:
            X = philox.normal(87654321, 43, 0, n_rows * V, np.float32).reshape(n_rows, V)
        else:
            X = (philox.uniform(87654321, 42, 0, n_rows * V).reshape(n_rows, V) < 0.1307).astype(np.float32)      # bench.py's density
        Xd = DeviceArray.from_numpy(X)
        W = philox.tf_random_normal((V, H), 0.01, 1337)                                                        # bench.py's weights
        Md, Sd = DeviceArray((B, H), np.float32), DeviceArray((B, H), np.float32)
        engs = {}
        for unit, h_unit in (('bernoulli', _ffi.UNIT_BERNOULLI), ('nrelu', _ffi.UNIT_NRELU)):
            e = RbmEngine(V, H, v_unit=v_unit, sample_v_states=not v_unit, sample_h_states=True, max_batch=B, l2=1e-5, h_unit=h_unit)
            e.set('W', W)
            e.seed(1)
            engs[unit] = e

        def update(e):
            for _ in range(args.updates // 4):
                e.train_epoch(Xd, n_rows, B, lr, 0.9, 1)

        def hidden(e):
            for _ in range(args.passes):
                e.sample_h(Xd, B, Md, Sd)
        n_upd = 4 * (args.updates // 4)
        legs = [('CD-1 update (bm_rbm_train_epoch)', update, n_upd), ('hidden pass alone (bm_rbm_sample_h)', hidden, args.passes)]
        for _, call, _ in legs:
            for e in engs.values():
                call(e)
                e.sync()
        for leg, call, per in legs:
            us = {u: [] for u in engs}
            for _ in range(args.runs):
                for u, e in engs.items():
                    e.timer_start()
                    call(e)
                    us[u].append(1e3 * e.timer_stop() / per)
            med = {u: float(np.median(v)) for u, v in us.items()}
            out.append('| %s | %s | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.3f |' % (
                name, leg, med['bernoulli'], min(us['bernoulli']), max(us['bernoulli']), med['nrelu'], min(us['nrelu']),
                max(us['nrelu']), med['nrelu'] / med['bernoulli']))
        for e in engs.values():
            e.close()
    out += ['', '%d runs per leg of %d updates / %d hidden passes, the two units alternating in one process (one handle each), HIP-event '
            'times per update or pass; batch 512.  The Bernoulli-hidden update runs its chain as the handle runs it by default (one chained '
            'launch where the shape allows it); the NReLU update issues per-pass launches (the NR flavour is never chained).  No speed target '
            'is set for this epilogue.' % (args.runs, n_upd, args.passes)]
    text = '\n'.join(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
