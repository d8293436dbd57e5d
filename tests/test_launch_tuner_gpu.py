"""-m gpu: what the launch tuner (csrc/bm_launch.h) promises.  With BM355_DEBUG=tune_log=1 every measurement prints one
`bm355 tune:` line per decision, so the log of a process shows that
  - a shape is measured ONCE per process: every distinct key (the text up to `->`, per line kind: geometry or tile map)
    appears exactly once, also when a second engine of the same shape runs in the same process;
  - every reported geometry is one of that tuner's candidates, every tile map the slab order or one of the four XCD grids;
  - the tuning launches have no side effects: the results still equal the oracle's bit for bit.
The switch is read once per process, hence the subprocess."""
import collections
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the candidate lists of tune_act_shape, launch_act_bf3 and tune_grad_shape
CANDIDATES = {'act': {8, 4, 1, 3, 108, 104, 101, 103, 6, 5, 7, 9}, 'bf16x3 act': {2, 8, 4}, 'grad': {4, 8, 104, 108, 9}}
# the slab order (-1 in the act lines, 9 in the grad line) or an XCD grid
TILE_MAPS = {'act': {-1, 8, 4, 2, 1}, 'grad': {9, 8, 4, 2, 1}}

SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tests.helpers import assert_state_equal, make_pair, synth_data
from boltzmann_machines_amd.engine import as_device, DbmEngine
from oracle import oracle as orc

# RBM updates; the first shape twice (two engines, one process: the second one must find every decision made)
for V, H, B, k, kw in ((100, 52, 37, 2, dict(sample_v_states=True, l2=1e-3, sparsity_cost=1e-3, dropout=0.8)),
                       (784, 256, 64, 1, dict(sample_v_states=True, l2=1e-5)),
                       (100, 52, 37, 2, dict(sample_v_states=True, l2=1e-3, sparsity_cost=1e-3, dropout=0.8))):
    eng, twin = make_pair(V, H, max_batch=B, **kw)
    eng.seed(11); twin.set_seed(11)
    for s in range(3):
        X = synth_data(B, V, s)
        eng.train_step(as_device(X), B, 0.05, 0.9, k)
        twin.train_step(X, 0.05, 0.9, k)
        assert_state_equal(eng, twin)
    eng.close()

# one DBM update: two-segment layer inputs, mean-field passes, PCD
V, nh, N = 40, [24, 32], 16
kw = dict(n_particles=N, batch_size=N, max_mf_updates=6, mf_tol=1e-6, l2=1e-3, max_norm=2.0)
eng = DbmEngine(V, nh, **kw)
twin = orc.OracleDBM(V, nh, **kw)
W0 = (orc.normal(1, 1, 0, V * nh[0]) * np.float32(0.1)).reshape(V, nh[0])
W1 = (orc.normal(1, 2, 0, nh[0] * nh[1]) * np.float32(0.1)).reshape(nh[0], nh[1])
P0 = (orc.uniform(1, 3, 0, N * V) < 0.3).astype(np.float32).reshape(N, V)
for name, val in (('W', W0), ('W_1', W1), ('v', P0)):
    eng.set(name, val); twin.p[name][...] = val
eng.seed(7); twin.set_seed(7)
X = (orc.uniform(1, 4, 0, N * V) < 0.2).astype(np.float32).reshape(N, V)
eng.train_step(as_device(X), 0.05, 0.5, 2)
twin.train_step(X, 0.05, 0.5, 2)
for n in ('W', 'W_1', 'vb', 'hb', 'hb_1', 'v', 'mu', 'mu_1'):
    assert np.array_equal(eng.get(n).view(np.uint32), twin.p[n].view(np.uint32)), n
print('TUNER_OK')
'''

LINE = re.compile(r'^bm355 tune: ((act|bf16x3 act|grad) .*?) -> (geometry|tile map) (-?\d+)')


def test_tuner_measures_each_shape_once_and_picks_a_candidate(gpu_lib):
    env = dict(os.environ, BM355_DEBUG='tune_log=1')
    r = subprocess.run([sys.executable, '-c', SCRIPT % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'TUNER_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith('bm355 tune:')]
    seen = collections.Counter()
    tuners = set()
    for l in lines:
        m = LINE.match(l)
        assert m, l
        key, tuner, kind, value = m.group(1), m.group(2), m.group(3), int(m.group(4))
        seen[(key, kind)] += 1
        tuners.add(tuner)
        if kind == 'geometry':
            assert value in CANDIDATES[tuner], l
            m2 = re.search(r', tile map (-?\d+) ', l)        # the grad line reports both decisions
            assert (m2 is not None) == (tuner == 'grad'), l
            if m2:
                assert int(m2.group(1)) in TILE_MAPS['grad'], l
        else:
            assert tuner == 'act' and value in TILE_MAPS['act'], l
    print('\n'.join(lines))
    assert {'act', 'grad'} <= tuners, lines
    again = {k: n for k, n in seen.items() if n != 1}
    assert not again, again
    # the two RBM shapes alone give two grad shapes and four act shapes (a prop-up and a prop-down each); the DBM adds its own
    assert sum(1 for (k, kind) in seen if k.startswith('grad ')) >= 2, lines
    assert sum(1 for (k, kind) in seen if k.startswith('act ') and kind == 'geometry') >= 4, lines
