"""-m gpu: the Normal sampler of csrc/bm_rng.h (`box_muller`) ON THE DEVICE, at chosen Philox words and through every code
path that consumes a pair.  tests/normal_probes.py finds the stream positions of the edge words and holds the float64
reference; tests/test_normal_sampler.py is the proof, without a GPU, that the oracle passes each assertion made here.

The probe: an RbmEngine with Gaussian visible units, sample_v_states = True and W = 0.  `seed(s)` (it resets the call
counter), `set_row_offset(row0)`, `gibbs(Hd, Vd, B, n_steps)`: the last step's V is n * sigma + vb with n the draw of site
3 + 16 (n_steps - 1), call 0, flat index (row0 + j) * V + i.  Every tensor of raw draws meets three assertions: bit for
bit the oracle twin, equal to orc.normal at the same stream position, and within DRAW_ATOL of the float64 Box-Muller of
the same two words (the device is held to float64 directly, not through the oracle).

Which path draws:
  * V % 4 == 0: the block(s) precomputed under the pipeline fill.  The RBM prop-down reads W x-major, which exists for the
    geometries with MI = 1 only (csrc/bm_launch.h: launch_act_as) - so an RBM probe runs `PhiloxOne` whatever geometry is
    forced.  `PhiloxPair` (MI = 2; its second block is `block + 1` across the counter words) draws visible units in the
    DBM's visible pass when the hidden width is no multiple of 4 (k-major W^T): the DBM probe with 18 hidden units.
  * V % 4 != 0: the generic `draw4`, a Philox block per element, pair (idx & 3) >> 1, sin or cos by idx & 1.
  * six passes or more and eight row blocks: the chained launch, with an `rng.init` of its own (csrc/bm_chain.h).
The DBM's `sample_v` returns the MEANS of its last mean sweep; the sampled visible layer of sweep 0 (site 12) of
sample_v(2) stays in the variable `v_new` (oracle: orc_dbm_particles), which is what the DBM probe reads.

Out of scope: the float64 engines.  They draw with the device's log / sin / cos, compared at 1e-12
(csrc/bm_rbm64.hip), and RbmEngine64 has no `gibbs` that would return raw draws."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import normal_probes as nb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SITE = nb.SEED, nb.SITE_V


class Probe(object):
    """the W = 0 RbmEngine of the module docstring; one handle serves every row offset"""

    def __init__(self, V, B, H=16, v_unit=1, sigma=None, vb=None):
        from boltzmann_machines_amd.engine import RbmEngine
        self.V, self.H, self.B, self.v_unit = V, H, B, v_unit
        self.sigma, self.vb = sigma, vb
        self.eng = RbmEngine(V, H, v_unit=v_unit, sample_v_states=True, max_batch=B)
        self.eng.set('W', np.zeros((V, H), dtype=np.float32))
        self.eng.set('hb', np.zeros(H, dtype=np.float32))
        self.eng.set('vb', np.zeros(V, dtype=np.float32) if vb is None else vb)
        if sigma is not None:
            self.eng.set('sigma', sigma)

    def draws(self, row0, n_steps=1):
        """(V, H) of the device and of the twin after n_steps from an all-zero hidden bitmap at row offset row0"""
        from boltzmann_machines_amd._ffi import DeviceArray
        H0 = np.zeros((self.B, self.H), dtype=np.float32)
        self.eng.seed(SEED)
        self.eng.set_row_offset(row0)
        Hd, Vd = DeviceArray.from_numpy(H0), DeviceArray((self.B, self.V))
        self.eng.gibbs(Hd, Vd, self.B, n_steps)
        self.eng.sync()
        twin = orc.OracleRBM(self.V, self.H, v_unit=self.v_unit, sample_v_states=True)
        if self.sigma is not None:
            twin.p['sigma'][...] = self.sigma
        if self.vb is not None:
            twin.p['vb'][...] = self.vb
        twin.set_seed(SEED)
        twin.row0 = int(row0)
        Ht, Vt = twin.gibbs(H0, n_steps)
        return Vd.numpy(), Hd.numpy(), Vt, Ht

    def close(self):
        self.eng.close()


def check_raw(p, row0, what, site=SITE, n_steps=1):
    """the three assertions on the raw draws of probe p at row0 -> (device V, largest error against float64)"""
    Vd, Hd, Vt, Ht = p.draws(row0, n_steps)
    nb.assert_bits(Vd, Vt, what + ': device against the twin')
    nb.assert_bits(Hd, Ht, what + ': hidden bitmap against the twin')
    return Vd, nb.assert_draws(Vd, SEED, site, p.B * p.V, row0 * p.V, what + ': device')


def edge_pairs(found, targets, widths=(64, 37)):
    """part a for the given targets: V = 64 (precomputed block) and V = 37 (generic draw4, pairs straddling rows)"""
    worst = 0.0
    for V in widths:
        p = Probe(V, 3)
        for tgt in targets:
            idx = found[tgt]
            row0, B = nb.rows_for(idx, V)
            assert B == p.B
            Vd, err = check_raw(p, row0, 'V = %d, word %d mantissa %#x at element %d' % ((V,) + tgt + (idx,)))
            worst = max(worst, err)
            if tgt == nb.CLAMP:
                nb.check_clamp_pair(Vd, SEED, SITE, idx, row0)
        p.close()
    return worst


@pytest.fixture(scope='module')
def found():
    return nb.find_words(SEED, SITE, 0)


# ---- a. every edge pair, aligned and generic
def test_edge_pairs_aligned_and_generic(gpu_lib, found):
    worst = edge_pairs(found, sorted(found))
    print('device, %d edge pairs x 2 widths: worst draw %.3e from float64 (bound %.3e)' % (len(found), worst, nb.DRAW_ATOL))


# ---- b. bulk
@pytest.mark.parametrize('B,V', nb.BULK, ids=lambda x: str(x))
def test_bulk_of_draws(gpu_lib, B, V):
    p = Probe(V, B)
    Vd, err = check_raw(p, nb.BULK_ROW0, '%d x %d' % (B, V))
    p.close()
    N = Vd.size
    x = Vd.astype(np.float64)
    mean, var = x.mean(), x.var()
    print('device bulk %d x %d: worst draw %.3e from float64, mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e)'
          % (B, V, err, mean, 5 / np.sqrt(N), var - 1, 5 * np.sqrt(2.0 / N)))
    assert abs(mean) < 5 / np.sqrt(N)                    # five standard errors of the mean of N unit normals
    assert abs(var - 1) < 5 * np.sqrt(2.0 / N)           # ... of their variance (Var s^2 = 2 / N)


# ---- c. n * sigma + vb is two roundings
def test_scale_and_shift_is_two_roundings(gpu_lib):
    sigma, vb, n, want, fused = nb.two_roundings_case()
    assert np.sum(nb.bits(want) != nb.bits(fused)) > 100                          # the points can tell a contracted fma
    B, V = n.shape
    p = Probe(V, B, sigma=sigma, vb=vb)
    Vd, Hd, Vt, Ht = p.draws(3)
    p.close()
    nb.assert_bits(Vd, want, 'device n * sigma + vb against float32(float32(n * sigma) + vb)')
    nb.assert_bits(Vd, Vt, 'device against the twin')


# ---- d. the chained launch
def test_chained_launch_draws(gpu_lib):
    V, H, B = nb.CHAIN_SHAPE
    site = SITE + 16 * (nb.CHAIN_STEPS - 1)
    p = Probe(V, B, H=H)
    for tgt, idx in sorted(nb.find_words(SEED, site, 0, nb.CHAIN_TARGETS).items()):
        before = p.eng.chain_stats()[0]
        check_raw(p, idx // V - 1, 'chained, word %d mantissa %#x' % tgt, site=site, n_steps=nb.CHAIN_STEPS)
        st = p.eng.chain_stats()
        assert st[0] == before + 1, 'the six passes did not run as one chained launch: chain_stats %r' % (st,)
    p.close()


# ---- e. every geometry, forced
def geometry_leg(found, dbm_idx):
    """what one subprocess of test_forced_geometry runs (the geometry is read once per process)"""
    edge_pairs(found, (nb.CLAMP, nb.ANGLE0, nb.FOLD))
    p = Probe(256, 64)
    check_raw(p, nb.BULK_ROW0, '64 x 256')
    p.close()
    # PhiloxPair draws visible units in the DBM's k-major visible pass only (module docstring): the clamp word and the
    # block-counter carry there
    dbm_draws(64, 18, dbm_idx // 64 - 1)
    dbm_draws(nb.CARRY[0][0], 18, nb.CARRY[0][1])


SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
from tests import test_normal_sampler_gpu as t
t.geometry_leg(%(found)r, %(dbm_idx)r)
print('NORMAL_GEOMETRY_OK')
'''


@pytest.mark.parametrize('geo', ['4', '8', '1', '3', '104', '6', '9', '5'])
def test_forced_geometry(gpu_lib, found, geo):
    dbm_idx = nb.find_words(SEED, nb.SITE_DBM_V, 0, (nb.CLAMP,))[nb.CLAMP]
    env = dict(os.environ, BM355_DEBUG='act_geo=' + geo)
    r = subprocess.run([sys.executable, '-c', SCRIPT % dict(root=ROOT, found=found, dbm_idx=dbm_idx)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'NORMAL_GEOMETRY_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- f. the carry of the block counter
@pytest.mark.parametrize('V,row0', nb.CARRY)
def test_block_counter_carry(gpu_lib, V, row0):
    p = Probe(V, 3)
    check_raw(p, row0, 'Gaussian units across block 2^32')
    p.close()
    p = Probe(V, 3, v_unit=0)
    Vd, Hd, Vt, Ht = p.draws(row0)
    p.close()
    nb.assert_bits(Vd, Vt, 'Bernoulli units across block 2^32: device against the twin')
    nb.assert_bits(Hd, Ht, 'hidden bitmap against the twin')
    nb.assert_bits(Vd, (orc.uniform(SEED, SITE, 0, 3 * V, idx0=row0 * V) < 0.5).astype(np.float32).reshape(3, V),
                   'Bernoulli units across block 2^32: device against u < 1/2')


# ---- g. the DBM's visible pass
def dbm_draws(V, H, particle0):
    from boltzmann_machines_amd.engine import DbmEngine
    sigma, vb = nb.dbm_case(V)
    eng = DbmEngine(V, [H], v_unit=1, n_particles=3, batch_size=3)
    eng.set('W', np.zeros((V, H), dtype=np.float32))
    eng.set('sigma', sigma)
    eng.set('vb', vb)
    eng.set('v', np.zeros((3, V), dtype=np.float32))
    eng.set('h', np.zeros((3, H), dtype=np.float32))
    eng.seed(SEED)
    eng.set_row_offset(0, particle0)
    eng.sample_v(2)
    v, v_new, h = eng.get('v'), eng.get('v_new'), eng.get('h')
    eng.close()
    twin, vt = nb.dbm_twin(V, H, particle0)
    what = 'DBM %d-%d at particle %d' % (V, H, particle0)
    nb.assert_bits(v, vt, what + ': sample_v against the twin')
    nb.assert_bits(h, twin.p['h'], what + ': h against the twin')
    nb.assert_bits(v_new, twin.p['v_new'], what + ': the sampled visible layer (v_new) against the twin')
    return v_new, nb.check_dbm_draws(v_new, V, particle0, what)


@pytest.mark.parametrize('V', [64, 37])
@pytest.mark.parametrize('H', nb.DBM_HIDDEN)
def test_dbm_visible_pass(gpu_lib, V, H):
    idx = nb.find_words(SEED, nb.SITE_DBM_V, 0, (nb.CLAMP,))[nb.CLAMP]
    p0 = idx // V - 1
    v_new, worst = dbm_draws(V, H, p0)
    sigma, vb = nb.dbm_case(V)
    n = ((v_new.astype(np.float64) - vb[None, :]) / sigma[None, :]).reshape(-1)
    k = idx - p0 * V
    assert 5.6777 * 0.7071 - 1e-4 < np.abs(n[k:k + 2]).max() < nb.R_MAX + 1e-4          # the clamp word's pair is in the tensor
    print('DBM %d-%d: largest error / bound %.3f' % (V, H, worst))


def test_dbm_visible_pass_across_the_block_counter_carry(gpu_lib):
    V, p0 = nb.CARRY[0]
    for H in nb.DBM_HIDDEN:
        dbm_draws(V, H, p0)
