"""-m gpu: the engine handles own their device memory, streams and events (csrc/bm_common.h).  A create that fails part
way - here on an allocation far larger than the card, after a first few that succeed - raises Bm355Error, frees what it
had allocated and leaves HIP's last error clear, so that the next engine of the process creates and trains normally."""
import ctypes as C

import numpy as np
import pytest

from boltzmann_machines_amd import _ffi
from boltzmann_machines_amd._ffi import Bm355Error, DeviceArray
from boltzmann_machines_amd.engine import DbmEngine, DbmEngine64, RbmEngine, RbmEngine64

pytestmark = pytest.mark.gpu

MiB = 1 << 20
REPEATS = 8
# Each create below allocates its weights first (under 1 GiB) and then asks for a [rows][units] workspace of about
# 4 TiB, which hipMalloc refuses at once.  A create that kept its weights lost 384 MiB (float64 RBM) to 771 MiB (the
# float32 kinds) per attempt, 3 GiB or more over REPEATS attempts.  Free memory is read device-wide, so the tolerance
# also has to absorb what anything else on the card allocates meanwhile: 256 MiB is under a quarter of the smallest
# such loss and far above what a create that frees everything leaves behind (nothing).
TOL = 256 * MiB
HUGE = 1 << 27                      # rows of the workspace that cannot be allocated

FAILING = {
    'rbm': lambda: RbmEngine(8192, 8192, max_batch=HUGE),                       # W, dW, Wt: 3 x 257 MiB, then [rows][H]
    'rbm64': lambda: RbmEngine64(4096, 4096, max_batch=HUGE),                   # W, Wt, dW: 3 x 128 MiB, then [rows][H]
    'dbm': lambda: DbmEngine(8192, (8192,), batch_size=HUGE, n_particles=8),    # W, Wt, dW: 3 x 257 MiB, then mu [N][n1]
    'dbm64': lambda: DbmEngine64(4096, (4096,), batch_size=HUGE, n_particles=8),  # W, Wt, dW, pos, neg: 5 x 128 MiB, then mu
}


def _hip_free_bytes():
    """hipMemGetInfo's free bytes of the current device, through the HIP runtime libbm355 is linked against"""
    _ffi.load()
    with open('/proc/self/maps') as f:
        path = next(line.split()[-1] for line in f if 'libamdhip64' in line)
    hip = C.CDLL(path)
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _small_step(kind):
    """a small engine of the kind creates and runs one train_step"""
    rng = np.random.RandomState(7)
    if kind in ('rbm', 'rbm64'):
        cls, dt = (RbmEngine, np.float32) if kind == 'rbm' else (RbmEngine64, np.float64)
        eng = cls(16, 8, max_batch=4)
        X = DeviceArray.from_numpy((rng.rand(4, 16) < 0.5).astype(dt), dt)
        eng.train_step(X, 4, 0.01, 0.9, 1)
    else:
        cls, dt = (DbmEngine, np.float32) if kind == 'dbm' else (DbmEngine64, np.float64)
        eng = cls(16, (8, 4), batch_size=4, n_particles=4)
        X = DeviceArray.from_numpy((rng.rand(4, 16) < 0.5).astype(dt), dt)
        eng.train_step(X, 0.01, 0.9, 1)
    W = eng.get('W')
    eng.close()
    assert np.all(np.isfinite(W))


@pytest.mark.parametrize('kind', sorted(FAILING))
def test_failed_create_frees_everything(gpu_lib, kind):
    with pytest.raises(Bm355Error):
        FAILING[kind]()                          # warm-up: one-time runtime allocations are not counted
    before = _hip_free_bytes()
    for _ in range(REPEATS):
        with pytest.raises(Bm355Error):
            FAILING[kind]()
    lost = before - _hip_free_bytes()
    assert lost <= TOL, '%d failed creates lost %.0f MiB of device memory' % (REPEATS, lost / MiB)
    _small_step(kind)
