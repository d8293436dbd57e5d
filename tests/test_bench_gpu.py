"""-m gpu: bench.py's plain run - the one JSON line of the headline alone, exactly --steps timed steps, and
--dump-outputs writing the same arrays from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2',
                        '--dump-outputs', str(out_dir)] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs_are_reproducible(gpu_lib, tmp_path):
    a = _bench(tmp_path / 'a')
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in a, k
    assert a['steps'] == 7 and a['warmup'] == 2 and a['ms_per_step'] > 0 and a['higher_is_better'] is True
    assert a['dtype'] == 'f32'
    assert 'other_configs' not in a and 'cpu_baseline' not in a            # --full only
    names = sorted(os.listdir(str(tmp_path / 'a')))
    assert names == ['W.npy', 'dW.npy', 'dhb.npy', 'dvb.npy', 'hb.npy', 'vb.npy'], names
    assert sum(os.path.getsize(str(tmp_path / 'a' / n)) for n in names) <= 64 << 20
    W = np.load(str(tmp_path / 'a' / 'W.npy'))
    assert W.dtype == np.float32 and W.shape == (784, 1024) and np.all(np.isfinite(W))
    _bench(tmp_path / 'b')
    for n in names:
        x, y = np.load(str(tmp_path / 'a' / n)), np.load(str(tmp_path / 'b' / n))
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), n


@pytest.mark.gpu
def test_bench_dump_of_a_dbm_run(gpu_lib, tmp_path):
    d = _bench(tmp_path, '--config', 'dbm')
    assert d['steps'] == 7
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ['W.npy', 'W_1.npy', 'h.npy', 'h_1.npy', 'hb.npy', 'hb_1.npy', 'n_mf_updates.npy', 'v.npy', 'vb.npy'], names
    assert np.load(str(tmp_path / 'W_1.npy')).shape == (512, 1024)
