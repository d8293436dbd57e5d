"""The flavour table of csrc/bm_launch.h routes every pass as the hand-written preconditions did: tests/launch_route_check.hip, a
stand-alone host program with the earlier ladder and preconditions frozen inside it, compares flavour, verdict, stripped args and
memo flags over every single and double change of the selecting fields from eight start points.  No GPU, no HIP runtime call."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flavour_table_routes_as_the_frozen_preconditions(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path / 'launch_route_check')
    cmd = [hipcc, '--cuda-host-only', '-O1', '-std=c++17',          # host code only: the program makes no device call '-Wall', '-Wno-unused-function',
           '-I', os.path.join(ROOT, 'boltzmann_machines_amd', 'csrc'), os.path.join(ROOT, 'tests', 'launch_route_check.hip'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r'(\d+) cases from 8 start points, (\d+) admitted, 0 mismatches', r.stdout)
    assert m, r.stdout
    # a few thousand cases per start point, refusals and admissions both well represented
    assert int(m.group(1)) >= 8 * 2000 and 1000 <= int(m.group(2)) <= int(m.group(1)) - 1000
