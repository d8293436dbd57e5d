#!/usr/bin/env python3
"""Is the device code of libbm355.so the same in two source trees?  For host-only changes (no GPU needed).

    tools/devcode_diff.py asm <tree> <outdir>      cross-compile every unit of build.py's SOURCES of <tree> for gfx950, device
                                                   side only, with build.py's flags; keeps <outdir>/<unit>.s
    tools/devcode_diff.py cmp <outdirA> <outdirB>  compare the two, per kernel symbol (emission order may differ): the sets of
                                                   symbols, each function's text with the compiler-local labels renumbered, each
                                                   kernel's descriptor and its VGPR / AGPR / SGPR / LDS / scratch figures.
                                                   Prints a markdown table; exit status 1 if anything differs
"""
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys

FIGURES = ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')


def _build_py(tree):
    spec = importlib.util.spec_from_file_location('bm_build', os.path.join(tree, 'boltzmann_machines_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def asm(tree, outdir):
    b = _build_py(tree)
    os.makedirs(outdir, exist_ok=True)
    flags = [f for f in b.FLAGS if f != '-shared']

    def one(src):
        out = os.path.join(outdir, os.path.splitext(src)[0] + '.s')
        cmd = ['/opt/rocm/bin/hipcc'] + flags + ['--cuda-device-only', '-S', os.path.join(b.CSRC, src), '-o', out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return src, r.returncode, r.stdout

    bad = 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, len(b.SOURCES))) as ex:
        for src, rc, log in ex.map(one, b.SOURCES):
            print('%-24s %s' % (src, 'ok' if rc == 0 else 'FAILED\n' + log))
            bad |= rc != 0
    return int(bad)


def parse(path):
    """{symbol: text} of every function (labels renumbered, comments dropped; a kernel's text includes its descriptor) and
    {kernel symbol: figures}"""
    s = open(path).read()
    local = re.compile(r'\.L([A-Za-z_]+)\d+(_\d+)?')           # .LBB<function index>_<block>, .Lfunc_end<index>, ...
    funcs = {}
    for m in re.finditer(r'^\t\.type\t(\S+),@function\n(.*?)^\t\.size\t\1,[^\n]*\n', s, re.S | re.M):
        lines = (re.sub(r'\s*;.*', '', ln).rstrip() for ln in m.group(2).split('\n'))
        funcs[m.group(1)] = '\n'.join(local.sub(lambda q: '.L%s%s' % (q.group(1), q.group(2) or ''), ln) for ln in lines if ln)
    for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel', s, re.S | re.M):
        funcs[m.group(1)] = funcs.get(m.group(1), '') + '\n' + re.sub(r'[ \t]*;[^\n]*', '', m.group(2))
    figs = {}
    # (one metadata entry per kernel: its keys are sorted, .agpr_count first and .wavefront_size last - as tools/resusage.sh reads them;
    #  the kernel counts of the table would show it if that changed)
    for m in re.finditer(r'- \.agpr_count:.*?\.wavefront_size', s, re.S):
        blk = m.group(0)
        get = lambda k: re.search(r'\.%s:\s+(\S+)' % k, blk).group(1)
        figs[get('name')] = tuple(get(k) for k in FIGURES)
    return funcs, figs


def cmp(da, db):
    units = sorted(set(f for d in (da, db) for f in os.listdir(d) if f.endswith('.s')))
    print('| unit | kernels, A | kernels, B | symbols in one only | kernels whose instructions differ | kernels whose VGPR / AGPR / SGPR / LDS / scratch figures differ |')
    print('|---|---|---|---|---|---|')
    total, detail = 0, []
    for u in units:
        pa, pb = os.path.join(da, u), os.path.join(db, u)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print('| `%s` | %s | %s | - | - | - |' % (u[:-2] + '.hip', 'yes' if os.path.exists(pa) else 'missing', 'yes' if os.path.exists(pb) else 'missing'))
            total += 1
            continue
        (fa, ga), (fb, gb) = parse(pa), parse(pb)
        only = sorted(set(fa) ^ set(fb))
        text = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
        figs = sorted(k for k in set(ga) & set(gb) if ga[k] != gb[k])
        print('| `%s` | %d | %d | %d | %d | %d |' % (u[:-2] + '.hip', len(ga), len(gb), len(only), len(text), len(figs)))
        total += len(only) + len(text) + len(figs)
        detail += ['%s: %s: %s' % (u, what, k) for what, ks in (('in one only', only), ('instructions', text), ('figures', figs)) for k in ks]
    if detail:
        out = subprocess.run(['c++filt'], input='\n'.join(detail), capture_output=True, text=True).stdout
        print('\n' + out)
    return int(total != 0)


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] in ('asm', 'cmp'):
        sys.exit((asm if sys.argv[1] == 'asm' else cmp)(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
