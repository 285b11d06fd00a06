"""CPU-only (hipcc cross-compiles): per-kernel register / spill / scratch report of every HIP source, and the list of
`s_waitcnt vmcnt(0)` that sit inside loops of the hot kernels.  Why it exists: vector memory retires in order on gfx950, so
a scratch reload -- or any load the compiler cannot count precisely -- placed after a burst of stores waits for the stores'
acknowledgements; round 1 lost a third of the reconstruction kernel to exactly that.

  python tools/isa_lint.py            # table; exit code 1 if a product kernel spills or touches scratch
  python tools/isa_lint.py --against <commit>
                                      # a refactor's proof: every kernel source compiled from <commit> and from this tree with the
                                      # build's flags gives the same device and host assembly; exit code 1 on any difference
"""
import os
import re
import subprocess
import sys
import shutil
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from synergynet_amd.build import CFLAGS, CSRC, SOURCES  # noqa: E402

HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def main():
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        for src in SOURCES:
            if src == 'synergy_abi.hip':
                continue
            out = os.path.join(td, src + '.s')
            r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-w',
                                '-I' + os.path.join(ROOT, 'include'), '-o', out, os.path.join(CSRC, src)],
                               capture_output=True, text=True)
            if r.returncode:
                print(src, 'FAILED TO COMPILE\n', r.stderr[-2000:])
                bad += 1
                continue
            text = open(out).read()
            print(f'== {src}')
            for m in re.finditer(r'\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n'
                                 r'\s+\.vgpr_spill_count:\s+(\d+)', text):
                name, scratch, vgpr, spill = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
                dem = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
                short = re.sub(r'\(.*', '', dem)[:110]
                flag = ''
                if scratch or spill:
                    # PROF = second template argument of the fused-block kernels, third of the reconstruction kernel
                    is_prof = bool(re.search(r'(fused_block_\w+<.*>, true(, \d+)?(, (true|false))?>$)|(recon_f16_kernel<\d+, (true|false), true>$)', short))
                    flag = '  <-- spills (profiling instantiation)' if is_prof else '  <-- SPILLS / SCRATCH'
                    bad += 0 if is_prof else 1
                print(f'   {vgpr:4d} vgprs {spill:4d} spilled {scratch:5d} B scratch  {short}{flag}')
    print('product kernels with spills or scratch:', bad)
    return 1 if bad else 0


def _first_difference(a, b):
    """(symbol, line of a, line of b) at the first line where two assembly texts part; symbol = the last non-local label above it."""
    sym = '(file header)'
    la, lb = a.split('\n'), b.split('\n')
    for x, y in zip(la, lb):
        if x != y:
            return sym, x.strip(), y.strip()
        m = re.match(r'([A-Za-z_$][\w.$]*):', x)
        if m:
            sym = m.group(1)
    return sym, f'({len(la)} lines)', f'({len(lb)} lines)'


def against(commit):
    """Assembly of every kernel source at `commit` against this tree's: same flags as the build, device pass and host pass apart.  The only
    thing that legitimately differs is the id of up to 16 hex digits that hipcc derives from a compilation unit's path and text
    (__hip_cuid_<id>, __hip_gpubin_handle_<id>, __hip_fatbin_<id>): replaced by a fixed token.  The output carries no line information."""
    from concurrent.futures import ThreadPoolExecutor
    passes = (('device', ['--cuda-device-only']), ('host', ['--cuda-host-only']))
    with tempfile.TemporaryDirectory() as td:
        old = os.path.join(td, 'old')
        os.makedirs(old)
        ar = subprocess.run(['git', '-C', ROOT, 'archive', commit, 'synergynet_amd/csrc', 'include'], capture_output=True)
        if ar.returncode:
            print(ar.stderr.decode()[-2000:])
            return 1
        subprocess.run(['tar', '-x', '-C', old], input=ar.stdout, check=True)
        trees = {'old': os.path.join(old, 'synergynet_amd', 'csrc'), 'new': CSRC}
        srcs = [s for s in SOURCES if '__global__' in open(os.path.join(CSRC, s)).read()]

        def asm(job):
            src, tree, (pname, pflags) = job
            sp = os.path.join(trees[tree], src)
            if not os.path.isfile(sp):
                return job, None, f'{src}: not in the {tree} tree'
            out = os.path.join(td, f'{tree}.{pname}.{src}.s')
            r = subprocess.run([HIPCC] + CFLAGS + ['-w', '-S'] + pflags + ['-o', out, sp], capture_output=True, text=True)
            if r.returncode:
                return job, None, r.stderr[-2000:]
            return job, re.sub(r'\b(__hip_cuid_|__hip_gpubin_handle_|__hip_fatbin_)[0-9a-f]{1,16}\b', r'\1ID', open(out).read()), ''

        jobs = [(s, t, p) for s in srcs for t in ('old', 'new') for p in passes]
        with ThreadPoolExecutor(max_workers=16) as ex:
            got = {(j[0], j[1], j[2][0]): (text, err) for j, text, err in ex.map(asm, jobs)}
    bad = 0
    for src in srcs:
        for pname, _ in passes:
            (a, ea), (b, eb) = got[src, 'old', pname], got[src, 'new', pname]
            if a is None or b is None:
                print(f'{src:26s} {pname:6s} FAILED TO COMPILE\n{ea or eb}')
                bad += 1
            elif a == b:
                print(f'{src:26s} {pname:6s} identical  ({a.count(chr(10))} lines)')
            else:
                sym, x, y = _first_difference(a, b)
                dem = subprocess.run(['c++filt', sym], capture_output=True, text=True).stdout.strip() or sym
                print(f'{src:26s} {pname:6s} DIFFERS first in {dem[:160]}\n      {commit}: {x[:160]}\n      this tree: {y[:160]}')
                bad += 1
    print(f'{len(srcs)} kernel sources against {commit}:', 'identical device and host assembly' if not bad else f'{bad} differences')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--against':
        sys.exit(against(sys.argv[2]))
    if len(sys.argv) > 1:
        sys.exit(__doc__)
    sys.exit(main())
