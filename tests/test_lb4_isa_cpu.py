"""CPU-only (hipcc cross-compiles gfx950): the features.15-17 kernels spend the registers the direct global -> LDS weight loads free on
operands requested ahead -- "as deep as compiles without scratch".  fused_block_lb4.hip compiled to assembly with the build's flags: every
lb4 kernel's metadata says ScratchSize 0 and NumVgprs <= 256 (two waves per SIMD).  Nothing else about the instruction stream is asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason='hipcc not available')
def test_lb4_kernels_use_no_scratch_and_at_most_256_vgprs(tmp_path):
    out = str(tmp_path / 'fused_block_lb4.s')
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-w', '-I' + os.path.join(ROOT, 'include'),
                        '-o', out, os.path.join(ROOT, 'synergynet_amd', 'csrc', 'fused_block_lb4.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read()
    # the resource comment block behind every kernel body: "; Kernel Name: ..." is not printed by every compiler, the symbol's .size line is
    found = {}
    for m in re.finditer(r'^\s*\.size\s+(\S+), \.Lfunc_end\d+-\S+\n(?:.*\n)*?; NumVgprs: (\d+)\n(?:.*\n)*?; ScratchSize: (\d+)\n', text, re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    lb4 = {k: v for k, v in found.items() if 'lb4' in k}
    print('\n'.join(f'{v[0]:4d} vgprs {v[1]:5d} B scratch  {k}' for k, v in sorted(lb4.items())))
    names = ' '.join(lb4)
    assert 'fused_chain_lb4_kernel' in names and names.count('fused_block_lb4_kernel') == 4 and names.count('lb4_reduce_kernel') == 2, sorted(lb4)
    bad = {k: v for k, v in lb4.items() if v[1] != 0 or v[0] > 256}
    assert not bad, bad
