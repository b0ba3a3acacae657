"""Register, LDS and scratch budgets of the kernels whose occupancy the decode's speed rests on
(DESIGN.md sections 3a, 6l), read from the metadata of the gfx950 code object inside the built
libldgpu.so: resource figures only, no instructions.  An occupancy step lost to a later edit
fails here instead of showing up as a slower benchmark.

The VGPR allocation granule is 8 and a SIMD holds 512, so waves per SIMD = 512 // (VGPRs rounded
up to 8), at most 8: <= 64 -> 8, 72 -> 7, 80 -> 6, 96 -> 5, 128 -> 4.  A CU has 163,840 B of LDS;
a kernel that is to keep `w` workgroups resident on a CU needs w x its LDS within that.

ldg_k_final_lines is budgeted at the step it runs at, 6 waves (<= 80 VGPRs, 6 x LDS): the 7-wave
build (65 VGPRs, 7 x 22,944 B) was measured and dropped, its CU-busy cycles rose by 2.9%
(section 6l).  The SGPR-spill ceilings are what the build has; they may only fall.

Not a GPU test; skipped where the LLVM tools that read a code object are not installed."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), 'ld-decode_amd', 'ldgpu', 'libldgpu.so')
LDS_PER_CU = 163840
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'

# kernel: (max VGPRs, workgroups per CU its LDS must allow, max spilled SGPRs)
BUDGET = {
    'ldg_k_hsync_lines': (64, 1, 0),
    'ldg_k_final_lines': (80, 6, 8),
    'ldg_k_final_lines_div': (80, 6, 8),
    'ldg_k_sync_walk': (80, 1, 0),
    'ldg_k_burst_lines': (96, 1, 0),
    'ldg_k_comb_fused': (80, 6, 0),
    'ldg_k_demod': (128, 1, 6),
    'ldg_k_demod_iso': (128, 1, 7),
    'ldg_k_demod_iso_cut': (128, 1, 6),
    'ldg_k_demod_probe': (128, 1, 7),
}


def _tool(name):
    for d in (os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin'), None):
        p = shutil.which(name, path=d) if d else shutil.which(name)
        if p:
            return p
    return None


def parse_notes(text):
    """{kernel name: {key: value}} from llvm-readelf --notes of an AMDGPU code object."""
    out = {}
    body = text[text.index('amdhsa.kernels:'):]
    for block in re.split(r'\n  - (?=\.)', body)[1:]:
        block = block.split('\namdhsa.', 1)[0]
        kv = dict(re.findall(r'^\s{0,4}(\.\w+):\s+(\S+)\s*$', block, re.M))
        if '.name' in kv:
            out[kv['.name']] = kv
    return out


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    tools = {n: _tool(n) for n in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf')}
    if not all(tools.values()):
        pytest.skip('no hipcc toolchain (llvm-objcopy, clang-offload-bundler, llvm-readelf)')
    assert os.path.exists(LIB), 'libldgpu.so not built; run __graft_entry__.build()'
    d = tmp_path_factory.mktemp('codeobj')
    fat, co = str(d / 'fat.bin'), str(d / 'dev.co')
    subprocess.run([tools['llvm-objcopy'], '--dump-section', '.hip_fatbin=' + fat, LIB, str(d / 'rest.so')], check=True)
    subprocess.run([tools['clang-offload-bundler'], '--unbundle', '--type=o', '--input=' + fat,
                    '--targets=' + TARGET, '--output=' + co], check=True)
    notes = subprocess.run([tools['llvm-readelf'], '--notes', co], check=True, capture_output=True, text=True).stdout
    return parse_notes(notes)


def test_parse_notes():
    """(no tools needed) The metadata reader on a two-kernel sample."""
    sample = ('amdhsa.kernels:\n  - .agpr_count:     0\n    .args:\n      - .offset:         0\n'
              '        .size:           8\n    .group_segment_fixed_size: 160\n    .name:           k_a\n'
              '    .private_segment_fixed_size: 0\n    .sgpr_count:     54\n    .sgpr_spill_count: 0\n'
              '    .symbol:         k_a.kd\n    .vgpr_count:     52\n'
              '  - .agpr_count:     0\n    .args:           []\n    .group_segment_fixed_size: 0\n'
              '    .name:           k_b\n    .vgpr_count:     98\namdhsa.target: amdgcn-amd-amdhsa--gfx950\n')
    k = parse_notes(sample)
    assert sorted(k) == ['k_a', 'k_b']
    assert k['k_a']['.vgpr_count'] == '52' and k['k_a']['.group_segment_fixed_size'] == '160'
    assert k['k_b']['.vgpr_count'] == '98'


@pytest.mark.parametrize('name', sorted(BUDGET))
def test_budget(name, kernels):
    assert name in kernels, 'kernel missing from the code object'
    k = kernels[name]
    vmax, wgs, smax = BUDGET[name]
    vgprs, agprs = int(k['.vgpr_count']), int(k['.agpr_count'])
    lds, scratch = int(k['.group_segment_fixed_size']), int(k['.private_segment_fixed_size'])
    sspill, vspill = int(k['.sgpr_spill_count']), int(k['.vgpr_spill_count'])
    print('%s: %d VGPRs (%d waves per SIMD), %d AGPRs, LDS %d B, scratch %d B, %d SGPRs spilled, %d VGPRs spilled'
          % (name, vgprs, min(8, 512 // (-(-vgprs // 8) * 8)), agprs, lds, scratch, sspill, vspill))
    assert agprs == 0
    assert vgprs <= vmax
    assert wgs * lds <= LDS_PER_CU
    assert scratch == 0 and vspill == 0
    assert sspill <= smax
