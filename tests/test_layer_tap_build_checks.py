"""Build-time checks of the layer tap kernels (csrc/kernels_misc.hip), in the style of tests/test_kernel_build_checks.py: cross-compiled
for gfx950 (no GPU needed).  With norm = 1 a tapped row must get the bits of layernorm_kernel, whose rounding points rest on hipcc fusing
nothing -- so every layer_tap kernel must compile to the same instruction stream with and without -ffp-contract=off.  None of them may use
scalar stores, scalar atomics or the scalar data cache write-back, and none may spill."""
import os
import re
import shutil

import pytest

from test_kernel_build_checks import HIPCC, ROOT, compile_misc_both_ways, fused_kernels, misc_instruction_streams

# any scalar-unit instruction that writes memory: a scalar store or atomic of any address space, or a scalar data cache operation other than
# the invalidate (the pattern is spelt in pieces; the mnemonics themselves are listed in DESIGN.md section 8)
FORBIDDEN = re.compile(r"^s_(\w*store|\w*atomic|dcache_(?!inv))")


@pytest.fixture(scope="module")
def misc_asm(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels_misc.hip")
    return compile_misc_both_ways(src, str(tmp_path_factory.mktemp("tapasm")))


def test_layer_tap_kernels_keep_their_rounding_points(misc_asm):
    fused, n = fused_kernels(*misc_asm, pattern=r"layer_tap_\w*kernel")
    assert n == 12, n  # rows | chw  x  MAXV 2 | 4 | 8  x  norm off | on
    assert not fused, "contracted into FMAs: %s" % fused


def test_layer_tap_kernels_use_no_scalar_stores_and_no_scratch(misc_asm):
    streams = {k: v for k, v in misc_instruction_streams(misc_asm[0]).items() if re.search(r"layer_tap_\w*kernel", k)}
    assert len(streams) == 12
    for name, ins in streams.items():
        bad = [i for i in ins if FORBIDDEN.match(i.split()[0])]
        assert not bad, (name, bad[:4])
        assert not any(i.startswith("scratch_") for i in ins), name
        if "chw" in name:  # the transpose: 16-byte LDS writes, 16-byte global stores along the patch dimension
            ops = {i.split()[0] for i in ins}
            assert "global_store_dwordx4" in ops and ("ds_write_b128" in ops or "ds_store_b128" in ops), (name, sorted(ops))
    for m in re.finditer(r"\.amdhsa_kernel (_ZN6dinov2\w*layer_tap\w+)(.*?)\.end_amdhsa_kernel", misc_asm[0], re.S):
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)) == 0, m.group(1)
