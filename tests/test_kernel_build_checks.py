"""Build-time checks of the hand-ordered GEMM K loop: csrc/gemm4.hip writes its K loop as `asm volatile` statements that the
compiler's scheduler, waitcnt insertion and hazard recogniser cannot see into -- correctness and speed rest on hipcc only ALLOCATING registers
there.  This test cross-compiles the file for gfx950 (no GPU needed), finds the steady-state K loop of every gemm4 kernel in the assembly (the
basic block with 256 MFMAs that branches back to itself: two K-tiles) and asserts that it is exactly the stream the source spells out: nothing
but the 256 MFMAs, the 64 fragment reads, the 32 LDS-DMA pieces with their M0 set-up, the counted waits and four barriers -- no scratch
access, no v_accvgpr / v_mov traffic (a spill or a copy of a fragment register between its ds_read and its s_waitcnt would read stale data
silently), no vector ALU at all."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

ALLOWED = {"v_mfma_f32_16x16x32_f16", "v_mfma_f32_16x16x32_bf16", "ds_read_b128", "global_load_lds_dwordx4", "s_add_u32", "s_addc_u32", "s_add_i32",
           "s_nop", "s_waitcnt", "s_barrier", "s_cmp_ge_i32", "s_cmp_lt_i32", "s_cbranch_scc0", "s_cbranch_scc1", "s_mov_b32", "s_mov_b64"}


@pytest.fixture(scope="module")
def gemm4_asm(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asm") / "gemm4.s"
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "gemm4.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-lambda-capture", "-x", "hip", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    return out.read_text()


def _functions(txt):
    for f in re.split(r"\n(?=_ZN6dinov2\w+:\s)", txt):
        name = f.split(":", 1)[0]
        if name.startswith("_ZN6dinov2") and "gemm4" in name and "kernel" in name:
            yield name, f


def _blocks(body):
    lab, cur = None, []
    for line in body.splitlines():
        s = line.strip()
        if re.match(r"^\.LBB\d+_\d+:", s):
            if cur:
                yield lab, cur
            lab, cur = s.split(":")[0], []
        elif s and not s.startswith(";") and not s.startswith("."):
            cur.append(s.split(";")[0].strip())
    if cur:
        yield lab, cur


def test_gemm4_steady_state_k_loop_is_the_hand_written_stream(gemm4_asm):
    seen = 0
    for name, body in _functions(gemm4_asm):
        loops = [(lab, b) for lab, b in _blocks(body)
                 if sum(x.startswith("v_mfma") for x in b) >= 200 and any(x.startswith("s_cbranch") and lab in x for x in b)]
        if "Li8EEE" not in name and "mixed" not in name:
            continue  # (short one-tile-per-workgroup instantiations, NI = 2 / 3 / 4: their K-tiles have 32 - 64 MFMAs; same macros)
        assert len(loops) >= 1, name
        for lab, b in loops:
            ops = collections.Counter(x.split()[0] for x in b)
            assert set(ops) <= ALLOWED, (name, lab, sorted(set(ops) - ALLOWED))
            nm = ops["v_mfma_f32_16x16x32_f16"] + ops["v_mfma_f32_16x16x32_bf16"]
            assert nm in (256, 192), (name, lab, nm)  # two K-tiles of the 256-row body (128 MFMAs each) or of the 192-row body (96)
            assert ops["ds_read_b128"] == (64 if nm == 256 else 56), (name, lab, ops["ds_read_b128"])
            assert ops["global_load_lds_dwordx4"] == (32 if nm == 256 else 28), (name, lab, ops["global_load_lds_dwordx4"])
            assert ops["s_barrier"] == 4 and ops["s_waitcnt"] == 6, (name, lab, dict(ops))
            seen += 1
    assert seen >= 20  # 2 dtypes x 5 epilogues x (plain kernel: one loop; mixed kernel: the 256- and the 192-row body)


def test_gemm4_kernels_use_the_whole_register_file_and_little_scratch(gemm4_asm):
    """512 registers per lane (256 accumulators + fragments): one wave per SIMD by construction.  Scratch: the residual epilogue keeps three
    passes of residual rows in flight next to the next tile's fragments and spills a handful of registers OUTSIDE the K loop (checked
    above); anything beyond that would be a regression of the register budget."""
    n = 0
    for m in re.finditer(r"\.amdhsa_kernel (_ZN6dinov2\w+)(.*?)\.end_amdhsa_kernel", gemm4_asm, re.S):
        name, desc = m.group(1), m.group(2)
        if "gemm4" not in name:
            continue
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1))
        nvgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
        assert scratch <= 64, (name, scratch)
        if "Li8EEE" in name or "mixed" in name:
            assert 440 <= nvgpr <= 512, (name, nvgpr)
        n += 1
    assert n >= 20


def _regs(tok):
    """VGPR numbers named by an operand token: v12 -> {12}, v[24:27] -> {24, 25, 26, 27}; anything else -> {}."""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def test_gemm4_no_instruction_touches_a_fragment_before_its_wait(gemm4_asm):
    """The fragment reads are `asm volatile("ds_read_b128 ...")` statements whose s_waitcnt is ANOTHER statement: to the compiler the output
    register holds its value the moment the statement ends.  Anything it places in between that reads or moves such a register -- a spill,
    an AGPR park, a copy -- picks up whatever the register held BEFORE the LDS data arrived.  Round 6 hit exactly that: under the register
    pressure of the first EPI_QKV_LN epilogue hipcc spilled Pw[3] right behind its ds_read (scratch_store two lines later, the wait after it);
    every tile lost its first k-step in sixteen columns.  Checked here for every gemm4 kernel, over the whole function: between a
    ds_read_b128 and the next `s_waitcnt lgkmcnt(0)` no other instruction may name the destination registers."""
    checked = 0
    for name, body in _functions(gemm4_asm):
        pending = set()
        for line in body.splitlines():
            s = line.split(";")[0].strip()
            if not s or s.startswith(".") or s.endswith(":"):
                continue
            op, _, rest = s.partition(" ")
            toks = [t.strip() for t in rest.split(",")] if rest else []
            if op == "s_waitcnt" and "lgkmcnt(0)" in rest:
                pending.clear()
                continue
            if op == "ds_read_b128":
                pending |= _regs(toks[0])
                checked += 1
                continue
            if pending:
                used = set()
                for t in toks:
                    used |= _regs(t.split(" ")[0])
                assert not (used & pending), (name, s, sorted(used & pending))
    assert checked > 1000


# ------------------------------------------------------------------------------------------------------------- kernels_misc.hip
MISC_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-Wno-unused-lambda-capture"]  # the Makefile's


def misc_instruction_streams(asm_text):
    """kernel name -> its instructions (comments and directives dropped, branch labels numbered per function)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm_text, re.S | re.M):
        ins = []
        for line in m.group(2).splitlines():
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                ins.append(re.sub(r"\.LBB\d+_(\d+)", r"L\1", s))
        out[m.group(1)] = ins
    return out


def compile_misc_both_ways(src, outdir):
    """Cross-compile `src` with the Makefile's flags and again with -ffp-contract=off (in parallel): (default, contract-off) asm."""
    outs = [os.path.join(outdir, "misc_default.s"), os.path.join(outdir, "misc_nocontract.s")]
    procs = [subprocess.Popen([HIPCC, *MISC_FLAGS, *extra, "-x", "hip", "-S", "--cuda-device-only", src, "-o", o],
                              stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
             for o, extra in zip(outs, ([], ["-ffp-contract=off"]))]
    for p in procs:
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, err.decode(errors="replace")[-2000:]
    return tuple(open(o).read() for o in outs)


def fused_kernels(asm_default, asm_nocontract, pattern=r"preprocess_u8_kernel|layernorm_kernel"):
    """Kernels matching `pattern` whose instruction stream changes when contraction is switched off, and how many matched."""
    a, b = misc_instruction_streams(asm_default), misc_instruction_streams(asm_nocontract)
    names = [n for n in a if re.search(pattern, n)]
    return [n for n in names if a[n] != b.get(n)], len(names)


def test_misc_kernels_keep_their_rounding_points(tmp_path):
    """preprocess_u8_kernel (bit-equal to the host preprocess, which has no FMA) and every layernorm_kernel instance (ggml's three
    rounding points) must compile to the same instruction stream with and without -ffp-contract=off: hipcc fused nothing the source
    writes as separate operations -- including in helpers they inline (cubic_taps_dev was one).  On the tree before the two
    `fp contract(off)` pragmas this failed for all ten kernels."""
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels_misc.hip")
    fused, n = fused_kernels(*compile_misc_both_ways(src, str(tmp_path)))
    assert n == 10, n  # preprocess_u8_kernel + layernorm_kernel<f32 | f16 | bf16, MAXV 2 | 4 | 8>
    assert not fused, "contracted into FMAs: %s" % fused


# ------------------------------------------------------------------------------------------------------------- gemm_epilogue.h
def test_gemm_epilogue_arithmetic_has_a_single_source():
    """The three GEMM kernel files must give an accumulator the same bits, so the epilogue arithmetic is written once, in
    csrc/gemm_epilogue.h, and gemm.hip, gemm2.hip and gemm4.hip include it.  Its fingerprints -- the two GELU constants, the SwiGLU's
    `__expf(`, the 16-byte store macro -- may not reappear in any other file of csrc/.  (attention.hip's softmax has exponentials of its
    own, `__expf(` among them; it includes nothing of this and is the one file the `__expf(` count leaves out.)"""
    csrc = os.path.join(ROOT, "dinov2.cpp_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f))}
    assert "gemm_epilogue.h" in text
    for needle in ("0.1029432397", "2.302208199", "__expf("):
        holders = [f for f, t in text.items() if needle in t and not (needle == "__expf(" and f == "attention.hip")]
        assert holders == ["gemm_epilogue.h"], (needle, holders)
    for f in ("gemm.hip", "gemm2.hip", "gemm4.hip"):
        assert re.search(r'^#include "gemm_epilogue\.h"', text[f], re.M), f
    assert "gemm_epilogue.h" not in text["attention.hip"]
    for needle in ("#define DINO2_ST16", "#define DINO4_ST16"):
        assert not [f for f, t in text.items() if needle in t], needle


# ------------------------------------------------------------------------------------------------------------------ sim_tile.h
def test_similarity_tile_and_its_order_have_a_single_source():
    """match, bank top-k and k-means must give a pair the same similarity bits and choose by the same total order, so the 128 x 128 tile
    (staging addresses, swizzled LDS image, K loop, MFMAs) and the order are written once, in csrc/sim_tile.h, which match.hip, bank.hip and
    kmeans.hip include.  The tile's fingerprints -- the swizzle of the LDS destination, the chunk expression of the fragment reads, the
    MFMA call -- and a definition of the pair type or of a comparison may not reappear in those three files."""
    csrc = os.path.join(ROOT, "dinov2.cpp_amd", "csrc")
    assert os.path.isfile(os.path.join(csrc, "sim_tile.h"))
    header = open(os.path.join(csrc, "sim_tile.h")).read()
    for needle in ("(row >> 1) & 7)) << 4", "^ p.sw) << 4", "mfma16(", "bool before("):
        assert needle in header, needle
    for f in ("match.hip", "bank.hip", "kmeans.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert re.search(r'^#include "sim_tile\.h"', text, re.M), f
        for needle in ("(row >> 1) & 7)) << 4", "^ sw) << 4", "^ p.sw) << 4", "mfma16(", "struct Best", "bool better(", "bool before("):
            assert needle not in text, (f, needle)
