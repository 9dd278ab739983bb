"""The numpy restatement of the dense-head contract (tests/dense_cases.py) through the very cases tests/test_gpu_dense.py applies to the
kernels, and the planted bugs those cases must reject; the restatement against its own bounds; the planner against the axis formula and the
GEMM planner over the head shapes; plus the declarations, exports and struct layouts of the new C-ABI and the build checks of
csrc/dense.hip (kernel descriptors and instruction streams only).  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_cases as dc
from test_kernel_build_checks import HIPCC, MISC_FLAGS, ROOT, compile_misc_both_ways, fused_kernels, misc_instruction_streams

SYMBOLS = ["dinov2_hip_dense_head_create", "dinov2_hip_dense_head_free", "dinov2_hip_predict_dense"]
OPS = ["dinov2_hip_op_dense_reduce", "dinov2_hip_op_dense_pack", "dinov2_hip_op_dense_reduce_plan"]
EPI_PLAIN_F32 = 5


def _failures(mutant):
    if mutant in dc.LOGIT_MUTANTS:
        return dc.logit_failures(lambda c: dc.emulate_logits_case(c, mutant))
    return dc.reduce_failures(lambda L, h0, w0, oh, ow, red, cen, eps: dc.emulate(L, h0, w0, oh, ow, red, cen, eps, mutant))


def test_restatement_passes_every_case():
    assert _failures(None) == [] and dc.logit_failures(dc.emulate_logits_case) == []


@pytest.mark.parametrize("mutant", dc.MUTANTS)
def test_planted_bugs_are_rejected(mutant):
    assert _failures(mutant), f"planted bug {mutant} passed every case"


def test_cases_are_well_formed():
    assert set(dc.MUTANTS) == set(dc.REDUCE_MUTANTS) | set(dc.LOGIT_MUTANTS) and len(dc.MUTANTS) == 13
    grids = {s[:2] for s in dc.SHAPES}
    assert {(1, 1), (3, 3), (4, 6)} <= grids and set(dc.CLASSES) == {2, 21, 150, 256}
    for want in ((4, 6, 56, 84), (4, 6, 50, 77), (4, 6, 16, 24), (4, 6, 2, 3)):  # scale 14, non-integer, dyadic 4, downscale
        assert want in dc.SHAPES
    names = [p[0] for p in dc.exact_probes()]
    assert any(n.startswith("integer-") for n in names) and {"tie-3-7", "tie-minus-zero", "argmax-after-interpolation", "bins-all-negative"} <= set(names)
    # the logit cases reach every switch a logit mutant turns
    cases = dc.LOGIT_CASES
    assert any(c[5] for c in cases) and any(c[6] for c in cases) and any(len(c[4]) > 1 for c in cases)


@pytest.mark.parametrize("C_", dc.CLASSES)
def test_restatement_sits_inside_the_bounds_with_room(C_):
    """Gaussian operands: the float32 logits restatement within three quarters of logits_bound, and from there the float32 interpolation
    and the BINS expectation within three quarters of val_bound / bins_bound, against the float64 pipeline of the float64 logits."""
    rng = np.random.default_rng(C_)
    h0, w0, oh, ow, K = 4, 6, 50, 77, 512
    A = rng.standard_normal((h0 * w0, K)).astype(np.float16)
    W, bias = dc.head_weights(C_, K, 5)
    ref, bound = dc.logits_reference(A, W, bias)
    L = dc.logits_emulate(A, W, bias)
    assert (np.abs(L - ref) <= 0.75 * bound).all()
    vb = dc.val_bound(bound, np.abs(ref), h0, w0, oh, ow)
    val = dc.interpolate(L, h0, w0, oh, ow).astype(np.float64)
    assert (np.abs(val - dc.reference(ref, h0, w0, oh, ow)["val"]) <= 0.75 * vb).all()
    cen = dc.bin_centers(C_)
    got = dc.emulate(L, h0, w0, oh, ow, dc.BINS, cen, 0.1)["value"].astype(np.float64)
    d64 = dc.reference(ref, h0, w0, oh, ow, dc.BINS, cen, 0.1)["value"]
    tol = dc.bins_bound(bound, ref, h0, w0, oh, ow, cen, 0.1)
    assert (np.abs(got - d64) <= 0.75 * tol).all(), float((np.abs(got - d64) / tol).max())


def test_margin_excludes_few_pixels_of_gaussian_logits():
    """numpy alone: for Gaussian low-resolution logits of standard deviation 4 on these grids, a top-2 margin of 1e-2 -- above twice the
    bound of every case of tests/test_gpu_dense.py, which is about K 2^-24 sum |a w| < 4e-3 -- excludes about 1 % of the pixels at C = 256
    and fewer below, so the 2 % cap asserted there has room."""
    for (h0, w0, oh, ow) in ((5, 5, 70, 70), (4, 6, 56, 84), (3, 3, 42, 42), (4, 6, 16, 24)):
        for C_ in dc.CLASSES:
            m = np.concatenate([dc.reference(dc.gaussian_logits(h0 * w0, C_, s), h0, w0, oh, ow)["margin"].ravel() for s in range(4)])
            assert (m <= 1e-2).mean() <= 0.02, (h0, w0, oh, ow, C_, float((m <= 1e-2).mean()))


# ------------------------------------------------------------------------------------------------------------------- planners
def test_reduce_planner_covers_every_tile_within_the_lds_budget(api):
    hdr = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert "DENSE_LDS_BUDGET = (size_t)64 << 10" in hdr and "DENSE_C_MAX = 256" in hdr and "DENSE_OUT_MAX = 8192" in hdr
    cases = [s + (C_,) for s in dc.SHAPES for C_ in dc.CLASSES]
    cases += [(37, 37, 518, 518, 150), (37, 37, 148, 148, 256), (37, 37, 8192, 8192, 256), (64, 64, 1, 1, 256), (100, 3, 7, 8192, 256),
              (37, 37, 37, 37, 2), (585, 585, 8192, 8192, 256), (585, 585, 16, 16, 256)]
    for h0, w0, oh, ow, C_ in cases:
        p = api.dense_reduce_plan(h0, w0, C_, oh, ow)
        assert p["lds_bytes"] <= 64 << 10 and p["pitch"] % 4 == 0 and (p["pitch"] // 4) % 2 == 1 and p["pitch"] >= C_, p
        assert p["lds_bytes"] == p["span_y"] * p["span_x"] * p["pitch"] * 4 + (C_ + 3) // 4 * 16 + (p["tile_y"] * p["tile_x"] + 15) // 16 * 16
        for n_in, n_out, tile, span in ((h0, oh, p["tile_y"], p["span_y"]), (w0, ow, p["tile_x"], p["span_x"])):
            i0, i1, _ = dc.axis(n_in, n_out)  # the restated axis formula: every tile's rows lie inside the span the planner reserved
            need = max(int(i1[min(d + tile, n_out) - 1] - i0[d]) + 1 for d in range(0, n_out, tile))
            assert need == span, (h0, w0, oh, ow, C_, need, span)
    for bad in ((0, 1, 2, 1, 1), (1, 1, 257, 1, 1), (1, 1, 2, 8193, 1), (1, 1, 2, 1, 0)):
        with pytest.raises(ValueError):
            api.dense_reduce_plan(*bad)


def test_every_head_shape_gets_a_gemm_plan(api):
    """launch_gemm(DT_F16, EPI_PLAIN_F32) with M = B P, N = C padded to 128, K = n_layers H (1 + concat_cls): the shapes of the tests and ViT-L
    at 518 px, batch 32 and 1, C = 150 and 256, K = 1 024, 4 096 and 8 192.  No device."""
    cpad = lambda c: (c + 127) // 128 * 128
    shapes = set()
    for B in (1, 2, 3):
        for P in (9, 24, 25):
            for C_ in dc.CLASSES + (5,):
                for K in (128, 256, 512):
                    shapes.add((B * P, cpad(C_), K))
    for B in (1, 32):
        for C_ in (150, 256):
            for K in (1024, 4096, 8192):
                shapes.add((B * 1369, cpad(C_), K))
    for M, N, K in sorted(shapes):
        assert api.gemm_plan(0, EPI_PLAIN_F32, M, N, K), (M, N, K)


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (fails before this feature: the symbols are not there)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\(" % name, hdr), name
    for name in OPS:
        assert re.search(r"\bint %s\(" % name, ops), name
    assert "typedef struct dinov2_hip_dense_desc" in hdr and "typedef struct dinov2_hip_dense_out" in hdr
    assert "typedef struct dinov2_hip_dense_head dinov2_hip_dense_head;" in hdr
    assert "#define DINOV2_HIP_ABI_VERSION 1" in hdr or api.lib().dinov2_hip_abi_version() == 1
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert set(SYMBOLS) | set(OPS) <= exported


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    sec = hdr[hdr.index("linear dense-prediction heads"):hdr.index("int dinov2_hip_predict_dense(")]
    for text in ("no reference counterpart", "linear_head.py", "s = gamma / sqrt(var + eps)", "W' = W diag(s)", "b' = b + W (beta - mean * s)",
                 "round to nearest even", "layer-major, patch then cls", "whatever the", "within the f16 range", "depends on K alone",
                 "bit-identical whatever batch", "align_corners=False", "scale = (float)n_in / (float)n_out", "max(scale * (dst + 0.5f) - 0.5f, 0)",
                 "min(i0 + 1, n_in - 1)", "rounded on its own", "fused multiply-add", "LOWEST class", "-0 equals +0", "never before it",
                 "max(val_c, 0) + eps", "ascending c", "correctly rounded division", "launch geometry", "Out of scope", "C > 256",
                 "softmax probabilities", "dinov2_compat.hpp", "4 h0 x 4 w0", "sliding-window", "mmseg",
                 "before anything is launched, allocated or copied", "once per pass", "runs eagerly under DINOV2_HIP_GRAPHS=1",
                 "profiles/dense_head.md"):
        assert text in sec, text


def test_ctypes_structs_match_the_header(api, tmp_path):
    cxx = "g++"  # as tests/test_bank_probes.py: no guard, a missing compiler fails
    layouts = {"dinov2_hip_dense_desc": (api.DenseDesc, ["layers", "n_layers", "norm", "concat_cls", "num_classes", "weight", "bias", "reduce",
                                                         "bin_centers", "bins_eps", "reserved"]),
               "dinov2_hip_dense_out": (api.DenseOut, ["out_h", "out_w", "labels", "value", "logits", "on_device", "reserved"])}
    body = ""
    for name, (_, fields) in layouts.items():
        body += 'std::printf(" %%zu", sizeof(%s));\n' % name + "".join('std::printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in fields)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    exe = tmp_path / "sz"
    subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, (T, fields) in layouts.items():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert got == want
    assert (api.DENSE_ARGMAX, api.DENSE_BINS) == (0, 1)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "dinov2_hip.h"\nint main(void) { dinov2_hip_dense_desc d = {0}; dinov2_hip_dense_out o = {0};\n'
                   '    int (*f)(dinov2_hip_session *, const dinov2_hip_input *, dinov2_hip_output *, const dinov2_hip_dense_head *,\n'
                   '             const dinov2_hip_dense_out *, uint32_t, char *, size_t) = dinov2_hip_predict_dense;\n'
                   '    int (*g)(dinov2_hip_model *, const dinov2_hip_dense_desc *, dinov2_hip_dense_head **, char *, size_t) = dinov2_hip_dense_head_create;\n'
                   '    void (*h)(dinov2_hip_dense_head *) = dinov2_hip_dense_head_free;\n'
                   '    d.reduce = DINOV2_HIP_DENSE_BINS;\n'
                   '    return d.n_layers + o.out_h + (f ? 0 : 1) + (g ? 0 : 1) + (h ? 0 : 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                   check=True, capture_output=True, timeout=120)


def test_fold_batchnorm_equals_batchnorm_then_linear(api):
    rng = np.random.default_rng(3)
    C_, K = 7, 40
    W, b = rng.standard_normal((C_, K)), rng.standard_normal(C_)
    g, bt, mu, var = rng.standard_normal(K), rng.standard_normal(K), rng.standard_normal(K), rng.random(K) + 0.5
    x = rng.standard_normal((11, K))
    want = ((x - mu) / np.sqrt(var + 1e-5) * g + bt) @ W.T + b
    W2, b2 = api.fold_batchnorm(W, b, g, bt, mu, var, 1e-5)
    assert W2.dtype == np.float32 and b2.dtype == np.float32
    assert np.abs(x @ W2.astype(np.float64).T + b2 - want).max() < 1e-4
    W3, b3 = api.fold_batchnorm(W, None, g, bt, mu, var, 1e-5)
    assert np.abs(b3 - (b2 - b.astype(np.float32))).max() < 1e-5 and np.array_equal(W3, W2)


# ------------------------------------------------------------------------------------------------------------------- build checks
@pytest.fixture(scope="module")
def dense_asm(tmp_path_factory):
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "dense.hip")
    return compile_misc_both_ways(src, str(tmp_path_factory.mktemp("denseasm")))


def test_dense_cross_compiles_without_scratch(dense_asm):
    """csrc/dense.hip compiles for gfx950 with the Makefile's flags; every kernel has private segment size 0 and at most 256 VGPRs (read
    from the kernel descriptors); the reduction reads its rows 16 bytes at a time and the packing stores 16 bytes."""
    assert MISC_FLAGS and os.path.exists(HIPCC)
    txt = dense_asm[0]
    names = []
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256, name
        names.append(name)
    assert len(names) == 8 and sum("dense_pack_kernel" in n for n in names) == 6 and sum("dense_reduce_kernel" in n for n in names) == 2, names
    streams = misc_instruction_streams(txt)
    for name, ins in streams.items():
        ops = {i.split()[0] for i in ins}
        assert not any(o.startswith("scratch_") for o in ops), name
        if "dense_reduce_kernel" in name:
            assert {"ds_read_b128", "ds_write_b128", "global_load_dwordx4"} <= ops, (name, sorted(ops))
        else:
            assert "global_store_dwordx4" in ops and "global_store_short" not in ops, (name, sorted(ops))
    # the row routine has one source
    src = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "dense.hip")).read()
    misc = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels_misc.hip")).read()
    assert '#include "ln_row.h"' in src and '#include "ln_row.h"' in misc and "ln_row_scale(" not in src.replace("ln_row.h", "")
    assert "static __device__ __forceinline__ float ln_row_scale" not in misc


def test_dense_kernels_keep_their_rounding_points(dense_asm):
    """dense_reduce_kernel (contracts 3 - 5: no fused multiply-add) and dense_pack_kernel (the LayerNorm's rounding points) compile to the same
    instruction stream with and without -ffp-contract=off."""
    fused, n = fused_kernels(*dense_asm, pattern=r"dense_\w+_kernel")
    assert n == 8, n
    assert not fused, "contracted into FMAs: %s" % fused
