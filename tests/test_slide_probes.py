"""The numpy restatement of the sliding-window contract (tests/slide_cases.py) through the very cases tests/test_gpu_slide.py applies to the
kernels, and the planted bugs those cases must reject; the window formula against mmsegmentation's loop; the restatement against float64 and
against the upstream procedure in torch on the CPU; the planner; the declarations, exports and struct layout of the new C-ABI; and the build
checks of csrc/slide.hip (kernel descriptors and instruction streams only).  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_cases as dc
import slide_cases as sl
from test_kernel_build_checks import HIPCC, MISC_FLAGS, ROOT, compile_misc_both_ways, fused_kernels, misc_instruction_streams

SYMBOLS = ["dinov2_hip_slide_windows", "dinov2_hip_predict_dense_slide"]
OPS = ["dinov2_hip_op_slide_reduce", "dinov2_hip_op_slide_gather", "dinov2_hip_op_slide_reduce_plan"]
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------- contract 1
def _mmseg_windows(h_img, w_img, h_crop, w_crop, h_stride, w_stride):
    """mmsegmentation's slide_inference, restated as its loop: (y1, x1) of every window in visiting order."""
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    out = []
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1 = h_idx * h_stride
            x1 = w_idx * w_stride
            y2 = min(y1 + h_crop, h_img)
            x2 = min(x1 + w_crop, w_img)
            y1 = max(y2 - h_crop, 0)
            x1 = max(x2 - w_crop, 0)
            out.append((y1, x1))
    return out


def _sweep():
    rng = np.random.default_rng(5)
    cases = list(sl.CASES) + [sl.REFUSED_CASE, (1024, 2048, 518, 518, 345, 345), (8192, 8192, 518, 518, 518, 518), (518, 518, 518, 518, 1, 1)]
    for _ in range(200):
        ch, cw = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        cases.append((ch + int(rng.integers(0, 200)), cw + int(rng.integers(0, 200)), ch, cw, int(rng.integers(1, ch + 1)), int(rng.integers(1, cw + 1))))
    return cases


def test_starts_are_the_mmseg_windows_and_tile_the_image():
    for h, w, ch, cw, sh, sw in _sweep():
        ys, xs = sl.starts(h, ch, sh), sl.starts(w, cw, sw)
        assert [(int(y), int(x)) for y in ys for x in xs] == _mmseg_windows(h, w, ch, cw, sh, sw)  # window k = iy nx + ix
        for st, crop, length in ((ys, ch, h), (xs, cw, w)):
            cov = np.zeros(length, np.int64)
            for s in st:
                assert 0 <= s and s + crop <= length
                cov[s:s + crop] += 1
            assert cov.min() >= 1 and st[0] == 0 and st[-1] + crop == length and (np.diff(st) > 0).all()
    assert sl.starts(70, 42, 20).tolist() == [0, 20, 28] and sl.starts(91, 42, 20).tolist() == [0, 20, 40, 49]
    assert sl.starts(43, 42, 14).tolist() == [0, 1] and sl.starts(57, 56, 1).tolist() == [0, 1]
    assert len(sl.starts(100, 28, 19)) == 5 and len(sl.starts(61, 42, 42)) == 2 and sl.starts(42, 42, 28).tolist() == [0]


def test_cases_are_well_formed():
    covers = []
    for c in sl.CASES + (sl.REFUSED_CASE,):
        h, w, ch, cw, sh, sw = c
        assert ch % sl.PATCH == 0 and cw % sl.PATCH == 0
        covers.append(int(sl.cover_map(sl.starts(h, ch, sh), sl.starts(w, cw, sw), ch, cw, h, w).max()))
    assert covers == [1, 1, 9, 4, 4, 16, 49] and sl.COVER_MAX == 16
    assert set(np.unique(sl.cover_map(*sl.case_geometry(sl.CASES[2])[:2], 42, 42, 70, 91))) == {1, 2, 3, 4, 6, 9}
    assert any(int(x) % 2 for x in sl.case_geometry(sl.CASES[2])[1]) and set(sl.CLASSES) == {2, 21, 150, 256} and len(sl.MUTANTS) == 9
    names = {p[0] for p in sl.exact_probes()}
    assert {"integer-C2", "integer-C21", "tie-3-7", "one-window-argmax", "one-window-bins", "plus-minus", "bins-all-negative"} <= names


def test_the_mutants_resampling_is_dense_cases_interpolate():
    L = dc.gaussian_logits(12, 5, 3)
    got = sl._interp_at(L, 3, 4, 42, 56, np.arange(42), np.arange(56))
    assert np.array_equal(got.view(np.uint32), dc.interpolate(L, 3, 4, 42, 56).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- restatement and mutants
def _failures(mutant, classes=sl.CLASSES):
    return sl.reduce_failures(lambda Ls, ys, xs, h0, w0, ch, cw, h, w, red, cen, eps: sl.emulate(Ls, ys, xs, h0, w0, ch, cw, h, w, red, cen, eps, mutant),
                              classes=classes)


def test_restatement_passes_every_case():
    assert _failures(None) == []


@pytest.mark.parametrize("mutant", sl.MUTANTS)
def test_planted_bugs_are_rejected(mutant):
    fails = _failures(mutant, classes=(2, 21))
    assert fails, f"planted bug {mutant} passed every case"
    print(mutant, "rejected by:", fails[0])


def _margin_check(labels, ref, bound, what):
    sure = ref["margin"] > 2 * bound
    assert (labels[sure] == ref["labels"][sure]).all(), what + ": labels differ from the reference outside the margin"
    return int((~sure).sum()), sure.size


@pytest.mark.parametrize("ci", range(len(sl.CASES)))
def test_restatement_against_float64(ci):
    """|mean_f32 - mean_64| <= (8 + n) u max|L| (slide_cases.mean_bound); labels equal wherever the float64 top-two margin exceeds twice that
    bound; at most 2 % of the pixels excluded by the margin."""
    h, w, ch, cw, _, _ = sl.CASES[ci]
    ys, xs, h0, w0 = sl.case_geometry(sl.CASES[ci])
    excluded = total = 0
    for C_ in sl.CLASSES:
        Ls = sl.case_logits(ci, C_)
        ref = sl.reference(Ls, ys, xs, h0, w0, ch, cw, h, w)
        bound = sl.mean_bound(ref["n"], np.abs(Ls).max())
        mean = sl.mean_logits(Ls, ys, xs, h0, w0, ch, cw, h, w).astype(np.float64)
        err = np.abs(mean - ref["val"])
        assert (err <= bound[..., None]).all(), float((err / bound[..., None]).max())
        e, t = _margin_check(sl.emulate(Ls, ys, xs, h0, w0, ch, cw, h, w)["labels"], ref, bound, "%s C=%d" % (sl.case_id(sl.CASES[ci]), C_))
        excluded, total = excluded + e, total + t
    print("%s: %d of %d pixels inside the margin" % (sl.case_id(sl.CASES[ci]), excluded, total))
    assert excluded <= 0.02 * total


@pytest.mark.parametrize("ci", range(len(sl.CASES)))
def test_restatement_against_the_upstream_procedure_in_torch(ci):
    """mmsegmentation's slide_inference in float64: F.interpolate(bilinear, align_corners=False) of every window's logits to the crop,
    F.pad-accumulate, a count matrix, the division.  Upstream computes its interpolation weights in float64 where the contract computes them
    in float32 -- a coordinate error of a few u max(h0, w0), times the largest difference of neighbouring logits 2 max|L|: the bound is
    (16 max(h0, w0) + 8 + n) u max|L|."""
    import torch
    import torch.nn.functional as F
    h, w, ch, cw, _, _ = sl.CASES[ci]
    ys, xs, h0, w0 = sl.case_geometry(sl.CASES[ci])
    excluded = total = 0
    worst = 0.0
    for C_ in (21, 256):
        Ls = sl.case_logits(ci, C_)
        preds = torch.zeros((1, C_, h, w), dtype=torch.float64)
        count = torch.zeros((1, 1, h, w), dtype=torch.float64)
        for k, (y1, x1) in enumerate((int(y), int(x)) for y in ys for x in xs):
            low = torch.from_numpy(Ls[k].astype(np.float64).T.reshape(1, C_, h0, w0).copy())
            crop = F.interpolate(low, size=(ch, cw), mode="bilinear", align_corners=False)
            preds += F.pad(crop, (x1, w - x1 - cw, y1, h - y1 - ch))
            count[:, :, y1:y1 + ch, x1:x1 + cw] += 1
        assert (count == 0).sum() == 0
        up = (preds / count)[0].permute(1, 2, 0).numpy()
        n = count[0, 0].numpy()
        bound = (16 * max(h0, w0) + 8 + n) * U * float(np.abs(Ls).max())
        mean = sl.mean_logits(Ls, ys, xs, h0, w0, ch, cw, h, w).astype(np.float64)
        err = np.abs(mean - up)
        worst = max(worst, float((err / bound[..., None]).max()))
        assert (err <= bound[..., None]).all(), worst
        srt = np.sort(up, axis=2)
        ref = {"labels": np.argmax(up, axis=2).astype(np.uint8), "margin": srt[..., -1] - srt[..., -2]}
        e, t = _margin_check(sl.emulate(Ls, ys, xs, h0, w0, ch, cw, h, w)["labels"], ref, bound, "%s C=%d" % (sl.case_id(sl.CASES[ci]), C_))
        excluded, total = excluded + e, total + t
    print("%s: worst error %.3f of the bound, %d of %d pixels inside the margin" % (sl.case_id(sl.CASES[ci]), worst, excluded, total))
    assert excluded <= 0.02 * total


# ------------------------------------------------------------------------------------------------------------------- planner
def _check_plan(api, h0, w0, C_, ch, cw, h, w, ys, xs):
    p = api.op_slide_reduce_plan(h0, w0, C_, (ch, cw), (h, w), ys, xs)
    what = (h0, w0, C_, ch, cw, h, w, p)
    assert p["lds_bytes"] <= 64 << 10 and p["tile_y"] * p["tile_x"] <= 256, what
    assert p["chunk"] % 4 == 0 and 4 <= p["chunk"] <= (C_ + 3) // 4 * 4 and p["pitch"] >= p["chunk"] and (p["pitch"] // 4) % 2 == 1, what
    assert p["lds_bytes"] == (p["slots_y"] * p["slots_x"] * p["span_y"] * p["span_x"] * p["pitch"] * 4 + (C_ + 3) // 4 * 16 +
                              (p["tile_y"] * p["slots_y"] + p["tile_x"] * p["slots_x"] + p["slots_y"] + p["slots_x"]) * 16 +
                              (p["tile_y"] * p["tile_x"] + 15) // 16 * 16), what
    assert p["cover"] == int(sl.cover_map(ys, xs, ch, cw, h, w).max()) <= sl.COVER_MAX, what
    # every tile's windows fit the slots, and every window's rows under a tile fit the span (the restated axis formula)
    for st, crop, length, n_in, tile, slots, span in ((ys, ch, h, h0, p["tile_y"], p["slots_y"], p["span_y"]),
                                                      (xs, cw, w, w0, p["tile_x"], p["slots_x"], p["span_x"])):
        i0, i1, _ = dc.axis(n_in, crop)
        most = rows = 0
        for p0 in range(0, length, tile):
            p1 = min(p0 + tile, length) - 1
            touching = [int(s) for s in st if s <= p1 and s + crop > p0]
            most = max(most, len(touching))
            rows = max([rows] + [int(i1[min(p1 - s, crop - 1)] - i0[max(p0 - s, 0)]) + 1 for s in touching])
        assert most == slots and rows == span, what
    return p


def test_reduce_planner_fits_the_lds_budget_for_every_accepted_request(api):
    hdr = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert "SLIDE_COVER_MAX = 16" in hdr and "DENSE_LDS_BUDGET = (size_t)64 << 10" in hdr
    chunked = 0
    for c in sl.CASES:
        h, w, ch, cw, _, _ = c
        ys, xs, h0, w0 = sl.case_geometry(c)
        for C_ in sl.CLASSES:
            _check_plan(api, h0, w0, C_, ch, cw, h, w, ys, xs)
    # crop grids up to 37 x 37 (518 / 14) and the stride-7 grid 73 x 73 under the same crop, C up to 256, cover up to 16
    for (h, w, crop, stride) in ((1024, 2048, 518, 345), (1100, 1100, 518, 173), (2000, 600, 518, 130), (518, 518, 518, 518), (8192, 8192, 518, 518),
                                 (600, 600, 518, 1), (1036, 777, 518, 37)):
        ys, xs = sl.starts(h, crop, stride), sl.starts(w, crop, stride)
        if int(sl.cover_map(ys, xs, crop, crop, h, w).max()) > sl.COVER_MAX:
            with pytest.raises(ValueError):
                api.op_slide_reduce_plan(37, 37, 150, crop, (h, w), ys, xs)
            continue
        for h0 in (37, 73):
            for C_ in (19, 150, 256):
                p = _check_plan(api, h0, h0, C_, crop, crop, h, w, ys, xs)
                chunked += p["chunk"] < C_
    assert chunked  # the staging in class chunks is reached
    ys, xs, h0, w0 = sl.case_geometry(sl.REFUSED_CASE)
    bad = [dict(y1=ys, x1=xs),                                                      # cover 49
           dict(y1=[0, 20, 40], x1=[0, 20, 40, 49], size=(70, 91)),                 # the last window not pulled back: it leaves the image
           dict(y1=[0, 28], x1=[0, 49], size=(70, 91)),                             # a gap between neighbours
           dict(y1=[28, 0], x1=[0, 20, 40, 49], size=(70, 91)),                     # not ascending
           dict(y1=[0], x1=[0], size=(42, 8193), crop=(42, 42)), dict(y1=[0], x1=[0], size=(42, 42), C_=257), dict(y1=[0], x1=[0], size=(42, 42), h0=0)]
    for kw in bad:
        a = dict(h0=3, w0=3, C_=21, crop=(42, 42), size=(70, 70))
        a.update(kw)
        with pytest.raises(ValueError):
            api.op_slide_reduce_plan(a["h0"], a["w0"], a["C_"], a["crop"], a["size"], a["y1"], a["x1"])


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (fails before this feature: the symbols are not there)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % name, hdr), name
    for name in OPS:
        assert re.search(r"\bint %s\(" % name, ops), name
    assert "typedef struct dinov2_hip_slide {" in hdr and "#define DINOV2_HIP_SLIDE_COVER_MAX 16" in hdr
    assert api.lib().dinov2_hip_abi_version() == 1 and api.SLIDE_COVER_MAX == 16
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert set(SYMBOLS) | set(OPS) <= exported


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    sec = hdr[hdr.index("sliding-window dense inference (no reference"):hdr.index("int dinov2_hip_predict_dense_slide(")]
    for text in ("slide_inference", "max(len - crop + stride - 1, 0) / stride + 1", "max(min(i * stride + crop, len) - crop, 0)", "pulled back",
                 "k = iy * nx + ix", "bit for bit", "ascending k", "acc_c / (float)n", "correctly rounded division", "fused multiply-add",
                 "lowest", "BEFORE the argmax", "One window", "launch geometry", "split into passes", "Out of scope", "softmax probabilities",
                 "DINOV2_HIP_U8_BGR_HWC is refused", "65 535", "DINOV2_HIP_SLIDE_COVER_MAX", "before anything is", "dinov2_hip_predict_list",
                 "complete on return", "runs eagerly under DINOV2_HIP_GRAPHS=1", "\"head\"", "profiles/dense_slide.md"):
        assert text in sec, text
    dense = hdr[hdr.index("linear dense-prediction heads"):hdr.index("int dinov2_hip_predict_dense(")]
    assert "multi-scale or sliding-window" not in dense


def test_slide_windows_refuses_without_a_model(api):
    """What needs no loaded model: the NULL refusals (the starts themselves are checked against a model in tests/test_gpu_slide.py)."""
    s = api.Slide(42, 42, 20, 20)
    ny, nx = C.c_int32(-1), C.c_int32(-1)
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_slide_windows(None, 70, 91, C.byref(s), C.byref(ny), C.byref(nx), None, None, err, len(err)) == 4 and err.value
    assert (ny.value, nx.value) == (-1, -1)
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_slide_windows(None, 70, 91, C.byref(s), None, None, None, None, err, len(err)) == 4 and err.value
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_predict_dense_slide(None, None, None, None, None, err, len(err)) == 4 and err.value


def test_ctypes_struct_matches_the_header(api, tmp_path):
    fields = ["crop_h", "crop_w", "stride_h", "stride_w", "reserved"]
    body = 'std::printf(" %zu", sizeof(dinov2_hip_slide));\n' + "".join('std::printf(" %%zu", offsetof(dinov2_hip_slide, %s));\n' % f for f in fields)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.Slide)] + [getattr(api.Slide, f).offset for f in fields]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "dinov2_hip.h"\nint main(void) { dinov2_hip_slide s = {0};\n'
                   '    int (*f)(dinov2_hip_session *, const dinov2_hip_input *, const dinov2_hip_dense_head *, const dinov2_hip_slide *,\n'
                   '             const dinov2_hip_dense_out *, char *, size_t) = dinov2_hip_predict_dense_slide;\n'
                   '    int (*g)(const dinov2_hip_model *, int32_t, int32_t, const dinov2_hip_slide *, int32_t *, int32_t *, int32_t *, int32_t *, char *,\n'
                   '             size_t) = dinov2_hip_slide_windows;\n'
                   '    return s.crop_h + DINOV2_HIP_SLIDE_COVER_MAX - 16 + (f ? 0 : 1) + (g ? 0 : 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                   check=True, capture_output=True, timeout=120)


# ------------------------------------------------------------------------------------------------------------------- build checks
@pytest.fixture(scope="module")
def slide_asm(tmp_path_factory):
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "slide.hip")
    return compile_misc_both_ways(src, str(tmp_path_factory.mktemp("slideasm")))


def test_slide_cross_compiles_without_scratch(slide_asm):
    """csrc/slide.hip compiles for gfx950 with the Makefile's flags; every kernel has private segment size 0 and at most 256 VGPRs (read from
    the kernel descriptors)."""
    assert MISC_FLAGS and os.path.exists(HIPCC)
    names = []
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", slide_asm[0], re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256, name
        names.append(name)
    assert len(names) == 3 and sum("slide_gather_kernel" in n for n in names) == 1 and sum("slide_reduce_kernel" in n for n in names) == 2, names
    assert set(misc_instruction_streams(slide_asm[0])) >= set(names)


def test_slide_reduce_keeps_its_rounding_points(slide_asm):
    """slide_reduce_kernel (contracts 3 and 4: no fused multiply-add) compiles to the same instruction stream with and without
    -ffp-contract=off."""
    fused, n = fused_kernels(*slide_asm, pattern=r"slide_reduce_kernel")
    assert n == 2, n
    assert not fused, fused
