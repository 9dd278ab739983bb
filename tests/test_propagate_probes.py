"""The numpy restatement of the propagate contract (tests/propagate_cases.py) through the very cases tests/test_gpu_propagate.py applies to the
kernels, and the planted bugs those cases must reject; the restatement against an independent float64 transcription of the published
procedure and against its own bound; the planner against its restatement and a brute-force proof of the tile skip; plus the declarations,
exports and struct layouts of the new C-ABI and the build check of csrc/propagate.hip (kernel descriptors only).  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import propagate_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dinov2.cpp_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ["dinov2_hip_propmem_create", "dinov2_hip_propmem_free", "dinov2_hip_propmem_set", "dinov2_hip_propmem_drop", "dinov2_hip_propagate"]
OPS = ["dinov2_hip_op_propagate", "dinov2_hip_op_propagate_plan", "dinov2_hip_op_propagate_bench"]


def _fn(mutant):
    return lambda q, rows, labels, grid, slots, radius, k, T, ct: pc.emulate(q, rows, labels, grid, slots, radius, k, T, ct, mutant)


def _memory(mutant):
    return lambda H, grid, frames, channels: pc.PropModel(H, grid, frames, channels, mutant)


@pytest.mark.parametrize("name", pc.case_names())
def test_restatement_passes_every_case(name):
    """With margin 1: the float32 numpy emulation stays inside the UNDOUBLED output bound on every shape."""
    report = []
    failures = pc.case_failures(name, _fn(None), _memory(None), margin=1.0, report=report)
    print("\n".join(report))
    assert failures == []


@pytest.mark.parametrize("mutant", list(pc.MUTANTS))
def test_planted_bugs_are_rejected_by_their_named_case(mutant):
    name = pc.MUTANTS[mutant]
    assert name in pc.case_names()
    assert pc.case_failures(name, _fn(mutant), _memory(mutant)), f"planted bug {mutant} passed {name}"


def test_restatement_equals_the_published_procedure():
    """Tie-free Gaussian rows, the same f16 unit rows on both sides: the restatement selects the indices the published procedure keeps
    (exp(S / T) masked, top k, normalised, labels x affinity -- all in float64), and contract 5 and 6 evaluated in float64 on those indices
    give its output within 1e-12."""
    for (h0, w0), H, frames, slots, radius, k, T in (((7, 9), 64, 3, 0b101, 2, 5, 0.1), ((12, 12), 72, 2, 0b11, -1, 7, 0.07),
                                                    ((4, 5), 32, 1, 0b1, 1, 64, 0.5)):
        P = h0 * w0
        for seed in range(8):  # the first draw whose k + 1 best candidates of every query are 1e-5 apart: far above the f32 sums' error
            rng = np.random.default_rng(P + H + seed)
            q = mc.gaussian_tokens(P, H, 3 + P + seed, outliers=False)
            rows = (q[None] + rng.standard_normal((frames, P, H))).astype(np.float32)
            labels = rng.standard_normal((frames, P, 3)).astype(np.float32)
            q16 = mc.normalise_f16(q)
            rows16 = np.stack([mc.normalise_f16(r) for r in rows])
            S = q16.astype(np.float64) @ rows16.reshape(-1, H).astype(np.float64).T
            cand = pc.candidates(h0, w0, frames, slots, radius)
            srt = -np.sort(-np.where(cand, S, -np.inf), 1)[:, :k + 1]
            with np.errstate(invalid="ignore"):
                gaps = (srt[:, :-1] - srt[:, 1:])[np.isfinite(srt[:, 1:])]
            if gaps.min() > 1e-5:
                break
        assert gaps.min() > 1e-5, "no tie-free draw"
        out_pub, idx_pub = pc.published(q16, rows16, labels, h0, w0, slots, radius, k, T)
        got = pc.emulate(q, rows, labels, (h0, w0), slots, radius, k, T)
        assert np.array_equal(got["idx"], idx_pub)
        sim64 = np.where(got["idx"] >= 0, np.take_along_axis(S, np.maximum(got["idx"], 0).astype(np.int64), 1), -np.inf)
        with np.errstate(invalid="ignore"):
            w = np.where(got["idx"] >= 0, np.exp((sim64 - sim64[:, :1]) / T), 0.0)
        out = (w[:, :, None] * labels.reshape(-1, 3).astype(np.float64)[np.maximum(got["idx"], 0)]).sum(1) / w.sum(1)[:, None]
        assert np.abs(out - out_pub).max() <= 1e-12


def test_cases_are_well_formed():
    hdr = open(os.path.join(CSRC, "kernels.h")).read()
    assert "PROP_FRAMES_MAX = 64, PROP_GRID_MAX = 256, PROP_C_MAX = 256, PROP_RADIUS_MAX = 255" in hdr and "PROP_ROWS_MAX = 1 << 24" in hdr
    assert (pc.K_MAX, pc.FRAMES_MAX, pc.GRID_MAX, pc.C_MAX, pc.RADIUS_MAX) == (64, 64, 256, 256, 255)
    assert set(pc.MUTANTS.values()) <= set(pc.case_names())
    # the skip case really skips: query tile 0 of the 20 x 20 grid at radius 1 walks column tiles 0 and 1 of 4
    assert pc.plan(20, 20, 2, 1, 3)["ranges"] == [(0, 2), (0, 3), (1, 4), (2, 4)]
    assert pc.plan(20, 20, 2, -1, 3)["ranges"] == [(0, 4)] * 4 == pc.plan(20, 20, 2, 255, 3)["ranges"]
    # the chunking cases really differ
    assert [pc.plan(20, 20, 2, 1, 64, ct)["nchunks"] for ct in pc.CHUNKINGS] == [6, 6, 3, 1]
    # the corner-heavy case: no window holds k candidates
    h0, w0, _, frames, slots, radius, k, _ = pc.SHAPES[6]
    assert pc.candidates(h0, w0, frames, slots, radius).sum(1).max() < k
    # every duplicates window holds at least k copies where k is small, and fewer than k where the tail is wanted
    for grid, frames, slots, radius, k in pc.DUPLICATES.values():
        n = pc.candidates(grid[0], grid[1], frames, slots, radius).sum(1)
        assert n.min() >= k or n.max() < k


def test_planner_equals_its_restatement(api):
    """propagate_plan (csrc/kernels.h, through dinov2_hip_op_propagate_plan; no device) against propagate_cases.plan over a sweep of grids
    and radii, and the bound it promises."""
    grids = [(1, 1), (5, 7), (12, 12), (20, 20), (9, 15), (16, 8), (37, 37), (1, 256), (256, 1), (64, 48), (256, 256)]
    for h0, w0 in grids:
        for radius in (-1, 0, 1, 2, 5, 12, 255):
            for nactive, k, ct in ((1, 1, 0), (2, 5, 0), (8, 64, 0), (3, 8, 1), (64, 64, 2), (2, 3, 1 << 20)):
                if nactive * (-(-h0 * w0 // 128) * 128) > 1 << 24:
                    continue
                p = api.op_propagate_plan((h0, w0), 64, nactive, radius, k, 4, ct)
                want = pc.plan(h0, w0, nactive, radius, k, ct)
                assert {key: p[key] for key in ("chunk_tiles", "nchunks", "qtiles", "max_items", "kept_items")} == \
                    {key: want[key] for key in ("chunk_tiles", "nchunks", "qtiles", "max_items", "kept_items")}, (h0, w0, radius, nactive, k, ct)
                assert [tuple(r) for r in p["ranges"].tolist()] == want["ranges"]
                assert p["nchunks"] * p["chunk_tiles"] >= p["max_items"] > (p["nchunks"] - 1) * p["chunk_tiles"]
                assert p["partial_bytes"] <= pc.PARTIAL_MAX, p
    for bad in (dict(grid=(0, 4)), dict(grid=(4, 257)), dict(k=65), dict(k=0), dict(radius=256), dict(radius=-2), dict(nactive=0), dict(nactive=65),
                dict(H=7), dict(C_=257)):
        kw = dict(grid=(4, 4), H=64, nactive=1, radius=1, k=1, C_=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            api.op_propagate_plan(**kw)


def test_no_skipped_tile_ever_holds_a_candidate():
    """Brute force over small and awkward grids: every candidate of every query lies in a column tile its query tile walks."""
    for h0, w0 in [(1, 1), (1, 200), (200, 1), (5, 7), (12, 12), (20, 20), (9, 15), (16, 8), (37, 37), (3, 129), (129, 3), (11, 128), (23, 17)]:
        P = h0 * w0
        y, x = np.divmod(np.arange(P), w0)
        for radius in (0, 1, 2, 3, 7, 12, 40, 255):
            win = np.maximum(np.abs(y[:, None] - y[None]), np.abs(x[:, None] - x[None])) <= radius
            for qt in range(-(-P // 128)):
                t0, t1 = pc.tile_range(qt, P, w0, radius)
                assert 0 <= t0 < t1 <= -(-P // 128)
                cols = np.flatnonzero(win[qt * 128:(qt + 1) * 128].any(0)) // 128
                assert cols.min() >= t0 and cols.max() < t1, (h0, w0, radius, qt)


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (fails before this feature: the symbols are not there)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\(" % name, hdr), name
    for name in OPS:
        assert re.search(r"\bint %s\(" % name, ops), name
    assert "typedef struct dinov2_hip_propmem dinov2_hip_propmem;" in hdr and "typedef struct dinov2_hip_propagate_req" in hdr
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert set(SYMBOLS) | set(OPS) <= exported


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    sec = hdr[hdr.index("video label propagation over a frame memory"):hdr.index("int  dinov2_hip_propagate(")]
    for text in ("Contract 1 of dinov2_hip_match", "Contract 2 of dinov2_hip_match", "(i / w0, i % w0)", "max(|qy - py|, |qx - px|) <= radius",
                 "LOWEST index", "index = f * P + p", "idx = -1 and", "sim = -INFINITY", "bit for bit", "expf((sim_j - sim_0) / T)",
                 "w_0 = 1 exactly", "j ascending", "No atomics", "LOWEST c", "keeps ALL the tied entries", "never moved", "may outlive the model",
                 "Out of scope", "k > 64", "non-rectangular windows", "before anything is launched, allocated or copied", "32 MiB",
                 "profiles/propagate.md"):
        assert text in sec, text


def test_ctypes_structs_match_the_header(api, tmp_path):
    fields = ["queries", "slots", "radius", "k", "temperature", "keep", "labels", "argmax", "idx", "sim", "reserved"]
    body = 'std::printf(" %zu", sizeof(dinov2_hip_propagate_req));\n'
    body += "".join('std::printf(" %%zu", offsetof(dinov2_hip_propagate_req, %s));\n' % f for f in fields)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.PropagateReq)] + [getattr(api.PropagateReq, f).offset for f in fields]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "dinov2_hip.h"\nint main(void) { dinov2_hip_propagate_req r = {{0}};\n'
                   '    int (*f)(dinov2_hip_session *, dinov2_hip_propmem *, const dinov2_hip_propagate_req *, char *, size_t) = dinov2_hip_propagate;\n'
                   '    int (*g)(dinov2_hip_session *, dinov2_hip_propmem *, int32_t, const dinov2_hip_rows *, const float *, int32_t, char *, size_t)'
                   ' = dinov2_hip_propmem_set;\n'
                   '    r.queries.source = DINOV2_HIP_ROWS_LAST_PATCHES;\n'
                   '    return r.k + (int)r.slots + (f ? 0 : 1) + (g ? 0 : 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                   check=True, capture_output=True, timeout=120)


# ------------------------------------------------------------------------------------------------------------------- build check
def test_propagate_cross_compiles_without_scratch(tmp_path):
    """csrc/propagate.hip compiles for gfx950 to its two kernels, neither of which spills (private segment size 0, read from the kernel
    descriptors), within 256 VGPRs; the selection runs on the matrix cores; the tile, the order and the list each have their one source."""
    out = tmp_path / "propagate.s"
    src = os.path.join(CSRC, "propagate.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    txt = out.read_text()
    names = []
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256, name
        names.append(name)
    assert len(names) == 2 and sum("propagate_topk_kernel" in n for n in names) == 1 and sum("propagate_combine_kernel" in n for n in names) == 1, names
    topk = next(n for n in names if "propagate_topk_kernel" in n)
    body = txt[txt.index(topk + ":"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    assert "v_mfma_f32_16x16x32_f16" in body
    text = open(src).read()
    assert re.search(r'^#include "sim_tile\.h"', text, re.M) and re.search(r'^#include "topk_list\.h"', text, re.M)
    for needle in ("(row >> 1) & 7)) << 4", "^ sw) << 4", "^ p.sw) << 4", "mfma16(", "struct Best", "bool better(", "bool before("):
        assert needle not in text, needle
    # the list has one source, and the merge kernel is reached through its launcher
    defs = [f for f in sorted(os.listdir(CSRC)) if re.search(r"\bvoid wave_insert\(", open(os.path.join(CSRC, f)).read())]
    assert defs == ["topk_list.h"]
    assert "bank_merge_kernel" not in text and "launch_bank_merge(" in text
    assert "match_normalise_kernel" not in text and "launch_match_normalise(" in text
