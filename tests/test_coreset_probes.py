"""The numpy restatement of the coreset contract (tests/coreset_cases.py) through the very probes tests/test_gpu_coreset.py applies to the
kernels, and the planted bugs those probes must reject; the planner against its restatement; plus the declarations, exports and struct layout
of the new C-ABI, the build check of csrc/coreset.hip (kernel descriptors only) and the argument checks of Bank.keep that need no device.
No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coreset_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
OPS = ["dinov2_hip_op_coreset", "dinov2_hip_op_coreset_plan", "dinov2_hip_op_coreset_bench"]


def _run(mutant):
    return lambda x, m, first, stop_sim, patch: cc.emulate(x, m, first, stop_sim, mutant, patch, exact=True)


@pytest.mark.parametrize("kind", cc.PROBES)
def test_restatement_passes_every_probe(kind):
    ok, msg = cc.check_probe(_run(None), kind)
    assert ok, msg


@pytest.mark.parametrize("mutant", sorted(cc.MUTANTS))
def test_planted_bugs_are_rejected_by_their_probe(mutant):
    ok, msg = cc.check_probe(_run(mutant), cc.MUTANTS[mutant])
    assert not ok, f"planted bug {mutant} passed probe {cc.MUTANTS[mutant]}"


def test_cover_is_non_decreasing_on_every_case():
    for shape in cc.SHAPES:
        n, H, m = shape
        r = cc.emulate(cc.shape_inputs(shape), m)
        assert r["selected"] == m and r["cover"][0] == -np.inf and cc.non_decreasing(r["cover"]), shape
        assert len(set(r["idx"].tolist())) == m and r["nearest"].max() <= m - 1 and r["nearest"].min() >= 0, shape
        assert (r["near_sim"][r["idx"]] >= 1 - 2.0 ** -9).all(), shape  # a pick's own similarity
    for kind in cc.PROBES:
        r = cc.expected(cc.build_probe(kind))
        assert cc.non_decreasing(r["cover"]), kind


def test_cases_are_well_formed():
    hdr = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert "CORESET_N_MAX = 1 << 20, CORESET_BANK_N_MAX = 1 << 24, CORESET_PARTS_MAX = 1024" in hdr
    assert "CORESET_WG_BYTES = (size_t)64 << 10" in hdr
    assert {s[0] for s in cc.SHAPES} >= {1, 2, 127, 128, 129, 257, 1374} and {s[1] for s in cc.SHAPES} >= {8, 72, 384, 1536}
    assert {s[2] for s in cc.SHAPES} >= {1, 2, 64} and any(s[0] == s[2] > 2 for s in cc.SHAPES)
    assert set(cc.MUTANTS.values()) <= set(cc.PROBES)
    for kind in cc.PROBES:  # 131 rows, the last three in a second tile; x^ of every probe row is +-2^-1, +-2^-2 or +-2^-3 (or 0)
        x = cc.build_probe(kind)["x"]
        assert len(x) == cc.TILE + 3
        assert np.isin(np.abs(cc.mc.normalise_f16(x).astype(np.float64)), [0.0, 0.5, 0.25, 0.125]).all(), kind
    a, b = cc.build_probe("stop_equal"), cc.build_probe("stop_ulp_above")
    assert np.float32(b["stop_sim"]) == np.nextafter(np.float32(a["stop_sim"]), np.float32(np.inf))


def test_planner_equals_its_restatement(api):
    """coreset_plan (csrc/kernels.h, through dinov2_hip_op_coreset_plan; no device) against coreset_cases.plan, and what it promises."""
    rng = np.random.default_rng(29)
    cases = [(s[0], s[1], r) for s in cc.SHAPES for r in (0, 1, 128, 129, 1 << 20)]
    cases += [(1369, 1024, 0), (43808, 1024, 0), (1 << 20, 1024, 0), (1 << 20, 128, 0), (1 << 20, 8, 0), (1 << 20, 8, 128), (65536, 64, 0), (65537, 64, 0)]
    for _ in range(200):
        cases.append((int(rng.integers(1, 1 << int(rng.integers(1, 21))) + 1), int(rng.integers(8, 4097)), int(rng.choice([0, 0, 1, 300, 5000, 1 << 19]))))
    for n, H, r in cases:
        p, q = api.op_coreset_plan(n, H, 1, r), cc.plan(n, H, r)
        assert {k: p[k] for k in q} == q, (n, H, r)
        assert p["rows_per_wg"] % 128 == 0 and 1 <= p["nparts"] <= cc.PARTS_MAX, p
        assert (p["nparts"] - 1) * p["rows_per_wg"] < n <= p["nparts"] * p["rows_per_wg"], p  # the workgroups partition the rows, none is empty
    assert api.op_coreset_plan(43808, 1024)["nparts"] == 343 and api.op_coreset_plan(1 << 20, 1024)["nparts"] == 1024
    assert api.op_coreset_plan(1 << 20, 128, 1 << 20)["bytes"] - api.op_coreset_plan(1 << 20, 128, 64)["bytes"] == 2 * ((4 << 20) - 256)
    for bad in ((0, 8, 1, 0), ((1 << 20) + 1, 8, 1, 0), (1, 7, 1, 0), (1, 4097, 1, 0), (4, 8, 0, 0), (4, 8, 5, 0), (4, 8, 1, -1)):
        with pytest.raises(ValueError):
            api.op_coreset_plan(*bad)


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (fails before this feature: the symbols are not there)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    assert re.search(r"\bint\s+dinov2_hip_coreset_tokens\(", hdr) and "typedef struct dinov2_hip_coreset {" in hdr
    assert re.search(r"\bint\s+dinov2_hip_bank_keep\(", hdr)
    assert hdr.index("dinov2_hip_bank_topk(") < hdr.index("int  dinov2_hip_bank_keep(") < hdr.index("dinov2_hip_kmeans_tokens(")
    assert "#define DINOV2_HIP_ABI_VERSION 1" in hdr or api.lib().dinov2_hip_abi_version() == 1
    for name in OPS:
        assert re.search(r"\bint %s\(" % name, ops), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert set(OPS) | {"dinov2_hip_coreset_tokens", "dinov2_hip_bank_keep"} <= exported


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    sec = hdr[hdr.index("greedy k-center selection of rows"):hdr.index("int dinov2_hip_coreset_tokens(")]
    for text in ("Contract 1 of dinov2_hip_match", "hpad / 32", "cover[0] = -INFINITY", "LOWEST such u", "-0 is read as +0", "LOWEST row index",
                 "non-decreasing", "never\n *       selected again", "Rows >= n never take part", "selected = t", "cover = +INFINITY", "No atomics",
                 "no grid-wide barrier", "Out of scope", "Euclidean", "random-projection", "warm starts", "bf16 operands", "list forward",
                 "before anything is launched, allocated or copied", "profiles/coreset.md"):
        assert text in sec, text
    bank = hdr[hdr.index("a resident feature bank"):hdr.index("int  dinov2_hip_bank_keep(")]
    assert "dinov2_hip_bank_keep below" in bank and "idx[j] >= j" in bank and "change nothing" in bank
    km = hdr[hdr.index("spherical k-means of token rows"):hdr.index("int dinov2_hip_kmeans_tokens(")]
    assert 'init="maximin"' in km and "dinov2_hip_coreset_tokens" in km


def test_ctypes_struct_matches_the_header(api, tmp_path):
    fields = ["rows", "all_images", "bank", "m", "first", "stop_sim", "idx", "cover", "selected", "nearest", "near_sim", "reserved"]
    body = 'std::printf(" %zu", sizeof(dinov2_hip_coreset));\n' + "".join('std::printf(" %%zu", offsetof(dinov2_hip_coreset, %s));\n' % f for f in fields)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.Coreset)] + [getattr(api.Coreset, f).offset for f in fields]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "dinov2_hip.h"\nint main(void) { dinov2_hip_coreset c = {{0}};\n'
                   '    int (*f)(dinov2_hip_session *, const dinov2_hip_coreset *, char *, size_t) = dinov2_hip_coreset_tokens;\n'
                   '    int (*g)(dinov2_hip_session *, dinov2_hip_bank *, const int32_t *, int32_t, char *, size_t) = dinov2_hip_bank_keep;\n'
                   '    c.rows.source = DINOV2_HIP_ROWS_LAST_PATCHES;\n'
                   '    return c.m + c.rows.n + (c.bank ? 1 : 0) + (f ? 0 : 1) + (g ? 0 : 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                   check=True, capture_output=True, timeout=120)


# ------------------------------------------------------------------------------------------------------------------- build check
def test_coreset_cross_compiles_without_scratch(tmp_path):
    """csrc/coreset.hip compiles for gfx950 and none of its kernels spills (private segment size 0, read from the kernel descriptors); the
    sweep runs on the matrix cores through sim_tile.h's chain and writes no K loop of its own; the normaliser is match.hip's; no atomics."""
    out = tmp_path / "coreset.s"
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "coreset.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    txt = out.read_text()
    names = []
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 128, name
        names.append(name)
    kinds = ["coreset_init", "coreset_sweep", "bank_gather"]
    assert len(names) == len(kinds) and all(sum(f"{k}_kernel" in n for n in names) == 1 for k in kinds), names
    body = txt[txt.index("coreset_sweep_kernel"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    assert "v_mfma_f32_16x16x32_f16" in body
    assert "atomic" not in txt and "s_sleep" not in txt
    text = open(src).read()
    assert re.search(r'^#include "sim_tile\.h"', text, re.M) and "sim_column(" in text
    for needle in ("mfma16(", "struct Best", "bool before(", "match_normalise_kernel", "hipLaunchCooperativeKernel"):
        assert needle not in text, needle
    header = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "sim_tile.h")).read()
    assert "float sim_column(" in header and "coreset_sweep_kernel" in header[:header.index("#pragma once")]


# ------------------------------------------------------------------------------------------------------------------- Bank.keep
def test_bank_keep_checks_its_indices_before_any_call(api):
    """Bank.keep sorts and validates on the host: what is not a non-empty 1-D integer array of distinct in-range indices raises ValueError
    before the library is asked for anything but the count (0 for a bank without a handle)."""
    bank = api.Bank.__new__(api.Bank)
    for bad in ([], [[0, 1]], [0.5, 1.0], np.zeros((2, 2), np.int32), [0], [-1], [1, 1]):
        with pytest.raises(ValueError):
            bank.keep(None, bad)
