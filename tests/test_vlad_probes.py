"""The numpy restatement of the VLAD contract (tests/vlad_cases.py) through the very cases tests/test_gpu_vlad.py applies to the kernels, and
the planted bugs those cases must reject; the planner against its restatement; the refusals that need no device; plus the declarations,
exports and struct layout of the new C-ABI.  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vlad_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["dinov2_hip_op_vlad_plan", "dinov2_hip_op_vlad", "dinov2_hip_op_vlad_bench"]


@pytest.fixture(scope="module")
def clean_failures():
    return vc.all_failures(vc.emulate_vlad)


def test_restatement_passes_every_case(clean_failures):
    """Probes bit for bit, shapes under their bounds, the three normalised modes, the position case."""
    assert clean_failures == []


@pytest.mark.parametrize("mutant", sorted(vc.MUTANTS))
def test_planted_bugs_are_rejected_by_their_named_case(mutant):
    failures = vc.all_failures(lambda x, off, c, flags: vc.emulate_vlad(x, off, c, flags, mutant))
    assert any(f.startswith(vc.MUTANTS[mutant]) for f in failures), (mutant, failures[:4])


def test_cases_are_well_formed():
    hdr = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert "VLAD_SEG_MAX = 4096, VLAD_N_MAX = 1 << 20" in hdr and "VLAD_PARTIAL_MAX = (size_t)32 << 20" in hdr
    assert vc.SEG_LENS == [1, 63, 64, 65, 127, 128, 129, 257]
    assert {(K, H) for _, K, H in vc.SHAPES} >= {(1, 8), (2, 8), (128, 72), (129, 384), (300, 1536)} and ([1369, 1369], 32, 1024) in vc.SHAPES
    kh, chunk, lens = vc.CHUNK_EDGE
    assert vc.chunk_rows(*kh) == chunk and sorted(lens) == [chunk - 1, chunk + 1] and (lens, *kh) in vc.SHAPES
    seg, c, lists = vc.position_case()
    assert sorted(lists) == [0, 2, 4] and len({int(off[pos]) % 64 for pos, (_, off) in lists.items()}) == 3
    for pos, (x, off) in lists.items():
        assert len(off) == 6 and np.array_equal(x[off[pos]:off[pos + 1]], seg)
    for kind in vc.PROBES:  # every probe has its exact expectation (the asserts inside it hold)
        pr = vc.build_probe(kind)
        vc.exact_expectation(pr["x"], pr["off"], pr["c"])
    assert len(vc.build_probe("k1")["c"]) == 1


def test_planner_equals_its_restatement(api):
    """vlad_plan (csrc/kernels.h, through dinov2_hip_op_vlad_plan; no device) against vlad_cases.plan, and what it promises.  Fails before
    this feature: the symbol is not there."""
    rng = np.random.default_rng(29)
    cases = [(vc.offsets_of(lens), K, H) for lens, K, H in vc.SHAPES]
    cases += [(vc.offsets_of([1369] * 32), 32, 1024), (vc.offsets_of([1369] * 32), 64, 1024), (vc.offsets_of([1369]), 64, 1024),
              (vc.offsets_of([1 << 20]), 1024, 4096), (vc.offsets_of([1 << 20]), 1, 8), (vc.offsets_of([256] * 4096), 2, 8),
              (vc.offsets_of([1] * 64), 1024, 4096), (vc.offsets_of([5000, 1, 7000]), 1024, 4096)]
    for _ in range(100):
        n_seg = int(rng.integers(1, 40))
        lens = rng.integers(1, 1 << int(rng.integers(1, 14)), size=n_seg) + 1
        cases.append((vc.offsets_of(lens), int(rng.integers(1, 1025)), int(rng.integers(8, 4097))))
    for off, K, H in cases:
        if (len(off) - 1) * K * H > vc.OUT_MAX:
            continue
        p, q = api.op_vlad_plan(off, K, H), vc.plan(off, K, H)
        for k, v in q.items():
            assert np.array_equal(p[k], v), (list(off[:6]), K, H, k)
        assert p["partial_bytes"] <= vc.PARTIAL_MAX and p["bytes"] > p["partial_bytes"] and p["cap"] >= 2
        assert p["chunk"] % 64 == 0 and p["chunk"] == vc.chunk_rows(K, H)
        # every segment has a block of whole tiles of its own, and its chunks partition the block in K-tiles of 64 from its first row on
        row = 0
        for s, (row0, ln, ch0, nch) in enumerate(p["segs"]):
            assert row0 == row and row0 % 128 == 0 and ln == off[s + 1] - off[s]
            ch = p["chunks"][ch0:ch0 + nch]
            assert (ch[:, 0] == s).all() and ch[0, 1] == row0 and (ch[:-1, 2] * 64 == p["chunk"]).all()
            assert np.array_equal(ch[1:, 1], ch[:-1, 1] + 64 * ch[:-1, 2])
            row = int(ch[-1, 1] + 64 * ch[-1, 2])
            assert row == row0 + -(-ln // 128) * 128
        assert row == p["npad"]
    # a segment's chunks depend on (its length, K, H) alone: the same with other neighbours
    a, b = api.op_vlad_plan(vc.offsets_of([300, 777, 5]), 40, 520), api.op_vlad_plan(vc.offsets_of([777]), 40, 520)
    ca, cb = a["chunks"][a["segs"][1][2]:][:a["segs"][1][3]], b["chunks"]
    assert np.array_equal(ca[:, 1] - a["segs"][1][0], cb[:, 1]) and np.array_equal(ca[:, 2], cb[:, 2])


def test_refusals_that_need_no_device(api):
    L = api.lib()
    good = vc.offsets_of([3, 4])
    bad = [(good, 0, 8), (good, 1025, 8), (good, 1, 7), (good, 1, 4097), (np.array([1, 3], np.int32), 1, 8), (np.array([0, 3, 3], np.int32), 1, 8),
           (np.array([0, 4, 3], np.int32), 1, 8), (np.array([0, (1 << 20) + 1], np.int32), 1, 8), (np.array([0], np.int32), 1, 8),
           (vc.offsets_of([1] * 4097), 1, 8), (vc.offsets_of([1] * 65), 1024, 4096)]
    for off, K, H in bad:
        with pytest.raises(ValueError):
            api.op_vlad_plan(off, K, H)
    x, c = np.ones((7, 8), np.float32), np.ones((2, 8), np.float32)
    out = np.full(7 * 2 * 8, -7.0, np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    xp, cp, op, gp = x.ctypes.data_as(fp), c.ctypes.data_as(fp), out.ctypes.data_as(fp), good.ctypes.data_as(ip)
    assert L.dinov2_hip_op_vlad(None, gp, 2, cp, 2, 8, 3, None, None, None, op, None, None) == 4
    assert L.dinov2_hip_op_vlad(xp, gp, 2, None, 2, 8, 3, None, None, None, op, None, None) == 4
    assert L.dinov2_hip_op_vlad(xp, None, 2, cp, 2, 8, 3, None, None, None, op, None, None) == 4
    assert L.dinov2_hip_op_vlad(xp, gp, 2, cp, 2, 8, 4, None, None, None, op, None, None) == 4  # an unknown flag bit
    assert L.dinov2_hip_op_vlad(xp, gp, 2, cp, 0, 8, 3, None, None, None, op, None, None) == 4
    ms = (C.c_float * 3)()
    assert L.dinov2_hip_op_vlad_bench(None, gp, 2, None, 2, 8, 3, 0, 1, ms) == 4
    assert L.dinov2_hip_op_vlad_bench(0x1000, gp, 2, 0x1000, 2, 8, 3, 0, 0, ms) == 4  # iters = 0
    v = api.Vlad(api.Rows(0, x.ctypes.data, 7, 8, 0, 0), 0, good.ctypes.data, 2, 2, c.ctypes.data, 3, out.ctypes.data, None, None, None)
    err = C.create_string_buffer(256)
    assert L.dinov2_hip_vlad_tokens(None, C.byref(v), err, len(err)) == 4 and b"null session" in err.value
    assert (out == -7.0).all()


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_and_exported(api):
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    assert re.search(r"\bint\s+dinov2_hip_vlad_tokens\(", hdr) and "typedef struct dinov2_hip_vlad {" in hdr
    assert "enum dinov2_hip_vlad_flags { DINOV2_HIP_VLAD_INTRA_NORM = 1, DINOV2_HIP_VLAD_L2_NORM = 2 };" in hdr
    assert hdr.index("dinov2_hip_kmeans_tokens(") < hdr.index("dinov2_hip_vlad_tokens(") < hdr.index("typedef struct dinov2_hip_dense_desc")
    for name in OPS:
        assert re.search(r"\bint %s\(" % name, ops), name
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert set(OPS) | {"dinov2_hip_vlad_tokens"} <= exported


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    sec = hdr[hdr.index("VLAD descriptors of row segments"):hdr.index("int dinov2_hip_vlad_tokens(")]
    for text in ("contract 1 of dinov2_hip_match", "Contract 2 of dinov2_hip_kmeans", "bit for bit", "a zero row counts", "(len_s, K, H) alone",
                 "No atomics", "whatever segments travel with it", "not the caller's vector", "empty cluster gives a zero row", "depends on H alone",
                 "(K, H) alone", "Nothing is normalised\n *       across segments", "Out of scope", "soft assignment", "the bank stops at 4096",
                 "device-side outputs", "whitening", "device group", "list forward", "bf16 operands", "dinov2_compat.hpp", "LAST_CLS is refused",
                 "before\n * anything is launched, allocated or copied", "32 MiB", "last forward stays", "profiles/vlad.md"):
        assert text in sec, text


def test_ctypes_struct_matches_the_header(api, tmp_path):
    fields = ["rows", "all_images", "offsets", "n_seg", "K", "centers", "flags", "vlad", "counts", "labels", "sim", "reserved"]
    body = 'std::printf(" %zu", sizeof(dinov2_hip_vlad));\n' + "".join('std::printf(" %%zu", offsetof(dinov2_hip_vlad, %s));\n' % f for f in fields)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.Vlad)] + [getattr(api.Vlad, f).offset for f in fields]
    assert (api.VLAD_INTRA_NORM, api.VLAD_L2_NORM) == (1, 2)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "dinov2_hip.h"\nint main(void) { dinov2_hip_vlad v = {{0}};\n'
                   '    int (*f)(dinov2_hip_session *, const dinov2_hip_vlad *, char *, size_t) = dinov2_hip_vlad_tokens;\n'
                   '    v.flags = DINOV2_HIP_VLAD_INTRA_NORM | DINOV2_HIP_VLAD_L2_NORM;\n'
                   '    return v.K + v.rows.n + (f ? 0 : 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                   check=True, capture_output=True, timeout=120)
