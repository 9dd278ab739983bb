"""The numpy restatement of the k-means contract (tests/kmeans_cases.py) through the very cases tests/test_gpu_kmeans.py applies to the kernels,
and the planted bugs those cases must reject; the driver cases' margin condition; the planner against its restatement; plus the declarations,
exports and struct layout of the new C-ABI and the build check of csrc/kmeans.hip (kernel descriptors only).  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kmeans_cases as kc
import match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
OPS = ["dinov2_hip_op_kmeans_assign", "dinov2_hip_op_kmeans_update", "dinov2_hip_op_kmeans_plan", "dinov2_hip_op_kmeans", "dinov2_hip_op_kmeans_bench"]


def _update(mutant):
    def fn(x, labels, K, prev, nsplit):
        xhat = mc.normalise_f16(x).astype(np.float32)
        res = kc.emulate_update(xhat, labels, K, prev, nsplit, mutant)
        res["xhat"] = xhat
        return res
    return fn


def _failures(mutant):
    return (kc.kernel_failures(lambda x, c: kc.emulate_assign(x, c, mutant), _update(mutant))
            + kc.run_failures(lambda x, K, m, init: kc.emulate_run(x, K, m, init, mutant)))


def test_restatement_passes_every_case():
    """Shapes under their bounds, probes bit for bit, and on the driver cases the labels, counts, iterations and converged of the float64 run."""
    assert _failures(None) == []


@pytest.mark.parametrize("mutant", kc.MUTANTS)
def test_planted_bugs_are_rejected(mutant):
    failures = _failures(mutant)
    assert failures, f"planted bug {mutant} passed every case"


@pytest.mark.parametrize("which", kc.DRIVER_CASES)
def test_driver_cases_meet_the_margin_condition(which):
    """Every best-minus-second gap of the float64 run is >= 4 tol(H), no `changed` is 0 before the last assignment, the run needs at least 3
    updates, and a centre that starts inside cluster 0 ends up owning the cluster no init row came from."""
    d = kc.driver_case(which)
    x, K = d["x"], d["K"]
    ref = kc.reference_run(x, K, d["max_iter"], x[d["init"]])
    assert kc.margin_ok(ref, x.shape[1]), [(g, ch) for _, g, ch in ref["history"]]
    assert ref["converged"] and ref["iterations"] >= 3
    assert len({int(d["cluster"][i]) for i in d["init"]}) == K - 1  # two init rows from one planted cluster
    # the converged labels are the planted clusters up to a permutation: the orphaned cluster was re-populated by a moved centre
    pairs = {(int(a), int(b)) for a, b in zip(ref["labels"], d["cluster"])}
    assert len(pairs) == K and (ref["counts"] > 0).all()


def test_cases_are_well_formed():
    hdr = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert "KMEANS_K_MAX = 1024, KMEANS_ITER_MAX = 1000, KMEANS_N_MAX = 1 << 20, KMEANS_TARGET_WGS = 256" in hdr
    assert "KMEANS_PARTIAL_MAX = (size_t)32 << 20" in hdr
    assert {s[0] for s in kc.SHAPES} >= {1, 127, 128, 129, 257} and {s[1] for s in kc.SHAPES} >= {1, 2, 128, 129, 300}
    assert {s[2] for s in kc.SHAPES} >= {8, 72, 384, 1536} and (1374, 8, 1024) in kc.SHAPES
    for shape, (chunk, rem) in kc.CHUNK_EDGE.items():
        assert shape in kc.SHAPES and kc.plan(*shape)["chunk"] == chunk and shape[0] % chunk == rem and rem in (1, chunk - 1)
    pr = kc.build_probe("last_chunk")
    spans = kc.chunks(kc.plan(len(pr["x"]), 2, pr["x"].shape[1]))
    a, b = [sp for sp in spans if sp[0] < len(pr["x"])][-1]  # the last chunk that holds real rows, and holds them only in part
    assert a > 0 and len(pr["x"]) < b and np.flatnonzero(pr["labels"] == 1).min() >= a
    for kind in kc.PROBES:  # x^ of every probe row is +-2^-1, +-2^-2 or +-2^-3 (or 0)
        xh = np.abs(mc.normalise_f16(kc.build_probe(kind)["x"]).astype(np.float64))
        assert np.isin(xh, [0.0, 0.5, 0.25, 0.125]).all(), kind


def test_planner_equals_its_restatement(api):
    """kmeans_plan (csrc/kernels.h, through dinov2_hip_op_kmeans_plan; no device) against kmeans_cases.plan, and what it promises."""
    rng = np.random.default_rng(23)
    cases = [s + (ns,) for s in kc.SHAPES for ns in (0, 1, 2, kc.NSPLIT_MAX)]
    cases += [(1369, 8, 1024, 0), (1369, 64, 1024, 0), (43808, 64, 1024, 0), (43808, 256, 1024, 0), (1 << 20, 1024, 4096, 0), (1 << 20, 1024, 4096, 9),
              (1 << 20, 1, 8, 0), (1, 1024, 4096, 0)]
    for _ in range(200):
        cases.append((int(rng.integers(1, 1 << int(rng.integers(1, 21))) + 1), int(rng.integers(1, 1025)), int(rng.integers(8, 4097)),
                      int(rng.choice([0, 0, 1, 3, 17, 4096]))))
    for n, K, H, ns in cases:
        p, q = api.op_kmeans_plan(n, K, H, ns), kc.plan(n, K, H, ns)
        assert {k: p[k] for k in q} == q, (n, K, H, ns)
        assert p["partial_bytes"] <= kc.PARTIAL_MAX and p["bytes"] > p["partial_bytes"], p
        assert p["chunk"] % 64 == 0 and p["nsplit"] >= 1
        spans = kc.chunks(q)  # the chunks partition [0, npad), none empty
        assert spans[0][0] == 0 and spans[-1][1] == p["npad"] and all(a < b for a, b in spans)
        assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
    assert api.op_kmeans_plan(43808, 256, 1024)["nsplit"] * 16 == 256  # 8 x 2 tiles: the update grid fills the device
    for bad in ((0, 1, 8, 0), ((1 << 20) + 1, 1, 8, 0), (1, 0, 8, 0), (1, 1025, 8, 0), (1, 1, 7, 0), (1, 1, 4097, 0), (1, 1, 8, -1)):
        with pytest.raises(ValueError):
            api.op_kmeans_plan(*bad)


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (fails before this feature: the symbols are not there)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    assert re.search(r"\bint\s+dinov2_hip_kmeans_tokens\(", hdr) and "typedef struct dinov2_hip_kmeans {" in hdr
    assert hdr.index("dinov2_hip_bank_topk(") < hdr.index("dinov2_hip_kmeans_tokens(") < hdr.index("typedef struct dinov2_hip_dense_desc")
    assert "enum dinov2_hip_rows_source { DINOV2_HIP_ROWS_GIVEN = 0, DINOV2_HIP_ROWS_LAST_CLS = 1, DINOV2_HIP_ROWS_LAST_PATCHES = 2 };" in hdr
    for name in OPS:
        assert re.search(r"\bint %s\(" % name, ops), name
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert set(OPS) | {"dinov2_hip_kmeans_tokens"} <= exported


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    sec = hdr[hdr.index("spherical k-means of token rows"):hdr.index("int dinov2_hip_kmeans_tokens(")]
    for text in ("contract 1 of dinov2_hip_match", "0 x NaN", "LOWEST c", "bit for bit", "No atomics", "exact integers", "EMPTY cluster keeps its vector",
                 "not unit length", "max_iter = 0", "one 4-byte `changed` per iteration", "Out of scope", "Euclidean", "k-means++", "K > 1024",
                 "bf16 operands", "list forward", "before anything\n * is launched, allocated or copied", "32 MiB", "profiles/kmeans.md"):
        assert text in sec, text


def test_ctypes_struct_matches_the_header(api, tmp_path):
    fields = ["rows", "all_images", "K", "max_iter", "init", "init_centers", "init_rows", "labels", "sim", "centers", "counts", "iterations",
              "converged", "reserved"]
    body = 'std::printf(" %zu", sizeof(dinov2_hip_kmeans));\n' + "".join('std::printf(" %%zu", offsetof(dinov2_hip_kmeans, %s));\n' % f for f in fields)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.KMeans)] + [getattr(api.KMeans, f).offset for f in fields]
    assert (api.KMEANS_INIT_GIVEN, api.KMEANS_INIT_ROWS) == (0, 1)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "dinov2_hip.h"\nint main(void) { dinov2_hip_kmeans k = {{0}};\n'
                   '    int (*f)(dinov2_hip_session *, const dinov2_hip_kmeans *, char *, size_t) = dinov2_hip_kmeans_tokens;\n'
                   '    k.init = DINOV2_HIP_KMEANS_INIT_ROWS;\n'
                   '    return k.K + k.rows.n + (f ? 0 : 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                   check=True, capture_output=True, timeout=120)


# ------------------------------------------------------------------------------------------------------------------- build check
def test_kmeans_cross_compiles_without_scratch(tmp_path):
    """csrc/kmeans.hip compiles for gfx950 and none of its kernels spills (private segment size 0, read from the kernel descriptors); the
    assignment and the update run on the matrix cores; the normaliser is match.hip's, reached through its launcher; no atomics."""
    out = tmp_path / "kmeans.s"
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kmeans.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    txt = out.read_text()
    names = []
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256, name
        names.append(name)
    kinds = ["assign", "fold", "transpose", "update", "finish", "count", "gather"]
    assert len(names) == len(kinds) and all(sum(f"kmeans_{k}_kernel" in n for n in names) == 1 for k in kinds), names
    for k in ("assign", "update"):
        body = txt[txt.index(f"kmeans_{k}_kernel"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        assert "v_mfma_f32_16x16x32_f16" in body, k
    assert "v_rsq_f32" not in txt and "atomic" not in txt
    text = open(src).read()
    assert "match_normalise_kernel" not in text and "launch_match_normalise" in text
