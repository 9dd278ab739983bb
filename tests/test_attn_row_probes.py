"""The numpy restatement of attn_rows_kernel (tests/attn_row_cases.py) through the very probes tests/test_gpu_attn_rows.py applies to the
kernel, and the planted bugs those probes must reject; the float64 reference against its own bound; plus the declarations, exports and
struct layout of the new C-ABI and the build check of csrc/attn_rows.hip (kernel descriptors only).  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import attention_cases as ac
import attn_row_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# B > 1, nh > 1, T past key 64, not a multiple of 32, a view that drops columns: every planted bug has something to get wrong
B, T, NH = 3, 70, 2
QUERIES = [[0], [0, T - 1], [1, T // 2], list(range(T))]
VIEWS = [(0, T), (5, T - 5)]


def _run_probes(dt, mutant):
    """Every probe x query set x view through `emulate`; returns the list of failure messages."""
    failures = []
    for kind in rc.PROBES:
        qkv, exp = rc.build_probe(kind, B, T, NH, seed=7)
        for qs in QUERIES:
            full = rc.emulate(qkv, B, T, NH, dt, qs, mutant=mutant)
            for key0, nkeys in VIEWS:
                got = full if (key0, nkeys) == (0, T) else rc.emulate(qkv, B, T, NH, dt, qs, key0, nkeys, mutant=mutant)
                ok, msg = rc.check_probe(kind, got, rc.expected_view(exp, qs, key0, nkeys), "nq=%d view=%s" % (len(qs), (key0, nkeys)))
                if not ok:
                    failures.append(msg)
                ok, msg = rc.check_exact(got, full[..., key0:key0 + nkeys], "view %s vs columns of the full view" % ((key0, nkeys),))
                if not ok:
                    failures.append(msg)
    return failures


@pytest.mark.parametrize("dt", [ac.F16, ac.BF16])
def test_restatement_passes_every_probe(dt):
    assert _run_probes(dt, None) == []


@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_planted_bugs_are_rejected(mutant):
    failures = _run_probes(ac.F16, mutant)
    assert failures, f"planted bug {mutant} passed every probe"


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 2), (1, 63, 1), (1, 65, 2), (3, 261, 2)], ids=rc.shape_id)
def test_probes_are_well_formed_at_the_gpu_shapes(shape):
    """The expected rows of every probe sum to exactly 1, and the restatement reproduces them at the small GPU shapes."""
    b, t, nh = shape
    for kind in rc.PROBES:
        qkv, exp = rc.build_probe(kind, b, t, nh, seed=3)
        assert np.abs(exp.sum(-1) - 1.0).max() < 1e-12, kind
        if kind != "uniform":  # (its k is random and does not matter: q = 0)
            assert np.array_equal(ac.round_t(qkv, ac.BF16)[:, :2 * nh * 64], qkv[:, :2 * nh * 64]), kind + ": q, k not exact in bf16"
        qs = rc.query_sets(t)[-1]
        ok, msg = rc.check_probe(kind, rc.emulate(qkv, b, t, nh, ac.BF16, qs), rc.expected_view(exp, qs, 0, t), rc.shape_id(shape))
        assert ok, msg


@pytest.mark.parametrize("regime", ac.REGIMES)
@pytest.mark.parametrize("dt", [ac.F16, ac.BF16])
def test_reference_sits_inside_its_own_bound_and_so_does_the_restatement(dt, regime):
    """The float64 reference rounded to f32 uses at most a quarter of the bound (room to spare: the bound is not vacuous at f32 resolution
    and not tighter than the output format), and the restatement of the kernel's arithmetic is inside it, with rows that sum to 1."""
    b, t, nh = 3, 261, 2
    qkv = ac.regime_input(regime, b, t, nh, dt, True, seed=11)
    qs = list(range(t))
    P, S, M = rc.reference(qkv, b, t, nh, qs)
    bound = rc.error_bound(P, S, M, t)
    assert (np.abs(P.astype(np.float32).astype(np.float64) - P) <= 0.25 * bound).all()
    got = rc.emulate(qkv, b, t, nh, dt, qs)
    ok, msg = rc.check_against_reference(got, P, bound, regime)
    assert ok, msg
    ok, msg = rc.check_rows_sum_to_one(got, t, regime)
    assert ok, msg


def test_query_sets_and_views():
    assert rc.query_sets(1) == [[0]]
    assert rc.query_sets(2) == [[0], [0, 1]]
    assert rc.query_sets(63)[-1] == list(range(63)) and [1, 31] in rc.query_sets(63)
    assert len(rc.query_sets(1374)) == 3
    assert rc.key_views(2) == [(0, 2)] and rc.key_views(65) == [(0, 65), (5, 60)]
    assert rc.denominator_depth(1) == 9 and rc.denominator_depth(4101) == 25


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (fails before this feature: the symbols are not there)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    assert re.search(r"\bint dinov2_hip_predict_attention\(", hdr) and "typedef struct dinov2_hip_attention" in hdr
    assert re.search(r"\bint dinov2_hip_op_attn_rows\(", ops)
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert {"dinov2_hip_predict_attention", "dinov2_hip_op_attn_rows"} <= exported


def test_header_documents_convention_contract_and_scope():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    for text in ("attentions[k - 1]", "get_last_selfattention", "NOT", "layer_tap", "dinov2_hip_group_", "DINOV2_HIP_ATTN_KEYS_PATCHES"):
        assert text in hdr, text


def test_ctypes_struct_matches_the_header(api, tmp_path):
    cxx = "g++"  # as tests/test_layer_probes.py: no guard, a missing compiler fails
    fields = ["layers", "n_layers", "queries", "n_queries", "keys", "probs", "on_device", "reserved"]
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() { std::printf("%zu", sizeof(dinov2_hip_attention));\n'
                   + "".join('std::printf(" %%zu", offsetof(dinov2_hip_attention, %s));\n' % f for f in fields) + "}\n")
    exe = tmp_path / "sz"
    subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    At = api.Attention
    assert got == [C.sizeof(At)] + [getattr(At, f).offset for f in fields]
    assert (api.ATTN_KEYS_ALL, api.ATTN_KEYS_PATCHES) == (0, 1)


# ------------------------------------------------------------------------------------------------------------------- build check
def test_attn_rows_cross_compiles_without_scratch(tmp_path):
    """csrc/attn_rows.hip compiles for gfx950 and no kernel of it spills: read from the kernel descriptors (private segment size 0, scratch
    disabled), six kernels = f16 | bf16 x (8 queries, 1 query, two-pass)."""
    out = tmp_path / "attn_rows.s"
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "attn_rows.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    txt = out.read_text()
    n = 0
    for m in re.finditer(r"\.amdhsa_kernel (\w*attn_rows_kernel\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        en = re.search(r"\.amdhsa_enable_private_segment (\d+)|\.amdhsa_scratch_en (\d+)", desc)
        assert en is None or int(en.group(1) or en.group(2)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 128, name  # two workgroups of 256 per CU at least
        n += 1
    assert n == 6, n
