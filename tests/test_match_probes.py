"""The numpy restatement of the match contract (tests/match_cases.py) through the very cases tests/test_gpu_match.py applies to the kernels,
and the planted bugs those cases must reject; the float64 reference against its own bound; plus the declarations, exports and struct layout
of the new C-ABI and the build check of csrc/match.hip (kernel descriptors only).  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _failures(mutant):
    def resident(fin, R, ia, ib):
        return mc.emulate(mc.resident_rows(fin, R, ia, mutant), mc.resident_rows(fin, R, ib, mutant), mutant)
    return mc.all_failures(lambda a, b: mc.emulate(a, b, mutant), resident)


def test_restatement_passes_every_case():
    assert _failures(None) == []


@pytest.mark.parametrize("mutant", mc.MUTANTS)
def test_planted_bugs_are_rejected(mutant):
    failures = _failures(mutant)
    assert failures, f"planted bug {mutant} passed every case"


@pytest.mark.parametrize("H", [64, 384, 1536])
def test_restatement_sits_inside_the_bound_with_room(H):
    """Gaussian tokens with two x50 outlier channels: every similarity of the f16 / f32 restatement is within tol = 2^-10 + H 2^-24 of the
    float64 cosine, and uses at most three quarters of it (the bound is neither vacuous nor tight against the format)."""
    a, b = mc.gaussian_tokens(200, H, 1), mc.gaussian_tokens(230, H, 2)
    S = mc.reference(a, b)
    got = mc.normalise_f16(a).astype(np.float32) @ mc.normalise_f16(b).astype(np.float32).T
    err = np.abs(got.astype(np.float64) - S).max()
    assert err <= 0.75 * mc.tol(H), (err, mc.tol(H))


def test_cases_are_well_formed():
    assert (mc.TM, mc.TN) == (128, 128) and mc.PASS == 16384
    hdr = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert "MATCH_TM = 128, MATCH_TN = 128, MATCH_PASS = 128" in hdr  # the cases sit on the kernel's real tile and pass edges
    for kind, H in mc.PROBES:
        a, b, exp = mc.build_probe(kind, H)
        for x in (a, b):
            nz = (x != 0).sum(1)
            assert set(np.unique(nz)) <= {0, 1, 4, 16, 64} and set(np.unique(np.abs(x))) <= {0.0, 1.0}, kind
        assert len(a) % mc.TM and len(b) % mc.TN, kind
    a, b, perm = mc.planted()
    assert len(a) == len(b) == len(perm) and not np.array_equal(np.argsort(perm), perm)  # (swapped directions would show)


# ------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (fails before this feature: the symbols are not there)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    assert re.search(r"\bint dinov2_hip_match_tokens\(", hdr) and "typedef struct dinov2_hip_match" in hdr
    assert re.search(r"\bint dinov2_hip_op_match\(", ops)
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert {"dinov2_hip_match_tokens", "dinov2_hip_op_match"} <= exported


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    for text in ("correctly rounded", "LOWEST index", "depends on H alone", "SAME products", "padding never wins", "never CLS or registers",
                 "profiles/match.md"):
        assert text in hdr, text


def test_ctypes_struct_matches_the_header(api, tmp_path):
    cxx = "g++"  # as tests/test_layer_probes.py: no guard, a missing compiler fails
    fields = ["a", "b", "na", "nb", "H", "image_a", "image_b", "on_device", "idx_ab", "sim_ab", "idx_ba", "sim_ba", "reserved"]
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() { std::printf("%zu", sizeof(dinov2_hip_match));\n'
                   + "".join('std::printf(" %%zu", offsetof(dinov2_hip_match, %s));\n' % f for f in fields) + "}\n")
    exe = tmp_path / "sz"
    subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Mt = api.Match
    assert got == [C.sizeof(Mt)] + [getattr(Mt, f).offset for f in fields]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "dinov2_hip.h"\nint main(void) { dinov2_hip_match m = {0}; int (*f)(dinov2_hip_session *, const dinov2_hip_match *, char *, size_t) = dinov2_hip_match_tokens;\n'
                   '    return m.na + (f ? 0 : 1); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")],
                   check=True, capture_output=True, timeout=120)


# ------------------------------------------------------------------------------------------------------------------- build check
def test_match_cross_compiles_without_scratch(tmp_path):
    """csrc/match.hip compiles for gfx950 and none of its three kernels spills: read from the kernel descriptors (private segment size 0)."""
    out = tmp_path / "match.s"
    src = os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "match.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-S", "--cuda-device-only", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    txt = out.read_text()
    names = []
    for m in re.finditer(r"\.amdhsa_kernel (\w*match_\w+_kernel\w+|\w*match_kernel\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256, name  # one workgroup of 256 per CU at least; no AGPR spill
        names.append(name)
    assert len(names) == 3, names
    assert "v_mfma_f32_16x16x32_f16" in txt and "v_rsq_f32" not in txt  # matrix cores in the hot path; no approximate reciprocal square root
