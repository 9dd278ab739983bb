"""Build checks of csrc/vlad.hip from its source text and its gfx950 assembly (kernel descriptors only).  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dinov2.cpp_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_vlad_takes_the_similarity_tile_and_the_one_hot_operand_from_their_single_sources():
    """vlad.hip's assignment must give a pair the bits k-means and match give it, and its sums are k-means' one-hot GEMM: the tile comes from
    csrc/sim_tile.h and the one-hot operand from csrc/onehot_rows.h, which kmeans.hip includes too.  None of the tile's fingerprints that
    test_kernel_build_checks.py::test_similarity_tile_and_its_order_have_a_single_source lists may reappear in vlad.hip, nor a second
    definition of the one-hot operand anywhere."""
    text = open(os.path.join(CSRC, "vlad.hip")).read()
    assert re.search(r'^#include "sim_tile\.h"', text, re.M) and re.search(r'^#include "onehot_rows\.h"', text, re.M)
    for needle in ("(row >> 1) & 7)) << 4", "^ sw) << 4", "^ p.sw) << 4", "mfma16(", "struct Best", "bool better(", "bool before("):
        assert needle not in text, needle
    holders = [f for f in sorted(os.listdir(CSRC)) if "struct OneHotRows" in open(os.path.join(CSRC, f)).read()]
    assert holders == ["onehot_rows.h"], holders
    assert re.search(r'^#include "onehot_rows\.h"', open(os.path.join(CSRC, "kmeans.hip")).read(), re.M)
    # a row's f16 bits come from one routine, csrc/normalise_row.h, for match's kernel and for vlad's kernel over the tile table
    assert re.search(r'^#include "normalise_row\.h"', text, re.M) and "match_normalise_row(" in text
    holders = [f for f in sorted(os.listdir(CSRC)) if "void match_normalise_row(" in open(os.path.join(CSRC, f)).read()]
    assert holders == ["normalise_row.h"], holders
    assert "match_normalise_row(" in open(os.path.join(CSRC, "match.hip")).read() and "sqrtf" not in open(os.path.join(CSRC, "match.hip")).read()
    assert "match_normalise_kernel" not in text and "kmeans_transpose_kernel" not in text and "launch_kmeans_transpose" in text
    # the assignment walk too: sim_tile.h's, for k-means and for vlad
    for f in ("kmeans.hip", "vlad.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert "sim_best_of_rows(" in src and "sim_row_fold(" not in src and "sim_fold_waves(" not in src, f
    assert "vlad.hip" in open(os.path.join(ROOT, "dinov2.cpp_amd", "Makefile")).read()
    # the host side is a file of its own: the waits of the files the stream contract pins stay where they are
    assert "dinov2_hip_vlad_tokens" in open(os.path.join(CSRC, "vlad.cpp")).read()
    assert "dinov2_hip_vlad_tokens" not in open(os.path.join(CSRC, "resident.cpp")).read()


def test_vlad_cross_compiles_without_scratch(tmp_path):
    """csrc/vlad.hip compiles for gfx950 and none of its kernels spills; the assignment and the sums run on the matrix cores; no atomics and
    no approximate reciprocal square root."""
    out = tmp_path / "vlad.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-S", "--cuda-device-only", os.path.join(CSRC, "vlad.hip"),
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    txt = out.read_text()
    names = []
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, desc = m.group(1), m.group(2)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256, name
        names.append(name)
    kinds = ["normalise", "assign", "update", "finish", "l2"]
    assert len(names) == len(kinds) and all(sum(f"vlad_{k}_kernel" in n for n in names) == 1 for k in kinds), names
    for k in ("assign", "update"):
        body = txt[txt.index(f"vlad_{k}_kernel"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        assert "v_mfma_f32_16x16x32_f16" in body, k
    assert "v_rsq_f32" not in txt and "atomic" not in txt
