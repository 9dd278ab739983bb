"""dinov2_hip_bank_topk_probe without a GPU: the struct layout, the planner against a brute-force inversion of the probe table, the refusals
by name, and api.ivf_order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import probe_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["queries", "n_seg", "first", "len", "n_probe", "probe", "k", "idx", "sim", "reserved"]
NAMES = {"dinov2_hip_bank_topk_probe", "dinov2_hip_op_bank_probe", "dinov2_hip_op_bank_probe_plan"}


def test_new_symbols_are_declared_and_exported(api, tmp_path):
    """Declared in the headers, exported by the built library (fails before this feature), and api.TopkProbe has the header's layout."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read() + open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    assert all(re.search(r"\bint %s\(" % n, hdr) for n in NAMES) and "typedef struct dinov2_hip_topk_probe" in hdr
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    assert NAMES <= set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    body = 'std::printf(" %zu", sizeof(dinov2_hip_topk_probe));\n' + "".join(
        'std::printf(" %%zu", offsetof(dinov2_hip_topk_probe, %s));\n' % f for f in FIELDS)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.TopkProbe)] + [getattr(api.TopkProbe, f).offset for f in FIELDS]


def _ivf(nq, lists, n_probe, seed):
    """`lists` segments of 100 .. 3000 rows back to back, n_probe distinct random ones per query with a few slots unused."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(100, 3000, lists)
    segments = list(zip((np.cumsum(ln) - ln).tolist(), ln.tolist()))
    probes = np.stack([rng.choice(lists, n_probe, replace=False) for _ in range(nq)]).astype(np.int32)
    probes[rng.random(probes.shape) < 0.1] = -1
    return segments, probes


# (queries, segments, probes, k, piece_tiles, pass_bytes, force_form)
PLANS = {
    "one query": (1, pc.SEGMENTS, pc.all_probes(1), 5, 0, 0, "auto"),
    "subsets, one tile a piece, three passes": (200, pc.SEGMENTS, pc.subset_probes(200), 5, 1, 4 * 5 * 8 * 70, "auto"),
    "all, 1 byte a pass": (17, pc.SEGMENTS, pc.all_probes(17), 64, 1, 1, "narrow"),
    "140 a segment: a wide and a narrow item": (140, pc.SEGMENTS, pc.all_probes(140), 1, 0, 0, "auto"),
    "forced wide": (200, pc.SEGMENTS, pc.subset_probes(200), 64, 2, 0, "wide"),
    "forced narrow": (200, pc.SEGMENTS, pc.subset_probes(200), 64, 0, 0, "narrow"),
    "ivf 64 lists, 8 probes": (1369, *_ivf(1369, 64, 8, 3), 10, 0, 0, "auto"),
    "ivf 64 lists, k = 64, small passes": (300, *_ivf(300, 64, 16, 4), 64, 3, 1 << 16, "auto"),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_planner_inverts_the_probe_table(api, name):
    nq, segments, probes, k, piece_tiles, pass_bytes, form = PLANS[name]
    nb = max(f + n for f, n in segments)
    plan = api.op_bank_probe_plan(nq, nb, 72, segments, probes, k, piece_tiles, pass_bytes, form)
    assert (plan["nq_pad"], plan["hpad"]) == (-(-nq // 128) * 128, 128) and plan["piece_tiles"] == (piece_tiles or plan["piece_tiles"])
    assert 1 <= plan["piece_tiles"] <= 8 and plan["n_wide"] + plan["n_narrow"] == len(plan["items"])
    assert pc.plan_failures(plan, nq, segments, probes, k, pass_bytes, form) == []
    if "three passes" in name:
        assert plan["npass"] >= 3
    if "140" in name:
        assert plan["n_wide"] > 0 and plan["n_narrow"] > 0


REFUSALS = {  # name: (changes to the good request, what the message must name)
    "segments 1 and 3 overlap": (dict(segments=[(0, 4), (4, 4), (8, 2), (7, 1)]), r"segments 1 and 3 overlap"),
    "query 2 probes segment 1 twice": (dict(probes=[[0, 1], [1, -1], [1, 1]]), r"query 2 probes segment 1 twice"),
    "query 1 probes segment 3": (dict(probes=[[0, 1], [3, -1], [2, 1]]), r"query 1 probes segment 3\b"),
    "query 0 probes segment -2": (dict(probes=[[-2, 1], [0, -1], [2, 1]]), r"query 0 probes segment -2\b"),
    "segment 2 outside the bank": (dict(segments=[(0, 4), (4, 4), (8, 3)]), r"segment 2 is rows \[8, 8 \+ 3\)"),
    "segment 0 empty": (dict(segments=[(0, 0), (4, 4), (8, 2)]), r"segment 0 "),
    "k = 65": (dict(k=65), r"k <= 64"),
    "65 probe slots": (dict(probes=np.full((3, 65), -1)), r"n_probe <= 64"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_are_reported_by_name(api, name):
    change, names = REFUSALS[name]
    req = dict(nq=3, nb=10, H=8, segments=[(0, 4), (4, 4), (8, 2)], probes=[[0, 1], [1, -1], [2, 0]], k=2)
    api.op_bank_probe_plan(**req)
    with pytest.raises(ValueError, match=names):
        api.op_bank_probe_plan(**dict(req, **change))
    q, b = np.ones((3, 8), np.float32), np.ones((10, 8), np.float32)
    bad = dict(req, **change)
    with pytest.raises(ValueError):  # the launching op refuses the same request before it touches a device
        api.op_bank_probe(q, b, bad["segments"], bad["probes"], bad["k"])


def test_null_handles_are_refused(api):
    err = C.create_string_buffer(256)
    h, r = C.c_void_p(1), api.TopkProbe()  # (never dereferenced: a NULL beside it is refused first)
    for s, b, req in ((None, h, C.byref(r)), (h, None, C.byref(r)), (h, h, None)):
        assert api.lib().dinov2_hip_bank_topk_probe(s, b, req, err, len(err)) == 4 and b"null" in err.value


@pytest.mark.parametrize("n, lists", [(0, 3), (1, 1), (1000, 7), (50, 64)])
def test_ivf_order_is_a_stable_sort_by_label(api, n, lists):
    lab = np.random.default_rng(n).integers(0, lists, n)
    perm, first, ln = api.ivf_order(lab, lists)
    assert np.array_equal(perm, np.argsort(lab, kind="stable")) and perm.dtype == first.dtype == ln.dtype == np.int32
    assert np.array_equal(ln, np.bincount(lab, minlength=lists)) and np.array_equal(first, np.cumsum(ln) - ln)
    assert all((lab[perm[f:f + c]] == i).all() for i, (f, c) in enumerate(zip(first, ln)))
    with pytest.raises(ValueError):
        api.ivf_order([0, lists], lists)
