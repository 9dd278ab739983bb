"""dinov2_hip_bank_rerank without a GPU: the struct layout against api.Rerank, the planner's bound and its whole-segment rule, and the
refusals that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["queries", "n_seg", "first", "len", "min_sim", "score_q", "score_b", "mutual", "mutual_sim", "reserved"]
PARTIAL_MAX = 32 << 20


def test_ctypes_struct_matches_the_header(api, tmp_path):
    body = 'std::printf(" %zu", sizeof(dinov2_hip_rerank));\n' + "".join(
        'std::printf(" %%zu", offsetof(dinov2_hip_rerank, %s));\n' % f for f in FIELDS)
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() {\n' + body + "}\n")
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.Rerank)] + [getattr(api.Rerank, f).offset for f in FIELDS]


@pytest.mark.parametrize("n, lens, pass_bytes", [
    (1, [1], 0), (131, [1, 128, 129, 261], 0), (131, [1, 128, 129, 261], 1), (131, [1, 128, 129, 261], 2 * 129 * 128 * 8),
    (1369, [1369] * 100, 0), (16384, [16384, 1, 16384, 16384, 5000], 0), (16384, [16384] * 65536, 0), (1, [1] * 65536, 0)],
    ids=["1x1", "small", "small, 1 byte", "small, two of the largest", "shortlist", "largest rows", "largest list", "shortest rows"])
def test_planner_keeps_its_bound_and_never_splits_a_segment(api, n, lens, pass_bytes):
    """Every segment is in exactly one pass, the passes are runs of the list in order, and the column partials of a pass (query tiles x len
    rounded up to 128 x 8 bytes a segment) stay within the bound -- 32 MiB, or a smaller pass_bytes unless one segment alone is larger."""
    p = api.op_rerank_plan(n, 384, lens, pass_bytes)
    qtiles = -(-n // 128)
    assert (p["nq_pad"], p["hpad"], p["qtiles"]) == (qtiles * 128, 384, qtiles)
    pass_of = p["pass_of"]
    assert pass_of[0] == 0 and pass_of[-1] == p["npass"] - 1 and set(np.diff(pass_of)) <= {0, 1}
    mine = qtiles * 8 * (-(-np.asarray(lens, np.int64) // 128) * 128)
    per_pass = np.bincount(pass_of, weights=mine).astype(np.int64)
    bound = min(pass_bytes or PARTIAL_MAX, PARTIAL_MAX)
    assert per_pass.max() == p["partial_bytes"] <= PARTIAL_MAX
    assert ((per_pass <= bound) | (np.bincount(pass_of) == 1)).all()
    # greedy: a pass ends only where the next segment would not have fitted
    ends = np.flatnonzero(np.diff(pass_of)) + 1
    assert (per_pass[pass_of[ends] - 1] + mine[ends] > bound).all()
    assert np.bincount(pass_of).max() == p["max_segs"]


def test_refusals_that_need_no_device(api):
    L = api.lib()
    err = C.create_string_buffer(256)
    r = api.Rerank()
    h = C.c_void_p(1)  # (never dereferenced: a NULL beside it is refused first)
    for s, b, req in ((None, h, C.byref(r)), (h, None, C.byref(r)), (h, h, None)):
        assert L.dinov2_hip_bank_rerank(s, b, req, err, len(err)) == 4 and b"null" in err.value
    x, one, out = np.ones((4, 8), np.float32), np.ones(1, np.int32), np.zeros(1, np.float32)
    fp, ip = x.ctypes.data_as(C.POINTER(C.c_float)), one.ctypes.data_as(C.POINTER(C.c_int32))
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    zero = np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    good = [fp, 4, fp, 4, 8, zero, ip, 1, -np.inf, 0, op, None, None, None]
    # (argument, value): NULLs, both ends of nq, nb, H and n_seg, len = 0, a range past nb, NaN, a negative pass_bytes
    for i, v in ((0, None), (1, 0), (1, 16385), (2, None), (3, 0), (4, 7), (4, 4097), (5, None), (6, None), (6, zero), (5, ip), (7, 0), (7, 65537),
                 (8, np.nan), (9, -1)):
        args = list(good)
        args[i] = v
        if (i, v) == (5, ip):  # first = 1, len = 4 of nb = 4 rows
            args[6] = (C.c_int32 * 1)(4)
        assert L.dinov2_hip_op_bank_rerank(*args) == 4, (i, v)
    with pytest.raises(ValueError):
        api.op_rerank_plan(16385, 8, [1])
    with pytest.raises(ValueError):
        api.op_rerank_plan(1, 8, [16385])
