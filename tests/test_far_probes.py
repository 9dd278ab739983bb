"""CPU probes of the far-offset cases (tests/far_cases.py): the pattern against its C++ original, its aperiodicity, where each case's byte
products sit, what the planner says of each shape and of the shape one row larger, the plan's parts, and a break-it check of the samples in
integers.  No GPU; the kernels run in tests/test_gpu_far.py."""
import os
import subprocess

import numpy as np
import pytest

import far_cases as fc
from test_gemm_plans import check_plan_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_IDS = [c.name for c in fc.GEMM_CASES]
ATTN_IDS = [c.name for c in fc.ATTN_CASES]


def test_pattern_equals_the_cpp_original(tmp_path):
    """csrc/far_pattern.h built by a plain C++ compiler prints the values the numpy restatement gives, rows past 2^32 included; the values are
    multiples of 1/64 in [-1, 1) and use the whole range."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "far_pattern_print")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "far_pattern_print.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(0)
    triples = [(s, r_, c) for s in (0, fc.SEED_A, fc.SEED_QKV, 2 ** 63 + 5) for r_ in (0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 33554430, 2 ** 40 + 3)
               for c in (0, 1, 63, 1023, 6143)]
    triples += [(int(s), int(r_), int(c)) for s, r_, c in zip(rng.integers(0, 100, 64), rng.integers(0, 2 ** 34, 64), rng.integers(0, 6144, 64))]
    out = subprocess.run([exe] + ["%d:%d:%d" % t for t in triples], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    got = [int(x) for x in out.stdout.split()]
    exp = [int(fc.far_q(s, [r_], [c])[0, 0]) for s, r_, c in triples]
    assert got == exp
    q = fc.far_q(fc.SEED_A, np.arange(4096), np.arange(64))
    assert q.min() == -64 and q.max() == 63 and len(np.unique(q)) == 128
    v = fc.far_value(fc.SEED_A, np.arange(64), np.arange(64))
    assert np.array_equal(v * 64, q[:64]) and np.array_equal(v.astype(np.float16).astype(np.float32), v)
    assert not (v.view(np.uint32) & 0xFFFF).any()  # bf16 holds them too: the low 16 bits of the f32 are zero


def _distances(row_bytes):
    return sorted({d for dist in (fc.B31, fc.B32) for d in (dist // row_bytes, -(-dist // row_bytes))})


def _rows_differ(seed, rows, ncols, M, row_bytes):
    """Every row of `rows` differs, over its first ncols columns, from the rows 2^31 and 2^32 bytes away (those inside [0, M))."""
    rows = np.asarray(rows, np.int64)
    cols = np.arange(ncols)
    own = fc.far_q(seed, rows, cols)
    for d in _distances(row_bytes):
        for sign in (-1, 1):
            other = rows + sign * d
            ok = (other >= 0) & (other < M)
            if ok.any():
                same = (own[ok] == fc.far_q(seed, other[ok], cols)).all(1)
                assert not same.any(), (seed, d, rows[ok][same][:4])


@pytest.mark.parametrize("c", fc.GEMM_CASES, ids=GEMM_IDS)
def test_gemm_pattern_has_no_period_at_the_alias_distances(c):
    """A wrapped or sign-flipped offset must land on OTHER data: for the sampled rows of every case, the rows 2^31 and 2^32 bytes away in A and
    in the output (the initial contents of a residual) differ from the row itself."""
    for epi in c.epis:
        rows = fc.gemm_sample(c, epi)
        rows = rows[:: max(1, len(rows) // 512)]
        _rows_differ(fc.SEED_A, rows, 64, c.M, c.a_row_bytes)
        _rows_differ(fc.SEED_A, rows, 64, c.M, c.out_row_bytes(epi))
        if epi == fc.EPI_RESID:
            _rows_differ(fc.SEED_OUT, rows, min(64, c.N), c.M, c.out_row_bytes(epi))
            _rows_differ(fc.SEED_OUT, rows, min(64, c.N), c.M, c.a_row_bytes)
    if c.limit == "W":
        _rows_differ(fc.SEED_W, np.arange(c.N), 64, c.N, c.w_row_bytes)


@pytest.mark.parametrize("c", fc.ATTN_CASES, ids=ATTN_IDS)
def test_attention_pattern_has_no_period_at_the_alias_distances(c):
    rows = fc.attn_rows(c)
    _rows_differ(fc.SEED_QKV, rows, 128, c.B * c.T, c.row_bytes)
    _rows_differ(fc.SEED_QKV, rows, 128, c.B * c.T, c.H * 2)


@pytest.mark.parametrize("c", fc.GEMM_CASES, ids=GEMM_IDS)
def test_gemm_byte_products_sit_at_the_limit(c):
    """The operand at the limit ends below 2^32 bytes and would reach it with one more row; the outputs that the table says pass 2^32 do."""
    if c.limit == "A":
        # G2 is the one case a few panels short of the limit (895 rows, 0.04 %): the M at which the two-height and the split plans appear
        short = -(-fc.B32 // c.a_row_bytes) - 1 - c.M
        assert c.M * c.a_row_bytes < fc.B32 and short == (895 if c.name.startswith("G2") else 0)
        assert c.N * c.w_row_bytes < fc.B32
    elif c.limit == "W":
        assert c.N * c.w_row_bytes < fc.B32 <= (c.N + 1) * c.w_row_bytes
        assert c.M * c.a_row_bytes < fc.B32
    else:
        assert c.M * c.a_row_bytes < fc.B31 and all(c.M * c.out_row_bytes(e) > fc.B32 for e in c.epis)
    assert c.K <= 4096 and c.K % 64 == 0
    if c.name.startswith("G4") or c.name == "G6":
        assert all(c.M * c.out_row_bytes(e) > fc.B32 for e in c.epis if e in (fc.EPI_RESID, fc.EPI_PLAIN_F32))
    if c.name.startswith("G2"):
        assert c.M * c.a_row_bytes == 4293120000
    sample = {e: fc.gemm_sample(c, e) for e in c.epis}
    for e, rows in sample.items():
        assert rows[0] == 0 and rows[-1] == c.M - 1 and len(np.unique(rows)) == len(rows) and len(rows) < 16384
        assert set(range(256)) <= set(rows.tolist()) and set(range((c.M - 1) // 256 * 256, c.M)) <= set(rows.tolist())
        if c.M * c.a_row_bytes > fc.B31:
            r = fc.B31 // c.a_row_bytes  # the row that holds byte 2^31 of A, and its panel
            assert set(range(r // 256 * 256, min(c.M, r // 256 * 256 + 256))) <= set(rows.tolist())
        if c.M * c.out_row_bytes(e) > fc.B32:
            r = fc.B32 // c.out_row_bytes(e)
            assert set(range(r // 256 * 256, min(c.M, r // 256 * 256 + 256))) <= set(rows.tolist())


@pytest.mark.parametrize("c", fc.ATTN_CASES, ids=ATTN_IDS)
def test_attention_byte_products_sit_at_the_limit(c):
    total = c.B * c.T * c.row_bytes
    assert total < c.bound
    # one more row (A2, A3: one more token; A1: one more image is the unit the launcher is handed) reaches the bound
    unit = c.row_bytes if c.B == 1 else c.image_bytes
    assert total + unit >= c.bound
    assert {"A1": 4294717440, "A2": 2147475456, "A3": 4294963200}[c.name] == total
    images, queries = fc.attn_sample(c)
    if c.B > 1:
        b = fc.B31 // c.image_bytes
        assert b * c.image_bytes < fc.B31 <= (b + 1) * c.image_bytes and {0, 1, b, b + 1, c.B - 2, c.B - 1} == set(images)
    else:
        assert set(range(128)) <= set(queries.tolist()) and queries[-1] == c.T - 1 and c.T % 128 != 0


def test_planner_accepts_each_shape_and_refuses_one_more_row(api):
    """The plan text of every GEMM run is the one the case table states, strides included; the same shape with one more row of the operand at
    the limit is refused, by the planner and by the far op itself (which then allocates and launches nothing, so this needs no device)."""
    leaves = set()
    try:
        for c, epi, gen, dt, rid in fc.gemm_runs():
            api.set_tuning("gemm_gen", gen)
            plan = api.gemm_plan(dt, epi, c.M, c.N, c.K, c.lda, c.ldw)
            assert plan == c.plan(gen, epi), rid
            assert plan == api.gemm_plan(dt, epi, c.M, c.N, c.K), rid  # the stride does not enter the plan
            leaves |= set(plan.split(";"))
            if c.limit == "out":  # (nothing bounds an output's size: its offsets are 64-bit)
                continue
            M1, N1 = (-(-fc.B32 // c.a_row_bytes), c.N) if c.limit == "A" else (c.M, c.N + 1)
            assert (M1, N1) in ((c.M + 1, c.N), (c.M, c.N + 1)) or c.name.startswith("G2")
            if c.limit == "A":
                assert api.gemm_plan(dt, epi, M1 - 1, N1, c.K, c.lda, c.ldw)  # the last shape that is taken (G2: 895 rows past the case)
            with pytest.raises(ValueError):
                api.gemm_plan(dt, epi, M1, N1, c.K, c.lda, c.ldw)
            W = np.zeros((N1, c.K), np.float32)
            with pytest.raises(ValueError):
                api.op_gemm_far(dt, epi, M1, N1, c.K, W, np.zeros(N1, np.float32), np.zeros(N1, np.float32), [0], lda=c.lda, ldw=c.ldw)
    finally:
        api.reset_tuning("gemm_gen")
    for want in fc.LEAVES_WANTED:
        assert any(leaf.startswith(want) for leaf in leaves), (want, sorted(leaves))
    assert len({leaf for leaf in leaves if leaf.startswith("small<")}) >= 2
    with pytest.raises(ValueError):
        api.gemm_plan(0, fc.EPI_GELU, 2097152, 256, 1024)
    for c in fc.ATTN_CASES:
        if c.bound == fc.B32:  # (A2 sits under the limit of a PASS; the launcher takes it and more)
            B1, T1 = (c.B + 1, c.T) if c.B > 1 else (1, c.T + 1)
            with pytest.raises(ValueError):
                api.op_attention_far(0, B1, T1, c.nh, [0])


@pytest.mark.parametrize("c", fc.GEMM_CASES, ids=GEMM_IDS)
def test_plan_parts_tile_the_output_once_with_64_bit_offsets(api, c):
    """check_plan_parts (tests/test_gemm_plans.py) on the far shapes: the parts tile the output exactly once and every part's pointers are
    advanced by the 64-bit products slice() should give -- here past 2^32 for the outputs of G4 and G6."""
    try:
        far = 0
        for gen in sorted({g for g, _ in c.runs}):
            api.set_tuning("gemm_gen", gen)
            for epi in c.epis:
                for dt in sorted({d for _, d in c.runs}):
                    check_plan_parts(api, dt, epi, c.M, c.N, c.K)
                    far = max([far] + [p["off_out"] for p in api.gemm_plan_parts(dt, epi, c.M, c.N, c.K)])
        if c.name in ("G2-split", "G6"):
            assert far > 0  # a split plan: its second part starts inside the output
    finally:
        api.reset_tuning("gemm_gen")


# (case name, mutant) pairs that move no row of the whole problem, so no sample can see them.  Everything else must be caught.
#   out_wrap32: only G4 (f32 output) and G6 write past 2^32 bytes.  G5's A and output are small; its operand at the limit is W, whose 512 rows
#   are two whole panels: the second starts 4 096 bytes below 2^31 and ends below 2^32.  G2's M is a multiple of 256, so its last panel ends
#   where A ends.  G6's A is small: only its output is far.
#   A2 sits below 2^31 with its rows, its tile-ahead cursor passes 2^31 but not 2^32, and has one image (base 0), as has A3.
OUT_PAST_32 = {("G2-split", fc.EPI_RESID), ("G4-64", fc.EPI_PLAIN_F32), ("G4-128", fc.EPI_PLAIN_F32), ("G6", fc.EPI_RESID)}
NOT_APPLICABLE = {
    ("G2-mixed", "a_wrap32"), ("G2-split", "a_wrap32"), ("G5", "a_wrap32"), ("G5", "base32"),
    ("G6", "a_signed32"), ("G6", "a_wrap32"), ("G6", "base32"),
    ("A1", "out_wrap32"), ("A2", "out_wrap32"), ("A3", "out_wrap32"), ("A2", "a_wrap32"), ("A2", "base32"), ("A3", "base32"),
}


@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_every_address_mutant_is_seen_by_the_sample(mutant):
    """In integers only.  Under each mutant of far_cases.MUTANTS at least one sampled row must be read from or written to another address than
    it should be; a write mutant is also seen by the untouched count (a row written elsewhere leaves its own place untouched: offsets only
    wrap DOWN, so nothing else lands there).  The pairs where the mutant moves no row of the whole problem are listed, not skipped over: a case
    that stops being at its limit would fall into the list's complement and fail here."""
    for c in fc.GEMM_CASES:
        for epi in c.epis:
            v = fc.gemm_mutant_view(c, epi)
            kw = dict(row_bytes=v["row_bytes"], out_row_bytes=v["out_row_bytes"], tile=v["tile"], group=v["group"])
            n_all = c.N if c.limit == "W" else c.M
            applies = fc.any_row_hit(mutant, n_all, **kw)
            seen = bool(fc.mutant_hits(mutant, v["rows"], **kw).any())
            listed = (c.name, mutant) in NOT_APPLICABLE
            if mutant == "out_wrap32":  # by epilogue: the f32 outputs of these pass 2^32 bytes, no two-byte output does
                listed = (c.name, epi) not in OUT_PAST_32
            assert applies != listed, (c.name, fc.EPI_NAME[epi], mutant, applies)
            assert seen == applies, (c.name, fc.EPI_NAME[epi], mutant)
    for c in fc.ATTN_CASES:
        v = fc.attn_mutant_view(c)
        kw = dict(row_bytes=v["row_bytes"], out_row_bytes=v["out_row_bytes"], tile=v["tile"], group=v["group"])
        applies = fc.any_row_hit(mutant, v["M"], **kw)
        rows = v["write_rows"] if mutant == "out_wrap32" else v["read_rows"]
        seen = bool(fc.mutant_hits(mutant, rows, **kw).any())
        assert applies != ((c.name, mutant) in NOT_APPLICABLE), (c.name, mutant, applies)
        assert seen == applies, (c.name, mutant)
