"""CPU probes of the far-row cases (tests/rows_far_cases.py): the selection rule against its C++ original and its aperiodicity, the
expectation builders against brute force on a scaled-down operand, the dictionary facts they rest on, where each case's byte products sit
against the interface limits, and a break-it check of the planted rows under the address mutants of tests/far_cases.py, in integers.
No GPU; the entry points run in tests/test_gpu_rows_far.py."""
import os
import subprocess

import numpy as np
import pytest

import bank_cases as bc
import far_cases as fc
import kmeans_cases as kc
import match_cases as mc
import rows_far_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- the selection rule
def test_selection_equals_the_cpp_original(tmp_path):
    """far_rows_sel / far_rows_entry of csrc/far_pattern.h built by a plain C++ compiler give what the numpy restatement gives: rows past 2^32,
    several d_common, planted rows at both ends of the list and beside unplanted neighbours; the common entries are all used."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "far_rows_print")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "far_rows_print.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(1)
    rows = [0, 1, 127, 128, 2 ** 20 - 1, 2 ** 24 - 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 63 + 9]
    rows += [int(x) for x in rng.integers(0, 2 ** 34, 64)]
    plants = [(0, 140), (128, 131), (2 ** 24 - 1, 133), (2 ** 32, 150), (2 ** 40 + 3, 132)]
    for d_common, pl in ((rc.D_COMMON, plants), (rc.D_COMMON, []), (1, plants[:1]), (16384, plants), (200, plants[1:])):
        for seed in (0, rc.SEED, 2 ** 63 + 5):
            arg = ",".join("%d:%d" % p for p in pl) or "-"
            out = subprocess.run([exe, str(d_common), arg] + ["%d:%d" % (seed, r_) for r_ in rows], capture_output=True, text=True, timeout=60)
            assert out.returncode == 0, (out.returncode, out.stderr)
            got = np.array(out.stdout.split(), np.int64).reshape(-1, 2)
            exp_sel = rc.sel(seed, rows, d_common)
            exp_ent = exp_sel.copy()
            for r_, e in pl:
                exp_ent[rows.index(r_)] = e
            assert np.array_equal(got[:, 0], exp_sel) and np.array_equal(got[:, 1], exp_ent), (d_common, seed)
            one_by_one = np.array([rc.entries(seed, 1, pl, d_common, row0=r_)[0] for r_ in rows[:12]])  # (uint64 rows: below 2^63 here)
            assert np.array_equal(one_by_one, exp_ent[:12])
    s = rc.sel(rc.SEED, np.arange(1 << 16))
    cnt = np.bincount(s, minlength=rc.D_COMMON)
    assert s.min() == 0 and s.max() == rc.D_COMMON - 1 and cnt.min() > 0.6 * cnt.mean() and cnt.max() < 1.4 * cnt.mean()


@pytest.mark.parametrize("c", [c for c in rc.CASES if not c.host], ids=[c.name for c in rc.CASES if not c.host])
def test_selection_has_no_period_at_the_alias_distances(c):
    """Rows 2^31 / 2^32 bytes apart, at either row width of the case, hold unrelated entries: over 4096 rows the two entries agree about
    once in D_COMMON (a period would make them agree always), and a planted row's alias never holds its rare entry."""
    rng = np.random.default_rng(len(c.name) + c.n)
    rows = rng.integers(0, c.n, 4096)
    ent = rc.sel(rc.SEED, rows)
    planted = dict(c.plant_list)
    seen = 0
    for rb in c.strides:
        for dist in (rc.B31, rc.B32):
            for d in {dist // rb, -(-dist // rb)}:
                for sign in (-1, 1):
                    other = rows + sign * d
                    ok = (other >= 0) & (other < c.n)
                    if ok.sum() < 64:
                        continue
                    seen += 1
                    same = (rc.sel(rc.SEED, other[ok]) == ent[ok]).mean()
                    assert same < 3.0 / rc.D_COMMON, (c.name, rb, d, same)
                for r, e in planted.items():
                    for a in (r - d, r + d):
                        assert planted.get(a, -1) != e or c.rares, (c.name, r, a)
    assert seen > 0


# ------------------------------------------------------------------------------------------------------------- the dictionary
@pytest.mark.parametrize("c", rc.CASES, ids=rc.IDS)
def test_dictionary_facts(c):
    """What the expectations rest on: exactly 4, 16 or 64 non-zeros of +-1 per entry, normalised f16 rows that are exact powers of two,
    every similarity exact in f32 (asserted inside exact_sims), a rare entry at similarity < 1 from every other entry and exactly 1 from its
    copy on the other side, the tie row at exactly 1/2 from four entries and nothing above, the planted rows where the docstring says."""
    dic = c.dictionary()
    D = rc.D_COMMON + c.n_rare
    assert dic.shape == (D, c.H) and len({x.tobytes() for x in dic}) == D
    nnz = (dic != 0).sum(1)
    assert set(np.unique(np.abs(dic))) <= {0.0, 1.0} and set(nnz) <= {4, 16, 64}
    xh = mc.normalise_f16(dic).astype(np.float64)
    assert np.array_equal(np.abs(xh[dic != 0]), (1.0 / np.sqrt(nnz))[np.nonzero(dic)[0]])
    S = rc.exact_sims(dic, dic)
    off = S - 2.0 * np.eye(D)
    assert (np.diag(S) == 1.0).all() and off.max() < 1.0
    other = rc.small_rows(c, dic)
    assert other.shape == (c.small, c.H)
    So = rc.exact_sims(dic, other)
    if c.H >= 16 and c.kind != "kmeans":
        t = rc.exact_sims(dic, rc.tie_row(dic)[None])[:, 0]
        assert (t[:4] == 0.5).all() and t[4:].max() <= 0.5
        assert (other == 0).all(1).sum() == 1  # the zero row
    rows = c.plant_rows
    assert rows[0] == 0 and rows[-1] == c.n - 1 and (c.n - 1) // 128 * 128 in rows and len(rows) <= rc.MAX_PLANTS
    per_entry = np.bincount([e for _, e in c.plant_list], minlength=D)[rc.D_COMMON:]
    assert per_entry.min() >= 1 and (not c.ks or per_entry.max() < max(c.ks))
    # as many rare entries as fit are on the other side, at similarity exactly 1 there and nowhere else
    named = min(c.n_rare, max(c.small - (3 if c.kind == "kmeans" else 2), 1)) if not c.host else c.n_rare
    for i in range(named):
        col = np.flatnonzero(So[rc.D_COMMON + i] == 1.0)
        assert len(col) >= 1 and (np.delete(So[:, col[0]], rc.D_COMMON + i) < 1.0).all(), (c.name, i)
    if not c.host:
        f16, src = c.strides
        for rb, total in ((f16, c.n), (src, c.n if c.far != "bank" else max(c.adds))):
            for byte in (rc.B31, rc.B32, rc.B33):
                if total * rb > byte:
                    r = byte // rb
                    assert {r - 1, r, r // 128 * 128, r // 128 * 128 + 127} <= set(rows), (c.name, rb, byte)


def test_kmeans_cluster_sums_are_exact():
    """K1 / K2: the first update's sums (and the second's) are exact in f32 -- asserted inside expected_kmeans for every cluster -- one cluster
    stays empty and keeps its vector, and the run is not over after the first assignment."""
    for name in ("K1", "K2"):
        c = rc.BY_NAME[name]
        dic = c.dictionary()
        init = rc.small_rows(c, dic)
        ent = c.entries()
        assert np.array_equal(init[-1], init[0])
        e = rc.expected_kmeans(dic, ent, init, 1, _int_assign)
        # (the counts returned are those of the SECOND assignment, in which the repeated centre may win rows from the moved centre 0)
        assert e["counts"].sum() == c.n and np.bincount(e["first"]["labels"], minlength=c.small)[-1] == 0
        assert np.array_equal(_bits(e["centers"][-1]), _bits(init[-1])) and not np.array_equal(_bits(e["centers"][0]), _bits(init[0]))
        assert e["iterations"] == 1 and np.abs(e["centers"]).max() > 64  # sums of many rows
        first = rc.exact_assign(dic, init)
        assert np.array_equal(e["first"]["labels"], first["labels"][ent]) and (first["labels"] != c.small - 1).all()


# ------------------------------------------------------------------------------------------------------------- builders against brute force
def _int_assign(rows, vec):
    """An assignment whose every pair is computed alone: the f16 unit rows as integers (x 2^24), int64 dot products -- exact, so the same
    pair gives the same value whichever rows travel with it -- then float64 -> f32.  The first maximum wins."""
    X = np.round(mc.normalise_f16(rows).astype(np.float64) * 2.0 ** 24).astype(np.int64)
    Cn = np.round(mc.normalise_f16(vec).astype(np.float64) * 2.0 ** 24).astype(np.int64)
    S = ((X @ Cn.T).astype(np.float64) / 2.0 ** 48).astype(np.float32) + np.float32(0.0)
    lab = S.argmax(1).astype(np.int32)
    return {"labels": lab, "sim": S[np.arange(len(S)), lab]}


def _small_case(kind, far, n=3001, small=70, H=72, ks=()):
    """A scaled-down case with the same D, planted rows at both ends and mid-way, and the same tie structure."""
    c = rc.Case("small-" + kind, kind, far, n, small, H, ks=ks, adds=(n,) if far == "bank" else (), extra=(127, 128, n // 2, n - 2))
    dic = c.dictionary()
    ent = c.entries()
    other = rc.small_rows(c, dic)
    return c, dic, ent, other


def test_match_builder_agrees_with_brute_force():
    c, dic, ent, other = _small_case("match", "a")
    a = dic[ent]
    S = mc.reference(a, other)
    e = rc.expected_match(rc.exact_sims(dic, other), ent)
    assert np.array_equal(e["idx_far"], S.argmax(1)) and np.array_equal(e["idx_other"], S.argmax(0))
    S32 = S.astype(np.float32) + np.float32(0.0)
    assert np.array_equal(_bits(e["sim_far"]), _bits(S32.max(1))) and np.array_equal(_bits(e["sim_other"]), _bits(S32.max(0)))
    # the rare entries find their planted rows at similarity exactly 1; the tie row and the repeated common entries are decided by ROW index
    for i, (r, _) in enumerate(c.plant_list):
        assert e["idx_other"][i] == r and e["sim_other"][i] == 1.0 and e["idx_far"][r] == i
    tie = c.n_rare + 1
    winners = np.flatnonzero(np.isin(ent, [0, 1, 2, 3]))
    assert e["sim_other"][tie] == 0.5 and e["idx_other"][tie] == winners[0] and len(set(ent[winners[:8]])) > 1
    # the restatement of the kernels agrees too (exact operands: any order gives these bits)
    em = mc.emulate(a, other)
    for k_far, k_exp in zip(rc.match_result_keys("a"), ("idx_far", "sim_far", "idx_other", "sim_other")):
        assert np.array_equal(em[k_far].view(np.uint32) if em[k_far].dtype == np.float32 else em[k_far],
                              _bits(e[k_exp]) if e[k_exp].dtype == np.float32 else e[k_exp]), k_far


def test_bank_builders_agree_with_brute_force():
    c, dic, ent, other = _small_case("bank", "bank", ks=(64,))
    S = rc.exact_sims(dic, other)
    full = (mc.reference(other, dic[ent]).astype(np.float32) + np.float32(0.0))
    for k in (1, 5, 64):
        e, b = rc.expected_topk_far_bank(S, ent, k), bc.expected_topk(full, k)
        assert np.array_equal(e["idx"], b["idx"]) and np.array_equal(_bits(e["sim"]), _bits(b["sim"])), k
    # a bank shorter than k: the (-1, -inf) tail
    e, b = rc.expected_topk_far_bank(S, ent[:3], 5), bc.expected_topk(full[:, :3], 5)
    assert np.array_equal(e["idx"], b["idx"]) and np.array_equal(_bits(e["sim"]), _bits(b["sim"])) and (e["idx"][:, 3:] == -1).all()
    # far queries against a small bank
    Sq = rc.exact_sims(dic, other)
    fq = (mc.reference(dic[ent], other).astype(np.float32) + np.float32(0.0))
    e, b = rc.expected_topk_far_queries(Sq, ent, 5), bc.expected_topk(fq, 5)
    assert np.array_equal(e["idx"], b["idx"]) and np.array_equal(_bits(e["sim"]), _bits(b["sim"]))
    em = bc.emulate(dic[ent][:400], other, 5)
    assert np.array_equal(em["idx"], e["idx"][:400]) and np.array_equal(_bits(em["sim"]), _bits(e["sim"][:400]))


@pytest.mark.parametrize("max_iter", [0, 1, 2, 5])
def test_kmeans_builder_agrees_with_brute_force(max_iter):
    """expected_kmeans on the dictionary with multiplicities == the same loop on every row (kmeans_cases.emulate_run's loop with the
    pair-by-pair assignment above and exact sums)."""
    c, dic, ent, init = _small_case("kmeans", "x", small=9)
    x = dic[ent]
    e = rc.expected_kmeans(dic, ent, init, max_iter, _int_assign)
    K, n = len(init), len(x)
    xh = mc.normalise_f16(x).astype(np.float64)
    vec, prev, it, conv, counts = init.copy(), None, 0, False, np.zeros(K, np.int32)
    while True:
        a = _int_assign(x, vec)
        changed = n if prev is None else int((a["labels"] != prev).sum())
        prev = a["labels"]
        if changed == 0:
            conv = True
            break
        if it == max_iter:
            counts = np.bincount(prev, minlength=K).astype(np.int32)
            break
        vec, counts = kc.exact_update_expectation(xh, prev, K, vec)
        it += 1
    assert (e["iterations"], e["converged"]) == (it, conv)
    assert np.array_equal(e["labels"], prev) and np.array_equal(_bits(e["sim"]), _bits(a["sim"]))
    assert np.array_equal(e["counts"], counts) and np.array_equal(_bits(e["centers"]), _bits(vec))
    if max_iter == 0:
        ex = rc.exact_assign(dic, init)
        assert np.array_equal(e["labels"], ex["labels"][ent]) and np.array_equal(_bits(e["sim"]), _bits(ex["sim"][ent]))
        ref = kc.emulate_run(x, K, 0, init)
        assert np.array_equal(ref["labels"], e["labels"]) and np.array_equal(_bits(ref["sim"]), _bits(e["sim"]))
    if max_iter >= 1:
        assert np.bincount(e["first"]["labels"], minlength=K)[-1] == 0  # the repeated centre is empty in the first update ...
    if max_iter == 1:
        assert np.array_equal(_bits(e["centers"][-1]), _bits(init[-1]))  # ... which leaves its vector alone


# ------------------------------------------------------------------------------------------------------------- byte products and limits
def test_byte_products_sit_where_the_table_says(api):
    """Each case is accepted by the interface limits of csrc/resident.cpp and the planners, one more row at a limit is refused, and the byte
    quantities the table names pass the boundaries it names."""
    C = rc.BY_NAME
    for c in rc.CASES:
        assert 8 <= c.H <= rc.H_MAX and c.device_bytes() < 40 << 30
        pad = -(-c.n // 128) * 128
        f16, src = pad * c.hpad * 2, c.n * c.H * 4
        if c.kind == "match":
            assert max(c.n, c.small) <= rc.MATCH_N_MAX
        elif c.kind == "kmeans":
            assert c.n <= rc.KMEANS_N_MAX and c.small <= kc.K_MAX
            p = api.op_kmeans_plan(c.n, c.small, c.H)
            assert p == {**kc.plan(c.n, c.small, c.H), "bytes": p["bytes"]}
            assert p["bytes"] > f16 + p["hpad128"] * p["npad"] * 2 and p["bytes"] + src <= c.device_bytes()
        else:
            count, nq = (c.n, c.small) if c.far == "bank" else (c.small, c.n)
            assert count <= rc.BANK_CAP_MAX and nq <= rc.BANK_NQ_MAX and max(c.ks) <= bc.K_MAX
            for k in c.ks:
                assert tuple(api.bank_plan(nq, count, c.H, k)[f] for f in ("chunk_tiles", "nchunks", "pass_tiles", "ntiles")) == bc.plan(nq, count, k)
            if c.far == "bank":
                assert sum(c.adds) == c.n
        if c.name == "M0":
            assert c.n == c.small == mc.PASS + 1 and f16 < rc.B31
        else:
            assert f16 > rc.B32, c.name
    assert C["M1"].n * C["M1"].H * 4 > rc.B33 and (C["M1"].n - 257 - 128) * C["M1"].hpad * 2 <= rc.B32  # just past 2^32
    assert C["M2"].n == rc.MATCH_N_MAX and C["M2"].H % 4 != 0 and C["M2"].n // mc.PASS == 64 and C["M2"].n * C["M2"].H * 4 > rc.B33
    assert C["B1"].n == rc.BANK_CAP_MAX and (C["B1"].adds[0] + C["B1"].adds[1]) * C["B1"].hpad * 2 > rc.B32 and C["B1"].n - 1 > 1 << 23
    assert api.bank_plan(C["B1"].small, C["B1"].n, C["B1"].H, 64)["ntiles"] == 131072
    assert C["B2"].small > 128 and C["B3"].n == rc.BANK_NQ_MAX and C["B3"].n // bc.PASS == 256
    assert C["B3"].n * max(C["B3"].ks) * 4 < rc.B31  # the result offsets idx + r0 * k stay small in bytes: what is far is r0's range
    assert C["K1"].small > 128 and C["K2"].n == rc.KMEANS_N_MAX and C["K2"].H % 4 != 0
    p = kc.plan(C["K1"].n, C["K1"].small, C["K1"].H)
    assert p["hpad128"] * p["npad"] * 2 > rc.B32  # XT: its last rows h start past 2^32 bytes
    # one more row at an interface limit is refused by the planners' front doors (no device)
    with pytest.raises(ValueError):
        api.op_kmeans_plan(rc.KMEANS_N_MAX + 1, 3, 4094)
    with pytest.raises(ValueError):
        api.bank_plan(5, rc.BANK_CAP_MAX + 1, 136, 64)
    with pytest.raises(ValueError):
        api.bank_plan(rc.BANK_NQ_MAX + 1, 300, 4096, 5)
    x = np.zeros((2, 8), np.float32)
    i, f = np.zeros(2, np.int32), np.zeros(2, np.float32)
    for na, nb in ((rc.MATCH_N_MAX + 1, 2), (2, rc.MATCH_N_MAX + 1)):  # dinov2_hip_op_match validates before it touches a device
        assert api.lib().dinov2_hip_op_match(api._ptr(x), na, api._ptr(x), nb, 8, api._ptr(i), api._ptr(f), api._ptr(i), api._ptr(f)) == 4


# ------------------------------------------------------------------------------------------------------------- address mutants
# (case, stage, mutant) triples that move no row of the whole operand, so nothing can see them.  Everything else must be caught.
#   M0: nothing of it is far in bytes (16 385 rows of 128 bytes): it is there for the first-flags of the two reduces.
#   tile / out_wrap32: the tile kernels write a few bytes per row (labels, indices, k-lists: at most 20 MB in all).
#   B2 normalise: a far bank's SOURCE is one add's rows, and B2's adds are 2^17 rows of 16 KiB: 2^31 bytes exactly.  No row's own offset
#   reaches 2^31; only the end of the last tile does, and that is no address anything reads (CURSOR_ONLY: asserted below, not assumed).
NOT_APPLICABLE = {("M0", s, m) for s in rc.STAGES for m in fc.MUTANTS}
NOT_APPLICABLE |= {(c.name, "tile", "out_wrap32") for c in rc.CASES}
NOT_APPLICABLE |= {("B2", "normalise", "a_wrap32"), ("B2", "normalise", "base32")}
CURSOR_ONLY = {("B2", "normalise", "a_signed32")}


def _per_row_signature(c, dic):
    """[D, m] what a far row's checked outputs are made of: its entry's similarities with the other side."""
    return rc.exact_sims(dic, rc.small_rows(c, dic))


@pytest.mark.parametrize("stage", rc.STAGES)
@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_every_address_mutant_is_seen_by_the_planted_rows(mutant, stage):
    """In integers only.  Under each address mutant of far_cases.MUTANTS, applied to the far operand of each case at each stage that walks its
    rows, at least one PLANTED row is read from (or written to) the place of a row with another entry whose similarities with the other side
    differ -- so the planted row's own checked output (its match, its place in a top-k list, its label and sim) cannot come out right, or,
    for a write, the overwritten row's cannot.  The triples a mutant cannot affect are listed above, not skipped over."""
    for c in rc.CASES:
        v = rc.stage_view(c, stage)
        n_stage = max(c.adds) if (c.far == "bank" and stage == "normalise" and mutant != "out_wrap32") else c.n
        applies = fc.any_row_hit(mutant, n_stage, **v)
        assert applies != ((c.name, stage, mutant) in NOT_APPLICABLE), (c.name, stage, mutant, applies)
        if not applies:
            continue
        planted = dict(c.plant_list)
        if n_stage != c.n:  # a far bank's source: rows of one add, the planted rows in the add's own numbering
            rows, at = [], 0
            for a in c.adds:
                rows += [(r - at, r) for r in planted if at <= r < at + a and a == n_stage]
                at += a
            local = np.array([r for r, _ in rows], np.int64)
            glob = np.array([g for _, g in rows], np.int64)
        else:
            local = glob = np.array(sorted(planted), np.int64)
        hit = fc.mutant_hits(mutant, local, **v)
        to, moved = rc.alias_rows(mutant, local, **v)
        if (c.name, stage, mutant) in CURSOR_ONLY:
            assert not rc.alias_rows(mutant, [n_stage - 1], **v)[1].any() and max(c.adds) * v["row_bytes"] == rc.B31
            continue
        assert hit.any() and (moved <= hit).all(), (c.name, stage, mutant)
        dic = c.dictionary()
        sig = _per_row_signature(c, dic)
        seen = 0
        for r_local, g, t, mv in zip(local, glob, to, moved):
            if not mv:
                continue
            if t < 0 or t >= n_stage:  # outside the operand, or inside another row: other data whatever it is
                seen += 1
                continue
            other = int(t + (g - r_local))
            e_own, e_other = planted[int(g)], int(rc.entries(rc.SEED, 1, c.plant_list, row0=other)[0])
            if e_own != e_other and not np.array_equal(sig[e_own], sig[e_other]):
                seen += 1
        assert seen > 0, (c.name, stage, mutant)
