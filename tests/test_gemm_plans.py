"""CPU side of the GEMM dispatcher's coverage argument: enumerate, through the library's own plan query
(dinov2_hip_op_gemm_plan -- nothing is launched, no device needed), every kernel plan that the DINOv2 family can reach -- ViT-S / B / L / g,
batch 1 ... 64, 224 and 518 pixels, with and without register tokens, f16 and bf16, all five GEMMs of a layer plus the patch embedding -- and
assert that each (kernel, epilogue, dtype) is launched by a case of tests/gemm_plan_cases.py::COVERAGE_CASES, which
tests/test_gpu_ops.py::test_gemm_plan_coverage_case_bits runs on the GPU and holds to bit-equality with the small-tile kernel."""
import re

import pytest

from gemm_plan_cases import BF16, COVERAGE_CASES, EPI_GELU, EPI_PLAIN, EPI_QKV, EPI_RESID, F16, LN_COVERAGE_CASES, cases_leaves, reachable, reachable_ln

LEAF = re.compile(r"^(gemm2<(128|192|256)>|gemm2_mixed<256\+192>|gemm4<256>|gemm4_mixed<256\+192>|gemm4_short<(64|96|128)>|small<\d+x\d+,w\dx\d,st\d,ks\d>)$")


def test_every_reachable_plan_is_covered(api):
    need = reachable(api)
    have = cases_leaves(api, COVERAGE_CASES)
    missing = sorted(k for k in need if k not in have)
    assert not missing, f"plans no bit-equality case launches (regenerate tests/gemm_plan_cases.py): {[(k, need[k]) for k in missing][:10]}"
    assert all(LEAF.match(leaf) for leaf, _, _ in need), sorted({leaf for leaf, _, _ in need if not LEAF.match(leaf)})
    # the headline shapes land where DESIGN.md section 3 says they do
    assert api.gemm_plan(F16, EPI_GELU, 43968, 4096, 1024) == "gemm4_mixed<256+192>"
    assert api.gemm_plan(F16, EPI_RESID, 43968, 1024, 4096) == "gemm4_mixed<256+192>"
    assert api.gemm_plan(F16, EPI_RESID, 43968, 1024, 1024) == "gemm2_mixed<256+192>"
    assert api.gemm_plan(F16, EPI_QKV, 43968, 3072, 1024).startswith("gemm4<256>;small<")
    assert api.gemm_plan(F16, EPI_QKV, 1374, 3072, 1024) == "gemm4_short<96>"


def test_cases_are_current_and_not_padded(api):
    """every case still reaches a plan that is needed (a dispatcher change must come with a regenerated list), and none is refused"""
    need = reachable(api)
    for case in COVERAGE_CASES:
        got = cases_leaves(api, [case])
        assert got and got <= set(need), case


def test_every_reachable_ln_fold_plan_is_covered(api):
    """The same for the LN-fold launches (epilogues 6 .. 9; forward() with ln_fold): every (kernel, epilogue, dtype) a model of the family can
    reach with the option on is run by tests/test_gpu_ln_fold.py::test_ln_plan_coverage_case_bits, and the list holds nothing stale."""
    need = set(reachable_ln(api))
    have = cases_leaves(api, LN_COVERAGE_CASES)
    assert not (need - have), sorted(need - have)[:10]
    assert not (have - need), sorted(have - need)[:10]
    assert all(leaf.startswith(("gemm4", "small<")) for leaf, _, _ in need)  # (the LN epilogues do not exist in gemm2.hip)


def test_plan_query_refuses_what_launch_gemm_refuses(api):
    with pytest.raises(ValueError):
        api.gemm_plan(F16, EPI_PLAIN, 100, 256, 100)  # K % 64 != 0
    with pytest.raises(ValueError):
        api.gemm_plan(BF16, EPI_PLAIN, 0, 256, 128)


def test_tuning_switch_changes_the_plan_and_resets(api):
    base = api.gemm_plan(F16, EPI_GELU, 43968, 4096, 1024)
    try:
        api.set_tuning("gemm_gen", 2)
        assert api.gemm_plan(F16, EPI_GELU, 43968, 4096, 1024) == "gemm2_mixed<256+192>"
        api.set_tuning("gemm_tile", 128)
        assert api.gemm_plan(F16, EPI_GELU, 43968, 4096, 1024).startswith("small<")
    finally:
        api.reset_tuning("gemm_gen")
        api.reset_tuning("gemm_tile")
    assert api.gemm_plan(F16, EPI_GELU, 43968, 4096, 1024) == base
    with pytest.raises(ValueError):
        api.set_tuning("no_such_switch", 1)


# ---- the plan as data: every part's rectangle and the arguments its kernel would get (api.gemm_plan_parts; no device) ----
EPI_PATCH, EPI_SWIGLU, EPI_RESID_LN = 0, 4, 6
EPI_BASE = {6: EPI_RESID, 7: EPI_QKV, 8: EPI_GELU, 9: EPI_SWIGLU}
LN_GROUP = 64
SMALL = re.compile(r"^small<(\d+)x(\d+),w(\d)x(\d),st(\d),ks(\d)>$")


def family_problems():
    """(epilogue, M, N, K) of every GEMM of the family sweep reachable() / reachable_ln() walk, plus the plain f32 epilogue (5: the head, the
    tests) on each of those shapes, so that all ten epilogues are planned."""
    from gemm_plan_cases import BATCHES, MODELS, REGISTERS, SIDES, model_gemms, model_gemms_ln
    out = set()
    for name in MODELS:
        for b in BATCHES:
            for side in SIDES:
                for r in REGISTERS:
                    for epi, M, N, K in model_gemms(name, b, side, r) + model_gemms_ln(name, b, side, r):
                        if M * max(N, K) * 2 >= 1 << 32:
                            continue
                        out.add((epi, M, N, K))
                        out.add((EPI_PLAIN, M, N, K))
    return sorted(out)


def check_plan_parts(api, dt, epi, M, N, K):
    names = api.gemm_plan(dt, epi, M, N, K).split(";")
    parts = api.gemm_plan_parts(dt, epi, M, N, K)
    what = (dt, epi, M, N, K, names)
    eb = EPI_BASE.get(epi, epi)
    ln = epi >= EPI_RESID_LN
    ldo = N // 2 if eb == EPI_SWIGLU else N
    assert sorted({p["step"] for p in parts}) == list(range(len(names))), what
    # -- the parts tile [0, M) x [0, N) exactly once: inside, pairwise disjoint, areas adding up
    rects = [(p["row0"], p["row0"] + p["rows"], p["col0"], p["col0"] + p["cols"]) for p in parts if p["rows"] > 0]
    for r0, r1, c0, c1 in rects:
        assert 0 <= r0 < r1 <= M and 0 <= c0 < c1 <= N, what
    for i, a in enumerate(rects):
        for b in rects[i + 1:]:
            assert a[1] <= b[0] or b[1] <= a[0] or a[3] <= b[2] or b[3] <= a[2], (what, a, b)
    assert sum((r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in rects) == M * N, what
    # -- one store policy, one clock-probe slot, one statistics layout per logical output (csrc/gemm.hip stamp_args, device_types.h)
    nt_out = int(eb in (EPI_QKV, EPI_GELU, EPI_SWIGLU) and M * ldo * 2 > 48 << 20)
    clk = 0 if eb == EPI_QKV else (3 if K > N else 1) if eb == EPI_RESID else 2 if eb in (EPI_GELU, EPI_SWIGLU) else 5
    gs = 0 if not ln else 12 if (N if epi == EPI_RESID_LN else K) // LN_GROUP <= 12 else 24
    for p in parts:
        assert (p["nt_out"], p["clk_slot"], p["ln_gs"]) == (p["whole_nt_out"], p["whole_clk_slot"], p["whole_ln_gs"]) == (nt_out, clk, gs), (what, p)
    for p in parts:
        name, rows, cols, row0, col0 = names[p["step"]], p["rows"], p["cols"], p["row0"], p["col0"]
        assert (p["M"], p["N"], p["K"], p["ldo"]) == (rows, cols, K, ldo), (what, p)
        # -- each kernel's own preconditions
        if name.startswith("gemm"):
            assert cols % 256 == 0 and (K // 64) % 2 == 0, (what, p)
        if name.startswith("gemm4"):
            assert epi != EPI_PATCH and K % 128 == 0 and K >= 256, (what, p)  # gemm4_ok
        if name.startswith("gemm2"):
            assert not ln and (epi != EPI_PATCH or name == "gemm2<192>"), (what, p)
        if name.startswith("gemm4_short<"):
            h = int(name[len("gemm4_short<"):-1])
            assert cols // 256 * -(-rows // h) <= 256 and eb != EPI_PLAIN and epi != EPI_RESID, (what, p)
        if "mixed" in name and p["part"] == 0:
            assert rows % 256 == 0 and (rows > 0) == ("<256+" in name), (what, p)
        m = SMALL.match(name)
        if m:
            bm, bn, wm, wn, nst, ksub = map(int, m.groups())
            assert (K // 64) % ksub == 0 and (bn // wn == 64 or eb != EPI_SWIGLU), (what, p)
        if epi == EPI_PATCH:
            assert (row0, rows, col0, cols) == (0, M, 0, N), (what, p)
        if eb == EPI_SWIGLU:
            assert (col0, cols) == (0, N), (what, p)
        assert col0 % 256 == 0 and col0 % LN_GROUP == 0, (what, p)
        # -- what the part's arguments add to the caller's pointers, in bytes (dense A and W: K elements of 2 bytes per row)
        osz = 4 if eb in (EPI_PATCH, EPI_RESID, EPI_PLAIN) else 2
        exp = {"off_A": row0 * K * 2, "off_W": col0 * K * 2, "off_bias": col0 * 4, "off_aux": col0 * 4, "off_out": (row0 * ldo + col0) * osz,
               "off_xg": 0, "off_stats": 0, "off_ln_gamma": 0, "off_ln_s": 0, "off_ln_c": 0}
        if epi == EPI_RESID_LN:
            exp.update(off_xg=(row0 * ldo + col0) * 2, off_stats=(row0 * gs + col0 // LN_GROUP) * 8, off_ln_gamma=col0 * 4)
        elif ln:
            exp.update(off_stats=row0 * gs * 8, off_ln_s=col0 * 4, off_ln_c=col0 * 4)
        assert {k: p[k] for k in exp} == exp, (what, p)
        assert p["qcols"] == min(max(N // 3 - col0, 0), cols), (what, p)  # (the plan query asks with qcols = N / 3)
    return len(parts)


@pytest.mark.parametrize("gen", [0, 2, 4])
@pytest.mark.parametrize("tile", [0, 128, 256])
def test_plan_parts_tile_the_output_exactly_once(api, gen, tile):
    """Over the whole family sweep, both dtypes, epilogues 0 .. 9, under every setting of the two GEMM tuning switches: the rectangles of a
    plan's parts are disjoint and cover [0, M) x [0, N); every part carries the whole problem's nt_out / clk_slot / ln_gs; every part
    satisfies its kernel's preconditions; and its pointers sit where its rectangle says (csrc/gemm.hip slice)."""
    try:
        api.set_tuning("gemm_gen", gen)
        api.set_tuning("gemm_tile", tile)
        split = 0
        for epi, M, N, K in family_problems():
            for dt in (F16, BF16):
                split += check_plan_parts(api, dt, epi, M, N, K) > 1
        assert split > 0 or tile == 128  # (the sweep does reach split plans; gemm_tile = 128 is the small-tile kernel alone)
        with pytest.raises(ValueError):
            api.gemm_plan_parts(F16, EPI_PLAIN, 100, 256, 100)  # refused as by the text query: K % 64 != 0
    finally:
        api.reset_tuning("gemm_gen")
        api.reset_tuning("gemm_tile")
