"""The NaN tracers of tests/tracer_cases.py are worth running (no GPU): for every placement the GPU tests use, the definition's clean output is
finite and the expected footprint is non-empty and -- but for the deliberate dense sweeps -- a strict subset of the output; the unmutated numpy
emulators pass check_footprint; and every planted mutant, none of which the finite-data tests can see, fails a placement that the test
NAMES.  A mutant no placement catches is a gap in the placements."""
import numpy as np
import pytest

import attention_cases as ac
import attn_row_cases as rc
import layer_cases as lyc
import list_cases as lc
import misc_cases as mc
import tracer_cases as tc
from gemm_plan_cases import COVERAGE_CASES, LN_COVERAGE_CASES

EPIS = (tc.EPI_PATCH, tc.EPI_QKV, tc.EPI_RESID, tc.EPI_GELU, tc.EPI_SWIGLU, tc.EPI_RESID_LN, tc.EPI_QKV_LN, tc.EPI_GELU_LN, tc.EPI_SWIGLU_LN)
LEAVES = [(0, 100, 64), (100, 50, 32)]  # a ragged main leaf and a tail of another tile height, as a split plan hands them out
M_, N_, K_ = 150, 256, 256


def _ok(res):
    assert res[0], res[1]


# ------------------------------------------------------------------------------------------------------------------- the checker itself
def test_check_footprint_names_each_kind_of_failure():
    clean = np.arange(12, dtype=np.float32).reshape(3, 4)
    mask = np.zeros((3, 4), bool)
    mask[1] = True
    good = clean.copy()
    good[1] = np.nan
    _ok(tc.check_footprint(good, clean, mask, "good"))
    wide = good.copy()
    wide[2, 3] = np.nan
    ok, msg = tc.check_footprint(wide, clean, mask, "wide")
    assert not ok and "(2, 3) is NaN and must not depend" in msg
    narrow = good.copy()
    narrow[1, 2] = 6.0
    ok, msg = tc.check_footprint(narrow, clean, mask, "narrow")
    assert not ok and "(1, 2) is 6.0 and must be NaN" in msg
    moved = good.copy()
    moved[0, 1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    ok, msg = tc.check_footprint(moved, clean, mask, "moved")
    assert not ok and "(0, 1) is outside the footprint and changed" in msg
    negzero = good.copy()
    negzero[0, 0] = -0.0  # equal as a number, other bits
    assert not tc.check_footprint(negzero, clean, mask, "-0")[0]
    unwritten = clean.copy()
    unwritten[2, 0] = np.nan
    ok, msg = tc.check_footprint(unwritten, unwritten, mask, "unwritten")
    assert not ok and "the clean launch is not finite at (2, 0)" in msg
    assert not tc.check_footprint(good[:2], clean, mask, "shape")[0]


# ------------------------------------------------------------------------------------------------------------------- GEMM
def _emulate(epi, c, mutant=None):
    out = tc.emulate_gemm(epi, c["A"], c["W"], LEAVES, mutant=mutant, bias=c.get("bias"), aux=c.get("aux"), x0=c.get("x0"),
                          stats=c.get("stats"), s=c.get("s"), c=c.get("c"), gamma=c.get("gamma"), **c["kw"])
    return [np.asarray(o, np.float32) for o in (out if isinstance(out, tuple) else (out,))]


def _placements(epi, c):
    heights, row0 = [[th] for _, _, th in LEAVES], [r0 for r0, _, _ in LEAVES[1:]]
    return tc.gemm_sweeps(epi, c, heights, row0) + [(n, k, w, False) for n, k, w in tc.gemm_side_tracers(epi, c)]


def _failing(epi, c, mutant):
    """Names of the placements at which the emulator (with `mutant`) fails check_footprint in some output."""
    clean = _emulate(epi, c, mutant)
    bad = []
    for name, key, where, _ in _placements(epi, c):
        p = tc.poisoned(c, key, where)
        got, masks = _emulate(epi, p, mutant), tc.gemm_expected(epi, p)
        if not all(tc.check_footprint(g, cl, m, name)[0] for g, cl, m in zip(got, clean, masks)):
            bad.append(name)
    return bad


@pytest.mark.parametrize("epi", EPIS)
def test_gemm_placements_are_informative_and_the_emulator_passes(epi):
    c = tc.gemm_case(tc.F16, epi, M_, N_, K_)
    clean = _emulate(epi, c)
    assert all(np.isfinite(o).all() for o in clean)
    for name, key, where, dense in _placements(epi, c):
        p = tc.poisoned(c, key, where)
        masks = tc.gemm_expected(epi, p)
        assert any(tc.informative(m, dense) for m in masks), name
        assert dense or all(int(m.sum()) < m.size for m in masks), name
        # the dependence shortcut of A W^T and the identity that stands for GELU / SiLU have the footprint of the real arithmetic
        full = tc.gemm_expected(epi, p, h=tc.gemm_h(p["A"], p["W"]))
        for m, f in zip(masks, full):
            assert np.array_equal(m, f), name
        for g, cl, m in zip(_emulate(epi, p), clean, masks):
            _ok(tc.check_footprint(g, cl, m, "epilogue %d, %s" % (epi, name)))
    assert _failing(epi, c, None) == []


def test_activations_have_the_dependence_of_their_argument():
    v = np.array([np.nan, -30.0, -9.0, -1e-3, 0.0, 2.5, 11.0, 80.0])
    for epi in (tc.EPI_GELU, tc.EPI_SWIGLU):
        a = tc.activation(epi, v, np.full_like(v, 1.5))
        assert np.array_equal(np.isnan(a), np.isnan(v)) and np.isfinite(a[1:]).all()
    assert np.isnan(tc.activation(tc.EPI_SWIGLU, np.array([0.0, 3.0]), np.array([np.nan, np.nan]))).all()  # silu(0) * NaN is NaN too


# mutant -> (epilogue it is planted under, the placement that must catch it, by the start of its name)
GEMM_CATCHES = {
    "k_tile_skipped": (tc.EPI_GELU, "sparse A"),               # (64, 64): the first row of the second tile, in the second K step
    "tail_rows_from_next_matrix": (tc.EPI_QKV, "sparse A"),    # (100, K - 64): the first row handed to the tail leaf; row 99 must stay clean
    "rows_swapped_in_tile": (tc.EPI_RESID, "sparse A"),        # (63, 63): the last row of the first tile
    "x1_x2_swapped": (tc.EPI_SWIGLU, "sparse W"),              # weight rows 69 (x1 of unit 37) and 167 (x2 of unit 71)
    "bias_of_neighbour_column": (tc.EPI_GELU, "bias["),
    "stats_of_neighbour_row": (tc.EPI_QKV_LN, "stats["),
}


@pytest.mark.parametrize("mutant", tc.GEMM_MUTANTS)
def test_every_gemm_mutant_is_caught_by_a_named_placement(mutant):
    epi, placement = GEMM_CATCHES[mutant]
    c = tc.gemm_case(tc.F16, epi, M_, N_, K_)
    # finite data cannot show it where the skipped / leaked operand contributes nothing: the clean launch of the mutant is finite
    assert all(np.isfinite(o).all() for o in _emulate(epi, c, mutant))
    bad = _failing(epi, c, mutant)
    assert any(b.startswith(placement) for b in bad), "%s: caught by %r, expected by %r" % (mutant, bad, placement)


def test_k_tile_and_dropped_product_show_in_the_dense_sweep():
    """A dropped product anywhere shows as a finite element of the dense A sweep: the second K step of the second row tile is hit by the rows
    r of that tile with 64 <= 7 r mod K < 128."""
    c = tc.gemm_case(tc.F16, tc.EPI_GELU, M_, N_, K_)
    assert any(64 <= (7 * r) % K_ < 128 for r in range(64, 100))
    assert "dense A, k = 7 r mod K" in _failing(tc.EPI_GELU, c, "k_tile_skipped")


@pytest.mark.parametrize("cases", [COVERAGE_CASES, LN_COVERAGE_CASES], ids=["plain", "ln"])
def test_gpu_gemm_placements_follow_the_plans(api, cases):
    """For every coverage case the GPU test runs: the plan string parses, each sparse row is planted once and lies inside M, every tile height of
    the plan and every later leaf's first row has its tracers, and the sparse footprints (rows x N, M x columns) are strict subsets."""
    for dt, epi, M, N, K in cases:
        plan = api.gemm_plan(dt, epi, M, N, K)
        heights = tc.plan_heights(plan)
        parts = api.gemm_plan_parts(dt, epi, M, N, K)
        row0, col0 = tc.plan_edges(parts)
        assert (len(row0) + len(col0) > 0) == (";" in plan or "+" in plan and "<0+" not in plan), (plan, row0, col0)
        tr = tc.a_tracers(M, K, heights, row0)
        rows = [r for r, _ in tr]
        assert len(set(rows)) == len(rows) and 0 in rows and M - 1 in rows and all(0 <= r < M and 0 <= k < K for r, k in tr)
        assert all(k in tc.k_choices(K) for _, k in tr)
        for h in {h for hs in heights for h in hs}:
            if h < M:
                assert dict(tr)[h - 1] == 63 and dict(tr)[h] == 64, (plan, h)
        assert all(r in rows for r in row0)
        cols = tc.w_cols(epi, N, N // 3, col0)
        assert len(rows) < M and len(cols) < N and {0, N - 1} <= set(cols) and all(c in cols and c - 1 in cols for c in col0)
        if epi in (tc.EPI_SWIGLU, tc.EPI_SWIGLU_LN):
            oc = tc.swiglu_out_col(N)
            assert oc[69] == 37 and oc[128 + 32 + 7] == 71 and oc[64 + 32 + 5] == 37


# ------------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("log2", [True, False], ids=["log2", "exp"])
@pytest.mark.parametrize("T", tc.ATTN_T)
def test_attention_placements(T, log2):
    B, nh = tc.ATTN_B, tc.ATTN_NH
    qkv = ac.regime_input("random", B, T, nh, ac.F16, log2, seed=T)
    clean = ac.emulate(qkv, B, T, nh, ac.F16, log2)
    assert np.isfinite(ac.reference(qkv, B, T, nh, log2, want_stats=False)[0]).all() and np.isfinite(clean).all()
    mutant_clean = ac.emulate(qkv, B, T, nh, ac.F16, log2, mutant="mask_by_multiply")
    assert np.array_equal(mutant_clean, clean)  # finite data cannot tell the mutant from the kernel
    caught = []
    for name, where in tc.attn_placements(T):
        p = tc.plant(qkv, where)
        mask = tc.attn_footprint(p, B, T, nh, log2)
        assert tc.informative(mask), name
        assert not mask.reshape(B, T, nh, 64)[:, :, 0].any() or not mask.reshape(B, T, nh, 64)[:, :, 1].any(), name  # one head only
        _ok(tc.check_footprint(ac.emulate(p, B, T, nh, ac.F16, log2), clean, mask, name))
        if not tc.check_footprint(ac.emulate(p, B, T, nh, ac.F16, log2, mutant="mask_by_multiply"), mutant_clean, mask, name)[0]:
            caught.append(name)
    if T % ac.KT:  # a key tail exists: image 0's is staged from image 1's first keys
        assert "k row 0 of image 1 head 0" in caught and any(n.startswith("v[0, ") and "image 1" in n for n in caught), caught
    else:
        assert caught == []


def test_attention_footprints_in_closed_form():
    """What the reference says, spelled out: a q tracer is its row of its head; a k tracer every query and column of its (image, head); a v
    tracer one column of its head for every query -- also where the probability underflows to 0 (0 x NaN is NaN)."""
    B, T, nh = 2, 129, 2
    qkv = ac.regime_input("peaky", B, T, nh, ac.F16, True, seed=5)
    m = tc.attn_footprint(tc.plant(qkv, [tc.attn_index("q", 1, 0, 64, T, nh, 9)]), B, T, nh, True).reshape(B, T, nh, 64)
    e = np.zeros_like(m)
    e[1, 64, 0] = True
    assert np.array_equal(m, e)
    m = tc.attn_footprint(tc.plant(qkv, [tc.attn_index("k", 0, 1, 128, T, nh, 0)]), B, T, nh, True).reshape(B, T, nh, 64)
    e[:] = False
    e[0, :, 1] = True
    assert np.array_equal(m, e)
    m = tc.attn_footprint(tc.plant(qkv, [tc.attn_index("v", 1, 1, 3, T, nh, 17)]), B, T, nh, True).reshape(B, T, nh, 64)
    e[:] = False
    e[1, :, 1, 17] = True
    assert np.array_equal(m, e)


@pytest.mark.parametrize("name", ["edges", "long_first"])
def test_list_attention_placements(name):
    T, nh = lc.SEGMENTS[name], 2
    if name == "long_first":
        T = [200, 6, 261]  # the emulation of 1374 tokens is the GPU test's business; the placement rule is the same
    qkv = lc.segment_input(T, nh, ac.F16, True, seed=11)
    clean = lc.emulate_list(qkv, T, nh, ac.F16, True)
    leaky = lc.emulate_list(qkv, T, nh, ac.F16, True, mutant="neighbour_keys_staged")
    caught = []
    for pname, where in tc.list_placements(T, nh):
        p = tc.plant(qkv, where)
        mask = tc.list_footprint(p, T, nh, True)
        assert tc.informative(mask), pname
        _ok(tc.check_footprint(lc.emulate_list(p, T, nh, ac.F16, True), clean, mask, pname))
        if not tc.check_footprint(lc.emulate_list(p, T, nh, ac.F16, True, mutant="neighbour_keys_staged"), leaky, mask, pname)[0]:
            caught.append(pname)
    assert any(n.startswith("k row 0 of segment %d" % (len(T) - 1)) for n in caught), caught  # the last segment's first key, staged by the one before


def test_attn_rows_placements():
    B, T, nh, queries, key0, nkeys = 2, 129, 2, [0, 64, 128], 5, 70
    qkv = ac.regime_input("random", B, T, nh, ac.F16, True, seed=3)
    clean = rc.emulate(qkv, B, T, nh, ac.F16, queries, key0, nkeys)
    assert np.isfinite(clean).all()
    for name, where, rows in (("k inside the window", [tc.attn_index("k", 1, 0, 40, T, nh, 2)], (1, 0, slice(None))),
                              ("k outside the window", [tc.attn_index("k", 1, 0, 100, T, nh, 2)], (1, 0, slice(None))),
                              ("q of a requested query", [tc.attn_index("q", 0, 1, 64, T, nh, 5)], (0, 1, 1)),
                              ("q of an unrequested query", [tc.attn_index("q", 0, 1, 63, T, nh, 5)], None)):
        p = tc.plant(qkv, where)
        mask = tc.attn_rows_footprint(p, B, T, nh, queries, key0, nkeys)
        exp = np.zeros_like(mask)
        if rows is not None:
            exp[rows] = True  # the denominator runs over all T keys: a key outside the window still reaches every written column
        assert np.array_equal(mask, exp), name
        _ok(tc.check_footprint(rc.emulate(p, B, T, nh, ac.F16, queries, key0, nkeys), clean, mask, name))


# ------------------------------------------------------------------------------------------------------------------- per-row kernels, head
@pytest.mark.parametrize("rows,H", [(r, H) for H in tc.ROW_H for r in tc.ROW_ROWS])
def test_row_kernel_placements(rows, H):
    x = mc.ln_offset_rows(rows, H, seed=rows + H) / 1e4
    w, b = mc.ln_affine(H, seed=H)
    clean = mc.ln_emulate(x, w, b, 1e-6, mc.F32)
    xt = tc.row_tracers(rows, H)
    p = tc.plant(x, xt)
    mask = tc.ln_footprint(p, w, b, 1e-6)
    exp = np.zeros((rows, H), bool)
    exp[[r for r, _ in xt]] = True
    assert np.array_equal(mask, exp) and (tc.informative(mask) or rows == len(xt))
    _ok(tc.check_footprint(mc.ln_emulate(p, w, b, 1e-6, mc.F32), clean, mask, "x"))
    for c in tc.col_tracers(H):
        for vec in ("w", "b"):
            mask = tc.ln_footprint(x, tc.plant(w, [(c,)]) if vec == "w" else w, tc.plant(b, [(c,)]) if vec == "b" else b, 1e-6)
            exp[:] = False
            exp[:, c] = True
            assert np.array_equal(mask, exp)
    # the gathers of layer_tap and dense_pack move rows: the footprint of x[b, t, c] is the image of row t in the destination
    B, R, h0, w0 = 2, 4, 3, 5
    xs = lyc.tap_stream(None, B, 1 + R + h0 * w0, H, seed=H)
    for t in (0, 2, 1 + R, R + h0 * w0):
        for layout in (lyc.TOKENS, lyc.CHW):
            g = lyc.gather(tc.plant(xs, [(1, t, 7)]), R, h0, w0, layout)
            n = {k: int(np.isnan(v).sum()) for k, v in g.items()}
            assert n == {"cls": int(t == 0), "reg": int(1 <= t <= R), "patch": int(t > R)}, (t, layout, n)


HEAD_CATCHES = {"pool_starts_late": "the first pooled row", "pool_includes_registers": "a register row"}


@pytest.mark.parametrize("pool_regs", [False, True])
def test_head_placements_and_pool_mutants(pool_regs):
    B, R, H, P = 3, 4, 128, 16
    T = 1 + R + P
    first = 1 if pool_regs else 1 + R
    inv = 1.0 / (T - first)
    fin = mc.head_dyadic_case(B, T, H, 3, R, mc.F16, seed=1)[0]
    clean = mc.head_pool_emulate(fin, first, inv, mc.F16)
    names = {0: "cls", 1 + R // 2: "a register row", first - 1: "the row before first", first: "the first pooled row", T - 1: "the last pooled row"}
    caught = {m: [] for m in HEAD_CATCHES}
    for t in tc.head_rows(T, R, first):
        p = tc.plant(fin, [(1, t, 9)])
        mask = tc.head_feat_footprint(p, first, inv)
        exp = np.zeros((B, 2 * H), bool)
        if t == 0:
            exp[1, 9] = True
        if t >= first:
            exp[1, H + 9] = True
        # (a register row or the row before `first` that the definition does not pool has the EMPTY footprint: it must not be read)
        assert np.array_equal(mask, exp) and (tc.informative(mask) or not (t == 0 or t >= first)), names[t]
        _ok(tc.check_footprint(mc.head_pool_emulate(p, first, inv, mc.F16), clean, mask, names[t]))
        for m in HEAD_CATCHES:
            if not tc.check_footprint(mc.head_pool_emulate(p, first, inv, mc.F16, mutant=m), mc.head_pool_emulate(fin, first, inv, mc.F16, mutant=m),
                                      mask, names[t])[0]:
                caught[m].append(names[t])
    assert HEAD_CATCHES["pool_starts_late"] in caught["pool_starts_late"], caught
    if not pool_regs:  # (with the registers pooled by definition the mutant is the definition)
        assert HEAD_CATCHES["pool_includes_registers"] in caught["pool_includes_registers"], caught


def test_im2col_and_patch_token_closed_forms():
    """The closed forms against the reshape restatement of tests/test_gpu_ops.py::test_im2col_bit_exact."""
    for B, Hh, Ww, ps in ((2, 70, 98, 14), (2, 64, 83, 16), (2, 11, 38, 3)):
        h0, w0 = Hh // ps, Ww // ps
        for b, c, y, x in ((0, 0, 0, 0), (1, 2, h0 * ps - 1, w0 * ps - 1), (1, 1, ps, ps - 1), (0, 1, Hh - 1, Ww - 1)):
            rgb = np.zeros((B, 3, Hh, Ww), np.float32)
            rgb[b, c, y, x] = np.nan
            col = rgb[:, :, :h0 * ps, :w0 * ps].reshape(B, 3, h0, ps, w0, ps).transpose(0, 2, 4, 1, 3, 5).reshape(B * h0 * w0, 3 * ps * ps)
            at = tc.im2col_element(b, c, y, x, Hh, Ww, ps)
            assert [tuple(i) for i in np.argwhere(np.isnan(col))] == ([at] if at else [])
            if at:
                assert tc.patch_token(y, x, ps, w0, 4) == 1 + 4 + at[0] - b * h0 * w0


IM2COL_TRACER_CASES = ((2, 70, 98, 14), (2, 64, 83, 16), (2, 11, 38, 3))  # tests/test_gpu_tracers.py::test_im2col


def _im2col_pixels(Hh, Ww, ps):
    """The placements of tests/test_gpu_tracers.py::test_im2col: the joint one, then one pixel in each of its three channels in turn."""
    h0, w0 = Hh // ps, Ww // ps
    joint = [(0, 0, 0, 0), (1, 2, h0 * ps - 1, w0 * ps - 1), (0, 1, ps, ps - 1), (1, 0, ps - 1, ps), (1, 1, Hh - 1, Ww - 1), (0, 2, 2 * ps + 3, Ww - 1)]
    chunk = tc.IM2COL_CHUNK * ps
    if w0 > tc.IM2COL_CHUNK:
        joint += [(0, 0, 1, chunk - 1), (1, 2, 1, chunk), (0, 1, ps + 1, chunk + 1)]
    y, x = ps + 1, min(chunk, (w0 - 1) * ps) + 1
    return [joint] + [[(1, c, y, x)] for c in range(3)]


def test_im2col_restatement_and_the_swapped_divisions():
    """The kernel's index arithmetic restated in numpy equals the reshape definition at every small patch size and at the tracer's cases, with
    no write outside the tile.  With the two divisions by multiplication of the interleaved path exchanged, the tracer's placements fail at
    patch 14 and 16 (and most writes leave the LDS tile, which is why that mutant is tried here and not on a device); at patch 3 the exchange
    is the identity -- both multipliers are 21 846 -- so there is nothing for any test to see."""
    shapes = IM2COL_TRACER_CASES + ((1, 1, 1, 1), (2, 3, 23, 1), (1, 4, 22, 2), (1, 7, 31, 3), (1, 8, 44, 4), (1, 10, 55, 5), (1, 12, 60, 6), (1, 14, 77, 7))
    for B, Hh, Ww, ps in shapes:
        rgb = np.random.default_rng(Hh + Ww).standard_normal((B, 3, Hh, Ww)).astype(np.float32)
        h0, w0 = Hh // ps, Ww // ps
        K = 3 * ps * ps
        ref = np.zeros((B * h0 * w0, (K + 63) // 64 * 64), np.float32)
        ref[:, :K] = rgb[:, :, :h0 * ps, :w0 * ps].reshape(B, 3, h0, ps, w0, ps).transpose(0, 2, 4, 1, 3, 5).reshape(B * h0 * w0, K)
        for layout in (1, 0):
            col, outside = tc.im2col_emulate(rgb, ps, layout)
            assert outside == 0 and np.array_equal(col, ref), (B, Hh, Ww, ps, layout)
    assert 65536 // 3 + 1 == 21846
    for B, Hh, Ww, ps in IM2COL_TRACER_CASES:
        rgb = np.random.default_rng(Hh + Ww).standard_normal((B, 3, Hh, Ww)).astype(np.float32)
        clean = tc.im2col_emulate(rgb, ps, 0)[0]
        caught = []
        for pixels in _im2col_pixels(Hh, Ww, ps):
            mask = np.zeros(clean.shape, bool)
            for px in pixels:
                at = tc.im2col_element(*px, Hh, Ww, ps)
                if at is not None:
                    mask[at] = True
            _ok(tc.check_footprint(tc.im2col_emulate(tc.plant(rgb, pixels), ps, 0)[0], clean, mask, "unmutated"))
            got, outside = tc.im2col_emulate(tc.plant(rgb, pixels), ps, 0, mutant="div3_divps_swapped")
            caught.append(not tc.check_footprint(got, clean, mask, "swapped")[0])
            assert (outside > 0) == (ps != 3)
        assert all(caught) if ps != 3 else not any(caught), (ps, caught)
