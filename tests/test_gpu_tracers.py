"""NaN tracers through the HIP kernels: which inputs each output element depends on (tests/tracer_cases.py; the CPU proof that the placements
are worth running: tests/test_tracer_probes.py).

Every test launches twice, clean and with one or a few NaN planted in one input, and asserts through tracer_cases.check_footprint that the
clean launch is finite, that the poisoned launch is NaN exactly on the footprint the operation's DEFINITION gives, and that every other
element kept the clean launch's bits.  There is no tolerance and no measured number in this file.  What that pins, which finite data cannot:
row / column / head / segment / image isolation (no neighbour's row staged and weighted to nothing, no mask by multiplication); "every k
consumed" for every reachable GEMM kernel x epilogue x dtype (a dropped product is a finite element of a dense sweep); and who has to write or
zero which pad: the im2col columns K .. Kpad, the key tail of attention, the statistics slots past hidden / 64.

Covered: the GEMM family (dinov2_hip_op_gemm, _op_gemm_resid_ln, _op_gemm_ln_consumer: every tests/gemm_plan_cases.py case), attention
(attention_ex, attention_list, attn_rows), the per-row kernels (layernorm, ln_prepare, layer_tap, dense_pack), the classifier head, im2col,
convert_weight, and the forward end to end (predict, predict_layers, predict_list, predict_attention, predict_dense, split passes, stale
session state).

LEFT OUT, because they reduce by COMPARISON (argmax, top-k, sort, clamp) and IEEE comparisons drop NaN, so the contract defines no result on
a NaN input: dinov2_hip_op_match / Session.match, bank_topk, dense_reduce (labels / value of predict_dense), the PCA kernels and pca3, and
`topk` of the head.  preprocess_u8 takes 8-bit pixels: it has no NaN to plant.

Control flow: every kernel a tracer goes through here was read for loop bounds, branches and addresses computed from data.  There is one
data-dependent branch, the wave-uniform `if (__any(need))` of the attention kernels' deferred maximum (csrc/attention.hip): it only decides
whether O and l are rescaled, bounds no loop and forms no address, and a lane that does not need the rescale multiplies by exactly 1.  The
maxima of attention, attn_rows and the head's softmax drop a NaN operand (v_max / fmaxf); the exponential that follows restores it.
Only NaN is planted, never Inf.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_cases as ac
import dense_cases as dc
import layer_cases as lyc
import list_cases as lc
import misc_cases as mc
import tracer_cases as tc
from gemm_plan_cases import COVERAGE_CASES, LN_COVERAGE_CASES
from test_gpu_misc_kernels import _convert, _head

pytestmark = pytest.mark.gpu

fp = C.POINTER(C.c_float)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6


def _p(a):
    return a.ctypes.data_as(fp) if a is not None else fp()


def _ok(res):
    assert res[0], res[1]


# ------------------------------------------------------------------------------------------------------------------- GEMM
def _run_gemm(api, dt, epi, c):
    """One launch of problem `c` (tracer_cases.gemm_case) -> the list of its outputs."""
    A, W, kw = c["A"], c["W"], c["kw"]
    M, K = A.shape
    N = W.shape[0]
    lib = api.lib()
    if epi == tc.EPI_RESID_LN:
        x = c["x0"].copy()
        xg = np.full((M, N), np.nan, np.float32)
        st = np.full((M, 12 if N // 64 <= 12 else 24, 2), np.nan, np.float32)
        assert lib.dinov2_hip_op_gemm_resid_ln(dt, _p(A), _p(W), _p(c["bias"]), _p(c["aux"]), _p(c["gamma"]), _p(x), _p(xg), _p(st), M, N, K) == 0
        return [x, xg, st]
    oc = N // 2 if epi in (tc.EPI_SWIGLU, tc.EPI_SWIGLU_LN) else N
    if epi >= tc.EPI_QKV_LN:
        out = np.full((M, oc), np.nan, np.float32)
        assert lib.dinov2_hip_op_gemm_ln_consumer(dt, epi, _p(A), _p(W), _p(c["s"]), _p(c["c"]), _p(c["stats"]), EPS, _p(out), oc, M, N, K,
                                                  kw["qcols"], kw["qscale"]) == 0
        return [out]
    out = c["x0"].copy() if "x0" in c else np.full((M, oc), np.nan, np.float32)
    aux = c.get("aux")
    assert lib.dinov2_hip_op_gemm(dt, epi, _p(A), _p(W), _p(c["bias"]), _p(aux), 0 if aux is None else aux.size, _p(out), out.shape[0], oc, M, N,
                                  K, kw.get("P", 0), kw.get("T", 0), kw.get("R", 0), kw["qcols"], kw["qscale"]) == 0
    return [out]


def _gemm_placement(api, dt, epi, c, clean, name, key, where, what):
    p = tc.poisoned(c, key, where)
    for i, (g, cl, m) in enumerate(zip(_run_gemm(api, dt, epi, p), clean, tc.gemm_expected(epi, p))):
        _ok(tc.check_footprint(g, cl, m, "%s, output %d, %s" % (what, i, name)))


@pytest.mark.parametrize("case", COVERAGE_CASES + LN_COVERAGE_CASES, ids=lambda c: "dt%d-epi%d-%dx%dx%d" % c)
def test_gemm_consumes_every_k_of_its_own_rows_and_columns(api, case):
    """Every reachable kernel x epilogue x dtype (the coverage lists; tests/test_gemm_plans.py holds them to the planner on the CPU, and
    the plan string of each case is parsed here for its tile heights).  Sparse A tracers at the tile and leaf edges of THIS plan: those
    rows, all columns.  Sparse W tracers at the column edges: those columns (SwiGLU: their units), all rows.  Dense sweeps, one NaN in every row of A (k = 7 r mod K) and
    in every row of W (k = 5 n mod K): everything the launch writes must be NaN -- a finite element is a dropped product."""
    dt, epi, M, N, K = case
    plan = api.gemm_plan(dt, epi, M, N, K)
    heights = tc.plan_heights(plan)  # (asserts that every leaf is a kernel it knows the tile heights of)
    assert len(heights) == len(plan.split(";")) and all(h and all(v in (32, 64, 96, 128, 192, 256) for v in h) for h in heights), plan
    row0, col0 = tc.plan_edges(api.gemm_plan_parts(dt, epi, M, N, K))
    c = tc.gemm_case(dt, epi, M, N, K)
    clean = _run_gemm(api, dt, epi, c)
    for name, key, where, _ in tc.gemm_sweeps(epi, c, heights, row0, col0):
        _gemm_placement(api, dt, epi, c, clean, name, key, where, "%r %s" % (case, plan))


def _first_case(epi, dt, min_images=1):
    for c in COVERAGE_CASES + LN_COVERAGE_CASES:
        if c[0] == dt and c[1] == epi and (epi != tc.EPI_PATCH or c[2] // tc.patch_split(c[2]) >= min_images):
            return c
    raise KeyError((epi, dt))


@pytest.mark.parametrize("dt", [tc.F16, tc.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4, 6, 7, 8, 9])
def test_gemm_side_inputs(api, epi, dt):
    """One tracer in each side input of every epilogue: bias[n] and LayerScale aux[n] give column n; x0[r, c] that one element; pos[1 + p, c]
    element c of row 1 + R + p of EVERY image and nothing in rows 0 .. R; gamma[c] gives xg[:, c] only (x and the statistics stay clean);
    the LN consumers' stats[r, slot, sum] gives row r, s[n] and c[n] column n."""
    case = _first_case(epi, dt, min_images=2)
    _, _, M, N, K = case
    c = tc.gemm_case(dt, epi, M, N, K)
    clean = _run_gemm(api, dt, epi, c)
    side = tc.gemm_side_tracers(epi, c)
    assert side
    for name, key, where in side:
        _gemm_placement(api, dt, epi, c, clean, name, key, where, repr(case))
    if epi == tc.EPI_PATCH:
        B, T, R = M // c["kw"]["P"], c["kw"]["T"], c["kw"]["R"]
        p = tc.poisoned(c, "aux", [(1 + 5, 7)])
        got = _run_gemm(api, dt, epi, p)[0].reshape(B, T, N)
        assert B >= 2 and np.isnan(got[:, 1 + R + 5, 7]).all() and int(np.isnan(got).sum()) == B


@pytest.mark.parametrize("dt", [tc.F16, tc.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("epi", [7, 8, 9])
def test_ln_consumer_statistics_slots(api, epi, dt):
    """The two places where the definition says "no NaN" although a NaN went in.
    A sum-of-squares slot: var = var > 0 ? var : 0 (device_types.h ln_row_finish) is a select and swallows a NaN variance: row r changes
    (its variance is taken as 0, so it is scaled by 1 / sqrt(eps) = 1000 and may overflow the 16-bit output type to +-inf) but holds no
    NaN, and no other row moves.
    A slot at or past K / 64: the contract of device_types.h is that those slots are zero and stay zero, and the kernels add them without a
    bound.  The op harness uploads what the test gives it, so a NaN planted there DOES reach row r.  This is why apply_carve must keep
    zeroing those slots once per carve: nothing downstream would stop a stale value."""
    case = _first_case(epi, dt)
    _, _, M, N, K = case
    c = tc.gemm_case(dt, epi, M, N, K)
    clean = _run_gemm(api, dt, epi, c)[0]
    r, gs = M // 2, c["stats"].shape[1]
    p = tc.poisoned(c, "stats", [(r, 1, 1)])
    assert not tc.gemm_expected(epi, p)[0].any()  # (the restatement has the select too: tracer_cases.ln_coeffs)
    got = _run_gemm(api, dt, epi, p)[0]
    assert not np.isnan(got[r]).any() and not np.array_equal(got[r], clean[r])
    rest = np.arange(M) != r
    _ok(tc.check_footprint(got[rest], clean[rest], np.zeros_like(got[rest], bool), "sum-of-squares slot: the other rows"))
    if K // 64 == gs:  # (ViT-g, the only SwiGLU model: 1536 / 64 = 24 slots, no pad)
        assert epi == tc.EPI_SWIGLU_LN
        return
    p = tc.poisoned(c, "stats", [(r, K // 64, 0)])
    mask = np.zeros_like(clean, bool)
    mask[r] = True
    assert np.array_equal(tc.gemm_expected(epi, p)[0], mask)  # (the restatement adds every slot too)
    _ok(tc.check_footprint(_run_gemm(api, dt, epi, p)[0], clean, mask, "pad slot %d" % (K // 64)))


# ------------------------------------------------------------------------------------------------------------------- attention
def _attention(api, dt, qkv, B, T, nh, log2, attn_v):
    out = np.zeros((B * T, nh * 64), np.float32)
    try:
        api.set_tuning("attn_v", attn_v)
        rc = api.lib().dinov2_hip_op_attention_ex(dt, _p(np.ascontiguousarray(qkv, np.float32)), _p(out), B, T, nh * 64, nh, int(log2))
    finally:
        api.reset_tuning("attn_v")
    assert rc != api.OP_GUARD_CHANGED, "attention wrote outside its output rows (guard band changed)"
    assert rc == 0
    return out


@pytest.mark.parametrize("attn_v", [1, 2])
@pytest.mark.parametrize("log2", [True, False], ids=["log2", "exp"])
@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("T", tc.ATTN_T)
def test_attention(api, T, dt, log2, attn_v):
    """q row i: that row of that head.  k row j: every query and column of that (image, head).  v[j, c]: column c of that head for every
    query, also where the probability underflows to 0.  The other head and the other image keep the clean bits: no tail key staged from the
    next image survives as 0 x NaN."""
    B, nh = tc.ATTN_B, tc.ATTN_NH
    qkv = ac.regime_input("random", B, T, nh, dt, log2, seed=T + dt)
    clean = _attention(api, dt, qkv, B, T, nh, log2, attn_v)
    for name, where in tc.attn_placements(T):
        p = tc.plant(qkv, where)
        _ok(tc.check_footprint(_attention(api, dt, p, B, T, nh, log2, attn_v), clean, tc.attn_footprint(p, B, T, nh, log2), name))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["edges", "long_first"])
def test_attention_list(api, name, dt, order):
    """k and v tracers in the first and last row of the first, a middle and the last segment: the footprint stays inside that segment and head."""
    T, nh = lc.SEGMENTS[name], 2
    qkv = lc.segment_input(T, nh, dt, True, seed=17)
    try:
        api.set_tuning("list_order", order)
        clean = api.op_attention_list(dt, qkv, T, nh)
        for pname, where in tc.list_placements(T, nh):
            p = tc.plant(qkv, where)
            _ok(tc.check_footprint(api.op_attention_list(dt, p, T, nh), clean, tc.list_footprint(p, T, nh, True), pname))
    finally:
        api.reset_tuning("list_order")


@pytest.mark.parametrize("lds_budget", [0, 256], ids=["scores_in_lds", "two_pass"])
@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
def test_attn_rows(api, dt, lds_budget):
    """A k tracer inside or outside the written key window reaches every written column of every requested query of its (image, head): the
    denominator runs over all T keys.  A q tracer reaches its own row if that query was requested, and nothing otherwise."""
    B, T, nh, queries, key0, nkeys = 2, 261, 2, [0, 64, 65, 260], 5, 130
    qkv = ac.regime_input("random", B, T, nh, dt, True, seed=29)
    clean = api.op_attn_rows(dt, qkv, B, T, nh, queries, key0, nkeys, lds_budget)
    for name, where in (("k inside the window", [tc.attn_index("k", 1, 0, 64, T, nh, 2)]),
                        ("k outside the window, first key", [tc.attn_index("k", 0, 1, 0, T, nh, 3)]),
                        ("k outside the window, last key", [tc.attn_index("k", 1, 1, 260, T, nh, 63)]),
                        ("q of requested queries", [tc.attn_index("q", 0, 0, 65, T, nh, 5), tc.attn_index("q", 1, 1, 260, T, nh, 0)]),
                        ("q of an unrequested query", [tc.attn_index("q", 0, 1, 63, T, nh, 5)])):
        p = tc.plant(qkv, where)
        mask = tc.attn_rows_footprint(p, B, T, nh, queries, key0, nkeys)
        assert mask.any() == ("unrequested" not in name)
        _ok(tc.check_footprint(api.op_attn_rows(dt, p, B, T, nh, queries, key0, nkeys, lds_budget), clean, mask, name))


# ------------------------------------------------------------------------------------------------------------------- per-row kernels
def _layernorm(api, dt, x, w, b):
    out = np.full(x.shape, np.nan, np.float32)
    assert api.lib().dinov2_hip_op_layernorm(dt, _p(x), _p(w), _p(b), _p(out), x.shape[0], x.shape[1], EPS) == 0
    return out


def _row_case(rows, H):
    x = (mc.ln_offset_rows(rows, H, seed=rows + H) / 1e4).astype(np.float32)
    w, b = mc.ln_affine(H, seed=H)
    return x, w, b


_ROW_SHAPES = [(r, H) for H in tc.ROW_H for r in tc.ROW_ROWS]


@pytest.mark.parametrize("dt", [mc.F32, mc.F16, mc.BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("rows,H", _ROW_SHAPES, ids=["%dx%d" % s for s in _ROW_SHAPES])
def test_layernorm(api, rows, H, dt):
    """x[r, c]: row r.  w[c], b[c]: column c."""
    x, w, b = _row_case(rows, H)
    clean = _layernorm(api, dt, x, w, b)
    p = tc.plant(x, tc.row_tracers(rows, H))
    _ok(tc.check_footprint(_layernorm(api, dt, p, w, b), clean, tc.ln_footprint(p, w, b, EPS), "x %r" % (tc.row_tracers(rows, H),)))
    cols = [(c,) for c in tc.col_tracers(H)]
    _ok(tc.check_footprint(_layernorm(api, dt, x, tc.plant(w, cols), b), clean, tc.ln_footprint(x, tc.plant(w, cols), b, EPS), "w %r" % cols))
    _ok(tc.check_footprint(_layernorm(api, dt, x, w, tc.plant(b, cols)), clean, tc.ln_footprint(x, w, tc.plant(b, cols), EPS), "b %r" % cols))


def _ln_prepare(api, dt, x, gamma):
    rows, H = x.shape
    xg = np.full((rows, H), np.nan, np.float32)
    st = np.full((rows, 12 if H // 64 <= 12 else 24, 2), np.nan, np.float32)
    assert api.lib().dinov2_hip_op_ln_prepare(dt, _p(x), _p(gamma), _p(xg), _p(st), rows, H) == 0
    return [xg, st]


def _ln_prepare_footprint(x, gamma):
    """xg = x gamma, elementwise; stats[r, g] = (sum, sum of squares) of columns 64 g .. 64 g + 63 of row r, zero past H / 64."""
    rows, H = x.shape
    with np.errstate(invalid="ignore"):
        g = x.astype(np.float64).reshape(rows, H // 64, 64)
        st = np.zeros((rows, 12 if H // 64 <= 12 else 24, 2))
        st[:, :H // 64, 0], st[:, :H // 64, 1] = g.sum(-1), (g * g).sum(-1)
        return [np.isnan(x.astype(np.float64) * gamma), np.isnan(st)]


@pytest.mark.parametrize("dt", [mc.F16, mc.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rows,H", _ROW_SHAPES, ids=["%dx%d" % s for s in _ROW_SHAPES])
def test_ln_prepare(api, rows, H, dt):
    """x[r, c]: xg[r, c] and the two statistics of slot c / 64 of row r.  gamma[c]: xg[:, c], and no statistic."""
    x, gamma, _ = _row_case(rows, H)
    clean = _ln_prepare(api, dt, x, gamma)
    for name, xx, gg in (("x", tc.plant(x, tc.row_tracers(rows, H)), gamma), ("gamma", x, tc.plant(gamma, [(c,) for c in tc.col_tracers(H)]))):
        for g, cl, m in zip(_ln_prepare(api, dt, xx, gg), clean, _ln_prepare_footprint(xx, gg)):
            _ok(tc.check_footprint(g, cl, m, name))


def _tap_footprint(x, w, b, norm, R, h0, w0, layout):
    """layer_cases.gather of the (normalised) stream's NaN pattern."""
    B, T, H = x.shape
    nan = tc.ln_footprint(x.reshape(B * T, H), w, b, EPS).reshape(B, T, H) if norm else np.isnan(x)
    return {k: np.isnan(v) for k, v in lyc.gather(np.where(nan, tc.NAN, np.float32(0)), R, h0, w0, layout).items()}


@pytest.mark.parametrize("chw", [False, True], ids=["rows", "chw"])
@pytest.mark.parametrize("norm", [0, 1], ids=["raw", "norm"])
@pytest.mark.parametrize("H", tc.ROW_H)
def test_layer_tap(api, H, norm, chw):
    """x[b, t, c]: the image of row t in the destination it belongs to (cls, registers, patch rows or the CHW permutation) -- one element
    without the norm, the row's H elements with it.  w[c], b[c]: column c of every destination, with the norm only."""
    B, R, h0, w0 = 3, 4, 5, 7
    T = 1 + R + h0 * w0
    x = lyc.tap_stream(None, B, T, H, seed=H)
    w, b = mc.ln_affine(H, seed=H + 1)
    layout = lyc.CHW if chw else lyc.TOKENS
    clean = api.op_layer_tap(x, w, b, EPS, R, h0, w0, norm=norm, chw=chw)
    spots = [(0, 0, 0), (0, 2, 3), (1, R, 4), (1, 1 + R, 255 % H), (2, T - 1, H - 1), (2, 1 + R + w0, 256 % H)]
    cases = [("x[%d, %d, %d]" % s, tc.plant(x, [s]), w, b) for s in spots]
    if norm:
        cases += [("w[%d]" % c, x, tc.plant(w, [(c,)]), b) for c in (0, H - 1)] + [("b[%d]" % c, x, w, tc.plant(b, [(c,)])) for c in (3, 4)]
    for name, xx, ww, bb in cases:
        got, exp = api.op_layer_tap(xx, ww, bb, EPS, R, h0, w0, norm=norm, chw=chw), _tap_footprint(xx, ww, bb, norm, R, h0, w0, layout)
        assert sum(int(m.sum()) for m in exp.values()) == (H if norm and name[0] == "x" else 1 if name[0] == "x" else B * T), name
        for k in ("patch", "cls", "reg"):
            _ok(tc.check_footprint(got[k], clean[k], exp[k], "%s -> %s" % (name, k)))


@pytest.mark.parametrize("slot,nslots", [(0, 1), (1, 2)])
@pytest.mark.parametrize("concat_cls", [False, True], ids=["patch", "patch_cls"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("H", tc.ROW_H)
def test_dense_pack(api, H, norm, concat_cls, slot, nslots):
    """x[b, t, c]: a patch row gives its own row of the operand, the cls row the cls half of EVERY patch row of its image (concat_cls) and
    nothing otherwise, a register row nothing.  Only column block `slot` is written (the rest of the operand stays the harness's NaN fill)."""
    B, R, P = 2, 4, 35
    T = 1 + R + P
    x = lyc.tap_stream(None, B, T, H, seed=H + 3)
    w, b = mc.ln_affine(H, seed=H + 1)
    width = H * (2 if concat_cls else 1)
    block = slice(slot * width, (slot + 1) * width)
    run = lambda xx: api.op_dense_pack(xx, w, b, EPS, R, norm=norm, concat_cls=concat_cls, slot=slot, nslots=nslots)
    whole = run(x)
    clean = whole[:, block]
    assert np.isnan(np.delete(whole, np.arange(block.start, block.stop), axis=1)).all()
    for s in ((0, 0, 5), (1, 2, 5), (0, 1 + R, 0), (1, T - 1, H - 1), (1, 1 + R + 17, 256 % H)):
        xx = tc.plant(x, [s])
        with np.errstate(invalid="ignore"):
            mask = np.isnan(dc.operand(xx[None], w, b, EPS, R, [0], norm, concat_cls).astype(np.float32))
        assert mask.any() == (s[1] > R or (s[1] == 0 and concat_cls)), s
        _ok(tc.check_footprint(run(xx)[:, block], clean, mask, "x[%d, %d, %d]" % s))


# ------------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("dt", [mc.F16, mc.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("const_div", [False, True], ids=["countdiv", "constdiv"])
@pytest.mark.parametrize("pool_regs", [False, True], ids=["skipregs", "poolregs"])
def test_head(api, pool_regs, const_div, dt):
    """fin[b, t, c]: feat[b, c] for the cls row, feat[b, H + c] exactly when the definition pools row t; then every logit and probability of
    image b.  A row the definition does not pool (a register, the row before `first`) leaves nothing.  The other images keep their bits."""
    B, R, H, Cn, Mg = 3, 4, 384, 37, 6
    T = 1 + R + Mg * Mg
    first = 1 if pool_regs else 1 + R
    inv_div = 1.0 / (37 * 37 if const_div else T - first)
    fin, W, bias = mc.head_dyadic_case(B, T, H, Cn, R, dt, seed=3)
    clean = _head(api, dt, fin, W, bias, first, inv_div)
    for t in tc.head_rows(T, R, first):
        p = tc.plant(fin, [(1, t, 70)])
        got = _head(api, dt, p, W, bias, first, inv_div)
        fmask = tc.head_feat_footprint(p, first, inv_div)
        assert int(fmask.sum()) == (t == 0) + (t >= first)
        rows = np.zeros((B, Cn), bool)
        rows[1] = fmask.any()
        for g, cl, m, what in zip(got, clean, (fmask, rows, rows), ("feat", "logits", "probs")):
            _ok(tc.check_footprint(g, cl, m, "fin[1, %d, 70] -> %s" % (t, what)))


# ------------------------------------------------------------------------------------------------------------------- im2col, convert_weight
@pytest.mark.parametrize("dt", [tc.F16, tc.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("layout", [1, 0], ids=["rgb_chw", "bgr_hwc"])
@pytest.mark.parametrize("B,Hh,Ww,ps", [(2, 70, 98, 14), (2, 64, 83, 16), (2, 11, 38, 3)])
def test_im2col(api, dt, layout, B, Hh, Ww, ps):
    """One pixel gives exactly one element of col (none when the patch grid crops it); the pad columns K .. Kpad are written, as zeros.
    Patch 3 (the patch size equals the channel count, 27 of 64 columns are real, 12 patches per grid row): also the pixel columns either side
    of the chunk boundary (patch 9 | 10).  Every case then plants one pixel in each of its three channels IN TURN: which (c, ky, kx) turns NaN
    is the only thing that tells a division by 3 (channels) from a division by the patch size when the two agree on the patch index."""
    rng = np.random.default_rng(Hh + Ww)
    K, Kpad = 3 * ps * ps, (3 * ps * ps + 63) // 64 * 64
    h0, w0 = Hh // ps, Ww // ps
    rgb = (rng.standard_normal((B, 3, Hh, Ww)) * 1.5).astype(np.float32)
    pixels = [(0, 0, 0, 0), (1, 2, h0 * ps - 1, w0 * ps - 1), (0, 1, ps, ps - 1), (1, 0, ps - 1, ps), (1, 1, Hh - 1, Ww - 1), (0, 2, 2 * ps + 3, Ww - 1)]
    chunk = 10 * ps  # IM2COL_CHUNK patches
    if w0 > 10:
        pixels += [(0, 0, 1, chunk - 1), (1, 2, 1, chunk), (0, 1, ps + 1, chunk + 1)]

    def run(a):
        img = a if layout == 1 else np.ascontiguousarray(a[:, ::-1].transpose(0, 2, 3, 1))  # BGR interleaved
        col = np.full((B * h0 * w0, Kpad), np.nan, np.float32)
        assert api.lib().dinov2_hip_op_im2col(dt, _p(img), _p(col), B, Hh, Ww, ps, Kpad, layout) == 0
        return col

    clean = run(rgb)
    assert (Kpad > K) == (ps != 16) and not clean[:, K:].any()  # (patch 16: 768 columns, no pad)
    mask = np.zeros(clean.shape, bool)
    hit = [tc.im2col_element(*px, Hh, Ww, ps) for px in pixels]
    assert (None in hit) == (Ww % ps != 0 or Hh % ps != 0)
    for at in hit:
        if at is not None:
            mask[at] = True
    _ok(tc.check_footprint(run(tc.plant(rgb, pixels)), clean, mask, "pixels %r" % (pixels,)))
    y, x = ps + 1, min(chunk, (w0 - 1) * ps) + 1  # an interior pixel: second patch row, the first patch of the second chunk where there is one
    for c in range(3):
        one = np.zeros(clean.shape, bool)
        one[tc.im2col_element(1, c, y, x, Hh, Ww, ps)] = True
        assert one.sum() == 1 and one[B * h0 * w0 // 2 + w0 + x // ps, c * ps * ps + ps + x % ps]
        _ok(tc.check_footprint(run(tc.plant(rgb, [(1, c, y, x)])), clean, one, "pixel %r" % ((1, c, y, x),)))


@pytest.mark.parametrize("dt", [mc.F16, mc.BF16], ids=["to_f16", "to_bf16"])
@pytest.mark.parametrize("tname", ["f32", "q8_0", "q4_0"])
@pytest.mark.parametrize("N,K,Kpad,F", [(96, 160, 192, 0), (192, 96, 104, 96)])
def test_convert_weight(api, dt, tname, N, K, Kpad, F):
    """One f32 weight (n, k) gives exactly its destination element, interleaved or not; a NaN f16 scale of a q8_0 / q4_0 block exactly that
    block's 32 elements (the oracle's dequantiser on the same bytes is the definition).  The pad columns K .. Kpad stay zero."""
    from oracle import gguf_np as G
    raw, gt, vals = mc.weight_source(tname, N, K, seed=N + K)
    clean = _convert(api, dt, raw, gt, N, K, Kpad, F)
    buf = bytearray(raw)
    if tname == "f32":
        spots = [(0, 0), (N - 1, K - 1), (33, 31), (64 % N, 32)]
        pv = tc.plant(vals, spots)
        buf = bytearray(pv.tobytes())
    else:
        bb = {"q8_0": 34, "q4_0": 18}[tname]
        for blk in (0, K // 32, N * (K // 32) - 1, 40 * (K // 32) + 1):
            buf[blk * bb:blk * bb + 2] = np.array([np.nan], np.float16).tobytes()
        pv = G.dequantize(np.frombuffer(bytes(buf), np.uint8), gt, (N, K))
    mask = np.isnan(mc.convert_expected(pv, dt, Kpad, F))
    assert int(mask.sum()) == (4 if tname == "f32" else 4 * 32) and not mask[:, K:].any()
    _ok(tc.check_footprint(_convert(api, dt, bytes(buf), gt, N, K, Kpad, F), clean, mask, tname))


# ------------------------------------------------------------------------------------------------------------------- end to end
PIXEL = (1, 33, 47)  # channel, y, x of the poisoned pixel


def _setup(api, pkg, golden_dir, tmp_path_factory, name, fold):
    """(model, images): the fixtures at 70 x 98, batch 5; a synthetic ViT-S with 4 registers at 224, batch 24 (the setup of
    tests/test_gpu_ln_fold.py::test_fold_batch_invariance: persistent and column-split GEMM plans)."""
    if name == "small224":
        path = str(tmp_path_factory.mktemp("tracer") / "small.gguf")
        pkg.synth.write_synthetic_gguf(path, "small", registers=4, num_classes=100, seed=3)
        return api.Model(path, classify=True, ln_fold=fold), pkg.synth.synthetic_images(24, 224, 224, seed=5)
    return api.Model(os.path.join(golden_dir, name + ".gguf"), classify=True, ln_fold=fold), pkg.synth.synthetic_images(5, 70, 98, seed=7)


def _positions(B):
    return [0, B // 2, B - 1]


def _image_mask(shape, b):
    m = np.zeros(shape, bool)
    m[b] = True
    return m


SETUPS = [(n, f) for n in ("tiny_gelu_reg4", "tiny_swiglu_reg4", "small224") for f in (-1, 1)]
_setup_ids = ["%s-fold%d" % s for s in SETUPS]


@pytest.mark.parametrize("name,fold", SETUPS, ids=_setup_ids)
def test_predict(api, pkg, golden_dir, tmp_path_factory, name, fold):
    """One NaN pixel in one image (first, middle, last of the batch): that image's cls, patch tokens, logits and probabilities are all NaN;
    every other image has the bits of the clean batch AND of a batch-1 predict of that image."""
    model, imgs = _setup(api, pkg, golden_dir, tmp_path_factory, name, fold)
    sess = api.Session(model)
    B = len(imgs)
    clean = sess.predict(imgs, classify=True)
    alone = [sess.predict(imgs[b:b + 1], classify=True) for b in range(B)]
    for b in _positions(B):
        got = sess.predict(tc.plant(imgs, [(b,) + PIXEL]), classify=True)
        for k in ("cls", "patch_tokens", "logits", "probs"):
            _ok(tc.check_footprint(got[k], clean[k], _image_mask(clean[k].shape, b), "image %d poisoned: %s" % (b, k)))
            for o in range(B):
                if o != b:
                    assert got[k][o].tobytes() == alone[o][k][0].tobytes(), (b, o, k)


@pytest.mark.parametrize("name,fold", SETUPS, ids=_setup_ids)
def test_predict_layers(api, pkg, golden_dir, tmp_path_factory, name, fold):
    """Layers [0, 1, L] without the norm.  Layer 0 (the embeddings) has NaN in exactly the patch row 1 + R + (y / ps) w0 + x / ps of that
    image, its cls and register rows are finite; from layer 1 on the image is NaN throughout.  The other images are clean."""
    model, imgs = _setup(api, pkg, golden_dir, tmp_path_factory, name, fold)
    hp = model.hparams
    L, R, ps = int(hp.num_hidden_layers), int(hp.num_register_tokens), int(hp.patch_size)
    w0 = imgs.shape[3] // ps
    sess = api.Session(model)
    kw = dict(norm=False, return_class_token=True, return_registers=True)
    clean = sess.predict_layers(imgs, [0, 1, L], **kw)
    p_row = tc.patch_token(PIXEL[1], PIXEL[2], ps, w0, R) - 1 - R
    for b in _positions(len(imgs)):
        got = sess.predict_layers(tc.plant(imgs, [(b,) + PIXEL]), [0, 1, L], **kw)
        for i, (g, cl) in enumerate(zip(got["layers"], clean["layers"])):
            for k in ("patch_tokens", "cls", "registers"):
                mask = _image_mask(cl[k].shape, b)
                if i == 0:
                    mask[:] = False
                    if k == "patch_tokens":
                        mask[b, p_row] = True
                _ok(tc.check_footprint(g[k], cl[k], mask, "image %d poisoned: layer %d %s" % (b, g["layer"], k)))


@pytest.mark.parametrize("fold", [-1, 1])
@pytest.mark.parametrize("which", ["mixed", "repeat_apart"])
def test_predict_list(api, golden_dir, which, fold):
    """A list of images of different sizes: the poisoned image is NaN throughout, every other image has the clean list's bits."""
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True, ln_fold=fold)
    sess = api.Session(model)
    images = [lc.image(s, seed=i) for i, s in enumerate(lc.LISTS[which])]
    clean = sess.predict_list(images, classify=True)
    off = clean["offsets"]
    for b in _positions(len(images)):
        bad = [a.copy() for a in images]
        bad[b][1, 5, 9] = np.nan
        got = sess.predict_list(bad, classify=True)
        assert np.array_equal(got["offsets"], off)
        for k in ("cls", "logits", "probs"):
            _ok(tc.check_footprint(got[k], clean[k], _image_mask(clean[k].shape, b), "image %d poisoned: %s" % (b, k)))
        mask = np.zeros(clean["patch_packed"].shape, bool)
        mask[off[b]:off[b + 1]] = True
        _ok(tc.check_footprint(got["patch_packed"], clean["patch_packed"], mask, "image %d poisoned: patch rows" % b))


@pytest.mark.parametrize("name,fold", [s for s in SETUPS if s[0] != "small224"], ids=[i for i in _setup_ids if "small" not in i])
def test_predict_attention_and_dense(api, pkg, golden_dir, tmp_path_factory, name, fold):
    """The softmax rows of predict_attention and the logits of predict_dense: the poisoned image NaN throughout (its one NaN patch row is a key
    of every query of every head from block 1 on), the other images bit-equal.  Labels and values of a NaN image are an argmax over NaN:
    not asserted."""
    model, imgs = _setup(api, pkg, golden_dir, tmp_path_factory, name, fold)
    hp = model.hparams
    L, R = int(hp.num_hidden_layers), int(hp.num_register_tokens)
    sess = api.Session(model)
    queries = [0, 1, 1 + R, R + 35]
    Wd, bd = dc.head_weights(21, 2 * 2 * int(hp.hidden_size), seed=77)
    head = api.DenseHead(model, [1, L], Wd, bd, norm=True, concat_cls=True)
    rows = sess.predict_attention(imgs, [1, L], queries)
    logits = sess.predict_dense(imgs, head, want=("logits",))["logits"]
    for b in _positions(len(imgs)):
        bad = tc.plant(imgs, [(b,) + PIXEL])
        mask = np.zeros(rows.shape, bool)
        mask[:, b] = True
        _ok(tc.check_footprint(sess.predict_attention(bad, [1, L], queries), rows, mask, "image %d poisoned: attention rows" % b))
        _ok(tc.check_footprint(sess.predict_dense(bad, head, want=("logits",))["logits"], logits, _image_mask(logits.shape, b),
                               "image %d poisoned: dense logits" % b))


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")
imgs = pkg.synth.synthetic_images(5, 70, 98, seed=7)
bad = imgs.copy(); bad[2, 1, 33, 47] = np.nan
out = {}
for fold in (-1, 1):
    sess = api.Session(api.Model(sys.argv[2], classify=True, ln_fold=fold))
    for tag, x in (("clean", imgs), ("bad", bad)):
        for k, v in sess.predict(x, classify=True).items():
            out["%s_%d_%s" % (tag, fold, k)] = v
np.savez(sys.argv[3], **out); print("TRACER_OK")
'''


def test_split_passes_in_a_fresh_process(api, golden_dir, tmp_path):
    """DINOV2_HIP_MAX_CHUNK=2 (read once per process, hence a child): a batch of 5 in passes of 2, 2 and 1 images.  The poison sits in
    the middle pass: its pass mate, image 3, and the images of the other passes keep the clean bits."""
    f = str(tmp_path / "split.npz")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), f], cwd=ROOT,
                         env=dict(os.environ, DINOV2_HIP_MAX_CHUNK="2"), capture_output=True, text=True, timeout=600)
    assert "TRACER_OK" in out.stdout, out.stdout + out.stderr
    res = dict(np.load(f))
    for fold in (-1, 1):
        for k in ("cls", "patch_tokens", "logits", "probs"):
            clean, bad = res["clean_%d_%s" % (fold, k)], res["bad_%d_%s" % (fold, k)]
            _ok(tc.check_footprint(bad, clean, _image_mask(clean.shape, 2), "fold %d %s" % (fold, k)))


@pytest.mark.parametrize("fold", [-1, 1])
@pytest.mark.parametrize("call", ["predict", "predict_list", "predict_layers"])
def test_no_stale_nan_in_the_session(api, pkg, golden_dir, call, fold):
    """After a poisoned call a clean call on the SAME session -- at the same shape, a smaller one and a larger one -- has a fresh session's
    bits: nothing the poisoned forward left in the workspace (residual stream, statistics slots, staged tails) is read again."""
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True, ln_fold=fold)
    L = int(model.hparams.num_hidden_layers)

    def run(sess, imgs):
        if call == "predict":
            r = sess.predict(imgs, classify=True)
        elif call == "predict_list":
            r = sess.predict_list(list(imgs) + [imgs[0][:, :56, :70]], classify=True)
            r = {k: r[k] for k in ("cls", "patch_packed", "logits", "probs")}
        else:
            r = sess.predict_layers(imgs, [0, L], norm=True, return_class_token=True, return_registers=True, classify=True)
            for i, d in enumerate(r.pop("layers")):
                r.update({"%d_%s" % (i, k): v for k, v in d.items() if k != "layer"})
        return r

    shapes = {"same": (3, 70, 98), "smaller": (1, 56, 84), "larger": (4, 98, 126)}
    imgs = {k: pkg.synth.synthetic_images(*s, seed=11) for k, s in shapes.items()}
    used = api.Session(model)
    for k in ("same", "smaller", "larger", "same"):
        bad = run(used, tc.plant(imgs["same"], [(1,) + PIXEL]))
        assert np.isnan(bad["cls"][1]).all()
        got, fresh = run(used, imgs[k]), run(api.Session(model), imgs[k])
        for key in fresh:
            assert np.isfinite(fresh[key]).all() and got[key].tobytes() == fresh[key].tobytes(), (k, key)
