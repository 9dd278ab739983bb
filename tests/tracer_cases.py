"""NaN tracers: which inputs each output element depends on.

A TRACER is one NaN planted in one element of one input of an operation; its FOOTPRINT is the set of output elements that are NaN afterwards.
The EXPECTED footprint comes from the operation's definition -- np.isnan of a float64 / numpy restatement run on the same poisoned input, or a
closed form ("row r", "column n") -- never from the code under test.  Every tracer test makes a clean and a poisoned launch that differ in
the tracer(s) only and asserts, through check_footprint: the clean launch is finite everywhere; the poisoned launch is NaN exactly on the
expected footprint; every other element has the clean launch's bits.  No tolerance, no measured number.

This module holds the checker, the placements (taken from the code's own numbers: the row-tile heights of the plan string of
dinov2_hip_op_gemm_plan, K steps of 64, attention_cases.KT, list_cases.QB, the 64 lanes x float4 of a LayerNorm row), the footprint
functions, and a small tiled GEMM emulator with planted mutants that finite data cannot show.  Imported by tests/test_tracer_probes.py (CPU:
the placements are informative and every mutant is caught by a named placement) and tests/test_gpu_tracers.py (the HIP kernels).  Plain
module, no fixtures.
"""
import re

import numpy as np

import attention_cases as ac
import misc_cases as mc

F16, BF16 = 0, 1
EPI_PATCH, EPI_QKV, EPI_RESID, EPI_GELU, EPI_SWIGLU, EPI_PLAIN, EPI_RESID_LN, EPI_QKV_LN, EPI_GELU_LN, EPI_SWIGLU_LN = range(10)
KSTEP = 64  # K elements per staged tile of every GEMM kernel (csrc/gemm.hip, gemm2.hip, gemm4.hip)
NAN = np.float32(np.nan)


# ------------------------------------------------------------------------------------------------------------------- the checker
def check_footprint(got, clean, expected_mask, what):
    """(ok, message).  `clean` must be finite everywhere (an unwritten NaN-filled element cannot pose as a footprint), `got` must be NaN
    exactly where `expected_mask` says, and everywhere else carry the bits of `clean`.  The message names the first offending element."""
    got, clean = np.asarray(got, np.float32), np.asarray(clean, np.float32)
    mask = np.asarray(expected_mask, bool)
    if got.shape != clean.shape or got.shape != mask.shape:
        return False, "%s: shapes %r (poisoned) %r (clean) %r (footprint)" % (what, got.shape, clean.shape, mask.shape)
    fin = np.isfinite(clean)
    if not fin.all():
        i = tuple(int(v) for v in np.argwhere(~fin)[0])
        return False, "%s: the clean launch is not finite at %r (%r): %d such elements" % (what, i, float(clean[i]), int((~fin).sum()))
    nan = np.isnan(got)
    extra = nan & ~mask
    if extra.any():
        i = tuple(int(v) for v in np.argwhere(extra)[0])
        return False, "%s: %r is NaN and must not depend on the tracer (%d such elements; footprint has %d)" % (
            what, i, int(extra.sum()), int(mask.sum()))
    missing = mask & ~nan
    if missing.any():
        i = tuple(int(v) for v in np.argwhere(missing)[0])
        return False, "%s: %r is %r and must be NaN: the tracer was not consumed (%d of %d footprint elements)" % (
            what, i, float(got[i]), int(missing.sum()), int(mask.sum()))
    moved = (got.view(np.uint32) != clean.view(np.uint32)) & ~mask
    if moved.any():
        i = tuple(int(v) for v in np.argwhere(moved)[0])
        return False, "%s: %r is outside the footprint and changed: %r, clean %r (%d such elements)" % (
            what, i, float(got[i]), float(clean[i]), int(moved.sum()))
    return True, "%s: %d NaN exactly on the footprint, the rest unchanged" % (what, int(mask.sum()))


def plant(a, where):
    """A copy of `a` with NaN at every index tuple of `where`."""
    a = np.array(a, np.float32, copy=True)
    for idx in where:
        a[idx] = NAN
    return a


def informative(mask, dense=False):
    """A placement is worth a launch when its footprint is non-empty and (but for the deliberate dense sweeps) a strict subset."""
    n = int(np.asarray(mask, bool).sum())
    return n > 0 and (dense or n < np.asarray(mask).size)


# ------------------------------------------------------------------------------------------------------------------- GEMM: placements
def plan_heights(plan):
    """Row-tile heights of a plan string, per ';'-separated leaf: "gemm4_mixed<256+192>;small<64x128,w2x2,st3,ks1>" -> [[256, 192], [64]]."""
    out = []
    for leaf in plan.split(";"):
        m = re.match(r"small<(\d+)x(\d+)", leaf)
        if m:
            out.append([int(m.group(1))])
            continue
        m = re.match(r"gemm\d\w*<(\d+)(?:\+(\d+))?>", leaf)
        assert m, "unknown plan leaf %r" % leaf
        out.append([int(v) for v in m.groups() if v is not None and int(v) > 0])
    return out


def k_choices(K):
    return [0, KSTEP - 1, KSTEP, K - KSTEP, K - 1]


def a_tracers(M, K, heights, leaf_row0=()):
    """[(r, k_r)] of the sparse A tracers, one per row, k_r from {0, 63, 64, K - 64, K - 1} by the row's role: row 0 -> 0 and row M - 1 ->
    K - 1; the first row handed to each later leaf of a split plan -> K - 64; for every tile height h of the plan (counted from row 0 and
    from every leaf's first row) the last row of the first tile -> 63 and the first row of the second -> 64, the first K element of the
    SECOND K step.  A row with two roles keeps the first."""
    ks = k_choices(K)
    tr = {0: ks[0]}
    tr.setdefault(M - 1, ks[4])
    for r0 in leaf_row0:
        if 0 < r0 < M:
            tr.setdefault(int(r0), ks[3])
    for r0 in [0] + [int(r) for r in leaf_row0]:
        for hs in heights:
            for h in hs:
                if r0 + h < M:
                    tr.setdefault(r0 + h - 1, ks[1])
                    tr.setdefault(r0 + h, ks[2])
    return sorted(tr.items())


def swiglu_out_col(N):
    """Output column of weight row n of the interleaved SwiGLU weights_in (32-row blocks x1 | x2), from misc_cases.interleave_rows: row n holds
    source row src[n]; source rows [0, F) are x1 of unit u, [F, 2F) x2 of unit u - F."""
    F = N // 2
    return mc.interleave_rows(np.arange(N), F) % F


def plan_edges(parts):
    """(rows, columns) where a later argument block of a plan begins (api.gemm_plan_parts): the first row handed to a tail leaf or to the
    second height of a two-height kernel, and the first column of a column split."""
    live = [p for p in parts if p["rows"] > 0 and p["cols"] > 0]
    return sorted({int(p["row0"]) for p in live if p["row0"] > 0}), sorted({int(p["col0"]) for p in live if p["col0"] > 0})


def w_cols(epi, N, qcols, col0=()):
    """Weight rows n that carry a sparse tracer: the ends, 255 | 256, the q|k and k|v boundaries, both members of an x1 | x2 pair, and the
    two columns at every column split of the plan."""
    cols = {0, N - 1}
    for c0 in col0:
        cols |= {int(c0) - 1, int(c0)}
    if N > 256:
        cols |= {255, 256}
    if epi in (EPI_QKV, EPI_QKV_LN):
        cols |= {qcols - 1, qcols, 2 * qcols - 1, 2 * qcols}
    if epi in (EPI_SWIGLU, EPI_SWIGLU_LN):
        cols |= {64 + 5, 128 + 32 + 7}  # x1 of unit 37, x2 of unit 71: both members of a pair, in different units so that each shows alone
    return sorted(c for c in cols if 0 <= c < N)


def w_tracers(N, K, cols):
    ks = k_choices(K)
    return [(n, ks[(i + 2) % len(ks)]) for i, n in enumerate(cols)]


def dense_tracers(rows, K, step):
    """Every row one tracer at k = (step * r) mod K: the issue's sweeps use step 7 for A and 5 for W."""
    r = np.arange(rows)
    return r, (step * r) % K


# ------------------------------------------------------------------------------------------------------------------- GEMM: the definition
def gemm_h(A, W):
    """The matmul itself, float64: NaN propagates as in IEEE arithmetic."""
    with np.errstate(invalid="ignore"):
        return np.asarray(A, np.float64) @ np.asarray(W, np.float64).T


def gemm_h_dependence(A, W):
    """The DEPENDENCE of A W^T without its arithmetic: h[r, n] is NaN exactly when row r of A or row n of W holds a NaN (every product with a
    NaN is NaN and every sum with one stays NaN), 1 elsewhere.  tests/test_tracer_probes.py holds this to gemm_h on small shapes; the GPU tests
    use it because float64 matmuls of the coverage shapes would take minutes."""
    ra, rw = np.isnan(np.asarray(A)).any(axis=1), np.isnan(np.asarray(W)).any(axis=1)
    return np.where(ra[:, None] | rw[None, :], NAN, np.float32(1.0))


def ln_coeffs(stats, K, eps):
    """mean and r = 1 / sqrt(var + eps) of each row from its statistics slots (device_types.h ln_row_finish).
    RULE: var = var > 0 ? var : 0 is a select and swallows a NaN variance, so a NaN in a sum-of-squares slot leaves NO footprint (the row
    changes, it does not become NaN); a NaN in a sum slot makes the mean NaN and with it the whole row."""
    S, Q = stats[:, :, 0].astype(np.float64).sum(1), stats[:, :, 1].astype(np.float64).sum(1)
    mean = S / K
    with np.errstate(invalid="ignore"):
        var = Q / K - mean * mean
        var = np.where(var > 0, var, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)


def epilogue(epi, h, bias=None, aux=None, x0=None, P=0, T=0, R=0, qcols=0, qscale=1.0, stats=None, s=None, c=None, gamma=None, eps=1e-6,
             K=0, mutant=None):
    """What each epilogue makes of h = A W^T, restated for its DEPENDENCE (csrc/kernels.h, gemm_epilogue.h).  GELU and SiLU are elementwise,
    finite on finite input and NaN on NaN, so their dependence is that of their argument: they stand as the identity here
    (tests/test_tracer_probes.py checks that against the formulas).  EPI_RESID_LN returns (x, xg, stats)."""
    h = np.asarray(h)
    M, N = h.shape
    col = lambda v: np.asarray(v, h.dtype)[None, :]
    with np.errstate(invalid="ignore"):
        if epi >= EPI_QKV_LN:
            if mutant == "stats_of_neighbour_row":
                stats = np.roll(stats, -1, axis=0)
            mean, r = ln_coeffs(stats, K, eps)
            v = r[:, None] * (h - mean[:, None] * col(s)) + col(c)
        else:
            b = np.roll(bias, -1) if mutant == "bias_of_neighbour_column" else bias
            v = h + col(b)
        if epi in (EPI_QKV, EPI_QKV_LN):
            v = v.copy()
            v[:, :qcols] *= qscale
            return v
        if epi in (EPI_GELU, EPI_GELU_LN, EPI_PLAIN):
            return v
        if epi in (EPI_SWIGLU, EPI_SWIGLU_LN):
            b32 = v.reshape(M, N // 64, 2, 32)  # misc_cases.interleave_rows: alternating 32-column blocks x1 | x2
            x1, x2 = b32[:, :, 0], b32[:, :, 1]
            if mutant == "x1_x2_swapped":  # the pair window starts at the x2 block: x2 of block b with x1 of block b + 1
                x1, x2 = b32[:, :, 1], np.roll(b32[:, :, 0], -1, axis=1)
            return (x1 * x2).reshape(M, N // 2)
        if epi == EPI_RESID:
            return np.asarray(x0, h.dtype) + col(aux) * v
        if epi == EPI_RESID_LN:
            x = np.asarray(x0, h.dtype) + col(aux) * v
            xg = x * col(gamma)
            g = x.reshape(M, N // 64, 64)
            gs = 12 if N // 64 <= 12 else 24
            st = np.zeros((M, gs, 2), h.dtype)
            st[:, :N // 64, 0], st[:, :N // 64, 1] = g.sum(-1), (g * g).sum(-1)
            return x, xg, st
        assert epi == EPI_PATCH
        out = np.array(x0, h.dtype, copy=True).reshape(M // P, T, N)
        out[:, 1 + R:] = v.reshape(M // P, P, N) + np.asarray(aux, h.dtype)[None, 1:]  # row 1 + R + p of every image, + pos[1 + p]
        return out.reshape(-1, N)


def activation(epi, v1, v2=None):
    """The real activation of an epilogue (float64), for the CPU check that the identity above has its dependence."""
    with np.errstate(invalid="ignore", over="ignore"):
        if epi in (EPI_GELU, EPI_GELU_LN):
            return 0.5 * v1 * (1 + np.tanh(0.79788456080286535587989211986876 * v1 * (1 + 0.044715 * v1 * v1)))
        return v1 / (1 + np.exp(-v1)) * v2


# ------------------------------------------------------------------------------------------------------------------- GEMM: emulator + mutants
GEMM_MUTANTS = ("k_tile_skipped", "tail_rows_from_next_matrix", "rows_swapped_in_tile", "x1_x2_swapped", "bias_of_neighbour_column",
                "stats_of_neighbour_row")


def emulate_gemm(epi, A, W, leaves, tn=64, mutant=None, **kw):
    """A tiled GEMM as the kernels walk it: `leaves` = [(row0, rows, tile height)] of one operand buffer A (a split plan hands the rows after a
    leaf to the next one), column tiles of `tn`, K in steps of 64; the rows of a leaf's last tile past its end re-read the leaf's last row
    and are not stored (csrc/gemm.hip clamps out-of-range rows to the last row).  Then `epilogue`.  Mutants, none of which finite data shows
    unless its values happen to matter:
      k_tile_skipped              the second K step of every leaf's second row tile is never accumulated
      tail_rows_from_next_matrix  the rows past a leaf's end are read from what FOLLOWS in the buffer, and their accumulators are multiplied
                                  by 0 into the leaf's last stored row
      rows_swapped_in_tile        the last two rows of every leaf's first tile are stored in each other's place
      x1_x2_swapped / bias_of_neighbour_column / stats_of_neighbour_row   see `epilogue`"""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    N, K = W.shape
    M = sum(rows for _, rows, _ in leaves)
    h = np.full((M, N), np.nan)
    with np.errstate(invalid="ignore"):
        for row0, rows, th in leaves:
            end = row0 + rows
            for ti, r0 in enumerate(range(row0, end, th)):
                want = np.arange(r0, r0 + th)
                live = want < end
                idx = np.minimum(want, end - 1)
                if mutant == "tail_rows_from_next_matrix":
                    idx = np.minimum(want, A.shape[0] - 1)
                for c0 in range(0, N, tn):
                    acc = np.zeros((th, min(tn, N - c0)))
                    for ki, k0 in enumerate(range(0, K, KSTEP)):
                        if mutant == "k_tile_skipped" and ti == 1 and ki == 1:
                            continue
                        acc += A[idx, k0:k0 + KSTEP] @ W[c0:c0 + tn, k0:k0 + KSTEP].T
                    if mutant == "rows_swapped_in_tile" and ti == 0 and live.sum() >= 2:
                        n = int(live.sum())
                        acc[[n - 2, n - 1]] = acc[[n - 1, n - 2]]
                    if mutant == "tail_rows_from_next_matrix" and not live.all():
                        acc[int(live.sum()) - 1] += 0.0 * acc[~live].sum(0)
                    h[r0:min(r0 + th, end), c0:c0 + tn] = acc[live]
    return epilogue(epi, h, K=K, mutant=mutant, **kw)


# ------------------------------------------------------------------------------------------------------------------- attention
ATTN_T = (1, 64, 65, 129, 261)
ATTN_B, ATTN_NH = 2, 2


def attn_q_rows(T):
    """Queries that carry a tracer: 0, T - 1 and the edges of the 64-, 96- and 128-query blocks of the kernels (attention_cases.QBLOCK)."""
    edges = {q + d for q in set(ac.QBLOCK.values()) for d in (-1, 0)}
    return sorted(i for i in {0, T - 1} | edges if 0 <= i < T)


def attn_keys(T):
    """Keys that carry a tracer: the ends of the first key tile, the first key of the second, and the last key."""
    return sorted(j for j in {0, ac.KT - 1, ac.KT, T - 1} if 0 <= j < T)


def attn_index(kind, b, h, j, T, nh, col):
    """Index into qkv [B * T, 3 * 64 * nh] of element `col` of the q / k / v row j of (image b, head h)."""
    return (b * T + j, {"q": 0, "k": 1, "v": 2}[kind] * 64 * nh + h * 64 + col)


def attn_placements(T, B=ATTN_B, nh=ATTN_NH):
    """[(name, [index tuples])]: all the q tracers of one (image, head) in one launch (their footprints are disjoint rows); one launch per k
    and per v tracer, in both images (key 0 of image 1 is what a tail of image 0 would stage)."""
    out = [("q rows %r of image 0 head 1" % (attn_q_rows(T),), [attn_index("q", 0, 1, i, T, nh, (7 * i + 3) % 64) for i in attn_q_rows(T)])]
    for b in range(B):
        for j in attn_keys(T):
            out.append(("k row %d of image %d head 0" % (j, b), [attn_index("k", b, 0, j, T, nh, (5 * j + 1) % 64)]))
            out.append(("v[%d, %d] of image %d head 1" % (j, (3 * j + 2) % 64, b), [attn_index("v", b, 1, j, T, nh, (3 * j + 2) % 64)]))
    return out


def attn_footprint(qkv, B, T, nh, log2):
    """np.isnan of the float64 attention of the poisoned input (attention_cases.reference)."""
    with np.errstate(invalid="ignore"):
        return np.isnan(ac.reference(qkv, B, T, nh, log2, want_stats=False)[0])


def list_footprint(qkv, T, nh, log2):
    """The same per segment: segment i is attention on its own rows alone (list_cases: the contract of the list kernels)."""
    out, r0 = [], 0
    for t in T:
        out.append(attn_footprint(np.asarray(qkv)[r0:r0 + t], 1, t, nh, log2))
        r0 += t
    return np.concatenate(out)


def list_placements(T, nh):
    """k and v tracers in the first and last row of the first, a middle and the last segment."""
    starts = np.concatenate([[0], np.cumsum(T)[:-1]])
    out = []
    for seg in sorted({0, len(T) // 2, len(T) - 1}):
        for j in sorted({0, T[seg] - 1}):
            row = int(starts[seg]) + j
            out.append(("k row %d of segment %d head 0" % (j, seg), [(row, 64 * nh + (5 * j + 1) % 64)]))
            out.append(("v row %d of segment %d head %d" % (j, seg, nh - 1), [(row, 2 * 64 * nh + (nh - 1) * 64 + (3 * j + 2) % 64)]))
    return out


def attn_rows_footprint(qkv, B, T, nh, queries, key0, nkeys):
    """np.isnan of attn_row_cases.reference on the poisoned input, cut to the requested key window."""
    import attn_row_cases as rc
    with np.errstate(invalid="ignore"):
        return np.isnan(rc.reference(qkv, B, T, nh, queries)[0][..., key0:key0 + nkeys])


# ------------------------------------------------------------------------------------------------------------------- per-row kernels
ROW_H = (128, 384, 1536)
ROW_ROWS = (1, 5, 301)


def row_tracers(rows, H):
    """(r, c) of the x tracers: the first and last row; the rows around a 4-row (one wave each of a 256-thread workgroup) and a 256-row edge;
    columns at the ends of a lane's float4 and of the 64-lane sweep (c = 4 * 64 = 256 starts a lane's second float4)."""
    rs = sorted(r for r in {0, 3, 4, 255, 256, rows - 1} if r < rows)
    cs = [c for c in (0, 3, 4, 255, 256, H - 1) if c < H]
    return [(r, cs[i % len(cs)]) for i, r in enumerate(rs)]


def col_tracers(H):
    return [c for c in (0, 3, 4, 255, 256, H - 1) if c < H]


def ln_footprint(x, w, b, eps):
    with np.errstate(invalid="ignore"):
        return np.isnan(mc.ln_reference(x, w, b, eps))


# ------------------------------------------------------------------------------------------------------------------- head
def head_rows(T, R, first):
    """Tokens of fin that carry a tracer: cls, a register row, the row just before `first`, the first and last pooled rows."""
    rows = {0, first - 1, first, T - 1}
    if R:
        rows.add(1 + R // 2)
    return sorted(rows)


def head_feat_footprint(fin, first, inv_div, mutant=None):
    """np.isnan of feat = [cls ; mean of the tokens from `first` on] (misc_cases.head_pool_emulate: float64 sums)."""
    with np.errstate(invalid="ignore"):
        return np.isnan(mc.head_pool_emulate(fin, first, inv_div, mc.F32, mutant=mutant))


# ------------------------------------------------------------------------------------------------------------------- im2col, end to end
def im2col_element(b, c_rgb, y, x, Hh, Ww, ps):
    """(row, k) of col [B * h0 * w0, Kpad] that pixel (y, x) of RGB channel c of image b lands in; None when the pixel is cropped."""
    h0, w0 = Hh // ps, Ww // ps
    if y >= h0 * ps or x >= w0 * ps:
        return None
    return (b * h0 * w0 + (y // ps) * w0 + x // ps, c_rgb * ps * ps + (y % ps) * ps + x % ps)


IM2COL_CHUNK = 10  # csrc/kernels.h


def im2col_emulate(rgb, ps, layout, mutant=None):
    """im2col_kernel's index arithmetic restated (csrc/kernels_misc.hip), values in float32: per (image, patch row, chunk of ten patches) the
    LDS tile [np][Kpad] is zero in the K padding and filled from contiguous image runs -- planar: element e of the run of (channel c0, row
    ky) goes to patch pl = e / ps (by multiplication, magic = 65536 / ps + 1) at k = c0 ps^2 + ky ps + e % ps; BGR-interleaved: element e of
    the run of row ky is pixel e / 3 (by multiplication with 21 846), channel 2 - e % 3.  Returns (col [B h0 w0, Kpad], the number of writes
    that fell outside the tile: they are dropped here).
    mutant "div3_divps_swapped": the two multipliers of the interleaved path exchanged.  At patch 3 it is NOT a mutant -- 65536 / 3 + 1 is
    21 846, the same number --; at every other patch size the channel term leaves 0 .. 2 and most writes leave the tile."""
    B, _, Hh, Ww = rgb.shape
    img = rgb if layout == 1 else np.ascontiguousarray(rgb[:, ::-1].transpose(0, 2, 3, 1))
    Kreal, pp2 = 3 * ps * ps, ps * ps
    Kpad = (Kreal + 63) // 64 * 64
    h0, w0 = Hh // ps, Ww // ps
    magic, third = 65536 // ps + 1, 21846
    if mutant == "div3_divps_swapped":
        magic, third = third, magic
    col = np.full((B * h0 * w0, Kpad), NAN, np.float32)  # (as the testing op pre-fills it)
    outside = 0
    for b in range(B):
        for py in range(h0):
            for px0 in range(0, w0, IM2COL_CHUNK):
                np_ = min(IM2COL_CHUNK, w0 - px0)
                run = np_ * ps
                tile = np.full(np_ * Kpad, NAN, np.float32)
                tile.reshape(np_, Kpad)[:, Kreal:] = 0.0
                for rr in range(3 * ps if layout == 1 else ps):
                    c0, ky = (rr // ps, rr % ps) if layout == 1 else (0, rr)
                    y = py * ps + ky
                    src = img[b, c0, y, px0 * ps:px0 * ps + run] if layout == 1 else img[b, y, px0 * ps:px0 * ps + run].reshape(-1)
                    e = np.arange(len(src), dtype=np.int64)
                    xo, cc = e, np.zeros_like(e)
                    if layout != 1:
                        xo = (e * third) >> 16
                        cc = (2 - (e - 3 * xo)) * pp2
                    pl = (xo * magic) >> 16
                    at = pl * Kpad + cc + (xo - pl * ps) + c0 * pp2 + ky * ps
                    ok = (at >= 0) & (at < tile.size)
                    outside += int((~ok).sum())
                    tile[at[ok]] = src[ok]
                row0 = b * h0 * w0 + py * w0 + px0
                col[row0:row0 + np_] = tile.reshape(np_, Kpad)
    return col, outside


def patch_token(y, x, ps, w0, R):
    """Token row of the patch that pixel (y, x) of an image belongs to: 1 + R + (y // ps) * w0 + x // ps."""
    return 1 + R + (y // ps) * w0 + x // ps


# ------------------------------------------------------------------------------------------------------------------- GEMM: whole problems
def patch_split(M):
    """P of a patch-embed problem of M rows, as tests/test_gpu_ops.py::test_gemm_plan_coverage_case_bits splits it."""
    return 1369 if M % 1369 == 0 else 256 if M % 256 == 0 else M


def gemm_case(dt, epi, M, N, K, seed=None):
    """Every input of one GEMM launch as a dict of f32 arrays (rows repeat every 128: only their finiteness matters here) plus `kw`, the
    scalar arguments.  Keys: A, W and, by epilogue, bias, aux (LayerScale | pos), x0, gamma, stats, s, c."""
    rng = np.random.default_rng(M + 3 * N + 7 * K + 11 * epi + dt if seed is None else seed)
    tile = lambda a, rows: np.ascontiguousarray(np.tile(a, ((rows + 127) // 128,) + (1,) * (a.ndim - 1))[:rows])
    c = {"A": tile(rng.standard_normal((128, K)).astype(np.float32), M), "W": (rng.standard_normal((N, K)) * 0.05).astype(np.float32)}
    kw = {"qcols": N // 3, "qscale": 0.125}
    if epi >= EPI_QKV_LN:
        xs = (rng.standard_normal((128, K)) * 2 + 0.3).astype(np.float32).reshape(128, K // 64, 64)
        st = np.zeros((128, 12 if K // 64 <= 12 else 24, 2), np.float32)
        st[:, :K // 64, 0], st[:, :K // 64, 1] = xs.sum(-1), (xs * xs).sum(-1)
        c["stats"] = tile(st, M)
        c["s"], c["c"] = (rng.standard_normal(N) * 0.5).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    else:
        c["bias"] = rng.standard_normal(N).astype(np.float32)
    if epi in (EPI_RESID, EPI_RESID_LN):
        c["aux"] = (rng.standard_normal(N) * 0.3 + 1).astype(np.float32)
        c["x0"] = tile((rng.standard_normal((128, N)) * 2 + 0.4).astype(np.float32), M)
    if epi == EPI_RESID_LN:
        c["gamma"] = (rng.standard_normal(N) * 0.3 + 1.5).astype(np.float32)
    if epi == EPI_PATCH:
        P = patch_split(M)
        B, R = M // P, 4
        kw.update(P=P, T=P + 1 + R, R=R)
        c["aux"] = rng.standard_normal((1 + P, N)).astype(np.float32)
        c["x0"] = tile(rng.standard_normal((128, N)).astype(np.float32), B * (P + 1 + R))
    c["kw"] = kw
    return c


def gemm_expected(epi, c, h=None):
    """[footprint of each output] of a (poisoned) problem: np.isnan of `epilogue` over `h`, or, without it, over the dependence of A W^T.
    Then rows that differ in nothing but finite values share one evaluation (every output is row-wise, and the coverage shapes have up to
    87 680 rows): a row with a NaN in one of its own side inputs (x0, stats) is evaluated itself, the others once per class "row of A
    holds a NaN" / "holds none".  tests/test_tracer_probes.py holds this to the evaluation of every row with the real matmul."""
    A = c["A"]
    M, K = A.shape
    side = dict(bias=c.get("bias"), aux=c.get("aux"), s=c.get("s"), c=c.get("c"), gamma=c.get("gamma"), K=K, **c["kw"])
    rows = np.arange(M)
    if h is None and epi != EPI_PATCH:
        special = np.zeros(M, bool)
        for key in ("x0", "stats"):
            if key in c:
                special |= np.isnan(c[key]).reshape(M, -1).any(axis=1)
        ra = np.isnan(A).any(axis=1)
        rows, cls = list(np.flatnonzero(special)), np.zeros(M, np.int64)
        cls[special] = np.arange(len(rows))
        for flag in (False, True):
            members = ~special & (ra == flag)
            if members.any():
                cls[members] = len(rows)
                rows.append(int(np.flatnonzero(members)[0]))
        rows = np.array(rows)
    pick = lambda key: None if key not in c else c[key] if epi == EPI_PATCH else c[key][rows]
    hh = gemm_h_dependence(A[rows], c["W"]) if h is None else h
    out = epilogue(epi, hh, x0=pick("x0"), stats=pick("stats"), **side)
    masks = [np.isnan(o) for o in (out if isinstance(out, tuple) else (out,))]
    return masks if h is not None or epi == EPI_PATCH else [m[cls] for m in masks]


def gemm_sweeps(epi, c, heights, leaf_row0=(), col0=()):
    """[(name, input key, index arrays or tuples, dense)] of the four poisoned launches every coverage case gets."""
    M, K = c["A"].shape
    N = c["W"].shape[0]
    ra, ka = dense_tracers(M, K, 7)
    rw, kw_ = dense_tracers(N, K, 5)
    return [("sparse A %r" % (a_tracers(M, K, heights, leaf_row0),), "A", a_tracers(M, K, heights, leaf_row0), False),
            ("sparse W %r" % (w_tracers(N, K, w_cols(epi, N, c["kw"]["qcols"], col0)),), "W", w_tracers(N, K, w_cols(epi, N, c["kw"]["qcols"], col0)),
             False),
            ("dense A, k = 7 r mod K", "A", [(ra, ka)], True), ("dense W, k = 5 n mod K", "W", [(rw, kw_)], True)]


def gemm_side_tracers(epi, c):
    """[(name, input key, index tuples)]: one tracer in each side input of an epilogue.  A NaN in a sum-of-squares slot is not here: it
    leaves no footprint (ln_coeffs)."""
    M, K = c["A"].shape
    N = c["W"].shape[0]
    n, r = N - 3, M // 2 + 1
    out = []
    if "bias" in c:
        out.append(("bias[%d]" % n, "bias", [(n,)]))
    if epi in (EPI_RESID, EPI_RESID_LN):
        out += [("LayerScale aux[%d]" % 1, "aux", [(1,)]), ("x0[%d, %d]" % (r, 65), "x0", [(r, 65)])]
    if epi == EPI_RESID_LN:
        out.append(("gamma[%d]" % 66, "gamma", [(66,)]))
    if epi == EPI_PATCH:
        p = c["kw"]["P"] - 1
        out.append(("pos[1 + %d, %d]" % (p, 7), "aux", [(1 + p, 7)]))
    if epi >= EPI_QKV_LN:
        g = K // 64 - 1
        out += [("stats[%d, %d, sum]" % (r, g), "stats", [(r, g, 0)]), ("stats[0, 0, sum]", "stats", [(0, 0, 0)]),
                ("s[%d]" % n, "s", [(n,)]), ("c[%d]" % 2, "c", [(2,)])]
    return out


def poisoned(c, key, where):
    d = dict(c)
    d[key] = plant(c[key], where)
    return d
