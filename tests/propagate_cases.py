"""Cases for dinov2_hip_propagate / dinov2_hip_op_propagate (csrc/propagate.hip), shared by tests/test_propagate_probes.py (CPU: the numpy
restatement of the contract passes them, planted bugs do not) and tests/test_gpu_propagate.py (the kernels and the session calls).

Contract under test (include/dinov2_hip.h): rows to unit length in f16 exactly as dinov2_hip_match does, f32 accumulation of exact products;
query i sits at cell (i / w0, i % w0) and column (f, p) is a candidate iff bit f of `slots` is set and the cells are within `radius`
(Chebyshev; -1: no window); per query the first k candidates in ONE strict total order -- larger f32 value first (-0 read as +0), then the
lowest index f * P + p -- with (-1, -inf) past the candidates; w_j = expf((sim_j - sim_0) / T); out = sum_j w_j L_j / sum_j w_j in f32 with
j ascending; argmax to the lowest channel.

  shapes      Gaussian tokens and labels.  Selection against the float64 cosine S of the un-rounded inputs restricted to the candidates,
              tol = match_cases.tol(H): indices distinct and candidates; |sim_j - S| <= tol; the list sorted exactly by the total order;
              every candidate left out has S <= S[k-th] + 2 tol.  Output against float64 computed from the RETURNED idx and sim, bound below.
  probes      the +-1 rows of match_cases (every similarity exact in f32 in any order, full of ties) on a 10 x 13 grid, two frames, at k in
              {1, 3, 64} and radius in {-1, 0, 2}: idx and the 32-bit patterns of sim against a stable sort over the candidates.
  duplicates  every row of the memory and every query is the same unit vector (16 entries of +-1/4): every window holds only exact copies
              of its query, all weights are 1, the labels are small integers -- idx is the lowest k candidate indices, and out / argmax
              are bit-equal to the f32 mean in index order.  Run on grids and windows chosen to expose one planted bug each.
  scenario    a memory driven through set / propagate(keep) / set(labels=None) / overwrite / drop against the same chain with the labels
              passed through the host.

The output bound.  Let d_j = sim_j - sim_0 (|d_j| <= 2) and a_j = d_j / T.  The f32 subtraction errs by at most 2^-24 |d_j| <= 2^-23, which
the division by T turns into 2^-23 / T; the correctly rounded division adds 2^-24 |a_j| <= 2^-23 / T: the argument of expf is off by at
most 2^-22 / T, so w_j carries a relative error of that size (e^x - 1 ~ x), plus expf's own, taken as 2 ulp = 2^-22 (the device library
documents 1 ulp; numpy's float32 exp is within 1 ulp too).  A weighted mean whose weights each carry a relative error eps moves by at most
2 eps max|L| (numerator and denominator each by eps).  The two f32 sums: k products and k - 1 additions above, k - 1 additions below and one
division, each 2^-24 relative to a partial sum that never exceeds sum w |L|: (k + 2) 2^-24 max|L| covers them to first order.
    bound = (2 (2^-22 / T + 2^-22) + (k + 2) 2^-24) max|L|
The GPU test doubles it for margin; the CPU test shows that a float32 numpy emulation stays inside the undoubled bound on every shape.
"""
import numpy as np

import bank_cases as bc
import match_cases as mc

TM = TN = 128                 # propagate_topk_kernel's tile (match_kernel's)
TARGET_WGS = 256              # BANK_TARGET_WGS
PARTIAL_MAX = 32 << 20        # BANK_PARTIAL_MAX
K_MAX, FRAMES_MAX, GRID_MAX, C_MAX, RADIUS_MAX = 64, 64, 256, 256, 255
EMPTY = bc.EMPTY

# (h0, w0, H, frames, slots, radius, k, C)
SHAPES = [
    (1, 1, 8, 1, 0b1, 0, 1, 1),                       # the smallest
    (5, 7, 8, 2, 0b11, 1, 5, 3),                      # P < 128, non-square
    (12, 12, 72, 3, 0b101, 2, 8, 4),                  # a partial second tile, an unset slot, K padding
    (20, 20, 64, 2, 0b11, 1, 3, 2),                   # four tiles: query tile 0 must skip column tiles 2 and 3
    (20, 20, 64, 2, 0b11, -1, 3, 2),                  # the same grid without a window ...
    (20, 20, 64, 2, 0b11, 255, 3, 2),                 # ... and with one that holds everything
    (9, 15, 64, 1, 0b1, 1, 64, 5),                    # corner-heavy: k = 64 > any window's candidates (4 .. 9): the tail
    (16, 8, 384, 64, 1 << 0 | 1 << 31 | 1 << 63, 3, 20, 2),  # the high slot indices
]
TEMPERATURES = {s: 0.1 for s in SHAPES}
TEMPERATURES[SHAPES[1]] = 1e-3   # cold: exp(sim / T) overflows f32 unless the weights are shifted by sim_0
TEMPERATURES[SHAPES[2]] = 0.07
PROBES = list(mc.PROBES)
PROBE_KS = (1, 3, 64)
PROBE_RADII = (-1, 0, 2)
PROBE_GRID = (10, 13)          # P = 130: two tiles, the second partial
CHUNKINGS = (0, 1, 2, 1 << 20)  # the planner's choice, one item a chunk, two, all items in one chunk

# planted bug -> the named case that must reject it (CASES below)
MUTANTS = {
    "window_lt": "dup 20x20 r1 k64",
    "manhattan": "dup 20x20 r1 k64",
    "xy_swapped": "dup 5x7 r1 k64",
    "query_cell_padded_index": "dup 20x20 r1 k64",
    "unset_slot_counted": "dup 20x20 r1 k64",
    "stale_rows_counted": "scenario",
    "pad_rows_counted": "probe negated H=72 r=-1 k=3",
    "index_without_fp": "dup 20x20 r1 k64",
    "skip_range_short_lo": "dup 20x20 r1 k3",
    "skip_range_short_hi": "dup 20x20 r1 k64",
    "last_chunk_dropped": "dup 20x20 r1 k64",
    "tie_highest": "dup 20x20 r1 k3",
    "kth_slot_lost": "dup 20x20 r1 k3",
    "weights_unshifted": "shape 5x7x8x2x3x1x5x3",
    "t_multiplied": "shape 12x12x72x3x5x2x8x4",
    "empty_slot_weighted": "dup 20x20 r1 k64",
    "denominator_without_w0": "dup 20x20 r1 k3",
    "argmax_tie_highest": "dup 20x20 r1 k3",
    "kept_not_refreshed": "scenario",
}


def shape_id(s):
    return "x".join(str(v) for v in s)


def shape_inputs(shape):
    """(q [P, H], rows [frames, P, H], labels [frames, P, C]): Gaussian tokens; the frames are noisy copies of the queries, so that the
    similarities spread (a video's frames resemble each other); Gaussian labels."""
    h0, w0, H, frames, _, _, _, C = shape
    P = h0 * w0
    q = mc.gaussian_tokens(P, H, 500 + P + H)
    rng = np.random.default_rng(600 + P + H + frames)
    rows = (q[None] + 0.7 * np.abs(q).mean() * rng.standard_normal((frames, P, H))).astype(np.float32)
    labels = rng.standard_normal((frames, P, C)).astype(np.float32)
    return q, rows, labels


# ------------------------------------------------------------------------------------------------------------------- the planner, restated
def tile_range(qt, P, w0, radius):
    """propagate_tile_range of csrc/kernels.h: column tiles [t0, t1) of a slot that query tile qt walks."""
    if radius < 0:
        return 0, -(-P // TN)
    q0, q1 = qt * TM, min(qt * TM + TM - 1, P - 1)
    h0 = P // w0
    y0, y1 = max(q0 // w0 - radius, 0), min(q1 // w0 + radius, h0 - 1)
    return y0 * w0 // TN, ((y1 + 1) * w0 - 1) // TN + 1


def plan(h0, w0, nactive, radius, k, chunk_tiles=0):
    """propagate_plan of csrc/kernels.h: dict of chunk_tiles, nchunks, qtiles, max_items, kept_items, ranges."""
    P = h0 * w0
    ppad = -(-P // TN) * TN
    qtiles = ppad // TM
    ranges = [tile_range(qt, P, w0, radius) for qt in range(qtiles)]
    items = [nactive * (t1 - t0) for t0, t1 in ranges]
    max_items = max(items)
    want = -(-TARGET_WGS // qtiles)
    if chunk_tiles <= 0:
        chunk_tiles = -(-max_items // want)
    per = ppad * k * 8
    max_chunks = PARTIAL_MAX // per
    chunk_tiles = min(max(chunk_tiles, -(-max_items // max_chunks)), max_items)
    return {"chunk_tiles": chunk_tiles, "nchunks": -(-max_items // chunk_tiles), "qtiles": qtiles, "max_items": max_items,
            "kept_items": sum(items), "ranges": ranges}


# ------------------------------------------------------------------------------------------------------------------- candidates, references
def slot_list(slots):
    return [f for f in range(64) if slots >> f & 1]


def window(h0, w0, radius):
    """[P, P] bool: patch p lies within `radius` cells (Chebyshev) of query i."""
    P = h0 * w0
    y, x = np.divmod(np.arange(P), w0)
    if radius < 0:
        return np.ones((P, P), bool)
    return np.maximum(np.abs(y[:, None] - y[None]), np.abs(x[:, None] - x[None])) <= radius


def candidates(h0, w0, frames, slots, radius):
    """[P, frames * P] bool over the index f * P + p."""
    win = window(h0, w0, radius)
    return np.concatenate([win if slots >> f & 1 else np.zeros_like(win) for f in range(frames)], 1)


def output_bound(k, T, lmax):
    return (2 * (2.0 ** -22 / T + 2.0 ** -22) + (k + 2) * 2.0 ** -24) * lmax


def combine64(idx, sim, labels, T):
    """out [P, C] in float64 from a returned list: labels [frames * P, C]."""
    idx, sim = np.asarray(idx), np.asarray(sim, np.float64)
    with np.errstate(invalid="ignore"):
        w = np.where(idx >= 0, np.exp((sim - sim[:, :1]) / T), 0.0)
    L = np.asarray(labels, np.float64)[np.where(idx >= 0, idx, 0)]
    return (w[:, :, None] * L).sum(1) / w.sum(1)[:, None]


def published(q16, rows16, labels, h0, w0, slots, radius, k, T):
    """An independent float64 transcription of the published procedure on the given unit rows: the affinity exp(S / T) of every query with
    every patch of the context frames, masked to the window, the top k per query kept, normalised, labels x affinity."""
    frames, P = rows16.shape[:2]
    ctx = slot_list(slots)
    feats = np.concatenate([rows16[f] for f in ctx]).astype(np.float64)          # [n P, H]
    labs = np.concatenate([labels[f] for f in ctx]).astype(np.float64)           # [n P, C]
    aff = np.exp(feats @ q16.astype(np.float64).T / T)                            # [n P, P]: column i = query i
    mask = np.concatenate([window(h0, w0, radius)] * len(ctx), 1).T             # [n P, P]
    aff = aff * mask
    top = np.argsort(-aff, 0, kind="stable")[:k]                                  # [k, P]
    keep = np.zeros_like(aff, bool)
    np.put_along_axis(keep, top, True, 0)
    aff = np.where(keep, aff, 0.0)
    aff = aff / aff.sum(0, keepdims=True)
    out = labs.T @ aff                                                            # [C, P]
    top_idx = np.array(ctx)[top // P] * P + top % P                               # memory indices f * P + p
    valid = np.take_along_axis(aff, top, 0) > 0
    idx = np.full((P, k), -1, np.int64)
    idx[:, :len(top)] = np.where(valid, top_idx, -1).T
    return out.T, idx


# ------------------------------------------------------------------------------------------------------------------- restatement
class PropModel:
    """numpy restatement of the memory, the selection and the combine with the padding, the per-slot tiles, the skip range, the chunking
    and the merge made explicit.  `mutant`: one of MUTANTS, planted."""

    def __init__(self, H, grid, frames, channels, mutant=None):
        self.H, (self.h0, self.w0), self.frames, self.C, self.mutant = H, grid, frames, channels, mutant
        self.P = self.h0 * self.w0
        self.ppad = -(-self.P // TN) * TN
        self.hpad = -(-H // 64) * 64
        self.rows = np.zeros((frames, self.ppad, self.hpad), np.float32)  # the f16 rows, held as f32; zeroed at create
        self.labels = np.zeros((frames, self.P, channels), np.float32)
        self.kept = None
        self.kept_writes = 0
        self.filled = 0
        self.ever = 0

    def set(self, slot, rows, labels=None):
        if not 0 <= slot < self.frames:
            raise ValueError("slot")
        rows = np.asarray(rows, np.float32)
        if rows.shape != (self.P, self.H):
            raise ValueError("rows")
        if labels is None:
            if self.kept is None:
                raise ValueError("nothing kept")
            labels = self.kept
        if not (self.mutant == "stale_rows_counted" and self.ever >> slot & 1):  # (the planted bug: an overwrite leaves the old rows)
            self.rows[slot, :self.P, :self.H] = mc.normalise_f16(rows).astype(np.float32)
        self.labels[slot] = np.asarray(labels, np.float32)
        self.filled |= 1 << slot
        self.ever |= 1 << slot

    def drop(self, slot):
        if not 0 <= slot < self.frames:
            raise ValueError("slot")
        self.filled &= ~(1 << slot)  # the memory stays

    def _cell(self, i):
        if self.mutant == "xy_swapped":
            return i % self.h0, i // self.h0
        return i // self.w0, i % self.w0

    def propagate(self, q, slots, radius, k, T, keep=False, chunk_tiles=0):
        m = self.mutant
        q = np.asarray(q, np.float32)
        if q.shape != (self.P, self.H) or slots == 0 or slots & ~self.filled or not 1 <= k <= K_MAX:
            raise ValueError("request")
        P, C = self.P, self.C
        active = slot_list(self.ever if m == "stale_rows_counted" else self.filled if m == "unset_slot_counted" else slots)
        pl = plan(self.h0, self.w0, len(active), radius, k, chunk_tiles)
        ct, nchunks = pl["chunk_tiles"], pl["nchunks"]
        Q = np.zeros((self.ppad, self.hpad), np.float32)
        Q[:P, :self.H] = mc.normalise_f16(q).astype(np.float32)
        cy, cx = np.array([self._cell(p) for p in range(self.ppad)]).T  # the cell table (entries >= P are never candidates' cells)
        idx = np.empty((P, k), np.int32)
        sim = np.empty((P, k), np.float32)
        for qt in range(pl["qtiles"]):
            t0, t1 = pl["ranges"][qt]
            if m == "skip_range_short_lo" and t1 - t0 > 1:
                t0 += 1
            if m == "skip_range_short_hi" and t1 - t0 > 1:
                t1 -= 1
            items = [(f, t) for f in active for t in range(t0, t1)]
            S = {it: (Q[qt * TM:(qt + 1) * TM] @ self.rows[it[0], it[1] * TN:(it[1] + 1) * TN].T).astype(np.float32) + np.float32(0.0)
                 for it in items}
            for r in range(min(TM, P - qt * TM)):
                i = qt * TM + r
                qy, qx = (cy[r], cx[r]) if m == "query_cell_padded_index" else (cy[i], cx[i])  # (the bug: the index inside the padded tile)
                pv, pi = [], []
                for c in range(nchunks):  # one sorted list per chunk of items
                    cv, ci = [np.empty(0, np.float32)], [np.empty(0, np.int32)]
                    for f, t in items[c * ct:(c + 1) * ct]:
                        p = np.arange(t * TN, (t + 1) * TN)
                        ok = p < (self.ppad if m == "pad_rows_counted" else P)
                        dy, dx = np.abs(cy[p] - qy), np.abs(cx[p] - qx)
                        if radius >= 0:
                            d = dy + dx if m == "manhattan" else np.maximum(dy, dx)
                            ok &= d < radius if m == "window_lt" else d <= radius
                        cv.append(S[(f, t)][r][ok])
                        ci.append(((0 if m == "index_without_fp" else f * P) + p[ok]).astype(np.int32))
                    v, ii = bc._first_k(np.concatenate(cv), np.concatenate(ci), k, m if m in ("tie_highest", "kth_slot_lost") else None)
                    pv.append(v)
                    pi.append(ii)
                if m == "last_chunk_dropped" and nchunks > 1:
                    last = max(c for c in range(nchunks) if items[c * ct:(c + 1) * ct])
                    pv, pi = pv[:last] + pv[last + 1:], pi[:last] + pi[last + 1:]
                v, ii = bc._first_k(np.concatenate(pv), np.concatenate(pi), k, "tie_highest" if m == "tie_highest" else None)  # the merge
                empty = ii == EMPTY
                ii[empty], v[empty] = -1, -np.inf
                idx[i], sim[i] = ii, v
        out, amax = self.combine(idx, sim, T)
        if keep and not (m == "kept_not_refreshed" and self.kept_writes > 0):
            self.kept = out.copy()
            self.kept_writes += 1
        return {"labels": out, "argmax": amax, "idx": idx, "sim": sim}

    def combine(self, idx, sim, T):
        """Contract 5 and 6 in float32: the weights once, both sums with j ascending, products rounded before they are added."""
        m = self.mutant
        T = np.float32(T)
        k = idx.shape[1]
        L = self.labels.reshape(-1, self.C)
        with np.errstate(over="ignore", invalid="ignore"):
            arg = sim if m == "weights_unshifted" else sim - sim[:, :1]
            arg = (arg * T if m == "t_multiplied" else arg / T).astype(np.float32)
            w = np.where(idx >= 0, np.exp(arg, dtype=np.float32), np.float32(1.0 if m == "empty_slot_weighted" else 0.0)).astype(np.float32)
            num = np.zeros((len(idx), self.C), np.float32)
            den = np.zeros(len(idx), np.float32)
            for j in range(k):
                num = num + (w[:, j, None] * L[idx[:, j]]).astype(np.float32)  # (idx -1 reads the last row: weight 0 unless the bug is planted)
                if not (m == "denominator_without_w0" and j == 0):
                    den = den + w[:, j]
            out = (num / den[:, None]).astype(np.float32)
        if m == "argmax_tie_highest":
            amax = (self.C - 1 - np.argmax(out[:, ::-1], 1)).astype(np.int32)
        else:
            amax = np.argmax(out, 1).astype(np.int32)  # the FIRST maximum
        return out, amax


def emulate(q, rows, labels, grid, slots, radius, k, T, chunk_tiles=0, mutant=None):
    """The op's shape: every slot written, `slots` the context.  Returns labels, argmax, idx, sim and kept."""
    frames = len(rows)
    model = PropModel(q.shape[1], grid, frames, labels.shape[2], mutant)
    for f in range(frames):
        model.set(f, rows[f], labels[f])
    res = model.propagate(q, slots, radius, k, T, keep=True, chunk_tiles=chunk_tiles)
    res["kept"] = model.kept
    return res


# ------------------------------------------------------------------------------------------------------------------- checks
def check_selection(res, S, cand, H, k, what, report=None):
    """The four per-row checks of the module docstring, restricted to the candidates.  S [P, frames * P] float64, cand the same shape."""
    P = len(S)
    idx, sim = np.asarray(res["idx"]), np.asarray(res["sim"])
    if idx.shape != (P, k) or sim.shape != (P, k):
        return False, f"{what}: shapes {idx.shape} {sim.shape}, expected {(P, k)}"
    t = mc.tol(H)
    worst_err = worst_over = 0.0
    for i in range(P):
        real = min(k, int(cand[i].sum()))
        if not ((idx[i, real:] == -1).all() and np.isneginf(sim[i, real:]).all()):
            return False, f"{what}: row {i}: slots {real} .. {k - 1} of {int(cand[i].sum())} candidates must hold (-1, -inf)"
        ii, vv = idx[i, :real], sim[i, :real]
        if ii.min() < 0 or ii.max() >= S.shape[1] or not cand[i, ii].all():
            return False, f"{what}: row {i} returns an index that is no candidate: {ii.tolist()}"
        if len(set(ii.tolist())) != real:
            return False, f"{what}: row {i} returns an index twice"
        err = np.abs(vv.astype(np.float64) - S[i, ii]).max()
        worst_err = max(worst_err, err)
        if not err <= t:
            return False, f"{what}: row {i}: |sim - S| = {err:.3e} > tol {t:.3e}"
        if not ((vv[:-1] > vv[1:]) | ((vv[:-1] == vv[1:]) & (ii[:-1] < ii[1:]))).all():
            return False, f"{what}: row {i}: the list is out of order"
        left = cand[i].copy()
        left[ii] = False
        if left.any():
            over = S[i, left].max() - S[i, ii[-1]]
            worst_over = max(worst_over, over)
            if over > 2 * t:
                return False, f"{what}: row {i}: a candidate left out is over the k-th by {over:.3e} > 2 tol"
    if report is not None:
        report.append(f"{what}: max |sim - S| {worst_err:.3e} (tol {t:.3e}), best excluded over the k-th {worst_over:.3e} (2 tol {2 * t:.3e})")
    return True, ""


def check_output(res, labels, k, T, what, margin=1.0, report=None):
    """out against float64 from the returned idx and sim, within margin x output_bound; argmax = the first maximum of the returned out;
    kept (when returned) = out bit for bit."""
    L = np.asarray(labels).reshape(-1, np.asarray(labels).shape[-1])
    out = np.asarray(res["labels"])
    if out.shape != (len(res["idx"]), L.shape[1]) or not np.isfinite(out).all():
        return False, f"{what}: out has shape {out.shape} or is not finite"
    ref = combine64(res["idx"], res["sim"], L, T)
    bound = margin * output_bound(k, T, np.abs(L).max())
    err = np.abs(out.astype(np.float64) - ref).max()
    if report is not None:
        report.append(f"{what}: max |out - float64| {err:.3e} (bound {bound:.3e})")
    if not err <= bound:
        return False, f"{what}: |out - float64| = {err:.3e} > bound {bound:.3e}"
    if not np.array_equal(res["argmax"], np.argmax(out, 1)):
        return False, f"{what}: argmax is not the first maximum of out"
    if res.get("kept") is not None and not np.array_equal(np.asarray(res["kept"]).view(np.uint32), out.view(np.uint32)):
        return False, f"{what}: the kept copy differs from out"
    return True, ""


def check_exact(res, exp, what, keys=("idx", "sim")):
    """The named arrays bit for bit (floats as their 32-bit patterns)."""
    for key in keys:
        g, e = np.asarray(res[key]), np.asarray(exp[key])
        if g.shape != e.shape:
            return False, f"{what}: {key} has shape {g.shape}, expected {e.shape}"
        if g.dtype.kind == "f" or e.dtype.kind == "f":
            g, e = g.astype(np.float32).view(np.uint32), e.astype(np.float32).view(np.uint32)
        if not np.array_equal(g, e):
            i = tuple(int(v) for v in np.argwhere(g != e)[0])
            return False, f"{what}: {key}{list(i)} = {np.asarray(res[key])[i]!r}, expected {np.asarray(exp[key])[i]!r} ({int((g != e).sum())} of {g.size} differ)"
    return True, ""


def expected_list(S32, cand, k):
    """Stable sort of -S over the candidates (ties to the lowest index), the first k, the (-1, -inf) tail."""
    P = len(S32)
    idx = np.full((P, k), -1, np.int32)
    sim = np.full((P, k), -np.inf, np.float32)
    for i in range(P):
        c = np.flatnonzero(cand[i])
        order = c[np.argsort(-S32[i, c], kind="stable")][:k]
        idx[i, :len(order)], sim[i, :len(order)] = order, S32[i, order]
    return {"idx": idx, "sim": sim}


# ------------------------------------------------------------------------------------------------------------------- probes
def probe_case(kind, H, radius, k):
    """(q, rows, labels, grid, slots, expected) of an exact probe: match_cases' rows on PROBE_GRID, two frames."""
    a, b, _ = mc.build_probe(kind, H)
    h0, w0 = PROBE_GRID
    P = h0 * w0
    q, rows = a[:P], np.stack([b[:P], b[len(b) - P:]])
    S = mc.reference(q, rows.reshape(2 * P, H))
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S), "probe similarities are not exact in f32"
    labels = np.zeros((2, P, 1), np.float32)
    return q, rows, labels, PROBE_GRID, 0b11, expected_list(S32 + np.float32(0.0), candidates(h0, w0, 2, 0b11, radius), k)


def duplicates_case(grid, frames, slots, radius, k, H=64, C=4):
    """(q, rows, labels, expected): every row is one unit vector, so every similarity is exactly 1 and every weight exactly 1.  Labels are
    small integers; channels 1 and 2 are equal and the largest, so argmax meets a tie on every row.  `expected`: idx, sim, labels, argmax."""
    h0, w0 = grid
    P = h0 * w0
    v = np.zeros(H, np.float32)
    v[:16] = [1, -1] * 8
    q = np.tile(v, (P, 1))
    rows = np.tile(v, (frames, P, 1))
    rng = np.random.default_rng(P + frames + k)
    labels = rng.integers(0, 8, (frames, P, C)).astype(np.float32)
    labels[:, :, 1] += 8
    labels[:, :, 2] = labels[:, :, 1]
    cand = candidates(h0, w0, frames, slots, radius)
    exp = expected_list(np.ones((P, frames * P), np.float32), cand, k)
    L = labels.reshape(-1, C)
    num = np.zeros((P, C), np.float32)
    den = np.zeros(P, np.float32)
    for j in range(k):
        live = exp["idx"][:, j] >= 0
        num = num + np.where(live[:, None], L[exp["idx"][:, j]], np.float32(0.0))
        den = den + live.astype(np.float32)
    exp["labels"] = (num / den[:, None]).astype(np.float32)
    exp["argmax"] = np.argmax(exp["labels"], 1).astype(np.int32)
    assert (exp["argmax"] == 1).all()
    return q, rows, labels, exp


DUPLICATES = {  # name -> (grid, frames, slots, radius, k)
    "dup 20x20 r1 k64": ((20, 20), 3, 0b110, 1, 64),   # an unset slot below the set ones; k > every window: all candidates, then the tail
    "dup 20x20 r1 k3": ((20, 20), 3, 0b110, 1, 3),
    "dup 5x7 r1 k64": ((5, 7), 1, 0b1, 1, 64),         # non-square
}


# ------------------------------------------------------------------------------------------------------------------- scenario
def scenario_rows(H=32, grid=(6, 8), C=3, seed=21):
    """Three frames of Gaussian tokens on a small grid and the labels of the first."""
    P = grid[0] * grid[1]
    rng = np.random.default_rng(seed)
    base = mc.gaussian_tokens(P, H, seed)
    frames = [(base + 0.5 * np.abs(base).mean() * rng.standard_normal((P, H))).astype(np.float32) for _ in range(3)]
    return frames, rng.standard_normal((P, C)).astype(np.float32)


def scenario_failures(make_memory, frames=None, labels0=None, grid=(6, 8), k=4, T=0.1, radius=2):
    """make_memory(H, grid, frames, channels) -> object with set(slot, rows, labels=None), drop(slot), propagate(q, slots, radius, k, T, keep)
    -> dict.  The realtime chain -- set, propagate with keep, set without labels, propagate -- against the same chain with the labels
    passed through the host on a second memory; then an overwrite and a drop, after which the old rows never appear."""
    failures = []

    def note(ok_msg):
        if not ok_msg[0]:
            failures.append(ok_msg[1])

    if frames is None:
        frames, labels0 = scenario_rows(grid=grid)
    f0, f1, f2 = frames
    P, H = f0.shape
    C = labels0.shape[1]
    keys = ("idx", "sim", "labels", "argmax")
    kept, host = make_memory(H, grid, 3, C), make_memory(H, grid, 3, C)
    kept.set(0, f0, labels0)
    host.set(0, f0, labels0)
    r1 = kept.propagate(f1, 0b1, radius, k, T, keep=True)
    note(check_exact(r1, host.propagate(f1, 0b1, radius, k, T, keep=False), "scenario: frame 1", keys))
    kept.propagate(f2, 0b1, radius, k, T, keep=False)  # a call without keep in between leaves the kept result alone
    r1b = kept.propagate(f1, 0b1, -1, k, T, keep=True)  # ... and a second one with keep replaces it
    kept.set(1, f1, None)
    host.set(1, f1, r1b["labels"])
    r2 = kept.propagate(f2, 0b11, radius, k, T, keep=False)
    note(check_exact(r2, host.propagate(f2, 0b11, radius, k, T, keep=False), "scenario: frame 2 from the kept labels", keys))
    ref = emulate(f2, np.stack([f0, f1]), np.stack([labels0, r1b["labels"]]), grid, 0b11, radius, k, T)
    note(check_exact(r2, ref, "scenario: frame 2 against the restatement's selection", ("idx",)))
    # slot 2 holds copies of the queries (similarity 1); it is then overwritten with frame 0 -- the old rows must be gone
    kept.set(2, f2, labels0)
    if not (kept.propagate(f2, 0b100, 0, 1, T)["idx"][:, 0] == 2 * P + np.arange(P)).all():
        failures.append("scenario: a frame does not find itself at radius 0")
    kept.set(2, f0, labels0)
    fresh = make_memory(H, grid, 3, C)
    fresh.set(2, f0, labels0)
    note(check_exact(kept.propagate(f2, 0b100, radius, k, T), fresh.propagate(f2, 0b100, radius, k, T), "scenario: an overwritten slot", keys))
    # slot 1 is dropped: asking for it is refused, and what is asked for is all that counts
    kept.drop(1)
    try:
        kept.propagate(f2, 0b110, radius, k, T)
        failures.append("scenario: a dropped slot was accepted as context")
    except Exception:  # noqa: BLE001 (the model raises ValueError, the binding DinoError)
        pass
    note(check_exact(kept.propagate(f2, 0b100, radius, k, T), fresh.propagate(f2, 0b100, radius, k, T), "scenario: after a drop", keys))
    return failures


# ------------------------------------------------------------------------------------------------------------------- everything
def case_names():
    names = ["shape " + shape_id(s) for s in SHAPES]
    names += [f"probe {kind} H={H} r={r} k={k}" for kind, H in PROBES for r in PROBE_RADII for k in PROBE_KS]
    return names + list(DUPLICATES) + ["chunking", "scenario"]


def case_failures(name, fn, make_memory=None, margin=1.0, report=None):
    """One named case through fn(q, rows, labels, grid, slots, radius, k, T, chunk_tiles) -> dict (and make_memory for "scenario")."""
    def one(ok_msg):
        return [] if ok_msg[0] else [ok_msg[1]]

    if name.startswith("shape "):
        shape = next(s for s in SHAPES if "shape " + shape_id(s) == name)
        h0, w0, H, frames, slots, radius, k, C = shape
        q, rows, labels = shape_inputs(shape)
        T = TEMPERATURES[shape]
        res = fn(q, rows, labels, (h0, w0), slots, radius, k, T, 0)
        S = shape_reference(shape)
        return (one(check_selection(res, S, candidates(h0, w0, frames, slots, radius), H, k, name, report))
                + one(check_output(res, labels, k, T, name, margin, report)))
    if name.startswith("probe "):
        _, kind, H, r, k = name.split()
        H, r, k = int(H[2:]), int(r[2:]), int(k[2:])
        q, rows, labels, grid, slots, exp = probe_case(kind, H, r, k)
        return one(check_exact(fn(q, rows, labels, grid, slots, r, k, 0.1, 0), exp, name))
    if name in DUPLICATES:
        grid, frames, slots, radius, k = DUPLICATES[name]
        q, rows, labels, exp = duplicates_case(grid, frames, slots, radius, k)
        res = fn(q, rows, labels, grid, slots, radius, k, 0.1, 0)
        return one(check_exact(res, exp, name, ("idx", "sim", "labels", "argmax"))) + one(check_exact(res, {"kept": exp["labels"]}, name, ("kept",)))
    if name == "chunking":
        grid, frames, slots, radius, k = DUPLICATES["dup 20x20 r1 k64"]
        q, rows, labels, exp = duplicates_case(grid, frames, slots, radius, k)
        out = []
        for ct in CHUNKINGS[1:]:
            out += one(check_exact(fn(q, rows, labels, grid, slots, radius, k, 0.1, ct), exp, f"{name} chunk_tiles={ct}", ("idx", "sim", "labels")))
        return out
    if name == "scenario":
        return scenario_failures(make_memory)
    raise ValueError(name)


_SHAPE_REF = {}


def shape_reference(shape):
    """The float64 cosine [P, frames * P] of a shape's inputs, computed once and shared (never modified)."""
    if shape not in _SHAPE_REF:
        q, rows, _ = shape_inputs(shape)
        _SHAPE_REF[shape] = mc.reference(q, rows.reshape(-1, rows.shape[2]))
    return _SHAPE_REF[shape]
