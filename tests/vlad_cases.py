"""Cases for dinov2_hip_vlad_tokens / dinov2_hip_op_vlad* (csrc/vlad.hip), shared by tests/test_vlad_probes.py (CPU: the numpy restatement
of the contract passes them, planted bugs do not) and tests/test_gpu_vlad.py (the kernels).

Contract under test (include/dinov2_hip.h, dinov2_hip_vlad): rows and centre vectors to unit length in f16 by match's normaliser (x^, c^);
label = k-means' assignment; per segment s and centre c the count n_sc and the f32 sum S_sc of the members' x^ in an order the planner fixes
from (len_s, K, H) alone; R_sc = S_sc - n_sc c^_c; INTRA: R_sc / |R_sc|; L2: the segment's K H values over their norm.

Bounds, u = 2^-24, first order, valid for any summation order.
  raw      |R_sc[h] - float64(sum of the device's own x^ over the device's own labels - n c^)| <=
           (n_sc + chunks_s + 2) u (sum_members |x^_ih| + n_sc |c^_ch|).
           A chunk's sum of m exact terms errs by at most (m - 1) u sum|x^|, over all chunks of the segment by less than n_sc u sum|x^|; the
           fold of the chunks_s partials adds at most (chunks_s - 1) u sum|x^|; the product n_sc c^ is rounded once, u n_sc |c^|; the
           difference is rounded once, u |R| <= u (sum|x^| + n_sc |c^|).  Every term is below its share of the bound.
  intra    against the float64 normalisation of the device's own raw R (the same inputs with flags = 0): relative (H / 2 + 4) u per element.
           ss = the f32 sum of H f32 squares: each square u, the sum (H - 1) u: relative H u; the square root halves it and rounds once, the
           division rounds once: (H / 2 + 2) u, and 2 u of room for the second-order terms.
  l2       the same over the K H values of a segment: relative (K H / 2 + 4) u.
  both     the L2 step sees INTRA's values, each off by at most (H / 2 + 4) u relative; so is their norm: 2 (H / 2 + 4) u, and the L2 step's own
           (K H / 2 + 4) u: relative (H + K H / 2 + 12) u.
  norms    the float64 norm of every written row (INTRA), of every segment (L2, both) is 0 or within the mode's bound of 1: elements that are
           all within e relative of a unit vector's have a norm within e of 1.
  probes   rows and centres with exactly 4, 16 or 64 non-zeros of +-1 (kmeans_cases.pm_rows): x^ and c^ are +-2^-1, +-2^-2, +-2^-3, every
           similarity, S, n c^ and R is a short dyadic number, exact in f32 in any order -- labels, counts and raw R bit for bit.
"""
import numpy as np

import kmeans_cases as kc
import match_cases as mc

U = 2.0 ** -24
INTRA, L2 = 1, 2
SEG_MAX, N_MAX, OUT_MAX, PARTIAL_MAX = 4096, 1 << 20, 1 << 28, 32 << 20

SEG_LENS = [1, 63, 64, 65, 127, 128, 129, 257]
KH = [(1, 8), (2, 8), (128, 72), (129, 384), (300, 1536)]
CHUNK_EDGE = ((2, 8), 256, [255, 257])  # (K, H), the planner's chunk for it, two segment lengths at chunk -+ 1
REALISTIC = ([1369, 1369], 32, 1024)
SHAPES = [(SEG_LENS, K, H) for K, H in KH] + [(CHUNK_EDGE[2], *CHUNK_EDGE[0]), REALISTIC]
PROBES = ["lens", "zero_row", "empty_cluster", "k1", "last_partial_chunk", "twin_segments", "two_passes"]
# planted bug -> the case that must reject it
MUTANTS = {
    "neighbour_in_ktile": "probe lens",            # segments packed back to back: a neighbour's rows in a shared K-tile are summed
    "pad_rows_counted": "probe lens",              # padding rows take label 0: -c^_0 per padding row
    "counts_over_all_segments": "probe lens",      # n_c of the whole call in every segment
    "residual_from_raw_centre": "probe lens",      # R = S - n c with the caller's vector
    "empty_returns_centre": "probe empty_cluster",  # an empty cluster gives -c^
    "l2_before_intra": "norm both",
    "l2_over_batch": "norm l2",
    "last_chunk_dropped": "probe last_partial_chunk",
    "order_from_offset": "position",               # the summation order depends on the segment's offset mod 64
    "fold_restarts_at_a_pass": "probe two_passes",  # what the pass before left of a segment is dropped
}


def shape_id(s):
    lens, K, H = s
    return "%dseg%d_%dx%d" % (len(lens), sum(lens), K, H)


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------- the planner
def chunk_rows(K, H):
    tiles = -(-H // 128) * -(-K // 128)
    return 64 * min(32, max(4, tiles))


def plan(offsets, K, H):
    """vlad_plan (csrc/kernels.h) restated: the dict of api.op_vlad_plan without `bytes`."""
    kpad, hpad, hpad128 = -(-K // 128) * 128, -(-H // 64) * 64, -(-H // 128) * 128
    chunk = chunk_rows(K, H)
    per_chunk = kpad * hpad128 * 4
    cap = PARTIAL_MAX // per_chunk
    segs, chunks, npad = [], [], 0
    for s in range(len(offsets) - 1):
        ln = int(offsets[s + 1] - offsets[s])
        pad = -(-ln // 128) * 128
        nch = -(-pad // chunk)
        segs.append((npad, ln, len(chunks), nch))
        for j in range(nch):
            r0 = j * chunk
            chunks.append((s, npad + r0, (min(r0 + chunk, pad) - r0) // 64))
        npad += pad
    return {"kpad": kpad, "hpad": hpad, "hpad128": hpad128, "chunk": chunk, "cap": cap, "npad": npad, "ntiles": npad // 128,
            "nchunks": len(chunks), "npass": -(-len(chunks) // cap), "partial_bytes": per_chunk * min(cap, len(chunks)),
            "segs": np.asarray(segs, np.int32).reshape(-1, 4), "chunks": np.asarray(chunks, np.int32).reshape(-1, 3)}


# ------------------------------------------------------------------------------------------------------------------- inputs
def shape_inputs(shape):
    """(rows, offsets, centre vectors): Gaussian tokens with match's two outlier channels; the centres are perturbed rows of any length."""
    lens, K, H = shape
    n = sum(lens)
    x = mc.gaussian_tokens(n, H, 700 + n + H)
    rng = np.random.default_rng(800 + K + H)
    c = ((x[rng.integers(n, size=K)] + 0.5 * rng.standard_normal((K, H))) * rng.uniform(0.5, 3.0, (K, 1))).astype(np.float32)
    return x, offsets_of(lens), c


def build_probe(kind, seed=31):
    """dict of an exact probe: x, offsets, c and what is planted."""
    rng = np.random.default_rng(seed)
    if kind == "lens":  # the eight lengths; more than one centre tile
        K, H = 130, 72
        off = offsets_of(SEG_LENS)
        return {"x": kc.pm_rows(rng, int(off[-1]), H), "off": off, "c": kc.pm_rows(rng, K, H)}
    if kind == "zero_row":  # a zero row is a member of centre 0 (all its similarities tie at 0): it counts, and adds -c^_0
        K, H = 5, 72
        off = offsets_of([3, 130])
        x = kc.pm_rows(rng, int(off[-1]), H)
        x[1] = 0.0
        x[3 + 128] = 0.0
        return {"x": x, "off": off, "c": kc.pm_rows(rng, K, H), "zero": [1, 3 + 128]}
    if kind == "empty_cluster":  # centre 3 is the negation of centre 0, and every row contains centre 0's pattern: no row takes centre 3
        K, H = 4, 72
        off = offsets_of([70, 5])
        x = np.zeros((int(off[-1]), H), np.float32)
        for i in range(len(x)):
            x[i, :4] = 1.0
            x[i, 4 + rng.choice(H - 4, 12, replace=False)] = rng.choice([-1.0, 1.0], 12)
        c = kc.pm_rows(rng, K, H, nnz=(16,))
        c[0], c[3] = 0.0, 0.0
        c[0, :4], c[3, :4] = 1.0, -1.0
        return {"x": x, "off": off, "c": c, "empty": 3}
    if kind == "k1":
        H = 8
        off = offsets_of([2, 129])
        return {"x": kc.pm_rows(rng, int(off[-1]), H), "off": off, "c": kc.pm_rows(rng, 1, H)}
    if kind == "last_partial_chunk":  # (K, H) = (2, 8): chunks of 256 rows; the members of centre 1 are rows 256 .. 259 of segment 1 alone
        K, H = CHUNK_EDGE[0]
        off = offsets_of([5, 260, 7])
        pats = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 0, 0, 1, -1, 0, 0], [1, 0, 1, 0, 0, 0, -1, 1]], np.float32)  # 1 or 1/2 to centre 0
        x = pats[rng.integers(3, size=int(off[-1]))]
        x[5 + 256:5 + 260] = -pats[0]
        c = np.zeros((K, H), np.float32)
        c[0, :4], c[1, :4] = 1.0, -1.0
        return {"x": x, "off": off, "c": c, "last": (1, 1, 4)}  # (segment, centre, its count)
    if kind == "twin_segments":  # segment 1 is segment 0 and three more rows: the first 66 labels agree, the descriptors do not
        K, H = 6, 72
        a = kc.pm_rows(rng, 66, H)
        x = np.concatenate([a, a, kc.pm_rows(rng, 3, H)])
        return {"x": x, "off": offsets_of([66, 69]), "c": kc.pm_rows(rng, K, H), "twin": 66}
    if kind == "two_passes":  # (K, H) = (1024, 512): 16 chunks a pass; segment 15 has chunk 15 in the first pass, chunks 16 and 17 in the second
        K, H = 1024, 512
        off = offsets_of([1] * 15 + [4100, 3])
        return {"x": kc.pm_rows(rng, int(off[-1]), H), "off": off, "c": kc.pm_rows(rng, K, H), "spans": 15}
    raise ValueError(kind)


def position_case():
    """A segment of 200 rows alone and at positions 0, 2 and 4 of a five-segment list whose other lengths are no multiples of 64.  Its
    elements are Gaussian times 2^-12 .. 2^0: the f16 values of one column spread over more binades than an f32 sum holds exactly, so the
    bits of a cluster sum depend on the order of its terms (Gaussian tokens alone do not show that: a column's f16 values share a few
    exponents, and their f32 sums are mostly exact)."""
    H, K = 72, 7
    rng = np.random.default_rng(899)
    seg = (mc.gaussian_tokens(200, H, 900, outliers=False) * np.exp2(rng.uniform(-12.0, 0.0, (200, H)))).astype(np.float32)
    other = [mc.gaussian_tokens(m, H, 901 + m) for m in (37, 101, 150, 9)]
    c = mc.gaussian_tokens(K, H, 950)
    lists = {}
    for pos in (0, 2, 4):
        parts = other[:pos] + [seg] + other[pos:]
        lists[pos] = (np.concatenate(parts), offsets_of([len(p) for p in parts]))
    return seg, c, lists


# ------------------------------------------------------------------------------------------------------------------- restatement
def _seq_sum(rows):
    """The f32 sum of rows [m, H] in ascending order, one rounding per addition."""
    return np.cumsum(rows, axis=0, dtype=np.float32)[-1] if len(rows) else np.zeros(rows.shape[1], np.float32)


def _norm_rows(v, axis_all=False):
    """v / sqrt(f32 sum of f32 squares) per row (or over all of v); a zero sum stays zero."""
    v = np.asarray(v, np.float32)
    ss = (v * v).sum(dtype=np.float32) if axis_all else (v * v).sum(-1, dtype=np.float32, keepdims=True)
    nrm = np.sqrt(ss, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ss > 0, v / nrm, v).astype(np.float32)


def emulate_vlad(x, offsets, c, flags, mutant=None):
    """Contracts 1 - 5 with the kernel's layout made explicit; the dict of api.op_vlad."""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    n, H = x.shape
    K = len(c)
    xhat, chat = mc.normalise_f16(x).astype(np.float32), mc.normalise_f16(c).astype(np.float32)
    a = kc.emulate_assign(x, c)
    labels, sim = a["labels"], a["sim"]
    p = plan(offsets, K, H)
    n_seg = len(offsets) - 1
    R = np.zeros((n_seg, K, H), np.float32)
    counts = np.zeros((n_seg, K), np.int32)
    for s in range(n_seg):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        row0, ln, ch0, nch = (int(v) for v in p["segs"][s])
        if mutant == "neighbour_in_ktile":  # the K-tiles of a packed layout start at multiples of 64 of the caller's rows
            lo, hi = lo // 64 * 64, min(-(-hi // 64) * 64, n)
            ln = hi - lo
        xs, ls = xhat[lo:hi], labels[lo:hi]
        shift = int(offsets[s]) % 64 if mutant == "order_from_offset" else 0
        spans = [(int(r0) - row0, int(r0) - row0 + 64 * int(kt)) for _, r0, kt in p["chunks"][ch0:ch0 + nch]]
        if mutant == "neighbour_in_ktile":
            spans = [(0, ln)]
        if mutant == "last_chunk_dropped" and len(spans) > 1:
            spans = spans[:-1]
        if mutant == "fold_restarts_at_a_pass":
            spans = [sp for j, sp in enumerate(spans) if (ch0 + j) // p["cap"] == (ch0 + nch - 1) // p["cap"]]
        for cc in range(K):
            S = None
            cnt = 0
            for r0, r1 in spans:  # chunks ascending, rows ascending within a chunk
                m = np.flatnonzero(ls[r0:min(r1, ln)] == cc) + r0
                cnt += len(m)
                part = _seq_sum(xs[np.roll(m, shift)] if shift else xs[m])
                S = part if S is None else (S + part).astype(np.float32)
            if mutant == "pad_rows_counted" and cc == 0:
                cnt += -(-ln // 128) * 128 - ln
            if mutant == "counts_over_all_segments":
                cnt = int((labels == cc).sum())
            counts[s, cc] = cnt
            cen = c[cc] if mutant == "residual_from_raw_centre" else chat[cc]
            if cnt > 0:
                R[s, cc] = (S - (np.float32(cnt) * cen).astype(np.float32)).astype(np.float32)
            elif mutant == "empty_returns_centre":
                R[s, cc] = -chat[cc]
    V = R
    if mutant == "l2_before_intra" and flags == INTRA | L2:
        V = _norm_rows(np.stack([_norm_rows(V[s], axis_all=True) for s in range(n_seg)]))
    else:
        if flags & INTRA:
            V = _norm_rows(V)
        if flags & L2:
            V = _norm_rows(V, axis_all=True) if mutant == "l2_over_batch" else np.stack([_norm_rows(V[s], axis_all=True) for s in range(n_seg)])
    return {"labels": labels, "sim": sim, "counts": counts, "vlad": V, "xhat": xhat, "chat": chat}


# ------------------------------------------------------------------------------------------------------------------- checks
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exact_expectation(x, offsets, c):
    """Probe rows: labels from the exact similarities (ties to the lowest centre), counts, and R exact in f32, so float64 gives the bits."""
    S = mc.reference(x, c)
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S), "probe similarities are not exact in f32"
    labels = S.argmax(1).astype(np.int32)
    xh, chh = mc.normalise_f16(x).astype(np.float64), mc.normalise_f16(c).astype(np.float64)
    assert np.isin(np.abs(xh), [0.0, 0.5, 0.25, 0.125]).all() and np.isin(np.abs(chh), [0.0, 0.5, 0.25, 0.125]).all()
    n_seg, K = len(offsets) - 1, len(c)
    R = np.zeros((n_seg, K, x.shape[1]))
    counts = np.zeros((n_seg, K), np.int32)
    for s in range(n_seg):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        for cc in range(K):
            m = labels[lo:hi] == cc
            counts[s, cc] = m.sum()
            if m.any():
                R[s, cc] = xh[lo:hi][m].sum(0) - counts[s, cc] * chh[cc]
    assert np.array_equal(R.astype(np.float32).astype(np.float64), R)
    return labels, counts, (R + 0.0).astype(np.float32)


def check_probe(run_fn, kind):
    pr = build_probe(kind)
    x, off, c = pr["x"], pr["off"], pr["c"]
    what = "probe " + kind
    exp_l, exp_n, exp_r = exact_expectation(x, off, c)
    if "zero" in pr:
        assert all(exp_l[i] == 0 for i in pr["zero"])
    if "empty" in pr:
        assert (exp_n[:, pr["empty"]] == 0).all() and (exp_n.sum(1) == np.diff(off)).all()
    if "last" in pr:
        s, cc, cnt = pr["last"]
        p = plan(off, len(c), x.shape[1])
        assert exp_n[s, cc] == cnt and p["segs"][s][3] == 2 and p["chunk"] == CHUNK_EDGE[1] and (exp_n[[0, 2], cc] == 0).all()
        assert np.flatnonzero(exp_l[off[s]:off[s + 1]] == cc).min() >= p["chunk"]  # the members sit in the partial second chunk only
    if "spans" in pr:
        p = plan(off, len(c), x.shape[1])
        _, _, ch0, nch = (int(v) for v in p["segs"][pr["spans"]])
        assert p["npass"] == 2 and ch0 // p["cap"] == 0 and (ch0 + nch - 1) // p["cap"] == 1 and nch == 3
    if "twin" in pr:
        t = pr["twin"]
        assert np.array_equal(exp_l[:t], exp_l[t:2 * t]) and not np.array_equal(exp_n[0], exp_n[1])
    got = run_fn(x, off, c, 0)
    if not np.array_equal(got["labels"], exp_l):
        i = int(np.flatnonzero(np.asarray(got["labels"]) != exp_l)[0])
        return False, f"{what}: label[{i}] = {got['labels'][i]}, expected {exp_l[i]}"
    if not np.array_equal(got["counts"], exp_n):
        s, cc = (int(v[0]) for v in np.nonzero(np.asarray(got["counts"]) != exp_n))
        return False, f"{what}: counts[{s}, {cc}] = {got['counts'][s, cc]}, expected {exp_n[s, cc]}"
    if not np.array_equal(bits(got["vlad"]), bits(exp_r)):
        s, cc = (int(v[0]) for v in np.nonzero((bits(got["vlad"]) != bits(exp_r)).any(2)))
        return False, f"{what}: the raw residual of segment {s}, centre {cc} differs in bits"
    return True, ""


def raw_reference(got, offsets):
    """(float64 R of the device's own x^, c^ and labels; its bound) per (s, c, h)."""
    xh, chh, lab = np.asarray(got["xhat"], np.float64), np.asarray(got["chat"], np.float64), np.asarray(got["labels"])
    n_seg, K, H = np.asarray(got["vlad"]).shape
    p = plan(offsets, K, H)
    ref, bound = np.zeros((n_seg, K, H)), np.zeros((n_seg, K, H))
    cnt = np.zeros((n_seg, K), np.int32)
    for s in range(n_seg):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        for cc in range(K):
            m = lab[lo:hi] == cc
            nn = int(m.sum())
            cnt[s, cc] = nn
            if nn:
                ref[s, cc] = xh[lo:hi][m].sum(0) - nn * chh[cc]
                bound[s, cc] = (nn + int(p["segs"][s][3]) + 2) * U * (np.abs(xh[lo:hi][m]).sum(0) + nn * np.abs(chh[cc]))
    return ref, bound, cnt


def check_raw(got, offsets, what, report=None):
    ref, bound, cnt = raw_reference(got, offsets)
    if not np.array_equal(got["counts"], cnt):
        return False, f"{what}: counts differ from the labels'"
    v = np.asarray(got["vlad"], np.float64)
    err = np.abs(v - ref)
    if not np.isfinite(v).all() or (err > bound).any():
        s, cc, h = (int(i) for i in np.unravel_index(np.argmax(err - bound), err.shape))
        return False, f"{what}: segment {s} centre {cc} column {h}: error {err[s, cc, h]:.3e} > bound {bound[s, cc, h]:.3e} (count {cnt[s, cc]})"
    if report is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            report.append(f"{what}: worst error / bound {float(np.nanmax(np.where(bound > 0, err / bound, 0.0))):.3f}")
    return True, ""


def norm_bound(flags, K, H):
    return {INTRA: (H / 2 + 4) * U, L2: (K * H / 2 + 4) * U, INTRA | L2: (H + K * H / 2 + 12) * U}[flags]


def normalise64(raw, flags):
    v = np.asarray(raw, np.float64).copy()

    def unit(a, axes):
        nrm = np.sqrt((a * a).sum(axes, keepdims=True))
        return a / np.where(nrm > 0, nrm, 1.0)
    if flags & INTRA:
        v = unit(v, (2,))
    if flags & L2:
        v = unit(v, (1, 2))
    return v


def check_norm(got, raw, flags, what, report=None):
    """got: the result with `flags`; raw: the device's own result with flags = 0 from the same inputs."""
    name = {INTRA: "norm intra", L2: "norm l2", INTRA | L2: "norm both"}[flags]
    n_seg, K, H = np.asarray(raw["vlad"]).shape
    e = norm_bound(flags, K, H)
    for k in ("labels", "counts"):
        if not np.array_equal(got[k], raw[k]):
            return False, f"{name} {what}: {k} differ from the raw run's"
    ref, v = normalise64(raw["vlad"], flags), np.asarray(got["vlad"], np.float64)
    err = np.abs(v - ref)
    if not np.isfinite(v).all() or (err > e * np.abs(ref)).any():
        s, cc, h = (int(i) for i in np.unravel_index(np.argmax(err - e * np.abs(ref)), err.shape))
        return False, f"{name} {what}: segment {s} centre {cc} column {h}: {v[s, cc, h]!r} against {ref[s, cc, h]!r}, relative bound {e:.3e}"
    nrm = np.sqrt((v * v).sum(2)) if flags == INTRA else np.sqrt((v * v).sum((1, 2)))
    if not ((nrm == 0) | (np.abs(nrm - 1.0) <= e)).all():
        return False, f"{name} {what}: a norm is neither 0 nor within {e:.3e} of 1: {nrm.reshape(-1)[np.argmax(np.abs(nrm - 1.0) * (nrm != 0))]!r}"
    if report is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            report.append(f"{name} {what}: worst relative error / bound {float(np.nanmax(np.where(ref != 0, err / (e * np.abs(ref)), 0.0))):.3f}")
    return True, ""


def check_position(run_fn):
    """The segment alone and at positions 0, 2, 4 of a list: descriptor, counts and labels bit for bit, in all four flag settings."""
    seg, c, lists = position_case()
    for flags in (0, INTRA, L2, INTRA | L2):
        alone = run_fn(seg, offsets_of([len(seg)]), c, flags)
        for pos, (x, off) in lists.items():
            got = run_fn(x, off, c, flags)
            lo, hi = int(off[pos]), int(off[pos + 1])
            same = (np.array_equal(got["labels"][lo:hi], alone["labels"]) and np.array_equal(got["counts"][pos], alone["counts"][0])
                    and np.array_equal(bits(got["sim"][lo:hi]), bits(alone["sim"])) and np.array_equal(bits(got["vlad"][pos]), bits(alone["vlad"][0])))
            if not same:
                return False, f"position: flags {flags}: the segment at position {pos} differs in bits from the segment alone"
    return True, ""


def all_failures(run_fn, report=None):
    """Every case through run_fn(x, offsets, c, flags) -> the dict of api.op_vlad; the failure messages, each starting with its case's name."""
    failures = []

    def note(ok_msg):
        if not ok_msg[0]:
            failures.append(ok_msg[1])

    for kind in PROBES:
        note(check_probe(run_fn, kind))
    for shape in SHAPES:
        x, off, c = shape_inputs(shape)
        what = shape_id(shape)
        raw = run_fn(x, off, c, 0)
        note(kc.check_assign(raw, x, c, "assign " + what))
        note(check_raw(raw, off, "raw " + what, report))
        for flags in (INTRA, L2, INTRA | L2):
            note(check_norm(run_fn(x, off, c, flags), raw, flags, what, report))
    note(check_position(run_fn))
    return failures
