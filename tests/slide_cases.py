"""Cases for dinov2_hip_predict_dense_slide / dinov2_hip_op_slide_reduce / dinov2_hip_op_slide_gather (csrc/slide.hip), shared by
tests/test_slide_probes.py (CPU: the numpy restatement through these cases, and the planted bugs they must reject) and tests/test_gpu_slide.py
(the kernels through the same cases).  Plain module, no fixtures.  `mutant`: the name of one planted bug (MUTANTS) or None.

The restatement follows the contract of include/dinov2_hip.h, section "sliding-window dense inference":
  1 windows   per axis n = max(len - crop + stride - 1, 0) // stride + 1, start_i = max(min(i stride + crop, len) - crop, 0)
  3 mean      per pixel and class, over the covering windows in ascending k = iy nx + ix: val^k = dense_cases.interpolate of window k at
              (Y - y1, X - x1); acc starts as the first val and adds the next ones one at a time in float32; mean = acc / float32(n)
  4 reduce    ARGMAX / BINS of dense_cases on the mean
Checked bit for bit; `reference` is the same pipeline in float64 with the same float32 coordinates.
"""
import numpy as np

import dense_cases as dc
from dense_cases import ARGMAX, BINS, U, f32

PATCH = 14
COVER_MAX = 16

MUTANTS = ("divide_by_all_windows",    # mean = acc / (ny nx)
           "no_division",              # the sum instead of the mean
           "last_not_pulled_back",     # window i starts at i stride and is clipped at the image edge
           "starts_swapped",           # the y starts used along x and the x starts along y
           "n_out_image",              # resampled with n_out = the image size instead of the crop
           "dst_not_offset",           # dst = (Y, X) instead of (Y - y1, X - x1)
           "cover_off_by_one",         # a window's last row and column do not count
           "argmax_then_vote",         # argmax per window, then the most frequent label (lowest first)
           "mean_of_argmax_values")    # value = the mean of every window's own maximum
ARGMAX_ONLY_MUTANTS = MUTANTS[7:]

# (h, w, crop_h, crop_w, stride_h, stride_w) at patch 14: one window; four without overlap; pulled-back last windows with starts that are no
# patch multiple and an odd x1 (cover 1 .. 9); a non-square crop at stride 1 (cover up to 4); an output that is no multiple of any tile;
# cover exactly 16 (four by four windows over the pixels 33 .. 41)
CASES = ((42, 42, 42, 42, 28, 28), (84, 84, 42, 42, 42, 42), (70, 91, 42, 42, 20, 20), (43, 57, 42, 56, 14, 1), (100, 61, 28, 42, 19, 42),
         (75, 75, 42, 42, 11, 11))
REFUSED_CASE = (70, 70, 42, 42, 5, 5)  # cover 49
MODEL_CASE = CASES[2]
CLASSES = dc.CLASSES


def case_id(c):
    return "%dx%d-crop%dx%d-stride%dx%d" % c


def starts(length, crop, stride):
    n = max(length - crop + stride - 1, 0) // stride + 1
    return np.array([max(min(i * stride + crop, length) - crop, 0) for i in range(n)], np.int32)


def cover_map(ys, xs, ch, cw, h, w):
    cnt = np.zeros((h, w), np.int64)
    for y1 in ys:
        for x1 in xs:
            cnt[y1:y1 + ch, x1:x1 + cw] += 1
    return cnt


def _interp_at(L, h0, w0, ch, cw, dy, dx, scale_from=None):
    """dense_cases.interpolate for arbitrary destination coordinates dy [n], dx [m] (the mutants' resampling): float32, uncontracted."""
    L = np.asarray(L, f32)

    def ax(n_in, n_out, dst):
        scale = f32(n_in) / f32(n_out)
        src = np.maximum(scale * (dst.astype(f32) + f32(0.5)) - f32(0.5), f32(0))
        i0 = np.minimum(src.astype(np.int32), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), src - i0.astype(f32)

    oh, ow = scale_from or (ch, cw)
    y0, y1, ly = ax(h0, oh, np.asarray(dy))
    x0, x1, lx = ax(w0, ow, np.asarray(dx))
    g = L.reshape(h0, w0, -1)
    a, b = lx[None, :, None], ly[:, None, None]
    t = (f32(1) - a) * g[y0][:, x0] + a * g[y0][:, x1]
    u = (f32(1) - a) * g[y1][:, x0] + a * g[y1][:, x1]
    return (f32(1) - b) * t + b * u


def _reduce(val, reduce, centers, eps):
    """Contracts 4 and 5 of dinov2_hip_predict_dense on val [h, w, C] float32 (the loop of dense_cases.emulate)."""
    C = val.shape[2]
    if reduce == ARGMAX:
        labels = np.argmax(val, axis=2)
        return {"labels": labels.astype(np.uint8), "value": np.ascontiguousarray(np.take_along_axis(val, labels[..., None], 2)[..., 0])}
    cen = np.asarray(centers, f32)
    S = np.zeros(val.shape[:2], f32)
    D = np.zeros(val.shape[:2], f32)
    for c in range(C):
        r = np.maximum(val[..., c], f32(0)) + f32(eps)
        S = S + r
        D = D + r * cen[c]
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"value": D / S}


def mean_logits(Ls, ys, xs, h0, w0, ch, cw, h, w, mutant=None, dtype=f32, parts=False):
    """Contract 3: mean [h, w, C] in `dtype` (float64: the reference; the coordinates stay float32).  parts: also every window's
    (y1, x1, rows, columns, val)."""
    Ls = np.asarray(Ls, f32)
    ys, xs = [int(v) for v in ys], [int(v) for v in xs]
    ny, nx = len(ys), len(xs)
    assert Ls.shape[0] == ny * nx and Ls.shape[1] == h0 * w0
    C = Ls.shape[2]
    if mutant == "starts_swapped":
        ys, xs = xs, ys
    if mutant == "last_not_pulled_back":
        ys = [i * (ys[1] - ys[0]) for i in range(ny)] if ny > 1 else ys
        xs = [i * (xs[1] - xs[0]) for i in range(nx)] if nx > 1 else xs
    acc = np.zeros((h, w, C), dtype)
    cnt = np.zeros((h, w), np.int64)
    wins = []
    for k in range(len(ys) * len(xs)):
        y1, x1 = ys[k // len(xs)], xs[k % len(xs)]
        if mutant == "n_out_image":
            val = _interp_at(Ls[k % (ny * nx)], h0, w0, ch, cw, np.arange(ch), np.arange(cw), scale_from=(h, w))
        elif mutant == "dst_not_offset":
            val = _interp_at(Ls[k % (ny * nx)], h0, w0, ch, cw, y1 + np.arange(ch), x1 + np.arange(cw))
        else:
            val = dc.interpolate(Ls[k % (ny * nx)], h0, w0, ch, cw, dtype=dtype)
        rows = max(0, min(ch - (1 if mutant == "cover_off_by_one" else 0), h - y1))  # (only a mutant's window leaves the image)
        cols = max(0, min(cw - (1 if mutant == "cover_off_by_one" else 0), w - x1))
        if rows == 0 or cols == 0 or y1 >= h or x1 >= w:
            continue
        val = val[:rows, :cols].astype(dtype)
        a, n = acc[y1:y1 + rows, x1:x1 + cols], cnt[y1:y1 + rows, x1:x1 + cols]
        first = (n == 0)[..., None]
        acc[y1:y1 + rows, x1:x1 + cols] = np.where(first, val, a + val)  # starts as the first, then one addition per window, ascending k
        cnt[y1:y1 + rows, x1:x1 + cols] = n + 1
        wins.append((y1, x1, rows, cols, val))
    if mutant == "no_division":
        mean = acc
    else:
        den = np.full((h, w), ny * nx, np.int64) if mutant == "divide_by_all_windows" else cnt
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc / den.astype(dtype)[..., None]
    assert mean.dtype == dtype
    return (mean, cnt, wins) if parts else mean


def emulate(Ls, ys, xs, h0, w0, ch, cw, h, w, reduce=ARGMAX, centers=None, eps=0.0, mutant=None):
    """The restatement of slide_reduce_kernel on Ls [ny nx, h0 w0, C]: {"labels" [h, w] uint8, "value" [h, w] f32} (ARGMAX) or {"value"}."""
    mean, cnt, wins = mean_logits(Ls, ys, xs, h0, w0, ch, cw, h, w, mutant, parts=True)
    out = _reduce(mean, reduce, centers, eps)
    if reduce == ARGMAX and mutant in ARGMAX_ONLY_MUTANTS:
        C = mean.shape[2]
        votes = np.zeros((h, w, C), np.int64)
        vsum = np.zeros((h, w), f32)
        for y1, x1, rows, cols, val in wins:
            lab = np.argmax(val, axis=2)
            np.add.at(votes[y1:y1 + rows, x1:x1 + cols], (np.arange(rows)[:, None], np.arange(cols)[None, :], lab), 1)
            vsum[y1:y1 + rows, x1:x1 + cols] += val.max(axis=2)
        if mutant == "argmax_then_vote":
            out["labels"] = np.argmax(votes, axis=2).astype(np.uint8)
        else:
            out["value"] = vsum / cnt.astype(f32)
    return out


def reference(Ls, ys, xs, h0, w0, ch, cw, h, w, reduce=ARGMAX, centers=None, eps=0.0):
    """float64 of the same pipeline: {"val" [h, w, C] (the mean), "labels", "value", "margin" (top-1 minus top-2, ARGMAX), "n" [h, w]}."""
    mean, cnt, _ = mean_logits(Ls, ys, xs, h0, w0, ch, cw, h, w, dtype=np.float64, parts=True)
    out = {"val": mean, "n": cnt}
    if reduce == ARGMAX:
        out["labels"] = np.argmax(mean, axis=2).astype(np.uint8)
        srt = np.sort(mean, axis=2)
        out["value"] = srt[..., -1]
        out["margin"] = srt[..., -1] - srt[..., -2]
    else:
        r = np.maximum(mean, 0.0) + float(eps)
        out["value"] = (r * np.asarray(centers, np.float64)).sum(2) / r.sum(2)
    return out


def mean_bound(n, Lmax, extra=0):
    """|mean_f32 - mean_64| <= (8 + n) u max|L|: at most 7 roundings in the interpolation (dense_cases.val_bound), n - 1 additions and one
    division, each relative to a magnitude of at most max|L| (a mean of convex combinations).  extra: further roundings of a reference."""
    return (8 + np.asarray(n, np.float64) + extra) * U * float(Lmax)


# ------------------------------------------------------------------------------------------------------------------- data
def case_geometry(c):
    h, w, ch, cw, sh, sw = c
    return starts(h, ch, sh), starts(w, cw, sw), ch // PATCH, cw // PATCH


def window_logits(nwin, P, C, seed):
    return np.stack([dc.gaussian_logits(P, C, seed + 7 * k) for k in range(nwin)])


def case_logits(ci, C):
    ys, xs, h0, w0 = case_geometry(CASES[ci])
    return window_logits(len(ys) * len(xs), h0 * w0, C, 1000 * ci + C)


def exact_probes():
    """(name, Ls, ys, xs, h0, w0, ch, cw, h, w, reduce, centers, eps, expected dict) whose expectations do not come from `emulate`."""
    out = []
    rng = np.random.default_rng(17)
    # integer logits at a dyadic scale (grid 4 x 4 under a 16 x 16 crop: lambdas are multiples of 1/8) with covers 1, 2 and 4: every product, sum
    # and division is exact, so every order and float64 agree bit for bit
    ys, xs = starts(24, 16, 8), starts(24, 16, 8)
    assert ys.tolist() == [0, 8] and set(np.unique(cover_map(ys, xs, 16, 16, 24, 24))) == {1, 2, 4}
    for C in (2, 21):
        Ls = rng.integers(-64, 64, size=(4, 16, C)).astype(f32)
        ref = reference(Ls, ys, xs, 4, 4, 16, 16, 24, 24)
        assert (ref["val"] == ref["val"].astype(f32)).all()
        out.append(("integer-C%d" % C, Ls, ys, xs, 4, 4, 16, 16, 24, 24, ARGMAX, None, 0.0,
                    {"labels": ref["labels"], "value": ref["value"].astype(f32)}))
    # planted ties across windows: classes 3 and 7 hold the same values in every window and win everywhere; the lowest class takes them
    h, w, ch, cw, sh, sw = CASES[2]
    ys, xs, h0, w0 = case_geometry(CASES[2])
    Ls = window_logits(len(ys) * len(xs), h0 * w0, 21, 23)
    Ls[:, :, 3] = Ls[:, :, 7] = np.abs(Ls).max() + 1 + rng.random((Ls.shape[0], Ls.shape[1])).astype(f32)
    out.append(("tie-3-7", Ls, ys, xs, h0, w0, ch, cw, h, w, ARGMAX, None, 0.0, {"labels": np.full((h, w), 3, np.uint8)}))
    # one window: dinov2_hip_predict_dense's reduction (contract 5)
    L = dc.gaussian_logits(9, 21, 29)
    out.append(("one-window-argmax", L[None], [0], [0], 3, 3, 42, 42, 42, 42, ARGMAX, None, 0.0, dc.emulate(L, 3, 3, 42, 42)))
    cen = dc.bin_centers(21)
    out.append(("one-window-bins", L[None], [0], [0], 3, 3, 42, 42, 42, 42, BINS, cen, 0.1, dc.emulate(L, 3, 3, 42, 42, BINS, cen, 0.1)))
    # two windows holding +v and -v (v_c = c + 1 on every token; the dyadic geometry again, so a constant resamples to itself): 0 on the overlap
    # -- every class ties, the lowest wins, the value is +0 -- and +v / -v off it
    C = 5
    v = np.arange(1, C + 1, dtype=f32)
    Ls = np.stack([np.tile(v, (16, 1)), np.tile(-v, (16, 1))])
    lab = np.zeros((16, 24), np.uint8)
    val = np.zeros((16, 24), f32)
    lab[:, :8], val[:, :8] = C - 1, C
    val[:, 16:] = -1
    out.append(("plus-minus", Ls, [0], [0, 8], 4, 4, 16, 16, 16, 24, ARGMAX, None, 0.0, {"labels": lab, "value": val}))
    # BINS with all-negative logits: every mean is negative, every r is eps, the result is the mean of the centres (eps and centres dyadic)
    ys, xs, h0, w0 = case_geometry(CASES[2])
    Ls = -np.abs(window_logits(len(ys) * len(xs), h0 * w0, 16, 31)) - 1
    out.append(("bins-all-negative", Ls, ys, xs, h0, w0, ch, cw, h, w, BINS, np.arange(16, dtype=f32), 0.125, {"value": np.full((h, w), 7.5, f32)}))
    return out


compare = dc.compare


def reduce_failures(fn, cases=range(len(CASES)), classes=CLASSES):
    """fn(Ls, ys, xs, h0, w0, ch, cw, h, w, reduce, centers, eps) -> dict as `emulate`.  Every case x C x both reductions against the
    restatement, then the exact probes against their own expectations."""
    fails = []
    for ci in cases:
        h, w, ch, cw, _, _ = CASES[ci]
        ys, xs, h0, w0 = case_geometry(CASES[ci])
        for C in classes:
            Ls = case_logits(ci, C)
            what = "%s C=%d" % (case_id(CASES[ci]), C)
            fails += compare(fn(Ls, ys, xs, h0, w0, ch, cw, h, w, ARGMAX, None, 0.0), emulate(Ls, ys, xs, h0, w0, ch, cw, h, w), "argmax " + what)
            cen = dc.bin_centers(C)
            fails += compare(fn(Ls, ys, xs, h0, w0, ch, cw, h, w, BINS, cen, 0.1), emulate(Ls, ys, xs, h0, w0, ch, cw, h, w, BINS, cen, 0.1),
                             "bins " + what)
    for name, Ls, ys, xs, h0, w0, ch, cw, h, w, red, cen, eps, exp in exact_probes():
        fails += compare(fn(Ls, ys, xs, h0, w0, ch, cw, h, w, red, cen, eps), exp, "probe " + name)
    return fails


def gather_reference(img, ys, xs, ch, cw, chw=True):
    """The window batch by numpy slicing: img [3, h, w] (chw) or [h, w, 3]."""
    if chw:
        return np.stack([img[:, y:y + ch, x:x + cw] for y in ys for x in xs])
    return np.stack([img[y:y + ch, x:x + cw, :] for y in ys for x in xs])
