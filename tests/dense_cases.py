"""Cases for dinov2_hip_predict_dense / dinov2_hip_op_dense_reduce / dinov2_hip_op_dense_pack (csrc/dense.hip), shared by
tests/test_dense_probes.py (CPU: the numpy restatement through these cases, and the planted bugs they must reject) and tests/test_gpu_dense.py
(the kernels through the same cases).  Plain module, no fixtures.  `mutant`: the name of one planted bug (MUTANTS) or None.

The restatement follows the contract of include/dinov2_hip.h, section "linear dense-prediction heads":
  1 operand   A^ = f16 of the tapped patch rows (with the model's final LayerNorm when `norm`), per layer [patch ; cls of the image], W^ = f16(W)
  2 logits    L = sum_k A^ W^ + bias, f32 accumulation in an order fixed by K -- checked against float64 of the SAME f16 operands within
              logits_bound: (K + 2) 2^-24 (sum_k |a^ w^| + |bias|), the classical worst case of ANY f32 summation order of K exact products
              plus the bias addition (gamma_{K+1} <= (K + 2) u for K u << 1, u = 2^-24)
  3 resample  bilinear, half-pixel, align_corners=False, every operation a separate float32 rounding (numpy float32 arithmetic never fuses)
  4 ARGMAX    first maximum in ascending class order (numpy argmax: the first occurrence; -0 == +0)
  5 BINS      r = max(val, 0) + eps; S and D summed sequentially in ascending class order in float32; D / S in float32
Contracts 3 - 5 are checked bit for bit; `reference` is the same pipeline in float64.
"""
import numpy as np

from misc_cases import F32 as DT_F32
from misc_cases import check_exact, ln_emulate

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of float32
ARGMAX, BINS = "argmax", "bins"

MUTANTS = ("align_corners",        # src = dst (n_in - 1) / (n_out - 1)
           "no_clamp_at_zero",     # src may go negative: lambda < 0 in the first half pixel
           "i1_unclamped",         # i1 = i0 + 1 past the edge: reads the next row of the token-major matrix
           "xy_swapped",           # token index read as x * h0 + y
           "argmax_first",         # argmax per cell, then nearest-neighbour upsampling
           "tie_highest",          # equal values go to the highest class
           "fma",                  # interpolation contracted: float64, rounded once
           "bins_no_relu",         # r = val + eps
           "bins_no_eps",          # r = max(val, 0)
           "cls_patch_swapped",    # every layer's block is [cls ; patch]
           "layer_order_swapped",  # the layers' blocks in descending order
           "bias_dropped",
           "norm_ignored")         # the rows as they are
REDUCE_MUTANTS = MUTANTS[:9]
LOGIT_MUTANTS = MUTANTS[9:]

# (h0, w0, out_h, out_w): grids 1 x 1, 3 x 3 and the non-square 4 x 6; scale 14 (the patch size), a non-integer scale whose output is no
# multiple of any tile of dense_reduce_plan in either axis and needs several workgroups, the dyadic scale 4, a downscale, and the identity
SHAPES = ((1, 1, 1, 1), (1, 1, 14, 14), (3, 3, 42, 42), (3, 3, 7, 5), (4, 6, 56, 84), (4, 6, 50, 77), (4, 6, 16, 24), (4, 6, 2, 3), (4, 6, 4, 6))
CLASSES = (2, 21, 150, 256)


def shape_id(s):
    return "%dx%d-%dx%d" % s


# ------------------------------------------------------------------------------------------------------------------- contract 3
def axis(n_in, n_out, mutant=None):
    """(i0, i1, lambda) of every output coordinate of one axis, in float32."""
    dst = np.arange(n_out, dtype=f32)
    if mutant == "align_corners":
        scale = f32(n_in - 1) / f32(max(n_out - 1, 1))
        src = scale * dst
    else:
        scale = f32(n_in) / f32(n_out)
        src = scale * (dst + f32(0.5)) - f32(0.5)
    assert src.dtype == f32
    if mutant != "no_clamp_at_zero":
        src = np.maximum(src, f32(0))
    i0 = np.minimum(src.astype(np.int32), n_in - 1)  # (truncation, as the C cast)
    i1 = i0 + 1 if mutant == "i1_unclamped" else np.minimum(i0 + 1, n_in - 1)
    lam = src - i0.astype(f32)
    return i0, i1, lam


def interpolate(L, h0, w0, oh, ow, mutant=None, dtype=f32):
    """L [h0 * w0, C] token-major -> val [oh, ow, C].  dtype float64: the reference (same coordinates, no rounding of the arithmetic)."""
    L = np.asarray(L, f32)
    P, C = L.shape
    assert P == h0 * w0
    y0, y1, ly = axis(h0, oh, mutant)
    x0, x1, lx = axis(w0, ow, mutant)

    def rows(yy, xx):  # [oh, ow, C]; an index past the matrix (the unclamped mutant) wraps, as a read of neighbouring memory would
        tok = (xx[None, :] * h0 + yy[:, None]) if mutant == "xy_swapped" else (yy[:, None] * w0 + xx[None, :])
        return L[tok % P].astype(dtype)

    v00, v01, v10, v11 = rows(y0, x0), rows(y0, x1), rows(y1, x0), rows(y1, x1)
    if mutant == "fma" or dtype == np.float64:
        ax, ay = lx.astype(np.float64)[None, :, None], ly.astype(np.float64)[:, None, None]
        bx, by = (f32(1) - lx).astype(np.float64)[None, :, None], (f32(1) - ly).astype(np.float64)[:, None, None]
        v00, v01, v10, v11 = (v.astype(np.float64) for v in (v00, v01, v10, v11))
        val = by * (bx * v00 + ax * v01) + ay * (bx * v10 + ax * v11)
        return val.astype(dtype)
    ax, ay = lx[None, :, None], ly[:, None, None]
    bx, by = (f32(1) - lx)[None, :, None], (f32(1) - ly)[:, None, None]
    t = bx * v00 + ax * v01  # numpy: one float32 rounding per operation
    u = bx * v10 + ax * v11
    val = by * t + ay * u
    assert val.dtype == f32
    return val


# ------------------------------------------------------------------------------------------------------------------- contracts 4 and 5
def emulate(L, h0, w0, oh, ow, reduce=ARGMAX, centers=None, eps=0.0, mutant=None):
    """The restatement of dense_reduce_kernel: {"labels" [oh, ow] uint8, "value" [oh, ow] f32} (ARGMAX) or {"value"} (BINS)."""
    L = np.asarray(L, f32)
    C = L.shape[1]
    if reduce == ARGMAX and mutant == "argmax_first":
        lab_lr = np.argmax(L, axis=1).reshape(h0, w0)
        yy = np.minimum(((np.arange(oh) + 0.5) * h0 / oh).astype(np.int64), h0 - 1)
        xx = np.minimum(((np.arange(ow) + 0.5) * w0 / ow).astype(np.int64), w0 - 1)
        labels = lab_lr[yy[:, None], xx[None, :]]
        val = interpolate(L, h0, w0, oh, ow)
        return {"labels": labels.astype(np.uint8), "value": np.take_along_axis(val, labels[..., None], 2)[..., 0]}
    val = interpolate(L, h0, w0, oh, ow, mutant)
    if reduce == ARGMAX:
        if mutant == "tie_highest":
            labels = C - 1 - np.argmax(val[..., ::-1], axis=2)
        else:
            labels = np.argmax(val, axis=2)  # the first occurrence of the maximum; -0.0 == +0.0
        return {"labels": labels.astype(np.uint8), "value": np.ascontiguousarray(np.take_along_axis(val, labels[..., None], 2)[..., 0])}
    cen = np.asarray(centers, f32)
    S = np.zeros(val.shape[:2], f32)
    D = np.zeros(val.shape[:2], f32)
    for c in range(C):  # sequential, ascending: the stated order
        r = val[..., c] if mutant == "bins_no_relu" else np.maximum(val[..., c], f32(0))
        if mutant != "bins_no_eps":
            r = r + f32(eps)
        S = S + r
        D = D + r * cen[c]
    with np.errstate(invalid="ignore", divide="ignore"):
        value = D / S
    assert value.dtype == f32
    return {"value": value}


def reference(L, h0, w0, oh, ow, reduce=ARGMAX, centers=None, eps=0.0):
    """float64 of the same pipeline on float64 logits L: {"val" [oh, ow, C], "labels", "value", "margin" (top-1 minus top-2, ARGMAX)}."""
    L = np.asarray(L, np.float64)
    C = L.shape[1]
    y0, y1, ly = axis(h0, oh)
    x0, x1, lx = axis(w0, ow)
    ly, lx = ly.astype(np.float64)[:, None, None], lx.astype(np.float64)[None, :, None]
    g = L.reshape(h0, w0, C)
    val = (1 - ly) * ((1 - lx) * g[y0][:, x0] + lx * g[y0][:, x1]) + ly * ((1 - lx) * g[y1][:, x0] + lx * g[y1][:, x1])
    out = {"val": val}
    if reduce == ARGMAX:
        out["labels"] = np.argmax(val, axis=2).astype(np.uint8)
        srt = np.sort(val, axis=2)
        out["value"] = srt[..., -1]
        out["margin"] = srt[..., -1] - srt[..., -2]
    else:
        r = np.maximum(val, 0.0) + float(eps)
        out["value"] = (r * np.asarray(centers, np.float64)).sum(2) / r.sum(2)
    return out


def interp_abs(B, h0, w0, oh, ow):
    """The interpolation weights applied to a non-negative per-logit quantity B [P, C] (a bound, or |L|), float64: [oh, ow, C]."""
    return reference(np.asarray(B, np.float64), h0, w0, oh, ow, BINS, np.zeros(B.shape[1]), 1.0)["val"]


def val_bound(Lbound, Labs, h0, w0, oh, ow):
    """|val_f32(L~) - val_64(L)| per pixel and class, when every |L~ - L| <= Lbound: the logits' own error passes through the convex
    combination unamplified (the float32 weights 1 - lambda, lambda sum to 1 within u each: factor 1 + 2 u, folded into the 7 below), and the
    float32 interpolation adds at most 7 u times the interpolated magnitudes: each term passes one rounding of 1 - lambda, two products and
    two additions, and is bounded by the weighted sum of |L| + Lbound (gamma_5, taken as 7 u with the weight roundings)."""
    mag = np.asarray(Labs, np.float64) + np.asarray(Lbound, np.float64)
    return interp_abs(Lbound, h0, w0, oh, ow) + 7 * U * interp_abs(mag, h0, w0, oh, ow)


def bins_bound(Lbound, L64, h0, w0, oh, ow, centers, eps):
    """|value_f32 - value_64| per pixel for BINS, derived from val_bound:
        r_c = max(val_c, 0) + eps:       e_r <= e_val + u r~                               (max is 1-Lipschitz; one addition)
        S = sum r (sequential):          e_S <= sum e_r + (C - 1) u sum r~                 (gamma_{C-1} on non-negative terms)
        D = sum r cen (sequential):      e_D <= sum e_r |cen| + (C + 1) u sum r~ |cen|     (one product more per term)
        value = D / S:                   e   <= (e_D + |D/S| e_S) / (S - e_S) + u |D/S|    (S >= C eps > e_S is asserted)
    with r~ <= r + e_r."""
    C = L64.shape[1]
    cen = np.abs(np.asarray(centers, np.float64))
    ref = reference(L64, h0, w0, oh, ow, BINS, centers, eps)
    r = np.maximum(ref["val"], 0.0) + float(eps)
    e_r = val_bound(Lbound, np.abs(L64), h0, w0, oh, ow)
    e_r = e_r + U * (r + e_r)
    rt = r + e_r
    S = r.sum(2)
    e_S = e_r.sum(2) + (C - 1) * U * rt.sum(2)
    e_D = (e_r * cen).sum(2) + (C + 1) * U * (rt * cen).sum(2)
    assert (S >= C * float(eps) * (1 - 1e-12)).all() and (e_S < S).all()
    q = np.abs(ref["value"])
    return (e_D + q * e_S) / (S - e_S) + U * q


# ------------------------------------------------------------------------------------------------------------------- data
def gaussian_logits(P, C, seed, std=4.0):
    return (np.random.default_rng(seed).standard_normal((P, C)) * std).astype(f32)


def bin_centers(C, lo=0.001, hi=10.0):
    return np.linspace(lo, hi, C).astype(f32)


def exact_probes():
    """(name, L, h0, w0, oh, ow, reduce, centers, eps, expected dict) whose expectations do not come from `emulate`."""
    out = []
    # integer logits at dyadic scales: lambdas are multiples of 1/8, every product and sum is exact, so every order and float64 agree
    rng = np.random.default_rng(7)
    for (h0, w0, oh, ow) in ((4, 6, 16, 24), (3, 3, 6, 12), (4, 6, 8, 6)):
        for C in (2, 21):
            L = rng.integers(-64, 64, size=(h0 * w0, C)).astype(f32)
            ref = reference(L, h0, w0, oh, ow)  # (exact ties may occur: float64 argmax takes the first maximum too)
            assert (ref["val"] == ref["val"].astype(f32)).all()
            out.append(("integer-%s-C%d" % (shape_id((h0, w0, oh, ow)), C), L, h0, w0, oh, ow, ARGMAX, None, 0.0,
                        {"labels": ref["labels"], "value": ref["value"].astype(f32)}))
    # planted ties: classes 3 and 7 hold the same values everywhere and win; the lowest class takes them
    L = gaussian_logits(24, 21, 11)
    L[:, 3] = L[:, 7] = np.abs(L).max() + 1 + np.arange(24, dtype=f32)
    exp_val = interpolate(L, 4, 6, 50, 77)[..., 3]
    out.append(("tie-3-7", L, 4, 6, 50, 77, ARGMAX, None, 0.0, {"labels": np.full((50, 77), 3, np.uint8), "value": exp_val}))
    # -0 in class 0 against +0 in class 1, everything else negative: equal, so class 0 -- and the value keeps class 0's sign bit
    L = -np.abs(gaussian_logits(9, 5, 12)) - 1
    L[:, 0] = -0.0
    L[:, 1] = 0.0
    out.append(("tie-minus-zero", L, 3, 3, 42, 42, ARGMAX, None, 0.0,
                {"labels": np.zeros((42, 42), np.uint8), "value": np.full((42, 42), -0.0, f32)}))
    # between a cell where class 0 wins and a cell where class 1 wins, class 2 (second in both) wins the interpolated logits
    L = np.zeros((2, 3), f32)
    L[0] = (10, 0, 8)
    L[1] = (0, 10, 8)
    lab = np.array([[0, 2, 2, 1]], np.uint8)  # lambda = 0, .25, .75, (edge) 1: max(10 (1 - l), 10 l) = 7.5 against 8 in the middle
    val = np.array([[10, 8, 8, 10]], f32)
    out.append(("argmax-after-interpolation", L, 1, 2, 1, 4, ARGMAX, None, 0.0, {"labels": lab, "value": val}))
    # BINS with all-negative logits: every r is eps, the result is the mean of the centres (eps and the centres dyadic: exact)
    L = -np.abs(gaussian_logits(24, 16, 13)) - 1
    out.append(("bins-all-negative", L, 4, 6, 50, 77, BINS, np.arange(16, dtype=f32), 0.125, {"value": np.full((50, 77), 7.5, f32)}))
    return out


def compare(got, exp, what):
    """Failure messages: labels equal, value bit for bit."""
    fails = []
    for key in exp:
        if key not in got:
            fails.append("%s: no %s" % (what, key))
        elif key == "labels":
            g, e = np.asarray(got[key]), np.asarray(exp[key])
            if g.shape != e.shape or (g != e).any():
                n = int((g != e).sum()) if g.shape == e.shape else -1
                fails.append("%s labels: %d pixels differ" % (what, n))
        else:
            ok, msg = check_exact(got[key], exp[key], "%s %s" % (what, key))
            if not ok:
                fails.append(msg)
    return fails


def reduce_failures(fn):
    """fn(L, h0, w0, oh, ow, reduce, centers, eps) -> dict as `emulate`.  Every shape x C x both reductions against the restatement, then
    the exact probes against their own expectations."""
    fails = []
    for si, s in enumerate(SHAPES):
        h0, w0, oh, ow = s
        for C in CLASSES:
            L = gaussian_logits(h0 * w0, C, 100 * si + C)
            fails += compare(fn(L, h0, w0, oh, ow, ARGMAX, None, 0.0), emulate(L, h0, w0, oh, ow), "argmax %s C=%d" % (shape_id(s), C))
            cen = bin_centers(C)
            fails += compare(fn(L, h0, w0, oh, ow, BINS, cen, 0.1), emulate(L, h0, w0, oh, ow, BINS, cen, 0.1),
                             "bins %s C=%d" % (shape_id(s), C))
    for name, L, h0, w0, oh, ow, red, cen, eps, exp in exact_probes():
        fails += compare(fn(L, h0, w0, oh, ow, red, cen, eps), exp, "probe " + name)
    return fails


# ------------------------------------------------------------------------------------------------------------------- contracts 1 and 2
def operand(stream, ln_w, ln_b, ln_eps, R, layers, norm, concat_cls, mutant=None):
    """stream [L + 1, B, T, H] f32 (index = blocks applied), raw -> A^ [B * P, K] float16 (contract 1)."""
    stream = np.asarray(stream, f32)
    _, B, T, H = stream.shape
    P = T - 1 - R
    ids = list(layers)[::-1] if mutant == "layer_order_swapped" else list(layers)
    blocks = []
    for layer in ids:
        x = stream[layer].reshape(B * T, H)
        if norm and mutant != "norm_ignored":
            x = ln_emulate(x, ln_w, ln_b, ln_eps, DT_F32)  # the bits of dinov2_hip_predict_layers with norm = 1 (tests/misc_cases.py)
        x = x.reshape(B, T, H)
        patch = x[:, 1 + R:].reshape(B * P, H)
        if concat_cls:
            cls = np.repeat(x[:, 0], P, axis=0)
            blocks += [cls, patch] if mutant == "cls_patch_swapped" else [patch, cls]
        else:
            blocks.append(patch)
    return np.concatenate(blocks, axis=1).astype(np.float16)


def logits_reference(A16, W, bias):
    """(float64 logits of the f16 operands, their bound): contract 2."""
    A = np.asarray(A16, np.float16).astype(np.float64)
    Wh = np.asarray(W, f32).astype(np.float16).astype(np.float64)
    b = np.zeros(Wh.shape[0]) if bias is None else np.asarray(bias, np.float64)
    ref = A @ Wh.T + b[None, :]
    bound = (A.shape[1] + 2) * U * (np.abs(A) @ np.abs(Wh).T + np.abs(b)[None, :])
    return ref, bound


def logits_emulate(A16, W, bias, mutant=None):
    """float32 logits of the f16 operands in ONE of the orders the bound covers (k-steps of 32 ascending, float32 partial sums)."""
    A = np.asarray(A16, np.float16).astype(f32)
    Wh = np.asarray(W, f32).astype(np.float16).astype(f32)
    acc = np.zeros((A.shape[0], Wh.shape[0]), f32)
    for k0 in range(0, A.shape[1], 32):
        acc = acc + (A[:, k0:k0 + 32].astype(np.float64) @ Wh[:, k0:k0 + 32].astype(np.float64).T).astype(f32)
    if bias is not None and mutant != "bias_dropped":
        acc = acc + np.asarray(bias, f32)[None, :]
    return acc


def head_weights(C, K, seed, logit_std=4.0):
    """Gaussian head weights scaled so that logits of unit-variance features have a standard deviation of about logit_std, and a bias."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((C, K)) * (logit_std / np.sqrt(K))).astype(f32)
    b = rng.standard_normal(C).astype(f32)
    return W, b


LOGIT_CASES = (  # (B, R, P, H, layers, norm, concat_cls, C)
    (2, 0, 9, 128, (1, 2), 1, 0, 21), (1, 4, 24, 128, (0, 2), 1, 1, 2), (3, 4, 9, 128, (2,), 0, 1, 150), (2, 0, 24, 128, (0, 1, 2), 0, 0, 256))


def logit_case(i):
    B, R, P, H, layers, norm, cc, C = LOGIT_CASES[i]
    rng = np.random.default_rng(300 + i)
    T = 1 + R + P
    stream = (rng.standard_normal((3, B, T, H)) * 2 + 0.5).astype(f32)  # (not zero-mean: ignoring the LayerNorm shows)
    stream *= np.array([1.0, 1.5, 0.75], f32)[:, None, None, None]
    ln_w = (1.0 + 0.3 * rng.standard_normal(H)).astype(f32)
    ln_b = (0.3 * rng.standard_normal(H)).astype(f32)
    W, b = head_weights(C, len(layers) * H * (1 + cc), 400 + i)
    return dict(stream=stream, ln_w=ln_w, ln_b=ln_b, ln_eps=1e-6, R=R, layers=layers, norm=norm, concat_cls=cc, W=W, bias=b)


def logit_failures(fn):
    """fn(case dict) -> logits [B * P, C] f32.  Each within logits_bound of the float64 product of the restated f16 operands."""
    fails = []
    for i in range(len(LOGIT_CASES)):
        c = logit_case(i)
        A = operand(c["stream"], c["ln_w"], c["ln_b"], c["ln_eps"], c["R"], c["layers"], c["norm"], c["concat_cls"])
        ref, bound = logits_reference(A, c["W"], c["bias"])
        got = np.asarray(fn(c), np.float64)
        bad = ~(np.abs(got - ref) <= bound)
        if got.shape != ref.shape or bad.any():
            fails.append("logit case %d: %d of %d outside the bound (worst %.3g of it)"
                         % (i, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got - ref) / bound))))
    return fails


def emulate_logits_case(c, mutant=None):
    A = operand(c["stream"], c["ln_w"], c["ln_b"], c["ln_eps"], c["R"], c["layers"], c["norm"], c["concat_cls"], mutant)
    return logits_emulate(A, c["W"], c["bias"], mutant)
