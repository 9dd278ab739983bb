"""Helpers for the kernels of csrc/kernels_misc.hip that run around the GEMMs: LayerNorm, device preprocess, classifier head, weight
conversion and bias permutation.  float64 references, numpy emulations of each kernel's exact arithmetic (its rounding points), exact
probes and derived bounds.  Imported by tests/test_gpu_misc_kernels.py (the HIP kernels) and tests/test_misc_probes.py (the emulations and
their planted bugs, no GPU).  Plain module, no fixtures.

Every emulation takes `mutant`: the name of one planted bug (MUTANTS) or None.  test_misc_probes.py checks that each emulation passes the
checks the GPU tests apply, and that each mutant is rejected by them.
"""
import numpy as np

F32, F16, BF16 = -1, 0, 1
DT_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
U32 = 2.0 ** -24  # unit roundoff of f32

MUTANTS = ("bf16_truncate", "pool_includes_registers", "pool_starts_late", "interleave_swapped", "softmax_no_max",
           "ln_fused_affine", "ln_var_from_moments", "fused_bicubic_taps")

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- rounding
def round_t(a, dt, mutant=None):
    """f32 values -> the output type (nearest even), returned as f32.  dt = F32 leaves them alone."""
    a = np.asarray(a, np.float32)
    if dt == F32:
        return a.copy()
    if dt == F16:
        return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32)
    if mutant == "bf16_truncate":
        r = u & np.uint32(0xFFFF0000)
    else:
        r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.astype(np.uint32).view(np.float32)


def fma32(a, b, c):
    """f32(a * b + c) with one rounding: the product of two f32 is exact in double, the sum is rounded once to double and then to
    f32 -- a double rounding, which is close enough for a planted bug (it only has to differ from the unfused sequence)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def diff_count(a, b):
    """Number of elements whose bits differ (NaN counts as differing)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def check_exact(got, exp, what):
    """(ok, message): bit-for-bit equality, with the number of differing elements."""
    n = diff_count(got, exp)
    if n == 0:
        return True, ""
    a, b = np.asarray(got, np.float32).ravel(), np.asarray(exp, np.float32).ravel()
    i = int(np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))[0])
    return False, "%s: %d of %d elements differ (first at %d: got %r, expected %r)" % (what, n, a.size, i, a[i], b[i])


# ------------------------------------------------------------------------------------------------------------- LayerNorm
# layernorm_kernel (ggml_norm + mul + add, dinov2.cpp:694-700): mean = f32(sum / H) with sum in double; v = f32(x - mean);
# var = f32(sum_double(f32(v * v)) / H); scale = 1 / sqrtf(var + eps) in f32; y = f32(f32(f32(v * scale) * w) + b), then the
# store's rounding to T.  Widths: each MAXV branch of ln_dispatch (2: H <= 512, 4: <= 1024, 8: <= 2048), its edges, and widths that
# leave lanes idle (4, 516).
LN_WIDTHS = (4, 128, 256, 384, 512, 516, 768, 1024, 1536, 2048)
LN_ROWS = (1, 2, 3, 5, 301, 4097)


def ln_emulate(x, w, b, eps, dt, mutant=None):
    x = np.asarray(x, np.float32)
    H = x.shape[1]
    s = x.astype(np.float64).sum(axis=1, keepdims=True)
    mean = (s / H).astype(np.float32)
    v = (x - mean).astype(np.float32)
    if mutant == "ln_var_from_moments":  # E[x^2] - mean^2, squares in f32 as the kernel would form them
        var = ((x * x).astype(np.float64).sum(axis=1, keepdims=True) / H - mean.astype(np.float64) ** 2).astype(np.float32)
    else:
        var = ((v * v).astype(np.float64).sum(axis=1, keepdims=True) / H).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = (f32(1.0) / np.sqrt(var + f32(eps))).astype(np.float32)
    vs = (v * scale).astype(np.float32)
    if mutant == "ln_fused_affine":
        y = fma32(vs, w[None, :], b[None, :])
    else:
        y = ((vs * w[None, :]).astype(np.float32) + b[None, :]).astype(np.float32)
    return round_t(y, dt, mutant)


def ln_reference(x, w, b, eps):
    """float64 LayerNorm of the f32 input."""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(axis=1, keepdims=True) + eps) * w.astype(np.float64) + b.astype(np.float64)


def ln_affine(H, seed):
    """Random full-mantissa f32 w and b: fused and unfused affine differ in a good share of the elements."""
    rng = np.random.default_rng(seed)
    w = (1.0 + 0.5 * rng.standard_normal(H)).astype(np.float32)
    b = (0.5 * rng.standard_normal(H)).astype(np.float32)
    return w, b


def ln_dyadic_rows(rows, H, seed):
    """Rows whose statistics are exact in any summation order: x = c + p with c a short dyadic centre (a multiple of 1/8 below 128)
    and p a zero-sum pattern of multiples of 2^-4 (r - permutation(r), r integers in [-12, 12]).  So sum = H c exactly, mean = c,
    v = p exactly, f32(v * v) = p^2 exactly and the double sum of squares is exact: only var, scale and the affine round."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-1023, 1024, size=(rows, 1)) / 8.0
    r = rng.integers(-12, 13, size=(rows, H))
    p = (r - rng.permuted(r, axis=1)) / 16.0
    if H > 1:
        flat = np.flatnonzero((p == 0).all(axis=1))  # a constant row would make var 0: give it a +-1/16 pair
        p[flat, 0], p[flat, 1] = 1 / 16.0, -1 / 16.0
    return (c + p).astype(np.float32)


def ln_offset_rows(rows, H, seed):
    """Large-offset (outlier-channel) rows: mean ~ 1e4, std ~ 1e-2.  The f32 values are multiples of 2^-10 below 2^14, so the sums
    are still exact in double and the emulation stays bit-exact; against float64 the f32 mean costs up to half an ulp of 1e4."""
    rng = np.random.default_rng(seed)
    m = 1e4 + 100.0 * rng.standard_normal((rows, 1))
    return (m + 1e-2 * rng.standard_normal((rows, H))).astype(np.float32)


def ln_offset_bound(x, w, b, eps, dt):
    """Per-element bound of |kernel - float64| for ln_offset_rows, from the kernel's arithmetic:
      mean: f32(sum / H) is off by dm <= half an f32 ulp of the mean (+ 2^-52 |mean| for the double division);  v = x - mean is exact (Sterbenz),
      so every v is shifted by dm and var grows by dm^2;  var, v*v, +eps, sqrt and the division round with <= 4u relative in
      scale (f32);  then v * scale, * w and + b round once each (3u of |y| parts), and T adds u_T |y|.
    |y - y64| <= e + u_T (|y64| + e),  e = |w| (dm s + |z| (dm^2 / (2 sigma^2) + 4u)) + 3u (|z w| + |b|),  with s = 1/sqrt(var + eps), z = (x - mu) s."""
    x64 = np.asarray(x, np.float64)
    mu = x64.mean(axis=1, keepdims=True)
    var = ((x64 - mu) ** 2).mean(axis=1, keepdims=True)
    s = 1.0 / np.sqrt(var + eps)
    z = (x64 - mu) * s
    dm = np.abs(np.spacing(mu.astype(np.float32)).astype(np.float64)) / 2 + np.abs(mu) * 2.0 ** -52
    aw, ab = np.abs(w.astype(np.float64)), np.abs(b.astype(np.float64))
    y = z * w + b
    ut = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}[dt]
    e = aw * (dm * s + np.abs(z) * (dm * dm * s * s / 2 + 4 * U32)) + 3 * U32 * (np.abs(z) * aw + ab)
    return e + ut * (np.abs(y) + e) + 1e-30


# ------------------------------------------------------------------------------------------------------------- preprocess
# preprocess_u8_kernel against the host dinov2_hip_preprocess: the same sequence of f32 operations.  The sizes of
# tests/cpp/preprocess_san.cpp (tiny, smaller than a patch, odd, extreme aspect ratios) and a few seeded random ones.
PP_SIZES = [(1, 1), (1, 7), (7, 1), (13, 13), (14, 14), (15, 29), (224, 224), (518, 518), (480, 854), (3, 2000), (2000, 3), (257, 255)]
PP_SIZES += [tuple(int(v) for v in np.random.default_rng(2024 + i).integers(1, 701, 2)) for i in range(4)]
PP_MEAN = np.array([0.406, 0.456, 0.485], np.float32)  # BGR order
PP_STD = np.array([0.225, 0.224, 0.229], np.float32)


def cubic_taps(t, mutant=None):
    """cv::resize INTER_CUBIC taps (A = -0.75) in f32, every operation rounded (csrc/preprocess.cpp: cubic_taps).  mutant
    'fused_bicubic_taps': each a * b + c of the polynomials as one FMA (what hipcc made of cubic_taps_dev before its pragma)."""
    t = np.asarray(t, np.float32)
    A, one = f32(-0.75), f32(1.0)
    t1, mt = (t + one).astype(np.float32), (one - t).astype(np.float32)
    if mutant == "fused_bicubic_taps":
        w0 = fma32(fma32(fma32(A, t1, f32(-5.0) * A), t1, f32(8.0) * A), t1, f32(-4.0) * A)
        w1 = fma32((fma32(A + f32(2), t, -(A + f32(3))) * t).astype(np.float32), t, one)
        w2 = fma32((fma32(A + f32(2), mt, -(A + f32(3))) * mt).astype(np.float32), mt, one)
    else:
        w0 = ((((A * t1) - f32(5.0) * A) * t1 + f32(8.0) * A) * t1 - f32(4.0) * A).astype(np.float32)
        w1 = ((((A + f32(2)) * t - (A + f32(3))) * t) * t + one).astype(np.float32)
        w2 = ((((A + f32(2)) * mt - (A + f32(3))) * mt) * mt + one).astype(np.float32)
    w3 = (((one - w0) - w1) - w2).astype(np.float32)
    return np.stack([w0, w1, w2, w3], -1).astype(np.float32)


def _axis(src, dst, off, n, mutant):
    scale = f32(src) / f32(dst)
    d = np.arange(off, off + n, dtype=np.float32)
    f = ((d + f32(0.5)) * scale - f32(0.5)).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    w = cubic_taps((f - s.astype(np.float32)).astype(np.float32), mutant)
    idx = np.clip(s[:, None] - 1 + np.arange(4)[None, :], 0, src - 1)
    return idx, w


def preprocess_size(mode, h, w, patch):
    if mode == 1:
        return 224, 224
    return (h // patch + 1) * patch, (w // patch + 1) * patch


def preprocess_emulate(img, mode, patch, mutant=None):
    """u8 BGR [h, w, 3] -> f32 BGR [oh, ow, 3] with the rounding points of csrc/preprocess.cpp: x / 255 as x * f32(1/255); horizontal
    taps summed left to right, then vertical; (v - mean) / std."""
    h, w = img.shape[:2]
    oh, ow = preprocess_size(mode, h, w, patch)
    rh, rw = (256, 256) if mode == 1 else (oh, ow)
    y0, x0 = (rh - oh) // 2, (rw - ow) // 2
    ix, wx = _axis(w, rw, x0, ow, mutant)
    iy, wy = _axis(h, rh, y0, oh, mutant)
    inv = f32(1.0 / 255.0)
    src = img.astype(np.float32)
    hb = np.zeros((h, ow, 3), np.float32)
    for k in range(4):
        term = ((src[:, ix[:, k], :] * inv).astype(np.float32) * wx[None, :, k, None]).astype(np.float32)
        hb = term if k == 0 else (hb + term).astype(np.float32)
    out = np.zeros((oh, ow, 3), np.float32)
    for k in range(4):
        term = (hb[iy[:, k], :, :] * wy[:, k, None, None]).astype(np.float32)
        out = term if k == 0 else (out + term).astype(np.float32)
    return ((out - PP_MEAN) / PP_STD).astype(np.float32)


def pp_images(B, h, w, seed):
    """B different images: white noise, a ramp and, from the third on, noise again (other seeds)."""
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    if B > 1:
        yy, xx = np.mgrid[0:h, 0:w]
        imgs[1] = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) % 256)], -1).astype(np.uint8)
    return imgs


# ------------------------------------------------------------------------------------------------------------- head
# launch_head (forward_head, dinov2.cpp:792-821):
#   head_pool_kernel:   feat[b] = [T(fin[b, 0]) ; T(f32(f32(sum_{t >= first} fin[b, t]) * inv_div))], the sum in double;
#   head_logits_kernel: one wave per class, lane l sums k = 8 l + 512 j + e (e = 0..7) into an f32 accumulator, then 6 xor-shuffle
#                       levels, then + bias;
#   head_softmax_kernel: max, double sum of expf(l - max), inv = f32(1 / sum), p = expf(l - max) * inv.
HEAD_H = (384, 768, 1024, 1536)
HEAD_C = (1, 3, 1000, 1001)


def head_pool_emulate(fin, first, inv_div, dt, R=0, mutant=None):
    fin = np.asarray(fin, np.float32)
    if mutant == "pool_includes_registers":
        first = 1
    elif mutant == "pool_starts_late":
        first = first + 1
    tot = fin[:, first:, :].astype(np.float64).sum(axis=1)
    pm = (tot.astype(np.float32) * f32(inv_div)).astype(np.float32)
    return np.concatenate([round_t(fin[:, 0, :], dt, mutant), round_t(pm, dt, mutant)], axis=1)


def head_logits_n(K):
    """Length of the longest rounding chain of head_logits_kernel for a row of K = 2H: a lane adds 8 products per 512-column stride
    (ceil(K / 512) strides: 8 ceil(K / 512) additions, each product rounded too when not fused: +1), the wave sum is 6 xor-shuffle
    levels, and the bias is one more addition."""
    return 8 * ((K + 511) // 512) + 1 + 6 + 1


def head_logits_bound(feat, Wt, bias):
    """|logit - logit64| <= gamma_n (sum_k |w_k f_k| + |bias|) + u |logit64|, n = head_logits_n(K): Higham's bound for a recursive
    sum of n-deep chains over the same terms."""
    K = feat.shape[1]
    n = head_logits_n(K)
    g = n * U32 / (1 - n * U32)
    mag = np.abs(feat.astype(np.float64)) @ np.abs(Wt.astype(np.float64)).T + np.abs(bias.astype(np.float64))[None, :]
    ref = feat.astype(np.float64) @ Wt.astype(np.float64).T + bias.astype(np.float64)[None, :]
    return ref, g * mag + U32 * np.abs(ref) + 1e-30


def softmax_emulate(logits, mutant=None):
    """head_softmax_kernel in numpy; np.exp in float64 rounded to f32 stands in for the device expf."""
    l = np.asarray(logits, np.float32)
    mx = np.zeros_like(l[:, :1]) if mutant == "softmax_no_max" else l.max(axis=1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp((l - mx).astype(np.float32).astype(np.float64)).astype(np.float32)
        inv = (1.0 / e.astype(np.float64).sum(axis=1, keepdims=True)).astype(np.float32)
        return (e * inv).astype(np.float32)


EXPF_ULP = 2.0  # allowance for the device expf: the HIP math-function table lists 1 ulp for expf; not measured here, so taken twice


def softmax_bound(logits):
    """|p - p64| for p64 = the float64 softmax of the kernel's own f32 logits: d = f32(l - max) rounds by <= u |d|, which moves
    exp(d) by |d| u relative; expf adds EXPF_ULP ulps (2u each, relative); so every e_c is within eps_c = (|d_c| + 2 EXPF_ULP) u.
    The double sum adds nothing at f32 scale, 1 / sum and the final product round once each: |p_c - p64_c| <= p64_c (eps_c +
    max eps + 2u + 2^-40).  Plus 2^-126 absolute for results in the subnormal range."""
    l = np.asarray(logits, np.float64)
    d = l - l.max(axis=1, keepdims=True)
    p = np.exp(d)
    p /= p.sum(axis=1, keepdims=True)
    eps = (np.abs(d) + 2 * EXPF_ULP) * U32
    return p, p * (eps + eps.max(axis=1, keepdims=True) + 2 * U32 + 2.0 ** -40) + 2.0 ** -126


def head_dyadic_case(B, T, H, C, R, dt, seed):
    """fin multiples of 2^-12 with |x| < 8 (any double sum over <= 4101 tokens is exact); W, bias random; returns fin, W, bias."""
    rng = np.random.default_rng(seed)
    fin = (rng.integers(-32767, 32768, size=(B, T, H)) / 4096.0).astype(np.float32)
    W = round_t((rng.standard_normal((C, 2 * H)) * 0.05).astype(np.float32), dt)
    bias = (0.1 * rng.standard_normal(C)).astype(np.float32)
    return fin, W, bias


def head_exact_logits_case(B, H, C, seed):
    """A probe whose logits are exact in any order: 1 + 16 tokens of multiples of 2^-2 in [-1, 1], divisor 16 (inv_div 2^-4), so feat
    holds multiples of 2^-6 of magnitude <= 1 (7 bits: exact in bf16 and f16); W multiples of 2^-6 in [-1/16, 1/16]; bias multiples
    of 2^-12 in [-1, 1].  Every product is a multiple of 2^-12 below 1 and every partial sum stays below K + 1 <= 3073 < 2^12: 24 bits,
    exact in f32.  The small W keeps the logits within a few units of each other (head_logit_spread_ok), so that the softmax's double
    sum of expf values is exact in any order too.  Returns fin, W, bias, first, inv_div."""
    rng = np.random.default_rng(seed)
    T = 17
    fin = (rng.integers(-4, 5, size=(B, T, H)) / 4.0).astype(np.float32)
    W = (rng.integers(-4, 5, size=(C, 2 * H)) / 64.0).astype(np.float32)
    bias = (rng.integers(-4096, 4097, size=C) / 4096.0).astype(np.float32)
    return fin, W, bias, 1, 1.0 / 16


# ------------------------------------------------------------------------------------------------------------- weights
# convert_weight_kernel: dequantise (oracle/gguf_np.dequantize; F32 / F16 / BF16 as stored) and round to T (nearest even), zero
# padding columns K .. Kpad; interleaveF = F > 0: weight row n is source row ((n >> 5) & 1) F + (n >> 6) 32 + (n & 31).
CONVERT_TYPES = ("f32", "f16", "bf16", "q8_0", "q4_0", "q4_1", "q5_0", "q5_1")


def interleave_rows(a, F, mutant=None):
    """SwiGLU weights_in [x1 (F rows); x2 (F rows)] -> alternating 32-row blocks x1 | x2, restated with reshapes (independent of the
    kernel's index formula).  Works on rows of any trailing shape."""
    a = np.asarray(a)
    x1 = a[:F].reshape(F // 32, 32, *a.shape[1:])
    x2 = a[F:2 * F].reshape(F // 32, 32, *a.shape[1:])
    pair = (x2, x1) if mutant == "interleave_swapped" else (x1, x2)
    return np.stack(pair, axis=1).reshape(2 * F, *a.shape[1:])


def weight_source(tname, N, K, seed):
    """(raw bytes, ggml type id, f32 values the dequantiser gives) for a random [N, K] tensor stored as `tname`."""
    from oracle import gguf_np as G
    from importlib import import_module
    gw = import_module("dinov2_cpp_amd.gguf_writer")
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N, K)) * 0.05 + rng.standard_normal((N, 1)) * 0.01).astype(np.float32)
    gt = gw.NAME_TYPE[tname]
    if tname == "f32":
        return w.tobytes(), gt, w
    if tname == "f16":
        h = w.astype(np.float16)
        return h.tobytes(), gt, h.astype(np.float32)
    if tname == "bf16":
        v = round_t(w, BF16)
        return (v.view(np.uint32) >> 16).astype(np.uint16).tobytes(), gt, v
    q = gw.quantize(w, gt)
    return q.tobytes(), gt, G.dequantize(q, gt, (N, K))


def convert_expected(vals, dt, Kpad, F=0, mutant=None):
    N, K = vals.shape
    out = np.zeros((N, Kpad), np.float32)
    out[:, :K] = round_t(vals, dt, mutant)
    return interleave_rows(out, F, mutant) if F > 0 else out


def head_logit_spread_ok(logits):
    """True when every expf(l - max) >= e^-12 > 2^-18: then each is a multiple of 2^-41 below 1, and a double sum of <= 1001 of
    them (below 2^10) needs at most 51 bits -- exact in any order, so permuting classes permutes the probabilities bit for bit."""
    l = np.asarray(logits, np.float64)
    return bool((l.max(axis=1) - l.min(axis=1) < 12).all())


def head_logits_emulate(feat, Wt, bias):
    """head_logits_kernel's summation order in f32 (products rounded, not fused): lane l adds k = 8 l + 512 j + e in order, then the
    xor-shuffle tree (offsets 32 .. 1), then the bias."""
    feat, Wt = np.asarray(feat, np.float32), np.asarray(Wt, np.float32)
    B, K = feat.shape
    Cn = Wt.shape[0]
    acc = np.zeros((B, Cn, 64), np.float32)
    for k0 in range(0, K, 512):
        for e in range(8):
            k = k0 + 8 * np.arange(64) + e
            live = k < K
            kk = np.where(live, k, 0)
            prod = (feat[:, None, kk] * Wt[None, :, kk]).astype(np.float32)
            acc = np.where(live[None, None, :], (acc + prod).astype(np.float32), acc)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, :, np.arange(64) ^ o]).astype(np.float32)
    return (acc[:, :, 0] + bias[None, :]).astype(np.float32)
