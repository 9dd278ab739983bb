"""The kernels of csrc/kernels_misc.hip around the GEMMs, held bit-exact to the arithmetic they claim, or to a derived bound where
the arithmetic is not exact: the device preprocess (against the host implementation), LayerNorm in every output type (against
ggml's rounding points), the classifier head (through dinov2_hip_op_head), weight conversion in every source and target type, and
the bias permutation.  Every op entry point fills its device output with NaN first, so an element the kernel never wrote shows up.
Helpers, emulations and bounds: tests/misc_cases.py; their CPU self-test: tests/test_misc_probes.py."""
import ctypes as C
import os

import numpy as np
import pytest

import misc_cases as mc

pytestmark = pytest.mark.gpu

fp = C.POINTER(C.c_float)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(fp)


def _ok(res):
    ok, msg = res
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------- preprocess
def _device_preprocess(api, mode, imgs, patch):
    B, h, w = imgs.shape[:3]
    oh, ow = mc.preprocess_size(mode, h, w, patch)
    out = np.empty((B, oh, ow, 3), np.float32)
    imgs = np.ascontiguousarray(imgs)
    assert api.lib().dinov2_hip_op_preprocess_u8(mode, imgs.ctypes.data, B, h, w, patch, out.ctypes.data) == 0
    return out


def _host_preprocess(api, mode, img, patch):
    return (api.dino_classify_preprocess if mode == 1 else api.dino_preprocess)(img, patch)


@pytest.mark.parametrize("patch", [14, 16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hw", mc.PP_SIZES, ids=["%dx%d" % s for s in mc.PP_SIZES])
def test_device_preprocess_is_bit_equal_to_host(api, hw, mode, patch):
    """preprocess_u8_kernel makes the same f32 operations as dinov2_hip_preprocess: three different images per launch."""
    h, w = hw
    imgs = mc.pp_images(3, h, w, seed=h * 7919 + w + 13 * mode + patch)
    got = _device_preprocess(api, mode, imgs, patch)
    for b in range(3):
        _ok(mc.check_exact(got[b], _host_preprocess(api, mode, imgs[b], patch), "image %d" % b))


def test_device_preprocess_grid_stride(api):
    """12 x 518^2 output pixels: more than the 8192 x 256 threads of the launch, so the grid-stride loop runs twice."""
    imgs = mc.pp_images(12, 504, 504, seed=3)
    got = _device_preprocess(api, 0, imgs, 14)
    assert got.shape == (12, 518, 518, 3) and 12 * 518 * 518 > 8192 * 256
    for b in range(12):
        _ok(mc.check_exact(got[b], _host_preprocess(api, 0, imgs[b], 14), "image %d" % b))


@pytest.mark.parametrize("classify", [True, False])
def test_raw_u8_predict_equals_host_preprocess_then_predict(api, classify):
    """The whole forward on raw 8-bit input equals host preprocess + f32 BGR_HWC input, bit for bit, in every output."""
    model = api.Model(os.path.join(ROOT, "tests", "golden", "tiny_gelu_reg4.gguf"), device=0, dtype=api.F16, classify=True)
    sess = api.Session(model)
    imgs = mc.pp_images(2, 61, 90, seed=17)
    raw = sess.predict(imgs, classify=classify, layout=api.U8_BGR_HWC)
    pre = np.stack([_host_preprocess(api, 1 if classify else 0, im, model.hparams.patch_size) for im in imgs])
    ref = sess.predict(pre, classify=classify, layout=api.BGR_HWC)
    keys = ("logits", "probs", "cls", "patch_tokens") if classify else ("cls", "patch_tokens")
    for k in keys:
        assert raw.get(k) is not None and ref.get(k) is not None, k
        _ok(mc.check_exact(raw[k], ref[k], k))


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def _layernorm(api, dt, x, w, b, eps):
    rows, H = x.shape
    out = np.zeros((rows, H), np.float32)
    rc = api.lib().dinov2_hip_op_layernorm(dt, _p(x), _p(w), _p(b), _p(out), rows, H, eps)
    assert rc == 0
    return out


_LN_SHAPES = [(r, H) for H in mc.LN_WIDTHS for r in (1, 2, 3, 5, 301)] + [(4097, H) for H in (4, 516, 1024, 2048)]


@pytest.mark.parametrize("dt", [mc.F32, mc.F16, mc.BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("rows,H", _LN_SHAPES, ids=["%dx%d" % s for s in _LN_SHAPES])
def test_layernorm_rounding_points(api, dt, rows, H):
    """Dyadic rows (exact statistics) with full-mantissa w, b: bit-exact against ggml's norm -> mul -> add sequence."""
    x = mc.ln_dyadic_rows(rows, H, seed=rows * 31 + H)
    w, b = mc.ln_affine(H, seed=H)
    _ok(mc.check_exact(_layernorm(api, dt, x, w, b, 1e-6), mc.ln_emulate(x, w, b, 1e-6, dt), "layernorm"))


@pytest.mark.parametrize("dt", [mc.F32, mc.F16, mc.BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("H", [4, 384, 516, 1536, 2048])
def test_layernorm_exact_probes(api, dt, H):
    w, b = mc.ln_affine(H, seed=H + 1)
    rng = np.random.default_rng(H)
    # eps = 0, rows c +- 2: var 4, scale exactly 0.5, v * scale = +-1 -> T(f32(+-w + b))
    c = (rng.integers(-64, 65, size=(3, 1)) / 4.0)
    sign = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    x = (c + 2.0 * sign[None, :]).astype(np.float32)
    exp = mc.round_t(((sign[None, :] * w).astype(np.float32) + b).astype(np.float32), dt)
    _ok(mc.check_exact(_layernorm(api, dt, x, w, b, 0.0), np.broadcast_to(exp, x.shape), "eps = 0, c +- 2"))
    # constant rows: v = 0 -> exactly b
    x = np.broadcast_to(np.array([[0.0], [3.25], [-1e3]], np.float32), (3, H)).copy()
    _ok(mc.check_exact(_layernorm(api, dt, x, w, b, 1e-6), np.broadcast_to(mc.round_t(b, dt), x.shape), "constant rows"))
    # large offset: bit-exact against the emulation and within the derived bound of the float64 LayerNorm
    x = mc.ln_offset_rows(7, H, seed=H + 2)
    got = _layernorm(api, dt, x, w, b, 1e-6)
    _ok(mc.check_exact(got, mc.ln_emulate(x, w, b, 1e-6, dt), "large-offset rows"))
    err = np.abs(got - mc.ln_reference(x, w, b, 1e-6))
    assert (err <= mc.ln_offset_bound(x, w, b, 1e-6, dt)).all(), float(err.max())


@pytest.mark.parametrize("H", [6, 130, 2052, 4096])
def test_layernorm_refuses_unsupported_widths(api, H):
    """H % 4 != 0 and H > 2048: ln_dispatch returns an error before any launch."""
    x = np.ones((2, H), np.float32)
    w, b = np.ones(H, np.float32), np.zeros(H, np.float32)
    out = np.zeros((2, H), np.float32)
    for dt in (mc.F32, mc.F16, mc.BF16):
        assert api.lib().dinov2_hip_op_layernorm(dt, _p(x), _p(w), _p(b), _p(out), 2, H, 1e-6) == -1


# ------------------------------------------------------------------------------------------------------------- head
def _head(api, dt, fin, W, bias, first, inv_div):
    B, T, H = fin.shape
    Cn = W.shape[0]
    feat = np.zeros((B, 2 * H), np.float32)
    logits = np.zeros((B, Cn), np.float32)
    probs = np.zeros((B, Cn), np.float32)
    fin, W, bias = (np.ascontiguousarray(a, np.float32) for a in (fin, W, bias))
    rc = api.lib().dinov2_hip_op_head(dt, _p(fin), _p(W), _p(bias), _p(feat), _p(logits), _p(probs), B, T, H, Cn, first, inv_div)
    assert rc == 0
    return feat, logits, probs


def _head_cases():
    """dtype x H x C, with batch, registers, `first` and the divisor rule rotated through the 32 combinations."""
    cases, i = [], 0
    for dt in (mc.F16, mc.BF16):
        for H in mc.HEAD_H:
            for Cn in mc.HEAD_C:
                B = (1, 3, 64)[i % 3]
                R = (0, 4)[(i // 3) % 2]
                pool_regs = (i // 2) % 2 == 1  # first = 1 (registers pooled, the reference's quirk) or 1 + R
                const_div = i % 2 == 0          # divisor (img / patch)^2 (the reference's quirk) or the pooled count
                cases.append(pytest.param(dt, H, Cn, B, R, pool_regs, const_div,
                                          id="%s-H%d-C%d-B%d-R%d-%s-%s" % (mc.DT_NAME[dt], H, Cn, B, R, "poolregs" if pool_regs else "skipregs",
                                                                         "constdiv" if const_div else "countdiv")))
                i += 1
    return cases


@pytest.mark.parametrize("dt,H,Cn,B,R,pool_regs,const_div", _head_cases())
def test_head(api, dt, H, Cn, B, R, pool_regs, const_div):
    Mg = 4 if B == 64 else 16
    T = 1 + R + Mg * Mg
    first = 1 if pool_regs else 1 + R
    inv_div = 1.0 / (37 * 37 if const_div else T - first)
    fin, W, bias = mc.head_dyadic_case(B, T, H, Cn, R, dt, seed=H + Cn + B + R)
    feat, logits, probs = _head(api, dt, fin, W, bias, first, inv_div)
    _ok(mc.check_exact(feat, mc.head_pool_emulate(fin, first, inv_div, dt), "feat"))
    ref, bound = mc.head_logits_bound(feat, W, bias)
    err = np.abs(logits - ref)
    assert np.isfinite(logits).all() and (err <= bound).all(), "logits: max err %g, bound there %g" % (err.max(), bound.flat[err.argmax()])
    p64, pb = mc.softmax_bound(logits)
    err = np.abs(probs - p64)
    assert np.isfinite(probs).all() and (err <= pb).all(), "probs: max err %g, bound there %g" % (err.max(), pb.flat[err.argmax()])


@pytest.mark.parametrize("dt", [mc.F16, mc.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H", mc.HEAD_H)
@pytest.mark.parametrize("Cn", mc.HEAD_C)
def test_head_exact_probes(api, dt, H, Cn):
    B = 3
    fin, W, bias, first, inv_div = mc.head_exact_logits_case(B, H, Cn, seed=H * 3 + Cn)
    feat, logits, probs = _head(api, dt, fin, W, bias, first, inv_div)
    _ok(mc.check_exact(feat, mc.head_pool_emulate(fin, first, inv_div, dt), "feat"))
    exp = (feat.astype(np.float64) @ W.astype(np.float64).T + bias).astype(np.float32)
    _ok(mc.check_exact(logits, exp, "dyadic logits"))
    # rows of W (and bias) permuted: logits and probs permute bit for bit (|logits| are small: every double sum of expf is exact)
    assert mc.head_logit_spread_ok(logits)
    perm = np.random.default_rng(H + Cn).permutation(Cn)
    f2, l2, p2 = _head(api, dt, fin, W[perm], bias[perm], first, inv_div)
    _ok(mc.check_exact(l2, logits[:, perm], "permuted logits"))
    _ok(mc.check_exact(p2, probs[:, perm], "permuted probs"))
    # images 0 and 2 swapped: their outputs swap
    f3, l3, p3 = _head(api, dt, fin[[2, 1, 0]], W, bias, first, inv_div)
    for a, b_, n in ((f3, feat, "feat"), (l3, logits, "logits"), (p3, probs, "probs")):
        _ok(mc.check_exact(a, b_[[2, 1, 0]], "swapped images: " + n))
    # all-equal logits: exactly f32(1 / C)
    Wc = np.broadcast_to(W[:1], W.shape).copy()
    _, l4, p4 = _head(api, dt, fin, Wc, np.full(Cn, bias[0], np.float32), first, inv_div)
    assert (l4 == l4[:, :1]).all()
    _ok(mc.check_exact(p4, np.full_like(p4, np.float32(1.0) / np.float32(Cn)), "all-equal logits"))
    # one logit 200 above the rest: exactly 1 and 0, no NaN
    b5 = bias.copy()
    b5[Cn // 2] += 200.0
    _, l5, p5 = _head(api, dt, fin, W, b5, first, inv_div)
    exp5 = np.zeros_like(p5)
    exp5[:, Cn // 2] = 1.0
    assert (l5[:, Cn // 2:Cn // 2 + 1] - l5 >= 190).sum() == B * (Cn - 1)
    _ok(mc.check_exact(p5, exp5, "saturated softmax"))


# ------------------------------------------------------------------------------------------------------------- weights
def _convert(api, dt, raw, gt, N, K, Kpad, F=0):
    out = np.zeros((N, Kpad), np.float32)
    buf = (C.c_char * len(raw)).from_buffer_copy(raw)
    assert api.lib().dinov2_hip_op_convert_weight(dt, C.cast(buf, C.c_void_p), len(raw), gt, _p(out), N, K, Kpad, F) == 0
    return out


@pytest.mark.parametrize("dt", [mc.F16, mc.BF16], ids=["to_f16", "to_bf16"])
@pytest.mark.parametrize("tname", mc.CONVERT_TYPES)
@pytest.mark.parametrize("N,K,Kpad,F", [(96, 160, 192, 0), (37, 64, 64, 0), (192, 96, 104, 96)])
def test_convert_weight(api, dt, tname, N, K, Kpad, F):
    """Every source type into both targets, bit-exact against gguf_np.dequantize rounded to nearest even; padding exactly 0;
    interleaveF > 0 against the reshape restatement of the 32-row x1 | x2 interleave."""
    raw, gt, vals = mc.weight_source(tname, N, K, seed=N + K + len(tname))
    got = _convert(api, dt, raw, gt, N, K, Kpad, F)
    _ok(mc.check_exact(got, mc.convert_expected(vals, dt, Kpad, F), "%s -> %s" % (tname, mc.DT_NAME[dt])))


@pytest.mark.parametrize("dt", [mc.F16, mc.BF16], ids=["to_f16", "to_bf16"])
def test_convert_weight_vit_g_ffn_in(api, dt):
    """ViT-g's SwiGLU weights_in (8192 x 1536, F = 4096): 12.6M elements, three passes of the 16384 x 256-thread grid-stride loop."""
    N, K, F = 8192, 1536, 4096
    raw, gt, vals = mc.weight_source("f16", N, K, seed=5)
    got = _convert(api, dt, raw, gt, N, K, K, F)
    _ok(mc.check_exact(got, mc.convert_expected(vals, dt, K, F), "vit-g weights_in"))


@pytest.mark.parametrize("N,F", [(100, 0), (192, 96), (8192, 4096)])
def test_permute_bias(api, N, F):
    """permute_bias_kernel moves the bias as convert_weight moves the weight rows: against the restatement, and against the first
    column of a converted weight whose rows are the bias values (exact in f16)."""
    rng = np.random.default_rng(N)
    src = mc.round_t(rng.standard_normal(N).astype(np.float32), mc.F16)
    dst = np.zeros(N, np.float32)
    assert api.lib().dinov2_hip_op_permute_bias(_p(src), _p(dst), N, F) == 0
    _ok(mc.check_exact(dst, mc.interleave_rows(src, F) if F else src, "bias"))
    wt = np.ascontiguousarray(np.repeat(src[:, None], 32, axis=1))
    got = _convert(api, mc.F16, wt.tobytes(), 0, N, 32, 32, F)
    _ok(mc.check_exact(got[:, 0], dst, "bias vs weight rows"))
