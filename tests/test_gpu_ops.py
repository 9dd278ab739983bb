"""Per-kernel parity on the GPU: each hand-written HIP kernel, called through the C-ABI diagnostic entry points
(include/dinov2_hip_ops.h), against a numpy restatement of the ggml op it replaces."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16, BF16 = 0, 1
EPI_PATCH, EPI_QKV, EPI_RESID, EPI_GELU, EPI_SWIGLU, EPI_PLAIN = range(6)
fp = C.POINTER(C.c_float)


def _p(a):
    return a.ctypes.data_as(fp) if a is not None else fp()


def _round(a, dt):
    a = np.asarray(a, np.float32)
    if dt == F16:
        return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def _gemm(api, dt, epi, A, W, bias, aux, out, M, N, K, ldo, P=0, T=0, R=0, qcols=0, qscale=1.0):
    rc = api.lib().dinov2_hip_op_gemm(dt, epi, _p(A), _p(W), _p(bias), _p(aux), 0 if aux is None else aux.size, _p(out),
                                      out.shape[0], ldo, M, N, K, P, T, R, qcols, qscale)
    assert rc == 0
    return out


def test_tr16_lane_mapping(api):
    """ds_read_b64_tr_b16: lane l of 16-lane group g gets column (l & 15) of the 4x16 block its group addresses."""
    out = np.zeros((64, 4), np.int16)
    assert api.lib().dinov2_hip_op_probe_tr16(out.ctypes.data_as(C.POINTER(C.c_int16))) == 0
    lanes = np.arange(64)
    exp = (64 * (lanes >> 4))[:, None] + 16 * np.arange(4)[None, :] + (lanes & 15)[:, None]
    assert np.array_equal(out, exp), f"unexpected tr16 mapping:\n{out}"


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("M,N,K", [(300, 384, 128), (77, 128, 640), (12300, 1024, 256), (1374, 1000, 192)])
def test_gemm_plain(api, dt, M, N, K):
    """mul_mat(W, x) + bias with asymmetric operands (catches transposed fragments), M/N edge tiles, both tile configs."""
    rng = np.random.default_rng(M + N + K + dt)
    A = _round(rng.standard_normal((M, K)), dt)
    W = _round(rng.standard_normal((N, K)) * 0.1 + np.linspace(-0.2, 0.3, N)[:, None], dt)
    bias = rng.standard_normal(N).astype(np.float32)
    out = np.full((M, N), np.nan, np.float32)
    _gemm(api, dt, EPI_PLAIN, A, W, bias, None, out, M, N, K, N)
    ref = (A.astype(np.float64) @ W.astype(np.float64).T + bias).astype(np.float32)
    assert np.isfinite(out).all()
    np.testing.assert_allclose(out, ref, rtol=2e-5, atol=2e-4)


@pytest.mark.parametrize("dt", [F16, BF16])
def test_gemm_qkv_epilogue(api, dt):
    M, H, K = 500, 128, 128
    rng = np.random.default_rng(1)
    A, W = _round(rng.standard_normal((M, K)), dt), _round(rng.standard_normal((3 * H, K)) * 0.1, dt)
    bias = rng.standard_normal(3 * H).astype(np.float32)
    out = np.zeros((M, 3 * H), np.float32)
    _gemm(api, dt, EPI_QKV, A, W, bias, None, out, M, 3 * H, K, 3 * H, qcols=H, qscale=0.125)
    ref = A.astype(np.float64) @ W.astype(np.float64).T + bias
    ref[:, :H] *= 0.125
    ref = _round(ref.astype(np.float32), dt)
    tol = 2e-3 if dt == F16 else 1.6e-2  # one output ulp
    np.testing.assert_allclose(out, ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("dt", [F16, BF16])
def test_gemm_residual_epilogue(api, dt):
    M, N, K = 700, 256, 512
    rng = np.random.default_rng(2)
    A, W = _round(rng.standard_normal((M, K)), dt), _round(rng.standard_normal((N, K)) * 0.05, dt)
    bias, ls = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    x0 = rng.standard_normal((M, N)).astype(np.float32)
    out = x0.copy()
    _gemm(api, dt, EPI_RESID, A, W, bias, ls, out, M, N, K, N)
    ref = x0 + ls * (A.astype(np.float64) @ W.astype(np.float64).T + bias)
    np.testing.assert_allclose(out, ref.astype(np.float32), rtol=2e-5, atol=2e-4)


@pytest.mark.parametrize("dt", [F16, BF16])
def test_gemm_gelu_epilogue_matches_ggml_f16_lut(api, dt):
    """ggml_gelu = f16 LUT: table[f16(x)] = f16(gelu_tanh(f32(f16(x)))), x <= -10 -> 0, x >= 10 -> x.  The bf16 path keeps the SAME
    f16 table semantics (the table is ggml's, whatever the matmul dtype) and only rounds the table value to bf16 on the way out."""
    M, N, K = 300, 256, 64
    rng = np.random.default_rng(3)
    A = _round(rng.standard_normal((M, K)) * 2.0, dt)
    W = _round(rng.standard_normal((N, K)) * 0.4, dt)
    bias = (rng.standard_normal(N) * 3).astype(np.float32)
    out = np.zeros((M, N), np.float32)
    _gemm(api, dt, EPI_GELU, A, W, bias, None, out, M, N, K, N)
    h = (A.astype(np.float64) @ W.astype(np.float64).T + bias).astype(np.float32)
    xr = h.astype(np.float16).astype(np.float64)
    g = 0.5 * xr * (1 + np.tanh(0.79788456080286535587989211986876 * xr * (1 + 0.044715 * xr * xr)))
    g = g.astype(np.float32).astype(np.float16).astype(np.float32)
    ref = np.where(h <= -10, 0, np.where(h >= 10, h, g)).astype(np.float16).astype(np.float32)
    ref = _round(ref, dt)
    # the f32 pre-activation differs by accumulation order, so f16(x) may flip by one ulp near a rounding boundary (and the bf16
    # rounding of the table value by one bf16 ulp = 2^-8 relative)
    diff = np.abs(out - ref)
    lo, hi = (2e-3, 4e-3) if dt == F16 else (8e-3, 1.6e-2)
    assert (diff > lo * np.maximum(1, np.abs(ref))).mean() < 1e-3
    assert diff.max() <= hi * max(1.0, np.abs(ref).max())
    assert np.abs(h).max() > 10  # the |x| >= 10 branches are exercised
    if dt == BF16:  # every output IS a bf16 value of an f16 table entry: nothing finer than the table survives
        assert np.array_equal(out, _round(out, BF16))


@pytest.mark.parametrize("dt", [F16, BF16])
def test_gemm_swiglu_epilogue(api, dt):
    """weights_in rows interleaved in 32-blocks x1|x2 (done by the loader); out = silu(x1) * x2."""
    M, F, K = 400, 256, 128
    rng = np.random.default_rng(4)
    A = _round(rng.standard_normal((M, K)), dt)
    Win = _round(rng.standard_normal((2 * F, K)) * 0.2, dt)  # [x1 ; x2] like the GGUF tensor
    bin_ = rng.standard_normal(2 * F).astype(np.float32)
    n = np.arange(2 * F)
    src = ((n >> 5) & 1) * F + (n >> 6) * 32 + (n & 31)
    out = np.zeros((M, F), np.float32)
    _gemm(api, dt, EPI_SWIGLU, A, np.ascontiguousarray(Win[src]), np.ascontiguousarray(bin_[src]), None, out, M, 2 * F, K, F)
    h = A.astype(np.float64) @ Win.astype(np.float64).T + bin_
    x1, x2 = h[:, :F], h[:, F:]
    ref = _round((x1 / (1 + np.exp(-x1)) * x2).astype(np.float32), dt)
    tol = 2e-3 if dt == F16 else 1.6e-2
    np.testing.assert_allclose(out, ref, rtol=tol, atol=tol)


def test_gemm_patch_epilogue(api):
    """patch-embed GEMM: + bias + pos_embed[1 + p], scattered to token rows 1 + R + p of each image."""
    B, P, R, H, K = 3, 24, 4, 128, 640
    T = 1 + R + P
    rng = np.random.default_rng(5)
    A, W = _round(rng.standard_normal((B * P, K)), F16), _round(rng.standard_normal((H, K)) * 0.1, F16)
    bias = rng.standard_normal(H).astype(np.float32)
    pos = rng.standard_normal((1 + P, H)).astype(np.float32)
    x = np.full((B * T, H), 7.0, np.float32)
    _gemm(api, F16, EPI_PATCH, A, W, bias, pos, x, B * P, H, K, H, P=P, T=T, R=R)
    ref = np.full((B, T, H), 7.0, np.float32)
    c = (A.astype(np.float64) @ W.astype(np.float64).T + bias).reshape(B, P, H)
    ref[:, 1 + R:] = c + pos[1:]
    np.testing.assert_allclose(x.reshape(B, T, H), ref, rtol=2e-5, atol=2e-4)


def _attn_ref(qkv, B, T, H, nh, dt):
    q, k, v = (qkv.reshape(B, T, 3, nh, 64)[:, :, i].transpose(0, 2, 1, 3).astype(np.float64) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    o = (p / p.sum(-1, keepdims=True)) @ v
    return o.transpose(0, 2, 1, 3).reshape(B * T, H)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("B,T,nh", [(2, 200, 2), (1, 1374, 1), (1, 64, 3), (1, 37, 1), (2, 129, 2), (1, 100, 1), (1, 450, 2), (1, 513, 1)])
def test_attention(api, dt, B, T, nh):
    """soft_max_ext(K^T Q) V per head; T not a multiple of 64 exercises the masked key tail, T % 128 the query tail."""
    H = nh * 64
    rng = np.random.default_rng(T + nh)
    qkv = rng.standard_normal((B * T, 3 * H)).astype(np.float32)
    qkv[:, :H] *= 0.5  # plays the role of the pre-scaled q
    qkv[:, 2 * H:] += np.linspace(-1, 1, H)  # asymmetric V columns
    qkv = _round(qkv, dt)
    out = np.zeros((B * T, H), np.float32)
    assert api.lib().dinov2_hip_op_attention(dt, _p(qkv), _p(out), B, T, H, nh) == 0
    ref = _attn_ref(qkv, B, T, H, nh, dt)
    tol = 3e-3 if dt == F16 else 2.5e-2
    assert np.isfinite(out).all()
    np.testing.assert_allclose(out, ref, rtol=tol, atol=tol)


def test_attention_bitwise_repeatable(api):
    """Same input, four runs, identical bits: a softmax statistic read from MFMA accumulators before the matrix pipeline
    had written them back (an opaque asm reader hides the hazard from the compiler) showed up as run-to-run noise of 2e-4
    that every tolerance-based comparison passed."""
    B, T, nh = 2, 1374, 4
    H = nh * 64
    rng = np.random.default_rng(77)
    qkv = _round(rng.standard_normal((B * T, 3 * H)).astype(np.float32) * 0.7, F16)
    outs = []
    for _ in range(4):
        out = np.zeros((B * T, H), np.float32)
        assert api.lib().dinov2_hip_op_attention(F16, _p(qkv), _p(out), B, T, H, nh) == 0
        outs.append(out)
    assert np.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


@pytest.mark.parametrize("T", [1374, 257, 65])
def test_attention_kernels_agree_bit_for_bit(api, T):
    """The attention kernels (1: 32 queries per wave, 2: software-pipelined for few workgroups, 3: 64 queries per wave, 4:
    software-pipelined with 64 queries per wave and one wave per SIMD) are picked by grid size; an image must not change with the batch it travels in, so all are held to identical bits (same
    summation order, same rescale points).  T = 257 and 65 leave the last wave / the second query block of a wave ragged."""
    B, nh = 1, 3
    H = nh * 64
    rng = np.random.default_rng(5)
    qkv = _round(rng.standard_normal((B * T, 3 * H)).astype(np.float32) * 0.6, F16)
    qkv[T // 2, :H] *= 6.0  # a query with large scores: forces reference-point moves in some tiles
    outs = {}
    try:
        for v in ("1", "2", "3", "4"):
            api.set_tuning("attn_v", int(v))
            out = np.zeros((B * T, H), np.float32)
            assert api.lib().dinov2_hip_op_attention(F16, _p(qkv), _p(out), B, T, H, nh) == 0
            outs[v] = out
        assert np.isfinite(outs["1"]).all()
        assert np.array_equal(outs["1"], outs["2"])
        assert np.array_equal(outs["1"], outs["3"])
        assert np.array_equal(outs["1"], outs["4"])
        # the pipelined kernel's smaller workgroups (64- and 96-query blocks: what a batch-1 forward picks to fill the chip)
        api.set_tuning("attn_v", 2)
        for nwv in (2, 3, 4):
            api.set_tuning("attn_nwv", nwv)
            out = np.zeros((B * T, H), np.float32)
            assert api.lib().dinov2_hip_op_attention(F16, _p(qkv), _p(out), B, T, H, nh) == 0
            assert np.array_equal(outs["1"], out), nwv
    finally:
        api.reset_tuning("attn_v")
        api.reset_tuning("attn_nwv")


def test_attention_online_softmax_rescale(api):
    """Force the running-max update late in the key sequence: one query gets a spike on a key in the LAST tile."""
    B, T, nh, H = 1, 300, 1, 64
    rng = np.random.default_rng(9)
    qkv = (rng.standard_normal((T, 3 * H)) * 0.3).astype(np.float32)
    qkv[5, :H] = 0.0
    qkv[5, 0] = 6.0          # query 5
    qkv[290, H + 0] = 8.0    # key 290 -> score 48 vs O(1) elsewhere
    qkv = _round(qkv, F16)
    out = np.zeros((T, H), np.float32)
    assert api.lib().dinov2_hip_op_attention(F16, _p(qkv), _p(out), B, T, H, nh) == 0
    ref = _attn_ref(qkv, B, T, H, nh, F16)
    np.testing.assert_allclose(out, ref, rtol=3e-3, atol=3e-3)
    np.testing.assert_allclose(out[5], qkv[290, 2 * H:], rtol=2e-3, atol=2e-3)  # query 5 attends key 290 only


@pytest.mark.parametrize("H", [128, 384, 768, 1024, 1536])
def test_layernorm(api, H):
    rows = 301
    rng = np.random.default_rng(H)
    x = (rng.standard_normal((rows, H)) * 3 + rng.standard_normal((rows, 1)) * 5).astype(np.float32)
    w, b = (1 + 0.2 * rng.standard_normal(H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    x64 = x.astype(np.float64)
    mu = x64.mean(-1, keepdims=True)
    ref = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-6) * w + b
    out = np.zeros((rows, H), np.float32)
    assert api.lib().dinov2_hip_op_layernorm(-1, _p(x), _p(w), _p(b), _p(out), rows, H, 1e-6) == 0
    np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-5)
    assert api.lib().dinov2_hip_op_layernorm(F16, _p(x), _p(w), _p(b), _p(out), rows, H, 1e-6) == 0
    np.testing.assert_allclose(out, ref.astype(np.float32).astype(np.float16).astype(np.float32), rtol=1.5e-3, atol=1.5e-3)


@pytest.mark.parametrize("tname", ["f32", "f16", "q8_0", "q4_0", "q4_1", "q5_0", "q5_1"])
def test_convert_weight_dequant(api, pkg, tname):
    """Dequant-on-load kernel vs the oracle's numpy block decoder: bit-exact after the f16 rounding."""
    from oracle import gguf_np as G
    gw = pkg.gguf_writer
    N, K, Kpad = 96, 160, 192
    rng = np.random.default_rng(11)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    gt = gw.NAME_TYPE[tname]
    if tname == "f32":
        raw, ref = w.tobytes(), w
    elif tname == "f16":
        raw, ref = w.astype(np.float16).tobytes(), w.astype(np.float16).astype(np.float32)
    else:
        q = gw.quantize(w, gt)
        raw, ref = q.tobytes(), G.dequantize(q, gt, (N, K))
    out = np.zeros((N, Kpad), np.float32)
    buf = (C.c_char * len(raw)).from_buffer_copy(raw)
    assert api.lib().dinov2_hip_op_convert_weight(F16, C.cast(buf, C.c_void_p), len(raw), gt, _p(out), N, K, Kpad, 0) == 0
    assert np.array_equal(out[:, :K], ref.astype(np.float16).astype(np.float32))
    assert not out[:, K:].any()


@pytest.mark.parametrize("epi", ["plain", "resid", "qkv", "gelu"])
@pytest.mark.parametrize("M,N,K", [(20000, 1024, 512), (43968, 1024, 1024), (9000, 3072, 256), (70000, 256, 128), (33000, 512, 128)])
def test_gemm_persistent_multi_tile(api, epi, M, N, K):
    """The 256x256 persistent kernel with more tiles than CUs: every block walks several tiles, staging the next tile's
    first K-tile during its last phases and under its epilogue.  Whole output checked (a stale-LDS race shows up as a few
    wrong tiles).  K = 128 is the shortest K loop the kernel takes (two K-tiles: the cross-tile staging starts in the
    tile's very first phases)."""
    rng = np.random.default_rng(M + K)
    A = _round(rng.standard_normal((M, K)), F16)
    W = _round(rng.standard_normal((N, K)) * 0.05 + np.linspace(-0.02, 0.03, N)[:, None], F16)
    bias = rng.standard_normal(N).astype(np.float32)
    ref = A @ W.T + bias  # f32 sgemm: same rounding contract, different summation order
    if epi == "plain":
        out = np.full((M, N), np.nan, np.float32)
        _gemm(api, F16, EPI_PLAIN, A, W, bias, None, out, M, N, K, N)
        tol = 2e-4
    elif epi == "resid":
        ls = rng.standard_normal(N).astype(np.float32)
        x0 = rng.standard_normal((M, N)).astype(np.float32)
        out = x0.copy()
        _gemm(api, F16, EPI_RESID, A, W, bias, ls, out, M, N, K, N)
        ref = x0 + ls * ref
        tol = 5e-4
    elif epi == "qkv":
        out = np.zeros((M, N), np.float32)
        _gemm(api, F16, EPI_QKV, A, W, bias, None, out, M, N, K, N, qcols=N // 4 * 2 if N % 512 == 0 else 256, qscale=0.125)
        qc = N // 4 * 2 if N % 512 == 0 else 256
        ref[:, :qc] *= 0.125
        ref = _round(ref, F16)
        tol = 2e-3
    else:
        out = np.zeros((M, N), np.float32)
        _gemm(api, F16, EPI_GELU, A, W, bias, None, out, M, N, K, N)
        xr = ref.astype(np.float16).astype(np.float64)
        g = 0.5 * xr * (1 + np.tanh(0.79788456080286535587989211986876 * xr * (1 + 0.044715 * xr * xr)))
        ref = g.astype(np.float32).astype(np.float16).astype(np.float32)
        tol = 2e-3
    assert np.isfinite(out).all()
    bad = np.abs(out - ref) > tol * np.maximum(1.0, np.abs(ref))
    assert bad.mean() < (1e-4 if epi == "gelu" else 1e-7), f"{bad.sum()} mismatches, first at {np.argwhere(bad)[:4]}"


@pytest.mark.parametrize("name,epi,N", [("plain", EPI_PLAIN, 1024), ("qkv", EPI_QKV, 3072), ("gelu", EPI_GELU, 4096),
                                        ("gelu_small_tile", EPI_GELU, 384), ("resid", EPI_RESID, 1024)])
def test_gemm_rows_do_not_depend_on_their_position(api, name, epi, N):
    """A = [X; Y; X]: both X blocks must produce bit-identical outputs (B images == B independent forwards).  Caught a
    real defect: hipcc fused 'add bias, round to f16' into v_fma_mixlo_f16 (single rounding) for some unrolled epilogue
    instances only, so one element in ~1e5 depended on the row's lane."""
    rng = np.random.default_rng(7)
    T, K = 1374, 1024
    X = _round(rng.standard_normal((T, K)), F16)
    Y = _round(rng.standard_normal((T, K)), F16)
    A = np.ascontiguousarray(np.concatenate([X, Y, X]))
    W = _round(rng.standard_normal((N, K)) * 0.05, F16)
    bias, aux = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    out = np.zeros((3 * T, N), np.float32)
    _gemm(api, F16, epi, A, W, bias, aux, out, 3 * T, N, K, N, qcols=N // 3, qscale=0.125)
    assert np.array_equal(out[:T], out[2 * T:])


@pytest.mark.parametrize("name,epi,N,K", [("qkv", EPI_QKV, 3072, 1024), ("gelu", EPI_GELU, 4096, 1024), ("resid", EPI_RESID, 1024, 1024),
                                          ("resid_k4096", EPI_RESID, 1024, 4096)])
def test_gemm_small_and_large_m_agree_bit_for_bit(api, name, epi, N, K):
    """One image (M = 1374: 128-row one-tile-per-workgroup plan for QKV / FFN-in, 64x128 few-tile plan for the N = hidden GEMMs) against
    the same rows inside a batch of 32 (M = 43968: the persistent 256x256 kernel): identical bits, so a token's result does not depend
    on the batch it arrives in."""
    rng = np.random.default_rng(11)
    T = 1374
    X = _round(rng.standard_normal((T, K)), F16)
    W = _round(rng.standard_normal((N, K)) * 0.05, F16)
    bias, aux = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    x0 = rng.standard_normal((T, N)).astype(np.float32) if epi == EPI_RESID else np.zeros((T, N), np.float32)
    small = x0.copy()
    _gemm(api, F16, epi, X, W, bias, aux, small, T, N, K, N, qcols=N // 3, qscale=0.125)
    big = np.ascontiguousarray(np.tile(x0, (32, 1)))
    _gemm(api, F16, epi, np.ascontiguousarray(np.tile(X, (32, 1))), W, bias, aux, big, 32 * T, N, K, N, qcols=N // 3, qscale=0.125)
    assert np.array_equal(big[:T], small) and np.array_equal(big[-T:], small)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("epi,N,K,Ms", [(EPI_QKV, 3072, 1024, (100, 261, 783, 1374, 2088, 4122, 9000)),
                                        (EPI_RESID, 1024, 1024, (100, 261, 1374, 4122, 5496, 9000)),
                                        (EPI_GELU, 3072, 768, (261, 1374, 2748)), (EPI_RESID, 768, 3072, (261, 1374, 4122))])
def test_gemm_every_plan_gives_a_row_the_same_bits(api, dt, epi, N, K, Ms):
    """launch_gemm picks a plan by shape: small tiles of 32x64, 64x64, 64x128 (few-tile plans), 64x128 / 128x128 with co-resident
    workgroups, 128-row one-tile-per-workgroup tiles, 192- and 256-row persistent tiles and mixtures of them.  The same 100 rows put
    through launches of 100 ... 9 000 rows (every plan at least once) must come out with the same bits every time."""
    rng = np.random.default_rng(N + K + dt)
    X = _round(rng.standard_normal((100, K)), dt)
    W = _round(rng.standard_normal((N, K)) * 0.05, dt)
    bias, aux = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    x0 = rng.standard_normal((100, N)).astype(np.float32) if epi == EPI_RESID else np.zeros((100, N), np.float32)
    ref = None
    for M in Ms:
        reps = (M + 99) // 100
        A = np.ascontiguousarray(np.tile(X, (reps, 1))[:M])
        out = np.ascontiguousarray(np.tile(x0, (reps, 1))[:M])
        _gemm(api, dt, epi, A, W, bias, aux, out, M, N, K, N, qcols=N // 3, qscale=0.125)
        if ref is None:
            ref = out[:100].copy()
            assert np.isfinite(ref).all()
        assert np.array_equal(out[:100], ref), M
        if M >= 200:
            assert np.array_equal(out[M - M % 100 - 100:M - M % 100], ref), M  # the last whole copy of the rows: another tile, the same bits


def test_gemm_swiglu_small_and_large_m_agree_bit_for_bit(api):
    """SwiGLU epilogue: one image on the small-tile kernel vs the same rows inside 32 images on the persistent kernel with
    its mixed 256/192-row schedule (5.4 rounds of tiles): identical bits."""
    rng = np.random.default_rng(12)
    T, K, F = 1374, 1024, 1024
    X = _round(rng.standard_normal((T, K)), F16)
    W = _round(rng.standard_normal((2 * F, K)) * 0.05, F16)
    bias = rng.standard_normal(2 * F).astype(np.float32)
    small = np.zeros((T, F), np.float32)
    _gemm(api, F16, EPI_SWIGLU, X, W, bias, None, small, T, 2 * F, K, F)
    big = np.zeros((32 * T, F), np.float32)
    _gemm(api, F16, EPI_SWIGLU, np.ascontiguousarray(np.tile(X, (32, 1))), W, bias, None, big, 32 * T, 2 * F, K, F)
    assert np.isfinite(small).all()
    assert np.array_equal(big[:T], small) and np.array_equal(big[-T:], small)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("N,K,epi,qcols", [(1152, 384, EPI_QKV, 384), (384, 384, EPI_RESID, 0), (384, 1536, EPI_RESID, 0), (1152, 384, EPI_PLAIN, 0)])
def test_gemm_n_split_vit_s_shapes(api, N, K, epi, qcols, dt):
    """N not a multiple of 256 (ViT-S: hidden 384, QKV 1 152): at large M the leading multiple of 256 columns goes to the persistent
    kernel and the rest to the small-tile kernel (two launches).  The same rows at small M take the small-tile kernel alone: every
    row must come out with the same bits (q | k | v boundaries at multiples of 64 inside a 256-column tile included), and the whole
    output must match float64."""
    T, reps = 700, 40
    rng = np.random.default_rng(N + K + epi)
    X = _round(rng.standard_normal((T, K)), dt)
    W = _round(rng.standard_normal((N, K)) * 0.06, dt)
    bias, ls = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    x0 = rng.standard_normal((T, N)).astype(np.float32)
    small = x0.copy() if epi == EPI_RESID else np.zeros((T, N), np.float32)
    _gemm(api, dt, epi, X, W, bias, ls if epi == EPI_RESID else None, small, T, N, K, N, qcols=qcols, qscale=0.125)
    big = np.ascontiguousarray(np.tile(x0, (reps, 1))) if epi == EPI_RESID else np.zeros((reps * T, N), np.float32)
    _gemm(api, dt, epi, np.ascontiguousarray(np.tile(X, (reps, 1))), W, bias, ls if epi == EPI_RESID else None, big, reps * T, N, K, N,
          qcols=qcols, qscale=0.125)
    for r in (0, 17, reps - 1):
        assert np.array_equal(big[r * T:(r + 1) * T], small), r
    ref = X.astype(np.float64) @ W.astype(np.float64).T + bias
    if epi == EPI_QKV:
        ref[:, :qcols] *= 0.125
        np.testing.assert_allclose(small, _round(ref.astype(np.float32), dt), rtol=2e-3 if dt == F16 else 1.6e-2, atol=2e-3 if dt == F16 else 1.6e-2)
    elif epi == EPI_RESID:
        np.testing.assert_allclose(small, (x0 + ls * ref).astype(np.float32), rtol=2e-5, atol=3e-4)
    else:
        np.testing.assert_allclose(small, ref.astype(np.float32), rtol=2e-5, atol=3e-4)


@pytest.mark.parametrize("seed", range(14))
def test_gemm_random_shapes_all_plans(api, seed):
    """Random (M, N, K, epilogue) over the whole range the dispatcher sees -- one image to 50 images, every hidden size of the
    DINOv2 family, odd and even K / 64 -- so that every kernel plan (256-row, 192-row, mixed, small-tile tail, small-tile only)
    and every ragged edge is exercised against a float32 reference; whole output checked."""
    rng = np.random.default_rng(1000 + seed)
    M = int(rng.choice([1, 37, 1374, 2748, 4122, 5496, 10992, 21984, 32976, 43968, 51000, 68700])) + int(rng.integers(0, 3)) * int(rng.integers(0, 200))
    N = int(rng.choice([256, 384, 768, 1024, 1152, 1536, 2304, 3072, 4096]))
    K = int(rng.choice([128, 192, 384, 640, 768, 1024, 1536]))
    epi = [EPI_PLAIN, EPI_RESID, EPI_GELU, EPI_QKV][seed % 4]
    if M * N * K > 6e10:
        M = max(1, int(6e10 / (N * K)))
    A = _round(rng.standard_normal((M, K)), F16)
    W = _round(rng.standard_normal((N, K)) * 0.06, F16)
    bias, aux = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    ref = A @ W.T + bias
    if epi == EPI_PLAIN:
        out = np.full((M, N), np.nan, np.float32)
        tol = 3e-4
    elif epi == EPI_RESID:
        x0 = rng.standard_normal((M, N)).astype(np.float32)
        out = x0.copy()
        ref = x0 + aux * ref
        tol = 6e-4
    elif epi == EPI_GELU:
        out = np.zeros((M, N), np.float32)
        xr = ref.astype(np.float16).astype(np.float64)
        ref = (0.5 * xr * (1 + np.tanh(0.79788456080286535587989211986876 * xr * (1 + 0.044715 * xr * xr)))).astype(np.float32)
        ref = ref.astype(np.float16).astype(np.float32)
        tol = 2e-3
    else:
        out = np.zeros((M, N), np.float32)
        ref[:, :N // 2] *= 0.125
        ref = _round(ref, F16)
        tol = 2e-3
    _gemm(api, F16, epi, A, W, bias, aux, out, M, N, K, N, qcols=N // 2, qscale=0.125)
    assert np.isfinite(out).all()
    bad = np.abs(out - ref) > tol * np.maximum(1.0, np.abs(ref))
    assert bad.mean() < (2e-4 if epi in (EPI_GELU, EPI_QKV) else 1e-7), f"M={M} N={N} K={K}: {bad.sum()} mismatches, first at {np.argwhere(bad)[:4]}"




def _gen_case(api, rng, dt, epi, M, N, K, gens, expect):
    """One shape through the listed generations of the persistent GEMM (`expect[gen]` = a kernel name the dispatcher's plan for that
    generation must contain, so that the comparison provably runs the kernels it claims to -- ADVICE r4); the rows repeat every 100, so
    the small-tile kernel's rows (M = 100) are the reference bits for every tile position."""
    Nout = N // 2 if epi == EPI_SWIGLU else N
    X = _round(rng.standard_normal((100, K)), dt)
    A = np.ascontiguousarray(np.tile(X, ((M + 99) // 100, 1))[:M])
    W = _round(rng.standard_normal((N, K)) * 0.05, dt)
    bias, aux = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    x0 = rng.standard_normal((100, Nout)).astype(np.float32) if epi == EPI_RESID else np.zeros((100, Nout), np.float32)
    x0 = np.ascontiguousarray(np.tile(x0, ((M + 99) // 100, 1))[:M])
    outs = {}
    try:
        for gen in gens:
            api.set_tuning("gemm_gen", gen)
            plan = api.gemm_plan(dt, epi, M, N, K)
            assert expect[gen] in plan, (gen, M, N, K, plan)
            out = x0.copy()
            _gemm(api, dt, epi, A, W, bias, aux if epi == EPI_RESID else None, out, M, N, K, Nout, qcols=N // 4, qscale=0.125)
            outs[gen] = out
    finally:
        api.reset_tuning("gemm_gen")
    first = outs[gens[0]]
    assert np.isfinite(first).all()
    for gen in gens[1:]:
        assert np.array_equal(first, outs[gen]), (gen, M, N, K)
    small = x0[:100].copy()
    _gemm(api, dt, epi, X, W, bias, aux if epi == EPI_RESID else None, small, 100, N, K, Nout, qcols=N // 4, qscale=0.125)
    assert np.array_equal(small, first[:100]), (M, N, K)
    last = M - 100 - M % 100
    assert np.array_equal(small, first[last:last + 100]), (M, N, K)  # the last whole copy: another tile height / a ragged panel
    mid = (M // 200) * 100
    assert np.array_equal(small, first[mid:mid + 100]), (M, N, K)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("epi", [EPI_QKV, EPI_RESID, EPI_GELU, EPI_SWIGLU, EPI_PLAIN])
def test_gemm_generation_4_equals_generation_2_bit_for_bit(api, dt, epi):
    """gemm4.hip (four waves, accumulators in AGPRs, hand-ordered K loop) against gemm2.hip (eight waves, barrier-separated sections) on
    the SAME plans, each asserted by name through dinov2_hip_op_gemm_plan:
      * plan A with more tiles than workgroups and a ragged last panel (98 200 x 512: 384 x 2 = 768 tiles of 256 rows: three rounds, the
        `has_next` cross-tile staging of gemm4.hip, the last panel 152 rows) -- K / 64 = 4;
      * plan C, two whole rounds of 256-row tiles + a round of 192-row tiles in one launch (gemm4_mixed_kernel, NI = 8 then 6), ragged
        last panel -- K / 64 = 6;
      * plan D, one whole round + the small-tile tail -- K / 64 = 16;
      * at M = 1 374 the short one-tile-per-workgroup launches (NI = 3 at N = 3 072 / 4 096) for the 2-byte epilogues.
    Every output bit must agree (same MFMA, same K order, same epilogue expressions), and the small-tile kernel's rows (M = 100) must be
    those bits too."""
    rng = np.random.default_rng(40 + epi + dt)
    _gen_case(api, rng, dt, epi, 98200, 512, 256, (2, 4), {2: "gemm2<256>", 4: "gemm4<256>"})
    assert ";" not in api.gemm_plan(dt, epi, 98200, 512, 256)
    _gen_case(api, rng, dt, epi, 41100, 1024, 384, (2, 4), {2: "gemm2_mixed<256+192>", 4: "gemm4_mixed<256+192>"})
    _gen_case(api, rng, dt, epi, 9300, 2048, 1024, (2, 4), {2: "gemm2<256>;small", 4: "gemm4<256>;small"})
    if epi in (EPI_QKV, EPI_GELU, EPI_SWIGLU):
        for N in (3072, 4096):
            _gen_case(api, rng, dt, epi, 1374, N, 1024, (2, 4), {2: "gemm2<128>", 4: "gemm4_short<96>"})


@pytest.mark.parametrize("gen,M,N,K,name", [(4, 41100, 1024, 1024, "gemm4_mixed<256+192>"), (4, 98200, 512, 256, "gemm4<256>")])
def test_gemm_generation_race_screen(api, gen, M, N, K, name):
    """Fifty repeats of a multi-round launch of the hand-ordered kernels (gemm4.hip: plan C, 256- and 192-row tiles, next tile staged under
    the last K-tiles and the epilogue; plan A with four rounds) must reproduce the first
    result bit for bit: a fragment read ahead of its LDS-DMA data, or a buffer re-staged under a reader, shows up as a rare differing
    tile.  The generation is forced and the plan asserted by name (the round-4 form of this test ran gemm2.hip)."""
    rng = np.random.default_rng(77)
    A = _round(rng.standard_normal((M, K)), F16)
    W = _round(rng.standard_normal((N, K)) * 0.05, F16)
    bias = rng.standard_normal(N).astype(np.float32)
    try:
        api.set_tuning("gemm_gen", gen)
        assert name in api.gemm_plan(F16, EPI_PLAIN, M, N, K)
        ref = np.zeros((M, N), np.float32)
        _gemm(api, F16, EPI_PLAIN, A, W, bias, None, ref, M, N, K, N)
        exp = (A[:256].astype(np.float64) @ W.astype(np.float64).T + bias)
        np.testing.assert_allclose(ref[:256], exp, rtol=2e-5, atol=3e-4)
        np.testing.assert_allclose(ref[-200:], A[-200:].astype(np.float64) @ W.astype(np.float64).T + bias, rtol=2e-5, atol=3e-4)
        out = np.zeros_like(ref)
        for _ in range(50 if M < 100000 else 20):
            out[:] = 0
            _gemm(api, F16, EPI_PLAIN, A, W, bias, None, out, M, N, K, N)
            assert np.array_equal(out, ref)
    finally:
        api.reset_tuning("gemm_gen")


# ---- exhaustive sweeps of the activation epilogues -------------------------------------------------------------------
def _all_finite_f16():
    bits = np.concatenate([np.arange(0x0000, 0x7C00, dtype=np.uint16), np.arange(0x8000, 0xFC00, dtype=np.uint16)])
    return bits.view(np.float16).astype(np.float32)  # 63 488 values, both zeros included


def _f16_ulps(a, b):
    """distance in f16 representable steps between two arrays of f16-valued floats (monotone integer mapping of the bit patterns)"""
    def key(x):
        u = np.asarray(x, np.float32).astype(np.float16).view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.abs(key(a) - key(b))


def _record_sweep(name, **vals):
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "activation_sweeps_r06.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        cur = json.load(open(path)) if os.path.exists(path) else {}
        cur[name] = vals
        json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _identity_operands(x, dt, N, ncols_x):
    """A [M, 64], W [N, 64] with A @ W.T == x (exactly, in f32) in the first `ncols_x` columns pattern given by the caller: x is split
    into parts the compute dtype holds exactly (f16: x itself; bf16: hi + lo, 8 + 3 significant bits), each multiplied by a 1."""
    M = x.size
    A = np.zeros((M, 256), np.float32)  # K = 256: four K-tiles, the least the persistent kernels take; all but the first columns zero
    if dt == F16:
        A[:, 0] = x
        nparts = 1
    else:
        hi = _round(x, BF16)
        lo = x - hi
        assert np.array_equal(_round(lo, BF16), lo)
        A[:, 0], A[:, 1] = hi, lo
        nparts = 2
    return A, nparts


_IMPLS = {"small": ("gemm_tile", 128, "small<"), "gemm2": ("gemm_gen", 2, "gemm2<"), "gemm4": ("gemm_gen", 4, "gemm4<")}


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("impl", list(_IMPLS))
def test_gelu_epilogue_exhaustive_f16_table(api, dt, impl):
    """EVERY finite f16 value (63 488 of them) through the GELU epilogue with a pre-activation that IS that value (K = 64, one-hot
    operands, zero bias), against ggml's table semantics restated in float64: table[h] = f16(gelu_tanh(h)) for |h| < 10, 0 for h <= -10,
    h for h >= 10 (ggml_gelu_f32; /root/reference/dinov2.cpp:567).  The epilogue evaluates the tanh form with v_exp_f32 / v_rcp_f32
    (1 ulp approximations), so an entry can differ from the exactly rounded table where the exact value lies within that error of an f16
    rounding boundary: the test COUNTS those entries, bounds them (<= 1 f16 ulp each) and records the counts in
    gpurun_out/activation_sweeps_r06.json -- against the correctly rounded table AND against ggml's own f32-built table (the oracle's).  All three epilogue implementations (small-tile kernel, gemm2 / gemm4.hip) are
    swept, each forced and asserted by plan name."""
    x = _all_finite_f16()
    N = 256
    A, nparts = _identity_operands(x, dt, N, N)
    W = np.zeros((N, 256), np.float32)
    W[:, :nparts] = 1.0
    out = np.zeros((x.size, N), np.float32)
    key, val, name = _IMPLS[impl]
    try:
        api.set_tuning(key, val)
        plan = api.gemm_plan(dt, EPI_GELU, x.size, N, 256)
        assert plan.startswith(name), plan
        _gemm(api, dt, EPI_GELU, A, W, None, None, out, x.size, N, 256, N)
    finally:
        api.reset_tuning(key)
    assert (out == out[:, :1]).all()  # every column computed the same function of the same value
    got = out[:, 0]
    xd = x.astype(np.float64)
    g = 0.5 * xd * (1 + np.tanh(0.79788456080286535587989211986876 * xd * (1 + 0.044715 * xd * xd)))
    table = np.where(xd <= -10, 0.0, np.where(xd >= 10, xd, g)).astype(np.float16).astype(np.float32)
    # ggml builds its table in f32 with the C library's tanhf (ggml.c): the oracle exports exactly that table (oracle_gelu_table).  It is
    # itself NOT the correctly rounded one: 274 of its 37 376 entries with |h| < 10 differ from f16(gelu_tanh in double) (f32 rounding of
    # 1 + tanhf(u) and of the products, measured on this image's glibc), so "ggml's table bit for bit" is not a well-defined target across
    # hosts; the HIP epilogue is held to BOTH: <= 1 f16 ulp from either, a handful of entries off the correctly rounded table.
    from oracle import oracle as _oracle
    tab = _oracle.gelu_table().view(np.float16).astype(np.float32)
    idx = x.astype(np.float16).view(np.uint16)
    table32 = np.where(xd <= -10, np.float32(0), np.where(xd >= 10, x, tab[idx])).astype(np.float32)
    exp = _round(table, dt)
    exp32 = _round(table32, dt)
    ulps = _f16_ulps(got, exp) if dt == F16 else np.where(got == exp, 0, 1)
    ulps32 = _f16_ulps(got, exp32) if dt == F16 else np.where(got == exp32, 0, 1)
    nbad = int((got != exp).sum())
    nbad32 = int((got != exp32).sum())
    _record_sweep(f"gelu_{'f16' if dt == F16 else 'bf16'}_{impl}", plan=plan, entries=int(x.size), mismatches_vs_f64_table=nbad,
                  mismatches_vs_ggml_f32_table=nbad32, ggml_f32_table_vs_f64_table=int((table != table32).sum()), max_f16_ulps_vs_f64_table=int(ulps.max()),
                  max_f16_ulps_vs_ggml_f32_table=int(ulps32.max()), inputs_off_the_f64_table=[float(v) for v in x[got != exp][:8]])
    assert np.isfinite(got).all()
    assert ulps.max() <= 1, (nbad, x[ulps > 1][:8])
    assert nbad <= 8, nbad      # measured: 5 (f16) / 1 (bf16) of 63 488 entries one step off the correctly rounded table
    assert ulps32.max() <= 2 and nbad32 <= 400, (nbad32, int(ulps32.max()))  # measured: as many as ggml's own table is off the correctly rounded one


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("impl", list(_IMPLS))
def test_swiglu_epilogue_exhaustive_silu(api, dt, impl):
    """Every finite f16 value through silu(x1) * x2 with x2 == 1 (the SwiGLU epilogue; ggml_silu_f32 = x / (1 + expf(-x)),
    /root/reference/dinov2.cpp:605): the T-rounded result against float64, at most one output ulp (f16: 2^-11, bf16: 2^-8 relative) anywhere."""
    x = _all_finite_f16()
    F = 128
    A, nparts = _identity_operands(x, dt, 2 * F, F)
    # interleaved weights_in rows: 32 x1 units, then the 32 x2 units of the same hidden columns
    W = np.zeros((2 * F, 256), np.float32)
    bias = np.zeros(2 * F, np.float32)
    n = np.arange(2 * F)
    is_x2 = ((n >> 5) & 1) == 1
    W[~is_x2, :nparts] = 1.0
    bias[is_x2] = 1.0
    out = np.zeros((x.size, F), np.float32)
    key, val, name = _IMPLS[impl]
    try:
        api.set_tuning(key, val)
        plan = api.gemm_plan(dt, EPI_SWIGLU, x.size, 2 * F, 256)
        assert plan.startswith(name), plan
        _gemm(api, dt, EPI_SWIGLU, A, W, bias, None, out, x.size, 2 * F, 256, F)
    finally:
        api.reset_tuning(key)
    assert (out == out[:, :1]).all()
    got = out[:, 0].astype(np.float64)
    xd = x.astype(np.float64)
    with np.errstate(over="ignore"):
        ref = xd / (1 + np.exp(-xd))
    exp = _round(ref.astype(np.float32), dt).astype(np.float64)
    rel = 2.0 ** -11 if dt == F16 else 2.0 ** -8
    err = np.abs(got - ref)
    tol = rel * np.maximum(np.abs(ref), 2.0 ** -14) + 2.0 ** -24  # one output ulp (f16 subnormal spacing at the bottom)
    nbad = int((got != exp).sum())
    _record_sweep(f"silu_{'f16' if dt == F16 else 'bf16'}_{impl}", plan=plan, entries=int(x.size), not_correctly_rounded=nbad,
                  worst_err_over_ulp=float((err / tol).max()))
    assert np.isfinite(got).all()
    assert (err <= tol).all(), x[err > tol][:8]


# ---- every kernel plan the model family can reach, held to the small-tile kernel's bits (tests/gemm_plan_cases.py) ----
from gemm_plan_cases import COVERAGE_CASES  # noqa: E402


@pytest.mark.parametrize("case", COVERAGE_CASES, ids=lambda c: "dt%d-epi%d-%dx%dx%d" % c)
def test_gemm_plan_coverage_case_bits(api, case):
    """One problem per reachable (kernel, epilogue, dtype) of the dispatcher (the list is generated from the library's own plan query and
    checked for completeness on the CPU by tests/test_gemm_plans.py).  The launch under the plan the dispatcher picks must agree BIT FOR
    BIT (a) over the whole output with the same problem forced onto the plain 128 x 128 / 64 x 128 small-tile kernel
    (dinov2_hip_op_set_tuning("gemm_tile", 128)), and (b) -- the rows repeat every 100 -- with a 100-row launch of the same rows (few-tile
    plans: 32 x 64 tiles), so that a token's bits depend neither on the plan nor on the batch it travels in."""
    gemm_plan_case_bits(api, case)


def gemm_plan_case_bits(api, case):
    """The body of test_gemm_plan_coverage_case_bits, shared with tests/test_gpu_geometry.py (GEOMETRY_COVERAGE_CASES).  A problem of fewer than
    100 rows (the off-family sweep has them) is the head of the 100-row launch instead: its rows must carry that launch's bits (where both
    launches get the same configuration, as those cases do, this shows that a row's bits do not depend on M, nothing more)."""
    dt, epi, M, N, K = case
    rng = np.random.default_rng(M + 3 * N + 7 * K + 11 * epi + dt)
    Nout = N // 2 if epi == EPI_SWIGLU else N
    X = _round(rng.standard_normal((100, K)), dt)
    A = np.ascontiguousarray(np.tile(X, ((M + 99) // 100, 1))[:M])
    W = _round(rng.standard_normal((N, K)) * 0.05, dt)
    bias, aux = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    kw = dict(qcols=N // 3, qscale=0.125)
    if epi == EPI_PATCH:
        P = 1369 if M % 1369 == 0 else 256 if M % 256 == 0 else M
        B, R = M // P, 4
        T = P + 1 + R
        pos = rng.standard_normal((1 + P, N)).astype(np.float32)
        x0 = rng.standard_normal((B * T, N)).astype(np.float32)
        kw.update(P=P, T=T, R=R)
        auxv, ldo = pos, N
    else:
        x100 = rng.standard_normal((100, Nout)).astype(np.float32) if epi == EPI_RESID else np.zeros((100, Nout), np.float32)
        x0 = np.ascontiguousarray(np.tile(x100, ((M + 99) // 100, 1))[:M])
        auxv, ldo = (aux if epi == EPI_RESID else None), Nout
    plan = api.gemm_plan(dt, epi, M, N, K)
    out = x0.copy()
    _gemm(api, dt, epi, A, W, bias, auxv, out, M, N, K, ldo, **kw)
    assert np.isfinite(out).all()
    try:
        api.set_tuning("gemm_tile", 128)
        forced_plan = api.gemm_plan(dt, epi, M, N, K)
        assert forced_plan.startswith("small<"), forced_plan
        ref = x0.copy()
        _gemm(api, dt, epi, A, W, bias, auxv, ref, M, N, K, ldo, **kw)
    finally:
        api.reset_tuning("gemm_tile")
    assert np.array_equal(out, ref), (plan, forced_plan)
    if epi != EPI_PATCH and M > 100:
        small = x0[:100].copy()
        _gemm(api, dt, epi, X, W, bias, auxv, small, 100, N, K, ldo, **kw)
        assert np.array_equal(small, out[:100]), (plan, "rows 0..99")
        last = M - 100 - M % 100
        assert np.array_equal(small, out[last:last + 100]), (plan, "last whole copy of the rows")
    elif epi != EPI_PATCH and M < 100:
        whole = x100.copy()
        _gemm(api, dt, epi, X, W, bias, auxv, whole, 100, N, K, ldo, **kw)
        assert np.array_equal(whole[:M], out), (plan, api.gemm_plan(dt, epi, 100, N, K), "the rows inside a 100-row launch")
    elif epi == EPI_PATCH and M < 100:  # the same image eight times over (another tile grid): every copy's token rows carry the single launch's bits
        x8 = np.ascontiguousarray(np.tile(x0, (8, 1)))
        _gemm(api, dt, epi, np.ascontiguousarray(np.tile(A, (8, 1))), W, bias, auxv, x8, 8 * M, N, K, ldo, **kw)
        assert np.array_equal(x8, np.tile(out, (8, 1))), (plan, api.gemm_plan(dt, epi, 8 * M, N, K), "the image inside a batch of eight")


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("B,Hh,Ww,ps", [(2, 518, 518, 14), (1, 224, 224, 14), (3, 70, 98, 14), (1, 490, 868, 14), (2, 64, 83, 16), (1, 14, 14, 14),
                                        (1, 1, 1, 1), (2, 3, 23, 1), (1, 4, 22, 2), (2, 9, 33, 3), (1, 7, 31, 3), (1, 8, 44, 4), (1, 10, 55, 5),
                                        (1, 12, 60, 6), (3, 14, 147, 7)])
def test_im2col_bit_exact(api, dt, layout, B, Hh, Ww, ps):
    """im2col of ggml_conv_2d_sk_p0 (/root/reference/dinov2.cpp:636; BGR-interleaved input: the repack of :914-931 folded in): every element
    of [B * P, Kpad] equals the compute-type rounding of its pixel, k = c * ps^2 + ky * ps + kx with c the RGB index, zero in the K padding --
    square, non-square, several chunks per patch row (868 wide: 62 patches), widths that are no multiple of the patch size, one patch; and
    every patch size 1 .. 7 (3 p^2 = 3 .. 147 real columns of Kpad 64, 64, 64, 64, 128, 128, 192: one pixel, chunks of 10 + 10 + 3, 10 + 1 and
    exactly 10 patches, patch 3 = the channel count, a width that is no multiple of patch 3)."""
    rng = np.random.default_rng(B * 1000 + Ww)
    Kpad = (3 * ps * ps + 63) // 64 * 64
    rgb = (rng.standard_normal((B, 3, Hh, Ww)) * 1.5).astype(np.float32)
    img = rgb if layout == 1 else np.ascontiguousarray(rgb[:, ::-1].transpose(0, 2, 3, 1))  # BGR interleaved
    h0, w0 = Hh // ps, Ww // ps
    col = np.full((B * h0 * w0, Kpad), np.nan, np.float32)
    assert api.lib().dinov2_hip_op_im2col(dt, _p(img), _p(col), B, Hh, Ww, ps, Kpad, layout) == 0
    ref = np.zeros((B, h0, w0, Kpad), np.float32)
    patches = rgb[:, :, :h0 * ps, :w0 * ps].reshape(B, 3, h0, ps, w0, ps).transpose(0, 2, 4, 1, 3, 5).reshape(B, h0, w0, 3 * ps * ps)
    ref[..., :3 * ps * ps] = _round(patches, dt)
    assert np.array_equal(col, ref.reshape(B * h0 * w0, Kpad))
