"""The attention instances the forward launches, held to exact probes and to a float64 reference within a derived bound.

The forward scales q by log2(e)/8 in the QKV epilogue and runs attention with log2_scores = 1 (csrc/model.cpp); those are other template
instances (exp2, THR 8) than the natural-exp ones dinov2_hip_op_attention reaches.  dinov2_hip_op_attention_ex takes the flag, and
every case here runs both domains, both dtypes and every kernel variant (tests/attention_cases.py: VARIANTS), through a device
output framed by NaN-filled guard rows (a nonzero return = a guard byte changed).  Helpers, bound and probes: tests/attention_cases.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import attention_cases as ac

pytestmark = pytest.mark.gpu

fp = C.POINTER(C.c_float)
EPI_QKV = 1


def _p(a):
    return a.ctypes.data_as(fp)


def _attention(api, dt, qkv, B, T, nh, log2, variant="auto"):
    v, nw = ac.VARIANTS[variant]
    H = nh * 64
    qkv = np.ascontiguousarray(qkv, np.float32)
    out = np.zeros((B * T, H), np.float32)
    try:
        api.set_tuning("attn_v", v)
        api.set_tuning("attn_nwv", nw)
        rc = api.lib().dinov2_hip_op_attention_ex(dt, _p(qkv), _p(out), B, T, H, nh, int(log2))
    finally:
        api.reset_tuning("attn_v")
        api.reset_tuning("attn_nwv")
    assert rc != api.OP_GUARD_CHANGED, "attention wrote outside its output rows (guard band changed)"
    assert rc == 0, "dinov2_hip_op_attention_ex failed (%d)" % rc
    return out


# inputs, references and bounds are shared by the seven variants of a (shape, dtype, domain): computed once
_cache = {}


def _case_data(shape, dt, log2):
    key = (shape, dt, log2)
    if key not in _cache:
        _cache.clear()
        B, T, nh = shape
        seed = B * 100003 + T * 101 + nh
        probes = {k: ac.build_probe(k, B, T, nh, dt, seed) for k in ac.PROBES}
        refs = {}
        if ac.ref_affordable(B, T, nh):
            for i, rg in enumerate(ac.REGIMES):
                qkv = ac.regime_input(rg, B, T, nh, dt, log2, seed + 7 * i + 1)
                o, A, S, M = ac.reference(qkv, B, T, nh, log2)
                refs[rg] = (qkv, o, ac.error_bound(o, A, S, M, qkv, B, T, nh, dt, log2))
        _cache[key] = (probes, refs)
    return _cache[key]


def _cases():
    out = []
    for shape in ac.SHAPES:
        for dt in (ac.F16, ac.BF16):
            for log2 in (True, False):
                for variant in ac.VARIANTS:
                    out.append(pytest.param(shape, dt, log2, variant, id="%s-%s-%s-%s" % (
                        ac.DT_NAME[dt], "log2" if log2 else "exp", variant, ac.shape_id(shape))))
    return out


@pytest.mark.parametrize("shape,dt,log2,variant", _cases())
def test_attention_instance(api, shape, dt, log2, variant):
    """Exact probes (permutation and pairs bit for bit, one-hot uniform within 1 ulp), then -- where a float64 reference is
    affordable -- three score regimes within the derived per-element bound; the guard rows are checked on every call."""
    B, T, nh = shape
    probes, refs = _case_data(shape, dt, log2)
    fails = []
    for kind, (qkv, exp) in probes.items():
        ok, msg = ac.check_probe(kind, _attention(api, dt, qkv, B, T, nh, log2, variant), exp, dt)
        if not ok:
            fails.append(msg)
    for rg, (qkv, o, bound) in refs.items():
        ok, msg = ac.check_against_reference(_attention(api, dt, qkv, B, T, nh, log2, variant), o, bound)
        if not ok:
            fails.append("%s regime: %s" % (rg, msg))
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("T", [1374, 261, 65])
def test_log2_variants_bit_for_bit_and_batch_invariant(api, dt, T):
    """Every variant of the shipped (log2) instances gives the same bits for a batch of three images with six heads, and each image
    alone (the dispatcher's pick for one image) gives the bits it got inside the batch: an image does not depend on its batch."""
    B, nh = 3, 6
    qkv = ac.regime_input("random", B, T, nh, dt, True, 11 + T)
    qkv[T // 2, :nh * 64] = ac.round_t(qkv[T // 2, :nh * 64] * 6.0, dt)  # large scores: reference-point moves mid-sequence
    outs = {v: _attention(api, dt, qkv, B, T, nh, True, v) for v in ac.VARIANTS}
    assert np.isfinite(outs["v1"]).all()
    for v, o in outs.items():
        assert np.array_equal(o, outs["v1"]), v
    for b in range(B):
        alone = _attention(api, dt, qkv[b * T:(b + 1) * T], 1, T, nh, True)
        assert np.array_equal(alone, outs["v1"][b * T:(b + 1) * T]), b


@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
def test_log2_kernel1_bitwise_repeatable(api, dt):
    """The batch-32 kernel at the shipped instance: four runs, identical bits (see test_attention_bitwise_repeatable)."""
    B, T, nh = 2, 1374, 4
    qkv = ac.regime_input("random", B, T, nh, dt, True, 77)
    outs = [_attention(api, dt, qkv, B, T, nh, True, "v1") for _ in range(4)]
    assert np.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
def test_qkv_gemm_then_log2_attention(api, dt):
    """The forward's pair: the QKV GEMM epilogue with qscale = 0.125 * log2(e) (csrc/model.cpp forward()), then attention with
    log2_scores = 1, against a float64 softmax(Q K^T / 8) V of the unrounded x W^T + b: the log2(e) fold is applied exactly once.
    x, W and b lie on grids that make x W^T + b exact in f32, so the only input error is the rounding of q, k, v to T:
    q relative <= u + 2^-22 (scale product and rounding), k, v <= u; per query |ds| <= sum_d |q_d k_d| ((1 + e_q)(1 + e_k) - 1) in
    natural units, which moves the output by <= 2 ds A e^(2 ds); V's rounding adds u A."""
    B, T, nh = 2, 261, 2
    H, M = nh * 64, B * T
    u = ac.U[dt]
    rng = np.random.default_rng(21 + dt)
    x = rng.integers(-16, 17, (M, H)) / 8.0                 # multiples of 1/8, |x| <= 2
    W = rng.integers(-8, 9, (3 * H, H)) / 64.0              # multiples of 1/64, |W| <= 1/8
    bias = rng.integers(-256, 257, 3 * H) / 512.0
    qscale = 0.125 * math.log2(math.e)                      # csrc/model.cpp forward()
    qkv = np.zeros((M, 3 * H), np.float32)
    rc = api.lib().dinov2_hip_op_gemm(dt, EPI_QKV, _p(x.astype(np.float32)), _p(W.astype(np.float32)), _p(bias.astype(np.float32)),
                                      fp(), 0, _p(qkv), M, 3 * H, M, 3 * H, H, 0, 0, 0, H, qscale)
    assert rc == 0
    out = _attention(api, dt, qkv, B, T, nh, True)

    exact = x @ W.T + bias
    exact[:, :H] /= 8.0                                     # natural units
    o_x, A_x, S_x, _ = ac.reference(exact, B, T, nh, False)
    o_s, A_s, S_s, M_s = ac.reference(qkv, B, T, nh, True)  # the stored operands, in the kernel's units
    kb = ac.error_bound(o_s, A_s, S_s, M_s, qkv, B, T, nh, dt, True)
    eq, ek = u + 2.0 ** -22, u
    ds = np.repeat(S_x * ((1 + eq) * (1 + ek) - 1), 64, axis=1)
    bound = kb + 2 * ds * A_x * np.exp(2 * ds) + u * A_x * np.exp(2 * ds)
    ok, msg = ac.check_against_reference(out, o_x, bound)
    assert ok, msg
