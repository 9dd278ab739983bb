"""The checks of tests/test_gpu_misc_kernels.py, on the CPU: the numpy emulations of tests/misc_cases.py must pass every probe and stay
inside every derived bound -- the checks are not too tight -- and each planted bug of misc_cases.MUTANTS must be rejected by the same
checks -- the GPU tests would notice a subtly wrong kernel.  The preprocess emulation is also held bit-equal to the host library.
"""
import numpy as np
import pytest

import misc_cases as mc

DTS = [mc.F32, mc.F16, mc.BF16]
DT_IDS = ["f32", "f16", "bf16"]


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_checks(dt, H, rows, mutant=None):
    """The GPU file's LayerNorm checks with the emulation (mutant or not) in the kernel's place: a list of failure messages."""
    fails = []
    w, b = mc.ln_affine(H, seed=H)
    x = mc.ln_dyadic_rows(rows, H, seed=rows * 31 + H)
    ok, msg = mc.check_exact(mc.ln_emulate(x, w, b, 1e-6, dt, mutant), mc.ln_emulate(x, w, b, 1e-6, dt), "dyadic")
    fails += [] if ok else [msg]
    sign = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    x = (np.array([[1.25], [-3.0], [40.5]]) + 2.0 * sign[None, :]).astype(np.float32)
    exp = mc.round_t(((sign[None, :] * w).astype(np.float32) + b).astype(np.float32), dt)
    ok, msg = mc.check_exact(mc.ln_emulate(x, w, b, 0.0, dt, mutant), np.broadcast_to(exp, x.shape), "eps = 0")
    fails += [] if ok else [msg]
    x = np.broadcast_to(np.array([[0.0], [3.25], [-1e3]], np.float32), (3, H)).copy()
    ok, msg = mc.check_exact(mc.ln_emulate(x, w, b, 1e-6, dt, mutant), np.broadcast_to(mc.round_t(b, dt), x.shape), "constant")
    fails += [] if ok else [msg]
    x = mc.ln_offset_rows(7, H, seed=H + 2)
    got = mc.ln_emulate(x, w, b, 1e-6, dt, mutant)
    ok, msg = mc.check_exact(got, mc.ln_emulate(x, w, b, 1e-6, dt), "offset")
    fails += [] if ok else [msg]
    with np.errstate(invalid="ignore"):
        if not (np.abs(got - mc.ln_reference(x, w, b, 1e-6)) <= mc.ln_offset_bound(x, w, b, 1e-6, dt)).all():
            fails.append("offset rows outside the derived bound")
    return fails


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("H", [4, 384, 516, 1536, 2048])
def test_ln_emulation_passes(dt, H):
    assert not _ln_checks(dt, H, 5)


def test_ln_dyadic_rows_have_exact_statistics():
    x = mc.ln_dyadic_rows(50, 516, seed=1)
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=1, keepdims=True)
    assert (mean == np.round(mean * 8) / 8).all()  # the centre c, exactly
    v = (x - mean.astype(np.float32)).astype(np.float32)
    assert (v.astype(np.float64) == x64 - mean).all() and ((v * v).astype(np.float64) == (x64 - mean) ** 2).all()


@pytest.mark.parametrize("mutant,dts", [("ln_fused_affine", DTS), ("ln_var_from_moments", DTS), ("bf16_truncate", [mc.BF16])])
def test_ln_mutants_rejected(mutant, dts):
    """A fused affine moves about a third of the f32 results by one ulp; after the store's rounding to f16 / bf16 only the few that
    cross a rounding boundary show, so those types are checked at the GPU file's largest shape (4097 x 2048), as the GPU run sees it."""
    for dt in dts:
        shapes = [(5, 4), (5, 516), (5, 2048)] if dt == mc.F32 or mutant != "ln_fused_affine" else [(4097, 2048)]
        for rows, H in shapes:
            assert _ln_checks(dt, H, rows, mutant), (mutant, dt, H)


def test_ln_offset_bound_is_not_vacuous():
    """The derived bound at mean 1e4, std 1e-2 is dominated by the f32 mean's rounding (half of 2^-10, times scale ~ 100: ~0.05 |w|)."""
    w, b = mc.ln_affine(768, seed=1)
    x = mc.ln_offset_rows(7, 768, seed=2)
    bound = mc.ln_offset_bound(x, w, b, 1e-6, mc.F32)
    assert np.median(bound / np.abs(w)) < 0.07


# ------------------------------------------------------------------------------------------------------------- preprocess
_PP = [(1, 1), (7, 1), (15, 29), (224, 224), (257, 255), mc.PP_SIZES[-1]]


@pytest.mark.parametrize("patch", [14, 16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hw", _PP, ids=["%dx%d" % s for s in _PP])
def test_preprocess_emulation_equals_host(api, hw, mode, patch):
    """The numpy restatement of the host's f32 arithmetic is the host library, bit for bit: the same rounding points the device
    kernel is held to."""
    img = mc.pp_images(2, *hw, seed=hw[0] + hw[1])[1]
    host = (api.dino_classify_preprocess if mode == 1 else api.dino_preprocess)(img, patch)
    ok, msg = mc.check_exact(mc.preprocess_emulate(img, mode, patch), host, "emulation vs host")
    assert ok, msg


def test_fused_bicubic_taps_rejected(api):
    img = mc.pp_images(1, 90, 123, seed=4)[0]
    for mode in (0, 1):
        host = (api.dino_classify_preprocess if mode == 1 else api.dino_preprocess)(img, 14)
        ok, msg = mc.check_exact(mc.preprocess_emulate(img, mode, 14, "fused_bicubic_taps"), host, "fused taps")
        assert not ok


# ------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("dt", [mc.F16, mc.BF16], ids=["f16", "bf16"])
def test_head_emulation_within_bounds(dt):
    B, H, Cn, R = 3, 384, 1001, 4
    fin, W, bias = mc.head_dyadic_case(B, 1 + R + 64, H, Cn, R, dt, seed=3)
    feat = mc.head_pool_emulate(fin, 1 + R, 1.0 / 64, dt)
    logits = mc.head_logits_emulate(feat, W, bias)
    ref, bound = mc.head_logits_bound(feat, W, bias)
    assert (np.abs(logits - ref) <= bound).all()
    assert (bound < 1e-4 * (np.abs(feat) @ np.abs(W).T).max()).all()  # gamma_n, n ~ 30: a few 1e-6 relative
    probs = mc.softmax_emulate(logits)
    p64, pb = mc.softmax_bound(logits)
    assert (np.abs(probs - p64) <= pb).all()


def test_head_exact_logits_probe_is_exact():
    """The dyadic probe's logits in the kernel's order equal float64 bit for bit, and its logits leave the expf sums exact."""
    for dt in (mc.F16, mc.BF16):
        fin, W, bias, first, inv_div = mc.head_exact_logits_case(3, 1536, 1001, seed=2)
        feat = mc.head_pool_emulate(fin, first, inv_div, dt)
        assert (feat == mc.head_pool_emulate(fin, first, inv_div, mc.F32)).all()  # exact in T
        logits = mc.head_logits_emulate(feat, W, bias)
        exp = (feat.astype(np.float64) @ W.astype(np.float64).T + bias).astype(np.float32)
        assert mc.check_exact(logits, exp, "logits")[0] and mc.head_logit_spread_ok(logits)


@pytest.mark.parametrize("mutant", ["pool_includes_registers", "pool_starts_late", "bf16_truncate"])
def test_pool_mutants_rejected(mutant):
    R = 4
    fin, _, _ = mc.head_dyadic_case(3, 1 + R + 16, 384, 3, R, mc.BF16, seed=1)
    ok, _ = mc.check_exact(mc.head_pool_emulate(fin, 1 + R, 1.0 / 16, mc.BF16, mutant=mutant),
                           mc.head_pool_emulate(fin, 1 + R, 1.0 / 16, mc.BF16), "feat")
    assert not ok


def test_softmax_probes_and_mutant():
    Cn = 1001
    l = np.full((2, Cn), 3.5, np.float32)
    assert mc.check_exact(mc.softmax_emulate(l), np.full_like(l, np.float32(1) / np.float32(Cn)), "equal")[0]
    l = np.random.default_rng(0).standard_normal((2, Cn)).astype(np.float32)
    l[:, 7] += 200.0
    exp = np.zeros_like(l)
    exp[:, 7] = 1.0
    assert mc.check_exact(mc.softmax_emulate(l), exp, "saturated")[0]
    assert not mc.check_exact(mc.softmax_emulate(l, "softmax_no_max"), exp, "saturated")[0]


# ------------------------------------------------------------------------------------------------------------- weights
def test_interleave_restatement_matches_the_index_formula():
    """The reshape restatement against the formula the SwiGLU GEMM test uses (tests/test_gpu_ops.py::test_gemm_swiglu_epilogue)."""
    for F in (32, 96, 4096):
        n = np.arange(2 * F)
        src = ((n >> 5) & 1) * F + (n >> 6) * 32 + (n & 31)
        assert (mc.interleave_rows(np.arange(2 * F), F) == src).all()
        assert not (mc.interleave_rows(np.arange(2 * F), F, "interleave_swapped") == src).all()


@pytest.mark.parametrize("tname", mc.CONVERT_TYPES)
def test_convert_mutants_rejected(tname):
    raw, gt, vals = mc.weight_source(tname, 192, 96, seed=1)
    base = mc.convert_expected(vals, mc.BF16, 104, 96)
    assert not mc.check_exact(mc.convert_expected(vals, mc.BF16, 104, 96, "interleave_swapped"), base, "")[0]
    if tname not in ("bf16",) and not tname.startswith("q"):  # bf16 sources are exact in bf16; q-values are few-bit
        assert not mc.check_exact(mc.convert_expected(vals, mc.BF16, 104, 96, "bf16_truncate"), base, "")[0]
    assert not mc.convert_expected(vals, mc.F16, 104, 96)[:, 96:].any()
