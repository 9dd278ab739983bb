"""The forward's kernels at the far end of their 32-bit byte offsets (cases: tests/far_cases.py; CPU probes: tests/test_far_probes.py).

launch_gemm takes operands up to M * lda * 2 < 2^32 and N * ldw * 2 < 2^32 bytes, launch_attention qkv up to B * T * 3H * 2 < 2^32, and a pass
of the forward keeps rows * widest_row * 2 < 2^31.  The refusals at those limits are tested elsewhere; here the kernels RUN just below them:
ONE launch per test through dinov2_hip_op_gemm_far / dinov2_hip_op_attention_far (operands made on the device from far_value), and the model
at the largest batch and the longest list a pass takes.  What a test costs is fills and copies; the arithmetic is milliseconds but for A2 / A3.

Each test prints "far: <id> wall <s> device <GiB>" (profiles/far_offsets.md holds the figures of a run) and skips only when the device has
less memory free than the test needs."""
import time

import numpy as np
import pytest

import attention_cases as ac
import far_cases as fc
from test_gpu_ops import _gemm, _round

pytestmark = pytest.mark.gpu

GIB = float(1 << 30)


def _need(api, nbytes):
    free, _ = api.device_memory()
    if free < nbytes:
        pytest.skip("needs %.1f GiB of device memory, %.1f GiB are free" % (nbytes / GIB, free / GIB))


def _report(rid, t0, nbytes):
    print("far: %s wall %.2f s device %.2f GiB" % (rid, time.perf_counter() - t0, nbytes / GIB))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- GEMM
_A_ROWS = {}


def _a_rows(c, rows):
    """The sampled rows of A, shared by the runs of a case (the float64 side of every check starts from them)."""
    key = (c.name, len(rows), int(rows.sum()))
    if key not in _A_ROWS:
        _A_ROWS.clear()  # one case at a time: the runs of a case come one after the other
        _A_ROWS[key] = fc.far_value(fc.SEED_A, rows, np.arange(c.K))
    return _A_ROWS[key]


def _float64_check(c, epi, dt, got, A, W, bias, aux, x0, qcols, qscale):
    """The float64 restatement of each epilogue with the tolerances of tests/test_gpu_ops.py (test_gemm_plain, _qkv_epilogue,
    _residual_epilogue, _gelu_epilogue_matches_ggml_f16_lut, _swiglu_epilogue), unchanged."""
    h = A.astype(np.float64) @ W.astype(np.float64).T + bias
    if epi == fc.EPI_PLAIN_F32:
        assert np.array_equal(_bits(got), _bits(h.astype(np.float32)))  # bit for bit: the docstring of the test says why
    elif epi == fc.EPI_QKV:
        h[:, :qcols] *= qscale
        tol = 2e-3 if dt == fc.F16 else 1.6e-2
        np.testing.assert_allclose(got, _round(h.astype(np.float32), dt), rtol=tol, atol=tol)
    elif epi == fc.EPI_RESID:
        np.testing.assert_allclose(got, (x0 + aux * h).astype(np.float32), rtol=2e-5, atol=2e-4)
    elif epi == fc.EPI_GELU:
        h = h.astype(np.float32)
        xr = h.astype(np.float16).astype(np.float64)
        g = 0.5 * xr * (1 + np.tanh(0.79788456080286535587989211986876 * xr * (1 + 0.044715 * xr * xr)))
        g = g.astype(np.float32).astype(np.float16).astype(np.float32)
        ref = _round(np.where(h <= -10, 0, np.where(h >= 10, h, g)).astype(np.float16).astype(np.float32), dt)
        diff = np.abs(got - ref)
        lo, hi = (2e-3, 4e-3) if dt == fc.F16 else (8e-3, 1.6e-2)
        assert (diff > lo * np.maximum(1, np.abs(ref))).mean() < 1e-3
        assert diff.max() <= hi * max(1.0, np.abs(ref).max())
    else:  # EPI_SWIGLU: kernel row n of W is logical row src[n] of [x1 (F rows); x2 (F rows)]
        F = c.N // 2
        n = np.arange(c.N)
        src = ((n >> 5) & 1) * F + (n >> 6) * 32 + (n & 31)
        hl = np.empty_like(h)
        hl[:, src] = h
        x1, x2 = hl[:, :F], hl[:, F:]
        tol = 2e-3 if dt == fc.F16 else 1.6e-2
        np.testing.assert_allclose(got, _round((x1 / (1 + np.exp(-x1)) * x2).astype(np.float32), dt), rtol=tol, atol=tol)


@pytest.mark.parametrize("c,epi,gen,dt,rid", fc.gemm_runs(), ids=[r[4] for r in fc.gemm_runs()])
def test_gemm_at_the_far_end(api, c, epi, gen, dt, rid):
    """One launch_gemm with its operand at the limit (far_cases.GEMM_CASES), the sampled rows read back, all columns checked.

    * The plan is the one the case names.
    * Bit for bit against dinov2_hip_op_gemm on just the sampled rows as a small-M problem: "every plan gives a row the same bits" is this
      project's contract, and a row read from or written to a wrong offset has other bits (the pattern has no period at the alias distances:
      tests/test_far_probes.py).
    * EPI_PLAIN_F32 bit for bit against the float64 product of the pattern operands plus bias.  Exact by construction: the operands are
      multiples of 2^-6 of magnitude <= 1, so every product is a multiple of 2^-12 of magnitude <= 1 and every partial sum of at most K <= 4096
      of them, in any order, has 12 fraction bits and at most 12 integer bits -- 24 significant bits, an f32; the bias is a multiple of 2^-6
      below 1 and K <= 1024 here, so the sum with it still fits.  The other epilogues against their float64 restatements of
      tests/test_gpu_ops.py with that file's tolerances.
    * The untouched count is 0.  Outputs that start as 0xff bytes: an element that was written cannot be all ones, which is a NaN no epilogue
      produces from finite data.  EPI_RESID, x = x0 + ls * (acc + bias): acc is a multiple of 2^-12, the bias is a multiple of 2^-6 PLUS 2^-13,
      so acc + bias is an odd multiple of 2^-13 of magnitude < 2^11 -- never 0 and exact in f32 (24 bits); ls is 1, 1/2 or 1/4, so the update
      is at least 2^-15 in magnitude, and |x0| < 1 has an ulp of at most 2^-24: a written element always differs from the x0 it started as.
      The 0 is a check that every element was written, not a statistic."""
    rows = fc.gemm_sample(c, epi)
    W, bias, aux, qcols, qscale = fc.gemm_operands(c, epi)
    width = c.width(epi)
    _need(api, c.device_bytes(epi))
    t0 = time.perf_counter()
    try:
        api.set_tuning("gemm_gen", gen)
        assert api.gemm_plan(dt, epi, c.M, c.N, c.K, c.lda, c.ldw) == c.plan(gen, epi)
        got, untouched = api.op_gemm_far(dt, epi, c.M, c.N, c.K, W, bias, aux, rows, lda=c.lda, ldw=c.ldw, seed_a=fc.SEED_A,
                                         seed_out=fc.SEED_OUT, qcols=qcols, qscale=qscale)
    finally:
        api.reset_tuning("gemm_gen")
    _report(rid, t0, c.device_bytes(epi))
    assert got.shape == (len(rows), width)
    A = _a_rows(c, rows)
    x0 = fc.far_value(fc.SEED_OUT, rows, np.arange(width)) if epi == fc.EPI_RESID else None
    small = x0.copy() if x0 is not None else np.full((len(rows), width), np.nan if epi == fc.EPI_PLAIN_F32 else 0, np.float32)
    _gemm(api, dt, epi, A, W, bias, aux, small, len(rows), c.N, c.K, width, qcols=qcols, qscale=qscale)
    assert untouched == 0, "%d payload elements were never written" % untouched
    bad = np.argwhere(_bits(got) != _bits(small))
    assert len(bad) == 0, "%d elements differ from the small-M run, first at output row %d column %d" % (len(bad), rows[bad[0][0]], bad[0][1])
    _float64_check(c, epi, dt, got, A, W, bias, aux, x0, qcols, qscale)


def test_the_untouched_count_counts(api):
    """The harness itself, at a small shape (two panels, a ragged one): with LayerScale 0 a residual keeps every initial value, so the count
    must be M * N and the rows must come back as the pattern; with LayerScale 1 and the off-grid bias it is 0."""
    M, N, K = 300, 256, 64
    W = fc.far_value(fc.SEED_W, np.arange(N), np.arange(K))
    rows = np.array([0, 255, 256, 299], np.int64)
    x0 = fc.far_value(fc.SEED_OUT, rows, np.arange(N))
    bias = np.full(N, 2.0 ** -13, np.float32)
    got, untouched = api.op_gemm_far(fc.F16, fc.EPI_RESID, M, N, K, W, bias, np.zeros(N, np.float32), rows, seed_a=fc.SEED_A, seed_out=fc.SEED_OUT)
    assert untouched == M * N and np.array_equal(_bits(got), _bits(x0))
    got, untouched = api.op_gemm_far(fc.F16, fc.EPI_RESID, M, N, K, W, bias, np.ones(N, np.float32), rows, seed_a=fc.SEED_A, seed_out=fc.SEED_OUT)
    assert untouched == 0 and (got != x0).all()
    free, total = api.device_memory()
    assert 0 < free <= total


# ------------------------------------------------------------------------------------------------------------- attention
def _attn_run(api, c, v, dt, rid):
    rows = fc.attn_rows(c)
    _need(api, c.device_bytes())
    t0 = time.perf_counter()
    try:
        api.set_tuning("attn_v", v)
        got, untouched = api.op_attention_far(dt, c.B, c.T, c.nh, rows, seed=fc.SEED_QKV, log2_scores=True)
    finally:
        api.reset_tuning("attn_v")
    _report(rid, t0, c.device_bytes())
    assert untouched == 0, "%d output elements were never written" % untouched
    return rows, got


@pytest.mark.parametrize("v,dt", fc.ATTN_BY_NAME["A1"].runs, ids=["v%d-%s" % (v, fc.DT_NAME[d]) for v, d in fc.ATTN_BY_NAME["A1"].runs])
def test_attention_far_image_bases(api, v, dt):
    """A1: 10 754 images of 65 tokens, qkv ending 249 856 bytes below 2^32.  Images 0, 1, the one that straddles byte 2^31 and the next, and the
    last two, all heads and queries: within the bound of attention_cases.error_bound of the float64 reference, and bit for bit what the same
    six images give as a batch of their own."""
    c = fc.ATTN_BY_NAME["A1"]
    rows, got = _attn_run(api, c, v, dt, "A1-v%d-%s" % (v, fc.DT_NAME[dt]))
    images, _ = fc.attn_sample(c)
    qkv = fc.far_value(fc.SEED_QKV, rows, np.arange(3 * c.H))  # every row of the six images, image-major: a batch of six
    nb = len(images)
    ok, msg = ac.check_against_reference(got, *_ref_and_bound(qkv, nb, c.T, c.nh, dt))
    assert ok, msg
    small = np.zeros((nb * c.T, c.H), np.float32)
    rc = api.lib().dinov2_hip_op_attention_ex(dt, api._ptr(qkv), api._ptr(small), nb, c.T, c.H, c.nh, 1)
    assert rc == 0
    bad = np.argwhere(_bits(got) != _bits(small))
    assert len(bad) == 0, "%d elements differ from the six-image batch, first in image %d" % (len(bad), images[bad[0][0] // c.T])


def _ref_and_bound(qkv, B, T, nh, dt):
    o, A, S, M = ac.reference(qkv, B, T, nh, True)
    return o, ac.error_bound(o, A, S, M, qkv, B, T, nh, dt, True)


def _one_image(api, c, v, dt, rid):
    """A2 / A3: heads 0, 17 and 31 of the sampled queries against the row-subset form of the same reference and bound."""
    rows, got = _attn_run(api, c, v, dt, rid)
    _, queries = fc.attn_sample(c)
    assert np.array_equal(rows, queries)
    keys = np.arange(c.T)
    for h in fc.attn_heads(c):
        cols = h * 64 + np.arange(64)
        q = fc.far_value(fc.SEED_QKV, queries, cols)
        k = fc.far_value(fc.SEED_QKV, keys, c.H + cols)
        val = fc.far_value(fc.SEED_QKV, keys, 2 * c.H + cols)
        o, A, S, M = ac.reference_rows(q, k, val, True)
        ok, msg = ac.check_against_reference(got[:, cols], o, ac.error_bound_rows(o, A, S, M, val, dt, True))
        assert ok, "head %d: %s" % (h, msg)
    assert np.isfinite(got).all()  # the heads that are not compared were written with numbers too


@pytest.mark.parametrize("dt", [fc.F16, fc.BF16], ids=["f16", "bf16"])
def test_attention_one_image_at_the_limit_of_a_pass(api, dt):
    """A2: one image of 174 762 tokens and 32 heads, T * 3H * 2 = 2 147 475 456 < 2^31 -- the size just below the refusal of
    test_single_image_limit_of_a_pass (tests/test_gpu_stride.py), run."""
    c = fc.ATTN_BY_NAME["A2"]
    assert c.runs == ((0, fc.F16), (0, fc.BF16))
    _one_image(api, c, 0, dt, "A2-%s" % fc.DT_NAME[dt])


def test_attention_one_image_at_the_launchers_limit(api):
    """A3: one image of 349 525 tokens, 4 294 963 200 bytes of qkv < 2^32, attention_kernel (attn_v = 1), f16.  About 1e15 FLOP: the one case that
    cannot be made cheaper without leaving the limit (its wall time is in profiles/far_offsets.md)."""
    c = fc.ATTN_BY_NAME["A3"]
    assert c.runs == ((1, fc.F16),)
    _one_image(api, c, 1, fc.F16, "A3-v1-f16")


# ------------------------------------------------------------------------------------------------------------- the model at the limit of a pass
SIZE = 518
B_PASS = 190  # dinov2_max_pass_batch of ViT-L/14 with 4 registers at 518 x 518: 261 060 rows, an FFN hidden buffer of 2 138 603 520 bytes
_FIVE = {}


def _five():
    """Five distinct seeded images [5, 3, 518, 518], made once."""
    if "img" not in _FIVE:
        _FIVE["img"] = np.random.default_rng(518).standard_normal((5, 3, SIZE, SIZE)).astype(np.float32)
    return _FIVE["img"]


@pytest.fixture(scope="module")
def large1(pkg, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("far") / "large1.gguf")
    pkg.synth.write_synthetic_gguf(path, "large", layers=1, num_classes=10)
    return path


def _session_memory(api, free0):
    return free0 - api.device_memory()[0]


def _model_need(api, gib=8.5):
    """The sessions below were measured at 7.4 - 7.6 GiB of device memory (model, workspace, staged outputs), with the dense head 10.0."""
    _need(api, int(gib * GIB))


@pytest.mark.parametrize("ln_fold", [-1, 1], ids=["ln", "ln_fold"])
@pytest.mark.parametrize("dt", [fc.F16, fc.BF16], ids=["f16", "bf16"])
def test_predict_at_the_largest_batch_of_a_pass(api, large1, dt, ln_fold):
    """predict, classify, B = 190: the five images tiled.  Every image's cls, patch tokens, logits and probs equal, bit for bit, the same
    image's in the five-image batch.  With ln_fold the LN-fold producers, consumers and their statistics buffer run at that size too."""
    _model_need(api)
    free0 = api.device_memory()[0]
    t0 = time.perf_counter()
    model = api.Model(large1, dtype=dt, classify=True, ln_fold=ln_fold)
    hp = model.hparams
    assert model.tokens(SIZE, SIZE) * B_PASS == 261060 and B_PASS * 1374 * int(hp.ffn_hidden) * 2 == 2138603520 < fc.B31
    assert (B_PASS + 1) * 1374 * int(hp.ffn_hidden) * 2 >= fc.B31
    sess = api.Session(model)
    five = sess.predict(_five(), classify=True)
    got = sess.predict(np.ascontiguousarray(np.tile(_five(), (B_PASS // 5, 1, 1, 1))), classify=True)
    _report("predict-B190-%s-ln_fold%d" % (fc.DT_NAME[dt], ln_fold), t0, _session_memory(api, free0))
    for key in ("cls", "patch_tokens", "logits", "probs"):
        assert got[key].shape[0] == B_PASS and np.isfinite(five[key]).all()
        g = got[key].reshape((B_PASS // 5, 5) + got[key].shape[1:])
        bad = np.argwhere((_bits(g) != _bits(five[key])[None]).reshape(B_PASS, -1).any(1))
        assert len(bad) == 0, "%s: images %s differ from the five-image batch" % (key, bad[:8, 0].tolist())


def test_predict_real_split_at_191(api, large1):
    """B = 191 is cut into 190 + 1 by dinov2_max_pass_batch itself (no DINOV2_HIP_MAX_CHUNK): the same identities."""
    _model_need(api)
    free0 = api.device_memory()[0]
    t0 = time.perf_counter()
    sess = api.Session(api.Model(large1, dtype=fc.F16, classify=True))
    five = sess.predict(_five(), classify=True)
    idx = np.arange(B_PASS + 1) % 5
    got = sess.predict(np.ascontiguousarray(_five()[idx]), classify=True)
    _report("predict-B191-split", t0, _session_memory(api, free0))
    for key in ("cls", "patch_tokens", "logits", "probs"):
        bad = [b for b in range(B_PASS + 1) if not np.array_equal(_bits(got[key][b]), _bits(five[key][idx[b]]))]
        assert not bad, "%s: images %s differ from the five-image batch" % (key, bad[:8])


# predict_list: the longest list the row check takes has (2^31 - 1) // (2 * widest_row) = 262 143 rows (computed as n_fit is in
# tests/test_gpu_predict_list.py): as many 518 x 518 images (1 374 rows each) as leave a rest that a few images of one smaller size fill exactly
LIST_BIG = (518, 518)


def _list_sizes(widest):
    """(n_big, small size, n_small) with n_big * 1374 + n_small * T_small == the row limit exactly: the five images at two sizes."""
    limit = ((1 << 31) - 1) // (2 * widest)
    for n_big in range(B_PASS, 0, -1):
        rest = limit - n_big * 1374
        for n_small in range(1, 6):
            if rest % n_small:
                continue
            P = rest // n_small - 5
            for h0 in range(37, 0, -1):
                if P > 0 and P % h0 == 0 and P // h0 <= 37:
                    return limit, n_big, (14 * h0, 14 * (P // h0)), n_small
    raise AssertionError("no list reaches the limit")


def test_predict_list_at_the_row_limit(api, large1):
    """A list of the five images at two sizes whose rows are exactly the most the list check accepts (one more row is refused: the CPU side is
    test_argument_errors_run_nothing of tests/test_gpu_predict_list.py).  Every image equals, bit for bit, its single-image result."""
    _model_need(api)
    free0 = api.device_memory()[0]
    t0 = time.perf_counter()
    model = api.Model(large1, dtype=fc.F16, classify=True)
    hp = model.hparams
    widest = max(3 * int(hp.hidden_size), int(hp.ffn_hidden), -(-3 * 14 * 14 // 64) * 64)
    limit, n_big, small, n_small = _list_sizes(widest)
    sizes = [LIST_BIG] * n_big + [small] * n_small
    rows = api.list_rows(model, sizes, classify=True)
    assert n_big * 1374 + n_small * (5 + small[0] * small[1] // 196) == limit == 262143
    with pytest.raises(api.DinoError):
        api.list_rows(model, sizes + [(14, 14)], classify=True)  # six more rows: refused
    five = _five()
    imgs = [five[i % 5] if s == LIST_BIG else np.ascontiguousarray(five[i % 5][:, :s[0], :s[1]]) for i, s in enumerate(sizes)]
    sess = api.Session(model)
    got = sess.predict_list(imgs, classify=True)
    _report("predict_list-%d-rows" % limit, t0, _session_memory(api, free0))
    assert int(rows[-1]) == int(got["offsets"][-1])
    single = {}
    for i, s in enumerate(sizes):
        key = (i % 5, s)
        if key not in single:
            single[key] = sess.predict(imgs[i][None], classify=True)
        for name in ("cls", "logits", "probs"):
            assert np.array_equal(_bits(got[name][i]), _bits(single[key][name][0])), (name, i)
        assert np.array_equal(_bits(got["patch_tokens"][i]), _bits(single[key]["patch_tokens"][0])), i


def test_predict_layers_and_dense_at_the_largest_batch(api, large1):
    """predict_layers with layers [0, 1] and predict_dense with a 3-class head at out_size 37 x 37, B = 190: bit-equal to the five-image results."""
    _model_need(api, 11.0)
    free0 = api.device_memory()[0]
    t0 = time.perf_counter()
    model = api.Model(large1, dtype=fc.F16, classify=True)
    sess = api.Session(model)
    batch = np.ascontiguousarray(np.tile(_five(), (B_PASS // 5, 1, 1, 1)))
    five = sess.predict_layers(_five(), [0, 1], return_class_token=True, return_registers=True)
    got = sess.predict_layers(batch, [0, 1], return_class_token=True, return_registers=True)
    for k in range(2):
        for name in ("patch_tokens", "cls", "registers"):
            g = got["layers"][k][name]
            g = g.reshape((B_PASS // 5, 5) + g.shape[1:])
            assert np.isfinite(five["layers"][k][name]).all()
            assert (_bits(g) == _bits(five["layers"][k][name])[None]).all(), (k, name)
    del got
    rng = np.random.default_rng(3)
    H = int(model.hparams.hidden_size)
    head = api.DenseHead(model, [1], rng.standard_normal((3, H)).astype(np.float32) * 0.05, rng.standard_normal(3).astype(np.float32))
    five = sess.predict_dense(_five(), head, out_size=(37, 37))
    got = sess.predict_dense(batch, head, out_size=(37, 37))
    _report("predict_layers+dense-B190", t0, _session_memory(api, free0))
    for name in ("labels", "value", "logits"):
        g = got[name].reshape((B_PASS // 5, 5) + got[name].shape[1:])
        assert (g.view(np.uint8) == five[name].view(np.uint8)[None]).all(), name
