"""The off-family geometry sweep on the device (tests/geometry_cases.py; the CPU side is tests/test_geometry_probes.py).  For every geometry
the loader accepts, the forward meets the project's stated bound against the oracle; every other geometry is refused by
dinov2_hip_model_load with a message that names the limit.  Every row of the table is in one of the two parametrised tests below, so none of
them loads and then fails or is wrong.

Contracts, as the tests they are taken from state them:
  ggml-default oracle (tests/test_gpu_parity.py::test_synthetic_model_vs_oracle): logits 1e-3 * max(1, max|logit|), tokens and cls
      5e-3 * max(1, max|token|), probabilities 1e-3 absolute; 8 x in bf16 compute (three fewer mantissa bits);
  exact arithmetic (tests/test_gpu_trained_like.py::test_trained_like_small_configs): |HIP - exact| <= 1.5 |oracle - exact| + 1e-4 on the logits.
      The oracle rounds its activations to f16 whatever the compute type, so a bf16 row is held to 8 x that right-hand side -- the same factor,
      for the same reason, as in the first contract (a deviation from the f16 statement of that contract: without the factor no bf16 path can
      meet it against an f16-rounding yardstick; the oracle's own distance with bf16 activation rounding is recorded next to it).  The row
      without a classifier has no logits: its patch tokens and cls are held to the same form;
  quantised files (tests/test_gpu_parity.py::test_quantised_gguf_dequant_on_load): 1e-3 against the oracle's dequantised-weights mode, 2e-2
      against its ggml mode (activations quantised as well).
Measured distances go to geometry_parity.json, next to the parity record of tests/test_gpu_configs.py."""
import json
import os
import re

import numpy as np
import pytest

import attn_row_cases as rc
import attention_cases as ac
import gemm_plan_cases as gp
import geometry_cases as gc
import misc_cases as mc
from oracle.gguf_np import GGUFFile
from oracle.oracle import OracleModel
from test_gpu_attention_maps import _block, _float64_bound, _op_layernorm
from test_gpu_configs import _RESULTS as _PARITY_RECORD
from test_gpu_dense import _check_dense
from test_gpu_ln_fold import ln_plan_case_bits
from test_gpu_ops import _gemm, gemm_plan_case_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RESULTS = os.path.join(os.path.dirname(_PARITY_RECORD), "geometry_parity.json")  # the results directory of the other parity records
BF16 = 1
EPS = 1e-6
ERR_UNSUPPORTED, ERR_HIP, ERR_NO_HEAD = 3, 5, 6


def _record(name, **vals):
    try:
        os.makedirs(os.path.dirname(_RESULTS), exist_ok=True)
        cur = json.load(open(_RESULTS)) if os.path.exists(_RESULTS) else {}
        cur[name] = {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in vals.items()}
        json.dump(cur, open(_RESULTS, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _abs(a, b):
    return float(np.abs(a - b).max())


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


@pytest.fixture(scope="module")
def files(tmp_path_factory, pkg):
    return gc.file_cache(pkg, tmp_path_factory.mktemp("geometry"))


@pytest.fixture(scope="module")
def references(pkg, files):
    """The oracle's outputs for image 1 of a row's batch, computed once per row and shared by the ln_fold = -1 and ln_fold = 1 cases."""
    made = {}

    def get(g):
        if g["name"] not in made:
            path, img, head = files(g), gc.images(pkg, g, batch=2)[1], g["num_classes"] > 0
            quant = g["wtype"].startswith("q")
            ora = OracleModel(path, quant_mode="dequant") if quant else OracleModel(path)
            ref = {"classify": ora.forward(img, classify=True) if head else None, "features": ora.forward(img, classify=False)}
            if quant:
                ref["ggml"] = OracleModel(path, quant_mode="ggml").forward(img, classify=True)
            elif head:
                ref["exact"] = ora.forward_exact(img, classify=True)
            else:  # the file without a classifier: its features are what exact arithmetic is asked about
                ref["exact_features"] = ora.forward_exact(img, classify=False)
            if g["dtype"] == BF16 and head and not quant:  # recorded, not asserted: the oracle with bf16 activation rounding
                ref["bf16_acts"] = OracleModel(path, act_round=2).forward(img, classify=True)
            made[g["name"]] = ref
        return made[g["name"]]

    return get


@pytest.fixture(scope="module")
def forwards(api, pkg, files):
    """get(row, fold) -> _forward's result, run once: the ln_fold = 1 case compares itself with the row's ln_fold = -1 run, whichever of the
    two cases runs first."""
    made = {}

    def get(g, fold):
        if (g["name"], fold) not in made:
            made[g["name"], fold] = _forward(api, pkg, files, g, fold)
        return made[g["name"], fold]

    return get


def _forward(api, pkg, files, g, fold):
    """Load the row's model and run its batch: classify (where the file has a head) and features; image 1 alone on the same session."""
    model = api.Model(files(g), dtype=g["dtype"], classify=True, ln_fold=fold)
    hp = model.hparams
    cfg = g["cfg"]
    assert (hp.hidden_size, hp.num_attention_heads, hp.patch_size, hp.ffn_hidden, bool(hp.swiglu), hp.num_register_tokens, bool(hp.has_classifier)) == \
        (cfg["hidden"], cfg["heads"], cfg["patch"], cfg["ffn"], cfg["swiglu"], g["registers"], g["num_classes"] > 0)
    imgs = gc.images(pkg, g)
    sess = api.Session(model)
    out = {"arena": model.arena()[1]}
    if g["num_classes"] > 0:
        assert hp.num_classes == g["num_classes"]
        got = sess.predict(imgs, classify=True)
        one = sess.predict(imgs[1:2], classify=True)
        for k in ("logits", "probs", "cls", "patch_tokens"):
            assert got[k].shape[0] == g["batch"] and np.isfinite(got[k]).all(), k
            ok, msg = mc.check_exact(one[k][0], got[k][1], f"{g['name']} fold={fold}: image 1 alone vs in the batch, classify {k}")
            assert ok, msg
            out["classify." + k] = got[k][1].copy()
        np.testing.assert_allclose(got["probs"].sum(-1), 1.0, atol=1e-5)
    else:
        with pytest.raises(api.DinoError) as e:  # a file without a classifier: asked to classify, the call says so
            sess.predict(imgs[:1], classify=True)
        assert e.value.status == ERR_NO_HEAD
    feat = sess.predict(imgs, classify=False)
    one = sess.predict(imgs[1:2], classify=False)
    P = gc.tokens(g) - 1 - g["registers"]
    assert feat["patch_tokens"].shape == (g["batch"], P, cfg["hidden"])
    for k in ("cls", "patch_tokens"):
        assert np.isfinite(feat[k]).all(), k
        ok, msg = mc.check_exact(one[k][0], feat[k][1], f"{g['name']} fold={fold}: image 1 alone vs in the batch, features {k}")
        assert ok, msg
        out["features." + k] = feat[k][1].copy()
    return out


@pytest.mark.parametrize("fold", [-1, 1], ids=["nofold", "fold"])
@pytest.mark.parametrize("g", gc.RUNNING, ids=gc.geometry_id)
def test_running_geometry_meets_the_contracts(forwards, references, g, fold):
    got, ref = forwards(g, fold), references(g)
    scale = 8.0 if g["dtype"] == BF16 else 1.0
    quant = g["wtype"].startswith("q")
    rec = {"hidden": g["cfg"]["hidden"], "tokens": gc.tokens(g), "batch": g["batch"], "bf16": g["dtype"] == BF16}
    feat = ref["features"]
    rec["features_rel_dtoken"] = _rel(got["features.patch_tokens"], feat["patch_tokens"])
    rec["features_rel_dcls"] = _rel(got["features.cls"], feat["cls"])
    if ref["classify"] is not None:
        exp = ref["classify"]
        rec.update(max_abs_logit=float(np.abs(exp["logits"]).max()), rel_dlogit=_rel(got["classify.logits"], exp["logits"]),
                   abs_dlogit=_abs(got["classify.logits"], exp["logits"]), max_abs_dprob=_abs(got["classify.probs"], exp["probs"]),
                   rel_dtoken=_rel(got["classify.patch_tokens"], exp["patch_tokens"]), rel_dcls=_rel(got["classify.cls"], exp["cls"]))
    if quant:
        rec["rel_dlogit_vs_ggml_mode"] = _rel(got["classify.logits"], ref["ggml"]["logits"])
    elif "exact" in ref:
        ex = ref["exact"]
        rec.update(hip_vs_exact_abs=_abs(got["classify.logits"], ex["logits"]), oracle_vs_exact_abs=_abs(ref["classify"]["logits"], ex["logits"]),
                   hip_vs_exact_tokens_abs=_abs(got["classify.patch_tokens"], ex["patch_tokens"]),
                   oracle_vs_exact_tokens_abs=_abs(ref["classify"]["patch_tokens"], ex["patch_tokens"]))
        if "bf16_acts" in ref:
            rec["bf16_activation_oracle_vs_exact_abs"] = _abs(ref["bf16_acts"]["logits"], ex["logits"])
    elif "exact_features" in ref:
        ex = ref["exact_features"]
        rec.update(hip_vs_exact_tokens_abs=_abs(got["features.patch_tokens"], ex["patch_tokens"]), oracle_vs_exact_tokens_abs=_abs(feat["patch_tokens"], ex["patch_tokens"]),
                   hip_vs_exact_cls_abs=_abs(got["features.cls"], ex["cls"]), oracle_vs_exact_cls_abs=_abs(feat["cls"], ex["cls"]))
    # ln_fold: taken where hidden % 128 == 0 and hidden <= 1 536 (the arena then holds the fold's s / c vectors); elsewhere the model must
    # report it OFF: the arena and every output bit of the separate-LayerNorm model
    if fold > 0:
        base = forwards(g, -1)
        rec["ln_fold_taken"] = bool(got["arena"] > base["arena"])
        assert rec["ln_fold_taken"] == gp.ln_fold_applies(g["cfg"]["hidden"]), (got["arena"], base["arena"])
        if not rec["ln_fold_taken"]:
            assert got["arena"] == base["arena"]
            for k in base:
                if k != "arena":
                    ok, msg = mc.check_exact(got[k], base[k], f"{g['name']}: ln_fold = 1 where the width does not take it, {k}")
                    assert ok, msg
    print(g["name"], "fold" if fold > 0 else "nofold", json.dumps(rec, sort_keys=True))
    _record(g["name"] + ("_ln_fold" if fold > 0 else ""), **rec)
    assert rec["features_rel_dtoken"] <= 5e-3 * scale and rec["features_rel_dcls"] <= 5e-3 * scale, rec
    if ref["classify"] is not None:
        assert rec["rel_dlogit"] <= 1e-3 * scale, rec
        assert rec["rel_dtoken"] <= 5e-3 * scale and rec["rel_dcls"] <= 5e-3 * scale, rec
        assert rec["max_abs_dprob"] <= 1e-3 * scale, rec
    if quant:
        assert rec["rel_dlogit_vs_ggml_mode"] <= 2e-2, rec
    elif "exact" in ref:
        assert rec["hip_vs_exact_abs"] <= (1.5 * rec["oracle_vs_exact_abs"] + 1e-4) * scale, rec
    elif "exact_features" in ref:  # no logits to hold: the same contract on the features (tokens and cls)
        assert rec["hip_vs_exact_tokens_abs"] <= (1.5 * rec["oracle_vs_exact_tokens_abs"] + 1e-4) * scale, rec
        assert rec["hip_vs_exact_cls_abs"] <= (1.5 * rec["oracle_vs_exact_cls_abs"] + 1e-4) * scale, rec


@pytest.mark.parametrize("g", gc.REFUSALS, ids=gc.geometry_id)
def test_refused_geometry_is_refused_at_load(api, files, g):
    """DINOV2_HIP_ERR_UNSUPPORTED from dinov2_hip_model_load, the text naming the hparam, its value and the limit -- not a HIP error from the
    first forward.  The load raises and hands no model back: there is no handle that dinov2_hip_workspace_bytes, a session or a predict
    could be given."""
    for dt in (0, BF16):
        with pytest.raises(api.DinoError) as e:
            api.Model(files(g), dtype=dt, classify=True)
        hparam, value, limit = g["refusal"]
        msg = str(e.value)
        assert e.value.status == ERR_UNSUPPORTED != ERR_HIP, msg
        assert hparam in msg and re.search(r"\b%d\b" % value, msg) and re.search(r"\b%d\b" % limit, msg), msg


def test_every_row_of_the_table_is_in_one_of_the_two_tests_above():
    assert sorted(g["name"] for g in gc.RUNNING + gc.REFUSALS) == sorted(g["name"] for g in gc.GEOMETRIES)


# ---- the GEMM plans the sweep reaches and the family's lists do not launch ----
@pytest.mark.parametrize("case", gp.GEOMETRY_COVERAGE_CASES, ids=lambda c: "dt%d-epi%d-%dx%dx%d" % c)
def test_geometry_gemm_plan_coverage_case_bits(api, case):
    gemm_plan_case_bits(api, case)


KS1 = "small<64x128,w4x2,st3,ks1>"  # the one small-tile configuration no family shape selects (an odd K / 64, or K < 256, with few tiles)


@pytest.mark.parametrize("case", [c for c in gp.GEOMETRY_COVERAGE_CASES if c[2] < 100], ids=lambda c: "dt%d-epi%d-%dx%dx%d" % c)
def test_ks1_configuration_against_float64(api, case):
    """The bit-equality body above cannot cross-check this configuration against another kernel for most epilogues: forcing the small-tile
    kernel selects it again, and so does the 100-row launch (what those comparisons establish there is that a row's bits do not depend on M).
    So each of its epilogues -- patch, QKV, residual, GELU, SwiGLU -- is also held to float64 of the same operands, with the references and
    tolerances of tests/test_gpu_ops.py's per-epilogue tests (f32 outputs: rtol 2e-5, atol 2e-4; two-byte outputs: one output ulp)."""
    dt, epi, M, N, K = case
    assert api.gemm_plan(dt, epi, M, N, K) == KS1
    rng = np.random.default_rng(5 * M + 3 * N + K + 17 * epi + dt)
    rnd = lambda a: ac.round_t(np.asarray(a, np.float32), dt)  # noqa: E731
    A, W = rnd(rng.standard_normal((M, K))), rnd(rng.standard_normal((N, K)) * 0.1 + np.linspace(-0.05, 0.08, N)[:, None])
    bias = rng.standard_normal(N).astype(np.float32)
    h = A.astype(np.float64) @ W.astype(np.float64).T + bias
    ulp = 2e-3 if dt == 0 else 1.6e-2

    def launch(out, aux, ldo, W=W, bias=bias, **kw):
        return _gemm(api, dt, epi, A, np.ascontiguousarray(W), np.ascontiguousarray(bias), aux, out, M, N, K, ldo, **kw)

    if epi == gp.EPI_PATCH:
        R, T = 3, M + 4
        pos = rng.standard_normal((1 + M, N)).astype(np.float32)
        x = launch(np.full((T, N), 7.0, np.float32), pos, N, P=M, T=T, R=R)
        ref = np.full((T, N), 7.0, np.float32)
        ref[1 + R:] = h + pos[1:]
        np.testing.assert_allclose(x, ref, rtol=2e-5, atol=2e-4)
    elif epi == gp.EPI_QKV:
        out = launch(np.zeros((M, N), np.float32), None, N, qcols=N // 3, qscale=0.125)
        h[:, :N // 3] *= 0.125
        np.testing.assert_allclose(out, rnd(h), rtol=ulp, atol=ulp)
    elif epi == gp.EPI_RESID:
        ls, x0 = rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
        out = launch(x0.copy(), ls, N)
        np.testing.assert_allclose(out, (x0 + ls * h).astype(np.float32), rtol=2e-5, atol=2e-4)
    elif epi == gp.EPI_GELU:  # ggml's f16 table (tests/test_gpu_ops.py::test_gemm_gelu_epilogue_matches_ggml_f16_lut, its two bounds)
        out = launch(np.zeros((M, N), np.float32), None, N)
        xr = h.astype(np.float32).astype(np.float16).astype(np.float64)
        g = (0.5 * xr * (1 + np.tanh(0.79788456080286535587989211986876 * xr * (1 + 0.044715 * xr * xr)))).astype(np.float32).astype(np.float16).astype(np.float32)
        ref = rnd(np.where(h <= -10, 0, np.where(h >= 10, h, g)).astype(np.float16).astype(np.float32))
        diff = np.abs(out - ref)
        lo, hi = (2e-3, 4e-3) if dt == 0 else (8e-3, 1.6e-2)
        assert (diff > lo * np.maximum(1, np.abs(ref))).mean() < 1e-3 and diff.max() <= hi * max(1.0, float(np.abs(ref).max()))
    else:  # SwiGLU: W and bias are [x1 ; x2] as in the file, handed over interleaved in 32-row blocks as the loader does
        F = N // 2
        n = np.arange(N)
        src = ((n >> 5) & 1) * F + (n >> 6) * 32 + (n & 31)
        out = launch(np.zeros((M, F), np.float32), None, F, W=W[src], bias=bias[src])
        x1, x2 = h[:, :F], h[:, F:]
        np.testing.assert_allclose(out, rnd((x1 / (1 + np.exp(-x1)) * x2).astype(np.float32)), rtol=ulp, atol=ulp)


@pytest.mark.parametrize("case", gp.GEOMETRY_LN_COVERAGE_CASES, ids=lambda c: "dt%d-epi%d-%dx%dx%d" % c)
def test_geometry_ln_plan_coverage_case_bits(api, case):
    ln_plan_case_bits(api, case)


# ---- side outputs at H = 64, 320 and 2 048, and at patch 1 (H = 128, 3 x 23 patches, two registers) ----
def _final_ln(path):
    t = GGUFFile(path).tensors
    return t["layernorm.weight"].to_f32().reshape(-1).astype(np.float32), t["layernorm.bias"].to_f32().reshape(-1).astype(np.float32)


@pytest.mark.parametrize("name", gc.SIDE_OUTPUTS_TAPS)
def test_layer_taps_tokens_and_chw_against_float64_of_the_oracle(api, pkg, files, name):
    """predict_layers with norm = True, every layer, both layouts: ln_reference (float64) of the oracle's hidden states under the token bound
    5e-3 * max(1, max|ref|) (tests/test_gpu_layers.py::test_normalised_taps_against_float64_of_the_oracle); CHW is TOKENS transposed, bit for
    bit.  H = 64: a quarter of a wave holds the row; 320: the CHW kernel's second 256-channel chunk is a quarter full; 2 048: eight float4
    per lane."""
    g = gc.BY_NAME[name]
    path, imgs = files(g), gc.images(pkg, g, batch=2)
    L, R, H, ps = g["cfg"]["layers"], g["registers"], g["cfg"]["hidden"], g["cfg"]["patch"]
    h0, w0 = g["size"][0] // ps, g["size"][1] // ps
    sess = api.Session(api.Model(path, dtype=g["dtype"], classify=False))
    lw, lb = _final_ln(path)
    hid = OracleModel(path).forward(imgs[1], hidden=True)["hidden"]
    layers = list(range(L + 1))
    tok = sess.predict_layers(imgs, layers, norm=True, reshape=False, return_class_token=True, return_registers=R > 0)
    chw = sess.predict_layers(imgs, layers, norm=True, reshape=True, return_class_token=True, return_registers=R > 0)
    worst = 0.0
    for layer in layers:
        ref = mc.ln_reference(hid[layer], lw, lb, EPS)
        bound = 5e-3 * max(1.0, float(np.abs(ref).max()))
        for what, r in (("tokens", tok), ("chw", chw)):
            d = r["layers"][layer]
            patch = d["patch_tokens"][1]
            if what == "chw":
                assert patch.shape == (H, h0, w0)
                patch = patch.reshape(H, h0 * w0).T
            got = np.concatenate([d["cls"][1][None]] + ([d["registers"][1]] if R else []) + [patch])
            e = float(np.abs(got - ref).max())
            worst = max(worst, e / bound)
            assert e <= bound, f"{name} {what} layer {layer}: {e} > {bound}"
        ok, msg = mc.check_exact(chw["layers"][layer]["patch_tokens"].reshape(2, H, h0 * w0).transpose(0, 2, 1), tok["layers"][layer]["patch_tokens"],
                                 f"{name} layer {layer}: CHW vs TOKENS")
        assert ok, msg
    _record(name + "_layer_taps", worst_error_over_bound=worst)


@pytest.mark.parametrize("name", gc.SIDE_OUTPUTS_TAPS)
def test_cls_attention_row_of_the_last_block_against_float64(api, pkg, files, name):
    """predict_attention, the CLS query of the last block, all heads (1, 5 and 32 of them): the float64 softmax and the derived bound of
    tests/test_gpu_attention_maps.py::test_float64_reference (separate LayerNorm launches: the GEMM's operand is the LayerNorm kernel's output)."""
    g = gc.BY_NAME[name]
    path, imgs = files(g), gc.images(pkg, g, batch=2)
    L, nh, dt = g["cfg"]["layers"], g["cfg"]["heads"], g["dtype"]
    T = gc.tokens(g)
    model = api.Model(path, dtype=dt, classify=False, ln_fold=-1)
    got = api.Session(model).predict_attention(imgs, [L], [0])
    assert got.shape == (1, 2, nh, 1, T)
    w1, b1, W, bias = _block(path, L)
    x = api.Session(model).debug_hidden(imgs, L - 1).reshape(-1, len(w1))
    ln = _op_layernorm(api, dt, x, w1, b1).astype(np.float64)
    P, bound = _float64_bound(ln, np.zeros_like(ln), ac.round_t(W, dt), bias.astype(np.float64), dt, 2, T, nh, [0])
    ok, msg = rc.check_against_reference(got[0], P, bound, name)
    print(msg)
    assert ok, msg
    ok, msg = rc.check_rows_sum_to_one(got[0], T, name)
    assert ok, msg


@pytest.mark.parametrize("name", gc.SIDE_OUTPUTS)
def test_dense_three_class_linear_head(api, pkg, files, name):
    """predict_dense with a 3-class linear head on the last layer's normalised patch tokens: every check of tests/test_gpu_dense.py's model-level
    cases (logits against float64 of the f16 operands, labels and values against the restatement and the float64 pipeline)."""
    g = gc.BY_NAME[name]
    model = api.Model(files(g), dtype=g["dtype"], classify=False)
    _check_dense(api, api.Session(model), model, gc.images(pkg, g, batch=2), [g["cfg"]["layers"]], 3, norm=1, concat_cls=0, out_size=None, what=name)
