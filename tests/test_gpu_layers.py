"""Intermediate-layer taps (dinov2_hip_predict_layers, include/dinov2_hip.h; layer_tap_kernel, csrc/kernels_misc.hip).

Every equality is bit-for-bit (misc_cases.check_exact through layer_cases.check_taps) unless a bound is named, and every yardstick is
code that has tests of its own: dinov2_hip_op_layernorm(dtype = -1) (the kernel the tap shares its row routine with),
dinov2_hip_debug_hidden, dinov2_hip_predict, the CPU oracle and the HuggingFace hidden states stored with the golden fixtures.

  * op level: dinov2_hip_op_layer_tap over widths, grids, register counts, batches, layouts, norm, destination subsets and input kinds;
  * model level on the golden fixtures (f16 / bf16, ln_fold off / on): against debug_hidden, predict, subsets, batches, split passes,
    device outputs, raw 8-bit input, graphs;
  * the forward's launch counts with and without taps;
  * oracle and HuggingFace references (bounds derived below);
  * one full-size ViT-L/14 + 4 registers @518 case (P = 1 369: CHW runs start at every alignment);
  * argument errors.
The model-level tests need dinov2_hip_predict_layers, which does not exist before this feature: they fail there.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import layer_cases as lc
import misc_cases as mc
from oracle.oracle import OracleModel

pytestmark = pytest.mark.gpu

F16, BF16 = 0, 1
FIXTURES = ["tiny_gelu_noreg", "tiny_gelu_reg4", "tiny_swiglu_reg4"]
fp = C.POINTER(C.c_float)
EPS = 1e-6


def _p(a):
    return a.ctypes.data_as(fp)


def op_layernorm_f32(api, x, w, b, eps=EPS):
    """dinov2_hip_op_layernorm(dtype = -1) on every row of x [..., H]: the final LayerNorm kernel itself."""
    x = np.ascontiguousarray(x, np.float32)
    rows = x.reshape(-1, x.shape[-1])
    out = np.empty_like(rows)
    w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    assert api.lib().dinov2_hip_op_layernorm(-1, _p(rows), _p(w), _p(b), _p(out), rows.shape[0], rows.shape[1], eps) == 0
    return out.reshape(x.shape)


def final_ln(gguf):
    t = OracleModel(gguf).gguf.tensors
    return t["layernorm.weight"].to_f32().reshape(-1).astype(np.float32), t["layernorm.bias"].to_f32().reshape(-1).astype(np.float32)


def as_got(r):
    """Session.predict_layers' per-layer dicts -> the stacked arrays layer_cases.check_taps takes."""
    out = {"patch": np.stack([d["patch_tokens"] for d in r["layers"]])}
    if "cls" in r["layers"][0]:
        out["cls"] = np.stack([d["cls"] for d in r["layers"]])
    if "registers" in r["layers"][0]:
        out["reg"] = np.stack([d["registers"] for d in r["layers"]])
    return out


def keys_of(got):
    return tuple(k for k in ("patch", "cls", "reg") if k in got)


# ------------------------------------------------------------------------------------------------------------------ op level
GRIDS = [(1, 1), (5, 7), (16, 16), (37, 37), (35, 61)]
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(("patch", "cls", "reg"), n)]


def _op_case(api, H, h0, w0, R, B, norm, layout, want, rows_fn, seed):
    T = 1 + R + h0 * w0
    x = lc.tap_stream(rows_fn, B, T, H, seed)
    w, b = mc.ln_affine(H, seed + 1)
    want = tuple(k for k in want if not (k == "reg" and R == 0))
    if not want:
        return
    got = api.op_layer_tap(x, w, b, EPS, R, h0, w0, norm=norm, chw=layout == lc.CHW, want=want)  # raises if a guard band changed
    stream = op_layernorm_f32(api, x, w, b) if norm else x  # norm = 0: the input rows themselves
    got = {k: v[None] for k, v in got.items()}
    ok, msg = lc.check_taps(got, stream[None], [0], R, h0, w0, layout, f"H={H} grid={h0}x{w0} R={R} B={B} norm={norm} layout={layout} want={want}",
                            keys=want)
    assert ok, msg


@pytest.mark.parametrize("layout", [lc.TOKENS, lc.CHW])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("H", [128, 384, 516, 768, 1024, 1536])
def test_op_layer_tap_widths_grids_registers(api, H, norm, layout):
    """Every width class (MAXV 2 / 4 / 8, idle lanes at 128 and 516) x every grid (1 patch; short last tile; whole tiles; P = 1 369, odd;
    2 135) x R = 0 | 4, all three destinations, batch 3 (batch 1 for the two large grids at the wide widths, to bound the host work)."""
    for (h0, w0), R in itertools.product(GRIDS, (0, 4)):
        B = 1 if h0 * w0 > 1000 and H > 768 else 3
        _op_case(api, H, h0, w0, R, B, norm, layout, ("patch", "cls", "reg"), None, 100 + H + h0)


@pytest.mark.parametrize("layout", [lc.TOKENS, lc.CHW])
@pytest.mark.parametrize("norm", [0, 1])
def test_op_layer_tap_destination_subsets_and_batches(api, norm, layout):
    """Every subset of the three destinations (a NULL destination is not written; the others do not move) at B = 1, 3, 32."""
    for want, B in itertools.product(SUBSETS, (1, 3, 32)):
        _op_case(api, 384, 5, 7, 4, B, norm, layout, want, None, 7 + B)
    for want in SUBSETS:
        _op_case(api, 1024, 16, 16, 0, 3, norm, layout, want, None, 11)


@pytest.mark.parametrize("layout", [lc.TOKENS, lc.CHW])
@pytest.mark.parametrize("rows", ["dyadic", "offset"])
def test_op_layer_tap_exact_probe_rows(api, rows, layout):
    """Rows with exact statistics (ln_dyadic_rows) and large-offset rows (ln_offset_rows), through the norm and the raw path."""
    fn = mc.ln_dyadic_rows if rows == "dyadic" else mc.ln_offset_rows
    for H, norm in itertools.product((384, 1024, 1536), (0, 1)):
        _op_case(api, H, 5, 7, 4, 3, norm, layout, ("patch", "cls", "reg"), fn, 3 + H)
    _op_case(api, 1024, 37, 37, 4, 1, 1, layout, ("patch", "cls", "reg"), fn, 5)


# --------------------------------------------------------------------------------------------------------------- model level
def _model(api, golden_dir, name, dt=F16, fold=-1, classify=True):
    gguf = os.path.join(golden_dir, name + ".gguf")
    return gguf, api.Model(gguf, dtype=dt, classify=classify, ln_fold=fold)


def _grid(model, img):
    ps = model.hparams.patch_size
    return img.shape[-2] // ps, img.shape[-1] // ps


def _hidden(sess, imgs, L):
    return np.stack([sess.debug_hidden(imgs, layer) for layer in range(L + 1)])  # [L + 1, B, T, H]


@pytest.mark.parametrize("fold", [-1, 1])
@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("name", FIXTURES)
def test_taps_equal_debug_hidden_and_predict(api, golden_dir, name, dt, fold):
    gguf, model = _model(api, golden_dir, name, dt, fold)
    L, R = int(model.hparams.num_hidden_layers), int(model.hparams.num_register_tokens)
    gold = np.load(os.path.join(golden_dir, name + ".npz"))
    imgs = np.stack([gold["img_56x84"], gold["img_56x84"][:, ::-1].copy(), gold["img_56x84"][:, :, ::-1].copy()])
    h0, w0 = _grid(model, imgs)
    lw, lb = final_ln(gguf)
    hidden = _hidden(api.Session(model), imgs, L)
    normed = op_layernorm_f32(api, hidden, lw, lb)
    sess = api.Session(model)
    plain = api.Session(model).predict(imgs, classify=False)
    plain_cls = api.Session(model).predict(imgs, classify=True)
    all_layers = list(range(L + 1))
    res = {}
    for norm, layout in itertools.product((0, 1), (lc.TOKENS, lc.CHW)):
        r = sess.predict_layers(imgs, all_layers, norm=bool(norm), reshape=layout == lc.CHW, return_class_token=True,
                                return_registers=R > 0, classify=False)
        got = as_got(r)
        ok, msg = lc.check_taps(got, normed if norm else hidden, all_layers, R, h0, w0, layout, f"{name} norm={norm} layout={layout}",
                                keys=keys_of(got))
        assert ok, msg
        res[norm, layout] = got
        for k in ("cls", "patch_tokens"):  # `out` of the same call is a plain predict's
            ok, msg = mc.check_exact(r[k], plain[k], f"out.{k} of predict_layers")
            assert ok, msg
    # the tap of layer L, normalised, IS predict's cls / patch_tokens (features mode)
    for what, a, b in (("cls", res[1, lc.TOKENS]["cls"][L], plain["cls"]), ("patch", res[1, lc.TOKENS]["patch"][L], plain["patch_tokens"])):
        ok, msg = mc.check_exact(a, b, f"tap of layer L vs predict {what}")
        assert ok, msg
    # CHW is TOKENS transposed
    for norm in (0, 1):
        t = res[norm, lc.TOKENS]["patch"]
        ok, msg = mc.check_exact(res[norm, lc.CHW]["patch"], t.transpose(0, 1, 3, 2).reshape(t.shape[0], t.shape[1], t.shape[3], h0, w0), "CHW vs TOKENS")
        assert ok, msg
    # with DINOV2_HIP_CLASSIFY: the same taps, and the outputs of a classifying predict
    r = sess.predict_layers(imgs, all_layers, norm=True, return_class_token=True, return_registers=R > 0, classify=True)
    ok, msg = lc.check_taps(as_got(r), normed, all_layers, R, h0, w0, lc.TOKENS, f"{name} classify", keys=keys_of(as_got(r)))
    assert ok, msg
    for k in ("cls", "patch_tokens", "logits", "probs"):
        ok, msg = mc.check_exact(r[k], plain_cls[k], f"classify out.{k}")
        assert ok, msg
    # a subset equals the same layers out of the full request; an int means the last n layers
    sub = as_got(sess.predict_layers(imgs, [1, L], norm=True, return_class_token=True))
    for k in ("patch", "cls"):
        ok, msg = mc.check_exact(sub[k], res[1, lc.TOKENS][k][[1, L]], f"subset [1, L] {k}")
        assert ok, msg
    last = sess.predict_layers(imgs, 2, norm=True)
    assert [d["layer"] for d in last["layers"]] == [L - 1, L]
    ok, msg = mc.check_exact(as_got(last)["patch"], res[1, lc.TOKENS]["patch"][[L - 1, L]], "layers = 2")
    assert ok, msg
    # a predict after a predict_layers on the same session equals one on a fresh session
    ok, msg = mc.check_exact(sess.predict(imgs, classify=False)["patch_tokens"], plain["patch_tokens"], "predict after predict_layers")
    assert ok, msg


@pytest.mark.parametrize("layout", [lc.TOKENS, lc.CHW])
@pytest.mark.parametrize("dt,fold", [(F16, -1), (BF16, 1)])
@pytest.mark.parametrize("name", ["tiny_gelu_noreg", "tiny_swiglu_reg4"])
def test_batch_five_equals_five_calls_and_split_passes(api, golden_dir, monkeypatch, name, dt, fold, layout):
    gguf, model = _model(api, golden_dir, name, dt, fold)
    L, R = int(model.hparams.num_hidden_layers), int(model.hparams.num_register_tokens)
    imgs = np.random.default_rng(5).standard_normal((5, 3, 70, 98)).astype(np.float32)
    kw = dict(norm=True, reshape=layout == lc.CHW, return_class_token=True, return_registers=R > 0, classify=True)
    sess = api.Session(model)
    full = sess.predict_layers(imgs, [0, 1, L], **kw)
    g = as_got(full)
    for b in range(5):
        one = as_got(sess.predict_layers(imgs[b:b + 1], [0, 1, L], **kw))
        for k in one:
            ok, msg = mc.check_exact(one[k][:, 0], g[k][:, b], f"image {b} alone, {k}")
            assert ok, msg
    monkeypatch.setenv("DINOV2_HIP_MAX_CHUNK", "2")  # passes of 2, 2 and 1 images, last first
    split = api.Session(model).predict_layers(imgs, [0, 1, L], **kw)
    monkeypatch.delenv("DINOV2_HIP_MAX_CHUNK")
    gs = as_got(split)
    for k in g:
        ok, msg = mc.check_exact(gs[k], g[k], f"split passes, {k}")
        assert ok, msg
    for k in ("logits", "cls", "patch_tokens"):
        ok, msg = mc.check_exact(split[k], full[k], f"split passes, out.{k}")
        assert ok, msg


@pytest.mark.parametrize("layout", [lc.TOKENS, lc.CHW])
@pytest.mark.parametrize("dt,fold", [(F16, -1), (BF16, 1)])
def test_device_outputs_equal_host_outputs(api, golden_dir, dt, fold, layout):
    gguf, model = _model(api, golden_dir, "tiny_gelu_reg4", dt, fold)
    L, R, H = int(model.hparams.num_hidden_layers), 4, int(model.hparams.hidden_size)
    imgs = np.random.default_rng(9).standard_normal((3, 3, 56, 84)).astype(np.float32)
    h0, w0 = _grid(model, imgs)
    layers = [0, L]
    host = as_got(api.Session(model).predict_layers(imgs, layers, norm=True, reshape=layout == lc.CHW, return_class_token=True,
                                                      return_registers=True))
    sess = api.Session(model)
    x = api.DeviceArray.from_host(imgs)
    patch = api.DeviceArray((2, 3, H, h0, w0) if layout == lc.CHW else (2, 3, h0 * w0, H), fill_nan=True)
    cls = api.DeviceArray((2, 3, H), fill_nan=True)
    reg = api.DeviceArray((2, 3, R, H), fill_nan=True)
    sess.predict_layers_device(x.ptr, 3, 56, 84, layers, norm=True, reshape=layout == lc.CHW, layer_patch_ptr=patch.ptr,
                               layer_cls_ptr=cls.ptr, layer_reg_ptr=reg.ptr)
    sess.sync()
    for k, t in (("patch", patch), ("cls", cls), ("reg", reg)):
        ok, msg = mc.check_exact(t.to_host(), host[k], f"device {k}")
        assert ok, msg
    # afterwards dinov2_hip_fetch behaves as after a predict of the same shape
    o = api.Output()
    c = np.empty((3, H), np.float32)
    o.cls = c.ctypes.data
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_fetch(sess._h, C.byref(o), err, len(err)) == 0, err.value
    ok, msg = mc.check_exact(c, host["cls"][1], "fetch after predict_layers (cls == tap of layer L)")
    assert ok, msg


def test_pca3_of_the_session_tokens_after_predict_layers(api, golden_dir):
    """dinov2_hip_pca3(tokens = NULL) works on what the last forward left in the session: after a predict_layers it gives what it gives
    after a predict of the same shape (and what it gives for the same tokens handed in from the host)."""
    gguf, model = _model(api, golden_dir, "tiny_gelu_reg4", classify=False)
    L, H = int(model.hparams.num_hidden_layers), int(model.hparams.hidden_size)
    imgs = np.random.default_rng(12).standard_normal((2, 3, 70, 98)).astype(np.float32)
    ref_sess = api.Session(model)
    tok = ref_sess.predict(imgs, classify=False)["patch_tokens"]
    ref = ref_sess.pca3(None, (tok.shape[1], H))
    sess = api.Session(model)
    sess.predict_layers(imgs, [1, L], norm=False, reshape=True, return_class_token=True)
    got = sess.pca3(None, (tok.shape[1], H))
    for a, b, what in zip(got, ref, ("components", "mean", "projection")):
        ok, msg = mc.check_exact(a, b, f"pca3 {what} after predict_layers")
        assert ok, msg
    with pytest.raises(api.DinoError):
        sess.pca3(None, (tok.shape[1] + 1, H))


def test_misaligned_device_pointers_are_refused(api, golden_dir):
    """The kernel stores 16 bytes at a time through device pointers: one that is not 16-byte aligned is ERR_INVALID, nothing is launched,
    the buffers keep their contents and the session stays usable."""
    gguf, model = _model(api, golden_dir, "tiny_gelu_reg4")
    L, R, H = int(model.hparams.num_hidden_layers), 4, int(model.hparams.hidden_size)
    imgs = np.random.default_rng(3).standard_normal((1, 3, 56, 84)).astype(np.float32)
    sess = api.Session(model)
    x = api.DeviceArray.from_host(imgs)
    bufs = {"layer_patch_ptr": api.DeviceArray((2 * 24 * H + 4,), fill_nan=True), "layer_cls_ptr": api.DeviceArray((2 * H + 4,), fill_nan=True),
            "layer_reg_ptr": api.DeviceArray((2 * R * H + 4,), fill_nan=True)}
    for bad in bufs:
        for off in (4, 8):
            kw = {k: v.ptr + (off if k == bad else 0) for k, v in bufs.items()}
            with pytest.raises(api.DinoError) as e:
                sess.predict_layers_device(x.ptr, 1, 56, 84, [1, L], **kw)
            assert e.value.status == 4 and "aligned" in str(e.value), (bad, off)
    sess.sync()
    for k, v in bufs.items():
        assert np.isnan(v.to_host()).all(), k
    sess.predict_layers_device(x.ptr, 1, 56, 84, [1, L], **{k: v.ptr for k, v in bufs.items()})
    sess.sync()
    host = as_got(api.Session(model).predict_layers(imgs, [1, L], return_class_token=True, return_registers=True))
    ok, msg = mc.check_exact(bufs["layer_cls_ptr"].to_host()[:2 * H].reshape(2, 1, H), host["cls"], "aligned call after the refused ones")
    assert ok, msg


def test_raw_u8_layout(api, golden_dir):
    """Raw 8-bit input: the grid comes from dinov2_hip_preprocess_size; the taps equal those of the host-preprocessed image."""
    gguf, model = _model(api, golden_dir, "tiny_gelu_reg4")
    L = int(model.hparams.num_hidden_layers)
    raw = np.random.default_rng(4).integers(0, 256, size=(2, 50, 75, 3), dtype=np.uint8)
    pre = np.stack([api.dino_preprocess(r) for r in raw])
    sess = api.Session(model)
    a = as_got(sess.predict_layers(raw, [1, L], layout=api.U8_BGR_HWC, return_class_token=True, reshape=True))
    b = as_got(sess.predict_layers(pre, [1, L], layout=api.BGR_HWC, return_class_token=True, reshape=True))
    assert a["patch"].shape == b["patch"].shape and a["patch"].shape[-2:] == (pre.shape[1] // 14, pre.shape[2] // 14)
    for k in a:
        assert not np.isnan(a[k]).any()
        ok, msg = mc.check_exact(a[k], b[k], f"raw u8 vs host preprocess, {k}")
        assert ok, msg


def test_same_results_with_graphs_enabled(golden_dir):
    """DINOV2_HIP_GRAPHS=1 (read once per process, hence the subprocess): predict_layers between captured / replayed predicts gives the
    bits of a process without graphs, into whichever buffers the caller names, and does not disturb the replays."""
    import subprocess
    import sys
    code = r'''
import sys, numpy as np, torch
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
load_package(); api = import_module(PKG_NAME + ".api")
sess = api.Session(api.Model(sys.argv[1], classify=True))
x = torch.randn(3, 3, 70, 98, generator=torch.Generator().manual_seed(1)).cuda()
def plain():
    lo = torch.empty(3, 10, device="cuda")
    sess.predict_device(x.data_ptr(), 3, 70, 98, classify=True, logits_ptr=lo.data_ptr()); sess.sync()
    return lo.cpu().numpy()
def taps():
    p = torch.full((2, 3, 35, 128), float("nan"), device="cuda"); torch.cuda.synchronize()
    sess.predict_layers_device(x.data_ptr(), 3, 70, 98, [1, 2], classify=True, layer_patch_ptr=p.data_ptr()); sess.sync()
    return p.cpu().numpy()
r = [plain(), plain(), taps(), plain(), taps(), plain()]
assert all(np.array_equal(r[0], r[i]) for i in (1, 3, 5))
assert np.array_equal(r[2], r[4]) and not np.isnan(r[2]).any()
np.save(sys.argv[2], r[2]); print("LAYERS_OK")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    outs = []
    with tempfile.TemporaryDirectory() as td:
        for graphs in ("1", "0"):
            f = os.path.join(td, f"taps{graphs}.npy")
            out = subprocess.run([sys.executable, "-c", code, os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), f], cwd=root,
                                 env=dict(os.environ, DINOV2_HIP_GRAPHS=graphs), capture_output=True, text=True, timeout=600)
            assert "LAYERS_OK" in out.stdout, out.stdout + out.stderr
            outs.append(np.load(f))
    ok, msg = mc.check_exact(outs[0], outs[1], "graphs on vs off")
    assert ok, msg


# ----------------------------------------------------------------------------------------------------------- unchanged forward
@pytest.mark.parametrize("fold", [-1, 1])
def test_launch_counts_with_and_without_taps(api, golden_dir, fold):
    """A plain predict launches what DESIGN.md section 3 states and no tap; predict_layers with k taps launches exactly k more, all of the
    new kind.  Reconciling the numbers: DESIGN.md counts 3 + 7 L + 4 kernels (3 + 1 + 5 L + 4 with ln_fold), the "+ 4" being the final
    LayerNorm and the head's three kernels; the profile counts LOGICAL launches (one record per Scope in csrc/model.cpp), so the head is one
    entry and the sum asserted here is 3 + 7 L + 2 (3 + 1 + 5 L + 2).  For the same reason a GEMM whose plan hands left-over row panels to
    the small-tile kernel (ViT-L's QKV, "+ 24") is still one record of its kind: the per-kind dictionary is what pins the forward."""
    gguf, model = _model(api, golden_dir, "tiny_gelu_reg4", F16, fold)
    L = int(model.hparams.num_hidden_layers)
    imgs = np.random.default_rng(2).standard_normal((2, 3, 56, 84)).astype(np.float32)
    sess = api.Session(model)
    sess.predict(imgs, classify=True)
    sess.profile(True)
    sess.predict(imgs, classify=True)
    plain = {k: n for k, (ms, n) in sess.profile_read().items()}
    sess.profile(True)
    sess.predict_layers(imgs, [0, 1, L], classify=True, return_class_token=True)
    tapped = {k: n for k, (ms, n) in sess.profile_read().items()}
    sess.profile(False)
    assert list(plain)[-1] == "layer_tap" and plain["layer_tap"] == 0
    exp = {"im2col": 1, "init_tokens": 1, "gemm_patch_embed": 1, "layernorm": 1 if fold == 1 else 2 * L, "gemm_qkv": L, "attention": L,
           "gemm_attn_out": L, "gemm_ffn_in": L, "gemm_ffn_out": L, "final_layernorm": 1, "head": 1, "layer_tap": 0}
    assert plain == exp, plain
    assert sum(plain.values()) == (3 + 1 + 5 * L if fold == 1 else 3 + 7 * L) + 2
    assert tapped == dict(exp, layer_tap=3), tapped


# ------------------------------------------------------------------------------------------------------------------ references
def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("name", FIXTURES)
def test_raw_taps_against_the_oracle(api, golden_dir, name):
    """The bound of tests/test_gpu_parity.py::test_hidden_states_per_layer: 1e-5 for layer 0, 3e-3 relative after it."""
    gguf, model = _model(api, golden_dir, name, classify=False)
    L, R = int(model.hparams.num_hidden_layers), int(model.hparams.num_register_tokens)
    img = np.load(os.path.join(golden_dir, name + ".npz"))["img_56x84"]
    exp = OracleModel(gguf).forward(img, hidden=True)["hidden"]
    r = api.Session(model).predict_layers(img[None], list(range(L + 1)), norm=False, return_class_token=True, return_registers=R > 0)
    for layer, d in enumerate(r["layers"]):
        got = np.concatenate([d["cls"][0][None]] + ([d["registers"][0]] if R else []) + [d["patch_tokens"][0]])
        e = _rel(got, exp[layer])
        print(f"{name} layer {layer}: rel {e:.3e}")
        assert e <= (1e-5 if layer == 0 else 3e-3), f"layer {layer}: {e}"


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("name", FIXTURES)
def test_normalised_taps_against_float64_of_the_oracle(api, golden_dir, name, dt):
    """ln_reference (float64) of the oracle's hidden states; the project's token bound 5e-3 * max(1, max|ref|), 8 x that in bf16."""
    gguf, model = _model(api, golden_dir, name, dt, classify=False)
    L, R = int(model.hparams.num_hidden_layers), int(model.hparams.num_register_tokens)
    img = np.load(os.path.join(golden_dir, name + ".npz"))["img_56x84"]
    lw, lb = final_ln(gguf)
    hid = OracleModel(gguf).forward(img, hidden=True)["hidden"]
    r = api.Session(model).predict_layers(img[None], list(range(L + 1)), norm=True, return_class_token=True, return_registers=R > 0)
    for layer, d in enumerate(r["layers"]):
        ref = mc.ln_reference(hid[layer], lw, lb, EPS)
        got = np.concatenate([d["cls"][0][None]] + ([d["registers"][0]] if R else []) + [d["patch_tokens"][0]])
        bound = 5e-3 * max(1.0, float(np.abs(ref).max())) * (8 if dt == BF16 else 1)
        e = float(np.abs(got - ref).max())
        print(f"{name} dt={dt} layer {layer}: max|d| {e:.3e} bound {bound:.3e}")
        assert e <= bound, f"layer {layer}: {e} > {bound}"


@pytest.mark.parametrize("name", FIXTURES)
def test_taps_against_huggingface_hidden_states(api, golden_dir, name):
    """The HuggingFace hidden states stored with the fixture (hidden_<size>, final_<size>: an independent f32 implementation).  No existing
    test bounds the HIP path against them, so the bound is derived: the ggml-mode oracle's own distance from the fixture, measured here on
    the CPU for this image, plus the HIP-vs-oracle bounds of the two tests above (triangle inequality)."""
    gguf, model = _model(api, golden_dir, name, classify=False)
    L, R = int(model.hparams.num_hidden_layers), int(model.hparams.num_register_tokens)
    gold = np.load(os.path.join(golden_dir, name + ".npz"))
    img, hf_hidden, hf_final = gold["img_56x84"], gold["hidden_56x84"], gold["final_56x84"]
    lw, lb = final_ln(gguf)
    hid = OracleModel(gguf).forward(img, hidden=True)["hidden"]
    raw = api.Session(model).predict_layers(img[None], list(range(L + 1)), norm=False, return_class_token=True, return_registers=R > 0)
    for layer, d in enumerate(raw["layers"]):
        got = np.concatenate([d["cls"][0][None]] + ([d["registers"][0]] if R else []) + [d["patch_tokens"][0]])
        d_oracle = float(np.abs(hid[layer] - hf_hidden[layer]).max())
        bound = d_oracle + (1e-5 if layer == 0 else 3e-3) * max(1.0, float(np.abs(hid[layer]).max()))
        e = float(np.abs(got - hf_hidden[layer]).max())
        assert e <= bound, f"layer {layer}: |HIP - HF| {e:.3e} > {bound:.3e} (oracle vs HF measured {d_oracle:.3e})"
    # the normalised last layer against HF's last_hidden_state (all T rows)
    last = api.Session(model).predict_layers(img[None], [L], norm=True, return_class_token=True, return_registers=R > 0)["layers"][0]
    got = np.concatenate([last["cls"][0][None]] + ([last["registers"][0]] if R else []) + [last["patch_tokens"][0]])
    ref = mc.ln_reference(hid[L], lw, lb, EPS)
    assert hf_final.shape == ref.shape, (hf_final.shape, ref.shape)
    d_oracle = float(np.abs(ref - hf_final).max())
    bound = d_oracle + 5e-3 * max(1.0, float(np.abs(ref).max()))
    e = float(np.abs(got - hf_final).max())
    assert e <= bound, f"final: |HIP - HF| {e:.3e} > {bound:.3e} (ln_reference(oracle) vs HF measured {d_oracle:.3e})"


# ------------------------------------------------------------------------------------------------------------------- full size
def test_full_size_vit_large_chw_device_outputs(api, pkg, tmp_path):
    """Synthetic ViT-L/14 + 4 registers @518 (P = 1 369, odd: the CHW runs of consecutive channels start at every alignment), batch 2,
    layers [5, 12, 18, 24], CHW, device outputs: equal to debug_hidden through the final LayerNorm kernel, permuted; layer 24 equal to
    predict's own outputs."""
    path = str(tmp_path / "large.gguf")
    pkg.synth.write_synthetic_gguf(path, "large", registers=4, num_classes=1000, seed=42)
    imgs = pkg.synth.synthetic_images(2, 518, 518, seed=3)
    model = api.Model(path, classify=False)
    layers, L, R, H, h0 = [5, 12, 18, 24], 24, 4, 1024, 37
    lw, lb = final_ln(path)
    sess = api.Session(model)
    x = api.DeviceArray.from_host(imgs)
    patch = api.DeviceArray((4, 2, H, h0, h0), fill_nan=True)
    cls = api.DeviceArray((4, 2, H), fill_nan=True)
    reg = api.DeviceArray((4, 2, R, H), fill_nan=True)
    sess.predict_layers_device(x.ptr, 2, 518, 518, layers, norm=True, reshape=True, layer_patch_ptr=patch.ptr,
                               layer_cls_ptr=cls.ptr, layer_reg_ptr=reg.ptr)
    sess.sync()
    got = {"patch": patch.to_host(), "cls": cls.to_host(), "reg": reg.to_host()}
    ref_sess = api.Session(model)
    stream = np.zeros((L + 1, 2, 1 + R + h0 * h0, H), np.float32)
    for layer in layers:
        stream[layer] = op_layernorm_f32(api, ref_sess.debug_hidden(imgs, layer), lw, lb)
    ok, msg = lc.check_taps(got, stream, layers, R, h0, h0, lc.CHW, "ViT-L @518 CHW")
    assert ok, msg
    plain = ref_sess.predict(imgs, classify=False)
    ok, msg = mc.check_exact(got["cls"][3], plain["cls"], "layer 24 cls vs predict")
    assert ok, msg
    ok, msg = mc.check_exact(got["patch"][3].reshape(2, H, h0 * h0).transpose(0, 2, 1), plain["patch_tokens"], "layer 24 patches vs predict")
    assert ok, msg


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_argument_errors_leave_buffers_and_session_alone(api, golden_dir):
    gguf, model = _model(api, golden_dir, "tiny_gelu_noreg")
    L, H = int(model.hparams.num_hidden_layers), int(model.hparams.hidden_size)
    imgs = np.random.default_rng(1).standard_normal((2, 3, 56, 84)).astype(np.float32)
    sess = api.Session(model)
    before = sess.predict(imgs, classify=False)
    patch = np.full((L + 2, 2, 24, H), 7.0, np.float32)
    cls = np.full((L + 2, 2, H), 7.0, np.float32)
    reg = np.full((L + 2, 2, 4, H), 7.0, np.float32)

    def call(ids, n=None, layout=0, registers=False, null_struct=False):
        arr = (C.c_int32 * max(len(ids), 1))(*ids) if ids is not None else None
        ly = api.Layers(arr, len(ids) if n is None else n, 1, layout, patch.ctypes.data, cls.ctypes.data,
                        reg.ctypes.data if registers else None, 0)
        i = api.Input(imgs.ctypes.data, 2, 56, 84, api.RGB_CHW, 0)
        err = C.create_string_buffer(256)
        rc = api.lib().dinov2_hip_predict_layers(sess._h, C.byref(i), None, None if null_struct else C.byref(ly), 0, err, len(err))
        return rc, err.value.decode()

    bad = {"null layers struct": dict(ids=[1], null_struct=True), "null list": dict(ids=None, n=1), "n_layers 0": dict(ids=[], n=0),
           "n_layers L + 2": dict(ids=list(range(L + 1)), n=L + 2), "layer -1": dict(ids=[-1, 1]), "layer L + 1": dict(ids=[1, L + 1]),
           "not ascending": dict(ids=[1, 1]), "descending": dict(ids=[2, 1]), "unknown layout": dict(ids=[1], layout=2),
           "registers on a register-free model": dict(ids=[1], registers=True)}
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == 4 and msg, (what, rc, msg)
        assert (patch == 7.0).all() and (cls == 7.0).all() and (reg == 7.0).all(), what
    rc, msg = call([0, L])
    assert rc == 0, msg
    after = sess.predict(imgs, classify=False)
    ok, msg = mc.check_exact(after["patch_tokens"], before["patch_tokens"], "predict after the refused calls")
    assert ok, msg
    ok, msg = mc.check_exact(patch[1], before["patch_tokens"], "valid call after the refused ones")
    assert ok, msg
