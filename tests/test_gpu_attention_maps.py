"""dinov2_hip_predict_attention (include/dinov2_hip.h): the attention rows of chosen query tokens from one ordinary forward.

  * bit-exact chain (ln_fold off): debug_hidden(k - 1) -> op_layernorm(norm1 of block k) -> op_gemm(EPI_QKV, qscale = 0.125 log2 e) ->
    op_attn_rows equals predict_attention's layer k (every GEMM plan gives the same bits, so the op's plan need not match the forward's);
  * an independent float64 softmax((ln W_q^T + b_q)(ln W_k^T + b_k)^T / 8) under a derived bound, ln_fold off and on;
  * plumbing: predict's outputs and predict_layers' taps from the same call, PATCHES = columns of ALL, host = device, split batches,
    raw 8-bit input, graphs, fetch and pca3 afterwards, profile counts, argument errors.
All of them need the entry point, which does not exist before this feature: they fail there."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_cases as ac
import attn_row_cases as rc
from oracle.gguf_np import GGUFFile

pytestmark = pytest.mark.gpu

F16, BF16 = 0, 1
FIXTURES = ["tiny_gelu_noreg", "tiny_gelu_reg4", "tiny_swiglu_reg4"]
SIZES = [(70, 70), (56, 84)]
EPI_QKV = 1
EPS = 1e-6
QSCALE = 0.125 * math.log2(math.e)
fp = C.POINTER(C.c_float)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(fp)


def _block(gguf, k):
    """norm1 and the fused qkv projection of block k (1-based), f32."""
    t = GGUFFile(gguf).tensors
    b = "encoder.layer.%d." % (k - 1)
    g = lambda n: np.ascontiguousarray(t[b + n].to_f32(), np.float32)  # noqa: E731
    W = g("attention.attention.qkv.weight")
    return g("norm1.weight").reshape(-1), g("norm1.bias").reshape(-1), W.reshape(-1, W.shape[-1]), g("attention.attention.qkv.bias").reshape(-1)


def _op_layernorm(api, dt, x, w, b):
    rows = np.ascontiguousarray(x.reshape(-1, x.shape[-1]), np.float32)
    out = np.empty_like(rows)
    assert api.lib().dinov2_hip_op_layernorm(dt, _p(rows), _p(w), _p(b), _p(out), rows.shape[0], rows.shape[1], EPS) == 0
    return out


def _op_qkv(api, dt, ln, W, bias):
    M, H = ln.shape
    qkv = np.zeros((M, 3 * H), np.float32)
    assert api.lib().dinov2_hip_op_gemm(dt, EPI_QKV, _p(ln), _p(W), _p(bias), fp(), 0, _p(qkv), M, 3 * H, M, 3 * H, H, 0, 0, 0, H, QSCALE) == 0
    return qkv


def _queries(R, T):
    return sorted({0, 1 if R else 2, 1 + R, T - 1} & set(range(T)))  # CLS, a register (or a patch), first and last patch


@pytest.fixture(scope="module")
def small3(tmp_path_factory, pkg):
    """hidden 384 / 6 heads / 3 layers, 4 registers."""
    path = str(tmp_path_factory.mktemp("attn") / "small3.gguf")
    pkg.synth.write_synthetic_gguf(path, "small", registers=4, num_classes=10, layers=3, seed=5)
    return path


def _cases(golden_dir, small3):
    for name in FIXTURES:
        for hw in SIZES:
            yield os.path.join(golden_dir, name + ".gguf"), hw
    yield small3, (126, 98)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_bit_exact_chain(api, golden_dir, small3, dt):
    for gguf, (hh, ww) in _cases(golden_dir, small3):
        model = api.Model(gguf, dtype=dt, classify=False, ln_fold=-1)
        hp = model.hparams
        L, R, nh = int(hp.num_hidden_layers), int(hp.num_register_tokens), int(hp.num_attention_heads)
        imgs = np.random.default_rng(hh).standard_normal((2, 3, hh, ww)).astype(np.float32)
        T = 1 + R + (hh // 14) * (ww // 14)
        qs = _queries(R, T)
        sess = api.Session(model)
        got = sess.predict_attention(imgs, list(range(1, L + 1)), qs)
        assert got.shape == (L, 2, nh, len(qs), T)
        dbg = api.Session(model)
        for k in range(1, L + 1):
            w1, b1, W, bias = _block(gguf, k)
            ln = _op_layernorm(api, dt, dbg.debug_hidden(imgs, k - 1), w1, b1)
            rows = api.op_attn_rows(dt, _op_qkv(api, dt, ln, W, bias), 2, T, nh, qs)
            ok, msg = rc.check_exact(got[k - 1], rows, "%s %dx%d layer %d" % (os.path.basename(gguf), hh, ww, k))
            assert ok, msg


def _float64_bound(ln, dln, W, bias, dt, B, T, nh, qs):
    """Float64 softmax((ln W_q^T + b_q)(ln W_k^T + b_k)^T / 8) and the bound on |library - it|, as
    tests/test_gpu_attention.py::test_qkv_gemm_then_log2_attention derives it.  ln [M, H] float64 is the GEMM's A operand as the reference
    sees it and dln >= 0 [M, H] the absolute error of the operand the library really multiplies (0 when ln IS that operand).  Per element of
    q and k before their rounding:  a = dln |W|^T  (operand error)  +  (K + 2) 2^-24 (|ln| |W|^T + |b|)  (f32 accumulation of the K-deep
    GEMM, bias add).  Stored q: relative u + 2^-22 (scale product, rounding) on top; stored k: relative u.  Scores in natural units move by
        ds <= max_j sum_d (|q_d| + dq_d)(|k_jd| + dk_jd) - |q_d k_jd|,
    which moves a probability by at most 2 ds e^(2 ds) relative; the kernel's own error on the stored operands (attn_row_cases.error_bound,
    evaluated at the perturbed P, S, M) is added."""
    u = ac.U[dt]
    H = nh * 64
    W = np.asarray(W, np.float64)
    y = ln @ W[:2 * H].T + bias[:2 * H]
    a = dln @ np.abs(W[:2 * H]).T + (H + 2) * 2.0 ** -24 * (np.abs(ln) @ np.abs(W[:2 * H]).T + np.abs(bias[:2 * H]))
    sp = lambda z: z.reshape(B, T, nh, 64).transpose(0, 2, 1, 3)  # noqa: E731
    q, k = sp(y[:, :H] / 8.0), sp(y[:, H:])
    dq = np.abs(q) * (u + 2.0 ** -22) + sp(a[:, :H] / 8.0) * (1 + u)
    dk = np.abs(k) * u + sp(a[:, H:]) * (1 + u)
    qq, dqq = q[:, :, qs], dq[:, :, qs]
    s = qq @ k.transpose(0, 1, 3, 2)
    S = np.abs(qq) @ np.abs(k).transpose(0, 1, 3, 2)
    ds = ((np.abs(qq) + dqq) @ (np.abs(k) + dk).transpose(0, 1, 3, 2) - S).max(-1, keepdims=True)
    Mx = s.max(-1, keepdims=True)
    p = np.exp(s - Mx)
    P = p / p.sum(-1, keepdims=True)
    r = 2 * ds * np.exp(2 * ds)
    kb = rc.error_bound(P * (1 + r), (S.max(-1, keepdims=True) + ds) * ac.LOG2E, (np.abs(Mx) + ds) * ac.LOG2E, T)
    return P, kb + P * r


@pytest.mark.parametrize("fold", [-1, 1], ids=["nofold", "fold"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_float64_reference(api, golden_dir, small3, dt, fold):
    """ln_fold off: ln = the LayerNorm kernel's own output (rounded to T), exactly the GEMM's operand, dln = 0.  ln_fold on: the GEMM
    multiplies T(gamma x) and applies mean, rstd and beta in its epilogue -- the fold's own rounding point: ln = float64 LayerNorm of the
    f32 residual stream, and the operand's rounding is dln = rstd u |gamma x| per element (u = 2^-11 in f16, the fold's documented
    per-element rounding), plus the f32 row statistics, 2^-22 relative on |gamma x| rstd + |ln|."""
    u = ac.U[dt]
    for gguf, (hh, ww) in _cases(golden_dir, small3):
        model = api.Model(gguf, dtype=dt, classify=False, ln_fold=fold)
        hp = model.hparams
        L, R, nh = int(hp.num_hidden_layers), int(hp.num_register_tokens), int(hp.num_attention_heads)
        imgs = np.random.default_rng(ww).standard_normal((2, 3, hh, ww)).astype(np.float32)
        T = 1 + R + (hh // 14) * (ww // 14)
        qs = _queries(R, T)
        got = api.Session(model).predict_attention(imgs, list(range(1, L + 1)), qs)
        dbg = api.Session(model)
        for k in range(1, L + 1):
            w1, b1, W, bias = _block(gguf, k)
            x = dbg.debug_hidden(imgs, k - 1).reshape(-1, len(w1)).astype(np.float64)
            if fold == 1:
                mu = x.mean(-1, keepdims=True)
                rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + EPS)
                ln = (x - mu) * rstd * w1 + b1
                dln = rstd * np.abs(x * w1) * (u + 2.0 ** -22) + 2.0 ** -22 * np.abs(ln)
            else:
                ln = _op_layernorm(api, dt, x.astype(np.float32), w1, b1).astype(np.float64)
                dln = np.zeros_like(ln)
            P, bound = _float64_bound(ln, dln, ac.round_t(W, dt), bias.astype(np.float64), dt, 2, T, nh, qs)
            what = "%s %dx%d layer %d" % (os.path.basename(gguf), hh, ww, k)
            ok, msg = rc.check_against_reference(got[k - 1], P, bound, what)
            print(msg)
            assert ok, msg
            ok, msg = rc.check_rows_sum_to_one(got[k - 1], T, what)
            assert ok, msg


@pytest.mark.parametrize("dt,fold", [(F16, -1), (BF16, 1)])
def test_outputs_taps_views_and_device_path(api, golden_dir, dt, fold):
    gguf = os.path.join(golden_dir, "tiny_gelu_reg4.gguf")
    model = api.Model(gguf, dtype=dt, classify=True, ln_fold=fold)
    L, R, nh, H = 2, 4, 2, int(model.hparams.hidden_size)
    imgs = np.random.default_rng(9).standard_normal((3, 3, 56, 84)).astype(np.float32)
    T, P = 29, 24
    qs = [0, 2, 5, T - 1]
    sess = api.Session(model)
    rows, out = sess.predict_attention(imgs, [1, 2], qs, taps=[0, 2], classify=True)
    plain = api.Session(model).predict(imgs, classify=True)
    for key in ("logits", "probs", "cls", "patch_tokens"):
        ok, msg = rc.check_exact(out[key], plain[key], "out.%s of predict_attention vs predict" % key)
        assert ok, msg
    taps = api.Session(model).predict_layers(imgs, [0, 2], classify=True)
    for a, b in zip(out["layers"], taps["layers"]):
        ok, msg = rc.check_exact(a["patch_tokens"], b["patch_tokens"], "tap of layer %d vs predict_layers" % a["layer"])
        assert ok, msg
    assert rows.shape == (2, 3, nh, 4, T) and np.isfinite(rows).all()
    ok, msg = rc.check_exact(sess.predict_attention(imgs, [1, 2], qs), rows, "without taps vs with taps")
    assert ok, msg
    ok, msg = rc.check_exact(sess.predict_attention(imgs, [1, 2], qs, keys="patches"), rows[..., 1 + R:], "PATCHES vs columns of ALL")
    assert ok, msg
    ok, msg = rc.check_exact(sess.predict_attention(imgs, 2)[0], rows[1][:, :, :1], "default query = the CLS row; one layer")
    assert ok, msg
    ok, msg = rc.check_exact(sess.predict_attention(imgs, [2], [5])[0], rows[1][:, :, 2:3], "one layer, one query")
    assert ok, msg
    ok, msg = rc.check_exact(sess.predict_attention(imgs[1:2], [1, 2], qs), rows[:, 1:2], "image 1 alone vs in the batch")
    assert ok, msg
    # device path: the kernel writes into the caller's buffer
    x = api.DeviceArray.from_host(imgs)
    for keys, ref in (("all", rows), ("patches", rows[..., 1 + R:])):
        d = api.DeviceArray(ref.shape, fill_nan=True)
        sess.predict_attention_device(x.ptr, 3, 56, 84, [1, 2], d, qs, keys)
        sess.sync()
        ok, msg = rc.check_exact(d.to_host(), ref, "device path, keys = %s" % keys)
        assert ok, msg
    # afterwards fetch and pca3(tokens = NULL) behave as after a predict of the same shape
    o = api.Output()
    c = np.empty((3, H), np.float32)
    o.cls = c.ctypes.data
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_fetch(sess._h, C.byref(o), err, len(err)) == 0, err.value
    feats = api.Session(model)
    ok, msg = rc.check_exact(c, feats.predict(imgs, classify=False)["cls"], "fetch after predict_attention")
    assert ok, msg
    for a, b, what in zip(sess.pca3(None, (P, H)), feats.pca3(None, (P, H)), ("components", "mean", "projection")):
        ok, msg = rc.check_exact(a, b, "pca3 %s after predict_attention" % what)
        assert ok, msg


def test_raw_u8_input(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    raw = np.random.default_rng(4).integers(0, 256, size=(2, 50, 75, 3), dtype=np.uint8)
    pre = np.stack([api.dino_preprocess(r) for r in raw])
    sess = api.Session(model)
    a = sess.predict_attention(raw, [1, 2], [0, 3], layout=api.U8_BGR_HWC)
    b = sess.predict_attention(pre, [1, 2], [0, 3], layout=api.BGR_HWC)
    assert a.shape[-1] == 1 + 4 + (pre.shape[1] // 14) * (pre.shape[2] // 14) and np.isfinite(a).all()
    ok, msg = rc.check_exact(a, b, "raw u8 vs host preprocess")
    assert ok, msg


_CHILD = r'''
import sys, numpy as np
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
load_package(); api = import_module(PKG_NAME + ".api")
sess = api.Session(api.Model(sys.argv[1], classify=True, ln_fold=int(sys.argv[3])))
imgs = np.random.default_rng(5).standard_normal((5, 3, 70, 98)).astype(np.float32)
sess.predict(imgs, classify=True); sess.predict(imgs, classify=True)
rows, out = sess.predict_attention(imgs, [1, 2], [0, 3, 39], taps=[1], classify=True)
again = sess.predict_attention(imgs, [1, 2], [0, 3, 39], classify=True)
assert np.array_equal(rows, again) and np.isfinite(rows).all()
np.savez(sys.argv[2], rows=rows, logits=out["logits"], tap=out["layers"][0]["patch_tokens"], patch=out["patch_tokens"]); print("ATTN_OK")
'''


@pytest.mark.parametrize("fold", [-1, 1])
def test_split_batches_and_graphs_in_child_processes(golden_dir, tmp_path, fold):
    """DINOV2_HIP_MAX_CHUNK and DINOV2_HIP_GRAPHS are read once per process, hence fresh children: a batch of 5 in passes of 2, 2, 1 and a
    process with graphs on give the bits of the plain process -- rows, taps and outputs."""
    res = {}
    for tag, env in (("plain", {}), ("split", {"DINOV2_HIP_MAX_CHUNK": "2"}), ("graphs", {"DINOV2_HIP_GRAPHS": "1"})):
        f = str(tmp_path / (tag + ".npz"))
        out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(golden_dir, "tiny_swiglu_reg4.gguf"), f, str(fold)], cwd=ROOT,
                             env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert "ATTN_OK" in out.stdout, tag + ": " + out.stdout + out.stderr
        res[tag] = np.load(f)
    for tag in ("split", "graphs"):
        for key in ("rows", "logits", "tap", "patch"):
            ok, msg = rc.check_exact(res[tag][key], res["plain"][key], "%s vs plain, %s" % (tag, key))
            assert ok, msg


@pytest.mark.parametrize("fold", [-1, 1])
def test_profile_counts(api, golden_dir, fold):
    """a attention layers and b taps: layer_tap reads a + b, every other kind what a plain predict gives; a plain predict reads 0; the list
    of kinds is what it was."""
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True, ln_fold=fold)
    L = 2
    imgs = np.random.default_rng(2).standard_normal((2, 3, 56, 84)).astype(np.float32)
    sess = api.Session(model)
    sess.predict(imgs, classify=True)
    sess.profile(True)
    sess.predict(imgs, classify=True)
    plain = {k: n for k, (ms, n) in sess.profile_read().items()}
    sess.profile(True)
    sess.predict_attention(imgs, [1, 2], [0, 7], taps=[0, 1, L], classify=True)
    both = {k: n for k, (ms, n) in sess.profile_read().items()}
    sess.profile(True)
    sess.predict_attention(imgs, [2], classify=True)
    one = {k: n for k, (ms, n) in sess.profile_read().items()}
    sess.profile(True)
    sess.predict(imgs, classify=True)
    after = {k: n for k, (ms, n) in sess.profile_read().items()}
    sess.profile(False)
    assert list(plain) == ["im2col", "init_tokens", "gemm_patch_embed", "layernorm", "gemm_qkv", "attention", "gemm_attn_out", "gemm_ffn_in",
                           "gemm_ffn_out", "final_layernorm", "head", "layer_tap"]
    assert plain["layer_tap"] == 0 and plain["attention"] == L and after == plain
    assert both == dict(plain, layer_tap=2 + 3), both
    assert one == dict(plain, layer_tap=1), one


def test_argument_errors(api, golden_dir):
    """Every refused call returns DINOV2_HIP_ERR_INVALID (4) with a message and leaves the output (a sentinel) untouched; the session stays
    usable."""
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    L, T, nh = 2, 29, 2
    imgs = np.random.default_rng(3).standard_normal((1, 3, 56, 84)).astype(np.float32)
    sess = api.Session(model)
    probs = np.full((L, 1, nh, 2, T), -7.0, np.float32)
    dev = api.DeviceArray((L * nh * 2 * T + 8,), fill_nan=True)
    x = api.DeviceArray.from_host(imgs)
    I32 = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def call(at, taps=None, device=False):
        i = api.Input(x.ptr if device else imgs.ctypes.data, 1, 56, 84, api.RGB_CHW, 1 if device else 0)
        err = C.create_string_buffer(512)
        rc_ = api.lib().dinov2_hip_predict_attention(sess._h, C.byref(i), None, C.byref(taps) if taps is not None else None,
                                                     C.byref(at) if at is not None else None, 0, err, len(err))
        return rc_, err.value.decode()

    def at(layers=(1, 2), n_layers=None, queries=(0, 3), n_queries=None, keys=0, ptr=probs.ctypes.data, on_device=0):
        la, qa = (I32(layers) if layers is not None else None), (I32(queries) if queries is not None else None)
        a = api.Attention(la, len(layers or ()) if n_layers is None else n_layers, qa, len(queries or ()) if n_queries is None else n_queries,
                          keys, ptr, on_device)
        a._keep = (la, qa)
        return a

    bad_taps = api.Layers(I32([2, 1]), 2, 1, 0, None, None, None, 0)
    cases = {
        "null attn": (None, None, False), "null layer list": (at(layers=None, n_layers=1), None, False),
        "null probs": (at(ptr=None), None, False), "n_layers 0": (at(n_layers=0), None, False),
        "n_layers > L": (at(layers=(1, 2, 3)), None, False), "layer 0": (at(layers=(0, 1)), None, False),
        "layer > L": (at(layers=(1, 3)), None, False), "layers descending": (at(layers=(2, 1)), None, False),
        "layers repeated": (at(layers=(1, 1)), None, False), "queries descending": (at(queries=(3, 0)), None, False),
        "query >= T": (at(queries=(0, T)), None, False), "negative query": (at(queries=(-1, 3)), None, False),
        "n_queries > T": (at(n_queries=T + 1), None, False), "null queries with a count": (at(queries=None, n_queries=2), None, False),
        "unknown keys": (at(keys=2), None, False), "misaligned device pointer": (at(ptr=dev.ptr + 4, on_device=1), None, True),
        "misaligned by 8": (at(ptr=dev.ptr + 8, on_device=1), None, True), "bad taps": (at(), bad_taps, False),
    }
    for name, (a, taps, device) in cases.items():
        status, msg = call(a, taps, device)
        assert status == 4 and msg, (name, status, msg)
    sess.sync()
    assert (probs == -7.0).all() and np.isnan(dev.to_host()).all()
    status, msg = call(at())
    assert status == 0, msg
    ok, msg = rc.check_exact(probs, api.Session(model).predict_attention(imgs, [1, 2], [0, 3]), "the accepted call after the refused ones")
    assert ok, msg
