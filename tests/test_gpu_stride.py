"""dinov2_hip_load_opts.patch_stride on the device (cases and the identity behind them: tests/stride_cases.py).

A strided model on an image I must give, bit for bit, what the default model gives on the expanded image E -- the same col matrix, grid,
position embedding, M and kernel plans -- through every entry point; the strided im2col alone is held to a numpy gather; the oracle on E
bounds the strided forward at the project's parity bounds (tests/test_gpu_parity.py)."""
import os

import numpy as np
import pytest

import stride_cases as sc
from oracle.oracle import OracleModel
from test_gpu_ops import _p, _round

pytestmark = pytest.mark.gpu

F16, BF16 = 0, 1
P14 = 14
_models = {}


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _sess(api, path, dt=F16, stride=0, classify=True):
    """One (model, session) per (checkpoint, dtype, stride), shared by the tests of this file."""
    key = (path, dt, stride, classify)
    if key not in _models:
        m = api.Model(path, dtype=dt, classify=classify, patch_stride=stride)
        _models[key] = (m, api.Session(m))
    return _models[key]


def _tiny(golden_dir):
    return os.path.join(golden_dir, "tiny_gelu_reg4.gguf")


def _img(h, w, seed=0, B=1):
    return np.random.default_rng(1000 * h + w + seed).standard_normal((B, 3, h, w)).astype(np.float32)


def _as_layout(rgb, layout):
    return rgb if layout == 1 else np.ascontiguousarray(rgb[:, ::-1].transpose(0, 2, 3, 1))  # BGR interleaved


# ---------------------------------------------------------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("s,h,w", sc.FORWARD_14)
def test_forward_equals_default_on_expanded_image(api, golden_dir, dt, s, h, w):
    """predict (classify and features), both layouts: cls, patch_tokens, logits, probs; debug_hidden at layer 0 and the last layer."""
    (ms, ss), (md, sd) = _sess(api, _tiny(golden_dir), dt, s), _sess(api, _tiny(golden_dir), dt, 0)
    assert ms.patch_stride == s and md.patch_stride == P14
    rgb = _img(h, w, B=2)
    E = sc.expand(rgb, P14, s)
    h0, w0 = sc.grid(h, w, P14, s)
    assert ms.grid(h, w) == (h0, w0) == md.grid(*E.shape[2:]) and ms.tokens(h, w) == md.tokens(*E.shape[2:]) == 5 + h0 * w0
    for layout in (1, 0):
        for classify in (True, False):
            a = ss.predict(_as_layout(rgb, layout), classify=classify, layout=layout)
            b = sd.predict(_as_layout(E, layout), classify=classify, layout=layout)
            assert sorted(a) == sorted(b)
            assert a["patch_tokens"].shape == (2, h0 * w0 + (4 if classify else 0), 128)
            for k in a:
                assert np.array_equal(a[k], b[k]), (k, layout, classify)
    L = ms.hparams.num_hidden_layers
    for layer in (0, L):
        assert np.array_equal(ss.debug_hidden(rgb, layer), sd.debug_hidden(E, layer)), layer


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("s,h,w", [(7, 28, 42), (7, 70, 84), (2, 28, 42), (1, 14, 30)])
def test_layers_and_attention_equal_default_on_expanded_image(api, golden_dir, dt, s, h, w):
    (ms, ss), (md, sd) = _sess(api, _tiny(golden_dir), dt, s), _sess(api, _tiny(golden_dir), dt, 0)
    rgb = _img(h, w, seed=3, B=2)
    E = sc.expand(rgb, P14, s)
    h0, w0 = ms.grid(h, w)
    a = ss.predict_layers(rgb, [0, 1, 2], reshape=True, return_class_token=True, return_registers=True)
    b = sd.predict_layers(E, [0, 1, 2], reshape=True, return_class_token=True, return_registers=True)
    for la, lb in zip(a["layers"], b["layers"]):
        assert la["patch_tokens"].shape == (2, 128, h0, w0)
        for k in ("patch_tokens", "cls", "registers"):
            assert np.array_equal(la[k], lb[k]), k
    q = [0, 5 + h0 * w0 - 1]  # two query tokens: CLS and the last patch
    ra = ss.predict_attention(rgb, [1, 2], q)
    rb = sd.predict_attention(E, [1, 2], q)
    assert ra.shape == (2, 2, 2, 2, 5 + h0 * w0) and np.array_equal(ra, rb)


@pytest.mark.parametrize("s", [7, 2])
def test_predict_list_and_list_rows(api, golden_dir, s):
    """Three images of different sizes in one forward: each equals its batch-1 call, and the default model's list of the expanded images;
    the row offsets are those of the grids."""
    (ms, ss), (md, sd) = _sess(api, _tiny(golden_dir), F16, s), _sess(api, _tiny(golden_dir), F16, 0)
    sizes = [(28, 42), (14, 14), (42, 28)]
    imgs = [_img(h, w, seed=7)[0] for h, w in sizes]
    Es = [sc.expand(i, P14, s) for i in imgs]
    off = api.list_rows(ms, sizes)
    assert list(np.diff(off)) == [int(np.prod(sc.grid(h, w, P14, s))) for h, w in sizes]
    assert np.array_equal(off, api.list_rows(md, [e.shape[1:] for e in Es]))
    assert np.array_equal(api.list_rows(ms, sizes, classify=True), api.list_rows(md, [e.shape[1:] for e in Es], classify=True))
    for classify in (False, True):
        got = ss.predict_list(imgs, classify=classify)
        exp = sd.predict_list(Es, classify=classify)
        for k in got:
            if k == "patch_tokens":
                assert all(np.array_equal(x, y) for x, y in zip(got[k], exp[k]))
            else:
                assert np.array_equal(got[k], exp[k]), k
        offs = api.list_rows(ms, sizes, classify=classify)
        for i, im in enumerate(imgs):
            one = ss.predict(im[None], classify=classify)
            assert np.array_equal(got["patch_packed"][offs[i]:offs[i + 1]], one["patch_tokens"][0]) and np.array_equal(got["cls"][i], one["cls"][0])


def test_explicit_patch_size_is_the_default(api, golden_dir):
    (m14, s14), (m0, s0) = _sess(api, _tiny(golden_dir), F16, 14), _sess(api, _tiny(golden_dir), F16, 0)
    assert m14.patch_stride == m0.patch_stride == 14
    rgb = _img(56, 84, B=2)
    a, b = s14.predict(rgb, classify=True), s0.predict(rgb, classify=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("p,s,img_size,h,w", sc.SYNTH)
def test_synthetic_checkpoints(api, pkg, tmp_path, p, s, img_size, h, w):
    """Other patch sizes: 16 at strides 4 and 8, 8 at stride 1; 2, 3 and 7 at stride 1, 4 at stride 2, 6 at strides 2 and 3."""
    path = str(tmp_path / "synth.gguf")
    pkg.synth.write_synthetic_gguf(path, sc.synth_config(p, img_size), registers=2, num_classes=5)
    ms, md = api.Model(path, patch_stride=s), api.Model(path)
    rgb = _img(h, w, seed=p)
    E = sc.expand(rgb, p, s)
    assert ms.grid(h, w) == sc.grid(h, w, p, s) == md.grid(*E.shape[2:])
    a, b = api.Session(ms).predict(rgb, classify=True), api.Session(md).predict(E, classify=True)
    assert a["patch_tokens"].shape[1] == 2 + int(np.prod(ms.grid(h, w)))
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------- 2. oracle parity
@pytest.mark.parametrize("name", ["tiny_gelu_noreg", "tiny_gelu_reg4", "tiny_swiglu_reg4"])
def test_oracle_parity_on_expanded_image(api, golden_dir, name):
    """The oracle knows no stride: it runs on E.  The project's own bounds (tests/test_gpu_parity.py): logits 1e-3 relative, tokens and cls
    5e-3, layer-0 hidden 1e-5."""
    gguf = os.path.join(golden_dir, name + ".gguf")
    img = np.load(os.path.join(golden_dir, name + ".npz"))["img_56x84"]
    ms, ss = _sess(api, gguf, F16, 7)
    E = sc.expand(img, P14, 7)
    ora = OracleModel(gguf)
    exp = ora.forward(E, classify=True, hidden=True)
    got = ss.predict(img[None], classify=True)
    dl, dc, dp = _rel(got["logits"][0], exp["logits"]), _rel(got["cls"][0], exp["cls"]), _rel(got["patch_tokens"][0], exp["patch_tokens"])
    d0 = _rel(ss.debug_hidden(img[None], 0)[0], exp["hidden"][0])
    print("%s: logits %.3e  cls %.3e  tokens %.3e  hidden0 %.3e" % (name, dl, dc, dp, d0))
    assert got["patch_tokens"].shape[1] == exp["patch_tokens"].shape[0]
    assert dl <= 1e-3 and dc <= 5e-3 and dp <= 5e-3 and d0 <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 3. the kernel alone
def _op(api, dt, rgb, p, s, layout, Kpad=None):
    B, _, h, w = rgb.shape
    Kpad = Kpad or sc.kpad(p)
    h0, w0 = sc.grid(h, w, p, s)
    col = np.full((B * h0 * w0, Kpad), np.nan, np.float32)
    img = _as_layout(rgb, layout)
    rc = api.lib().dinov2_hip_op_im2col_stride(dt, _p(img), _p(col), B, h, w, p, s, Kpad, layout)
    return rc, col


KERNEL_CASES = [(P14, s, h, w) for s, h, w in sc.SIZES_14] + [(32, 16, 64, 400), (32, 1, 34, 321), (16, 4, 32, 48), (8, 1, 16, 20),
                                                              (33, 11, 55, 66), (14, 7, 518, 518)] + sc.SMALL_KERNEL


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("p,s,h,w", KERNEL_CASES)
def test_im2col_stride_bit_exact(api, dt, layout, p, s, h, w):
    """Every element of col equals the compute-type rounding of its pixel (one rounding), the K padding is exactly zero, every element is
    written (the op pre-fills NaN): both layouts, runs of one and of several workgroups, patch 32 at strides 16 and 1, and patch 33 at
    stride 11 -- the largest patch im2col_stride_ok admits; every (patch, stride) below patch 8 (stride_cases.SMALL_PS), a grid row of
    exactly one run and of a run plus two patches each."""
    assert sc.stride_ok(p, s, sc.kpad(p))
    rgb = (_img(h, w, seed=p + s, B=2) * 1.5).astype(np.float32)
    rc, col = _op(api, dt, rgb, p, s, layout)
    assert rc == 0
    ref = sc.col_reference(_round(rgb, dt), p, s, sc.kpad(p))
    assert np.array_equal(col, ref)
    assert not col[:, 3 * p * p:].any() and not np.signbit(col[:, 3 * p * p:]).any()


def test_im2col_stride_refuses_what_is_outside_its_limits(api):
    """Just outside im2col_stride_ok, by name of the launcher's check (hipErrorInvalidValue = 1), and its neighbour inside."""
    rgb = _img(68, 68)
    assert not sc.stride_ok(34, 17, sc.kpad(34)) and _op(api, F16, rgb, 34, 17, 1)[0] != 0
    assert sc.stride_ok(33, 11, sc.kpad(33)) and _op(api, F16, _img(66, 66), 33, 11, 1)[0] == 0
    assert _op(api, F16, _img(28, 28), 14, 3, 1)[0] != 0 and _op(api, F16, _img(28, 28), 14, 7, 1, Kpad=588)[0] != 0


@pytest.mark.parametrize("dt,layout", [(F16, 1), (BF16, 0)])
@pytest.mark.parametrize("p,s,h,w", [(P14, 7, 42, 154), (P14, 2, 16, 142), (P14, 1, 16, 141), (3, 1, 7, 33), (2, 1, 5, 24)],
                         ids=["7-42-154", "2-16-142", "1-16-141", "p3-1-7-33", "p2-1-5-24"])  # (the patch-14 cases keep their names)
def test_im2col_stride_nan_tracer(api, dt, layout, p, s, h, w):
    """One NaN in one pixel channel: exactly the col elements of the patches that cover the pixel turn NaN, each at its own (c, ky, kx);
    everything else keeps the bits of the clean launch.  Pixels: a corner (one patch), an interior pixel (the full (p / s)^2), the last
    column that only the first workgroup's run reads and the first that only the next one's does, the columns the two runs share, and one
    interior pixel in each of its three channels in turn (patch 3 = the channel count: only the (c, ky, kx) that turns NaN tells the
    channel index from the column inside the patch)."""
    rgb = _img(h, w, seed=11, B=2)
    rc, clean = _op(api, dt, rgb, p, s, layout)
    assert rc == 0 and not np.isnan(clean).any()
    r = sc.run(p, s)
    h0, w0 = sc.grid(h, w, p, s)
    assert w0 > r, "the case must span two runs"
    last_of_first = r * s - 1            # column r s - 1: under patches <= r - 1 only
    first_of_next = (r - 1) * s + p      # the first column patch r - 1 no longer covers
    pixels = [(0, 0, 0, 0), (1, 2, h - 1, w - 1), (0, 1, min(p - 1, h - 1), p - 1 + s), (1, 0, 0, last_of_first), (0, 2, h - 1, first_of_next),
              (1, 1, 1, r * s)] + [(0, c, min(p, h - 1), r * s + 1) for c in range(3)]
    for b, c, y, x in pixels:
        hit = sc.footprint(b, c, y, x, h, w, p, s)
        bad = rgb.copy()
        bad[b, c, y, x] = np.nan
        rc, col = _op(api, dt, bad, p, s, layout)
        assert rc == 0
        exp = np.zeros(col.shape, bool)
        for row, k in hit:
            exp[row, k] = True
        assert np.array_equal(np.isnan(col), exp), (b, c, y, x)
        assert np.array_equal(col[~exp], clean[~exp]), (b, c, y, x)
    assert len(sc.footprint(0, 0, 0, 0, h, w, p, s)) == 1
    if h >= 2 * p - s:
        assert len(sc.footprint(0, 1, p - 1, p - 1 + s, h, w, p, s)) == (p // s) ** 2
    assert {j for row, _ in sc.footprint(1, 0, 0, last_of_first, h, w, p, s) for j in [row % w0]} <= set(range(r))
    assert min(row % w0 for row, _ in sc.footprint(0, 2, h - 1, first_of_next, h, w, p, s)) >= r


# ---------------------------------------------------------------------------------------------------------------- 4. raw 8-bit input
@pytest.mark.parametrize("s", [7, 2])
def test_raw_u8_input(api, golden_dir, s):
    """The device preprocessing is untouched: a strided predict of a raw image of odd size equals the strided predict of its host
    preprocessing, features mode and classify mode."""
    ms, ss = _sess(api, _tiny(golden_dir), F16, s)
    raw = np.random.default_rng(5).integers(0, 256, (1, 45, 61, 3), dtype=np.uint8)
    for classify, pre in ((False, api.dino_preprocess), (True, api.dino_classify_preprocess)):
        f32 = pre(raw[0], P14)
        a = ss.predict(raw, classify=classify, layout=api.U8_BGR_HWC)
        b = ss.predict(f32[None], classify=classify, layout=api.BGR_HWC)
        h0, w0 = ms.grid(*f32.shape[:2])
        assert a["patch_tokens"].shape[1] == h0 * w0 + (4 if classify else 0)
        assert all(np.array_equal(a[k], b[k]) for k in a), classify


# ---------------------------------------------------------------------------------------------------------------- 5. consumers
def test_consumers_see_the_grid(api, golden_dir):
    """pca3, match and kmeans on the resident tokens of a stride-7 predict, predict_dense, and a one-device Group."""
    (ms, ss), (md, sd) = _sess(api, _tiny(golden_dir), F16, 7), _sess(api, _tiny(golden_dir), F16, 0)
    h, w = 56, 84
    rgb = _img(h, w, seed=2, B=2)
    E = sc.expand(rgb, P14, 7)
    h0, w0 = ms.grid(h, w)
    P, H = h0 * w0, 128
    assert (h0, w0) == (7, 11)
    res = []
    for sess, x in ((ss, rgb), (sd, E)):
        sess.predict(x, classify=False)
        pca = sess.pca3(None, shape=(P, H))
        mt = sess.match(shape=(P, H))
        km = sess.kmeans(source="last_patches", K=4, max_iter=5, seed=1)
        res.append((pca, mt, km))
    (pa, ma, ka), (pb, mb, kb) = res
    assert pa[2].shape == (P, 3) and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert ma["idx_ab"].shape == (P,) and all(np.array_equal(ma[k], mb[k]) for k in ma)
    assert ka["labels"].shape == (P,) and all(np.array_equal(ka[k], kb[k]) for k in ("labels", "sim", "centers", "counts"))
    W = np.random.default_rng(3).standard_normal((5, 2 * H)).astype(np.float32)
    da = ss.predict_dense(rgb, api.DenseHead(ms, [1, 2], W), out_size=(40, 60))
    db = sd.predict_dense(E, api.DenseHead(md, [1, 2], W), out_size=(40, 60))
    assert da["logits"].shape == (2, P, 5) and da["labels"].shape == (2, 40, 60)
    assert all(np.array_equal(da[k], db[k]) for k in ("labels", "value", "logits"))
    grp = api.Group(_tiny(golden_dir), devices=[0], classify=True, patch_stride=7)
    assert grp.patch_stride == 7
    ga, sa = grp.predict(rgb, classify=True), ss.predict(rgb, classify=True)
    assert ga["patch_tokens"].shape == (2, 4 + P, H) and all(np.array_equal(ga[k], sa[k]) for k in sa)
    grp.close()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_input_sizes_are_checked_against_patch_and_stride(api, golden_dir):
    (m14, s14), (m7, s7) = _sess(api, _tiny(golden_dir), F16, 0), _sess(api, _tiny(golden_dir), F16, 7)
    for model, sess, (h, w), stride in ((m14, s14, (21, 28), 14), (m7, s7, (20, 28), 7)):
        for call in (lambda: sess.predict(_img(h, w)), lambda: model.grid(h, w), lambda: sess.debug_hidden(_img(h, w), 0)):
            with pytest.raises(api.DinoError) as e:
                call()
            assert e.value.status == 4 and "patch_size 14" in str(e.value) and "patch_stride %d" % stride in str(e.value)
    assert m7.grid(21, 28) == (2, 3) and s7.predict(_img(21, 28))["patch_tokens"].shape == (1, 6, 128)
    with pytest.raises(api.DinoError):
        m7.grid(7, 28)  # below the patch size


def test_largest_patch_loads_at_its_strides(api, pkg, tmp_path):
    """The neighbours inside the limits: patch 32 at strides 16 and 1 load and run."""
    path = str(tmp_path / "p32.gguf")
    pkg.synth.write_synthetic_gguf(path, sc.synth_config(32, 64), registers=0, num_classes=3)
    md = api.Session(api.Model(path))
    for s in (16, 1):
        m = api.Model(path, patch_stride=s)
        rgb = _img(48, 64 if s == 16 else 40, seed=s)
        a, b = api.Session(m).predict(rgb, classify=True), md.predict(sc.expand(rgb, 32, s), classify=True)
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_single_image_limit_of_a_pass(api, pkg, tmp_path):
    """An image whose own token rows times the widest activation row times 2 bytes reach 2^31 is refused by every predict entry point
    before anything is allocated or launched; just below the limit the checks pass (attention over one image of that size is run by case A2 of tests/test_gpu_far.py)."""
    path = str(tmp_path / "small1.gguf")
    pkg.synth.write_synthetic_gguf(path, "small", registers=4, num_classes=10, layers=1)
    model = api.Model(path, patch_stride=1)
    sess = api.Session(model)
    hp = model.hparams
    assert max(3 * hp.hidden_size, hp.ffn_hidden) == sc.SMALL_WIDEST
    n, u = sc.OVER, sc.UNDER
    assert model.grid(u, u) == (u - 13, u - 13) and model.tokens(u, u) == 698901 and model.workspace_bytes(1, u, u) > 0
    assert model.workspace_bytes(1, n, n) == 0
    with pytest.raises(api.DinoError) as e:
        model.grid(n, n)
    assert e.value.status == 4 and "too many token rows for one pass" in str(e.value) and "702249" in str(e.value)
    big = np.zeros((1, 3, n, n), np.float32)
    head = api.DenseHead(model, [1], np.zeros((3, hp.hidden_size), np.float32))
    grp = api.Group(path, devices=[0], classify=True, patch_stride=1)
    sess.predict(np.zeros((1, 3, 28, 28), np.float32))  # a session in use: a workspace and a last forward exist
    sess.profile(True)
    calls = {"predict": lambda: sess.predict(big), "classify": lambda: sess.predict(big, classify=True),
             "layers": lambda: sess.predict_layers(big, [1]), "attention": lambda: sess.predict_attention(big, [1]),
             "dense": lambda: sess.predict_dense(big, head, out_size=(8, 8)), "hidden": lambda: sess.debug_hidden(big, 0),
             "list": lambda: sess.predict_list([big[0]]), "group": lambda: grp.predict(big)}
    for name, call in calls.items():
        with pytest.raises(api.DinoError) as e:
            call()
        assert e.value.status == 4 and "too many token rows for one pass" in str(e.value), name
    assert all(v[1] == 0 for v in sess.profile_read().values()), "a refused call launched something"
    sess.profile(False)
    assert sess.predict(np.zeros((1, 3, 28, 28), np.float32))["patch_tokens"].shape == (1, 225, 384)  # and the session still works
    grp.close()


# ---------------------------------------------------------------------------------------------------------------- 7. nothing moved
@pytest.mark.parametrize("stride", [0, 14, 7])
def test_profile_lists_the_launches(api, golden_dir, stride):
    """patch_stride 0 or 14: the kinds and launch counts of a predict are what they were -- im2col once, no strided kernel in the list.
    A smaller stride: the strided kernel once instead, everything else the same."""
    model, sess = _sess(api, _tiny(golden_dir), F16, stride)
    L = model.hparams.num_hidden_layers
    rgb = _img(56, 84, B=2)
    sess.predict(rgb, classify=True)
    sess.profile(True)
    sess.predict(rgb, classify=True)
    got = {k: n for k, (ms, n) in sess.profile_read().items()}
    sess.profile(False)
    exp = {"im2col": 1, "init_tokens": 1, "gemm_patch_embed": 1, "layernorm": 2 * L, "gemm_qkv": L, "attention": L, "gemm_attn_out": L,
           "gemm_ffn_in": L, "gemm_ffn_out": L, "final_layernorm": 1, "head": 1, "layer_tap": 0}
    if stride == 7:
        exp.update(im2col=0, im2col_stride=1)
    if got["layernorm"] != 2 * L:  # (DINOV2_HIP_LN_FOLD=1 in the environment: one ln_prepare launch instead)
        exp["layernorm"] = 1
    assert list(got) == list(exp) and got == exp, got
