"""GPU tests of dinov2_hip_predict_list (include/dinov2_hip.h): images of different sizes in one forward.  Contract: image i of a list has, BIT
FOR BIT, the outputs of Session.predict on that image alone -- cls, patch rows, logits, probs, top-k -- for both compute types, with and
without the head, with LN fold, for raw 8-bit input, for host and device outputs, whatever the order of the list.  One list is also held to the
CPU oracle with the shallow-model bounds of tests/test_gpu_parity.py (1e-3 logits, 5e-3 tokens, relative), which an error shared by both paths
would not pass.  Sizes and lists: tests/list_cases.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

import list_cases as lc
from oracle.oracle import OracleModel

pytestmark = pytest.mark.gpu

FIXTURES = ["tiny_gelu_noreg", "tiny_gelu_reg4", "tiny_swiglu_reg4"]
KEYS = ("cls", "logits", "probs", "topk_ids", "topk_probs")

_models, _alone_cache = {}, {}


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _model(api, golden_dir, name, dt=0, ln_fold=0, classify=True):
    key = (name, dt, ln_fold, classify)
    if key not in _models:
        _models[key] = api.Model(os.path.join(golden_dir, name + ".gguf"), dtype=dt, classify=classify, ln_fold=ln_fold)
    return _models[key]


def _images(sizes):
    return [lc.image(s, seed=i) for i, s in enumerate(sizes)]  # (a repeated size gets different pixels)


def _alone(api, golden_dir, name, dt, ln_fold, img, classify, seed_key):
    """Session.predict of one image alone; computed once per (model, image, flags) and left unchanged."""
    key = (name, dt, ln_fold, classify, seed_key, img.shape)
    if key not in _alone_cache:
        sess = api.Session(_model(api, golden_dir, name, dt, ln_fold))
        _alone_cache[key] = sess.predict(img[None], classify=classify, topk=3 if classify else 0)
    return _alone_cache[key]


def _assert_as_alone(api, golden_dir, name, dt, ln_fold, got, imgs, classify, tag=""):
    n = len(imgs)
    assert got["cls"].shape[0] == n and len(got["patch_tokens"]) == n and got["offsets"][-1] == got["patch_packed"].shape[0]
    for i, img in enumerate(imgs):
        exp = _alone(api, golden_dir, name, dt, ln_fold, img, classify, seed_key=hash(img.tobytes()))
        for k in KEYS if classify else ("cls",):
            assert np.array_equal(got[k][i], exp[k][0]), "%s image %d (%s): %s differs from predict alone" % (tag, i, img.shape, k)
        assert got["patch_tokens"][i].shape == exp["patch_tokens"][0].shape, (tag, i)
        assert np.array_equal(got["patch_tokens"][i], exp["patch_tokens"][0]), "%s image %d (%s): patch rows differ" % (tag, i, img.shape)


@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
@pytest.mark.parametrize("dt", [0, 1], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_every_image_equals_predict_alone(api, golden_dir, name, dt, classify):
    sess = api.Session(_model(api, golden_dir, name, dt))
    for lname, sizes in lc.LISTS.items():
        imgs = _images(sizes)
        got = sess.predict_list(imgs, classify=classify, topk=3 if classify else 0)
        _assert_as_alone(api, golden_dir, name, dt, 0, got, imgs, classify, tag=lname)


@pytest.mark.parametrize("name", FIXTURES)
def test_ln_fold_model(api, golden_dir, name):
    sess = api.Session(_model(api, golden_dir, name, 0, ln_fold=1))
    for lname in ("mixed", "repeat_apart"):
        imgs = _images(lc.LISTS[lname])
        _assert_as_alone(api, golden_dir, name, 0, 1, sess.predict_list(imgs, classify=True, topk=3), imgs, True, tag=lname + " ln_fold")


@pytest.mark.parametrize("name", FIXTURES)
def test_all_equal_list_is_the_uniform_batch(api, golden_dir, name):
    model = _model(api, golden_dir, name)
    imgs = _images(lc.LISTS["all_equal"])
    for classify in (False, True):
        uni = api.Session(model).predict(np.stack(imgs), classify=classify, topk=3 if classify else 0)
        got = api.Session(model).predict_list(imgs, classify=classify, topk=3 if classify else 0)
        for k in KEYS if classify else ("cls",):
            assert np.array_equal(got[k], uni[k]), k
        assert np.array_equal(got["patch_packed"].reshape(uni["patch_tokens"].shape), uni["patch_tokens"])


def test_reversed_list_permutes_the_outputs(api, golden_dir):
    sess = api.Session(_model(api, golden_dir, "tiny_gelu_reg4"))
    imgs = _images(lc.MIXED)
    a = sess.predict_list(imgs, classify=True, topk=3)
    b = sess.predict_list(imgs[::-1], classify=True, topk=3)
    n = len(imgs)
    for i in range(n):
        for k in KEYS:
            assert np.array_equal(a[k][i], b[k][n - 1 - i]), (k, i)
        assert np.array_equal(a["patch_tokens"][i], b["patch_tokens"][n - 1 - i]), i


def test_table_order_changes_no_bit(api, golden_dir):
    sess = api.Session(_model(api, golden_dir, "tiny_gelu_reg4"))
    imgs = _images(lc.MIXED)
    a = sess.predict_list(imgs, classify=True)
    try:
        api.set_tuning("list_order", 1)
        b = sess.predict_list(imgs, classify=True)
    finally:
        api.reset_tuning("list_order")
    for k in ("cls", "logits", "probs", "patch_packed"):
        assert np.array_equal(a[k], b[k]), k


def test_list_rows_equals_the_plan(api, golden_dir):
    for name in FIXTURES:
        model = _model(api, golden_dir, name)
        hp = model.hparams
        R = int(hp.num_register_tokens)
        for sizes in lc.LISTS.values():
            p = lc.plan(sizes, int(hp.patch_size), R, int(hp.num_attention_heads))
            for classify in (False, True):
                rows = p["images"][:, 1] - (1 if classify else 1 + R)
                assert np.array_equal(api.list_rows(model, sizes, classify=classify), np.concatenate([[0], np.cumsum(rows)]))


def test_device_inputs_and_outputs(api, golden_dir):
    """Device outputs equal host outputs; device images are read in place where a run is contiguous and gathered where it is not."""
    model = _model(api, golden_dir, "tiny_gelu_reg4")
    hp = model.hparams
    sizes = [lc.S70, lc.S70, lc.S154x168, lc.S70]  # run 0: two images in ONE allocation (in place); the last 70 x 70 stands apart
    imgs = _images(sizes)
    sess = api.Session(model)
    host = sess.predict_list(imgs, classify=True)
    pair = api.DeviceArray.from_host(np.stack(imgs[:2]))
    rest = [api.DeviceArray.from_host(im) for im in imgs[2:]]
    ptrs = [pair.ptr, pair.ptr + imgs[0].nbytes] + [d.ptr for d in rest]
    n, H, Cn = len(imgs), int(hp.hidden_size), int(hp.num_classes)
    off = api.list_rows(model, sizes, classify=True)
    d_cls, d_patch = api.DeviceArray((n, H), fill_nan=True), api.DeviceArray((int(off[-1]), H), fill_nan=True)
    d_logits, d_probs = api.DeviceArray((n, Cn), fill_nan=True), api.DeviceArray((n, Cn), fill_nan=True)
    sess.predict_list_device(ptrs, sizes, classify=True, cls_ptr=d_cls.ptr, patch_ptr=d_patch.ptr, logits_ptr=d_logits.ptr, probs_ptr=d_probs.ptr)
    sess.sync()
    assert np.array_equal(d_cls.to_host(), host["cls"]) and np.array_equal(d_patch.to_host(), host["patch_packed"])
    assert np.array_equal(d_logits.to_host(), host["logits"]) and np.array_equal(d_probs.to_host(), host["probs"])
    assert np.array_equal(off, host["offsets"])


@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
def test_raw_u8_images_of_different_sizes(api, golden_dir, classify):
    model = _model(api, golden_dir, "tiny_gelu_reg4")
    rng = np.random.default_rng(8)
    raws = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((30, 45), (64, 64), (50, 20), (30, 45), (97, 33))]
    got = api.Session(model).predict_list(raws, classify=classify, layout=api.U8_BGR_HWC, topk=3 if classify else 0)
    one = api.Session(model)
    for i, raw in enumerate(raws):
        exp = one.predict(raw[None], classify=classify, layout=api.U8_BGR_HWC, topk=3 if classify else 0)
        for k in KEYS if classify else ("cls",):
            assert np.array_equal(got[k][i], exp[k][0]), (i, k)
        assert np.array_equal(got["patch_tokens"][i], exp["patch_tokens"][0]), i


def test_bgr_hwc_layout(api, golden_dir):
    model = _model(api, golden_dir, "tiny_gelu_noreg")
    imgs = [lc.image(s, seed=i, layout_chw=False) for i, s in enumerate(lc.LISTS["repeat_apart"])]
    got = api.Session(model).predict_list(imgs, classify=True, layout=api.BGR_HWC)
    one = api.Session(model)
    for i, im in enumerate(imgs):
        exp = one.predict(im[None], classify=True, layout=api.BGR_HWC)
        assert np.array_equal(got["logits"][i], exp["logits"][0]) and np.array_equal(got["patch_tokens"][i], exp["patch_tokens"][0]), i


def test_one_list_within_the_oracle_bounds(api, golden_dir):
    name = "tiny_gelu_reg4"
    imgs = _images(lc.LISTS["repeat_apart"] + [lc.S154x168])
    got = api.Session(_model(api, golden_dir, name)).predict_list(imgs, classify=True)
    ora = OracleModel(os.path.join(golden_dir, name + ".gguf"))
    for i, img in enumerate(imgs):
        exp = ora.forward(img, classify=True)
        assert _rel(got["logits"][i], exp["logits"]) <= 1e-3, i
        assert _rel(got["cls"][i], exp["cls"]) <= 5e-3, i
        assert _rel(got["patch_tokens"][i], exp["patch_tokens"]) <= 5e-3, i


def _refused(api, fn):
    with pytest.raises(api.DinoError) as e:
        fn()
    return e.value


def test_session_state_after_a_list_call(api, golden_dir):
    model = _model(api, golden_dir, "tiny_gelu_reg4")
    hp = model.hparams
    H, P = int(hp.hidden_size), 25
    sess = api.Session(model)
    batch = np.stack([lc.image(lc.S70, 1), lc.image(lc.S70, 2)])
    sess.predict(batch)
    sess.predict_list(_images(lc.MIXED))
    out = np.empty((2, H), np.float32)
    o = api.Output()
    o.cls = out.ctypes.data
    bank = api.Bank(model, H, 64)
    err = _refused(api, lambda: api._call(api.lib().dinov2_hip_fetch, sess._h, C.byref(o)))
    assert "no forward to fetch from" in str(err)
    _refused(api, lambda: sess.pca3(None, shape=(P, H)))
    _refused(api, lambda: sess.match(None, None, shape=(P, H)))
    _refused(api, lambda: bank.add(sess, source="last_cls", n=2))
    _refused(api, lambda: bank.add(sess, source="last_patches", n=P))
    assert bank.count == 0
    # after the next uniform predict they work again, on that predict's bits
    uni = sess.predict(batch)
    api._call(api.lib().dinov2_hip_fetch, sess._h, C.byref(o))
    assert np.array_equal(out, uni["cls"])
    fresh = api.Session(model)
    fresh.predict(batch)
    for a, b in zip(sess.pca3(None, shape=(P, H)), fresh.pca3(None, shape=(P, H))):
        assert np.array_equal(a, b)
    m1, m2 = sess.match(None, None, shape=(P, H)), fresh.match(None, None, shape=(P, H))
    assert np.array_equal(m1["idx_ab"], m2["idx_ab"]) and np.array_equal(m1["sim_ab"], m2["sim_ab"])
    assert bank.add(sess, source="last_cls") is not None and bank.count == 2


def test_alternating_list_and_uniform_calls(api, golden_dir):
    """The workspace is carved by other keys for a list than for a batch: each kind of call re-carves after the other, and none sees the other."""
    model = _model(api, golden_dir, "tiny_swiglu_reg4")
    batch = np.stack([lc.image(lc.S112x126, 5), lc.image(lc.S112x126, 6), lc.image(lc.S112x126, 7)])
    want_uni = api.Session(model).predict(batch, classify=True)
    lists = [_images(lc.LISTS["mixed"]), _images(lc.LISTS["repeat_apart"])]
    want_list = [api.Session(model).predict_list(im, classify=True) for im in lists]
    sess = api.Session(model)
    for k in range(2):
        for want, imgs in zip(want_list, lists):
            got = sess.predict_list(imgs, classify=True)
            for key in ("cls", "logits", "probs", "patch_packed"):
                assert np.array_equal(got[key], want[key]), (k, key)
            uni = sess.predict(batch, classify=True)
            for key in ("cls", "logits", "probs", "patch_tokens"):
                assert np.array_equal(uni[key], want_uni[key]), (k, key)


def test_more_distinct_sizes_than_the_pos_embed_cache(api, golden_dir):
    name = "tiny_gelu_reg4"
    sizes = [(14 * k, 14 * (1 + k % 3)) for k in range(1, api.LIST_POS_GRIDS + 4)]
    assert len(set(sizes)) > api.LIST_POS_GRIDS
    sess = api.Session(_model(api, golden_dir, name))
    imgs = _images(sizes)
    _assert_as_alone(api, golden_dir, name, 0, 0, sess.predict_list(imgs, classify=True, topk=3), imgs, True, tag="many sizes")
    # a cache that has just been cleared and refilled, then a list that fits beside nothing of it, then the first again
    few = _images(lc.MIXED)
    _assert_as_alone(api, golden_dir, name, 0, 0, sess.predict_list(few, classify=True, topk=3), few, True, tag="after many sizes")
    _assert_as_alone(api, golden_dir, name, 0, 0, sess.predict_list(imgs[::-1], classify=True, topk=3), imgs[::-1], True, tag="many sizes again")


@pytest.mark.parametrize("ln_fold", [0, 1])
def test_launch_counts(api, golden_dir, ln_fold):
    model = _model(api, golden_dir, "tiny_gelu_reg4", 0, ln_fold)
    L = int(model.hparams.num_hidden_layers)
    sess = api.Session(model)
    sizes = lc.LISTS["repeat_apart"]
    runs = len(lc.plan(sizes, lc.PATCH, 4, 2)["runs"])
    assert runs == 5
    imgs = _images(sizes)
    sess.predict_list(imgs, classify=True)  # (position embeddings and the table are in place: the profiled call only launches)
    sess.profile(True)
    sess.predict_list(imgs, classify=True)
    got = {k: v[1] for k, v in sess.profile_read().items()}
    sess.profile(True)
    sess.predict(np.stack(imgs[:1]), classify=True)
    uni = {k: v[1] for k, v in sess.profile_read().items()}
    sess.profile(False)
    for k in ("im2col", "init_tokens", "gemm_patch_embed", "head"):
        assert got[k] == runs and uni[k] == 1, (k, got[k])
    for k in ("layernorm", "gemm_qkv", "gemm_attn_out", "gemm_ffn_in", "gemm_ffn_out", "final_layernorm", "layer_tap"):
        assert got[k] == uni[k], (k, got[k], uni[k])
    assert got["attention"] == L and got["final_layernorm"] == 1 and got["layernorm"] == (1 if ln_fold else 2 * L)


def test_argument_errors_run_nothing(api, golden_dir):
    model = _model(api, golden_dir, "tiny_gelu_reg4")
    nohead = _model(api, golden_dir, "tiny_gelu_reg4", classify=False)
    sess, sess_nohead = api.Session(model), api.Session(nohead)
    L = api.lib()
    buf = np.zeros((3, 70, 70), np.float32)
    out = np.empty((64, int(model.hparams.hidden_size)), np.float32)

    def call(s, ptrs, sizes, flags=0, layout=api.RGB_CHW, o=None, patch=lambda il: None):
        il, keep = api._image_list(ptrs, sizes, layout, 0)
        patch(il)
        err = C.create_string_buffer(512)
        rc = L.dinov2_hip_predict_list(s._h, C.byref(il), C.byref(o) if o is not None else None, flags, err, len(err))
        return rc, err.value.decode()

    sess.profile(True)
    sess_nohead.profile(True)
    p = buf.ctypes.data
    rc, msg = call(sess, [], [])
    assert rc == 4 and "at least one image" in msg
    rc, msg = call(sess, [p, p], [lc.S70, lc.S70], patch=lambda il: setattr(il, "n", -3))
    assert rc == 4
    rc, msg = call(sess, [p, p], [lc.S70, lc.S70], patch=lambda il: setattr(il, "height", None))
    assert rc == 4 and "null" in msg
    rc, msg = call(sess, [p, 0, p], [lc.S70] * 3)
    assert rc == 4 and "image 1" in msg
    rc, msg = call(sess, [p, p, p], [lc.S70, lc.S70, (70, 71)])
    assert rc == 4 and "image 2" in msg and "patch_size" in msg
    rc, msg = call(sess, [p, p], [lc.S70, (0, 70)])
    assert rc == 4 and "image 1" in msg
    rc, msg = call(sess, [p, p], [lc.S70, (0, 70)], layout=api.U8_BGR_HWC)
    assert rc == 4 and "image 1" in msg
    rc, msg = call(sess, [p], [lc.S70], layout=7)
    assert rc == 4 and "image 0" in msg and "layout" in msg
    rc, msg = call(sess_nohead, [p], [lc.S70], flags=api.CLASSIFY)
    assert rc == 6 and "classifier" in msg
    o = api.Output()
    o.on_device, o.topk, o.topk_ids = 1, 3, out.ctypes.data
    rc, msg = call(sess, [p], [lc.S70], flags=api.CLASSIFY, o=o)
    assert rc == 4 and "top-k" in msg
    # too many rows for one pass: rows * max(3 H, ffn, patch K) * 2 >= 2^31 -- refused, not split, and no image is read
    hp = model.hparams
    widest = max(3 * int(hp.hidden_size), int(hp.ffn_hidden), -(-3 * lc.PATCH * lc.PATCH // 64) * 64)
    big = (14 * 200, 14 * 200)
    n_fit = ((1 << 31) - 1) // (2 * widest) // lc.tokens(big, 4)  # the longest list of such images that fits
    rc, msg = call(sess, [p] * (n_fit + 1), [big] * (n_fit + 1))
    assert rc == 4 and "image %d" % n_fit in msg and "not split" in msg
    off = np.zeros(n_fit + 2, np.int64)
    il, keep = api._image_list([0] * (n_fit + 1), [big] * (n_fit + 1), api.RGB_CHW, 0)
    err = C.create_string_buffer(512)
    assert L.dinov2_hip_list_rows(model._h, C.byref(il), 0, api._ptr(off), err, len(err)) == 4
    assert np.array_equal(api.list_rows(model, [big] * n_fit), np.arange(n_fit + 1) * 40000)
    for s in (sess, sess_nohead):
        assert all(v[1] == 0 for v in s.profile_read().values()), "a refused call launched something"
        s.profile(False)
    # and the session still works
    imgs = _images(lc.LISTS["single"])
    _assert_as_alone(api, golden_dir, "tiny_gelu_reg4", 0, 0, sess.predict_list(imgs, classify=True, topk=3), imgs, True, tag="after errors")
