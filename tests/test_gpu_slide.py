"""dinov2_hip_predict_dense_slide on the device: the two kernels of csrc/slide.hip through dinov2_hip_op_slide_reduce / dinov2_hip_op_slide_gather
(no model) against the cases of tests/slide_cases.py, then the call itself on the golden tiny models -- every window's logits bit for bit
against dinov2_hip_predict_dense on the host-cropped window batch, labels and value bit for bit against the numpy restatement applied to
those logits, labels against the float64 pipeline outside its margin --, its equivalences, its refusals and the session afterwards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import misc_cases as mc
import slide_cases as sl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("tiny_gelu_noreg", "tiny_gelu_reg4", "tiny_swiglu_reg4")
F16, BF16 = 0, 1
H, W, CH, CW, SH, SW = sl.MODEL_CASE  # (70, 91, 42, 42, 20, 20): twelve windows, pulled back, odd x1, cover 1 .. 9
YS, XS = sl.starts(H, CH, SH), sl.starts(W, CW, SW)


def _images(B, size, seed):
    return np.random.default_rng(seed).standard_normal((B, 3, size[0], size[1])).astype(np.float32)


def _model(api, golden_dir, name, dt=F16, **kw):
    return api.Model(os.path.join(golden_dir, name + ".gguf"), dtype=dt, classify=False, **kw)


def _head(api, model, reduce="argmax", C_=21, layers=(1, 2), concat_cls=True, scale=1.0):
    K = len(layers) * model.hparams.hidden_size * (1 + concat_cls)
    W_, bias = dc.head_weights(C_, K, seed=77)
    kw = dict(reduce="bins", bin_centers=dc.bin_centers(C_), bins_eps=0.1) if reduce == "bins" else {}
    return api.DenseHead(model, list(layers), W_ * np.float32(scale), bias, norm=True, concat_cls=concat_cls, **kw)


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if a[k].dtype == np.uint8:
            assert np.array_equal(a[k], b[k]), "%s: %s differ" % (what, k)
        else:
            ok, msg = mc.check_exact(a[k], b[k], "%s %s" % (what, k))
            assert ok, msg


def _crops(imgs, ys, xs, ch, cw):
    return np.concatenate([sl.gather_reference(img, ys, xs, ch, cw) for img in imgs])


# ----------------------------------------------------------------------------------------------------------------- the kernels
def _op(api):
    return lambda Ls, ys, xs, h0, w0, ch, cw, h, w, red, cen, eps: api.op_slide_reduce(Ls, h0, w0, (ch, cw), (h, w), ys, xs, red, cen, eps)


@pytest.mark.parametrize("ci", range(len(sl.CASES)))
def test_op_slide_reduce_every_class_count_and_reduction(api, ci):
    fails = sl.reduce_failures(_op(api), cases=[ci]) if ci == 0 else \
        [f for f in sl.reduce_failures(_op(api), cases=[ci]) if not f.startswith("probe ")]  # (the probes run once, with case 0)
    assert not fails, "\n".join(fails[:10])


def test_op_slide_reduce_writes_only_what_is_asked_for_and_refuses_a_cover_of_49(api):
    ys, xs, h0, w0 = sl.case_geometry(sl.MODEL_CASE)
    Ls = sl.case_logits(2, 21)
    exp = sl.emulate(Ls, ys, xs, h0, w0, CH, CW, H, W)
    only_labels = api.op_slide_reduce(Ls, h0, w0, (CH, CW), (H, W), ys, xs, want=("labels",))
    only_value = api.op_slide_reduce(Ls, h0, w0, (CH, CW), (H, W), ys, xs, want=("value",))
    assert set(only_labels) == {"labels"} and set(only_value) == {"value"}
    assert not sl.compare(only_labels, {"labels": exp["labels"]}, "labels alone") and not sl.compare(only_value, {"value": exp["value"]}, "value alone")
    h, w, ch, cw, sh, sw = sl.REFUSED_CASE
    ys, xs, h0, w0 = sl.case_geometry(sl.REFUSED_CASE)
    with pytest.raises(Exception):
        api.op_slide_reduce(sl.window_logits(len(ys) * len(xs), h0 * w0, 2, 1), h0, w0, (ch, cw), (h, w), ys, xs)


@pytest.mark.parametrize("ci", [2, 3, 4])
def test_op_slide_gather_is_numpy_slicing(api, ci):
    h, w, ch, cw, _, _ = sl.CASES[ci]
    ys, xs, _, _ = sl.case_geometry(sl.CASES[ci])
    img = _images(1, (h, w), 40 + ci)[0]
    got = api.op_slide_gather(img, (ch, cw), ys, xs)
    assert mc.diff_count(got, sl.gather_reference(img, ys, xs, ch, cw)) == 0
    hwc = np.ascontiguousarray(img.transpose(1, 2, 0))
    got = api.op_slide_gather(hwc, (ch, cw), ys, xs, layout=api.BGR_HWC)
    assert mc.diff_count(got, sl.gather_reference(hwc, ys, xs, ch, cw, chw=False)) == 0


# ----------------------------------------------------------------------------------------------------------------- golden tiny models
def _operands(taps, concat_cls):
    blocks = []
    for d in taps["layers"]:
        B, P, Hh = d["patch_tokens"].shape
        blocks.append(d["patch_tokens"].reshape(B * P, Hh))
        if concat_cls:
            blocks.append(np.repeat(d["cls"], P, axis=0))
    return np.concatenate(blocks, axis=1).astype(np.float16)


def _check_slide(api, model, C_, layers, concat_cls, what, case=sl.MODEL_CASE, margin=True):
    """`case` = (h, w, crop h, crop w, stride h, stride w) of the images and windows; `margin`: also the float64 pipeline outside its top-2
    margin, with the cap on the pixels inside it (the off-family entry-point tests run the exact parts alone on their small outputs)."""
    h, w, ch, cw, sh, sw = case
    ys, xs = sl.starts(h, ch, sh), sl.starts(w, cw, sw)
    y1, x1 = model.slide_windows(h, w, (ch, cw), (sh, sw))
    assert list(y1) == list(ys) and list(x1) == list(xs), (what, list(y1), list(x1))
    sess = api.Session(model)
    h0, w0 = model.grid(ch, cw)
    P, nwin = h0 * w0, len(ys) * len(xs)
    imgs = _images(2, (h, w), C_)
    crops = _crops(imgs, ys, xs, ch, cw)
    taps = sess.predict_layers(crops, list(layers), norm=True, return_class_token=True)
    A16 = _operands(taps, concat_cls)
    rms = float(np.sqrt((A16.astype(np.float64) ** 2).mean()))
    K = len(layers) * model.hparams.hidden_size * (1 + concat_cls)
    Wt, bias = dc.head_weights(C_, K, seed=C_ + K, logit_std=4.0 / rms)
    cen = dc.bin_centers(C_)
    seg = api.DenseHead(model, list(layers), Wt, bias, norm=True, concat_cls=bool(concat_cls))
    dep = api.DenseHead(model, list(layers), Wt, bias, norm=True, concat_cls=bool(concat_cls), reduce="bins", bin_centers=cen, bins_eps=0.1)
    rs = sess.predict_dense_slide(imgs, seg, (ch, cw), (sh, sw))
    rd = sess.predict_dense_slide(imgs, dep, (ch, cw), (sh, sw))
    assert set(rs) == {"labels", "value", "logits"} and set(rd) == {"value", "logits"}
    assert rs["logits"].shape == (2, nwin, P, C_) and rs["labels"].shape == (2, h, w) and rs["value"].shape == (2, h, w)
    direct = api.Session(model).predict_dense(crops, seg, want=("logits",))["logits"]  # contract 2: the crop alone, through predict_dense
    ok, msg = mc.check_exact(rs["logits"].reshape(2 * nwin, P, C_), direct, what + ": window logits against predict_dense of the crops")
    assert ok, msg
    ok, msg = mc.check_exact(rd["logits"], rs["logits"], what + ": logits of the two heads")
    assert ok, msg
    ref, bound = dc.logits_reference(A16, Wt, bias)
    ref, bound = ref.reshape(2, nwin, P, C_), bound.reshape(2, nwin, P, C_)
    excluded = total = 0
    for b in range(2):
        Lb = rs["logits"][b]
        fails = sl.compare({"labels": rs["labels"][b], "value": rs["value"][b]}, sl.emulate(Lb, ys, xs, h0, w0, ch, cw, h, w), "%s image %d argmax" % (what, b))
        fails += sl.compare({"value": rd["value"][b]}, sl.emulate(Lb, ys, xs, h0, w0, ch, cw, h, w, dc.BINS, cen, 0.1), "%s image %d bins" % (what, b))
        assert not fails, "\n".join(fails)
        if not margin:
            continue
        f64 = sl.reference(ref[b], ys, xs, h0, w0, ch, cw, h, w)
        # the logits' own error passes through convex combinations and a mean unamplified; the float32 mean adds slide_cases.mean_bound
        lb = float(bound[b].max())
        tol = lb + sl.mean_bound(f64["n"], np.abs(ref[b]).max() + lb)
        sure = f64["margin"] > 2 * tol
        assert (rs["labels"][b][sure] == f64["labels"][sure]).all(), "%s image %d: labels differ from float64 outside the margin" % (what, b)
        excluded += int((~sure).sum())
        total += sure.size
    if not margin:
        return
    print("%s: %d of %d pixels inside the margin" % (what, excluded, total))
    assert excluded <= 0.02 * total, "%s: %d of %d pixels excluded by the margin" % (what, excluded, total)


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_models_window_logits_labels_and_values(api, golden_dir, name):
    k = FIXTURES.index(name)
    _check_slide(api, _model(api, golden_dir, name), (21, 150, 256)[k], ((1, 2), (2,), (1, 2))[k], k % 2, name)


def test_bf16_model_same_checks(api, golden_dir):
    _check_slide(api, _model(api, golden_dir, "tiny_gelu_reg4", BF16), 21, (1, 2), 1, "bf16")


def test_patch_stride_7_model_at_crop_42(api, golden_dir):
    """grid_of, not crop / patch: a patch_stride = 7 model has a 5 x 5 grid under a 42 x 42 crop."""
    model = _model(api, golden_dir, "tiny_gelu_reg4", patch_stride=7)
    assert model.grid(CH, CW) == (5, 5)
    head, sess = _head(api, model), api.Session(model)
    imgs = _images(1, (H, W), 9)
    r = sess.predict_dense_slide(imgs, head, CH, SH)
    assert r["logits"].shape == (1, 12, 25, 21)
    direct = api.Session(model).predict_dense(_crops(imgs, YS, XS, CH, CW), head, want=("logits",))["logits"]
    ok, msg = mc.check_exact(r["logits"][0], direct, "stride-7 window logits")
    assert ok, msg
    fails = sl.compare({"labels": r["labels"][0], "value": r["value"][0]}, sl.emulate(r["logits"][0], YS, XS, 5, 5, CH, CW, H, W), "stride-7")
    assert not fails, "\n".join(fails)


# ----------------------------------------------------------------------------------------------------------------- equivalences
@pytest.mark.parametrize("reduce", ["argmax", "bins"])
def test_one_window_equals_predict_dense(api, golden_dir, reduce):
    model = _model(api, golden_dir, "tiny_gelu_reg4")
    head = _head(api, model, reduce)
    imgs = _images(2, (42, 56), 5)
    got = api.Session(model).predict_dense_slide(imgs, head, (42, 56), (14, 1))
    exp = api.Session(model).predict_dense(imgs, head)
    _same({k: (v[:, 0] if k == "logits" else v) for k, v in got.items()}, exp, "one window")


@pytest.mark.parametrize("reduce", ["argmax", "bins"])
def test_an_image_alone_equals_the_image_in_a_batch_and_both_layouts_agree(api, golden_dir, reduce):
    model = _model(api, golden_dir, "tiny_swiglu_reg4")
    head, sess = _head(api, model, reduce), api.Session(model)
    imgs = _images(2, (H, W), 8)
    full = sess.predict_dense_slide(imgs, head, CH, SH)
    for b in range(2):
        one = sess.predict_dense_slide(imgs[b:b + 1], head, CH, SH)
        _same({k: v[0] for k, v in one.items()}, {k: v[b] for k, v in full.items()}, "image %d alone" % b)
    # the same pixels as [B, h, w, 3] with the channels reversed are the same images to the model (BGR_HWC against RGB_CHW)
    hwc = np.ascontiguousarray(imgs[:, ::-1].transpose(0, 2, 3, 1))
    _same(sess.predict_dense_slide(hwc, head, CH, SH, layout=api.BGR_HWC), full, "BGR_HWC")


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
load_package(); api = import_module(PKG_NAME + ".api")
import dense_cases as dc
model = api.Model(sys.argv[2], classify=False)
imgs = np.random.default_rng(8).standard_normal((1, 3, 70, 91)).astype(np.float32)
out = {}
for reduce in ("argmax", "bins"):
    W, bias = dc.head_weights(21, 512, seed=77)
    kw = dict(reduce="bins", bin_centers=dc.bin_centers(21), bins_eps=0.1) if reduce == "bins" else {}
    head = api.DenseHead(model, [1, 2], W, bias, norm=True, concat_cls=True, **kw)
    r = api.Session(model).predict_dense_slide(imgs, head, 42, 20)
    out.update({reduce + "_" + k: v for k, v in r.items()})
np.savez(sys.argv[3], **out); print("SLIDE_OK")
'''


def test_split_passes_equal_one_pass_in_a_fresh_process(api, golden_dir, tmp_path):
    """DINOV2_HIP_MAX_CHUNK=5: the twelve windows make three passes, each writing its logits at its window offset -- against the unsplit call
    of another fresh process, bit for bit."""
    res = []
    for chunk in ("5", "0"):
        f = str(tmp_path / ("slide%s.npz" % chunk))
        out = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), f], cwd=ROOT,
                             env=dict(os.environ, DINOV2_HIP_MAX_CHUNK=chunk), capture_output=True, text=True, timeout=600)
        assert "SLIDE_OK" in out.stdout, out.stdout + out.stderr
        res.append(dict(np.load(f)))
    assert set(res[0]) == {"argmax_labels", "argmax_value", "argmax_logits", "bins_value", "bins_logits"}
    _same(res[0], res[1], "split against unsplit")


@pytest.mark.parametrize("reduce", ["argmax", "bins"])
def test_device_input_and_outputs_equal_host_input_and_outputs(api, golden_dir, reduce):
    model = _model(api, golden_dir, "tiny_gelu_noreg")
    head, sess = _head(api, model, reduce), api.Session(model)
    imgs = _images(2, (H, W), 4)
    host = sess.predict_dense_slide(imgs, head, CH, SH)
    B, npx = 2, H * W
    for dev_in in (False, True):
        lab = api.DeviceArray(((B * npx + 3) // 4,), fill_nan=True) if reduce == "argmax" else None
        val = api.DeviceArray((B, H, W), fill_nan=True)
        lg = api.DeviceArray((B, 12, 9, 21), fill_nan=True)
        if dev_in:
            src = api.DeviceArray.from_host(imgs)
            sess.predict_dense_slide_device(src.ptr, B, H, W, head, CH, SH, labels_ptr=lab.ptr if lab else 0, value_ptr=val.ptr, logits_ptr=lg.ptr)
        else:
            do = api.DenseOut(0, 0, lab.ptr if lab else None, val.ptr, lg.ptr, 1)
            i = api.Input(imgs.ctypes.data, B, H, W, api.RGB_CHW, 0)
            s = api.Slide(CH, CW, SH, SW)
            err = C.create_string_buffer(256)
            rc = api.lib().dinov2_hip_predict_dense_slide(sess._h, C.byref(i), head._h, C.byref(s), C.byref(do), err, len(err))
            assert rc == 0, err.value.decode()
        sess.sync()
        out = {"value": val.to_host(), "logits": lg.to_host()}
        if lab:
            out["labels"] = lab.to_host().view(np.uint8)[:B * npx].reshape(B, H, W)
        _same(out, host, "device outputs, device input %s" % dev_in)


# ----------------------------------------------------------------------------------------------------------------- windows, refusals, session
def test_slide_windows_are_the_formula_and_refuse_what_the_call_refuses(api, golden_dir):
    model = _model(api, golden_dir, "tiny_gelu_noreg")
    for c in sl.CASES + (sl.REFUSED_CASE, (8192, 100, 42, 42, 42, 13)):
        h, w, ch, cw, sh, sw = c
        y1, x1 = model.slide_windows(h, w, (ch, cw), (sh, sw))
        assert y1.tolist() == sl.starts(h, ch, sh).tolist() and x1.tolist() == sl.starts(w, cw, sw).tolist(), c
    for bad in ((70, 91, 43, 42, 20, 20), (70, 91, 42, 0, 20, 20), (70, 91, 42, 42, 0, 20), (70, 91, 42, 42, 20, 43), (41, 91, 42, 42, 20, 20),
                (70, 41, 42, 42, 20, 20), (8193, 91, 42, 42, 20, 20), (70, 8193, 42, 42, 20, 20)):
        with pytest.raises(api.DinoError) as e:
            model.slide_windows(bad[0], bad[1], bad[2:4], bad[4:6])
        assert str(e.value), bad


def test_argument_errors_leave_the_outputs_alone(api, pkg, golden_dir, tmp_path):
    model = _model(api, golden_dir, "tiny_gelu_noreg")
    Hd = int(model.hparams.hidden_size)
    Wt, bias = dc.head_weights(5, 2 * Hd, 1)
    seg = api.DenseHead(model, [1, 2], Wt, bias)
    dep = api.DenseHead(model, [1, 2], Wt, bias, reduce="bins", bin_centers=dc.bin_centers(5))
    imgs = _images(2, (H, W), 1)
    raw = np.zeros((2, H, W, 3), np.uint8)
    sess = api.Session(model)
    labels = np.full((2, H, W), 7, np.uint8)
    value = np.full((2, H, W), 7.0, np.float32)
    logits = np.full((2, 12, 9, 5), 7.0, np.float32)
    dev = api.DeviceArray((2 * H * W + 8,), fill_nan=True)

    def call(head=seg, oh=0, ow=0, lab=True, val=True, lg=True, on_device=0, ptrs=None, null_in=False, null_out=False, null_slide=False, s=sess,
             null_sess=False, size=(H, W), crop=(CH, CW), stride=(SH, SW), layout=None, data=imgs, batch=2):
        p = ptrs or (labels.ctypes.data, value.ctypes.data, logits.ctypes.data)
        do = api.DenseOut(oh, ow, p[0] if lab else None, p[1] if val else None, p[2] if lg else None, on_device)
        i = api.Input(data.ctypes.data if data is not None else None, batch, size[0], size[1], api.RGB_CHW if layout is None else layout, 0)
        sd = api.Slide(crop[0], crop[1], stride[0], stride[1])
        err = C.create_string_buffer(512)
        rc = api.lib().dinov2_hip_predict_dense_slide(None if null_sess else s._h, None if null_in else C.byref(i), head._h if head else None,
                                                      None if null_slide else C.byref(sd), None if null_out else C.byref(do), err, len(err))
        return rc, err.value.decode()

    other_path = str(tmp_path / "other.gguf")
    pkg.synth.write_synthetic_gguf(other_path, "small", registers=0, num_classes=10, seed=1, layers=1)
    other = api.Model(other_path, classify=False)
    bad = {"null session": dict(null_sess=True), "null input": dict(null_in=True), "null data": dict(data=None), "null head": dict(head=None),
           "null slide": dict(null_slide=True), "null dense_out": dict(null_out=True), "batch 0": dict(batch=0),
           "raw 8-bit input": dict(layout=api.U8_BGR_HWC, data=raw), "unknown layout": dict(layout=3),
           "a crop that is no network size": dict(crop=(43, 42)), "crop 0": dict(crop=(42, 0)),
           "stride 0": dict(stride=(0, 20)), "stride above the crop": dict(stride=(20, 43)),
           "image smaller than the crop": dict(size=(41, W)), "image wider than 8192": dict(size=(H, 8193)),
           "out_h, out_w given": dict(oh=H, ow=W), "out_w alone": dict(ow=10),
           "labels from a bins head": dict(head=dep), "all outputs NULL": dict(lab=False, val=False, lg=False),
           "misaligned device value": dict(on_device=1, lab=False, lg=False, ptrs=(None, dev.ptr + 4, None)),
           "misaligned device labels": dict(on_device=1, val=False, lg=False, ptrs=(dev.ptr + 1, None, None)),
           "a head of another model size": dict(s=api.Session(other)),
           "more than 65 535 windows": dict(size=(8192, 8192), crop=(28, 28), stride=(28, 28)),
           "a cover of 49": dict(size=(70, 70), stride=(5, 5))}
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == 4 and msg, (what, rc, msg)
        assert (labels == 7).all() and (value == 7.0).all() and (logits == 7.0).all(), what
    assert "49" in call(size=(70, 70), stride=(5, 5))[1] and "8193" in call(size=(H, 8193))[1] and "43" in call(stride=(20, 43))[1]
    assert np.isnan(dev.to_host()).all()
    rc, msg = call()
    assert rc == 0, msg
    ref = api.Session(model).predict_dense_slide(imgs, seg, CH, SH)
    assert np.array_equal(labels, ref["labels"]) and mc.diff_count(value, ref["value"]) == 0 and mc.diff_count(logits, ref["logits"]) == 0


def test_the_session_afterwards_and_the_profile_kinds(api, golden_dir):
    """No last un-split forward, as after predict_list: fetch is refused; a later predict has the bits of a fresh session's.  The gather is
    booked under "im2col", the reduction under "head", beside what predict_dense books for the window batch."""
    model = _model(api, golden_dir, "tiny_gelu_reg4")
    head, sess = _head(api, model), api.Session(model)
    imgs = _images(1, (H, W), 2)
    crops = _crops(imgs, YS, XS, CH, CW)
    sess.profile(True)
    sess.predict_dense(crops, head, want=("logits",))
    base = sess.profile_read()
    sess.profile(True)
    sess.predict_dense_slide(imgs, head, CH, SH)
    prof = sess.profile_read()
    sess.profile(False)
    assert prof["im2col"][1] == base["im2col"][1] + 1 and prof["head"][1] == base["head"][1] + 1
    assert all(prof[k][1] == base[k][1] for k in base if k not in ("im2col", "head"))
    fetched, o = api._alloc_outputs(model.hparams, 1, CH, CW, api.RGB_CHW, False, 0, ("cls",))
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_fetch(sess._h, C.byref(o), err, len(err)) == 4 and err.value
    with pytest.raises(Exception):
        sess.pca3(None, (9, 128))
    small = _images(2, (56, 84), 3)
    _same(sess.predict(small), api.Session(model).predict(small), "a predict after the slide call")
