"""dinov2_hip_predict_dense on the device: the two kernels of csrc/dense.hip through dinov2_hip_op_dense_reduce / dinov2_hip_op_dense_pack (no
model) against the cases of tests/dense_cases.py, then the call itself on the golden tiny models -- the low-resolution logits against float64
of the f16 operands (taken from dinov2_hip_predict_layers of the same session), labels and value bit for bit against the numpy restatement
applied to the device's own logits, labels against the float64 pipeline wherever its top-2 margin is wider than twice the bound --, its
invariances, and its argument errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import misc_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("tiny_gelu_noreg", "tiny_gelu_reg4", "tiny_swiglu_reg4")
SIZES = ((70, 70), (56, 84), (42, 42))
F16, BF16 = 0, 1
EPS = 1e-6


def _images(B, size, seed):
    return np.random.default_rng(seed).standard_normal((B, 3, size[0], size[1])).astype(np.float32)


def _model(api, golden_dir, name, dt=F16, classify=False):
    return api.Model(os.path.join(golden_dir, name + ".gguf"), dtype=dt, classify=classify)


# ----------------------------------------------------------------------------------------------------------------- the kernels
def test_op_dense_reduce_every_shape_class_count_reduction_and_probe(api):
    fails = dc.reduce_failures(lambda L, h0, w0, oh, ow, red, cen, eps: api.op_dense_reduce(L, h0, w0, oh, ow, red, cen, eps))
    assert not fails, "\n".join(fails[:10])


def test_op_dense_reduce_writes_only_what_is_asked_for(api):
    L = dc.gaussian_logits(24, 21, 5)
    exp = dc.emulate(L, 4, 6, 50, 77)
    only_labels = api.op_dense_reduce(L, 4, 6, 50, 77, want=("labels",))
    only_value = api.op_dense_reduce(L, 4, 6, 50, 77, want=("value",))
    assert set(only_labels) == {"labels"} and set(only_value) == {"value"}
    assert not dc.compare(only_labels, {"labels": exp["labels"]}, "labels alone") and not dc.compare(only_value, {"value": exp["value"]}, "value alone")


@pytest.mark.parametrize("H", [128, 1024])
@pytest.mark.parametrize("R", [0, 4])
@pytest.mark.parametrize("norm,concat_cls", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_op_dense_pack_is_f16_of_the_layer_tap(api, H, R, norm, concat_cls):
    B, h0, w0 = 2, 1, 7  # 14 patch rows: more than one workgroup of four waves, and a last one that is half empty
    P, T = h0 * w0, 1 + R + h0 * w0
    x = (np.random.default_rng(H + R).standard_normal((B, T, H)) * 2 + 0.3).astype(np.float32)
    w, b = mc.ln_affine(H, 9)
    tap = api.op_layer_tap(x, w, b, EPS, R, h0, w0, norm=bool(norm), chw=False, want=("patch", "cls"))
    hblk = H * (1 + concat_cls)
    got = api.op_dense_pack(x, w, b, EPS, R, norm=norm, concat_cls=concat_cls, slot=1, nslots=2)
    assert got.shape == (B * P, 2 * hblk) and np.isnan(got[:, :hblk]).all()  # the other slot's columns were not written
    exp = [np.float16(tap["patch"].reshape(B * P, H))]
    if concat_cls:
        exp.append(np.float16(np.repeat(tap["cls"], P, axis=0)))
    ok, msg = mc.check_exact(got[:, hblk:], np.concatenate(exp, axis=1).astype(np.float32), "operand block")
    assert ok, msg


# ----------------------------------------------------------------------------------------------------------------- golden tiny models
def _operands(taps, concat_cls):
    """A^ [B * P, K] float16 from a predict_layers result of the same layers (norm as the head's), return_class_token=True."""
    blocks = []
    for d in taps["layers"]:
        B, P, H = d["patch_tokens"].shape
        blocks.append(d["patch_tokens"].reshape(B * P, H))
        if concat_cls:
            blocks.append(np.repeat(d["cls"], P, axis=0))
    return np.concatenate(blocks, axis=1).astype(np.float16)


def _check_dense(api, sess, model, imgs, layers, C_, norm, concat_cls, out_size, what, margin=True):
    """`margin`: also the float64 pipeline outside its top-2 margin, with the cap on the pixels inside it (stated for outputs of 56 pixels
    and more: the off-family entry-point tests run the exact parts alone on their small outputs)."""
    hp = model.hparams
    B, (hh, ww) = imgs.shape[0], imgs.shape[2:]
    h0, w0 = model.grid(hh, ww)
    P, K = h0 * w0, len(layers) * hp.hidden_size * (1 + concat_cls)
    oh, ow = (hh, ww) if out_size is None else out_size
    cen = dc.bin_centers(C_)
    taps = sess.predict_layers(imgs, layers, norm=bool(norm), return_class_token=True)
    A16 = _operands(taps, concat_cls)
    rms = float(np.sqrt((A16.astype(np.float64) ** 2).mean()))  # (the raw rows are not unit-variance: the logits' deviation stays about 4)
    W, bias = dc.head_weights(C_, K, seed=C_ + K, logit_std=4.0 / rms)
    ref, bound = dc.logits_reference(A16, W, bias)
    seg = api.DenseHead(model, layers, W, bias, norm=bool(norm), concat_cls=bool(concat_cls))
    dep = api.DenseHead(model, layers, W, bias, norm=bool(norm), concat_cls=bool(concat_cls), reduce="bins", bin_centers=cen, bins_eps=0.1)
    rs = sess.predict_dense(imgs, seg, out_size)
    rd = sess.predict_dense(imgs, dep, out_size)
    assert set(rs) == {"labels", "value", "logits"} and set(rd) == {"value", "logits"}
    ok, msg = mc.check_exact(rd["logits"], rs["logits"], what + ": logits of the two heads")
    assert ok, msg
    got = rs["logits"].reshape(B * P, C_).astype(np.float64)
    err = np.abs(got - ref)
    print("%s: logits std %.2f, worst |L - L64| / bound %.3f" % (what, float(got.std()), float((err / bound).max())))
    assert (err <= bound).all(), "%s: %d logits outside the bound" % (what, int((err > bound).sum()))
    excluded = total = 0
    for b in range(B):
        Lb = rs["logits"][b]
        fails = dc.compare({"labels": rs["labels"][b], "value": rs["value"][b]}, dc.emulate(Lb, h0, w0, oh, ow), "%s image %d argmax" % (what, b))
        fails += dc.compare({"value": rd["value"][b]}, dc.emulate(Lb, h0, w0, oh, ow, dc.BINS, cen, 0.1), "%s image %d bins" % (what, b))
        assert not fails, "\n".join(fails)
        if not margin:
            continue
        r64, b64 = ref[b * P:(b + 1) * P], bound[b * P:(b + 1) * P]
        f64 = dc.reference(r64, h0, w0, oh, ow)
        vb = dc.val_bound(b64, np.abs(r64), h0, w0, oh, ow).max(axis=2)
        sure = f64["margin"] > 2 * vb
        assert (rs["labels"][b][sure] == f64["labels"][sure]).all(), "%s image %d: labels differ from float64 outside the margin" % (what, b)
        excluded += int((~sure).sum())
        total += sure.size
        d64 = dc.reference(r64, h0, w0, oh, ow, dc.BINS, cen, 0.1)["value"]
        tol = dc.bins_bound(b64, r64, h0, w0, oh, ow, cen, 0.1)
        assert (np.abs(rd["value"][b] - d64) <= tol).all(), "%s image %d: bins outside the bound" % (what, b)
    if not margin:
        return
    print("%s: %d of %d pixels inside the margin" % (what, excluded, total))
    assert excluded <= 0.02 * total, "%s: %d of %d pixels excluded by the margin" % (what, excluded, total)


@pytest.mark.parametrize("layers", [(1, 2), (2,)])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_models_logits_labels_and_values(api, golden_dir, name, size, layers):
    model = _model(api, golden_dir, name)
    sess = api.Session(model)
    k = FIXTURES.index(name) + SIZES.index(size) + len(layers)
    C_ = dc.CLASSES[k % 4]
    h0, w0 = size[0] // 14, size[1] // 14
    # every C, both norms, both concat_cls over the 18 cases; output at the input size (scale 14) or at 4 h0 x 4 w0 (upstream's depth heads)
    _check_dense(api, sess, model, _images(2, size, k), list(layers), C_, norm=k % 2, concat_cls=(k // 2) % 2,
                 out_size=None if k % 3 else (4 * h0, 4 * w0), what="%s %dx%d %s C=%d" % (name, size[0], size[1], layers, C_))


def test_bf16_model_same_shapes_and_checks(api, golden_dir):
    """The operands are f16 whatever the compute type: a bf16 model goes through the same checks against its own taps."""
    model = _model(api, golden_dir, "tiny_gelu_reg4", BF16)
    _check_dense(api, api.Session(model), model, _images(2, (56, 84), 3), [1, 2], 21, norm=1, concat_cls=1, out_size=(50, 77), what="bf16")


# ----------------------------------------------------------------------------------------------------------------- invariances
def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if a[k].dtype == np.uint8:
            assert np.array_equal(a[k], b[k]), "%s: %s differ" % (what, k)
        else:
            ok, msg = mc.check_exact(a[k], b[k], "%s %s" % (what, k))
            assert ok, msg


def _head(api, model, reduce="argmax", C_=21, layers=(1, 2), concat_cls=True):
    K = len(layers) * model.hparams.hidden_size * (1 + concat_cls)
    W, bias = dc.head_weights(C_, K, seed=77)
    kw = dict(reduce="bins", bin_centers=dc.bin_centers(C_), bins_eps=0.1) if reduce == "bins" else {}
    return api.DenseHead(model, list(layers), W, bias, norm=True, concat_cls=concat_cls, **kw)


@pytest.mark.parametrize("reduce", ["argmax", "bins"])
def test_an_image_alone_equals_the_image_in_a_batch(api, golden_dir, reduce):
    model = _model(api, golden_dir, "tiny_swiglu_reg4")
    head, sess = _head(api, model, reduce), api.Session(model)
    imgs = _images(3, (56, 84), 8)
    full = sess.predict_dense(imgs, head, (50, 77))
    for b in range(3):
        one = sess.predict_dense(imgs[b:b + 1], head, (50, 77))
        _same({k: v[0] for k, v in one.items()}, {k: v[b] for k, v in full.items()}, "image %d alone" % b)


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
load_package(); api = import_module(PKG_NAME + ".api")
import dense_cases as dc
model = api.Model(sys.argv[2], classify=True)
imgs = np.random.default_rng(8).standard_normal((3, 3, 56, 84)).astype(np.float32)
out = {}
for reduce in ("argmax", "bins"):
    W, bias = dc.head_weights(21, 512, seed=77)
    kw = dict(reduce="bins", bin_centers=dc.bin_centers(21), bins_eps=0.1) if reduce == "bins" else {}
    head = api.DenseHead(model, [1, 2], W, bias, norm=True, concat_cls=True, **kw)
    r = api.Session(model).predict_dense(imgs, head, (50, 77), classify=True, predict_want=("cls", "logits"))
    pr = r.pop("predict")
    out.update({reduce + "_" + k: v for k, v in r.items()})
    out.update({reduce + "_predict_" + k: v for k, v in pr.items()})
np.savez(sys.argv[3], **out); print("DENSE_OK")
'''


def test_split_passes_equal_one_pass_in_a_fresh_process(api, golden_dir, tmp_path):
    """DINOV2_HIP_MAX_CHUNK=1: three passes of one image, last first, each writing at its image offset -- against the unsplit call of
    another fresh process, bit for bit, the classifier's outputs of the same call included."""
    res = []
    for chunk in ("1", "0"):
        f = str(tmp_path / ("dense%s.npz" % chunk))
        out = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), f], cwd=ROOT,
                             env=dict(os.environ, DINOV2_HIP_MAX_CHUNK=chunk), capture_output=True, text=True, timeout=600)
        assert "DENSE_OK" in out.stdout, out.stdout + out.stderr
        res.append(dict(np.load(f)))
    assert set(res[0]) == {"argmax_labels", "argmax_value", "argmax_logits", "argmax_predict_cls", "argmax_predict_logits", "bins_value", "bins_logits",
                           "bins_predict_cls", "bins_predict_logits"}
    _same(res[0], res[1], "split against unsplit")


def _device_call(api, sess, head, imgs, oh, ow, P, C_, want_labels):
    B = imgs.shape[0]
    lab = api.DeviceArray(((B * oh * ow + 3) // 4,), fill_nan=True) if want_labels else None
    val = api.DeviceArray((B, oh, ow), fill_nan=True)
    lg = api.DeviceArray((B, P, C_), fill_nan=True)
    do = api.DenseOut(oh, ow, lab.ptr if lab else None, val.ptr, lg.ptr, 1)
    i = api.Input(imgs.ctypes.data, B, imgs.shape[2], imgs.shape[3], api.RGB_CHW, 0)
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_predict_dense(sess._h, C.byref(i), None, head._h, C.byref(do), 0, err, len(err))
    assert rc == 0, err.value.decode()
    sess.sync()
    out = {"value": val.to_host(), "logits": lg.to_host()}
    if lab:
        out["labels"] = lab.to_host().view(np.uint8)[:B * oh * ow].reshape(B, oh, ow)
    return out


@pytest.mark.parametrize("reduce", ["argmax", "bins"])
def test_device_outputs_equal_host_outputs(api, golden_dir, reduce):
    model = _model(api, golden_dir, "tiny_gelu_noreg")
    head, sess = _head(api, model, reduce), api.Session(model)
    imgs = _images(2, (70, 70), 4)
    host = sess.predict_dense(imgs, head, (33, 51))
    dev = _device_call(api, sess, head, imgs, 33, 51, 25, 21, reduce == "argmax")
    _same(dev, host, "device outputs")


def test_out_of_the_same_call_and_the_session_afterwards(api, golden_dir):
    """`out` together with the dense outputs is a plain predict's; fetch, pca3 and match afterwards behave as after that predict."""
    model = _model(api, golden_dir, "tiny_gelu_reg4", classify=True)
    head = _head(api, model)
    imgs = _images(2, (56, 84), 6)
    plain_sess, sess = api.Session(model), api.Session(model)
    plain = plain_sess.predict(imgs, classify=True)
    r = sess.predict_dense(imgs, head, None, classify=True, predict_want=("cls", "patch_tokens", "logits", "probs"))
    for k in ("cls", "patch_tokens", "logits", "probs"):
        ok, msg = mc.check_exact(r["predict"][k], plain[k], "out." + k)
        assert ok, msg
    only = api.Session(model).predict_dense(imgs, head, None, classify=True)  # out = NULL
    _same({k: only[k] for k in ("labels", "value")}, {k: r[k] for k in ("labels", "value")}, "with and without out")
    fetched, o = api._alloc_outputs(model.hparams, 2, 56, 84, api.RGB_CHW, True, 0, ("cls", "logits"))
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_fetch(sess._h, C.byref(o), err, len(err)) == 0, err.value.decode()
    for k in ("cls", "logits"):
        ok, msg = mc.check_exact(fetched[k], plain[k], "fetch." + k)
        assert ok, msg
    for a, b in zip(sess.pca3(None, (28, 128)), plain_sess.pca3(None, (28, 128))):  # (classifying forward: rows 1 .. T - 1, registers included)
        ok, msg = mc.check_exact(a, b, "pca3 afterwards")
        assert ok, msg
    ma, mb = sess.match(shape=(24, 128)), plain_sess.match(shape=(24, 128))
    assert all(np.array_equal(ma[k], mb[k]) for k in ma)


def test_launches_are_booked_under_layer_tap_and_head(api, golden_dir):
    model = _model(api, golden_dir, "tiny_gelu_reg4")
    head, sess = _head(api, model), api.Session(model)
    imgs = _images(1, (42, 42), 2)
    sess.profile(True)
    sess.predict(imgs)
    base = sess.profile_read()
    sess.profile(True)
    sess.predict_dense(imgs, head)
    prof = sess.profile_read()
    assert prof["layer_tap"][1] == base["layer_tap"][1] + 2 and prof["head"][1] == base["head"][1] + 1
    assert all(prof[k][1] == base[k][1] for k in base if k not in ("layer_tap", "head"))


# ----------------------------------------------------------------------------------------------------------------- errors
def test_argument_errors_leave_the_outputs_alone(api, pkg, golden_dir, tmp_path):
    model = _model(api, golden_dir, "tiny_gelu_noreg")
    H, L = int(model.hparams.hidden_size), int(model.hparams.num_hidden_layers)
    W, bias = dc.head_weights(5, 2 * H, 1)
    cen = dc.bin_centers(5)

    def create(layers=(1, 2), n=None, C_=5, weight=W, reduce=0, centers=None, eps=0.1, null_desc=False, null_out=False, mdl=model):
        arr = (C.c_int32 * max(len(layers), 1))(*layers) if layers is not None else None
        d = api.DenseDesc(arr, len(layers) if n is None else n, 1, 0, C_, weight.ctypes.data if weight is not None else None, bias.ctypes.data,
                          reduce, centers.ctypes.data if centers is not None else None, eps)
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        rc = api.lib().dinov2_hip_dense_head_create(mdl._h if mdl else None, None if null_desc else C.byref(d), None if null_out else C.byref(h),
                                                    err, len(err))
        return rc, err.value.decode(), h

    bad_create = {"null model": dict(mdl=None), "null desc": dict(null_desc=True), "null out": dict(null_out=True), "null layers": dict(layers=None, n=1),
                  "null weight": dict(weight=None), "n_layers 0": dict(layers=(), n=0), "n_layers 9": dict(layers=(0, 1, 2), n=9),
                  "layer -1": dict(layers=(-1, 1)), "layer L + 1": dict(layers=(1, L + 1)), "not ascending": dict(layers=(1, 1)),
                  "descending": dict(layers=(2, 1)), "C = 1": dict(C_=1), "C = 257": dict(C_=257), "unknown reduce": dict(reduce=2),
                  "bins without centres": dict(reduce=1), "bins with eps 0": dict(reduce=1, centers=cen, eps=0.0),
                  "bins with eps < 0": dict(reduce=1, centers=cen, eps=-0.1)}
    for what, kw in bad_create.items():
        rc, msg, h = create(**kw)
        assert rc == 4 and msg and not h.value, (what, rc, msg)

    seg = api.DenseHead(model, [1, 2], W, bias)
    dep = api.DenseHead(model, [1, 2], W, bias, reduce="bins", bin_centers=cen)
    imgs = _images(2, (56, 84), 1)
    sess = api.Session(model)
    labels = np.full((2, 56, 84), 7, np.uint8)
    value = np.full((2, 56, 84), 7.0, np.float32)
    logits = np.full((2, 24, 5), 7.0, np.float32)
    dev = api.DeviceArray((2 * 56 * 84 + 8,), fill_nan=True)

    def call(head=seg, oh=0, ow=0, lab=True, val=True, lg=True, on_device=0, ptrs=None, null_in=False, null_out=False, s=sess, null_sess=False):
        p = ptrs or (labels.ctypes.data, value.ctypes.data, logits.ctypes.data)
        do = api.DenseOut(oh, ow, p[0] if lab else None, p[1] if val else None, p[2] if lg else None, on_device)
        i = api.Input(imgs.ctypes.data, 2, 56, 84, api.RGB_CHW, 0)
        err = C.create_string_buffer(256)
        rc = api.lib().dinov2_hip_predict_dense(None if null_sess else s._h, None if null_in else C.byref(i), None, head._h if head else None,
                                                None if null_out else C.byref(do), 0, err, len(err))
        return rc, err.value.decode()

    other_path = str(tmp_path / "other.gguf")
    pkg.synth.write_synthetic_gguf(other_path, "small", registers=0, num_classes=10, seed=1, layers=1)
    other = api.Model(other_path, classify=False)
    bad = {"null session": dict(null_sess=True), "null input": dict(null_in=True), "null head": dict(head=None), "null dense_out": dict(null_out=True),
           "out_h 0 with out_w given": dict(oh=0, ow=10), "out_h negative": dict(oh=-1, ow=10), "out_w 8193": dict(oh=10, ow=8193),
           "labels from a bins head": dict(head=dep), "all outputs NULL": dict(lab=False, val=False, lg=False),
           "misaligned device value": dict(on_device=1, lab=False, lg=False, ptrs=(None, dev.ptr + 4, None)),
           "misaligned device labels": dict(on_device=1, val=False, lg=False, ptrs=(dev.ptr + 1, None, None)),
           "a head of another model size": dict(s=api.Session(other))}
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == 4 and msg, (what, rc, msg)
        assert (labels == 7).all() and (value == 7.0).all() and (logits == 7.0).all(), what
    assert np.isnan(dev.to_host()).all()
    n = C.c_int(0)  # a session on another device than the head: only where there is a second device
    ndev = n.value if api.DeviceArray._rt().hipGetDeviceCount(C.byref(n)) == 0 else 1
    if ndev > 1:
        far = api.Model(os.path.join(golden_dir, "tiny_gelu_noreg.gguf"), device=1, classify=False)
        rc, msg = call(s=api.Session(far))
        assert rc == 4 and msg and (labels == 7).all(), (rc, msg)
    rc, msg = call()
    assert rc == 0, msg
    ref = api.Session(model).predict_dense(imgs, seg)
    assert np.array_equal(labels, ref["labels"]) and mc.diff_count(value, ref["value"]) == 0 and mc.diff_count(logits, ref["logits"]) == 0
