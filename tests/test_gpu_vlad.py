"""dinov2_hip_vlad_tokens on the device: the kernels of csrc/vlad.hip through dinov2_hip_op_vlad (no model) against the cases of
tests/vlad_cases.py -- the exact probes bit for bit, the assignment bit for bit against k-means' assign op, the Gaussian shapes under the raw
bound, the three normalised modes under theirs, a segment's bits wherever it travels -- and Session.vlad on a golden model: resident rows
against the fetched tokens and against each image's own forward, device rows, argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

import kmeans_cases as kc
import vlad_cases as vc

pytestmark = pytest.mark.gpu

_CASE = {}


def _shape_case(api, shape):
    """(inputs, the raw run) of a shape, computed once and shared (never modified)."""
    key = vc.shape_id(shape)
    if key not in _CASE:
        x, off, c = vc.shape_inputs(shape)
        _CASE[key] = (x, off, c, api.op_vlad(x, c, off, 0))
    return _CASE[key]


def _run(api):
    return lambda x, off, c, flags: api.op_vlad(x, c, off, flags)


def _same(a, b, what, keys=("vlad", "counts", "labels", "sim")):
    for k in keys:
        x, y = (vc.bits(a[k]), vc.bits(b[k])) if k in ("vlad", "sim") else (np.asarray(a[k]), np.asarray(b[k]))
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differ"


# ------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("kind", vc.PROBES)
def test_probes_bit_for_bit(api, kind):
    """Labels, counts and the raw residuals of the exact probes; a changed guard band raises inside op_vlad."""
    ok, msg = vc.check_probe(_run(api), kind)
    assert ok, msg


@pytest.mark.parametrize("shape", vc.SHAPES, ids=vc.shape_id)
def test_assignment_is_the_kmeans_assign_op_bit_for_bit(api, shape):
    x, off, c, raw = _shape_case(api, shape)
    a = api.op_kmeans_assign(x, c)
    assert np.array_equal(raw["labels"], a["labels"]) and np.array_equal(vc.bits(raw["sim"]), vc.bits(a["sim"]))
    ok, msg = kc.check_assign(raw, x, c, "assign " + vc.shape_id(shape))
    assert ok, msg


@pytest.mark.parametrize("shape", vc.SHAPES, ids=vc.shape_id)
def test_raw_residuals_are_inside_their_bound(api, shape):
    x, off, c, raw = _shape_case(api, shape)
    report = []
    ok, msg = vc.check_raw(raw, off, "raw " + vc.shape_id(shape), report)
    print(*report)
    assert ok, msg


@pytest.mark.parametrize("flags", [vc.INTRA, vc.L2, vc.INTRA | vc.L2], ids=["intra", "l2", "both"])
@pytest.mark.parametrize("shape", vc.SHAPES, ids=vc.shape_id)
def test_normalised_modes_are_inside_their_bounds(api, shape, flags):
    """Against the float64 normalisation of the device's own raw residuals; every row (INTRA) or segment (L2, both) has norm 0 or 1."""
    x, off, c, raw = _shape_case(api, shape)
    report = []
    ok, msg = vc.check_norm(api.op_vlad(x, c, off, flags), raw, flags, vc.shape_id(shape), report)
    print(*report)
    assert ok, msg


def test_a_segment_has_the_same_bits_wherever_it_travels(api):
    ok, msg = vc.check_position(_run(api))
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------------- the session
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(19).standard_normal((3, 3, 84, 112)).astype(np.float32)
    return model, img


def _session_run(api, sess, device):
    """run_fn of vlad_cases over Session.vlad: host rows (staged by the call) or a DeviceArray (on_device = 1)."""
    def fn(x, off, c, flags):
        rows = api.DeviceArray.from_host(np.ascontiguousarray(x, np.float32)) if device else x
        out = sess.vlad(rows, c, offsets=off, intra_norm=bool(flags & vc.INTRA), l2_norm=bool(flags & vc.L2), want=("vlad", "counts", "labels", "sim"))
        if device:
            rows.free()
        return out
    return fn


@pytest.mark.parametrize("device", [False, True], ids=["host_rows", "device_rows"])
def test_a_segment_has_the_same_bits_wherever_it_travels_through_the_session(api, golden, device):
    """The position case through dinov2_hip_vlad_tokens itself: alone and at positions 0, 2 and 4, in all four flag settings, with host rows
    and with device rows; and either kind gives the bits of the testing op."""
    model, _ = golden
    run = _session_run(api, api.Session(model), device)
    ok, msg = vc.check_position(run)
    assert ok, msg
    seg, c, lists = vc.position_case()
    x, off = lists[2]
    for flags in (0, vc.INTRA, vc.L2, vc.INTRA | vc.L2):
        _same(run(x, off, c, flags), api.op_vlad(x, c, off, flags), "session x testing op, flags %d" % flags)


@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
def test_resident_rows_equal_the_fetched_tokens_and_each_images_own_forward(api, golden, classify):
    model, img = golden
    sess = api.Session(model)
    R = int(model.hparams.num_register_tokens)
    want = ("vlad", "counts", "labels", "sim")
    tok = sess.predict(img, classify=classify, want=("cls", "patch_tokens"))["patch_tokens"]
    if classify:
        tok = tok[:, R:]
    B, P, H = tok.shape
    K = 5
    rng = np.random.default_rng(3)
    cen = (tok.reshape(B * P, H)[rng.integers(B * P, size=K)] * 1.7 + 0.3 * rng.standard_normal((K, H))).astype(np.float32)
    flat = np.ascontiguousarray(tok.reshape(B * P, H))
    off = vc.offsets_of([P] * B)
    for intra, l2 in ((False, False), (True, False), (False, True), (True, True)):
        kw = dict(intra_norm=intra, l2_norm=l2, want=want)
        every = sess.vlad(centers=cen, source="last_patches", all_images=True, **kw)
        assert every["vlad"].shape == (B, K, H) and (every["counts"].sum(1) == P).all()
        _same(every, sess.vlad(flat, cen, offsets=off, **kw), "all_images x GIVEN host rows with offsets")
        _same(every, api.op_vlad(flat, cen, off, (1 if intra else 0) | (2 if l2 else 0)), "all_images x testing op")
        d = api.DeviceArray.from_host(flat)
        _same(every, sess.vlad(d, cen, offsets=off, **kw), "all_images x DeviceArray with offsets")
        d.free()
        km = sess.kmeans(K=K, max_iter=0, init=cen, source="last_patches", all_images=True)
        assert np.array_equal(every["labels"], km["labels"]) and np.array_equal(vc.bits(every["sim"]), vc.bits(km["sim"]))
        for i in range(B):
            one = sess.vlad(centers=cen, source="last_patches", image=i, **kw)
            for k in ("vlad", "counts"):
                assert np.array_equal(one[k][0].view(np.uint32), every[k][i].view(np.uint32)), (i, k)
            assert np.array_equal(one["labels"], every["labels"][i * P:(i + 1) * P])
        # the session is as it was: the resident consumers still see the batch
        assert np.array_equal(sess.match(None, tok[1], image_a=1)["idx_ab"], np.arange(P))
    # image i's own batch-1 forward gives image i's descriptor of the batch
    kw = dict(want=want)
    every = sess.vlad(centers=cen, source="last_patches", all_images=True, **kw)
    for i in range(B):
        alone = api.Session(model)
        alone.predict(img[i:i + 1], classify=classify, want=("cls",))
        one = alone.vlad(centers=cen, source="last_patches", **kw)
        for k in ("vlad", "counts"):
            assert np.array_equal(one[k][0].view(np.uint32), every[k][i].view(np.uint32)), ("own forward", i, k)
        assert np.array_equal(one["labels"], every["labels"][i * P:(i + 1) * P])
        assert np.array_equal(vc.bits(one["sim"]), vc.bits(every["sim"][i * P:(i + 1) * P]))
    # a smaller problem after a larger one on the grown scratch; a subset of the outputs
    small = sess.vlad(tok[1], cen[:2], want=("vlad",))
    assert set(small) == {"vlad"} and np.array_equal(vc.bits(small["vlad"]), vc.bits(api.op_vlad(tok[1], cen[:2])["vlad"]))


def _vl(api, sess_h, **kw):
    n, H, K, n_seg = kw.get("n", 6), kw.get("H", 8), kw.get("K", 2), kw.get("n_seg", 2)
    vl, cnt = np.full(64 * 64, -7.0, np.float32), np.full(256, -7, np.int32)
    lab, sim = np.full(256, -7, np.int32), np.full(256, -7.0, np.float32)
    r = api.Rows(kw.get("source", 0), kw.get("data"), n, H, kw.get("image", 0), kw.get("on_device", 0))
    no = kw.get("no_outputs")
    v = api.Vlad(r, kw.get("all_images", 0), kw.get("offsets"), n_seg, K, kw.get("centers"), kw.get("flags", 3),
                 None if no else vl.ctypes.data, None if no else cnt.ctypes.data, None if no else lab.ctypes.data, None if no else sim.ctypes.data)
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_vlad_tokens(sess_h, None if kw.get("null_request") else C.byref(v), err, len(err))
    untouched = bool((vl == -7.0).all() and (cnt == -7).all() and (lab == -7).all() and (sim == -7.0).all())
    return rc, untouched, err.value.decode()


def test_argument_errors_return_invalid_and_touch_nothing(api, golden):
    model, img = golden
    x = np.ones((6, 8), np.float32)
    x[1, 0] = x[2, 1] = -1.0
    hx = x.ctypes.data
    off = np.array([0, 2, 6], np.int32)
    bad = {k: np.array(v, np.int32) for k, v in dict(first=[1, 2, 6], flat=[0, 2, 2], back=[0, 4, 3], short=[0, 2, 5], long=[0, 2, 7]).items()}
    d = api.DeviceArray.from_host(np.ones((7, 8), np.float32))
    fresh = api.Session(model)
    ok = dict(data=hx, centers=hx, offsets=off.ctypes.data)
    cases = {
        "null request": dict(ok, null_request=True),
        "n = 0": dict(ok, n=0),
        "n = 2^20 + 1": dict(ok, n=(1 << 20) + 1),
        "H = 7": dict(ok, H=7),
        "H = 4097": dict(ok, H=4097),
        "K = 0": dict(ok, K=0),
        "K = 1025": dict(ok, K=1025),
        "n_seg = 0": dict(ok, n_seg=0),
        "n_seg = 4097": dict(ok, n_seg=4097),
        "n_seg K H above 2^28": dict(ok, n=(1 << 20), n_seg=4096, K=1024, H=4096),
        "centers == NULL": dict(data=hx, offsets=off.ctypes.data),
        "unknown flag bit": dict(ok, flags=4),
        "no outputs": dict(ok, no_outputs=True),
        "offsets NULL with two segments": dict(data=hx, centers=hx),
        "offsets[0] != 0": dict(ok, offsets=bad["first"].ctypes.data),
        "offsets not strictly ascending": dict(ok, offsets=bad["flat"].ctypes.data),
        "offsets descending": dict(ok, offsets=bad["back"].ctypes.data),
        "offsets end before n": dict(ok, offsets=bad["short"].ctypes.data),
        "offsets end after n": dict(ok, offsets=bad["long"].ctypes.data),
        "GIVEN without data": dict(centers=hx, offsets=off.ctypes.data),
        "all_images with GIVEN": dict(ok, all_images=1),
        "all_images = 2": dict(centers=hx, all_images=2, source=2, n_seg=1),
        "LAST_CLS": dict(centers=hx, source=1, n=3, n_seg=1),
        "unknown source": dict(centers=hx, source=3, n_seg=1),
        "offsets with a resident source": dict(centers=hx, offsets=off.ctypes.data, source=2),
        "resident source, no forward yet": dict(centers=hx, source=2, n=3, n_seg=1),
        "all_images, no forward yet": dict(centers=hx, source=2, n=3, n_seg=1, all_images=1),
        "misaligned device pointer": dict(ok, data=d.ptr + 4, on_device=1),
    }
    for name, kw in cases.items():
        rc, untouched, msg = _vl(api, fresh._h, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    assert _vl(api, None, **ok)[:2] == (4, True)
    rc, untouched, msg = _vl(api, fresh._h, **dict(ok, data=d.ptr, on_device=1))  # the same kind of request, in order
    assert rc == 0 and not untouched, msg
    d.free()

    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    B, P, H = tok.shape
    cen = np.ascontiguousarray(tok[0, :2])
    before = sess.vlad(centers=cen, source="last_patches", all_images=True)
    res = dict(centers=cen.ctypes.data, H=H)
    cases = {
        "LAST_CLS after a forward": dict(res, source=1, n=B, n_seg=1),
        "LAST_PATCHES with n that is not P": dict(res, source=2, n=P - 1, n_seg=1),
        "LAST_PATCHES with two segments": dict(res, source=2, n=P, n_seg=2),
        "all_images with n = P": dict(res, source=2, n=P, n_seg=B, all_images=1),
        "all_images with n_seg = 1": dict(res, source=2, n=B * P, n_seg=1, all_images=1),
        "image = -1": dict(res, source=2, n=P, n_seg=1, image=-1),
        "image = batch": dict(res, source=2, n=P, n_seg=1, image=B),
        "a resident source with another H": dict(res, source=2, n=P, n_seg=1, H=H + 8),
    }
    for name, kw in cases.items():
        rc, untouched, msg = _vl(api, sess._h, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    with pytest.raises(api.DinoError):
        sess.vlad(centers=cen, source="last_patches", image=B)
    with pytest.raises(api.DinoError):
        sess.vlad(centers=cen, source="last_patches", offsets=[0, P])
    # the session's last forward is what it was
    _same(sess.vlad(centers=cen, source="last_patches", all_images=True), before, "after the refusals", keys=("vlad", "counts"))
    assert np.array_equal(sess.match(None, tok[2], image_a=2)["idx_ab"], np.arange(P))
