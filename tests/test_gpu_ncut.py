"""dinov2_hip_ncut_tokens on the device: the kernels of csrc/ncut.hip and the loop of csrc/ncut.cpp through the dinov2_hip_op_ncut* entry
points (no model) against the cases of tests/ncut_cases.py -- the exact probes bit for bit whatever the chunking, the Gaussian shapes and
the step under their bounds, the driver against eigh -- and Session.ncut / Session.tokencut on a golden model: resident rows against the
fetched tokens, device inputs, argument errors, refusal after a split predict and after predict_list, a stalled caller's stream."""
import ctypes as C
import os

import numpy as np
import pytest

import ncut_cases as nc

pytestmark = pytest.mark.gpu

KEYS = ("values", "vectors", "degree", "residual")


class Device:
    """The implementation interface of ncut_cases over the testing ops."""

    def __init__(self, api):
        self.api = api

    def apply(self, rows, affinity, tau, floor, scale, q, nchunk=0):
        return self.api.op_ncut_apply(rows, affinity, tau, floor, scale, q, nchunk)

    def step(self, rows, affinity, tau, floor, yprev, gprev_parts, nchunk=0):
        return self.api.op_ncut_step(rows, affinity, tau, floor, yprev, gprev_parts, nchunk)

    def run(self, rows, n_eig, affinity, tau, floor, max_iter, tol):
        return self.api.op_ncut(rows, n_eig, affinity, tau, floor, max_iter, tol)


def _same(a, b, what):
    for k in KEYS:
        x, y = nc.bits(np.asarray(a[k])), nc.bits(np.asarray(b[k]))
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differ"
    assert (a["iterations"], a["converged"]) == (b["iterations"], b["converged"]), what


def _run_case(api, name):
    lines = []
    bad = nc.CASES[name](Device(api), lines.append)
    for ln in lines:  # every figure before the assertion
        print(ln)
    assert bad == []


# ------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("case", [c for c in nc.CASES if c.startswith("probe_")])
def test_probes_bit_for_bit_whatever_the_chunking(api, case):
    _run_case(api, case)


@pytest.mark.parametrize("case", [c for c in nc.CASES if c.startswith("shape_")])
def test_shapes_inside_their_bounds(api, case):
    _run_case(api, case)


@pytest.mark.parametrize("case", list(nc.STEP_CASES))
def test_one_step_inside_its_bound(api, case):
    _run_case(api, case)


def test_apply_repeats_its_bits(api):
    """No atomics: two launches of a shape whose sums are not exact give the same bits."""
    rows, tau, floor, scale, q = nc.shape_case((300, 1536), "exp")
    a, b = (api.op_ncut_apply(rows, "exp", tau, floor, scale, q, 0, want=("t", "degree")) for _ in range(2))
    for k in ("t", "degree"):
        assert np.isfinite(a[k]).all() and np.array_equal(nc.bits(a[k]), nc.bits(b[k])), k


# ------------------------------------------------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("case", [c for c in nc.CASES if c.startswith("driver_")])
def test_driver_against_eigh(api, case):
    _run_case(api, case)


def test_exits_and_two_runs_with_identical_bits(api):
    _run_case(api, "exits")
    rows, _ = nc.planted("planted3")
    a, b = (api.op_ncut(rows, 3, "exp", nc.EXP_TAU, 0.0, nc.DRIVER_MAX_ITER, nc.DRIVER_TOL) for _ in range(2))
    _same(a, b, "two converged runs")
    assert a["converged"] and a["iterations"] % 8 == 0


def test_tokencut_mask_is_the_planted_foreground(api):
    rows, fg = nc.tokencut_expectation()
    res = api.op_ncut(rows, 2, "threshold", 0.2, 1e-5, nc.DRIVER_MAX_ITER, nc.DRIVER_TOL)
    assert res["converged"] and np.array_equal(api.tokencut_mask(res["vectors"][1]), fg)


def test_a_vertex_of_degree_zero_has_zero_entries(api):
    rows, aff, tau, floor, _ = nc.build_probe("zero_row")
    res = api.op_ncut(rows, 3, aff, tau, floor, 64, 1e-3)
    zero = np.abs(rows).sum(1) == 0
    assert zero.sum() == 3 and (res["degree"][zero] == 0).all() and (res["vectors"][:, zero] == 0).all()
    assert np.isfinite(res["vectors"]).all() and np.isfinite(res["values"]).all() and (res["degree"][~zero] > 0).all()


# ------------------------------------------------------------------------------------------------------------------- the session call
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(17).standard_normal((3, 3, 84, 112)).astype(np.float32)
    return model, img


ARGS = dict(n_eig=3, affinity="relu", tau=0.0, floor=0.0, max_iter=16, tol=1e-3)


def _op(api, rows, **kw):
    a = dict(ARGS, **kw)
    return api.op_ncut(rows, a["n_eig"], a["affinity"], a["tau"], a["floor"], a["max_iter"], a["tol"])


@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
def test_resident_rows_equal_the_fetched_tokens(api, golden, classify):
    model, img = golden
    sess = api.Session(model)
    R = int(model.hparams.num_register_tokens)
    out = sess.predict(img, classify=classify, want=("cls", "patch_tokens"))
    tok = out["patch_tokens"][:, R:] if classify else out["patch_tokens"]
    B, P, H = tok.shape
    resident = sess.ncut(source="last_patches", image=1, **ARGS)
    _same(resident, _op(api, tok[1]), "resident patches x testing op")
    _same(resident, sess.ncut(tok[1], **ARGS), "resident patches x host rows")
    d = api.DeviceArray.from_host(tok[1])
    _same(resident, sess.ncut(d, **ARGS), "resident patches x DeviceArray")
    d.free()
    assert resident["vectors"].shape == (3, P) and np.isfinite(resident["vectors"]).all() and abs(resident["values"][0]) < 1e-4
    flat = tok.reshape(B * P, H)
    every = sess.ncut(source="last_patches", all_images=True, **ARGS)
    _same(every, _op(api, flat), "all_images x testing op")
    _same(every, sess.ncut(flat, **ARGS), "all_images x host rows")
    # the three affinities through the session; TokenCut on image 1
    for aff, tau in (("threshold", 0.2), ("exp", 0.5)):
        kw = dict(ARGS, affinity=aff, tau=tau, floor=1e-5)
        _same(sess.ncut(source="last_patches", image=1, **kw), _op(api, tok[1], **kw), aff)
    v, mask = sess.tokencut(image=1, tau=0.2)
    ref = api.op_ncut(tok[1], 2, "threshold", 0.2, 1e-5, 1000, 1e-4)
    h0, w0 = model.grid(*img.shape[2:])
    assert v.shape == mask.shape == (h0, w0) and np.array_equal(nc.bits(v.ravel()), nc.bits(ref["vectors"][1]))
    assert np.array_equal(mask.ravel(), api.tokencut_mask(ref["vectors"][1]))
    # the session is as it was: the resident consumers still see the last forward
    comp, _, _ = sess.pca3(None, shape=(P + R if classify else P, H))
    assert np.isfinite(comp).all()
    assert np.array_equal(sess.match(None, tok[1], image_a=1)["idx_ab"], np.arange(P))
    init = np.array([1, 5, P - 1], np.int32)
    km = sess.kmeans(K=3, max_iter=2, init=init, source="last_patches", image=1)
    assert np.array_equal(km["labels"], api.op_kmeans(tok[1], 3, 2, init)["labels"])
    # a smaller problem after a larger one on the grown scratch
    _same(sess.ncut(tok[1], **ARGS), resident, "small after large")


def test_cls_rows_of_a_batch_of_sixteen(api, golden):
    model, _ = golden
    sess = api.Session(model)
    img = np.random.default_rng(19).standard_normal((16, 3, 28, 42)).astype(np.float32)
    cls = sess.predict(img, classify=False, want=("cls",))["cls"]
    kw = dict(ARGS, n_eig=2)
    _same(sess.ncut(source="last_cls", **kw), _op(api, cls, **kw), "LAST_CLS x testing op")


def test_a_call_behind_a_stalled_stream_equals_the_calm_call(api, golden):
    model, img = golden
    S = api.Stream()
    sess = api.Session(model, stream=S.handle)
    sess.predict(img, classify=False, want=("cls",))
    calm = sess.ncut(source="last_patches", image=2, **ARGS)
    api.stream_delay(S, 20)
    _same(sess.ncut(source="last_patches", image=2, **ARGS), calm, "behind a stalled stream")
    sess.sync()
    del sess
    S.destroy()


def _nc(api, sess_h, **kw):
    n, H = kw.get("n", 32), kw.get("H", 8)
    val, vec = np.full(8, -7.0, np.float32), np.full(8 * 64, -7.0, np.float32)
    deg, res = np.full(64, -7.0, np.float32), np.full(8, -7.0, np.float32)
    it, conv = C.c_int32(-7), C.c_int32(-7)
    r = api.Rows(kw.get("source", 0), kw.get("data"), n, H, kw.get("image", 0), kw.get("on_device", 0))
    no = kw.get("no_outputs")
    rq = api.NCut(r, kw.get("all_images", 0), kw.get("affinity", 1), kw.get("tau", 0.2), kw.get("floor", 0.0), kw.get("n_eig", 2),
                  kw.get("max_iter", 8), kw.get("tol", 1e-3), *(None if no else p for p in
                                                                (val.ctypes.data, vec.ctypes.data, deg.ctypes.data, res.ctypes.data,
                                                                 C.addressof(it), C.addressof(conv))))
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_ncut_tokens(sess_h, None if kw.get("null_request") else C.byref(rq), err, len(err))
    untouched = bool((val == -7.0).all() and (vec == -7.0).all() and (deg == -7.0).all() and (res == -7.0).all() and it.value == -7 and
                     conv.value == -7)
    return rc, untouched, err.value.decode()


def test_argument_errors_return_invalid_and_touch_nothing(api, golden, monkeypatch):
    model, img = golden
    x = np.random.default_rng(3).standard_normal((32, 8)).astype(np.float32)
    ok = dict(data=x.ctypes.data)
    d = api.DeviceArray.from_host(np.ones((33, 8), np.float32))
    fresh = api.Session(model)
    cases = {
        "null request": dict(ok, null_request=True), "n = 15": dict(ok, n=15), "n = 2^17 + 1": dict(ok, n=(1 << 17) + 1), "H = 7": dict(ok, H=7),
        "H = 4097": dict(ok, H=4097), "unknown affinity": dict(ok, affinity=3), "n_eig = 0": dict(ok, n_eig=0), "n_eig = 7": dict(ok, n_eig=7),
        "max_iter = 0": dict(ok, max_iter=0), "max_iter = 10 001": dict(ok, max_iter=10001), "tol = 1e-7": dict(ok, tol=1e-7),
        "tol = 0.2": dict(ok, tol=0.2), "threshold tau = 1": dict(ok, affinity=0, tau=1.0), "threshold floor = 2": dict(ok, affinity=0, floor=2.0),
        "exp tau = 2^-7": dict(ok, affinity=2, tau=2.0 ** -7), "exp tau = 17": dict(ok, affinity=2, tau=17.0),
        "all_images with GIVEN": dict(ok, all_images=1), "all_images = 2": dict(ok, all_images=2, source=2), "no outputs": dict(ok, no_outputs=True),
        "GIVEN without data": dict(), "unknown source": dict(ok, source=3), "resident source, no forward yet": dict(source=1, n=32),
        "all_images, no forward yet": dict(source=2, n=32, all_images=1), "misaligned device pointer": dict(data=d.ptr + 4, on_device=1),
    }
    for name, kw in cases.items():
        rc, untouched, msg = _nc(api, fresh._h, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    assert _nc(api, None, **ok)[:2] == (4, True)
    rc, untouched, msg = _nc(api, fresh._h, data=d.ptr, on_device=1)  # the same kind of request, in order
    assert rc == 0 and not untouched, msg
    d.free()

    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    B, P, H = tok.shape
    cases = {
        "LAST_CLS with n that is not the batch": dict(source=1, n=B + 16, H=H), "LAST_CLS of a batch below 16": dict(source=1, n=B, H=H),
        "LAST_CLS with all_images": dict(source=1, n=B, H=H, all_images=1), "LAST_PATCHES with n that is not P": dict(source=2, n=P - 1, H=H),
        "all_images with n = P": dict(source=2, n=P, H=H, all_images=1), "image = -1": dict(source=2, n=P, H=H, image=-1),
        "image = batch": dict(source=2, n=P, H=H, image=B), "a resident source with another H": dict(source=2, n=P, H=H + 8),
    }
    for name, kw in cases.items():
        rc, untouched, msg = _nc(api, sess._h, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    with pytest.raises(api.DinoError):
        sess.ncut(source="last_patches", image=B)

    # after a predict that was split into passes, and after a list forward, the session holds nothing resident
    monkeypatch.setenv("DINOV2_HIP_MAX_CHUNK", "1")
    split = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    monkeypatch.delenv("DINOV2_HIP_MAX_CHUNK")
    assert np.array_equal(split, tok)
    for kw in (dict(source=2, n=P, H=H), dict(source=2, n=B * P, H=H, all_images=1)):
        rc, untouched, msg = _nc(api, sess._h, **kw)
        assert rc == 4 and untouched, ("after a split predict", kw, msg)
    assert sess.ncut(tok[1], **ARGS)["vectors"].shape == (3, P)  # host rows still work
    sess.predict(img, classify=False, want=("patch_tokens",))
    assert _nc(api, sess._h, source=2, n=P, H=H)[0] == 0
    sess.predict_list([img[0], img[1][:, :56]])
    rc, untouched, msg = _nc(api, sess._h, source=2, n=P, H=H)
    assert rc == 4 and untouched, ("after predict_list", msg)
