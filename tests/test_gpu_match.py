"""dinov2_hip_match_tokens on the device: the three kernels of csrc/match.hip through dinov2_hip_op_match (no model) against the cases of
tests/match_cases.py -- shapes at tile, K-padding and pass edges under the tolerance rule, exact probes bit for bit (tie rule, zero rows,
padding that must never win), planted matches, both directions from the same products, row independence -- and the call itself on a golden
model: resident sides against the fetched tokens, with and without DINOV2_HIP_CLASSIFY, mixed resident / host sides, device inputs,
argument errors, refusal after a split predict."""
import ctypes as C
import os

import numpy as np
import pytest

import match_cases as mc

pytestmark = pytest.mark.gpu

_REF = {}


def _shape_case(shape):
    """inputs + float64 reference of a shape, computed once and shared (never modified)."""
    if shape not in _REF:
        a, b = mc.shape_inputs(shape)
        _REF[shape] = (a, b, mc.reference(a, b))
    return _REF[shape]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", mc.SHAPES, ids=mc.shape_id)
def test_shapes_against_the_float64_cosine(api, shape):
    a, b, S = _shape_case(shape)
    report = []
    ok, msg = mc.check_against_reference(api.op_match(a, b), S, shape[2], "shape " + mc.shape_id(shape), report)
    print("\n".join(report))
    assert ok, msg


@pytest.mark.parametrize("kind,H", mc.PROBES, ids=lambda v: str(v))
def test_exact_probes_bit_for_bit(api, kind, H):
    a, b, exp = mc.build_probe(kind, H)
    ok, msg = mc.check_exact(api.op_match(a, b), exp, f"probe {kind} H={H}")
    assert ok, msg


def test_planted_matches_are_all_found_and_mutual(api):
    a, b, perm = mc.planted()
    ok, msg = mc.check_planted(api.op_match(a, b), perm, "planted")
    assert ok, msg


@pytest.mark.parametrize("shape", [(mc.TM + 1, 2 * mc.TN + 1, 384), (257, 300, 1536)], ids=mc.shape_id)
def test_both_directions_come_from_the_same_products(api, shape):
    """sim_ab[i] == sim_ba[idx_ab[i]] bit for bit on every mutual pair (and there are some)."""
    a, b, _ = _shape_case(shape)
    r = api.op_match(a, b)
    i = np.flatnonzero(r["idx_ba"][r["idx_ab"]] == np.arange(len(a)))
    assert len(i) > 0
    assert np.array_equal(_bits(r["sim_ab"][i]), _bits(r["sim_ba"][r["idx_ab"][i]]))
    j = np.flatnonzero(r["idx_ab"][r["idx_ba"]] == np.arange(len(b)))
    assert np.array_equal(_bits(r["sim_ba"][j]), _bits(r["sim_ab"][r["idx_ba"][j]]))


def test_a_row_does_not_depend_on_the_rows_that_travel_with_it(api):
    """Rows [0, n) and a subset of them (one alone, too) against the same b: identical bits; and the transposed problem gives the two
    directions exchanged, bit for bit."""
    a, b, _ = _shape_case((257, 300, 1536))
    full = api.op_match(a, b)
    pick = np.array([0, 3, 127, 128, 129, 200, 256])
    part = api.op_match(a[pick], b)
    assert np.array_equal(part["idx_ab"], full["idx_ab"][pick]) and np.array_equal(_bits(part["sim_ab"]), _bits(full["sim_ab"][pick]))
    one = api.op_match(a[200:201], b)
    assert one["idx_ab"][0] == full["idx_ab"][200] and _bits(one["sim_ab"])[0] == _bits(full["sim_ab"])[200]
    swapped = api.op_match(b, a)  # the transposed problem: the same products from the other operand slot
    assert np.array_equal(swapped["idx_ba"], full["idx_ab"]) and np.array_equal(_bits(swapped["sim_ba"]), _bits(full["sim_ab"]))
    assert np.array_equal(swapped["idx_ab"], full["idx_ba"]) and np.array_equal(_bits(swapped["sim_ab"]), _bits(full["sim_ba"]))


def test_op_refuses_sizes_out_of_range(api):
    x = np.zeros((2, 8), np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    i, f = np.zeros(2, np.int32), np.zeros(2, np.float32)
    args = lambda na, nb, H: (x.ctypes.data_as(fp), na, x.ctypes.data_as(fp), nb, H, i.ctypes.data_as(ip), f.ctypes.data_as(fp),  # noqa: E731
                              i.ctypes.data_as(ip), f.ctypes.data_as(fp))
    for na, nb, H in ((0, 2, 8), (2, 0, 8), (2, 2, 7), (2, 2, 4097), ((1 << 20) + 1, 2, 8)):
        assert api.lib().dinov2_hip_op_match(*args(na, nb, H)) == 4


# ------------------------------------------------------------------------------------------------------------------- the session call
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(17).standard_normal((2, 3, 84, 112)).astype(np.float32)
    return model, img


def _same(x, y, what):
    ok, msg = mc.check_exact(x, y, what)
    assert ok, msg
    assert np.array_equal(x["mutual"], y["mutual"]), what


def check_resident_match(api, model, img, classify):
    """The body of test_resident_sides_equal_the_fetched_patch_tokens for any model and batch of two images (also run off the family by
    tests/test_gpu_geometry_entry_points.py)."""
    sess = api.Session(model)
    R = int(model.hparams.num_register_tokens)
    tok = sess.predict(img, classify=classify, want=("patch_tokens",))["patch_tokens"]
    if classify:
        tok = tok[:, R:]
    P, H = tok.shape[1:]
    host = sess.match(tok[0], tok[1])
    _same(sess.match(None, None, image_a=0, image_b=1, shape=(P, H)), host, "resident x resident")
    _same(sess.match(None, tok[1], image_a=0), host, "resident x host")
    _same(sess.match(tok[0], None, image_b=1), host, "host x resident")
    back = sess.match(None, None, image_a=1, image_b=0, shape=(P, H))
    assert np.array_equal(back["idx_ab"], host["idx_ba"]) and np.array_equal(_bits(back["sim_ab"]), _bits(host["sim_ba"]))
    same = sess.match(None, None, image_a=1, image_b=1, shape=(P, H))  # an image against itself: every patch finds itself
    assert np.array_equal(same["idx_ab"], np.arange(P)) and same["mutual"].all()
    ok, msg = mc.check_against_reference(host, mc.reference(tok[0], tok[1]), H, "golden tokens")
    assert ok, msg
    _same(host, api.op_match(tok[0], tok[1]) | {"mutual": host["mutual"]}, "session call x testing op")


@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
def test_resident_sides_equal_the_fetched_patch_tokens(api, golden, classify):
    """match(None, None) on what the last predict left on the device == match(tok[0], tok[1]) on the fetched patch tokens, bit for bit;
    under DINOV2_HIP_CLASSIFY too, where the rows predict hands out start with the registers and the resident view must not."""
    model, img = golden
    assert int(model.hparams.num_register_tokens) == 4
    check_resident_match(api, model, img, classify)


def test_device_inputs(api, golden):
    model, img = golden
    sess = api.Session(model)
    a, b, _ = _shape_case((mc.TM + 1, 2 * mc.TN + 1, 384))
    host = sess.match(a, b)
    da, db = api.DeviceArray.from_host(a), api.DeviceArray.from_host(b)
    _same(sess.match(da, db), host, "device inputs")
    # a smaller problem after a larger one on the grown scratch: the padding is rewritten on every call
    small = sess.match(a[:5], b)
    assert np.array_equal(small["idx_ab"], host["idx_ab"][:5]) and np.array_equal(_bits(small["sim_ab"]), _bits(host["sim_ab"][:5]))
    da.free()
    db.free()


def _call(api, sess_h, **kw):
    """dinov2_hip_match_tokens with raw fields; returns (status, the four output arrays) -- outputs pre-filled with a sentinel."""
    na, nb = kw.get("na", 4), kw.get("nb", 4)
    n = 64
    out = [np.full(n, -7, np.int32), np.full(n, -7.0, np.float32), np.full(n, -7, np.int32), np.full(n, -7.0, np.float32)]
    ptrs = [o.ctypes.data for o in out]
    if kw.get("no_outputs"):
        ptrs = [None] * 4
    m = api.Match(kw.get("a"), kw.get("b"), na, nb, kw.get("H", 8), kw.get("image_a", 0), kw.get("image_b", 1), kw.get("on_device", 0), *ptrs)
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_match_tokens(sess_h, C.byref(m) if not kw.get("null_request") else None, err, len(err))
    return rc, out, err.value.decode()


def _untouched(out):
    return all((o == -7).all() for o in out)


def test_argument_errors_return_invalid_and_touch_nothing(api, golden, monkeypatch):
    model, img = golden
    x = np.ones((4, 8), np.float32)
    hx = x.ctypes.data
    fresh = api.Session(model)
    cases = {
        "null request": dict(a=hx, b=hx, null_request=True),
        "na = 0": dict(a=hx, b=hx, na=0),
        "nb too large": dict(a=hx, b=hx, nb=(1 << 20) + 1),
        "H = 7": dict(a=hx, b=hx, H=7),
        "H = 4097": dict(a=hx, b=hx, H=4097),
        "no outputs": dict(a=hx, b=hx, no_outputs=True),
        "resident side, no forward yet": dict(a=None, b=hx, na=48, H=32),
    }
    for name, kw in cases.items():
        rc, out, msg = _call(api, fresh._h, **kw)
        assert rc == 4 and _untouched(out), (name, rc, msg)
    rc, out, msg = _call(api, None, a=hx, b=hx)
    assert rc == 4 and _untouched(out), ("null session", rc, msg)

    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    P, H = tok.shape[1:]
    t1 = np.ascontiguousarray(tok[1])
    d = api.DeviceArray.from_host(np.ones((5, 8), np.float32))
    cases = {
        "na is not P": dict(a=None, b=t1.ctypes.data, na=P - 1, nb=P, H=H),
        "nb is not P": dict(a=t1.ctypes.data, b=None, na=P, nb=P + 1, H=H),
        "H is not the hidden size": dict(a=None, b=None, na=P, nb=P, H=H + 8),
        "image_a = -1": dict(a=None, b=None, na=P, nb=P, H=H, image_a=-1),
        "image_b = batch": dict(a=None, b=None, na=P, nb=P, H=H, image_b=2),
        "misaligned device a": dict(a=d.ptr + 4, b=d.ptr, H=8, on_device=1),
        "misaligned device b": dict(a=d.ptr, b=d.ptr + 8, H=8, on_device=1),
    }
    for name, kw in cases.items():
        rc, out, msg = _call(api, sess._h, **kw)
        assert rc == 4 and _untouched(out), (name, rc, msg)
    rc, out, msg = _call(api, sess._h, a=None, b=None, na=P, nb=P, H=H)  # the same request, in order: accepted
    assert rc == 0 and not _untouched(out), msg
    d.free()
    with pytest.raises(api.DinoError):
        sess.match(None, None, shape=(P + 1, H))

    # after a predict that was split into passes the session holds one pass only: nothing resident to match
    monkeypatch.setenv("DINOV2_HIP_MAX_CHUNK", "1")
    split = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    monkeypatch.delenv("DINOV2_HIP_MAX_CHUNK")
    assert np.array_equal(split, tok)
    rc, out, msg = _call(api, sess._h, a=None, b=None, na=P, nb=P, H=H)
    assert rc == 4 and _untouched(out), msg
    with pytest.raises(api.DinoError):
        sess.match(None, tok[1])
    assert sess.match(tok[0], tok[1])["idx_ab"].shape == (P,)  # host sides still work
