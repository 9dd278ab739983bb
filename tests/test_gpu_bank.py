"""dinov2_hip_bank_topk on the device: the kernels of csrc/bank.hip through dinov2_hip_op_bank_topk (no model) against the cases of
tests/bank_cases.py -- shapes at tile, K-padding, k and pass edges under the tolerance rule, exact probes bit for bit, chunkings that must
not matter, top-1 against dinov2_hip_op_match, row independence -- and the session calls on a golden model: incremental adds, clear,
resident CLS / patch rows against the fetched tokens, device inputs, argument errors, refusal after a split predict."""
import ctypes as C
import os

import numpy as np
import pytest

import bank_cases as bc
import match_cases as mc

pytestmark = pytest.mark.gpu

_REF = {}


def _shape_case(shape):
    """inputs + float64 reference of a shape, computed once and shared (never modified)."""
    if shape not in _REF:
        q, b = bc.shape_inputs(shape)
        _REF[shape] = (q, b, mc.reference(q, b))
    return _REF[shape]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(x, y, what):
    ok, msg = bc.check_exact(x, y, what)
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.shape_id)
def test_shapes_against_the_float64_cosine(api, shape):
    q, b, S = _shape_case(shape)
    report = []
    ok, msg = bc.check_against_reference(api.op_bank_topk(q, b, shape[3]), S, shape[2], shape[3], "shape " + bc.shape_id(shape), report)
    print("\n".join(report))
    assert ok, msg


@pytest.mark.parametrize("k", bc.PROBE_KS)
@pytest.mark.parametrize("kind,H", bc.PROBES, ids=lambda v: str(v))
def test_exact_probes_bit_for_bit(api, kind, H, k):
    q, b, exp = bc.probe_case(kind, H, k)
    _same(api.op_bank_topk(q, b, k), exp, f"probe {kind} H={H} k={k}")


def test_chunking_does_not_matter(api):
    q, b, _ = _shape_case((129, 257, 384, 64))
    base = api.op_bank_topk(q, b, 64, 0)
    for ct in bc.CHUNKINGS[1:]:
        _same(api.op_bank_topk(q, b, 64, ct), base, f"129x257x384x64 chunk_tiles={ct}")
    q, b, exp = bc.probe_case("duplicates", 72, 64)
    for ct in bc.CHUNKINGS:
        _same(api.op_bank_topk(q, b, 64, ct), exp, f"probe duplicates chunk_tiles={ct}")


def test_top1_is_match(api):
    """Slot 0 equals dinov2_hip_op_match's idx_ab / sim_ab bit for bit; a sampled slot j > 0 equals the match of that single pair."""
    for shape in ((129, 257, 384, 64), (257, 300, 1536, 33)):
        q, b, _ = _shape_case(shape)
        got = api.op_bank_topk(q, b, shape[3])
        m = api.op_match(q, b)
        assert np.array_equal(got["idx"][:, 0], m["idx_ab"]) and np.array_equal(_bits(got["sim"][:, 0]), _bits(m["sim_ab"]))
    rng = np.random.default_rng(3)
    for _ in range(32):
        i, j = int(rng.integers(len(q))), int(rng.integers(1, shape[3]))
        c = int(got["idx"][i, j])
        assert _bits(api.op_match(q[i:i + 1], b[c:c + 1])["sim_ab"])[0] == _bits(got["sim"][i, j]), (i, j, c)


def test_a_row_does_not_depend_on_the_rows_that_travel_with_it(api):
    q, b, _ = _shape_case((257, 300, 1536, 33))
    full = api.op_bank_topk(q, b, 33)
    pick = np.array([0, 3, 127, 128, 129, 200, 256])
    part = api.op_bank_topk(q[pick], b, 33)
    _same(part, {"idx": full["idx"][pick], "sim": full["sim"][pick]}, "a subset of the queries")
    one = api.op_bank_topk(q[200:201], b, 33)
    _same(one, {"idx": full["idx"][200:201], "sim": full["sim"][200:201]}, "one query alone")


def test_op_refuses_sizes_out_of_range(api):
    x = np.zeros((2, 8), np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    i, f = np.zeros(128, np.int32), np.zeros(128, np.float32)
    for nq, nb, H, k, ct in ((0, 2, 8, 1, 0), (2, 0, 8, 1, 0), (2, 2, 7, 1, 0), (2, 2, 4097, 1, 0), (2, 2, 8, 0, 0), (2, 2, 8, 65, 0),
                             ((1 << 20) + 1, 2, 8, 1, 0), (2, (1 << 24) + 1, 8, 1, 0), (2, 2, 8, 1, -1)):
        rc = api.lib().dinov2_hip_op_bank_topk(x.ctypes.data_as(fp), nq, x.ctypes.data_as(fp), nb, H, k, ct, i.ctypes.data_as(ip), f.ctypes.data_as(fp))
        assert rc == 4, (nq, nb, H, k, ct)


# ------------------------------------------------------------------------------------------------------------------- the session calls
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(17).standard_normal((2, 3, 84, 112)).astype(np.float32)
    return model, img


class _SessionBank:
    """api.Bank with its session, in the shape bank_cases.scenario_failures drives."""

    def __init__(self, api, model, sess, H, capacity):
        self.bank, self.sess = api.Bank(model, H, capacity), sess

    def add(self, rows):
        return self.bank.add(self.sess, rows)

    def clear(self):
        self.bank.clear()

    def topk(self, q, k):
        return self.bank.topk(self.sess, q, k)

    @property
    def count(self):
        return self.bank.count


def test_incremental_adds_clear_and_refill(api, golden):
    """Adds of 1, 130 and 169 rows equal one add; a full bank refuses; after clear() and a shorter refill the stale rows (copies of the
    queries: similarity 1) never appear, at k = 5 and at k = 64."""
    model, _ = golden
    sess = api.Session(model)
    assert bc.scenario_failures(lambda H, cap: _SessionBank(api, model, sess, H, cap)) == []


def check_resident_bank(api, model, img, classify):
    """The body of test_resident_rows_equal_the_fetched_tokens for any model and batch of two images with at least five patches each (also
    run off the family by tests/test_gpu_geometry_entry_points.py): k = 5 neighbours.  Returns the top-3 of the CLS rows (on a model whose two
    CLS rows are equal after the f16 normalisation both find row 0: that each finds itself is asserted where the images make them differ)."""
    sess = api.Session(model)
    R = int(model.hparams.num_register_tokens)
    out = sess.predict(img, classify=classify, want=("cls", "patch_tokens"))
    tok, cls = out["patch_tokens"], out["cls"]
    if classify:
        tok = tok[:, R:]
    P, H = tok.shape[1:]
    bank = api.Bank(model, H, 2 + P)
    assert bank.add(sess, source="last_cls") == 0 and bank.count == 2
    assert bank.add(sess, source="last_patches", image=0) == 2 and bank.count == 2 + P
    rows = np.concatenate([cls, tok[0]])
    resident = bank.topk(sess, k=5, source="last_patches", image=1)
    _same(bank.topk(sess, tok[1], 5), resident, "host rows x resident")
    d = api.DeviceArray.from_host(tok[1])
    _same(bank.topk(sess, d, 5), resident, "DeviceArray x resident")
    d.free()
    _same(api.op_bank_topk(tok[1], rows, 5), resident, "testing op x resident")
    ok, msg = bc.check_against_reference(resident, mc.reference(tok[1], rows), H, 5, "golden tokens")
    assert ok, msg
    rc = bank.topk(sess, k=3, source="last_cls")
    _same(rc, api.op_bank_topk(cls, rows, 3), "LAST_CLS queries")
    # a bank filled from host rows holds the same bits
    host = api.Bank(model, H, 2 + P)
    assert host.add(sess, rows) == 0
    _same(host.topk(sess, tok[1], 5), resident, "bank of host rows")
    # a smaller problem after a larger one on the grown scratch
    big = bank.topk(sess, np.concatenate([tok[1]] * 12), 64)
    small = bank.topk(sess, tok[1][:3], 5)
    _same(small, {"idx": resident["idx"][:3], "sim": resident["sim"][:3]}, "small after large")
    assert np.array_equal(big["idx"][:P, :5], resident["idx"])
    bank.free()
    host.free()
    return rc


@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
def test_resident_rows_equal_the_fetched_tokens(api, golden, classify):
    model, img = golden
    rc = check_resident_bank(api, model, img, classify)
    assert np.array_equal(rc["idx"][:, 0], [0, 1])  # every CLS row finds itself


def _add(api, sess_h, bank_h, **kw):
    first = C.c_int32(-7)
    r = api.Rows(kw.get("source", 0), kw.get("data"), kw.get("n", 4), kw.get("H", 8), kw.get("image", 0), kw.get("on_device", 0))
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_bank_add(sess_h, bank_h, None if kw.get("null_rows") else C.byref(r), C.byref(first), err, len(err))
    return rc, first.value == -7, err.value.decode()


def _topk(api, sess_h, bank_h, **kw):
    k = kw.get("k", 2)
    idx, sim = np.full(64 * 64, -7, np.int32), np.full(64 * 64, -7.0, np.float32)
    r = api.Rows(kw.get("source", 0), kw.get("data"), kw.get("n", 4), kw.get("H", 8), kw.get("image", 0), kw.get("on_device", 0))
    t = api.TopK(r, k, None if kw.get("no_outputs") else idx.ctypes.data, None if kw.get("no_outputs") else sim.ctypes.data)
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_bank_topk(sess_h, bank_h, None if kw.get("null_request") else C.byref(t), err, len(err))
    return rc, bool((idx == -7).all() and (sim == -7.0).all()), err.value.decode()


def test_argument_errors_return_invalid_and_touch_nothing(api, golden, monkeypatch):
    model, img = golden
    L = api.lib()
    err = C.create_string_buffer(256)
    h = C.c_void_p()
    for H, cap in ((7, 4), (4097, 4), (8, 0), (8, (1 << 24) + 1)):
        assert L.dinov2_hip_bank_create(model._h, H, cap, C.byref(h), err, len(err)) == 4 and not h.value, (H, cap)
    assert L.dinov2_hip_bank_create(None, 8, 4, C.byref(h), err, len(err)) == 4
    assert L.dinov2_hip_bank_create(model._h, 8, 4, None, err, len(err)) == 4
    assert L.dinov2_hip_bank_count(None) == 0 and L.dinov2_hip_bank_clear(None) == 4

    x = np.ones((4, 8), np.float32)
    hx = x.ctypes.data
    d = api.DeviceArray.from_host(np.ones((5, 8), np.float32))
    fresh = api.Session(model)
    bank = api.Bank(model, 8, 6)
    empty = api.Bank(model, 8, 6)
    assert bank.add(fresh, x) == 0
    common = {
        "null rows / request": dict(data=hx, null_rows=True, null_request=True),
        "n = 0": dict(data=hx, n=0),
        "H is not the bank's": dict(data=hx, H=16),
        "GIVEN without data": dict(data=None),
        "unknown source": dict(data=hx, source=3),
        "resident source, no forward yet": dict(source=1, n=2),
        "misaligned device pointer": dict(data=d.ptr + 4, on_device=1),
    }
    for name, kw in common.items():
        rc, untouched, msg = _add(api, fresh._h, bank._h, **kw)
        assert rc == 4 and untouched and bank.count == 4, ("add", name, rc, msg)
        rc, untouched, msg = _topk(api, fresh._h, bank._h, **kw)
        assert rc == 4 and untouched, ("topk", name, rc, msg)
    for name, kw in {"k = 0": dict(data=hx, k=0), "k = 65": dict(data=hx, k=65), "no outputs": dict(data=hx, no_outputs=True)}.items():
        rc, untouched, msg = _topk(api, fresh._h, bank._h, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    rc, untouched, msg = _topk(api, fresh._h, empty._h, data=hx)
    assert rc == 4 and untouched, ("empty bank", rc, msg)
    for s_h, b_h in ((None, bank._h), (fresh._h, None)):
        assert _add(api, s_h, b_h, data=hx)[:2] == (4, True) and _topk(api, s_h, b_h, data=hx)[:2] == (4, True)
    rc, untouched, msg = _add(api, fresh._h, bank._h, data=hx, n=3)  # 4 of 6 held: 3 more do not fit
    assert rc == 4 and untouched and bank.count == 4, msg
    rc, untouched, msg = _topk(api, fresh._h, bank._h, data=d.ptr, on_device=1)  # the same kind of request, in order: accepted
    assert rc == 0 and not untouched, msg
    d.free()

    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    P, H = tok.shape[1:]
    res = api.Bank(model, H, 4 * P)
    wrong = api.Bank(model, H + 8, 4)
    cases = {
        "LAST_CLS with n that is not the batch": (res, dict(source=1, n=3, H=H)),
        "LAST_PATCHES with n that is not P": (res, dict(source=2, n=P - 1, H=H)),
        "image = -1": (res, dict(source=2, n=P, H=H, image=-1)),
        "image = batch": (res, dict(source=2, n=P, H=H, image=2)),
        "a resident source and a bank of another H": (wrong, dict(source=2, n=P, H=H + 8)),
    }
    assert res.add(sess, source="last_patches", image=0) == 0
    for name, (b, kw) in cases.items():
        n0 = b.count
        rc, untouched, msg = _add(api, sess._h, b._h, **kw)
        assert rc == 4 and untouched and b.count == n0, ("add", name, rc, msg)
        if b is res:
            rc, untouched, msg = _topk(api, sess._h, b._h, **kw)
            assert rc == 4 and untouched, ("topk", name, rc, msg)
    with pytest.raises(api.DinoError):
        res.add(sess, source="last_patches", image=5)

    # after a predict that was split into passes the session holds one pass only: nothing resident to add or to ask with
    monkeypatch.setenv("DINOV2_HIP_MAX_CHUNK", "1")
    split = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    monkeypatch.delenv("DINOV2_HIP_MAX_CHUNK")
    assert np.array_equal(split, tok)
    rc, untouched, msg = _add(api, sess._h, res._h, source=2, n=P, H=H)
    assert rc == 4 and untouched and res.count == P, msg
    rc, untouched, msg = _topk(api, sess._h, res._h, source=2, n=P, H=H)
    assert rc == 4 and untouched, msg
    with pytest.raises(api.DinoError):
        res.topk(sess, k=2, source="last_cls")
    assert res.topk(sess, tok[1], 2)["idx"].shape == (P, 2)  # host rows still work
    for b in (bank, empty, res, wrong):
        b.free()
