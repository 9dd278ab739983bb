"""dinov2_hip_propagate on the device: the kernels of csrc/propagate.hip through dinov2_hip_op_propagate (no model) against the cases of
tests/propagate_cases.py -- Gaussian shapes under the tolerance rule and the derived output bound, exact probes and the duplicates probe bit
for bit, equality with the bank's top-k without a window, chunkings that must not matter, row independence -- and the session calls on a
golden model: the realtime chain (forward, propagate with keep, set without labels) against the same chain through the host, overwrite and
drop, argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

import propagate_cases as pc

pytestmark = pytest.mark.gpu


def _op(api):
    return lambda q, rows, labels, grid, slots, radius, k, T, ct: api.op_propagate(q, rows, labels, grid, slots, radius, k, T, ct)


def _same(x, y, what, keys=("idx", "sim", "labels", "argmax")):
    ok, msg = pc.check_exact(x, y, what, keys)
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.shape_id)
def test_shapes_selection_and_output(api, shape):
    """Selection against the float64 cosine restricted to the candidates; out against float64 from the returned idx and sim within twice
    the derived bound (propagate_cases: the output bound)."""
    report = []
    failures = pc.case_failures("shape " + pc.shape_id(shape), _op(api), margin=2.0, report=report)
    print("\n".join(report))
    assert failures == []


@pytest.mark.parametrize("radius", pc.PROBE_RADII)
@pytest.mark.parametrize("kind,H", pc.PROBES, ids=lambda v: str(v))
def test_exact_probes_bit_for_bit(api, kind, H, radius):
    for k in pc.PROBE_KS:
        assert pc.case_failures(f"probe {kind} H={H} r={radius} k={k}", _op(api)) == []


@pytest.mark.parametrize("name", list(pc.DUPLICATES))
def test_duplicates_probe_means_in_index_order(api, name):
    """All weights are 1: idx is the lowest k candidate indices; out, argmax and the kept copy are the f32 mean in index order, bit for bit."""
    assert pc.case_failures(name, _op(api)) == []


def test_without_a_window_it_is_the_bank(api):
    """radius = -1, slots 0 .. n - 1: idx and sim equal dinov2_hip_op_bank_topk on a bank of the same frames in slot order, bit for bit."""
    for shape in (pc.SHAPES[4], pc.SHAPES[1], pc.SHAPES[2]):
        h0, w0, H, frames, _, _, k, C = shape
        q, rows, labels = pc.shape_inputs(shape)
        got = api.op_propagate(q, rows, labels, (h0, w0), (1 << frames) - 1, -1, k, 0.1)
        _same(got, api.op_bank_topk(q, rows.reshape(-1, H), k), "shape " + pc.shape_id(shape), ("idx", "sim"))
    q, rows, labels, grid, slots, _ = pc.probe_case("duplicates", 72, -1, 64)
    _same(api.op_propagate(q, rows, labels, grid, slots, -1, 64, 0.1), api.op_bank_topk(q, rows.reshape(-1, 72), 64), "probe duplicates", ("idx", "sim"))


def test_chunking_does_not_matter(api):
    assert pc.case_failures("chunking", _op(api)) == []
    shape = pc.SHAPES[3]
    q, rows, labels = pc.shape_inputs(shape)
    base = api.op_propagate(q, rows, labels, shape[:2], shape[4], shape[5], 64, 0.1, 0)
    for ct in pc.CHUNKINGS[1:]:
        _same(api.op_propagate(q, rows, labels, shape[:2], shape[4], shape[5], 64, 0.1, ct), base, f"20x20 Gaussian chunk_tiles={ct}")


def test_a_query_does_not_depend_on_the_queries_that_travel_with_it(api):
    shape = pc.SHAPES[3]
    q, rows, labels = pc.shape_inputs(shape)
    full = api.op_propagate(q, rows, labels, shape[:2], shape[4], shape[5], 8, 0.1)
    pick = np.array([0, 19, 127, 128, 129, 210, 399])
    other = np.random.default_rng(5).standard_normal(q.shape).astype(np.float32)
    other[pick] = q[pick]
    part = api.op_propagate(other, rows, labels, shape[:2], shape[4], shape[5], 8, 0.1)
    _same({key: part[key][pick] for key in part}, {key: full[key][pick] for key in full}, "the kept queries among replaced ones")
    assert not np.array_equal(part["idx"], full["idx"])  # the replaced ones did change


def test_op_refuses_sizes_out_of_range(api):
    x = np.zeros(4 * 4 * 8 * 2, np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    i, f = np.zeros(4096, np.int32), np.zeros(4096, np.float32)
    ok = dict(h0=4, w0=4, H=8, frames=2, C=1, slots=3, radius=1, k=2, T=0.1, ct=0)
    for bad in (dict(h0=0), dict(w0=257), dict(H=7), dict(H=4097), dict(frames=0), dict(frames=65), dict(C=0), dict(C=257), dict(slots=0),
                dict(slots=4), dict(radius=-2), dict(radius=256), dict(k=0), dict(k=65), dict(T=0.0), dict(T=1e4), dict(T=float("nan")), dict(ct=-1)):
        a = dict(ok, **bad)
        rc = api.lib().dinov2_hip_op_propagate(x.ctypes.data_as(fp), x.ctypes.data_as(fp), x.ctypes.data_as(fp), a["h0"], a["w0"], a["H"],
                                               a["frames"], a["C"], a["slots"], a["radius"], a["k"], a["T"], a["ct"], f.ctypes.data_as(fp),
                                               i.ctypes.data_as(ip), i.ctypes.data_as(ip), f.ctypes.data_as(fp), None)
        assert rc == 4, bad


# ------------------------------------------------------------------------------------------------------------------- the session calls
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(23).standard_normal((3, 3, 84, 112)).astype(np.float32)
    return model, img


class _SessionMemory:
    """api.PropMemory with its session, in the shape propagate_cases.scenario_failures drives."""

    def __init__(self, api, model, sess, H, grid, frames, channels):
        self.mem, self.sess = api.PropMemory(model, H, grid, frames, channels), sess

    def set(self, slot, rows, labels=None):
        self.mem.set(self.sess, slot, rows, labels)

    def drop(self, slot):
        self.mem.drop(slot)

    def propagate(self, q, slots, radius, k, T, keep=False):
        return self.mem.propagate(self.sess, q, slots=slots, radius=radius, k=k, temperature=T, keep=keep)


def test_scenario_on_host_rows(api, golden):
    """set / propagate(keep) / set(labels=None) / overwrite / drop on synthetic frames: the kept labels equal labels passed through the host,
    an overwritten or dropped slot's old rows never appear, and the selection is the restatement's."""
    model, _ = golden
    sess = api.Session(model)
    assert pc.scenario_failures(lambda H, grid, frames, channels: _SessionMemory(api, model, sess, H, grid, frames, channels)) == []


def test_realtime_chain_on_resident_tokens(api, golden):
    """A batch of three images is forwarded; slot 0 is set from LAST_PATCHES of image 0 with given labels, image 1 is propagated as
    LAST_PATCHES with keep, slot 1 is set with labels = NULL, image 2 is propagated.  Every output is bit-equal to the same chain on the
    fetched tokens as GIVEN rows with the labels passed through the host, to device rows, and to the testing op."""
    model, img = golden
    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    P, H = tok.shape[1:]
    grid = (84 // 14, 112 // 14)
    assert P == grid[0] * grid[1]
    labels0 = np.random.default_rng(29).standard_normal((P, 3)).astype(np.float32)
    kw = dict(radius=2, k=4, temperature=0.1)
    res, host = api.PropMemory(model, H, grid, 2, 3), api.PropMemory(model, H, grid, 2, 3)
    res.set(sess, 0, labels=labels0, source="last_patches", image=0)
    host.set(sess, 0, tok[0], labels0)
    r1 = res.propagate(sess, slots=[0], keep=True, source="last_patches", image=1, **kw)
    h1 = host.propagate(sess, tok[1], slots=0b1, **kw)
    _same(r1, h1, "image 1: resident x given")
    res.set(sess, 1, source="last_patches", image=1)  # labels = NULL: what the propagate with keep left
    host.set(sess, 1, tok[1], h1["labels"])
    r2 = res.propagate(sess, slots=[0, 1], source="last_patches", image=2, **kw)
    h2 = host.propagate(sess, tok[2], slots=0b11, **kw)
    _same(r2, h2, "image 2: resident x given")
    d = api.DeviceArray.from_host(tok[2])
    _same(host.propagate(sess, d, slots=0b11, **kw), h2, "image 2: DeviceArray queries")
    d.free()
    _same(api.op_propagate(tok[2], np.stack([tok[0], tok[1]]), np.stack([labels0, h1["labels"]]), grid, 0b11, 2, 4, 0.1), h2, "image 2: testing op")
    only = res.propagate(sess, tok[2], slots=[1], want=("argmax",), **kw)
    assert list(only) == ["argmax"] and only["argmax"].shape == (P,)
    # overwrite slot 0 with image 2 itself: at radius 0 every query now finds its own cell in slot 0; then drop it
    res.set(sess, 0, tok[2], labels0)
    assert np.array_equal(res.propagate(sess, tok[2], slots=[0], radius=0, k=1)["idx"][:, 0], np.arange(P))
    res.drop(0)
    with pytest.raises(api.DinoError):
        res.propagate(sess, tok[2], slots=[0, 1], **kw)
    _same(res.propagate(sess, tok[2], slots=[1], **kw), host.propagate(sess, tok[2], slots=[1], **kw), "after a drop")
    res.free()
    host.free()


def _set(api, sess_h, mem_h, slot=0, labels=None, labels_on_device=0, **kw):
    r = api.Rows(kw.get("source", 0), kw.get("data"), kw.get("n", 6), kw.get("H", 8), kw.get("image", 0), kw.get("on_device", 0))
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_propmem_set(sess_h, mem_h, slot, None if kw.get("null_rows") else C.byref(r), labels, labels_on_device, err, len(err))
    return rc, err.value.decode()


def _propagate(api, sess_h, mem_h, **kw):
    k = kw.get("k", 2)
    lab, amax, idx, sim = np.full(4096, -7.0, np.float32), np.full(4096, -7, np.int32), np.full(4096, -7, np.int32), np.full(4096, -7.0, np.float32)
    r = api.Rows(kw.get("source", 0), kw.get("data"), kw.get("n", 6), kw.get("H", 8), kw.get("image", 0), kw.get("on_device", 0))
    none = kw.get("no_outputs")
    req = api.PropagateReq(r, kw.get("slots", 1), kw.get("radius", 1), k, kw.get("temperature", 0.1), kw.get("keep", 0),
                           None if none else lab.ctypes.data, None if none else amax.ctypes.data, None if none else idx.ctypes.data,
                           None if none else sim.ctypes.data)
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_propagate(sess_h, mem_h, None if kw.get("null_request") else C.byref(req), err, len(err))
    untouched = bool((lab == -7.0).all() and (amax == -7).all() and (idx == -7).all() and (sim == -7.0).all())
    return rc, untouched, err.value.decode()


def test_argument_errors_return_invalid_and_touch_nothing(api, golden):
    model, img = golden
    L = api.lib()
    err = C.create_string_buffer(256)
    h = C.c_void_p()
    # (frames * Ppad <= 2^24 cannot be passed inside the other limits: 64 x 65 536 = 2^22)
    for H, h0, w0, frames, Cn in ((7, 2, 3, 2, 1), (4097, 2, 3, 2, 1), (8, 0, 3, 2, 1), (8, 2, 257, 2, 1), (8, 2, 3, 0, 1), (8, 2, 3, 65, 1),
                                  (8, 2, 3, 2, 0), (8, 2, 3, 2, 257)):
        assert L.dinov2_hip_propmem_create(model._h, H, h0, w0, frames, Cn, C.byref(h), err, len(err)) == 4 and not h.value, (H, h0, w0, frames, Cn)
    assert L.dinov2_hip_propmem_create(None, 8, 2, 3, 2, 1, C.byref(h), err, len(err)) == 4
    assert L.dinov2_hip_propmem_create(model._h, 8, 2, 3, 2, 1, None, err, len(err)) == 4
    assert L.dinov2_hip_propmem_drop(None, 0) == 4

    fresh = api.Session(model)
    mem = api.PropMemory(model, 8, (2, 3), 2, 1)
    x = np.random.default_rng(1).standard_normal((6, 8)).astype(np.float32)
    lab = np.arange(6, dtype=np.float32).reshape(6, 1)
    hx, hl = x.ctypes.data, lab.ctypes.data
    d = api.DeviceArray.from_host(np.ones((7, 8), np.float32))
    assert L.dinov2_hip_propmem_drop(mem._h, 2) == 4 and L.dinov2_hip_propmem_drop(mem._h, -1) == 4
    rc, msg = _set(api, fresh._h, mem._h, data=hx, labels=None)
    assert rc == 4, ("labels == NULL with nothing kept", msg)
    mem.set(fresh, 0, x, lab)
    base = mem.propagate(fresh, x, slots=[0], radius=1, k=2)
    common = {
        "null rows / request": dict(data=hx, null_rows=True, null_request=True),
        "n = 0": dict(data=hx, n=0),
        "n is not P": dict(data=hx, n=5),
        "H is not the memory's": dict(data=hx, H=16),
        "GIVEN without data": dict(data=None),
        "unknown source": dict(data=hx, source=3),
        "LAST_CLS": dict(source=1, n=6),
        "resident source, no forward yet": dict(source=2, n=6),
        "misaligned device pointer": dict(data=d.ptr + 4, on_device=1),
    }
    for name, kw in common.items():
        rc, msg = _set(api, fresh._h, mem._h, labels=hl, **kw)
        assert rc == 4, ("set", name, rc, msg)
        rc, untouched, msg = _propagate(api, fresh._h, mem._h, **kw)
        assert rc == 4 and untouched, ("propagate", name, rc, msg)
    for name, kw in {"slot = -1": dict(slot=-1), "slot = frames": dict(slot=2),
                     "misaligned device labels": dict(labels=d.ptr + 4, labels_on_device=1)}.items():
        rc, msg = _set(api, fresh._h, mem._h, data=hx, **dict({"labels": hl}, **kw))
        assert rc == 4, ("set", name, rc, msg)
    for name, kw in {"k = 0": dict(k=0), "k = 65": dict(k=65), "radius = -2": dict(radius=-2), "radius = 256": dict(radius=256),
                     "T = 0": dict(temperature=0.0), "T = 1e4": dict(temperature=1e4), "T = nan": dict(temperature=float("nan")),
                     "T = inf": dict(temperature=float("inf")), "keep = 2": dict(keep=2), "no outputs, keep = 0": dict(no_outputs=True),
                     "no slot": dict(slots=0), "an empty slot": dict(slots=0b11), "a slot past frames": dict(slots=0b101)}.items():
        rc, untouched, msg = _propagate(api, fresh._h, mem._h, data=hx, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    for s_h, m_h in ((None, mem._h), (fresh._h, None)):
        assert _set(api, s_h, m_h, data=hx, labels=hl)[0] == 4 and _propagate(api, s_h, m_h, data=hx)[:2] == (4, True)
    # the memory is as it was: slot 0 alone is filled, its rows and labels unchanged, nothing kept
    _same(mem.propagate(fresh, x, slots=[0], radius=1, k=2), base, "after the refusals")
    assert _set(api, fresh._h, mem._h, slot=1, data=hx, labels=None)[0] == 4
    rc, untouched, msg = _propagate(api, fresh._h, mem._h, data=hx, no_outputs=True, keep=1)  # keep alone is a request: accepted
    assert rc == 0 and untouched, msg
    assert _set(api, fresh._h, mem._h, slot=1, data=hx, labels=None)[0] == 0
    d.free()

    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    P, H = tok.shape[1:]
    res = api.PropMemory(model, H, (6, 8), 2, 1)
    other = api.PropMemory(model, H, (8, 8), 2, 1)
    labs = np.zeros((64, 1), np.float32)
    res.set(sess, 0, labels=labs[:P], source="last_patches", image=0)
    for name, (m, kw) in {"image = -1": (res, dict(source=2, n=P, H=H, image=-1)), "image = batch": (res, dict(source=2, n=P, H=H, image=3)),
                          "LAST_PATCHES with n that is not P": (res, dict(source=2, n=P - 1, H=H)),
                          "a grid that is not the forward's": (other, dict(source=2, n=64, H=H))}.items():
        rc, msg = _set(api, sess._h, m._h, slot=1, labels=labs.ctypes.data, **kw)
        assert rc == 4, ("set", name, rc, msg)
        if m is res:
            rc, untouched, msg = _propagate(api, sess._h, m._h, **kw)
            assert rc == 4 and untouched, ("propagate", name, rc, msg)
    for m in (mem, res, other):
        m.free()
