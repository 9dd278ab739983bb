"""dinov2_hip_coreset_tokens and dinov2_hip_bank_keep on the device: the kernels of csrc/coreset.hip through dinov2_hip_op_coreset (no model)
against the cases of tests/coreset_cases.py -- one pick bit for bit against dinov2_hip_op_match, the greedy choice replayed exactly over the
device's own similarity bits, the probes bit for bit under every geometry -- and Session.coreset / Bank.keep / Session.kmeans(init="maximin")
on a golden model: resident rows and a bank against the fetched tokens, argument errors, and one bank whose rows end past 2^32 bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import coreset_cases as cc
import kmeans_cases as kc
import match_cases as mc
import rows_far_cases as rc

pytestmark = pytest.mark.gpu

_CASE = {}


def _shape_case(shape):
    """inputs of a shape, computed once and shared (never modified)."""
    if shape not in _CASE:
        _CASE[shape] = cc.shape_inputs(shape)
    return _CASE[shape]


def _same(got, exp, what):
    ok, msg = cc.same(got, exp, what)
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("shape", cc.SHAPES, ids=cc.shape_id)
def test_one_pick_is_match(api, shape):
    """m = 1: near_sim is sim_ab of match(rows, the first row alone) bit for bit, nearest is 0 everywhere."""
    x = _shape_case(shape)
    n = len(x)
    for first in sorted({0, n // 2, n - 1}):
        got = api.op_coreset(x, 1, first)
        m = api.op_match(x, x[first:first + 1])
        assert np.array_equal(cc.bits(got["near_sim"]), cc.bits(m["sim_ab"])), (shape, first)
        assert (got["nearest"] == 0).all() and got["selected"] == 1 and got["idx"][0] == first and got["cover"][0] == -np.inf


@pytest.mark.parametrize("shape", [s for s in cc.SHAPES if s[2] <= 64], ids=cc.shape_id)
def test_the_choice_replays_exactly_over_the_device_similarities(api, shape):
    """Every similarity of every row to the m picks comes from the already-tested bank top-k (k = m over a bank of the picked rows: the same
    bits by contract 2); the greedy rule replayed over those bits must give idx, cover, selected, nearest and near_sim bit for bit -- no
    tolerance on the choice, nothing skipped -- and each similarity is within match's tolerance of float64."""
    n, H, m = shape
    x = _shape_case(shape)
    first = n // 3
    got = api.op_coreset(x, m, first)
    assert got["selected"] == m and len(set(got["idx"].tolist())) == m and got["idx"].min() >= 0 and got["idx"].max() < n
    tk = api.op_bank_topk(x, x[got["idx"]], m)
    Sm = np.full((n, m), np.nan, np.float32)
    np.put_along_axis(Sm, tk["idx"], tk["sim"], axis=1)
    assert np.isfinite(Sm).all()
    err = np.abs(Sm.astype(np.float64) - mc.reference(x, x[got["idx"]])).max()
    print("coreset %s: max |sim - float64| %.3e (tol %.3e)" % (cc.shape_id(shape), err, mc.tol(H)))
    assert err <= mc.tol(H)
    pos = {int(r): u for u, r in enumerate(got["idx"])}

    def column(p):
        assert p in pos, f"the rule picks row {p}, the device did not"
        return Sm[:, pos[p]]

    _same(got, cc.greedy(column, n, n, m, first), "replay " + cc.shape_id(shape))


@pytest.mark.parametrize("kind", cc.PROBES)
def test_probes_bit_for_bit_under_every_geometry(api, kind):
    """One row tile per workgroup, both tiles in one workgroup, the planner's choice."""
    for rpw in (128, 256, 0):
        ok, msg = cc.check_probe(lambda x, m, first, stop, patch: api.op_coreset(x, m, first, stop, rpw), kind, f"rows_per_wg={rpw}")
        assert ok, msg


def test_the_result_does_not_depend_on_the_geometry(api):
    shape = (1374, 384, 64)
    x = _shape_case(shape)
    ref = api.op_coreset(x, 64, 5)
    stop = float(ref["cover"][40])
    for rpw in (128, 384, 640, 1408):  # 11, 4, 3 workgroups and one
        assert api.op_coreset_plan(1374, 384, 64, rpw)["nparts"] == -(-11 // (rpw // 128))
        _same(api.op_coreset(x, 64, 5, None, rpw), ref, f"rows_per_wg={rpw}")
        cut = api.op_coreset(x, 64, 5, stop, rpw)
        assert cut["selected"] == int(np.flatnonzero(ref["cover"] >= stop)[0]) and (cut["idx"][cut["selected"]:] == -1).all()
        assert np.array_equal(cut["idx"][:cut["selected"]], ref["idx"][:cut["selected"]]) and cut["nearest"].max() == cut["selected"] - 1


def test_a_row_does_not_depend_on_the_rows_that_travel_with_it(api):
    x = _shape_case((257, 72, 64))
    full = api.op_coreset(x, 1, 0)
    pick = np.array([0, 3, 127, 128, 129, 200, 256])
    part = api.op_coreset(x[pick], 1, 0)
    assert np.array_equal(cc.bits(part["near_sim"]), cc.bits(full["near_sim"][pick]))
    two = api.op_coreset(x[[0, 200]], 1, 0)
    assert cc.bits(two["near_sim"])[1] == cc.bits(full["near_sim"])[200]


def test_op_refuses_arguments_out_of_range(api):
    x = np.zeros((4, 8), np.float32)
    for bad in (dict(m=0), dict(m=5), dict(first=-1), dict(first=4), dict(stop_sim=np.nan), dict(rows_per_wg=-1)):
        kw = dict(m=2, first=0, stop_sim=None, rows_per_wg=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            api.op_coreset(x, **kw)
    with pytest.raises(ValueError):
        api.op_coreset(np.zeros((4, 7), np.float32), 1)


# ------------------------------------------------------------------------------------------------------------------- the session calls
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(17).standard_normal((3, 3, 84, 112)).astype(np.float32)
    return model, img


def test_resident_rows_and_a_bank_equal_the_fetched_tokens(api, golden):
    model, img = golden
    sess = api.Session(model)
    out = sess.predict(img, classify=False, want=("cls", "patch_tokens"))
    tok, cls = out["patch_tokens"], out["cls"]
    B, P, H = tok.shape
    m = 12
    resident = sess.coreset(m=m, first=2, source="last_patches", image=1)
    _same(resident, api.op_coreset(tok[1], m, 2), "resident patches x testing op")
    _same(resident, sess.coreset(tok[1], m=m, first=2), "resident patches x host rows")
    d = api.DeviceArray.from_host(tok[1])
    _same(resident, sess.coreset(d, m=m, first=2), "resident patches x DeviceArray")
    d.free()
    flat = tok.reshape(B * P, H)
    every = sess.coreset(m=m, first=P + 1, source="last_patches", all_images=True)
    _same(every, api.op_coreset(flat, m, P + 1), "all_images x testing op")
    assert every["idx"].max() >= P  # picks reach into the later images
    _same(sess.coreset(m=B, first=1, source="last_cls"), api.op_coreset(cls, B, 1), "LAST_CLS x testing op")
    stop = float(resident["cover"][7])
    _same(sess.coreset(m=m, first=2, stop_sim=stop, source="last_patches", image=1), api.op_coreset(tok[1], m, 2, stop), "stop_sim")

    # a bank of the rows: selecting from it equals selecting from the rows that were added to it
    bank = api.Bank(model, H, B * P + 5)
    assert bank.add(sess, source="last_patches", image=0) == 0 and bank.add(sess, tok[1]) == P and bank.add(sess, tok[2]) == 2 * P
    _same(sess.coreset(m=m, first=P + 1, bank=bank), every, "bank x the rows added to it")

    # keep: the thinned bank searches like a fresh bank of the kept rows
    kept = bank.keep(sess, every["idx"])
    assert np.array_equal(kept, np.sort(every["idx"])) and bank.count == m
    fresh = api.Bank(model, H, m)
    fresh.add(sess, flat[kept])
    q = tok[0, :40]
    a, b = bank.topk(sess, q, 5), fresh.topk(sess, q, 5)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(cc.bits(a["sim"]), cc.bits(b["sim"]))
    assert bank.add(sess, tok[0, :3]) == m  # and it fills up again from the new count
    for bad in ([-1], [m + 3], [0, 0]):
        with pytest.raises(ValueError):
            bank.keep(sess, bad)
    err = C.create_string_buffer(256)
    two = np.array([1, 1], np.int32)
    assert api.lib().dinov2_hip_bank_keep(sess._h, bank._h, api._ptr(two), 2, err, len(err)) == 4 and bank.count == m + 3
    assert api.lib().dinov2_hip_bank_keep(sess._h, bank._h, api._ptr(two), 0, err, len(err)) == 4
    assert api.lib().dinov2_hip_bank_keep(sess._h, bank._h, None, 1, err, len(err)) == 4 and bank.count == m + 3

    # maximin seeding of k-means = the coreset's picks as init rows
    K = 5
    seeds = sess.coreset(m=K, first=0, source="last_patches", image=1)["idx"]
    a = sess.kmeans(K=K, max_iter=3, init="maximin", source="last_patches", image=1)
    b = sess.kmeans(K=K, max_iter=3, init=seeds, source="last_patches", image=1)
    for k in ("labels", "counts", "iterations", "converged"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(kc.bits(a["sim"]), kc.bits(b["sim"])) and np.array_equal(kc.bits(a["centers"]), kc.bits(b["centers"]))
    assert np.array_equal(sess.kmeans(tok[2], K=K, max_iter=0, init="maximin", seed=7)["centers"],
                          tok[2][sess.coreset(tok[2], m=K, first=7 % P)["idx"]])

    # the session is as it was: the resident consumers still see the last forward
    mres = sess.match(None, tok[1], image_a=1)
    assert np.array_equal(mres["idx_ab"], np.arange(P))
    _same(sess.coreset(m=m, first=2, source="last_patches", image=1), resident, "small after large")
    bank.close()
    fresh.close()


def test_keep_whose_chunks_overlap_their_sources(api, golden):
    """H = 8 (128-byte f16 rows): one staging chunk is 262 144 rows.  Every third row of 900 000 is kept: 300 000 rows, two chunks.  The first
    chunk's destinations, rows [0, 262 144), hold a third of its own sources (hence the stage), and the second chunk's sources, rows past
    786 432, lie beyond everything the first chunk wrote (hence in place).  Many rows repeat, so the top-64 lists are decided by index."""
    model, _ = golden
    sess = api.Session(model)
    n, H = 900_000, 8
    x = kc.pm_rows(np.random.default_rng(3), 4096, H, nnz=(4,))[np.random.default_rng(4).integers(4096, size=n)]
    x[np.arange(n), np.arange(n) % H] *= 3.0  # (rows differ in more than sign patterns)
    bank = api.Bank(model, H, n)
    bank.add(sess, x)
    idx = np.arange(1, n, 3, dtype=np.int32)
    assert len(idx) > (32 << 20) // 128
    kept = bank.keep(sess, idx[::-1])
    assert np.array_equal(kept, idx) and bank.count == len(idx)
    fresh = api.Bank(model, H, len(idx))
    fresh.add(sess, x[idx])
    q = x[[0, 1, 4, n // 2, n - 2]]
    a, b = bank.topk(sess, q, 64), fresh.topk(sess, q, 64)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(cc.bits(a["sim"]), cc.bits(b["sim"]))
    pick = sess.coreset(m=4, first=0, bank=bank)
    _same(pick, sess.coreset(m=4, first=0, bank=fresh), "coreset of the thinned bank x of the fresh one")
    bank.close()
    fresh.close()


def _cs(api, sess_h, **kw):
    n, H, m = kw.get("n", 4), kw.get("H", 8), kw.get("m", 2)
    idx, cov = np.full(64, -7, np.int32), np.full(64, -7.0, np.float32)
    near, sim = np.full(64, -7, np.int32), np.full(64, -7.0, np.float32)
    sel = C.c_int32(-7)
    r = api.Rows(kw.get("source", 0), kw.get("data"), n, H, kw.get("image", 0), kw.get("on_device", 0))
    no = kw.get("no_outputs")
    c = api.Coreset(r, kw.get("all_images", 0), kw.get("bank"), m, kw.get("first", 0), kw.get("stop_sim", np.inf),
                    None if no else idx.ctypes.data, None if no else cov.ctypes.data, None if no else C.addressof(sel),
                    None if no else near.ctypes.data, None if no else sim.ctypes.data)
    err = C.create_string_buffer(256)
    rc_ = api.lib().dinov2_hip_coreset_tokens(sess_h, None if kw.get("null_request") else C.byref(c), err, len(err))
    untouched = bool((idx == -7).all() and (cov == -7.0).all() and (near == -7).all() and (sim == -7.0).all() and sel.value == -7)
    return rc_, untouched, err.value.decode()


def test_argument_errors_return_invalid_and_touch_nothing(api, golden):
    model, img = golden
    x = np.ones((4, 8), np.float32)
    x[1, 0] = x[2, 1] = -1.0
    hx = x.ctypes.data
    d = api.DeviceArray.from_host(np.ones((5, 8), np.float32))
    fresh = api.Session(model)
    empty = api.Bank(model, 8, 4)
    ok = dict(data=hx)
    cases = {
        "null request": dict(ok, null_request=True),
        "n = 0": dict(ok, n=0),
        "n = 2^20 + 1": dict(ok, n=(1 << 20) + 1),
        "H = 7": dict(ok, H=7),
        "H = 4097": dict(ok, H=4097),
        "m = 0": dict(ok, m=0),
        "m = n + 1": dict(ok, m=5),
        "first = -1": dict(ok, first=-1),
        "first = n": dict(ok, first=4),
        "NaN stop_sim": dict(ok, stop_sim=np.nan),
        "all_images with GIVEN": dict(ok, all_images=1),
        "all_images = 2": dict(ok, all_images=2, source=2),
        "no outputs": dict(ok, no_outputs=True),
        "GIVEN without data": dict(),
        "unknown source": dict(ok, source=3),
        "resident source, no forward yet": dict(source=1, n=3),
        "all_images, no forward yet": dict(source=2, n=3, all_images=1),
        "misaligned device pointer": dict(data=d.ptr + 4, on_device=1),
        "an empty bank": dict(bank=empty._h.value),
    }
    for name, kw in cases.items():
        rc_, untouched, msg = _cs(api, fresh._h, **kw)
        assert rc_ == 4 and untouched, (name, rc_, msg)
    assert _cs(api, None, **ok)[:2] == (4, True)
    rc_, untouched, msg = _cs(api, fresh._h, data=d.ptr, on_device=1)  # the same kind of request, in order
    assert rc_ == 0 and not untouched, msg
    empty.add(fresh, x)
    for name, kw in {"bank: m = count + 1": dict(bank=empty._h.value, m=5), "bank: first = count": dict(bank=empty._h.value, first=4)}.items():
        rc_, untouched, msg = _cs(api, fresh._h, **kw)
        assert rc_ == 4 and untouched, (name, rc_, msg)
    assert _cs(api, fresh._h, bank=empty._h.value, n=0, H=0)[0] == 0  # `rows` is not read with a bank
    d.free()
    empty.close()

    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    B, P, H = tok.shape
    res = dict(H=H)
    cases = {
        "LAST_CLS with n that is not the batch": dict(res, source=1, n=B + 1),
        "LAST_CLS with all_images": dict(res, source=1, n=B, all_images=1),
        "LAST_PATCHES with n that is not P": dict(res, source=2, n=P - 1),
        "all_images with n = P": dict(res, source=2, n=P, all_images=1),
        "image = -1": dict(res, source=2, n=P, image=-1),
        "image = batch": dict(res, source=2, n=P, image=B),
        "a resident source with another H": dict(res, source=2, n=P, H=H + 8),
    }
    for name, kw in cases.items():
        rc_, untouched, msg = _cs(api, sess._h, **kw)
        assert rc_ == 4 and untouched, (name, rc_, msg)
    assert _cs(api, sess._h, **dict(res, source=2, n=P))[0] == 0
    with pytest.raises(api.DinoError):
        sess.coreset(m=2, source="last_patches", image=B)
    with pytest.raises(ValueError):
        sess.coreset(tok[0])  # m is required


# ------------------------------------------------------------------------------------------------------------------- far rows
def _view(api, d, n):
    """The first n rows of DeviceArray d as a DeviceArray that owns nothing."""
    class View(api.DeviceArray):
        def __init__(self):
            pass

        def free(self):
            self.ptr = 0

    v = View()
    v.shape, v.nbytes, v.device, v.ptr = (int(n), d.shape[1]), 4 * int(n) * d.shape[1], d.device, d.ptr
    return v


def test_a_bank_whose_rows_end_past_2_to_the_32_bytes(api, golden):
    """H = 4096, 2^19 + 257 rows: the f16 bank ends just past 2^32 bytes.  It is filled on the device from the +-1 dictionary of
    tests/rows_far_cases.py, a rare entry planted on every row around the byte boundary; the rare entry of the row AT the boundary is the
    negated entry of `first`, so pick 1 -- similarity exactly -1, alone -- lies past the boundary.  A row's s depends on its dictionary entry
    alone, so the rule runs over columns gathered per entry; m = 3; idx, cover, selected, nearest and near_sim of every row bit for bit."""
    model, _ = golden
    c = rc.Case("C1", "bank", "bank", (1 << 19) + 257, 1, 4096, adds=(1 << 17,) * 4 + (257,))
    free, _ = api.device_memory()
    need = c.device_bytes() + (2 << 30)
    if free < need:
        pytest.skip("needs %.1f GiB of device memory, %.1f GiB are free" % (need / 2.0 ** 30, free / 2.0 ** 30))
    first = 1000
    boundary = rc.B32 // (c.hpad * 2)
    plants = dict(c.plant_list)
    ent = c.entries()
    assert first not in plants and boundary in plants and first < boundary < c.n
    dic = c.dictionary().copy()
    dic[plants[boundary]] = -dic[ent[first]]
    Sd = rc.exact_sims(dic, dic).astype(np.float32)
    exp = cc.greedy(lambda p: Sd[ent, ent[p]], c.n, c.n, 3, first)
    assert exp["idx"][1] == boundary and exp["cover"][1] == -1.0 and exp["selected"] == 3

    sess = api.Session(model)
    bank = api.Bank(model, c.H, c.n)
    src = api.DeviceArray((max(c.adds), c.H))
    try:
        at = 0
        for a in c.adds:
            api.op_rows_fill(src, at, a, dic, rc.D_COMMON, rc.SEED, c.plant_list)
            assert bank.add(sess, _view(api, src, a)) == at
            at += a
        _same(sess.coreset(m=3, first=first, bank=bank), exp, "far bank")
    finally:
        src.free()
        bank.close()
        sess.close()
