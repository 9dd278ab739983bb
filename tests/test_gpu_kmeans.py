"""dinov2_hip_kmeans_tokens on the device: the kernels of csrc/kmeans.hip through the dinov2_hip_op_kmeans* entry points (no model) against
the cases of tests/kmeans_cases.py -- the assignment bit for bit against dinov2_hip_op_match, the update under its bound and bit for bit on
the exact probes whatever the chunking, the loop against the float64 Lloyd run -- and Session.kmeans on a golden model: resident rows against
the fetched tokens, device inputs, argument errors, refusal after a split predict and after predict_list."""
import ctypes as C
import os

import numpy as np
import pytest

import kmeans_cases as kc
import match_cases as mc

pytestmark = pytest.mark.gpu

_CASE = {}


def _shape_case(shape):
    """inputs of a shape, computed once and shared (never modified)."""
    if shape not in _CASE:
        _CASE[shape] = kc.shape_inputs(shape)
    return _CASE[shape]


def _same_run(a, b, what, loop=True):
    """labels, sim, centres and counts bit for bit; with `loop`, iterations and converged too."""
    keys = ("labels", "sim", "centers", "counts")
    for k in keys:
        x, y = (kc.bits(a[k]), kc.bits(b[k])) if k in ("sim", "centers") else (np.asarray(a[k]), np.asarray(b[k]))
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differ"
    for k in ("iterations", "converged") if loop else ():
        assert a[k] == b[k], f"{what}: {k} {a[k]} != {b[k]}"


# ------------------------------------------------------------------------------------------------------------------- assign
@pytest.mark.parametrize("shape", kc.SHAPES, ids=kc.shape_id)
def test_assign_is_match_bit_for_bit_and_inside_its_tolerance(api, shape):
    x, c = _shape_case(shape)
    got = api.op_kmeans_assign(x, c)
    m = api.op_match(x, c)
    assert np.array_equal(got["labels"], m["idx_ab"]) and np.array_equal(kc.bits(got["sim"]), kc.bits(m["sim_ab"]))
    ok, msg = kc.check_assign(got, x, c, "assign " + kc.shape_id(shape))
    assert ok, msg


def test_a_row_does_not_depend_on_the_rows_that_travel_with_it(api):
    x, c = _shape_case((257, 300, 1536))
    full = api.op_kmeans_assign(x, c)
    pick = np.array([0, 3, 127, 128, 129, 200, 256])
    part = api.op_kmeans_assign(x[pick], c)
    assert np.array_equal(part["labels"], full["labels"][pick]) and np.array_equal(kc.bits(part["sim"]), kc.bits(full["sim"][pick]))
    one = api.op_kmeans_assign(x[200:201], c)
    assert one["labels"][0] == full["labels"][200] and kc.bits(one["sim"])[0] == kc.bits(full["sim"])[200]


@pytest.mark.parametrize("kind", [k for k in kc.PROBES if k != "last_chunk"])
def test_assign_probes_bit_for_bit(api, kind):
    ok, msg = kc.check_probe_assign(api.op_kmeans_assign, kind, "probe")
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------------- update
def _update(api):
    return lambda x, labels, K, prev, nsplit: api.op_kmeans_update(x, labels, K, prev, nsplit)


@pytest.mark.parametrize("shape", kc.SHAPES, ids=kc.shape_id)
def test_update_counts_exact_and_sums_inside_the_bound(api, shape):
    """Random labels, all labels the same, clusters that straddle the chunk edges: exact counts, every S_c within (count_c + nsplit) 2^-24
    sum |x^| of the float64 sum of the device's own x^, empty clusters keep prev_centers bit for bit, guard bands intact (the op raises)."""
    n, K, H = shape
    x, c = _shape_case(shape)
    ns = api.op_kmeans_plan(n, K, H)["nsplit"]
    report = []
    for name, lab in kc.update_labelings(shape, 0).items():
        got = api.op_kmeans_update(x, lab, K, c)
        assert np.abs(got["xhat"] - mc.normalise_f16(x).astype(np.float32)).max() <= 2.0 ** -10, "x^ is not the normalised rows"
        ok, msg = kc.check_update(got, got["xhat"], lab, K, c, ns, f"update {kc.shape_id(shape)} {name}", report)
        print(report[-1] if ok else msg)
        assert ok, msg


@pytest.mark.parametrize("kind", kc.PROBES)
def test_update_probes_identical_bits_whatever_the_chunking(api, kind):
    for ns in (1, 2, 0, kc.NSPLIT_MAX):
        ok, msg = kc.check_probe_update(_update(api), kind, ns, "probe")
        assert ok, msg


def test_update_chunkings_agree_within_the_bound_and_repeat_their_bits(api):
    shape = (769, 300, 1536)
    n, K, H = shape
    x, c = _shape_case(shape)
    lab = kc.update_labelings(shape, 0)["random"]
    runs = {}
    for ns in (1, 2, 0, kc.NSPLIT_MAX):
        used = api.op_kmeans_plan(n, K, H, ns)["nsplit"]
        got = api.op_kmeans_update(x, lab, K, c, ns)
        again = api.op_kmeans_update(x, lab, K, c, ns)
        assert np.array_equal(kc.bits(got["centers"]), kc.bits(again["centers"])) and np.array_equal(got["counts"], again["counts"]), ns
        ok, msg = kc.check_update(got, got["xhat"], lab, K, c, used, f"nsplit={ns} ({used} chunks)")
        assert ok, msg
        runs[used] = got
    assert len(runs) >= 3, sorted(runs)  # the chunkings really differ


# ------------------------------------------------------------------------------------------------------------------- the loop
def test_driver_equals_the_float64_run_at_every_iteration(api):
    """op_kmeans on the driver cases and the loop probes: labels, counts, iterations and converged of the float64 Lloyd run for every
    max_iter up to convergence; max_iter = 0 returns the init vectors verbatim."""
    assert kc.run_failures(lambda x, K, m, init: api.op_kmeans(x, K, m, init)) == []


@pytest.mark.parametrize("which", kc.DRIVER_CASES)
def test_driver_results_are_consistent_with_the_kernels(api, which):
    d = kc.driver_case(which)
    x, K = d["x"], d["K"]
    full = api.op_kmeans(x, K, d["max_iter"], d["init"])
    assert full["converged"] and full["iterations"] >= 3
    _same_run(full, api.op_kmeans(x, K, d["max_iter"], x[d["init"]]), "row indices against the same rows as vectors")
    _same_run(full, api.op_kmeans(x, K, d["max_iter"], d["init"]), "two runs")
    a = api.op_kmeans_assign(x, full["centers"])
    assert np.array_equal(a["labels"], full["labels"]) and np.array_equal(kc.bits(a["sim"]), kc.bits(full["sim"]))
    u = api.op_kmeans_update(x, full["labels"], K, full["centers"])
    assert np.array_equal(kc.bits(u["centers"]), kc.bits(full["centers"])) and np.array_equal(u["counts"], full["counts"])
    back = api.op_kmeans(x, K, 0, full["centers"])
    _same_run(back, full, "centres fed back with max_iter = 0", loop=False)
    assert (back["iterations"], back["converged"]) == (0, False)
    cut = api.op_kmeans(x, K, 2, d["init"])  # the max_iter exit: labels / sim / counts are the assignment against the returned centres
    assert (cut["iterations"], cut["converged"]) == (2, False)
    a = api.op_kmeans_assign(x, cut["centers"])
    assert np.array_equal(a["labels"], cut["labels"]) and np.array_equal(kc.bits(a["sim"]), kc.bits(cut["sim"]))
    assert np.array_equal(cut["counts"], np.bincount(cut["labels"], minlength=K))


def test_op_refuses_sizes_out_of_range(api):
    x = np.zeros((2, 8), np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    i, f = np.zeros(128, np.int32), np.zeros(128, np.float32)
    xp = x.ctypes.data_as(fp)
    for n, K, H in ((0, 1, 8), ((1 << 20) + 1, 1, 8), (2, 0, 8), (2, 1025, 8), (2, 1, 7), (2, 1, 4097)):
        assert api.lib().dinov2_hip_op_kmeans_assign(xp, n, xp, K, H, i.ctypes.data_as(ip), f.ctypes.data_as(fp)) == 4, (n, K, H)
    bad = np.array([0, 2], np.int32)  # a label outside [0, K)
    assert api.lib().dinov2_hip_op_kmeans_update(xp, 2, bad.ctypes.data_as(ip), 2, 8, 0, xp, f.ctypes.data_as(fp), i.ctypes.data_as(ip), None) == 4


# ------------------------------------------------------------------------------------------------------------------- the session call
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(17).standard_normal((3, 3, 84, 112)).astype(np.float32)
    return model, img


def check_resident_kmeans(api, sess, img, classify, max_iter, init, max_iter_all, init_all):
    """The resident-row part of test_resident_rows_equal_the_fetched_tokens for any session and batch (also run off the family by
    tests/test_gpu_geometry_entry_points.py): the patch rows of image 1, and of every image, against the testing op, host rows and a
    DeviceArray, bit for bit, and inside the assign tolerance of the float64 cosine against the returned centres.  Returns (tok, cls, the
    image-1 result)."""
    R = int(sess.model.hparams.num_register_tokens)
    out = sess.predict(img, classify=classify, want=("cls", "patch_tokens"))
    tok, cls = out["patch_tokens"], out["cls"]
    if classify:
        tok = tok[:, R:]
    B, P, H = tok.shape
    K = len(init)
    resident = sess.kmeans(K=K, max_iter=max_iter, init=init, source="last_patches", image=1)
    _same_run(resident, api.op_kmeans(tok[1], K, max_iter, init), "resident patches x testing op")
    _same_run(resident, sess.kmeans(tok[1], K=K, max_iter=max_iter, init=init), "resident patches x host rows")
    d = api.DeviceArray.from_host(tok[1])
    _same_run(resident, sess.kmeans(d, K=K, max_iter=max_iter, init=init), "resident patches x DeviceArray")
    d.free()
    assert resident["labels"].shape == (P,) and resident["counts"].sum() == P
    ok, msg = kc.check_assign(resident, tok[1], resident["centers"], "resident patches")
    assert ok, msg
    # every image's patches, image-major; the init rows reach into the later images
    flat = tok.reshape(B * P, H)
    Ka = len(init_all)
    every = sess.kmeans(K=Ka, max_iter=max_iter_all, init=init_all, source="last_patches", all_images=True)
    _same_run(every, api.op_kmeans(flat, Ka, max_iter_all, init_all), "all_images x testing op")
    _same_run(every, sess.kmeans(flat, K=Ka, max_iter=max_iter_all, init=init_all), "all_images x host rows")
    ok, msg = kc.check_assign(every, flat, every["centers"], "all_images")
    assert ok, msg
    return tok, cls, resident


@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
def test_resident_rows_equal_the_fetched_tokens(api, golden, classify):
    model, img = golden
    sess = api.Session(model)
    R = int(model.hparams.num_register_tokens)
    P = int(np.prod(model.grid(*img.shape[2:])))
    init = np.array([1, 5, P - 1], np.int32)
    tok, cls, resident = check_resident_kmeans(api, sess, img, classify, 4, init, 3, np.array([0, P + 3, 2 * P + 7, 3 * P - 1], np.int32))
    B, P, H = tok.shape
    # CLS rows: one per image, strided through the token stream
    rc = sess.kmeans(K=2, max_iter=2, init=np.array([0, 2], np.int32), source="last_cls")
    _same_run(rc, api.op_kmeans(cls, 2, 2, np.array([0, 2], np.int32)), "LAST_CLS x testing op")
    # a vocabulary applied to the resident rows, and the seeded default init
    vocab = sess.kmeans(K=3, max_iter=0, init=resident["centers"], source="last_patches", image=1)
    _same_run(vocab, resident, "centres fed back with max_iter = 0", loop=False)
    seeded = sess.kmeans(tok[0], K=5, max_iter=3, seed=4)
    rows = np.sort(np.random.default_rng(4).choice(P, 5, replace=False)).astype(np.int32)
    _same_run(seeded, api.op_kmeans(tok[0], 5, 3, rows), "seeded init")
    # the session is as it was: the resident consumers still see the last forward
    comp, _, _ = sess.pca3(None, shape=(P + R if classify else P, H))  # (under classify pca3's resident rows include the registers)
    assert np.isfinite(comp).all()
    m = sess.match(None, tok[1], image_a=1)
    assert np.array_equal(m["idx_ab"], np.arange(P))
    # a smaller problem after a larger one on the grown scratch
    _same_run(sess.kmeans(tok[1], K=3, max_iter=4, init=init), resident, "small after large")


def _km(api, sess_h, **kw):
    n, H, K = kw.get("n", 4), kw.get("H", 8), kw.get("K", 2)
    lab, sim = np.full(64, -7, np.int32), np.full(64, -7.0, np.float32)
    cen, cnt = np.full(64 * 8, -7.0, np.float32), np.full(64, -7, np.int32)
    it, conv = C.c_int32(-7), C.c_int32(-7)
    r = api.Rows(kw.get("source", 0), kw.get("data"), n, H, kw.get("image", 0), kw.get("on_device", 0))
    no = kw.get("no_outputs")
    km = api.KMeans(r, kw.get("all_images", 0), K, kw.get("max_iter", 2), kw.get("init", 0), kw.get("init_centers"), kw.get("init_rows"),
                    None if no else lab.ctypes.data, None if no else sim.ctypes.data, None if no else cen.ctypes.data,
                    None if no else cnt.ctypes.data, None if no else C.addressof(it), None if no else C.addressof(conv))
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_kmeans_tokens(sess_h, None if kw.get("null_request") else C.byref(km), err, len(err))
    untouched = bool((lab == -7).all() and (sim == -7.0).all() and (cen == -7.0).all() and (cnt == -7).all() and it.value == -7 and conv.value == -7)
    return rc, untouched, err.value.decode()


def test_argument_errors_return_invalid_and_touch_nothing(api, golden, monkeypatch):
    model, img = golden
    x = np.ones((4, 8), np.float32)
    x[1, 0] = x[2, 1] = -1.0
    hx = x.ctypes.data
    idx = np.array([0, 3], np.int32)
    bad_lo, bad_hi = np.array([0, -1], np.int32), np.array([0, 4], np.int32)
    d = api.DeviceArray.from_host(np.ones((5, 8), np.float32))
    fresh = api.Session(model)
    ok = dict(data=hx, init_centers=hx)
    cases = {
        "null request": dict(ok, null_request=True),
        "n = 0": dict(ok, n=0),
        "n = 2^20 + 1": dict(ok, n=(1 << 20) + 1),
        "H = 7": dict(ok, H=7),
        "H = 4097": dict(ok, H=4097),
        "K = 0": dict(ok, K=0),
        "K = 1025": dict(ok, K=1025),
        "max_iter = -1": dict(ok, max_iter=-1),
        "max_iter = 1001": dict(ok, max_iter=1001),
        "unknown init": dict(ok, init=2),
        "INIT_GIVEN without centres": dict(data=hx),
        "INIT_ROWS without indices": dict(data=hx, init=1, init_centers=hx),
        "init row -1": dict(data=hx, init=1, init_rows=bad_lo.ctypes.data),
        "init row n": dict(data=hx, init=1, init_rows=bad_hi.ctypes.data),
        "all_images with GIVEN": dict(ok, all_images=1),
        "all_images = 2": dict(ok, all_images=2, source=2),
        "no outputs": dict(ok, no_outputs=True),
        "GIVEN without data": dict(init_centers=hx),
        "unknown source": dict(ok, source=3),
        "resident source, no forward yet": dict(source=1, n=3, init_centers=hx),
        "all_images, no forward yet": dict(source=2, n=3, all_images=1, init_centers=hx),
        "misaligned device pointer": dict(data=d.ptr + 4, on_device=1, init_centers=hx),
    }
    for name, kw in cases.items():
        rc, untouched, msg = _km(api, fresh._h, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    assert _km(api, None, **ok)[:2] == (4, True)
    rc, untouched, msg = _km(api, fresh._h, data=d.ptr, on_device=1, init=1, init_rows=idx.ctypes.data)  # the same kind of request, in order
    assert rc == 0 and not untouched, msg
    d.free()

    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    B, P, H = tok.shape
    cen = np.ascontiguousarray(tok[0, :2])
    res = dict(init_centers=cen.ctypes.data, H=H)
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
        rc, untouched, msg = _km(api, sess._h, **kw)
        assert rc == 4 and untouched, (name, rc, msg)
    with pytest.raises(api.DinoError):
        sess.kmeans(K=2, source="last_patches", image=B)

    # after a predict that was split into passes, and after a list forward, the session holds nothing resident
    monkeypatch.setenv("DINOV2_HIP_MAX_CHUNK", "1")
    split = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    monkeypatch.delenv("DINOV2_HIP_MAX_CHUNK")
    assert np.array_equal(split, tok)
    for kw in (dict(res, source=2, n=P), dict(res, source=2, n=B * P, all_images=1), dict(res, source=1, n=B)):
        rc, untouched, msg = _km(api, sess._h, **kw)
        assert rc == 4 and untouched, ("after a split predict", kw, msg)
    assert sess.kmeans(tok[1], K=2, max_iter=1, init=cen)["labels"].shape == (P,)  # host rows still work
    sess.predict(img, classify=False, want=("patch_tokens",))
    assert _km(api, sess._h, **dict(res, source=2, n=P))[0] == 0
    sess.predict_list([img[0], img[1][:, :56]])
    for kw in (dict(res, source=2, n=P), dict(res, source=2, n=B * P, all_images=1), dict(res, source=1, n=B)):
        rc, untouched, msg = _km(api, sess._h, **kw)
        assert rc == 4 and untouched, ("after predict_list", kw, msg)
