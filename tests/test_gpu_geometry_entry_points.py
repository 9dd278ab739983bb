"""The entry points the off-family geometry sweep (tests/test_gpu_geometry.py) does not call, at geometries off the four published ones
(tests/geometry_cases.py: ENTRY_ROWS and what goes with them): predict_list and list_rows, the consumers of the resident rows (match, bank,
kmeans, pca3), predict_dense and predict_dense_slide, patch_stride, raw 8-bit input and a one-device group.  What these hold is the host
bookkeeping -- list_plan, the resident-row offsets 1 + R, P and last_b * P, the window grid, the preprocessing size -- which must go through
grid_of / grid_dim and never through a family constant, and the attention work table of predict_list with 1, 2, 3, 5 and 32 heads.

Contracts, as the tests they are taken from state them:
  predict_list (include/dinov2_hip.h; tests/test_gpu_predict_list.py): image i has the bits of predict on it alone; list_rows gives the
      grids' products (+ R with CLASSIFY).  One image of a size no other test of the row runs is also held to the first contract of
      tests/test_gpu_geometry.py against the oracle: logits 1e-3, tokens and cls 5e-3 relative, 8 x in bf16 compute;
  resident rows (tests/test_gpu_match.py, test_gpu_bank.py, test_gpu_kmeans.py: the bodies are theirs): the bits of the same call on the
      fetched tokens, and each consumer's own acceptance rule against float64 of those tokens;
  predict_dense / predict_dense_slide (tests/test_gpu_dense.py::_check_dense, tests/test_gpu_slide.py::_check_slide): their exact parts.
      The float64-margin parts end in a cap on the share of pixels inside the margin that was stated for outputs of 56 pixels and more; the
      outputs here are as small as 3 x 23, so those parts stay with the golden fixtures and the sweep's three wide rows;
  patch_stride (tests/stride_cases.py): the strided model on I == the default model on the expanded image E, bit for bit."""
import numpy as np
import pytest

import geometry_cases as gc
import list_cases as lc
import misc_cases as mc
import pca_cases as pc
import stride_cases as sc
from oracle.oracle import OracleModel
from test_gpu_bank import check_resident_bank
from test_gpu_dense import _check_dense
from test_gpu_kmeans import check_resident_kmeans
from test_gpu_match import check_resident_match
from test_gpu_slide import _check_slide

pytestmark = pytest.mark.gpu

BF16 = 1
ERR_INVALID = 4


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _exact(got, exp, what):
    ok, msg = mc.check_exact(got, exp, what)
    assert ok, msg


@pytest.fixture(scope="module")
def files(tmp_path_factory, pkg):
    return gc.file_cache(pkg, tmp_path_factory.mktemp("geometry_entry"))


@pytest.fixture(scope="module")
def loaded(api, files):
    """get(row name, classify=True, **load options) -> (row, model), loaded once per module."""
    made = {}

    def get(name, classify=True, **kw):
        key = (name, classify, tuple(sorted(kw.items())))
        if key not in made:
            g = gc.BY_NAME[name]
            made[key] = api.Model(files(g), dtype=g["dtype"], classify=classify, **kw)
        return gc.BY_NAME[name], made[key]

    return get


def _grid(g, size):
    return size[0] // g["cfg"]["patch"], size[1] // g["cfg"]["patch"]


# ---------------------------------------------------------------------------------------------------------------- (a) predict_list
@pytest.mark.parametrize("name", gc.ENTRY_ROWS)
def test_predict_list_equals_predict_alone_and_list_rows_the_grids(api, pkg, files, loaded, name):
    g, model = loaded(name)
    R, nh, p = g["registers"], g["cfg"]["heads"], g["cfg"]["patch"]
    sizes = gc.list_sizes(g)
    assert len({tuple(s) for s in sizes}) == 4 and sizes[0] == g["size"] and sizes[1] == (p, p)
    imgs = [pkg.synth.synthetic_images(1, h, w, seed=g["seed"] + 10 * i)[0] for i, (h, w) in enumerate(sizes)]
    assert [model.grid(h, w) for h, w in sizes] == [_grid(g, s) for s in sizes]
    plan = lc.plan(sizes, p, R, nh)
    lst, one = api.Session(model), api.Session(model)
    ora = OracleModel(files(g))
    scale = 8.0 if g["dtype"] == BF16 else 1.0
    for classify in (False, True):
        rows = [h0 * w0 + (R if classify else 0) for h0, w0 in (_grid(g, s) for s in sizes)]
        off = api.list_rows(model, sizes, classify=classify)
        assert list(np.diff(off)) == rows and off[0] == 0
        assert np.array_equal(np.diff(off), plan["images"][:, 1] - (1 if classify else 1 + R))  # tests/test_gpu_predict_list.py's statement
        got = lst.predict_list(imgs, classify=classify)
        assert np.array_equal(got["offsets"], off) and got["patch_packed"].shape == (off[-1], g["cfg"]["hidden"])
        for i, img in enumerate(imgs):
            exp = one.predict(img[None], classify=classify)
            what = "%s %s image %d (%d x %d)" % (name, "classify" if classify else "features", i, *sizes[i])
            for k in ("cls", "logits", "probs") if classify else ("cls",):
                _exact(got[k][i], exp[k][0], what + " " + k)
            assert got["patch_tokens"][i].shape == exp["patch_tokens"][0].shape == (rows[i], g["cfg"]["hidden"]), what
            _exact(got["patch_tokens"][i], exp["patch_tokens"][0], what + " patch rows")
            _exact(got["patch_packed"][off[i]:off[i + 1]], exp["patch_tokens"][0], what + " packed rows")
        # the transposed (or widened) size: its position table is resampled by no other test of the row
        ref = ora.forward(imgs[2], classify=classify)
        d = {k: _rel(got[k][2], ref[k]) for k in (("logits",) if classify else ()) + ("cls", "patch_tokens")}
        print(name, "classify" if classify else "features", "list image 2 against the oracle:", d)
        assert d["cls"] <= 5e-3 * scale and d["patch_tokens"] <= 5e-3 * scale, d
        if classify:
            assert d["logits"] <= 1e-3 * scale, d


# ---------------------------------------------------------------------------------------------------------------- (b) resident rows
@pytest.mark.parametrize("classify", [False, True], ids=["features", "classify"])
@pytest.mark.parametrize("name", gc.ENTRY_ROWS)
def test_resident_rows_of_match_bank_kmeans_and_pca3(api, pkg, loaded, name, classify):
    """After a predict of two images, every consumer of the resident rows gives the bits of the same call on the fetched host tokens -- so
    the offsets 1 + R, P and image * T into the token stream are the row's, whatever its patch size, registers and grid -- and is inside
    its own acceptance rule against float64 of those tokens."""
    g, model = loaded(name)
    R, H = g["registers"], g["cfg"]["hidden"]
    imgs = gc.images(pkg, g, batch=2)
    P = int(np.prod(_grid(g, g["size"])))
    assert P >= 5 and H >= 8  # k = 5 neighbours; pca3 needs P >= 4 and H >= 8
    check_resident_match(api, model, imgs, classify)
    check_resident_bank(api, model, imgs, classify)
    sess = api.Session(model)
    init, init_all = np.array([0, P // 2, P - 1], np.int32), np.array([1, P, 2 * P - 1], np.int32)  # K = 3; the second image's rows too
    tok, _, _ = check_resident_kmeans(api, sess, imgs, classify, 3, init, 3, init_all)
    assert tok.shape == (2, P, H)
    # pca3 on image 0 of the last predict (with CLASSIFY its resident rows start with the registers, as the rows predict hands out do)
    rows = sess.predict(imgs, classify=classify, want=("patch_tokens",))["patch_tokens"][0]
    assert rows.shape == (P + (R if classify else 0), H)
    resident = sess.pca3(None, shape=rows.shape)
    for a, b, what in zip(resident, sess.pca3(rows), ("components", "mean", "projection")):
        _exact(a, b, "%s: pca3 of the resident rows against the fetched rows, %s" % (name, what))
    fails, figures = pc.e2e_failures(rows, *resident, what=name + " pca3")
    print(figures)
    assert not fails, fails
    with pytest.raises(api.DinoError):
        sess.pca3(None, shape=(rows.shape[0] + 1, H))


# ---------------------------------------------------------------------------------------------------------------- (c) dense heads
@pytest.mark.parametrize("name", gc.DENSE_ROWS)
def test_predict_dense_exact_parts(api, pkg, loaded, name):
    """A 3-class linear head on the last layer's normalised patch tokens: logits within the bound of float64 of the f16 operands, labels
    and values equal to the restatement applied to the device's own logits, argmax and bins."""
    g, model = loaded(name, classify=False)
    _check_dense(api, api.Session(model), model, gc.images(pkg, g, batch=2), [g["cfg"]["layers"]], 3, norm=1, concat_cls=0, out_size=None,
                 what=name, margin=False)


@pytest.mark.parametrize("name", gc.DENSE_ROWS)
def test_predict_dense_slide_exact_parts(api, loaded, name):
    """Windows of 2 x 3 patches, one patch down and -- above patch 1 -- a patch and a pixel across: the window starts are the formula's,
    the window logits the bits of predict_dense on the crops, labels and values the restatement of those logits."""
    g, model = loaded(name, classify=False)
    case = gc.slide_case(g)
    p = g["cfg"]["patch"]
    assert model.grid(case[2], case[3]) == (2, 3) and case[4] == p and (p == 1 or case[5] % p != 0)
    _check_slide(api, model, 3, (g["cfg"]["layers"],), 0, name, case=case, margin=False)


# ---------------------------------------------------------------------------------------------------------------- (d) patch_stride
def test_patch_stride_2_on_patch_8_bf16_swiglu(api, loaded):
    """predict in both modes, predict_list of two sizes and match on the resident tokens of a stride-2 model equal the default model on the
    expanded image(s), bit for bit."""
    g, md = loaded(gc.STRIDE_ROW)
    _, ms = loaded(gc.STRIDE_ROW, patch_stride=gc.STRIDE)
    p, s, R, H = g["cfg"]["patch"], gc.STRIDE, g["registers"], g["cfg"]["hidden"]
    assert (p, s, ms.patch_stride, md.patch_stride) == (8, 2, 2, 8)
    h, w = 16, 22
    rgb = np.random.default_rng(31).standard_normal((2, 3, h, w)).astype(np.float32)
    E = sc.expand(rgb, p, s)
    h0, w0 = sc.grid(h, w, p, s)
    P = h0 * w0
    assert ms.grid(h, w) == (h0, w0) == (5, 8) == md.grid(*E.shape[2:])
    ss, sd = api.Session(ms), api.Session(md)
    for classify in (False, True):
        a, b = ss.predict(rgb, classify=classify), sd.predict(E, classify=classify)
        assert sorted(a) == sorted(b) and a["patch_tokens"].shape == (2, P + (R if classify else 0), H)
        for k in a:
            _exact(a[k], b[k], "stride 2 predict %s %s" % ("classify" if classify else "features", k))
    # match on what a features predict left on the device
    ss.predict(rgb, classify=False)
    sd.predict(E, classify=False)
    ma, mb = ss.match(shape=(P, H)), sd.match(shape=(P, H))
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k
    sizes = [(h, w), (12, 10)]
    imgs = [rgb[0], np.random.default_rng(32).standard_normal((3, 12, 10)).astype(np.float32)]
    Es = [sc.expand(i, p, s) for i in imgs]
    for classify in (False, True):
        off = api.list_rows(ms, sizes, classify=classify)
        assert list(np.diff(off)) == [int(np.prod(sc.grid(hh, ww, p, s))) + (R if classify else 0) for hh, ww in sizes]
        assert np.array_equal(off, api.list_rows(md, [e.shape[1:] for e in Es], classify=classify))
        a, b = ss.predict_list(imgs, classify=classify), sd.predict_list(Es, classify=classify)
        for k in a:
            if k == "patch_tokens":
                assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
            else:
                assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------- (e) raw 8-bit input
@pytest.mark.parametrize("name", gc.RAW_U8_ROWS)
def test_raw_u8_input_equals_its_host_preprocessing(api, loaded, name):
    """A raw image of odd size: predict of it == predict of its host preprocessing, bit for bit, in both modes.  The features
    preprocessing ends on the patch grid whatever the patch size ((dim / p + 1) * p); the classify preprocessing crops to 224 x 224 whatever
    the patch size, so where 224 is not on the model's grid (patch 5) BOTH calls are refused, by name, before anything runs."""
    g, model = loaded(name)
    p, R = g["cfg"]["patch"], g["registers"]
    sess = api.Session(model)
    raw = np.random.default_rng(5).integers(0, 256, (1, 45, 61, 3), dtype=np.uint8)
    assert api.preprocess_size(0, 45, 61, p) == ((45 // p + 1) * p, (61 // p + 1) * p) and api.preprocess_size(1, 45, 61, p) == (224, 224)
    for classify, pre in ((False, api.dino_preprocess), (True, api.dino_classify_preprocess)):
        f32 = pre(raw[0], p)
        assert f32.shape[:2] == api.preprocess_size(1 if classify else 0, 45, 61, p)
        if any(d % p for d in f32.shape[:2]):
            assert classify and 224 % p != 0
            sess.profile(True)
            for call in (lambda: sess.predict(raw, classify=True, layout=api.U8_BGR_HWC), lambda: sess.predict(f32[None], classify=True, layout=api.BGR_HWC),
                         lambda: sess.predict_list([raw[0]], classify=True, layout=api.U8_BGR_HWC),
                         lambda: api.list_rows(model, [(45, 61)], classify=True, layout=api.U8_BGR_HWC)):
                with pytest.raises(api.DinoError) as e:
                    call()
                assert e.value.status == ERR_INVALID and "patch_size %d" % p in str(e.value) and "224" in str(e.value), str(e.value)
            assert all(v[1] == 0 for v in sess.profile_read().values()), "a refused call launched something"
            sess.profile(False)
            continue
        a = sess.predict(raw, classify=classify, layout=api.U8_BGR_HWC)
        b = sess.predict(f32[None], classify=classify, layout=api.BGR_HWC)
        h0, w0 = model.grid(*f32.shape[:2])
        assert (h0, w0) == (f32.shape[0] // p, f32.shape[1] // p) and a["patch_tokens"].shape[1] == h0 * w0 + (R if classify else 0)
        for k in a:
            _exact(a[k], b[k], "%s raw u8 %s %s" % (name, "classify" if classify else "features", k))


# ---------------------------------------------------------------------------------------------------------------- (f) group
def test_one_device_group_gives_the_sessions_bits(api, pkg, files, loaded):
    g, model = loaded("w192_p16_r1")
    imgs = gc.images(pkg, g, batch=2)
    grp = api.Group(files(g), devices=[0], dtype=g["dtype"], classify=True)
    try:
        assert (grp.hparams.patch_size, grp.patch_stride, grp.hparams.num_register_tokens) == (16, 16, 1)
        sess = api.Session(model)
        for classify in (True, False):
            ga, sa = grp.predict(imgs, classify=classify), sess.predict(imgs, classify=classify)
            assert ga["patch_tokens"].shape == (2, 15 + (1 if classify else 0), 192) and sorted(ga) == sorted(sa)
            for k in sa:
                _exact(ga[k], sa[k], "group %s %s" % ("classify" if classify else "features", k))
    finally:
        grp.close()
