"""CPU side of the off-family geometry sweep (tests/geometry_cases.py; the device side is tests/test_gpu_geometry.py).

  * the table is what it claims: every axis holds its smallest value, an interior off-family value and -- where the axis has a limit -- the last
    accepted and the first refused one; the limits are derived here from the kernels' conditions and compared with the source's constants;
  * dinov2_hip_model_load decides a refusal from the hparams alone, before it touches a device: the refused rows are refused HERE, with the
    message, and the rows next to a limit pass that validation;
  * every "runs" row is written, read back, and gives finite outputs in the oracle's ggml-default mode and in exact arithmetic;
  * the planner plans every GEMM of every "runs" row, in both dtypes, with and without the LN fold, and the parts of each plan tile the output
    exactly once (check_plan_parts of tests/test_gemm_plans.py); every (kernel, epilogue, dtype) the sweep reaches is launched by a bit-equality
    case of COVERAGE_CASES / LN_COVERAGE_CASES or of the two geometry lists, which hold nothing else;
  * the checker itself: the oracle's f32 mode against live, seeded HuggingFace models at three off-family geometries."""
import os
import re

import numpy as np
import pytest

import gemm_plan_cases as gp
import geometry_cases as gc
from oracle.oracle import OracleModel
from test_gemm_plans import LEAF, check_plan_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 0, 1
ERR_FORMAT, ERR_UNSUPPORTED = 2, 3


def _rows(axis, pos):
    """EVERY row of the table that stands at `pos` of `axis` (several may); never empty."""
    rows = [g for g in gc.GEOMETRIES for a, p in g["axes"] if (a, p) == (axis, pos)]
    assert rows, (axis, pos)
    return rows


def _grid(g):
    return g["size"][0] // g["cfg"]["patch"], g["size"][1] // g["cfg"]["patch"]


def _table(g):
    return g["cfg"]["img_size"] // g["cfg"]["patch"]


# ------------------------------------------------------------------------------------------------------------ the table
def test_the_table_holds_every_axis_and_its_boundary_pairs():
    assert 26 <= len(gc.GEOMETRIES) <= 30 and len({g["name"] for g in gc.GEOMETRIES}) == len(gc.GEOMETRIES)
    for g in gc.GEOMETRIES:
        large = g in gc.LARGE_M
        assert g["cfg"]["layers"] <= (1 if large else 2), g["name"]
        assert max(g["size"]) <= (224 if large else 112), g["name"]
        assert g["cfg"]["img_size"] % g["cfg"]["patch"] == 0 and all(s % g["cfg"]["patch"] == 0 for s in g["size"]), g["name"]
        assert (g["verdict"] == gc.REFUSED) == (g["refusal"] is not None), g["name"]
    run = {g["name"]: g for g in gc.RUNNING}
    # width and heads
    widths = {g["cfg"]["hidden"]: g["cfg"]["heads"] for g in gc.RUNNING}
    assert {64: 1, 192: 3, 320: 5, 448: 7, 640: 10, 1280: 20, 2048: 32}.items() <= widths.items()
    assert any(g["cfg"]["hidden"] == 1280 and g["cfg"]["ffn"] == 5120 for g in gc.RUNNING)  # ViT-H
    runs = lambda rows: all(g["verdict"] == gc.RUNS for g in rows)  # noqa: E731
    refused = lambda rows: all(g["verdict"] == gc.REFUSED for g in rows)  # noqa: E731
    family = {384, 768, 1024, 1536}
    assert all(g["cfg"]["hidden"] == 64 for g in _rows("width", "min")) and runs(_rows("width", "min"))
    assert all(64 < g["cfg"]["hidden"] < gc.LN_MAX_WIDTH and g["cfg"]["hidden"] not in family for g in _rows("width", "mid")) and runs(_rows("width", "mid"))
    assert {g["cfg"]["hidden"] for g in _rows("width", "mid")} == {192, 320, 448, 640, 1280}
    assert all(g["cfg"]["hidden"] == gc.LN_MAX_WIDTH for g in _rows("width", "last")) and runs(_rows("width", "last"))
    assert all(g["cfg"]["hidden"] == gc.LN_MAX_WIDTH + 64 for g in _rows("width", "first_refused")) and refused(_rows("width", "first_refused"))
    assert all(g["cfg"]["hidden"] != 64 * g["cfg"]["heads"] for g in _rows("heads", "first_refused")) and refused(_rows("heads", "first_refused"))
    # FFN
    assert all(g["cfg"]["ffn"] == 64 for g in _rows("ffn", "min")) and runs(_rows("ffn", "min"))
    assert all(g["cfg"]["ffn"] % 64 != 0 for g in _rows("ffn", "first_refused")) and refused(_rows("ffn", "first_refused"))
    assert all(g["cfg"]["ffn"] == g["cfg"]["hidden"] for g in _rows("ffn", "equals_hidden")) and runs(_rows("ffn", "equals_hidden"))
    for pos, swiglu in (("gelu_odd", False), ("swiglu_odd", True)):
        assert all(g["cfg"]["swiglu"] == swiglu and g["cfg"]["ffn"] % 64 == 0 and (g["cfg"]["ffn"] // 64) % 2 == 1 for g in _rows("ffn", pos)) and runs(_rows("ffn", pos))
    # patch: 1 (K_pe = 3 of 64), every size 2 .. 7, 8 (K_pe = 192) and 16 (768), the last accepted and the first refused
    assert all(g["cfg"]["patch"] == 1 for g in _rows("patch", "min"))
    assert {g["cfg"]["patch"] for g in _rows("patch", "small")} == {2, 3, 4, 5, 6, 7} and {g["cfg"]["patch"] for g in _rows("patch", "mid")} == {8, 16}
    assert [gc.kpe_pad(p) for p in range(1, 8)] == [64, 64, 64, 64, 128, 128, 192] and [3 * p * p for p in range(1, 8)] == [3, 12, 27, 48, 75, 108, 147]
    assert (gc.kpe_pad(8), gc.kpe_pad(16)) == (192, 768) and runs(_rows("patch", "min") + _rows("patch", "small") + _rows("patch", "mid"))
    assert all(g["cfg"]["img_size"] == 4 * g["cfg"]["patch"] and g["cfg"]["hidden"] in (128, 192) for g in _rows("patch", "min") + _rows("patch", "small"))
    assert all(g["cfg"]["patch"] == gc.MAX_PATCH for g in _rows("patch", "last")) and runs(_rows("patch", "last"))
    assert all(g["cfg"]["patch"] == gc.MAX_PATCH + 1 for g in _rows("patch", "first_refused")) and refused(_rows("patch", "first_refused"))
    # registers: 1, 3, 8, and 16 on a 1 x 1 and a 2 x 2 patch grid
    assert {1, 3, 8, 16} <= {g["registers"] for g in gc.RUNNING}
    assert all(g["registers"] == 1 for g in _rows("registers", "min")) and {g["registers"] for g in _rows("registers", "mid")} == {3, 8}
    assert all((g["registers"], _grid(g)) == (16, (1, 1)) for g in _rows("registers", "max_1x1"))
    assert all((g["registers"], _grid(g)) == (16, (2, 2)) for g in _rows("registers", "max_2x2"))
    # classes: 1, 3, 1001, none
    assert {0, 1, 3, 1001} <= {g["num_classes"] for g in gc.RUNNING}
    assert all(g["num_classes"] == 1 for g in _rows("classes", "min")) and {g["num_classes"] for g in _rows("classes", "mid")} == {3, 1001}
    assert all(g["num_classes"] == 0 for g in _rows("classes", "none"))
    # position table: the input grid, another one, a non-square one -- every row that claims a position holds it
    assert all(_grid(g) == (_table(g),) * 2 for g in _rows("pos", "identity"))
    assert all(_grid(g)[0] == _grid(g)[1] != _table(g) for g in _rows("pos", "different"))
    assert all(_grid(g)[0] != _grid(g)[1] and _grid(g)[0] * _grid(g)[1] != _table(g) ** 2 for g in _rows("pos", "nonsquare"))
    assert all(_grid(g)[0] != _grid(g)[1] and _grid(g)[0] * _grid(g)[1] == _table(g) ** 2 for g in _rows("pos", "identity_by_count"))
    assert runs([g for p in ("identity", "different", "nonsquare", "identity_by_count") for g in _rows("pos", p)])
    # types: bf16 on two of the odd widths, q4_0 at six blocks per row, q8_0 with two blocks per fc2 row
    bf = [g["cfg"]["hidden"] for g in gc.RUNNING if g["dtype"] == BF16]
    assert len(bf) >= 2 and all(h % 256 != 0 for h in bf)
    assert any(g["wtype"] == "q4_0" and g["cfg"]["hidden"] == 6 * 32 for g in gc.RUNNING)
    assert any(g["wtype"] == "q8_0" and g["cfg"]["ffn"] == 2 * 32 for g in gc.RUNNING)
    # large M: H = 320 and H = 1 280 at 224 pixels, one layer
    assert {g["cfg"]["hidden"] for g in gc.LARGE_M} == {320, 1280} and all(g["size"] == (224, 224) for g in gc.LARGE_M)
    assert all(g["dtype"] == BF16 for g in _rows("types", "bf16")) and len(_rows("types", "bf16")) >= 2
    for axis, (last, first) in gc.BOUNDARIES.items():
        assert runs(_rows(axis, last)) and refused(_rows(axis, first)), axis
    assert set(gc.SIDE_OUTPUTS) <= set(run) and [run[n]["cfg"]["hidden"] for n in gc.SIDE_OUTPUTS] == [64, 320, 2048]


def test_the_entry_point_rows_cover_what_they_claim():
    """ENTRY_ROWS and what goes with them (tests/test_gpu_geometry_entry_points.py): running rows with a classifier; widths 64 .. 2 048, heads
    1, 2, 3, 5 and 32, patches 1, 3, 7, 8, 14, 16 and 32, both compute types, registers 0 .. 4; four different list sizes per row, none above
    112 pixels; enough patches for k = 5 neighbours and pca3; window grids with more than one window each way and a cover far below the 48 the
    reduction takes."""
    import slide_cases as sl
    rows = [gc.BY_NAME[n] for n in gc.ENTRY_ROWS]
    assert all(g in gc.RUNNING and g["num_classes"] > 0 and g not in gc.LARGE_M for g in rows)
    assert {g["cfg"]["hidden"] for g in rows} == {64, 128, 192, 320, 2048} and {g["cfg"]["heads"] for g in rows} == {1, 2, 3, 5, 32}
    assert {g["cfg"]["patch"] for g in rows} == {1, 3, 7, 8, 14, 16, 32} and {g["dtype"] for g in rows} == {F16, BF16}
    assert {g["registers"] for g in rows} == {0, 1, 2, 3, 4}
    for g in rows:
        p, sizes = g["cfg"]["patch"], gc.list_sizes(g)
        assert len(set(sizes)) == 4 and all(h % p == 0 and w % p == 0 and p <= max(h, w) <= 112 for h, w in sizes), g["name"]
        assert _grid(g)[0] * _grid(g)[1] >= 5 and g["cfg"]["hidden"] >= 8, g["name"]
    assert set(gc.DENSE_ROWS) <= set(gc.ENTRY_ROWS) and {gc.BY_NAME[n]["cfg"]["patch"] for n in gc.DENSE_ROWS} == {1, 3, 8, 16}
    for n in gc.DENSE_ROWS:
        h, w, ch, cw, sh, sw = gc.slide_case(gc.BY_NAME[n])
        ys, xs = sl.starts(h, ch, sh), sl.starts(w, cw, sw)
        assert h > ch and w > cw and len(ys) >= 2 and len(xs) >= 3 and sl.cover_map(ys, xs, ch, cw, h, w).max() <= 8, n
        assert 2 * len(ys) * len(xs) <= 84  # windows of a batch of two
    assert [gc.BY_NAME[n]["cfg"]["patch"] for n in gc.RAW_U8_ROWS] == [16, 5] and 224 % 16 == 0 and 224 % 5 != 0
    g = gc.BY_NAME[gc.STRIDE_ROW]
    assert g["cfg"]["patch"] % gc.STRIDE == 0 and g["dtype"] == BF16 and g["cfg"]["swiglu"]


def test_the_list_plan_of_every_entry_point_row(api):
    """The library's list_plan (no device) on each row's list sizes, with the row's patch, registers and heads: the restatement of
    tests/list_cases.py, the token rows of the grids, one attention item per (image, head, query block) -- and, for every row whose patch is
    not 14, another plan than a patch of 14 would give (so a family constant in its place cannot pass the bit-equality of
    tests/test_gpu_geometry_entry_points.py: the forward would attend over other rows than predict alone does)."""
    import list_cases as lc
    for name in gc.ENTRY_ROWS:
        g = gc.BY_NAME[name]
        p, R, nh, sizes = g["cfg"]["patch"], g["registers"], g["cfg"]["heads"], gc.list_sizes(g)
        got, exp = api.list_plan(sizes, p, R, nh), lc.plan(sizes, p, R, nh)
        for k in ("images", "runs", "items"):
            assert np.array_equal(got[k], exp[k]), (name, k)
        assert [int(t) for t in got["images"][:, 1]] == [1 + R + (h // p) * (w // p) for h, w in sizes] and got["M"] == int(got["images"][:, 1].sum())
        assert {int(h) for h in got["items"][:, 2]} == set(range(nh)) and len(got["items"]) == got["units"]
        if p != 14:
            assert api.list_plan(sizes, 14, R, nh)["M"] != got["M"], name


def test_the_limits_follow_from_the_kernels_conditions():
    """Both patch limits from im2col's conditions, not from a comment: the LDS tile of ten patches (2-byte elements, Kpad = 3 p^2 up to a
    multiple of 64) within 64 KiB, and the two divisions by multiplication exact; the constants are those of csrc/kernels.h."""
    src = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert int(eval(re.search(r"constexpr int LN_MAX_WIDTH = ([0-9* ]+);", src).group(1))) == gc.LN_MAX_WIDTH == 2048
    assert int(re.search(r"constexpr int IM2COL_CHUNK = (\d+);", src).group(1)) == gc.IM2COL_CHUNK
    assert all(gc.im2col_patch_ok(p) for p in range(1, gc.MAX_PATCH + 1)) and not any(gc.im2col_patch_ok(p) for p in range(gc.MAX_PATCH + 1, 129))
    assert gc.MAX_PATCH == 32
    assert gc.IM2COL_CHUNK * gc.kpe_pad(32) * 2 == 61440 <= gc.IM2COL_LDS < gc.IM2COL_CHUNK * gc.kpe_pad(33) * 2 == 66560
    # the magic-number division is exact far beyond a chunk for every accepted patch: the LDS tile is the binding condition
    for p in range(1, gc.MAX_PATCH + 1):
        magic = 65536 // p + 1
        assert all((x * magic) >> 16 == x // p for x in range(2048))


# ------------------------------------------------------------------------------------------------------------ the loader's verdict
@pytest.fixture(scope="module")
def files(tmp_path_factory, pkg):
    return gc.file_cache(pkg, tmp_path_factory.mktemp("geometry"))


def _load_status(api, path):
    try:
        api.Model(path, classify=True)
    except api.DinoError as e:
        return e.status, str(e)
    return 0, ""


@pytest.mark.parametrize("g", gc.REFUSALS, ids=gc.geometry_id)
def test_refused_geometries_are_refused_at_load_by_name(api, files, g):
    """No device is needed: the loader refuses from the hparams, before it selects one."""
    status, msg = _load_status(api, files(g))
    hparam, value, limit = g["refusal"]
    assert status == ERR_UNSUPPORTED, (status, msg)
    assert hparam in msg and re.search(r"\b%d\b" % value, msg) and re.search(r"\b%d\b" % limit, msg), msg


@pytest.mark.parametrize("name", sorted({g["name"] for axis, (last, _) in gc.BOUNDARIES.items() for g in _rows(axis, last)}))
def test_the_last_accepted_geometries_pass_the_loaders_validation(api, files, name):
    """Whatever stops the load on a machine without a device, it is not the loader's verdict on the geometry or on the file."""
    status, msg = _load_status(api, files(gc.BY_NAME[name]))
    assert status not in (ERR_FORMAT, ERR_UNSUPPORTED), (status, msg)


# ------------------------------------------------------------------------------------------------------------ the oracle runs every row
@pytest.mark.parametrize("g", gc.RUNNING, ids=gc.geometry_id)
def test_running_geometries_are_written_read_back_and_finite_in_the_oracle(pkg, files, g):
    path = files(g)
    ora = OracleModel(path, quant_mode="dequant") if g["wtype"].startswith("q") else OracleModel(path)
    cfg = g["cfg"]
    assert (ora.hidden, ora.layers, ora.heads, ora.patch, ora.img_size, ora.registers) == \
        (cfg["hidden"], cfg["layers"], cfg["heads"], cfg["patch"], cfg["img_size"], g["registers"])
    assert (ora.ffn_hidden, bool(ora.swiglu), ora.num_classes, ora.has_head) == (cfg["ffn"], cfg["swiglu"], g["num_classes"], g["num_classes"] > 0)
    img = gc.images(pkg, g, batch=2)[1]
    classify = g["num_classes"] > 0
    out, ex = ora.forward(img, classify=classify), ora.forward_exact(img, classify=classify)
    P = gc.tokens(g) - 1 - g["registers"]
    assert out["patch_tokens"].shape == ex["patch_tokens"].shape == (P + (g["registers"] if classify else 0), cfg["hidden"])
    for k in out:
        assert np.isfinite(out[k]).all() and np.isfinite(ex[k]).all(), k
    assert 1e-3 < np.abs(out["patch_tokens"]).max() < 100
    if classify:
        assert out["logits"].shape == (g["num_classes"],) and np.abs(out["logits"]).max() < 30
        assert abs(float(out["probs"].sum()) - 1) < 1e-5


# ------------------------------------------------------------------------------------------------------------ the planner
def test_model_gemms_keeps_the_family_results():
    """The function as it was (names of MODELS, patch 14, a square side), restated."""
    for name, (H, F, swiglu) in gp.MODELS.items():
        for b, side, r in ((1, 224, 0), (8, 518, 4), (64, 518, 0)):
            P = (side // 14) ** 2
            M = b * (P + 1 + r)
            exp = [(gp.EPI_PATCH, b * P, H, 640), (gp.EPI_QKV, M, 3 * H, H), (gp.EPI_RESID, M, H, H), (gp.EPI_RESID, M, H, F),
                   (gp.EPI_SWIGLU, M, 2 * F, H) if swiglu else (gp.EPI_GELU, M, F, H)]
            assert gp.model_gemms(name, b, side, r) == exp
            cfg = dict(hidden=H, ffn=F, swiglu=swiglu, patch=14)
            assert gp.model_gemms(cfg, b, (side, side), r) == exp
            exp_ln = [(gp.EPI_QKV_LN, M, 3 * H, H), (gp.EPI_RESID_LN, M, H, H), (gp.EPI_RESID_LN, M, H, F),
                      (gp.EPI_SWIGLU_LN, M, 2 * F, H) if swiglu else (gp.EPI_GELU_LN, M, F, H)]
            assert gp.model_gemms_ln(name, b, side, r) == gp.model_gemms_ln(cfg, b, (side, side), r) == exp_ln
    # ... and off the family: patch 8 on 56 x 72 pixels, three registers, SwiGLU 832
    g = gc.BY_NAME["w320_swiglu832_p8_bf16"]
    assert gp.model_gemms(g["cfg"], 2, g["size"], 3) == [(0, 126, 320, 192), (1, 134, 960, 320), (2, 134, 320, 320), (2, 134, 320, 832), (4, 134, 1664, 320)]


def test_the_sweep_reaches_the_shapes_it_is_about():
    probs = gp.geometry_problems()
    ns, ks = {N for _, _, N, _ in probs}, {K for _, _, _, K in probs}
    assert {64, 192, 960, 3840, 6144} <= ns and {64, 5120, 3072} <= ks
    assert any(epi == gp.EPI_SWIGLU and (N // 128) % 2 == 1 for epi, _, N, _ in probs)


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln_fold"])
def test_every_gemm_of_the_sweep_is_planned_and_tiled_exactly_once(api, ln):
    probs = gp.geometry_problems(ln)
    assert len(probs) > (10 if ln else 60)
    for epi, M, N, K in probs:
        for dt in (F16, BF16):
            plan = api.gemm_plan(dt, epi, M, N, K)  # raises where launch_gemm would refuse
            # (the LN-fold epilogues' 192-row plan is gemm4.hip's two-height launch with an empty 256-row part)
            assert all(LEAF.match(leaf) or (ln and leaf == "gemm4_mixed<0+192>") for leaf in plan.split(";")), (dt, epi, M, N, K, plan)
            check_plan_parts(api, dt, epi, M, N, K)
    if ln:  # the rows that take the fold, and only those
        took = {g["cfg"]["hidden"] for g in gc.RUNNING if gp.ln_fold_applies(g["cfg"]["hidden"])}
        assert took == {128, 640, 1280} and not {64, 192, 320, 448, 2048} & took


@pytest.mark.parametrize("ln,base,cases", [(False, gp.COVERAGE_CASES, gp.GEOMETRY_COVERAGE_CASES), (True, gp.LN_COVERAGE_CASES, gp.GEOMETRY_LN_COVERAGE_CASES)],
                         ids=["plain", "ln_fold"])
def test_every_plan_the_sweep_reaches_is_covered_and_nothing_is_stale(api, ln, base, cases):
    """The sibling of test_every_reachable_plan_is_covered: every (kernel, epilogue, dtype) a geometry of the sweep launches is run by a
    bit-equality case -- of the family's list or of the geometry list --, every geometry case is there for a plan the family's list lacks, and
    no two of them for the same one."""
    need = set(gp.geometry_reachable(api, ln))
    fam = gp.cases_leaves(api, base)
    have = gp.cases_leaves(api, cases)
    assert not (need - fam - have), sorted(need - fam - have)[:10]
    assert cases and not set(cases) & set(base)
    for i, case in enumerate(cases):
        own = gp.cases_leaves(api, [case]) & need - fam
        others = gp.cases_leaves(api, cases[:i] + cases[i + 1:])
        assert own - others, f"{case}: stale (regenerate with `python tests/gemm_plan_cases.py`)"
    assert cases == gp.greedy_cases(api, gp.geometry_reachable(api, ln), fam)


def _first_batch(api, g, pred):
    for b in range(1, 257):
        plans = [api.gemm_plan(F16, *p) for p in gp.model_gemms(g["cfg"], b, g["size"], g["registers"])[1:]]  # the layer's four GEMMs
        if pred([not all(leaf.startswith("small<") for leaf in p.split(";")) for p in plans]):
            return b
    return None


def test_large_m_rows_are_the_first_batches_off_the_small_tile_kernel(api):
    rows = {(g["cfg"]["hidden"], pos): g for g in gc.LARGE_M for a, pos in g["axes"] if a == "large_m"}
    for H in (320, 1280):
        g = rows[H, "first_off_small"]
        assert _first_batch(api, g, any) == g["batch"], H
    g = rows[1280, "all_off_small"]
    assert _first_batch(api, g, all) == g["batch"]
    # H = 320: K / 64 is odd for three of the four, which therefore stay on the small-tile kernel at every batch
    assert _first_batch(api, rows[320, "first_off_small"], all) is None


# ------------------------------------------------------------------------------------------------------------ the checker, off-family
def _hf_model(kind, seed):
    import torch
    from transformers import Dinov2Config, Dinov2ForImageClassification, Dinov2WithRegistersConfig, Dinov2WithRegistersForImageClassification
    common = dict(hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, num_labels=7, layerscale_value=1.0, num_hidden_layers=2)
    torch.manual_seed(seed)
    if kind == "p16_h192_r1":
        model = Dinov2WithRegistersForImageClassification(Dinov2WithRegistersConfig(hidden_size=192, num_attention_heads=3, mlp_ratio=4, image_size=64,
                                                                                    patch_size=16, num_register_tokens=1, **common))
        size = (48, 80)
    elif kind == "p8_h320_r0":
        model = Dinov2ForImageClassification(Dinov2Config(hidden_size=320, num_attention_heads=5, mlp_ratio=4, image_size=64, patch_size=8, **common))
        size = (56, 72)
    else:  # SwiGLU: HF's hidden width (int(192 * 4 * 2 / 3) + 7) // 8 * 8 = 512 = 64 * 8
        model = Dinov2WithRegistersForImageClassification(Dinov2WithRegistersConfig(hidden_size=192, num_attention_heads=3, mlp_ratio=4, image_size=56,
                                                                                    patch_size=14, num_register_tokens=2, use_swiglu_ffn=True, **common))
        size = (70, 42)
    model.eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():  # as test_oracle_matches_hf_at_vit_s_scale: non-trivial values everywhere, weights f16-exact
        for pn, p in model.named_parameters():
            if pn.endswith("lambda1"):
                p.copy_(0.2 + 0.1 * torch.randn(p.shape, generator=g))
            elif "norm" in pn and pn.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.ndim >= 2 and "embeddings" not in pn or "projection.weight" in pn:
                p.copy_((0.04 * torch.randn(p.shape, generator=g)).half().float())
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return model, size


@pytest.mark.parametrize("kind", ["p16_h192_r1", "p8_h320_r0", "swiglu_h192_f512"])
def test_oracle_matches_hf_off_family(tmp_path, kind):
    """test_oracle_matches_hf_at_vit_s_scale at three geometries no published checkpoint has: patch 16 / three heads / one register, patch 8 /
    five heads / no registers, and SwiGLU at F = 512.  The oracle's f32 mode against HuggingFace's hidden states at that test's 5e-5 relative."""
    pytest.importorskip("transformers")
    import importlib.util
    import torch
    from importlib import import_module
    from __graft_entry__ import PKG_NAME
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)  # patches HF's pos-embed interpolation to the reference's (no antialias, identity on equal counts)
    model, (hh, ww) = _hf_model(kind, seed=11)
    cfg = model.config
    conv = import_module(PKG_NAME + ".convert")
    path = str(tmp_path / (kind + ".gguf"))
    conv.convert_state_dict({k: v.detach().numpy() for k, v in model.state_dict().items()}, cfg.to_dict(), path)
    img = torch.randn(3, hh, ww, generator=torch.Generator().manual_seed(3)).numpy()
    body = model.dinov2_with_registers if hasattr(model, "dinov2_with_registers") else model.dinov2
    with torch.no_grad():
        out = body(torch.from_numpy(img)[None], output_hidden_states=True)
        hidden = torch.stack([h[0] for h in out.hidden_states]).numpy()
        final = out.last_hidden_state[0].numpy()
    m = OracleModel(path, act_round=0, gelu_f16_lut=False)
    m.set(conv_round=0)
    R = int(getattr(cfg, "num_register_tokens", 0))
    assert (m.hidden, m.heads, m.patch, m.registers, bool(m.swiglu)) == (cfg.hidden_size, cfg.num_attention_heads, cfg.patch_size, R, bool(cfg.use_swiglu_ffn))
    assert m.ffn_hidden % 64 == 0
    o = m.forward(img, classify=True, hidden=True)
    T = 1 + R + (hh // cfg.patch_size) * (ww // cfg.patch_size)
    assert o["hidden"].shape == hidden.shape == (3, T, cfg.hidden_size)
    scale = max(1.0, float(np.abs(hidden).max()))
    err = float(np.abs(o["hidden"] - hidden).max())
    print(f"{kind}: max|oracle - HF| over the hidden states {err:.3e} (bound {5e-5 * scale:.3e})")
    assert err < 5e-5 * scale
    assert np.abs(o["cls"] - final[0]).max() < 1e-4 and np.abs(o["patch_tokens"] - final[1:]).max() < 1e-4
