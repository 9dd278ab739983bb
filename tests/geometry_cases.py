"""Model geometries OUTSIDE the four published checkpoints (ViT-S / B / L / g, patch 14), as data: what dinov2_hip_model_load accepts is far wider
than the family every other coverage argument of the suite is made for, and the kernels behind it have narrower domains.  The property the
sweep establishes: every geometry here either RUNS -- loads, and every forward holds the project's stated bound against the oracle -- or is
REFUSED by dinov2_hip_model_load with a message naming the hparam, its value and the limit.  Never "loads, then fails or is wrong".

Each row is a synth.write_synthetic_gguf config dict plus registers, classes, weight type, compute dtype, input size, batch and the verdict.
`axes` says which axis of the sweep a row stands on and where: "min" (smallest value), "mid" (interior, off-family), "last" (the last accepted
value of an axis that has a limit) or "first_refused" (the first value past it).  Every model has at most two layers and images of at most
112 pixels, except the large-M rows (one layer, 224 pixels: the smallest batch at which the GEMM planner leaves the small-tile kernel).

Imported by tests/test_geometry_probes.py (CPU: the table is what it claims, the oracle runs every row, the planner plans every GEMM of it)
and tests/test_gpu_geometry.py (the device); ENTRY_ROWS and what follows them by tests/test_gpu_geometry_entry_points.py (the entry points
the sweep itself does not call).  Plain module, no fixtures."""
F16, BF16 = 0, 1
RUNS, REFUSED = "runs", "refused"

# the limits, restated from the kernels' conditions (csrc/kernels.h: LN_MAX_WIDTH, im2col_patch_ok) -- tests/test_geometry_probes.py derives
# them again from these conditions and from the loader's verdicts
LN_MAX_WIDTH = 64 * 4 * 8          # one wave of 64 lanes keeps a row as at most 8 float4 per lane
IM2COL_CHUNK = 10                  # patches per LDS tile of im2col
IM2COL_LDS = 64 * 1024


def kpe_pad(patch):
    """K of the patch-embedding GEMM: 3 p^2 padded to a multiple of 64 (csrc/load.cpp)."""
    return (3 * patch * patch + 63) // 64 * 64


def im2col_patch_ok(patch):
    """csrc/kernels.h im2col_patch_ok with the loader's Kpad: the chunk's LDS tile fits, e / 3 by multiplication is exact over an interleaved
    run (below 32 768), and x / patch by multiplication (magic = 65536 / patch + 1) is exact for every pixel column of a chunk."""
    if patch <= 0 or IM2COL_CHUNK * kpe_pad(patch) * 2 > IM2COL_LDS or 3 * IM2COL_CHUNK * patch >= 32768:
        return False
    magic = 65536 // patch + 1
    return all((x * magic) >> 16 == x // patch for x in range(IM2COL_CHUNK * patch))


MAX_PATCH = max(p for p in range(1, 200) if all(im2col_patch_ok(q) for q in range(1, p + 1)))  # 32: Kpad 3 072 -> 60 KiB; 33: 3 328 -> 65 KiB


def _g(name, hidden, ffn, *, swiglu=False, patch=14, grid=4, layers=2, registers=0, classes=10, wtype="f16", dtype=F16, size=None, batch=2,
       verdict=RUNS, axes=(), refusal=None, heads=None, seed=0):
    heads = hidden // 64 if heads is None else heads
    cfg = dict(hidden=hidden, layers=layers, heads=heads, ffn=ffn, swiglu=swiglu, patch=patch, img_size=grid * patch)
    size = (grid * patch, grid * patch) if size is None else size
    return dict(name=name, cfg=cfg, registers=registers, num_classes=classes, wtype=wtype, dtype=dtype, size=size, batch=batch, verdict=verdict,
                axes=tuple(axes), refusal=refusal, seed=100 + seed)


# refusal = (hparam named in the message, its value, the limit named in the message)
GEOMETRIES = [
    # ---- width and heads (FFN, classes, position table and registers ride along) ----
    # H = 64: every GEMM narrower than any tile (N = 64, 192; K = 64); F = 64 = H, the smallest FFN; 3 classes; input grid = table (identity)
    _g("w64_f64", 64, 64, classes=3, axes=[("width", "min"), ("ffn", "min"), ("classes", "mid"), ("pos", "identity")], seed=1),
    # ViT-Ti/16: three heads, K_pe = 768, one register, a non-square input on a 4 x 4 table (3 x 5 = 15 patches: resampled)
    _g("w192_p16_r1", 192, 768, patch=16, registers=1, size=(48, 80), axes=[("width", "mid"), ("patch", "mid"), ("registers", "min"), ("pos", "nonsquare")], seed=2),
    # q4_0 at six blocks per row; the table is resampled 4 x 4 -> 5 x 5
    _g("w192_q4_0", 192, 768, registers=4, wtype="q4_0", size=(70, 70), classes=32, axes=[("types", "q4_0"), ("pos", "different")], seed=3),
    # H = 320: not a multiple of 128 (no LN fold) nor of the CHW tap's 256-channel chunk; N = 960 = 3 * 256 + 192; 1001 classes
    _g("w320_c1001", 320, 1280, grid=5, classes=1001, size=(84, 84), axes=[("width", "mid"), ("classes", "mid"), ("pos", "different")], seed=4),
    # SwiGLU with F = 64 * 13 (the loader interleaves x1 | x2 in 32-row blocks), patch 8 (K_pe = 192), three registers, bf16, 7 x 9 patches
    _g("w320_swiglu832_p8_bf16", 320, 832, swiglu=True, patch=8, grid=8, registers=3, classes=16, dtype=BF16, size=(56, 72),
       axes=[("ffn", "swiglu_odd"), ("patch", "mid"), ("registers", "mid"), ("types", "bf16"), ("pos", "nonsquare")], seed=5),
    # seven heads; GELU F = 64 * 17; eight registers; ONE class; 2 x 8 = 16 patches on a 4 x 4 table: the loader's identity path goes by the
    # patch COUNT (the reference compares counts, not shapes)
    _g("w448_f1088_r8_c1", 448, 1088, registers=8, classes=1, size=(28, 112), axes=[("width", "mid"), ("ffn", "gelu_odd"), ("registers", "mid"), ("classes", "min"), ("pos", "identity_by_count")], seed=6),
    # ten heads, F = H, a file with NO classifier, bf16
    _g("w640_f640_nohead_bf16", 640, 640, classes=0, dtype=BF16, size=(70, 42), axes=[("width", "mid"), ("ffn", "equals_hidden"), ("classes", "none"), ("types", "bf16")], seed=7),
    # ViT-H/14: 20 heads, N = 3 840, K = 5 120
    _g("w1280_vit_h", 1280, 5120, registers=4, classes=1000, axes=[("width", "mid")], seed=8),
    # the widest LayerNorm instance (8 float4 per lane), N = 6 144, with the largest patch im2col takes (K_pe = 3 072); 3 x 2 patches on a 2 x 2 table
    _g("w2048_p32", 2048, 2048, patch=MAX_PATCH, grid=2, layers=1, registers=4, size=(3 * MAX_PATCH, 2 * MAX_PATCH), axes=[("width", "last"), ("patch", "last"), ("pos", "nonsquare")], seed=9),
    # the first width past it: 33 heads
    _g("w2112_refused", LN_MAX_WIDTH + 64, 64, layers=1, verdict=REFUSED, refusal=("hidden_size", LN_MAX_WIDTH + 64, LN_MAX_WIDTH), axes=[("width", "first_refused")], seed=10),
    # head dim 32: the family and the kernels use 64
    _g("w128_h4_refused", 128, 512, heads=4, verdict=REFUSED, refusal=("head dim", 32, 64), axes=[("heads", "first_refused")], seed=11),
    # ---- patch: the largest accepted on a narrow model as well, and the first refused ----
    _g("w128_p32", 128, 512, patch=MAX_PATCH, grid=2, size=(2 * MAX_PATCH, 3 * MAX_PATCH), axes=[("patch", "last")], seed=12),
    _g("w128_p33_refused", 128, 512, patch=MAX_PATCH + 1, grid=2, verdict=REFUSED, refusal=("patch_size", MAX_PATCH + 1, MAX_PATCH), axes=[("patch", "first_refused")], seed=13),
    # ---- patch sizes 1 .. 7 (K_pe = 3 p^2 = 3 .. 147, padded to 64, 64, 64, 64, 128, 128, 192), each on a 4 x 4 position table ----
    # patch 1: 3 of 64 K columns are real; a grid row of 23 patches takes three im2col chunks (10, 10, 3); 3 x 23 = 69 patches (resampled)
    _g("w128_p1", 128, 512, patch=1, registers=2, classes=7, size=(3, 23), axes=[("patch", "min"), ("pos", "nonsquare")], seed=17),
    # patch 2, bf16: w0 = 11, a second chunk holding one patch
    _g("w128_p2_bf16", 128, 512, patch=2, dtype=BF16, size=(8, 22), axes=[("patch", "small"), ("types", "bf16"), ("pos", "nonsquare")], seed=18),
    # patch 3 = the channel count (the two divisors of the interleaved im2col coincide); three heads; 3 x 5 patches
    _g("w192_p3_r1", 192, 768, patch=3, registers=1, size=(9, 15), axes=[("patch", "small"), ("pos", "nonsquare")], seed=19),
    # patch 4: the position table's identity path
    _g("w128_p4", 128, 512, patch=4, size=(16, 16), axes=[("patch", "small"), ("pos", "identity")], seed=20),
    # patch 5: K_pe = 75 of 128; 4 x 3 patches
    _g("w128_p5", 128, 512, patch=5, size=(20, 15), axes=[("patch", "small"), ("pos", "nonsquare")], seed=21),
    # patch 6: w0 = 10, one full chunk exactly
    _g("w128_p6", 128, 512, patch=6, size=(18, 60), axes=[("patch", "small"), ("pos", "nonsquare")], seed=22),
    # patch 7: K_pe = 147 of 192; four registers; 3 x 5 patches
    _g("w128_p7_r4", 128, 512, patch=7, registers=4, size=(21, 35), axes=[("patch", "small"), ("pos", "nonsquare")], seed=23),
    # ---- FFN: q8_0 with two blocks per fc2 row; a width that is no multiple of 64 ----
    _g("w128_f64_q8_0", 128, 64, registers=1, wtype="q8_0", classes=32, axes=[("ffn", "min"), ("types", "q8_0")], seed=14),
    _g("w128_f96_refused", 128, 96, verdict=REFUSED, refusal=("FFN hidden size", 96, 64), axes=[("ffn", "first_refused")], seed=15),
    # ---- registers outnumber patches: 16 registers on a 1 x 1 and a 2 x 2 patch grid (T = 18, 21) ----
    _g("w128_r16_grid1", 128, 512, registers=16, classes=3, size=(14, 14), axes=[("registers", "max_1x1")], seed=16),
    _g("w128_r16_grid2", 128, 512, registers=16, classes=3, size=(28, 28), axes=[("registers", "max_2x2")], seed=16),
    # ---- large M, one layer, 224 x 224 on a 16 x 16 table: the smallest batch at which api.gemm_plan leaves the small-tile kernel for one of the
    # layer's GEMMs (tests/test_geometry_probes.py::test_large_m_rows_are_the_first_batches_off_the_small_tile_kernel) ----
    # H = 320: K / 64 = 5 is odd, so only FFN-out (K = 1 280, N = 320 = 256 + 64) can leave it: the 256 leading columns on gemm2<192>
    _g("w320_large_m_b143", 320, 1280, grid=16, layers=1, batch=143, axes=[("large_m", "first_off_small")], seed=4),
    # H = 1 280: QKV and FFN-in go to gemm4_short<64> at batch 2; at batch 11 all four GEMMs of the layer have left it
    _g("w1280_large_m_b2", 1280, 5120, grid=16, layers=1, batch=2, axes=[("large_m", "first_off_small")], seed=8),
    _g("w1280_large_m_b11", 1280, 5120, grid=16, layers=1, batch=11, axes=[("large_m", "all_off_small")], seed=8),
]

BY_NAME = {g["name"]: g for g in GEOMETRIES}
RUNNING = [g for g in GEOMETRIES if g["verdict"] == RUNS]
REFUSALS = [g for g in GEOMETRIES if g["verdict"] == REFUSED]
LARGE_M = [g for g in RUNNING if any(a == "large_m" for a, _ in g["axes"])]
SIDE_OUTPUTS = ("w64_f64", "w320_c1001", "w2048_p32")  # predict_layers / predict_attention / predict_dense at H = 64, 320, 2 048
# predict_layers / predict_attention also at patch 1 (its 3 x 23 output is too small for predict_dense's float64-margin cap: the exact parts of
# predict_dense run on it in tests/test_gpu_geometry_entry_points.py)
SIDE_OUTPUTS_TAPS = SIDE_OUTPUTS + ("w128_p1",)

# ---- the entry points the sweep above does not call (tests/test_gpu_geometry_entry_points.py): widths 64, 128, 192, 320 and 2 048; heads 1, 2,
# 3, 5 and 32; patches 1, 3, 7, 8, 14, 16 and 32; f16 and bf16; registers 0 .. 4 ----
ENTRY_ROWS = ("w64_f64", "w192_p16_r1", "w320_swiglu832_p8_bf16", "w2048_p32", "w128_p1", "w192_p3_r1", "w128_p7_r4")
DENSE_ROWS = ("w192_p16_r1", "w320_swiglu832_p8_bf16", "w192_p3_r1", "w128_p1")  # predict_dense / predict_dense_slide, exact parts
RAW_U8_ROWS = ("w192_p16_r1", "w128_p5")  # 224 (the classify preprocessing's crop) is a multiple of patch 16 and none of patch 5
STRIDE_ROW, STRIDE = "w320_swiglu832_p8_bf16", 2


def list_sizes(g):
    """The images a row's predict_list gets: its own size, one single patch, its size transposed (a square one: two patches wider), and a
    column of up to seven patches.  The last is there for the rows whose other grids a patch of 14 would also give (patch 16: 48 x 80 is
    3 x 5 patches either way): seven patches, or as many as 112 pixels hold, are another number of 14s at every patch size but 14."""
    p, (h, w) = g["cfg"]["patch"], g["size"]
    return [(h, w), (p, p), (w, h) if h != w else (h, w + 2 * p), (min(7, 112 // p) * p, p)]


def slide_case(g):
    """(h, w, crop h, crop w, stride h, stride w) of a row's sliding windows: the row's size, a crop of 2 x 3 patches, one patch down per
    window and -- where the patch is above 1 -- a horizontal stride that is no multiple of the patch."""
    p, (h, w) = g["cfg"]["patch"], g["size"]
    return (h, w, 2 * p, 3 * p, p, p + 1 if p > 1 else 1)


# axes that have a limit: (axis, position) of the last accepted and of the first refused value
BOUNDARIES = {"width": ("last", "first_refused"), "patch": ("last", "first_refused"), "ffn": ("min", "first_refused")}


def geometry_id(g):
    return g["name"]


def write(pkg, g, path):
    """The row's checkpoint (seeded; the same file on every machine)."""
    return pkg.synth.write_synthetic_gguf(path, g["cfg"], registers=g["registers"], num_classes=g["num_classes"], seed=g["seed"], wtype=g["wtype"])


def file_cache(pkg, root):
    """get(row) -> path of the row's checkpoint under `root`, written on first use; rows that share a model (the large-M rows, the two
    16-register rows) share the file.  Both test files build their module-scoped `files` fixture on it."""
    made = {}

    def get(g):
        key = (tuple(sorted(g["cfg"].items())), g["registers"], g["num_classes"], g["wtype"], g["seed"])
        if key not in made:
            made[key] = str(root / (g["name"] + ".gguf"))
            write(pkg, g, made[key])
        return made[key]

    return get


def tokens(g):
    p = g["cfg"]["patch"]
    return 1 + g["registers"] + (g["size"][0] // p) * (g["size"][1] // p)


def images(pkg, g, batch=None):
    return pkg.synth.synthetic_images(g["batch"] if batch is None else batch, g["size"][0], g["size"][1], seed=g["seed"])
