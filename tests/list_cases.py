"""Shared inputs of the predict_list tests: the size lists, a numpy restatement of list_plan (csrc/kernels.h), a list form of
attention_cases.emulate (one segment at a time) and planted mutants.  Imported by tests/test_list_probes.py (CPU),
tests/test_gpu_attention_list.py and tests/test_gpu_predict_list.py.  Plain module, no fixtures.

The contract under test (include/dinov2_hip.h, dinov2_hip_predict_list): image i of a list has, bit for bit, the outputs of predict on that
image alone.  So every check here is "segment i of the list == the same computation on segment i alone".
"""
import numpy as np

import attention_cases as ac

PATCH = 14
QB = 128  # queries per workgroup of the list kernels (ATTN_LIST_QB)

# pixels (h, w) -> T with R = 4: 6, 10, 30, 77, 126, 137, 261 (one partial key tile and query block; a strip; crosses the 64-key tile; just
# under one 128-query block; two query blocks with a ragged second; five key tiles and three query blocks).  R = 0: 2, 6, 26, 73, 122, 133, 257.
S14, S14x70, S70, S112x126, S154, S154x168, S224 = (14, 14), (14, 70), (70, 70), (112, 126), (154, 154), (154, 168), (224, 224)
MIXED = [S224, S14, S154x168, S70, S112x126, S14x70, S154, S70]
LISTS = {
    "mixed": MIXED,
    "reversed": MIXED[::-1],
    "all_equal": [S70] * 4,
    "single": [S154x168],
    "repeat_apart": [S70, S14, S70, S112x126, S14],  # a repeated size that is not adjacent: two runs, one position embedding
}
# segment lengths of the attention-only tests: every tail / block edge next to another, and a long segment in front of short ones
SEGMENTS = {"edges": [1, 64, 65, 128, 129, 2, 261, 6, 193], "long_first": [1374, 6, 261]}


def tokens(size, R, patch=PATCH):
    return 1 + R + (size[0] // patch) * (size[1] // patch)


def plan(sizes, patch, R, nh, order=0):
    """list_plan restated: images [n, 5] (row0, T, P, h0, w0), runs [nruns, 2] (first, count), items [units, 4] (row0, T, head, query block)
    image-major (list order, or longest first with equal lengths in list order), then head, then query block; totals."""
    images, runs, row0 = [], [], 0
    for i, (h, w) in enumerate(sizes):
        h0, w0 = h // patch, w // patch
        P = h0 * w0
        T = 1 + R + P
        images.append((row0, T, P, h0, w0))
        if i == 0 or tuple(sizes[i]) != tuple(sizes[i - 1]):
            runs.append([i, 0])
        runs[-1][1] += 1
        row0 += T
    walk = list(range(len(sizes)))
    if order == 1:
        walk.sort(key=lambda i: -images[i][1])  # (stable)
    items = [(images[i][0], images[i][1], hd, qb) for i in walk for hd in range(nh) for qb in range((images[i][1] + QB - 1) // QB)]
    return {"images": np.array(images, np.int64).reshape(-1, 5), "runs": np.array(runs, np.int32).reshape(-1, 2),
            "items": np.array(items, np.int32).reshape(-1, 4), "M": row0, "P": sum(im[2] for im in images),
            "pixels": sum(h * w for h, w in sizes), "units": len(items)}


def random_sizes(rng, n, patch=PATCH, max_side=24):
    """n sizes with sides of 1 .. max_side patches, with repeats (adjacent and apart) likely."""
    pool = [(int(rng.integers(1, max_side + 1)) * patch, int(rng.integers(1, max_side + 1)) * patch) for _ in range(max(1, n // 2))]
    return [pool[int(rng.integers(len(pool)))] for _ in range(n)]


# ---------------------------------------------------------------------------------------------------------------- attention over segments
ATTN_MUTANTS = ("neighbour_keys_staged", "row0_off_by_one", "T_from_previous", "last_block_into_next_image", "heads_swapped")


def emulate_list(qkv, T, nh, dt, log2, mutant=None):
    """attention_cases.emulate over segments of T[i] rows of the packed qkv [sum T, 3H], one segment at a time.  Rows nobody writes stay NaN.
    `mutant` plants one bug of ATTN_MUTANTS in every segment it can show in."""
    qkv = np.asarray(qkv, np.float32)
    M, H = int(np.sum(T)), 64 * nh
    out = np.full((M, H), np.nan, np.float32)
    r0 = 0
    for i, t in enumerate(T):
        a, n = r0, t
        if mutant == "row0_off_by_one" and i > 0:
            a = r0 + 1
            n = min(t, M - a)
        if mutant == "T_from_previous" and i > 0:
            n = min(T[i - 1], M - a)
        if mutant == "neighbour_keys_staged":  # the last key tile runs on into the next image's rows, unmasked
            n = min((t + ac.KT - 1) // ac.KT * ac.KT, M - a)
        if n > 0:
            o = ac.emulate(qkv[a:a + n], 1, n, nh, dt, log2)
            if mutant == "heads_swapped" and nh > 1 and i == 1:
                o = o.reshape(n, nh, 64)[:, [1, 0] + list(range(2, nh))].reshape(n, H)
            rows = min(n, t) if mutant != "T_from_previous" else n
            if mutant == "last_block_into_next_image" and i + 1 < len(T):
                start = (t - 1) // QB * QB
                out[r0:r0 + start] = o[:start]
                out[r0 + t:r0 + t + (t - start)] = o[start:t][:M - r0 - t]
            else:
                out[r0:r0 + rows] = o[:rows]
        r0 += t
    return out


def check_segments(out, qkv, T, nh, dt, log2):
    """(ok, message): every segment of `out` equals, bit for bit, attention_cases.emulate on that segment alone."""
    out = np.asarray(out, np.float32)
    r0 = 0
    for i, t in enumerate(T):
        exp = ac.emulate(np.asarray(qkv, np.float32)[r0:r0 + t], 1, t, nh, dt, log2)
        got = out[r0:r0 + t]
        if not np.array_equal(got, exp):  # (NaN != NaN: an unwritten row fails too)
            bad = np.argwhere(~(got == exp))
            return False, "segment %d (rows %d .. %d): %d elements differ, first at row %d col %d" % (i, r0, r0 + t, len(bad), bad[0][0], bad[0][1])
        r0 += t
    return True, "every segment equals its own attention"


def segment_input(T, nh, dt, log2, seed):
    """Random packed qkv for segments T: every segment its own attention_cases 'random' regime draw."""
    return np.concatenate([ac.regime_input("random", 1, t, nh, dt, log2, seed + 7919 * i) for i, t in enumerate(T)])


# ---------------------------------------------------------------------------------------------------------------- the host path's bookkeeping
# What forward() is handed for the per-run launches of a list, restated from the plan: for image i the position embedding it is embedded with (by patch
# grid) and the pooling divisor of the head (quirk off: T_i - first).  The truth is what predict would use for that image alone.
HOST_MUTANTS = ("pos_embed_of_wrong_size", "pool_divisor_of_first_image")


def host_bookkeeping(sizes, patch, R, first, mutant=None):
    """[(h0, w0) of the position embedding, pooling divisor] per image, as the forward derives them run by run."""
    p = plan(sizes, patch, R, 1)
    out = []
    for first_img, count in p["runs"]:
        _, T, _, h0, w0 = p["images"][first_img]
        if mutant == "pos_embed_of_wrong_size":  # the run before's embedding
            _, _, _, h0, w0 = p["images"][max(first_img - 1, 0)]
        if mutant == "pool_divisor_of_first_image":
            T = p["images"][0][1]
        out += [((int(h0), int(w0)), int(T) - first)] * int(count)
    return out


def check_bookkeeping(book, sizes, patch, R, first):
    """(ok, message): image i is embedded with the position embedding of its own grid and pooled with its own divisor."""
    for i, (h, w) in enumerate(sizes):
        want = ((h // patch, w // patch), tokens((h, w), R, patch) - first)
        if book[i] != want:
            return False, "image %d: %r, alone it would be %r" % (i, book[i], want)
    return True, "every image as alone"


def image(size, seed, layout_chw=True):
    """A deterministic f32 test image of network size (h, w): smooth + noise, roughly normalised-image range."""
    h, w = size
    rng = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(yy / 9.0 + c) + np.cos(xx / 7.0 - c) for c in range(3)])
    img = (base + 0.5 * rng.standard_normal((3, h, w))).astype(np.float32)
    return img if layout_chw else np.ascontiguousarray(img.transpose(1, 2, 0))
