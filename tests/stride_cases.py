"""Cases and closed forms of the patch_stride tests (tests/test_stride_probes.py on the CPU, tests/test_gpu_stride.py on the device).

The key is an identity.  For patch size p and stride s (s | p) the EXPANDED image of I,

    E[i p + a, j p + b] = I[i s + a, j s + b]        i < h0 = (h - p) / s + 1,  j < w0 = (w - p) / s + 1,  a, b < p,

lays every patch of I's grid out next to the others.  A model loaded with the default stride sees on E exactly the col matrix the strided
model sees on I, the same grid (hence the same position embedding), the same M and the same kernel plans: every output is bit-equal.
"""
import numpy as np

# restated from csrc/kernels.h (tests/test_stride_probes.py holds the closed forms below to brute force)
IM2COL_CHUNK = 10
LDS_BUDGET = 64 * 1024


def grid(h, w, p, s):
    return (h - p) // s + 1, (w - p) // s + 1


def kpad(p):
    return (3 * p * p + 63) // 64 * 64


def run(p, s):
    """patches of one grid row a workgroup of the strided im2col owns (im2col_stride_run): a strip of IM2COL_CHUNK patch widths"""
    return (IM2COL_CHUNK - 1) * p // s + 1


def pitch(p, s):
    """elements from one strip row to the next in LDS (im2col_stride_pitch): the strip's width up to an odd number of dwords"""
    width = (run(p, s) - 1) * s + p
    return (((width + 1) // 2) | 1) * 2


def stride_ok(p, s, Kpad):
    """csrc/kernels.h im2col_stride_ok: s | p; the strip of 3 p rows fits 64 KiB; e / 3 by multiplication (exact below 32 768) covers an
    interleaved strip row; k / p by (k * magic) >> 20 is exact for every piece start k < Kpad and stays inside 32 bits."""
    if p <= 0 or s <= 0 or s > p or p % s:
        return False
    if 3 * IM2COL_CHUNK * p >= 32768:
        return False
    if Kpad % 8 or Kpad < 3 * p * p or Kpad > 1 << 20:
        return False
    if 3 * p * pitch(p, s) * 2 > LDS_BUDGET:
        return False
    mg = (1 << 20) // p + 1
    return all(k * mg < 1 << 32 and (k * mg) >> 20 == k // p for k in range(0, Kpad, 8))


def expand(img, p, s, axes=(-2, -1)):
    """E of the module docstring; `axes`: the (row, column) axes of img ([.., h, w] by default; (0, 1) or (1, 2) for interleaved images)."""
    img = np.asarray(img)
    ay, ax = (a % img.ndim for a in axes)
    h0, w0 = grid(img.shape[ay], img.shape[ax], p, s)
    ri = (np.arange(h0)[:, None] * s + np.arange(p)[None, :]).reshape(-1)
    ci = (np.arange(w0)[:, None] * s + np.arange(p)[None, :]).reshape(-1)
    return np.ascontiguousarray(np.take(np.take(img, ri, axis=ay), ci, axis=ax))


def col_reference(rgb, p, s, Kpad):
    """The col matrix [B h0 w0, Kpad] of planar RGB images [B, 3, h, w], unrounded: a plain gather, k = c p^2 + ky p + kx, zero padding."""
    B, _, h, w = rgb.shape
    h0, w0 = grid(h, w, p, s)
    yy = np.arange(h0)[:, None] * s + np.arange(p)[None, :]  # [h0, p]
    xx = np.arange(w0)[:, None] * s + np.arange(p)[None, :]  # [w0, p]
    g = rgb[:, :, yy[:, None, :, None], xx[None, :, None, :]]  # [B, 3, h0, w0, p, p]
    col = np.zeros((B, h0, w0, Kpad), np.float32)
    col[..., :3 * p * p] = g.transpose(0, 2, 3, 1, 4, 5).reshape(B, h0, w0, 3 * p * p)
    return col.reshape(B * h0 * w0, Kpad)


def footprint(b, c, y, x, h, w, p, s):
    """The (row, k) elements of col that pixel (y, x) of RGB channel c of image b lands in: one per patch that covers it, at most (p / s)^2,
    each at its own (c, ky, kx).  Closed form: patch row i covers y iff i s <= y < i s + p."""
    h0, w0 = grid(h, w, p, s)
    out = []
    for i in range(max(0, (y - p) // s + 1), min(h0 - 1, y // s) + 1):
        for j in range(max(0, (x - p) // s + 1), min(w0 - 1, x // s) + 1):
            out.append((b * h0 * w0 + i * w0 + j, c * p * p + (y - i * s) * p + (x - j * s)))
    return out


# (stride, h, w) on patch 14, the smallest sizes at which the strided path can go wrong: a 1 x 1 grid; 3 x 5; w0 = 10 | 11 and 19 | 20 (either
# side of a workgroup's run of 19 patches at stride 7) and 21; stride 2 with w0 = 15 and with 64 | 65 (its run is 64); stride 1 with w0 = 17,
# 15 x 15 and 128 (its run is 127)
SIZES_14 = [(7, 14, 14), (7, 28, 42), (7, 70, 77), (7, 70, 84), (7, 28, 140), (7, 28, 147), (7, 70, 154),
            (2, 28, 42), (2, 14, 140), (2, 14, 142), (1, 14, 30), (1, 28, 28), (1, 14, 141)]
# the forward runs the smaller ones (grids of at most a few hundred tokens)
FORWARD_14 = [(7, 14, 14), (7, 28, 42), (7, 70, 77), (7, 70, 84), (7, 28, 140), (7, 28, 147), (7, 70, 154), (2, 28, 42), (2, 14, 142),
              (1, 14, 30), (1, 28, 28), (1, 14, 141)]
# synthetic checkpoints (write_synthetic_gguf with a dict config): (patch, stride, img_size of the checkpoint, h, w)
SYNTH = [(16, 4, 64, 32, 48), (16, 8, 64, 48, 64), (8, 1, 32, 16, 20),
         # patch sizes 2 .. 7 on a 4 x 4 table: grids 4 x 7, 4 x 5, 3 x 5, 3 x 4, 2 x 4, 4 x 6
         (2, 1, 8, 5, 8), (3, 1, 12, 6, 7), (4, 2, 16, 8, 12), (6, 2, 24, 10, 12), (6, 3, 24, 9, 15), (7, 1, 28, 10, 12)]
# (patch, stride) below patch 8 for the strided kernel alone: a 16-byte output piece (8 elements) spans four strip rows at patch 2, crosses a
# channel boundary inside one piece at patch 3 (k = 8 | 9), and 3 p^2 = 12 .. 147 real columns sit in Kpad = 64, 64, 64, 128, 128, 192
SMALL_PS = [(2, 1), (3, 1), (4, 1), (4, 2), (5, 1), (6, 1), (6, 2), (6, 3), (7, 1)]


def small_kernel_cases():
    """(p, s, h, w) for SMALL_PS, three grid rows each: a grid row that is exactly one workgroup's run, and one of a run plus two patches."""
    out = []
    for p, s in SMALL_PS:
        h = 2 * s + p
        for w0 in (run(p, s), run(p, s) + 2):
            out.append((p, s, h, (w0 - 1) * s + p))
    return out


SMALL_KERNEL = small_kernel_cases()


def synth_config(patch, img_size):
    return dict(hidden=128, layers=2, heads=2, ffn=512, swiglu=False, patch=patch, img_size=img_size)


# the single-image limit of a pass: rows * widest activation row * 2 bytes < 2^31.  A one-layer `small` checkpoint (hidden 384: qkv and the
# FFN hidden layer are 1 536 columns wide, the im2col matrix 640) at stride 1: 699 050 rows
SMALL_WIDEST = 1536
LIMIT_ROWS = (1 << 31) // (SMALL_WIDEST * 2)  # 699 050: more rows than this are refused (2^31 / 3 072 is not whole)
OVER = 851   # 838^2 + 5 = 702 249 rows
UNDER = 849  # 836^2 + 5 = 698 901 rows
