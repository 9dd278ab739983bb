"""Helpers for the intermediate-layer taps (dinov2_hip_predict_layers, layer_tap_kernel in csrc/kernels_misc.hip): a numpy restatement of
the gather -- from a token stream [B, T, H] the patch rows (as rows or as the CHW permutation), the CLS row and the register rows, for a
list of layers -- and the checks the GPU tests apply to what the library returns.  With `norm` the restatement works on an ALREADY
normalised stream (the GPU tests get it from dinov2_hip_op_layernorm(dtype = -1), the kernel the tap shares its row routine with): the
gather itself moves bits and rounds nothing, so every check here is bit-for-bit (misc_cases.check_exact).

Imported by tests/test_gpu_layers.py (the library) and tests/test_layer_probes.py (the restatement and its planted bugs, no GPU).  Plain
module, no fixtures.  `mutant`: the name of one planted bug (MUTANTS) or None.
"""
import numpy as np

from misc_cases import check_exact

TOKENS, CHW = 0, 1

MUTANTS = ("regs_not_skipped",      # patch rows start at token 1 instead of 1 + R
           "hw_swapped",            # CHW written as [H, w0, h0]
           "layer_off_by_one",      # upstream's block index taken for the number of blocks applied
           "norm1_weights",         # a layer's own norm1 instead of the model's final LayerNorm
           "pass_offset_dropped",   # every pass of a split batch writes at image 0
           "cls_stride_P")          # CLS row of image b read at flat row b * P instead of b * T


def gather(x, R, h0, w0, layout, mutant=None):
    """x [B, T, H], T = 1 + R + h0 * w0  ->  {"patch": [B, P, H] | [B, H, h0, w0], "cls": [B, H], "reg": [B, R, H]}."""
    x = np.asarray(x, np.float32)
    B, T, H = x.shape
    P = h0 * w0
    assert T == 1 + R + P
    first = 1 if mutant == "regs_not_skipped" else 1 + R
    patch = x[:, first:first + P]
    if layout == CHW:
        pt = np.ascontiguousarray(patch.transpose(0, 2, 1))  # [B, H, P]: element (c, p) = channel c of patch p = y * w0 + x
        if mutant == "hw_swapped":
            patch = np.ascontiguousarray(pt.reshape(B, H, w0, h0).transpose(0, 1, 3, 2))
        else:
            patch = pt.reshape(B, H, h0, w0)
    if mutant == "cls_stride_P":
        cls = x.reshape(B * T, H)[np.arange(B) * P]
    else:
        cls = x[:, 0]
    return {"patch": np.ascontiguousarray(patch), "cls": np.ascontiguousarray(cls), "reg": np.ascontiguousarray(x[:, 1:1 + R])}


def request(stream, layers, R, h0, w0, layout, mutant=None, wrong_stream=None, chunk=None):
    """What a predict_layers call returns for `layers` from stream [L + 1, B, T, H] (index = blocks applied; raw, or normalised when the
    request is): {"patch": [n, B, ...], "cls": [n, B, H], "reg": [n, B, R, H]}.  `chunk`: the batch is run in passes of that many images,
    last pass first, as dinov2_hip_predict splits it.  `wrong_stream`: what the "norm1_weights" mutant reads instead."""
    stream = np.asarray(stream, np.float32)
    B = stream.shape[1]
    out = None
    for k, layer in enumerate(layers):
        src = stream
        if mutant == "norm1_weights":
            src = wrong_stream
        if mutant == "layer_off_by_one":
            layer = max(layer - 1, 0)
        g = gather(src[layer], R, h0, w0, layout, mutant)
        if out is None:
            out = {key: np.full((len(layers),) + v.shape, np.nan, np.float32) for key, v in g.items()}
        step = chunk or B
        for b0 in reversed(range(0, B, step)):
            bn = min(step, B - b0)
            at = 0 if mutant == "pass_offset_dropped" else b0
            for key in g:
                out[key][k, at:at + bn] = g[key][b0:b0 + bn]
    return out


def check_taps(got, stream, layers, R, h0, w0, layout, what, keys=("patch", "cls", "reg")):
    """(ok, message): every destination in `keys` of `got` holds, bit for bit, what `request` says and no NaN is left."""
    exp = request(stream, layers, R, h0, w0, layout)
    for key in keys:
        if key == "reg" and R == 0:
            continue
        g = np.asarray(got[key], np.float32)
        if g.shape != exp[key].shape:
            return False, "%s %s: shape %r, expected %r" % (what, key, g.shape, exp[key].shape)
        if np.isnan(g).any():
            return False, "%s %s: %d elements left unwritten (NaN)" % (what, key, int(np.isnan(g).sum()))
        ok, msg = check_exact(g, exp[key], "%s %s" % (what, key))
        if not ok:
            return ok, msg
    return True, ""


def tap_stream(rows_fn, B, T, H, seed):
    """A [B, T, H] stream from one of misc_cases' row generators (ln_dyadic_rows, ln_offset_rows) or plain normal rows (None)."""
    if rows_fn is None:
        rng = np.random.default_rng(seed)
        return (rng.standard_normal((B, T, H)) * 2 + 0.3).astype(np.float32)
    return rows_fn(B * T, H, seed).reshape(B, T, H)
