"""ctypes binding of libdinov2_hip.so (include/dinov2_hip.h) + a mirror of the reference's host API.

The product path has NO fallback: if the HIP library is missing or fails to load, importing a model raises
(`HipLibraryMissing`) -- nothing here ever computes on the CPU.

Mirror of /root/reference/dinov2.h (same names, argument meaning and error behaviour where sane):
  dino_params            dinov2.h:57-68     (seed, topk, enable_flash_attn, n_threads, classify, model, ...)
  dino_hparams           dinov2.h:25-47
  dino_model_load(...)   dinov2.h:98-99     -> returns (ok: bool, model)   [reference: bool + out-param]
  dino_predict(...)      dinov2.h:111-112   -> dino_output | None          [reference: unique_ptr, {} on failure]
  dino_output            dinov2.h:85-88     preds / patch_tokens
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DINOV2_HIP_LIB") or os.path.join(_HERE, "libdinov2_hip.so")  # env override: tuning variants only

F16, BF16 = 0, 1
BGR_HWC, RGB_CHW = 0, 1
CLASSIFY = 1

STATUS = {0: "OK", 1: "ERR_IO", 2: "ERR_FORMAT", 3: "ERR_UNSUPPORTED", 4: "ERR_INVALID", 5: "ERR_HIP", 6: "ERR_NO_HEAD"}


class HipLibraryMissing(RuntimeError):
    pass


class DinoError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{STATUS.get(status, status)}: {msg}")
        self.status = status


class LoadOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("compute_dtype", C.c_int32), ("classify", C.c_int32),
                ("skip_tensor_data", C.c_int32), ("quirk_pool_const_divisor", C.c_int32),
                ("quirk_pool_includes_registers", C.c_int32), ("batch_invariant", C.c_int32), ("ln_fold", C.c_int32), ("patch_stride", C.c_int32),
                ("reserved", C.c_int32 * 7)]


class HParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_classes",
                                          "num_register_tokens", "patch_size", "img_size", "ftype")] + \
               [("eps", C.c_float)] + \
               [(n, C.c_uint32) for n in ("ffn_hidden", "swiglu", "has_classifier", "weight_type", "compute_dtype")]
    patch_stride = 0  # not a field of the C struct: the stride the model was loaded with (Model and Group set it); 0 = patch_size


class Input(C.Structure):
    _fields_ = [("data", C.c_void_p), ("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("layout", C.c_int32), ("on_device", C.c_int32)]


class Output(C.Structure):
    _fields_ = [("cls", C.c_void_p), ("patch_tokens", C.c_void_p), ("logits", C.c_void_p), ("probs", C.c_void_p),
                ("topk_ids", C.c_void_p), ("topk_probs", C.c_void_p), ("topk", C.c_int32), ("on_device", C.c_int32)]


class ImageList(C.Structure):
    """dinov2_hip_image_list (include/dinov2_hip.h)."""
    _fields_ = [("data", C.POINTER(C.c_void_p)), ("height", C.POINTER(C.c_int32)), ("width", C.POINTER(C.c_int32)), ("n", C.c_int32),
                ("layout", C.c_int32), ("on_device", C.c_int32)]


class Layers(C.Structure):
    """dinov2_hip_layers (include/dinov2_hip.h)."""
    _fields_ = [("layers", C.POINTER(C.c_int32)), ("n_layers", C.c_int32), ("norm", C.c_int32), ("layout", C.c_int32),
                ("patch_tokens", C.c_void_p), ("cls", C.c_void_p), ("registers", C.c_void_p), ("on_device", C.c_int32),
                ("reserved", C.c_int32 * 4)]


LAYERS_TOKENS, LAYERS_CHW = 0, 1


class Attention(C.Structure):
    """dinov2_hip_attention (include/dinov2_hip.h)."""
    _fields_ = [("layers", C.POINTER(C.c_int32)), ("n_layers", C.c_int32), ("queries", C.POINTER(C.c_int32)), ("n_queries", C.c_int32),
                ("keys", C.c_int32), ("probs", C.c_void_p), ("on_device", C.c_int32), ("reserved", C.c_int32 * 4)]


class Match(C.Structure):
    """dinov2_hip_match (include/dinov2_hip.h)."""
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("na", C.c_int32), ("nb", C.c_int32), ("H", C.c_int32), ("image_a", C.c_int32),
                ("image_b", C.c_int32), ("on_device", C.c_int32), ("idx_ab", C.c_void_p), ("sim_ab", C.c_void_p), ("idx_ba", C.c_void_p),
                ("sim_ba", C.c_void_p), ("reserved", C.c_int32 * 4)]


class Rows(C.Structure):
    """dinov2_hip_rows (include/dinov2_hip.h)."""
    _fields_ = [("source", C.c_int32), ("data", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32), ("image", C.c_int32), ("on_device", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class TopK(C.Structure):
    """dinov2_hip_topk (include/dinov2_hip.h)."""
    _fields_ = [("queries", Rows), ("k", C.c_int32), ("idx", C.c_void_p), ("sim", C.c_void_p), ("reserved", C.c_int32 * 4)]


class PropagateReq(C.Structure):
    """dinov2_hip_propagate_req (include/dinov2_hip.h)."""
    _fields_ = [("queries", Rows), ("slots", C.c_uint64), ("radius", C.c_int32), ("k", C.c_int32), ("temperature", C.c_float),
                ("keep", C.c_int32), ("labels", C.c_void_p), ("argmax", C.c_void_p), ("idx", C.c_void_p), ("sim", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class KMeans(C.Structure):
    """dinov2_hip_kmeans (include/dinov2_hip.h)."""
    _fields_ = [("rows", Rows), ("all_images", C.c_int32), ("K", C.c_int32), ("max_iter", C.c_int32), ("init", C.c_int32),
                ("init_centers", C.c_void_p), ("init_rows", C.c_void_p), ("labels", C.c_void_p), ("sim", C.c_void_p), ("centers", C.c_void_p),
                ("counts", C.c_void_p), ("iterations", C.c_void_p), ("converged", C.c_void_p), ("reserved", C.c_int32 * 4)]


KMEANS_INIT_GIVEN, KMEANS_INIT_ROWS = 0, 1


class Coreset(C.Structure):
    """dinov2_hip_coreset (include/dinov2_hip.h)."""
    _fields_ = [("rows", Rows), ("all_images", C.c_int32), ("bank", C.c_void_p), ("m", C.c_int32), ("first", C.c_int32),
                ("stop_sim", C.c_float), ("idx", C.c_void_p), ("cover", C.c_void_p), ("selected", C.c_void_p), ("nearest", C.c_void_p),
                ("near_sim", C.c_void_p), ("reserved", C.c_int32 * 4)]


class Vlad(C.Structure):
    """dinov2_hip_vlad (include/dinov2_hip.h)."""
    _fields_ = [("rows", Rows), ("all_images", C.c_int32), ("offsets", C.c_void_p), ("n_seg", C.c_int32), ("K", C.c_int32),
                ("centers", C.c_void_p), ("flags", C.c_uint32), ("vlad", C.c_void_p), ("counts", C.c_void_p), ("labels", C.c_void_p),
                ("sim", C.c_void_p), ("reserved", C.c_int32 * 4)]


VLAD_INTRA_NORM, VLAD_L2_NORM = 1, 2


class NCut(C.Structure):
    """dinov2_hip_ncut (include/dinov2_hip.h)."""
    _fields_ = [("rows", Rows), ("all_images", C.c_int32), ("affinity", C.c_int32), ("tau", C.c_float), ("floor", C.c_float),
                ("n_eig", C.c_int32), ("max_iter", C.c_int32), ("tol", C.c_float), ("values", C.c_void_p), ("vectors", C.c_void_p),
                ("degree", C.c_void_p), ("residual", C.c_void_p), ("iterations", C.c_void_p), ("converged", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


NCUT_THRESHOLD, NCUT_RELU, NCUT_EXP = 0, 1, 2
NCUT_NB = 8  # the block width (csrc/kernels.h NCUT_NB)
_NCUT_AFFINITY = {"threshold": NCUT_THRESHOLD, "relu": NCUT_RELU, "exp": NCUT_EXP}


def _ncut_affinity(affinity):
    if affinity in _NCUT_AFFINITY:
        return _NCUT_AFFINITY[affinity]
    if isinstance(affinity, (int, np.integer)):
        return int(affinity)  # (an unknown id reaches the library, which refuses it)
    raise ValueError(f"ncut: affinity must be one of {sorted(_NCUT_AFFINITY)}")


class DenseDesc(C.Structure):
    """dinov2_hip_dense_desc (include/dinov2_hip.h)."""
    _fields_ = [("layers", C.POINTER(C.c_int32)), ("n_layers", C.c_int32), ("norm", C.c_int32), ("concat_cls", C.c_int32),
                ("num_classes", C.c_int32), ("weight", C.c_void_p), ("bias", C.c_void_p), ("reduce", C.c_int32), ("bin_centers", C.c_void_p),
                ("bins_eps", C.c_float), ("reserved", C.c_int32 * 6)]


class DenseOut(C.Structure):
    """dinov2_hip_dense_out (include/dinov2_hip.h)."""
    _fields_ = [("out_h", C.c_int32), ("out_w", C.c_int32), ("labels", C.c_void_p), ("value", C.c_void_p), ("logits", C.c_void_p),
                ("on_device", C.c_int32), ("reserved", C.c_int32 * 4)]


class Slide(C.Structure):
    """dinov2_hip_slide (include/dinov2_hip.h)."""
    _fields_ = [("crop_h", C.c_int32), ("crop_w", C.c_int32), ("stride_h", C.c_int32), ("stride_w", C.c_int32), ("reserved", C.c_int32 * 4)]


SLIDE_COVER_MAX = 16


def _pair(v):
    """(a, b) of a crop or stride given as one number or as (h, w)."""
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else (int(v[0]), int(v[1]))


DENSE_ARGMAX, DENSE_BINS = 0, 1
_DENSE_REDUCE = {"argmax": DENSE_ARGMAX, "bins": DENSE_BINS}

ROWS_GIVEN, ROWS_LAST_CLS, ROWS_LAST_PATCHES = 0, 1, 2
_ROWS_SOURCE = {"given": ROWS_GIVEN, "last_cls": ROWS_LAST_CLS, "last_patches": ROWS_LAST_PATCHES}

ATTN_KEYS_ALL, ATTN_KEYS_PATCHES = 0, 1
_ATTN_KEYS = {"all": ATTN_KEYS_ALL, "patches": ATTN_KEYS_PATCHES}


class GroupOpts(C.Structure):
    _fields_ = [("load", LoadOpts), ("n_devices", C.c_int32), ("devices", C.POINTER(C.c_int32)), ("broadcast", C.c_int32),
                ("streams_per_device", C.c_int32), ("reserved", C.c_int32 * 7)]


_lib = None

# dinov2_hip_op_attention_ex: a guard row around the device output changed (include/dinov2_hip_ops.h)
OP_GUARD_CHANGED = -2


def set_tuning(key, value):
    """Testing aid (include/dinov2_hip_ops.h): flip one of the library's tuning switches inside this process; 0 = its own choice."""
    rc = lib().dinov2_hip_op_set_tuning(key.encode(), int(value))
    if rc != 0:
        raise ValueError(f"unknown tuning key {key!r}")


def reset_tuning(key):
    """Back to the value the environment gave the switch when the library first read it (0 if none)."""
    set_tuning(key, -1)


def build_id() -> str:
    """The commit libdinov2_hip.so was built from (dinov2_hip_build_id)."""
    return lib().dinov2_hip_build_id().decode()


def gemm_plan(dtype, epilogue, M, N, K, lda=0, ldw=0):
    """The kernel plan launch_gemm picks for a shape (text; no device needed).  lda, ldw: row strides of A and W in elements, 0 = K."""
    buf = C.create_string_buffer(256)
    if lda or ldw:
        rc = lib().dinov2_hip_op_gemm_plan_strided(int(dtype), int(epilogue), int(M), int(N), int(K), int(lda), int(ldw), buf, 256)
    else:
        rc = lib().dinov2_hip_op_gemm_plan(int(dtype), int(epilogue), int(M), int(N), int(K), buf, 256)
    if rc != 0:
        raise ValueError(f"launch_gemm refuses dtype={dtype} epilogue={epilogue} M={M} N={N} K={K} lda={lda} ldw={ldw}")
    return buf.value.decode()


PLAN_PART_FIELDS = ("step", "part", "row0", "rows", "col0", "cols", "M", "N", "K", "ldo", "qcols", "nt_out", "clk_slot", "ln_gs",
                    "whole_nt_out", "whole_clk_slot", "whole_ln_gs",
                    "off_A", "off_W", "off_bias", "off_aux", "off_out", "off_xg", "off_stats", "off_ln_gamma", "off_ln_s", "off_ln_c")


def gemm_plan_parts(dtype, epilogue, M, N, K):
    """The same plan as data (dinov2_hip_op_gemm_plan_parts): one dict per argument block a kernel of the plan is launched with."""
    nf = len(PLAN_PART_FIELDS)
    buf = (C.c_int64 * (8 * nf))()
    n = lib().dinov2_hip_op_gemm_plan_parts(int(dtype), int(epilogue), int(M), int(N), int(K), buf, 8)
    if n < 0:
        raise ValueError(f"launch_gemm refuses dtype={dtype} epilogue={epilogue} M={M} N={N} K={K}")
    return [dict(zip(PLAN_PART_FIELDS, buf[i * nf:(i + 1) * nf])) for i in range(n)]


def _op_rc(rc, name):
    if rc == OP_GUARD_CHANGED:
        raise AssertionError(f"{name} wrote outside its output (guard band changed)")
    if rc != 0:
        raise RuntimeError(f"dinov2_hip_op_{name} failed ({rc})")


def _ptr(a):
    """A numpy array as the typed pointer an op's argtypes ask for (its own dtype's; also taken where they say void *); None stays NULL."""
    return None if a is None else a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


OP_NO_MEMORY = -3  # DINOV2_HIP_OP_NO_MEMORY: a far op's allocation was refused


class DeviceMemoryRefused(RuntimeError):
    """A far-operand op could not allocate its buffers (it reports that apart from a HIP error)."""


def device_memory():
    """(free, total) bytes of the current device (hipMemGetInfo)."""
    free, total = C.c_int64(0), C.c_int64(0)
    _op_rc(lib().dinov2_hip_op_device_memory(C.byref(free), C.byref(total)), "device_memory")
    return free.value, total.value


def _far_rc(rc, name):
    if rc == OP_NO_MEMORY:
        raise DeviceMemoryRefused(f"dinov2_hip_op_{name}: a device allocation was refused")
    if rc == 4:
        raise ValueError(f"dinov2_hip_op_{name} refuses these arguments")
    _op_rc(rc, name)


def op_gemm_far(dtype, epilogue, M, N, K, W, bias, aux, rows, *, lda=0, ldw=0, ldo=0, seed_a=1, seed_out=2, qcols=0, qscale=1.0):
    """launch_gemm once on a device-made A [M, K] at row stride lda (dinov2_hip_op_gemm_far): W [N, K], bias [N], aux [N] host f32.  Returns
    (the output rows `rows` as f32 [len(rows), width], the number of payload elements the launch left untouched).  Raises ValueError for a
    shape the launcher refuses, DeviceMemoryRefused, AssertionError for a changed guard band."""
    W = _f32(W)
    assert W.shape == (N, K), W.shape
    width = N // 2 if epilogue == 4 else N
    r = np.ascontiguousarray(rows, np.int64)
    out = np.full((len(r), width), np.nan, np.float32)
    untouched = C.c_int64(-1)
    _far_rc(lib().dinov2_hip_op_gemm_far(int(dtype), int(epilogue), int(M), int(N), int(K), int(lda or K), int(ldw or K), int(ldo or width),
                                         int(seed_a), int(seed_out), _ptr(W), _ptr(_f32(bias)), _ptr(_f32(aux)), int(qcols), float(qscale),
                                         _ptr(r), len(r), _ptr(out), C.byref(untouched)), "gemm_far")
    return out, untouched.value


def op_attention_far(dtype, B, T, nh, rows, *, seed=1, log2_scores=True):
    """launch_attention once on a device-made qkv [B*T, 3*64*nh] (dinov2_hip_op_attention_far).  Returns (rows `rows` of the output as f32
    [len(rows), 64*nh], the untouched count); raises as op_gemm_far."""
    r = np.ascontiguousarray(rows, np.int64)
    out = np.full((len(r), 64 * nh), np.nan, np.float32)
    untouched = C.c_int64(-1)
    _far_rc(lib().dinov2_hip_op_attention_far(int(dtype), int(B), int(T), int(nh), int(seed), int(log2_scores), _ptr(r), len(r), _ptr(out),
                                              C.byref(untouched)), "attention_far")
    return out, untouched.value


def op_rows_fill(dst, row0, n, dictionary, d_common, seed, plants=(), *, ld=None):
    """Rows [row0, row0 + n) of a far operand into the first n rows of the DeviceArray dst [>= n, H] (dinov2_hip_op_rows_fill): row r is
    dictionary[entry(r)], entry = a hash of r onto [0, d_common) unless r is planted.  dictionary: host [D, H]; plants: (row, entry) pairs.
    ld: the row stride in floats (default: dst's row length).  A testing aid: nothing of the product path calls it."""
    dic = _f32(dictionary)
    D, H = dic.shape
    ld = int(dst.shape[1] if ld is None else ld)
    if len(dst.shape) != 2 or n < 1 or ld < H or (int(n) - 1) * ld + H > dst.shape[0] * dst.shape[1]:
        raise ValueError(f"rows_fill: {n} rows of {H} floats at stride {ld} do not fit a buffer of shape {dst.shape}")
    pl = sorted((int(r), int(e)) for r, e in plants)
    pr, pe = np.array([r for r, _ in pl], np.int64), np.array([e for _, e in pl], np.int32)
    rc = lib().dinov2_hip_op_rows_fill(C.c_void_p(dst.ptr), ld, int(row0), int(n), H, _ptr(dic), D, int(d_common), int(seed),
                                       _ptr(pr) if len(pl) else None, _ptr(pe) if len(pl) else None, len(pl))
    if rc == 4:
        raise ValueError("dinov2_hip_op_rows_fill refuses these arguments")
    _op_rc(rc, "rows_fill")


def op_layer_tap(x, w, b, eps, R, h0, w0, *, norm, chw, want=("patch", "cls", "reg")):
    """layer_tap_kernel alone (dinov2_hip_op_layer_tap): x [B, T, H] f32 -> dict of the destinations in `want`.  Raises on a HIP error or a
    changed guard band."""
    x = _f32(x)
    B, T, H = x.shape
    P = h0 * w0
    out = {}
    if "patch" in want:
        out["patch"] = np.zeros((B, H, h0, w0) if chw else (B, P, H), np.float32)
    if "cls" in want:
        out["cls"] = np.zeros((B, H), np.float32)
    if "reg" in want:
        out["reg"] = np.zeros((B, R, H), np.float32)
    _op_rc(lib().dinov2_hip_op_layer_tap(_ptr(x), _ptr(_f32(w)), _ptr(_f32(b)), float(eps), B, T, R, H, h0, w0, int(norm), int(chw),
                                         _ptr(out.get("patch")), _ptr(out.get("cls")), _ptr(out.get("reg"))), "layer_tap")
    return out


LIST_ORDER_AS_GIVEN, LIST_ORDER_LONGEST_FIRST = 0, 1
LIST_POS_GRIDS = 64  # DINOV2_HIP_LIST_POS_GRIDS


def list_plan(sizes, patch, R, nh, order=LIST_ORDER_AS_GIVEN):
    """The plan of a Session.predict_list (dinov2_hip_op_list_plan; no device): `sizes` = [(h, w)] NETWORK sizes in pixels.  Returns a dict:
    images [n, 5] int64 (row0, T, P, h0, w0), runs [nruns, 2] (first, count), items [units, 4] int32 (row0, T, head, query block) in the
    order of the attention launch's workgroups, and the totals M, P, pixels, units."""
    hw = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
    n = len(hw)
    h, w = np.ascontiguousarray(hw[:, 0]), np.ascontiguousarray(hw[:, 1])
    tot = np.zeros(5, np.int64)
    images, runs = np.zeros((n, 5), np.int64), np.zeros((n, 2), np.int32)
    args = (n, _ptr(h), _ptr(w), int(patch), int(R), int(nh), int(order))
    if lib().dinov2_hip_op_list_plan(*args, _ptr(images), _ptr(runs), None, 0, _ptr(tot)) != 0:
        raise ValueError(f"list_plan refuses sizes={hw.tolist()} patch={patch} R={R} nh={nh} order={order}")
    items = np.zeros((int(tot[3]), 4), np.int32)
    if lib().dinov2_hip_op_list_plan(*args, None, None, _ptr(items), len(items), _ptr(tot)) != 0:
        raise ValueError("list_plan: the table does not fit")
    return {"images": images, "runs": runs[:int(tot[4])], "items": items, "M": int(tot[0]), "P": int(tot[1]), "pixels": int(tot[2]),
            "units": int(tot[3])}


def op_attention_list(dtype, qkv, T, nh, log2_scores=True):
    """launch_attention_list alone (dinov2_hip_op_attention_list): qkv [sum T, 3*64*nh] f32, segments of T[i] tokens one after the other ->
    [sum T, 64*nh] f32 values of the compute type.  Raises on a HIP error or a changed guard band."""
    H = 64 * nh
    T = np.ascontiguousarray(T, np.int32)
    qkv = _f32(qkv)
    assert qkv.shape == (int(T.sum()), 3 * H), qkv.shape
    out = np.zeros((int(T.sum()), H), np.float32)
    _op_rc(lib().dinov2_hip_op_attention_list(int(dtype), _ptr(qkv), _ptr(out), len(T), _ptr(T), H, nh, int(log2_scores)), "attention_list")
    return out


def op_attn_rows(dtype, qkv, B, T, nh, queries, key0=0, nkeys=None, lds_budget=0):
    """attn_rows_kernel alone (dinov2_hip_op_attn_rows[_ex]): qkv [B*T, 3*64*nh] f32 (q pre-scaled by log2(e)/8) -> [B, nh, nq, nkeys] f32, columns
    [key0, key0 + nkeys) of the softmax rows of the tokens `queries` over all T keys.  lds_budget > 0: the LDS the scores may take, in bytes
    (below 4 T: the two-pass form).  Raises on a HIP error or a changed guard band."""
    H = 64 * nh
    qkv = _f32(qkv)
    assert qkv.shape == (B * T, 3 * H), qkv.shape
    q = np.ascontiguousarray(queries, np.int32)
    nkeys = T - key0 if nkeys is None else int(nkeys)
    out = np.zeros((B, nh, len(q), nkeys), np.float32)
    _op_rc(lib().dinov2_hip_op_attn_rows_ex(int(dtype), _ptr(qkv), B, T, H, nh, _ptr(q), len(q), int(key0), nkeys, _ptr(out), int(lds_budget)),
           "attn_rows")
    return out


def op_match(a, b):
    """The kernels of csrc/match.hip alone (dinov2_hip_op_match): a [na, H], b [nb, H] f32 -> dict of idx_ab, sim_ab [na], idx_ba, sim_ba [nb].
    No model, no session."""
    a, b = _f32(a), _f32(b)
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[1], (a.shape, b.shape)
    na, nb = a.shape[0], b.shape[0]
    out = {"idx_ab": np.full(na, -1, np.int32), "sim_ab": np.full(na, np.nan, np.float32),
           "idx_ba": np.full(nb, -1, np.int32), "sim_ba": np.full(nb, np.nan, np.float32)}
    _op_rc(lib().dinov2_hip_op_match(_ptr(a), na, _ptr(b), nb, a.shape[1], _ptr(out["idx_ab"]), _ptr(out["sim_ab"]), _ptr(out["idx_ba"]),
                                     _ptr(out["sim_ba"])), "match")
    return out


def op_bank_topk(q, b, k, chunk_tiles=0):
    """The kernels of csrc/bank.hip alone (dinov2_hip_op_bank_topk): q [nq, H] against the bank built from b [nb, H] -> dict of idx, sim
    [nq, k].  chunk_tiles: column tiles per workgroup, 0 = the planner's choice.  No model, no session."""
    q, b = _f32(q), _f32(b)
    assert q.ndim == 2 and b.ndim == 2 and q.shape[1] == b.shape[1], (q.shape, b.shape)
    nq, nb = q.shape[0], b.shape[0]
    out = {"idx": np.full((nq, k), -7, np.int32), "sim": np.full((nq, k), np.nan, np.float32)}
    _op_rc(lib().dinov2_hip_op_bank_topk(_ptr(q), nq, _ptr(b), nb, q.shape[1], int(k), int(chunk_tiles), _ptr(out["idx"]), _ptr(out["sim"])),
           "bank_topk")
    return out


def _slot_mask(slots):
    """A slots argument -- a mask, or an iterable of slot numbers -- as the 64-bit mask."""
    if isinstance(slots, (int, np.integer)):
        return int(slots)
    m = 0
    for f in slots:
        if not 0 <= int(f) < 64:
            raise ValueError(f"slot {f} outside 0 .. 63")
        m |= 1 << int(f)
    return m


def op_propagate(q, rows, labels, grid, slots, radius, k, temperature, chunk_tiles=0):
    """The kernels behind dinov2_hip_propagate alone (dinov2_hip_op_propagate): q [P, H] against a memory built from rows [frames, P, H] and
    labels [frames, P, C], grid = (h0, w0), `slots` a mask or a list of slot numbers -> dict of labels [P, C], argmax [P], idx / sim [P, k]
    and kept [P, C] (what a call with keep leaves in the memory).  chunk_tiles: items per workgroup, 0 = the planner's choice.  No model,
    no session."""
    q, rows, labels = _f32(q), _f32(rows), _f32(labels)
    h0, w0 = int(grid[0]), int(grid[1])
    P = h0 * w0
    assert q.ndim == 2 and rows.ndim == 3 and labels.ndim == 3 and q.shape[0] == P and rows.shape[1:] == q.shape, (q.shape, rows.shape)
    assert labels.shape[:2] == rows.shape[:2], (labels.shape, rows.shape)
    frames, Cn, k = rows.shape[0], labels.shape[2], int(k)
    out = {"labels": np.full((P, Cn), np.nan, np.float32), "argmax": np.full(P, -7, np.int32), "idx": np.full((P, k), -7, np.int32),
           "sim": np.full((P, k), np.nan, np.float32), "kept": np.full((P, Cn), np.nan, np.float32)}
    _op_rc(lib().dinov2_hip_op_propagate(_ptr(q), _ptr(rows), _ptr(labels), h0, w0, q.shape[1], frames, Cn, _slot_mask(slots), int(radius), k,
                                         float(temperature), int(chunk_tiles), _ptr(out["labels"]), _ptr(out["argmax"]), _ptr(out["idx"]),
                                         _ptr(out["sim"]), _ptr(out["kept"])), "propagate")
    return out


PROPAGATE_PLAN_FIELDS = ("chunk_tiles", "nchunks", "qtiles", "max_items", "kept_items", "partial_bytes", "bytes", "memory_bytes")


def op_propagate_plan(grid, H, nactive, radius, k, C_=1, chunk_tiles=0):
    """propagate_plan (csrc/kernels.h) as a dict, with "ranges" [query tiles, 2] = the kept column tiles [t0, t1) of every query tile; no
    device needed."""
    h0, w0 = int(grid[0]), int(grid[1])
    buf = (C.c_int64 * len(PROPAGATE_PLAN_FIELDS))()
    ranges = np.full((max(-(-h0 * w0 // 128), 1), 2), -1, np.int32)
    if lib().dinov2_hip_op_propagate_plan(h0, w0, int(H), int(nactive), int(radius), int(k), int(C_), int(chunk_tiles), buf, _ptr(ranges)) != 0:
        raise ValueError(f"propagate refuses grid={grid} H={H} nactive={nactive} radius={radius} k={k} C={C_}")
    p = dict(zip(PROPAGATE_PLAN_FIELDS, [int(v) for v in buf]))
    p["ranges"] = ranges
    return p


KMEANS_PLAN_FIELDS = ("npad", "kpad", "hpad", "hpad128", "chunk", "nsplit", "partial_bytes", "bytes")


def op_kmeans_plan(n, K, H, nsplit=0):
    """kmeans_plan (csrc/kernels.h) as a dict; no device needed."""
    buf = (C.c_int64 * len(KMEANS_PLAN_FIELDS))()
    if lib().dinov2_hip_op_kmeans_plan(int(n), int(K), int(H), int(nsplit), buf) != 0:
        raise ValueError(f"kmeans refuses n={n} K={K} H={H} nsplit={nsplit}")
    return dict(zip(KMEANS_PLAN_FIELDS, [int(v) for v in buf]))


def op_kmeans_assign(rows, centers):
    """kmeans_assign_kernel alone (dinov2_hip_op_kmeans_assign): rows [n, H] against centers [K, H] -> dict of labels [n] int32, sim [n] f32.
    No model, no session.  Raises on a HIP error or a changed guard band."""
    x, c = _f32(rows), _f32(centers)
    assert x.ndim == 2 and c.ndim == 2 and x.shape[1] == c.shape[1], (x.shape, c.shape)
    n = x.shape[0]
    out = {"labels": np.full(n, -7, np.int32), "sim": np.full(n, np.nan, np.float32)}
    _op_rc(lib().dinov2_hip_op_kmeans_assign(_ptr(x), n, _ptr(c), c.shape[0], x.shape[1], _ptr(out["labels"]), _ptr(out["sim"])), "kmeans_assign")
    return out


def op_kmeans_update(rows, labels, K, prev_centers, nsplit=0):
    """Transpose, update and finish of csrc/kmeans.hip for given labels (dinov2_hip_op_kmeans_update): dict of centers [K, H] (prev_centers
    where a cluster is empty), counts [K] and xhat [n, H], the f32 values of the f16 rows that were summed."""
    x, prev = _f32(rows), _f32(prev_centers)
    lab = np.ascontiguousarray(labels, np.int32)
    n, H = x.shape
    assert lab.shape == (n,) and prev.shape == (int(K), H), (lab.shape, prev.shape)
    out = {"centers": np.full((int(K), H), np.nan, np.float32), "counts": np.full(int(K), -7, np.int32), "xhat": np.full((n, H), np.nan, np.float32)}
    _op_rc(lib().dinov2_hip_op_kmeans_update(_ptr(x), n, _ptr(lab), int(K), H, int(nsplit), _ptr(prev), _ptr(out["centers"]), _ptr(out["counts"]),
                                             _ptr(out["xhat"])), "kmeans_update")
    return out


def _kmeans_init(init, n, K, H, seed):
    """(init id, centres or None, row indices or None) of the `init` argument of Session.kmeans / op_kmeans."""
    if init is None:
        if K > n:
            raise ValueError(f"kmeans: K = {K} distinct rows cannot be drawn from n = {n}")
        return KMEANS_INIT_ROWS, None, np.sort(np.random.default_rng(seed).choice(n, int(K), replace=False)).astype(np.int32)
    a = np.asarray(init)
    if a.ndim == 1 and np.issubdtype(a.dtype, np.integer):
        if a.shape != (int(K),):
            raise ValueError("kmeans: init row indices must be [K]")
        return KMEANS_INIT_ROWS, None, np.ascontiguousarray(a, np.int32)
    if a.shape != (int(K), int(H)):
        raise ValueError("kmeans: init must be None, [K] row indices or [K, H] centres")
    return KMEANS_INIT_GIVEN, _f32(a), None


def _kmeans_out(n, K, H):
    return {"labels": np.full(n, -7, np.int32), "sim": np.full(n, np.nan, np.float32), "centers": np.full((K, H), np.nan, np.float32),
            "counts": np.full(K, -7, np.int32)}


def op_kmeans(rows, K, max_iter=20, init=None, seed=0):
    """The whole loop of dinov2_hip_kmeans_tokens on host rows without a model or session (dinov2_hip_op_kmeans); the dict of Session.kmeans."""
    x = _f32(rows)
    n, H = x.shape
    _, cen, idx = _kmeans_init(init, n, int(K), H, seed)
    out = _kmeans_out(n, int(K), H)
    it, conv = C.c_int32(-1), C.c_int32(-1)
    _op_rc(lib().dinov2_hip_op_kmeans(_ptr(x), n, int(K), H, int(max_iter), _ptr(cen), _ptr(idx), _ptr(out["labels"]), _ptr(out["sim"]),
                                      _ptr(out["centers"]), _ptr(out["counts"]), C.byref(it), C.byref(conv)), "kmeans")
    out.update(iterations=int(it.value), converged=bool(conv.value))
    return out


CORESET_PLAN_FIELDS = ("npad", "hpad", "rows_per_wg", "nparts", "bytes")


def op_coreset_plan(n, H, m=1, rows_per_wg=0):
    """coreset_plan (csrc/kernels.h) as a dict; no device needed."""
    buf = (C.c_int64 * len(CORESET_PLAN_FIELDS))()
    if lib().dinov2_hip_op_coreset_plan(int(n), int(H), int(m), int(rows_per_wg), buf) != 0:
        raise ValueError(f"coreset refuses n={n} H={H} m={m} rows_per_wg={rows_per_wg}")
    return dict(zip(CORESET_PLAN_FIELDS, [int(v) for v in buf]))


def _coreset_out(n, m):
    return {"idx": np.full(m, -7, np.int32), "cover": np.full(m, np.nan, np.float32), "nearest": np.full(n, -7, np.int32),
            "near_sim": np.full(n, np.nan, np.float32)}


def op_coreset(rows, m, first=0, stop_sim=None, rows_per_wg=0):
    """The kernels of csrc/coreset.hip on host rows without a model or session (dinov2_hip_op_coreset); the dict of Session.coreset.
    rows_per_wg: rows per workgroup, 0 = the planner's choice."""
    x = _f32(rows)
    n, H = x.shape
    out = _coreset_out(n, int(m))
    sel = C.c_int32(-1)
    rc = lib().dinov2_hip_op_coreset(_ptr(x), n, H, int(m), int(first), float(np.inf if stop_sim is None else stop_sim), int(rows_per_wg),
                                     _ptr(out["idx"]), _ptr(out["cover"]), C.byref(sel), _ptr(out["nearest"]), _ptr(out["near_sim"]))
    if rc == 4:
        raise ValueError(f"coreset refuses n={n} H={H} m={m} first={first} stop_sim={stop_sim} rows_per_wg={rows_per_wg}")
    _op_rc(rc, "coreset")
    out["selected"] = int(sel.value)
    return out


VLAD_PLAN_FIELDS = ("kpad", "hpad", "hpad128", "chunk", "cap", "npad", "ntiles", "nchunks", "npass", "partial_bytes", "bytes")


def op_ncut_plan(n, H, nchunk=0):
    """ncut_plan (csrc/kernels.h) as a dict; no device needed."""
    buf = (C.c_int64 * 8)()
    if lib().dinov2_hip_op_ncut_plan(int(n), int(H), int(nchunk), buf) != 0:
        raise ValueError(f"ncut refuses n={n} H={H} nchunk={nchunk}")
    return dict(zip(("npad", "hpad", "ntiles", "chunk_tiles", "nchunks", "part_bytes", "bytes"), (int(v) for v in buf)))


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, np.float64)


def op_ncut_apply(rows, affinity, tau=0.2, floor=1e-5, scale=None, q=None, nchunk=0, want=("t", "degree", "xhat")):
    """ncut_apply_kernel and the degree pass on host rows [n, H] (dinov2_hip_op_ncut_apply): dict of t [n, 8] f64 = W (scale * q) (q [n, 8],
    scale [n] or None = ones), degree [n] f64, xhat [n, H] = the f32 values of the device's f16 rows."""
    x, s, qq = _f32(rows), _f64(scale), _f64(q)
    n, H = x.shape
    if qq is not None and qq.shape != (n, NCUT_NB) or s is not None and s.shape != (n,):
        raise ValueError("ncut_apply: q must be [n, 8] and scale [n]")
    out = {}
    if "t" in want and qq is not None:
        out["t"] = np.full((n, NCUT_NB), np.nan, np.float64)
    if "degree" in want:
        out["degree"] = np.full(n, np.nan, np.float64)
    if "xhat" in want:
        out["xhat"] = np.full((n, H), np.nan, np.float32)
    _op_rc(lib().dinov2_hip_op_ncut_apply(_ptr(x), n, H, _ncut_affinity(affinity), float(tau), float(floor), _ptr(s), _ptr(qq), int(nchunk),
                                          _ptr(out.get("t")), _ptr(out.get("degree")), _ptr(out.get("xhat"))), "ncut_apply")
    return out


def op_ncut_step(rows, affinity, tau, floor, yprev, gprev_parts, nchunk=0):
    """One full step of dinov2_hip_ncut's iteration on host rows (dinov2_hip_op_ncut_step): yprev [n, 8] f64 and the partials of its Gram
    matrix gprev_parts [<= row tiles, 64] (missing partials are zeros) -> dict of ynext [n, 8], gnext_parts, ritz_parts [row tiles, 64]."""
    x, y = _f32(rows), _f64(yprev)
    n, H = x.shape
    nt = op_ncut_plan(n, H, nchunk)["ntiles"]
    g = np.zeros((nt, 64), np.float64)
    gp = _f64(gprev_parts).reshape(-1, 64)
    if y.shape != (n, NCUT_NB) or gp.shape[0] > nt:
        raise ValueError("ncut_step: yprev must be [n, 8] and gprev_parts at most [row tiles, 64]")
    g[:gp.shape[0]] = gp
    out = {"ynext": np.full((n, NCUT_NB), np.nan), "gnext_parts": np.full((nt, 64), np.nan), "ritz_parts": np.full((nt, 64), np.nan)}
    _op_rc(lib().dinov2_hip_op_ncut_step(_ptr(x), n, H, _ncut_affinity(affinity), float(tau), float(floor), int(nchunk), _ptr(y), _ptr(g),
                                         _ptr(out["ynext"]), _ptr(out["gnext_parts"]), _ptr(out["ritz_parts"])), "ncut_step")
    return out


def _ncut_out(n, n_eig):
    n, n_eig = max(int(n), 0), max(int(n_eig), 0)
    return {"values": np.full(n_eig, np.nan, np.float32), "vectors": np.full((n_eig, n), np.nan, np.float32),
            "degree": np.full(n, np.nan, np.float32), "residual": np.full(n_eig, np.nan, np.float32)}


def op_ncut(rows, n_eig=4, affinity="threshold", tau=0.2, floor=1e-5, max_iter=1000, tol=1e-4):
    """The whole of dinov2_hip_ncut_tokens on host rows without a model or session (dinov2_hip_op_ncut); the dict of Session.ncut."""
    x = _f32(rows)
    n, H = x.shape
    out = _ncut_out(n, n_eig)
    it, conv = C.c_int32(-1), C.c_int32(-1)
    _op_rc(lib().dinov2_hip_op_ncut(_ptr(x), n, H, _ncut_affinity(affinity), float(tau), float(floor), int(n_eig), int(max_iter), float(tol),
                                    _ptr(out["values"]), _ptr(out["vectors"]), _ptr(out["degree"]), _ptr(out["residual"]), C.byref(it),
                                    C.byref(conv)), "ncut")
    out.update(iterations=int(it.value), converged=bool(conv.value))
    return out


def tokencut_mask(v):
    """TokenCut's bipartition of a second eigenvector: v > mean(v), with the side that holds the entry of largest magnitude as foreground."""
    v = np.asarray(v)
    mask = v > v.mean()
    return mask if mask[int(np.argmax(np.abs(v)))] else ~mask


def _vlad_offsets(offsets, n):
    """[n_seg + 1] int32 offsets; None = one segment of n rows."""
    return np.asarray([0, n], np.int32) if offsets is None else np.ascontiguousarray(offsets, np.int32)


def op_vlad_plan(offsets, K, H):
    """vlad_plan (csrc/kernels.h) as a dict: its numbers, segs [n_seg, 4] (first padded row, length, first chunk, chunks) and chunks
    [nchunks, 3] (segment, first padded row, K-tiles); no device needed."""
    off = _vlad_offsets(offsets, 0)
    n_seg = len(off) - 1
    buf = (C.c_int64 * 12)()
    segs = np.full((max(n_seg, 0), 4), -7, np.int32)
    if lib().dinov2_hip_op_vlad_plan(_ptr(off), n_seg, int(K), int(H), buf, _ptr(segs), None, 0) != 0:
        raise ValueError(f"vlad refuses offsets={list(off[:8])}.. K={K} H={H}")
    out = dict(zip(VLAD_PLAN_FIELDS, [int(v) for v in buf]))
    chunks = np.full((out["nchunks"], 3), -7, np.int32)
    if lib().dinov2_hip_op_vlad_plan(_ptr(off), n_seg, int(K), int(H), buf, _ptr(segs), _ptr(chunks), out["nchunks"]) != 0:
        raise ValueError("vlad_plan refuses its own chunk count")
    out.update(segs=segs, chunks=chunks)
    return out


def op_vlad(rows, centers, offsets=None, flags=VLAD_INTRA_NORM | VLAD_L2_NORM):
    """The device work of dinov2_hip_vlad_tokens on host rows without a model or session (dinov2_hip_op_vlad): dict of labels [n], sim [n],
    counts [n_seg, K], vlad [n_seg, K, H], and xhat [n, H] / chat [K, H], the f32 values of the f16 operands.  Raises on a HIP error or a
    changed guard band."""
    x, c = _f32(rows), _f32(centers)
    assert x.ndim == 2 and c.ndim == 2 and x.shape[1] == c.shape[1], (x.shape, c.shape)
    n, H = x.shape
    K = c.shape[0]
    off = _vlad_offsets(offsets, n)
    n_seg = len(off) - 1
    assert n_seg >= 1 and int(off[-1]) == n, (off, n)
    out = {"labels": np.full(n, -7, np.int32), "sim": np.full(n, np.nan, np.float32), "counts": np.full((n_seg, K), -7, np.int32),
           "vlad": np.full((n_seg, K, H), np.nan, np.float32), "xhat": np.full((n, H), np.nan, np.float32),
           "chat": np.full((K, H), np.nan, np.float32)}
    _op_rc(lib().dinov2_hip_op_vlad(_ptr(x), _ptr(off), n_seg, _ptr(c), K, H, int(flags), _ptr(out["labels"]), _ptr(out["sim"]),
                                    _ptr(out["counts"]), _ptr(out["vlad"]), _ptr(out["xhat"]), _ptr(out["chat"])), "vlad")
    return out


def op_dense_reduce(logits, h0, w0, out_h, out_w, reduce="argmax", centers=None, eps=0.0, want=("labels", "value")):
    """dense_reduce_kernel alone (dinov2_hip_op_dense_reduce): logits [h0 * w0, C] of one image -> dict of labels [out_h, out_w] uint8 (argmax
    only) and value [out_h, out_w] f32.  Raises on a HIP error or a changed guard band."""
    lg = _f32(logits)
    if lg.ndim != 2 or lg.shape[0] != h0 * w0:
        raise ValueError("op_dense_reduce: logits must be [h0 * w0, C]")
    red = _DENSE_REDUCE[reduce]
    out = {}
    if red == DENSE_ARGMAX and "labels" in want:
        out["labels"] = np.empty((int(out_h), int(out_w)), np.uint8)
    if "value" in want:
        out["value"] = np.empty((int(out_h), int(out_w)), np.float32)
    _op_rc(lib().dinov2_hip_op_dense_reduce(_ptr(lg), int(h0), int(w0), lg.shape[1], int(out_h), int(out_w), red, _ptr(_f32(centers)),
                                            float(eps), _ptr(out.get("labels")), _ptr(out.get("value"))), "dense_reduce")
    return out


def op_dense_pack(x, w, b, eps, R, *, norm, concat_cls, slot=0, nslots=1):
    """dense_pack_kernel alone (dinov2_hip_op_dense_pack): x [B, T, H] f32 -> [B * P, nslots * H * (1 + concat_cls)] f32, the values of the f16
    operand after one launch into column block `slot` (the other blocks come back as NaN).  Raises on a HIP error or a changed guard band."""
    x = _f32(x)
    B, T, H = x.shape
    P = T - 1 - R
    out = np.empty((B * P, nslots * H * (2 if concat_cls else 1)), np.float32)
    _op_rc(lib().dinov2_hip_op_dense_pack(_ptr(x), _ptr(_f32(w)), _ptr(_f32(b)), float(eps), B, T, int(R), H, int(bool(norm)),
                                          int(bool(concat_cls)), int(slot), int(nslots), _ptr(out)), "dense_pack")
    return out


DENSE_PLAN_FIELDS = ("tile_y", "tile_x", "span_y", "span_x", "pitch", "lds_bytes")


def dense_reduce_plan(h0, w0, C_, out_h, out_w):
    """dense_reduce_plan (csrc/kernels.h) as a dict; no device.  ValueError for sizes out of range."""
    buf = (C.c_int64 * 6)()
    if lib().dinov2_hip_op_dense_reduce_plan(int(h0), int(w0), int(C_), int(out_h), int(out_w), buf) != 0:
        raise ValueError(f"dense_reduce_plan: {(h0, w0, C_, out_h, out_w)} out of range")
    return dict(zip(DENSE_PLAN_FIELDS, (int(v) for v in buf)))


def _starts(y1, x1):
    ys, xs = np.ascontiguousarray(y1, np.int32).ravel(), np.ascontiguousarray(x1, np.int32).ravel()
    return ys, xs, ys.ctypes.data_as(C.POINTER(C.c_int32)), xs.ctypes.data_as(C.POINTER(C.c_int32))


def op_slide_reduce(logits, h0, w0, crop, size, y1, x1, reduce="argmax", centers=None, eps=0.0, want=("labels", "value")):
    """slide_reduce_kernel alone (dinov2_hip_op_slide_reduce): logits [len(y1) * len(x1), h0 * w0, C] of one image's windows (index order), crop
    (crop_h, crop_w), size (h, w) -> dict of labels [h, w] uint8 (argmax only) and value [h, w] f32.  Raises on refused arguments, a HIP error
    or a changed guard band."""
    lg = _f32(logits)
    ys, xs, yp, xp = _starts(y1, x1)
    if lg.ndim != 3 or lg.shape[0] != len(ys) * len(xs) or lg.shape[1] != h0 * w0:
        raise ValueError("op_slide_reduce: logits must be [ny * nx, h0 * w0, C]")
    (ch, cw), (h, w) = _pair(crop), _pair(size)
    red = _DENSE_REDUCE[reduce]
    out = {}
    if red == DENSE_ARGMAX and "labels" in want:
        out["labels"] = np.empty((h, w), np.uint8)
    if "value" in want:
        out["value"] = np.empty((h, w), np.float32)
    _op_rc(lib().dinov2_hip_op_slide_reduce(_ptr(lg), int(h0), int(w0), lg.shape[2], ch, cw, h, w, yp, len(ys), xp, len(xs), red,
                                            _ptr(_f32(centers)), float(eps), _ptr(out.get("labels")), _ptr(out.get("value"))), "slide_reduce")
    return out


def op_slide_gather(image, crop, y1, x1, layout=RGB_CHW):
    """slide_gather_kernel alone (dinov2_hip_op_slide_gather): image [3, h, w] (RGB_CHW) or [h, w, 3] f32 -> the window batch
    [len(y1) * len(x1), 3, crop_h, crop_w] or [.., crop_h, crop_w, 3].  Raises on refused arguments, a HIP error or a changed guard band."""
    img = _f32(image)
    if img.ndim != 3 or (img.shape[0] if layout == RGB_CHW else img.shape[2]) != 3:
        raise ValueError("op_slide_gather: image must be [3, h, w] (RGB_CHW) or [h, w, 3]")
    h, w = (img.shape[1], img.shape[2]) if layout == RGB_CHW else (img.shape[0], img.shape[1])
    ys, xs, yp, xp = _starts(y1, x1)
    ch, cw = _pair(crop)
    out = np.empty((len(ys) * len(xs),) + ((3, ch, cw) if layout == RGB_CHW else (ch, cw, 3)), np.float32)
    _op_rc(lib().dinov2_hip_op_slide_gather(_ptr(img), int(layout), h, w, ch, cw, yp, len(ys), xp, len(xs), _ptr(out)), "slide_gather")
    return out


SLIDE_PLAN_FIELDS = ("tile_y", "tile_x", "slots_y", "slots_x", "span_y", "span_x", "chunk", "pitch", "lds_bytes", "cover")


def op_slide_reduce_plan(h0, w0, C_, crop, size, y1, x1):
    """slide_reduce_plan (csrc/kernels.h) as a dict; no device.  ValueError for refused arguments (sizes out of range, starts that do not
    tile the image, a cover above SLIDE_COVER_MAX)."""
    ys, xs, yp, xp = _starts(y1, x1)
    (ch, cw), (h, w) = _pair(crop), _pair(size)
    buf = (C.c_int64 * 10)()
    if lib().dinov2_hip_op_slide_reduce_plan(int(h0), int(w0), int(C_), ch, cw, h, w, yp, len(ys), xp, len(xs), buf) != 0:
        raise ValueError(f"slide_reduce_plan: {(h0, w0, C_, ch, cw, h, w)} with starts {ys.tolist()} x {xs.tolist()} refused")
    return dict(zip(SLIDE_PLAN_FIELDS, (int(v) for v in buf)))


def fold_batchnorm(weight, bias, gamma, beta, mean, var, eps=1e-5):
    """The BatchNorm in front of a linear head folded into it (float64 arithmetic, float32 results): s = gamma / sqrt(var + eps),
    W' = W diag(s), b' = b + W (beta - mean * s).  weight [C, K]; bias [C] or None; the four BatchNorm vectors [K]."""
    W = np.asarray(weight, np.float64)
    g, bt, mu, v = (np.asarray(a, np.float64) for a in (gamma, beta, mean, var))
    s = g / np.sqrt(v + float(eps))
    b0 = np.zeros(W.shape[0]) if bias is None else np.asarray(bias, np.float64)
    return (W * s[None, :]).astype(np.float32), (b0 + W @ (bt - mu * s)).astype(np.float32)


BANK_PLAN_FIELDS = ("chunk_tiles", "nchunks", "pass_tiles", "ntiles", "partial_bytes", "bytes")


def bank_plan(nq, nb, H, k, chunk_tiles=0):
    """bank_topk_plan (csrc/kernels.h) as a dict; no device needed."""
    buf = (C.c_int64 * len(BANK_PLAN_FIELDS))()
    if lib().dinov2_hip_op_bank_plan(int(nq), int(nb), int(H), int(k), int(chunk_tiles), buf) != 0:
        raise ValueError(f"bank_topk refuses nq={nq} nb={nb} H={H} k={k}")
    return dict(zip(BANK_PLAN_FIELDS, [int(v) for v in buf]))


def pca_ppad(P):
    """Ppad of dinov2_hip_pca3: the token count padded to the K of its covariance GEMM (no device needed)."""
    return int(lib().dinov2_hip_op_pca_ppad(int(P)))


def pca_blocks(H):
    """Workgroups of pca_power_kernel = rows of its Gram partials (no device needed)."""
    return int(lib().dinov2_hip_op_pca_blocks(int(H)))


def op_pca_prepare(tok):
    """pca_mean_kernel + pca_center_transpose_kernel (dinov2_hip_op_pca_prepare): tok [P, H] f32 -> (mean [H] f32, xt [H, Ppad] f32 values of
    the f16 matrix, padded columns included).  Raises on a HIP error or a changed guard band."""
    tok = _f32(tok)
    P, H = tok.shape
    mean, xt = np.zeros(H, np.float32), np.zeros((H, pca_ppad(P)), np.float32)
    _op_rc(lib().dinov2_hip_op_pca_prepare(_ptr(tok), P, H, _ptr(mean), _ptr(xt)), "pca_prepare")
    return mean, xt


def op_pca_cov(tok):
    """prepare + the driver's aliased covariance GEMM (dinov2_hip_op_pca_cov): tok [P, H] f32 -> cov [H, H] f32 = Xt Xt^T."""
    tok = _f32(tok)
    P, H = tok.shape
    cov = np.zeros((H, H), np.float32)
    _op_rc(lib().dinov2_hip_op_pca_cov(_ptr(tok), P, H, _ptr(cov)), "pca_cov")
    return cov


def op_pca_power(cov, yprev, gprev_parts):
    """One pca_power_kernel launch (dinov2_hip_op_pca_power): cov [H, H] f32, yprev [H, 8] f64, gprev_parts [pca_blocks(H), 64] f64 ->
    (ynext [H, 8], gnext_parts [pca_blocks(H), 64]) f64."""
    cov = _f32(cov)
    H = cov.shape[0]
    yprev, gprev_parts = np.ascontiguousarray(yprev, np.float64), np.ascontiguousarray(gprev_parts, np.float64)
    nb = pca_blocks(H)
    assert cov.shape == (H, H) and yprev.shape == (H, 8) and gprev_parts.shape == (nb, 64), (cov.shape, yprev.shape, gprev_parts.shape)
    ynext, gnext = np.zeros((H, 8), np.float64), np.zeros((nb, 64), np.float64)
    _op_rc(lib().dinov2_hip_op_pca_power(_ptr(cov), _ptr(yprev), _ptr(gprev_parts), H, _ptr(ynext), _ptr(gnext)), "pca_power")
    return ynext, gnext


def op_pca_project(tok, mean, comp):
    """pca_project_kernel (dinov2_hip_op_pca_project): tok [P, H], mean [H], comp [3, H] f32 -> proj [P, 3] f32."""
    tok, mean, comp = _f32(tok), _f32(mean), _f32(comp)
    P, H = tok.shape
    assert mean.shape == (H,) and comp.shape == (3, H), (mean.shape, comp.shape)
    proj = np.zeros((P, 3), np.float32)
    _op_rc(lib().dinov2_hip_op_pca_project(_ptr(tok), _ptr(mean), _ptr(comp), P, H, _ptr(proj)), "pca_project")
    return proj


def pca_chol_rinv(gram):
    """pca_chol_rinv of csrc/kernels.h on the host: gram [8, 8] f64 -> rinv [8, 8] f64."""
    gram = np.ascontiguousarray(gram, np.float64)
    assert gram.shape == (8, 8), gram.shape
    rinv = np.zeros((8, 8), np.float64)
    _op_rc(lib().dinov2_hip_op_pca_chol_rinv(_ptr(gram), _ptr(rinv)), "pca_chol_rinv")
    return rinv


def lib():
    """Load libdinov2_hip.so; raise loudly if it is not built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    try:  # share ONE HIP runtime with torch when torch is in the process (same SONAME libamdhip64.so.7)
        import sys
        if "torch" in sys.modules:
            import torch  # noqa: F401
    except Exception:
        pass
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise HipLibraryMissing(f"cannot load {LIB_PATH}: {e}") from e
    vp, i32, u32, sz, cp = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t, C.c_char_p
    L.dinov2_hip_abi_version.restype = C.c_int
    L.dinov2_hip_default_load_opts.argtypes = [C.POINTER(LoadOpts)]
    L.dinov2_hip_default_load_opts.restype = None
    L.dinov2_hip_model_load.argtypes = [cp, C.POINTER(LoadOpts), C.POINTER(vp), cp, sz]
    L.dinov2_hip_model_free.argtypes = [vp]
    L.dinov2_hip_model_free.restype = None
    L.dinov2_hip_model_hparams.argtypes = [vp, C.POINTER(HParams)]
    L.dinov2_hip_model_patch_stride.argtypes = [vp]
    L.dinov2_hip_model_grid.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), cp, sz]
    L.dinov2_hip_model_label.argtypes = [vp, i32]
    L.dinov2_hip_model_label.restype = cp
    L.dinov2_hip_model_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.dinov2_hip_session_create.argtypes = [vp, vp, C.POINTER(vp), cp, sz]
    L.dinov2_hip_session_free.argtypes = [vp]
    L.dinov2_hip_session_free.restype = None
    L.dinov2_hip_workspace_bytes.argtypes = [vp, i32, i32, i32]
    L.dinov2_hip_workspace_bytes.restype = sz
    L.dinov2_hip_session_sync.argtypes = [vp]
    L.dinov2_hip_session_stream.argtypes = [vp]
    L.dinov2_hip_session_stream.restype = vp
    L.dinov2_hip_predict.argtypes = [vp, C.POINTER(Input), C.POINTER(Output), u32, cp, sz]
    L.dinov2_hip_predict_layers.argtypes = [vp, C.POINTER(Input), C.POINTER(Output), C.POINTER(Layers), u32, cp, sz]
    L.dinov2_hip_predict_attention.argtypes = [vp, C.POINTER(Input), C.POINTER(Output), C.POINTER(Layers), C.POINTER(Attention), u32, cp, sz]
    L.dinov2_hip_list_rows.argtypes = [vp, C.POINTER(ImageList), u32, C.POINTER(C.c_int64), cp, sz]
    L.dinov2_hip_predict_list.argtypes = [vp, C.POINTER(ImageList), C.POINTER(Output), u32, cp, sz]
    L.dinov2_hip_default_group_opts.argtypes = [C.POINTER(GroupOpts)]
    L.dinov2_hip_default_group_opts.restype = None
    L.dinov2_hip_group_create.argtypes = [cp, C.POINTER(GroupOpts), C.POINTER(vp), cp, sz]
    L.dinov2_hip_group_free.argtypes = [vp]
    L.dinov2_hip_group_free.restype = None
    L.dinov2_hip_group_size.argtypes = [vp]
    L.dinov2_hip_group_model.argtypes = [vp, i32]
    L.dinov2_hip_group_model.restype = vp
    L.dinov2_hip_group_broadcast_ms.argtypes = [vp]
    L.dinov2_hip_group_broadcast_ms.restype = C.c_double
    L.dinov2_hip_group_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.dinov2_hip_group_predict.argtypes = [vp, C.POINTER(Input), C.POINTER(Output), u32, cp, sz]
    L.dinov2_hip_group_submit.argtypes = [vp, C.POINTER(Input), C.POINTER(Output), u32, C.POINTER(C.c_int64), cp, sz]
    L.dinov2_hip_group_wait.argtypes = [vp, C.c_int64, cp, sz]
    L.dinov2_hip_fetch.argtypes = [vp, C.POINTER(Output), cp, sz]
    L.dinov2_hip_host_alloc.argtypes = [sz]
    L.dinov2_hip_host_alloc.restype = vp
    L.dinov2_hip_host_free.argtypes = [vp]
    L.dinov2_hip_host_free.restype = None
    L.dinov2_hip_interpolate_pos_embed.argtypes = [vp, i32, i32, vp]
    L.dinov2_hip_preprocess_size.argtypes = [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.dinov2_hip_preprocess.argtypes = [i32, vp, i32, i32, i32, vp]
    L.dinov2_hip_session_profile.argtypes = [vp, i32]
    L.dinov2_hip_session_profile_read.argtypes = [vp, i32, C.POINTER(cp), C.POINTER(C.c_float), C.POINTER(i32)]
    L.dinov2_hip_debug_hidden.argtypes = [vp, C.POINTER(Input), i32, vp, cp, sz]
    L.dinov2_hip_pca3.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, cp, sz]
    L.dinov2_hip_match_tokens.argtypes = [vp, C.POINTER(Match), cp, sz]
    L.dinov2_hip_kmeans_tokens.argtypes = [vp, C.POINTER(KMeans), cp, sz]
    L.dinov2_hip_vlad_tokens.argtypes = [vp, C.POINTER(Vlad), cp, sz]
    L.dinov2_hip_bank_create.argtypes = [vp, i32, i32, C.POINTER(vp), cp, sz]
    L.dinov2_hip_bank_free.argtypes = [vp]
    L.dinov2_hip_bank_free.restype = None
    L.dinov2_hip_bank_count.argtypes = [vp]
    L.dinov2_hip_bank_clear.argtypes = [vp]
    L.dinov2_hip_bank_add.argtypes = [vp, vp, C.POINTER(Rows), C.POINTER(i32), cp, sz]
    L.dinov2_hip_bank_topk.argtypes = [vp, vp, C.POINTER(TopK), cp, sz]
    L.dinov2_hip_propmem_create.argtypes = [vp, i32, i32, i32, i32, i32, C.POINTER(vp), cp, sz]
    L.dinov2_hip_propmem_free.argtypes = [vp]
    L.dinov2_hip_propmem_free.restype = None
    L.dinov2_hip_propmem_set.argtypes = [vp, vp, i32, C.POINTER(Rows), vp, i32, cp, sz]
    L.dinov2_hip_propmem_drop.argtypes = [vp, i32]
    L.dinov2_hip_propagate.argtypes = [vp, vp, C.POINTER(PropagateReq), cp, sz]
    L.dinov2_hip_dense_head_create.argtypes = [vp, C.POINTER(DenseDesc), C.POINTER(vp), cp, sz]
    L.dinov2_hip_dense_head_free.argtypes = [vp]
    L.dinov2_hip_dense_head_free.restype = None
    L.dinov2_hip_predict_dense.argtypes = [vp, C.POINTER(Input), C.POINTER(Output), vp, C.POINTER(DenseOut), u32, cp, sz]
    # diagnostic ops (include/dinov2_hip_ops.h)
    fp = C.POINTER(C.c_float)
    L.dinov2_hip_op_gemm.argtypes = [i32, i32, fp, fp, fp, fp, C.c_int64, fp, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                     C.c_float]
    L.dinov2_hip_build_id.restype = C.c_char_p
    L.dinov2_hip_op_gemm_resid_ln.argtypes = [i32, fp, fp, fp, fp, fp, fp, fp, fp, i32, i32, i32]
    L.dinov2_hip_op_gemm_ln_consumer.argtypes = [i32, i32, fp, fp, fp, fp, fp, C.c_float, fp, i32, i32, i32, i32, i32, C.c_float]
    L.dinov2_hip_op_ln_prepare.argtypes = [i32, fp, fp, fp, fp, i32, i32]
    L.dinov2_hip_op_im2col.argtypes = [i32, fp, fp, i32, i32, i32, i32, i32, i32]
    L.dinov2_hip_op_im2col_stride.argtypes = [i32, fp, fp, i32, i32, i32, i32, i32, i32, i32]
    L.dinov2_hip_op_ln_fold_vectors.argtypes = [i32, fp, fp, fp, fp, fp, fp, i32, i32]
    L.dinov2_hip_op_attention.argtypes = [i32, fp, fp, i32, i32, i32, i32]
    L.dinov2_hip_op_attention_ex.argtypes = [i32, fp, fp, i32, i32, i32, i32, i32]
    L.dinov2_hip_op_list_plan.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), i32, i32, i32, i32, C.POINTER(C.c_int64), C.POINTER(i32),
                                          C.POINTER(i32), C.c_int64, C.POINTER(C.c_int64)]
    L.dinov2_hip_op_attention_list.argtypes = [i32, fp, fp, i32, C.POINTER(i32), i32, i32, i32]
    L.dinov2_hip_op_layernorm.argtypes = [i32, fp, fp, fp, fp, i32, i32, C.c_float]
    L.dinov2_hip_op_layer_tap.argtypes = [fp, fp, fp, C.c_float, i32, i32, i32, i32, i32, i32, i32, i32, fp, fp, fp]
    L.dinov2_hip_op_attn_rows.argtypes = [i32, fp, i32, i32, i32, i32, C.POINTER(C.c_int32), i32, i32, i32, fp]
    L.dinov2_hip_op_attn_rows_ex.argtypes = [i32, fp, i32, i32, i32, i32, C.POINTER(C.c_int32), i32, i32, i32, fp, C.c_int64]
    L.dinov2_hip_op_convert_weight.argtypes = [i32, vp, C.c_uint64, u32, fp, i32, i32, i32, i32]
    L.dinov2_hip_op_permute_bias.argtypes = [fp, fp, i32, i32]
    L.dinov2_hip_op_head.argtypes = [i32, fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, C.c_float]
    L.dinov2_hip_op_pca_ritz.argtypes = [vp, vp, vp, i32, vp, vp]
    L.dinov2_hip_op_pca_ppad.argtypes = [i32]
    L.dinov2_hip_op_pca_blocks.argtypes = [i32]
    L.dinov2_hip_op_pca_prepare.argtypes = [vp, i32, i32, vp, vp]
    L.dinov2_hip_op_pca_cov.argtypes = [vp, i32, i32, vp]
    L.dinov2_hip_op_pca_power.argtypes = [vp, vp, vp, i32, vp, vp]
    L.dinov2_hip_op_pca_project.argtypes = [vp, vp, vp, i32, i32, vp]
    L.dinov2_hip_op_pca_chol_rinv.argtypes = [vp, vp]
    L.dinov2_hip_op_match.argtypes = [fp, i32, fp, i32, i32, C.POINTER(i32), fp, C.POINTER(i32), fp]
    L.dinov2_hip_op_bank_topk.argtypes = [fp, i32, fp, i32, i32, i32, i32, C.POINTER(i32), fp]
    ip = C.POINTER(i32)
    L.dinov2_hip_op_kmeans_assign.argtypes = [fp, i32, fp, i32, i32, ip, fp]
    L.dinov2_hip_op_kmeans_update.argtypes = [fp, i32, ip, i32, i32, i32, fp, fp, ip, fp]
    L.dinov2_hip_op_kmeans_plan.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_int64)]
    L.dinov2_hip_op_kmeans.argtypes = [fp, i32, i32, i32, i32, fp, ip, ip, fp, fp, ip, ip, ip]
    L.dinov2_hip_op_kmeans_bench.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, fp]
    L.dinov2_hip_coreset_tokens.argtypes = [vp, C.POINTER(Coreset), cp, sz]
    L.dinov2_hip_bank_keep.argtypes = [vp, vp, ip, i32, cp, sz]
    L.dinov2_hip_op_coreset.argtypes = [fp, i32, i32, i32, i32, C.c_float, i32, ip, fp, ip, ip, fp]
    L.dinov2_hip_op_coreset_plan.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_int64)]
    L.dinov2_hip_op_coreset_bench.argtypes = [vp, i32, i32, i32, i32, i32, i32, fp]
    dp, f32 = C.POINTER(C.c_double), C.c_float
    L.dinov2_hip_ncut_tokens.argtypes = [vp, C.POINTER(NCut), cp, sz]
    L.dinov2_hip_op_ncut_plan.argtypes = [i32, i32, i32, C.POINTER(C.c_int64)]
    L.dinov2_hip_op_ncut_apply.argtypes = [fp, i32, i32, i32, f32, f32, dp, dp, i32, dp, dp, fp]
    L.dinov2_hip_op_ncut_step.argtypes = [fp, i32, i32, i32, f32, f32, i32, dp, dp, dp, dp, dp]
    L.dinov2_hip_op_ncut.argtypes = [fp, i32, i32, i32, f32, f32, i32, i32, f32, fp, fp, fp, fp, ip, ip]
    L.dinov2_hip_op_ncut_bench.argtypes = [vp, i32, i32, i32, f32, f32, i32, i32, i32, f32, i32, i32, fp, ip]
    L.dinov2_hip_op_vlad_plan.argtypes = [ip, i32, i32, i32, C.POINTER(C.c_int64), ip, ip, i32]
    L.dinov2_hip_op_vlad.argtypes = [fp, ip, i32, fp, i32, i32, u32, ip, fp, ip, fp, fp, fp]
    L.dinov2_hip_op_vlad_bench.argtypes = [vp, ip, i32, vp, i32, i32, u32, i32, i32, fp]
    L.dinov2_hip_op_propagate.argtypes = [fp, fp, fp, i32, i32, i32, i32, i32, C.c_uint64, i32, i32, C.c_float, i32, fp, ip, ip, fp, fp]
    L.dinov2_hip_op_propagate_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int64), ip]
    L.dinov2_hip_op_propagate_bench.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_uint64, i32, i32, C.c_float, i32, i32, i32, fp]
    L.dinov2_hip_op_bank_plan.argtypes = [i32, i32, i32, i32, i32, C.POINTER(C.c_int64)]
    L.dinov2_hip_op_dense_reduce.argtypes = [fp, i32, i32, i32, i32, i32, i32, fp, C.c_float, C.POINTER(C.c_uint8), fp]
    L.dinov2_hip_op_dense_pack.argtypes = [fp, fp, fp, C.c_float, i32, i32, i32, i32, i32, i32, i32, i32, fp]
    L.dinov2_hip_op_dense_reduce_plan.argtypes = [i32, i32, i32, i32, i32, C.POINTER(C.c_int64)]
    L.dinov2_hip_slide_windows.argtypes = [vp, i32, i32, C.POINTER(Slide), ip, ip, ip, ip, cp, sz]
    L.dinov2_hip_predict_dense_slide.argtypes = [vp, C.POINTER(Input), vp, C.POINTER(Slide), C.POINTER(DenseOut), cp, sz]
    L.dinov2_hip_op_slide_reduce.argtypes = [fp, i32, i32, i32, i32, i32, i32, i32, ip, i32, ip, i32, i32, fp, C.c_float, C.POINTER(C.c_uint8), fp]
    L.dinov2_hip_op_slide_gather.argtypes = [fp, i32, i32, i32, i32, i32, ip, i32, ip, i32, fp]
    L.dinov2_hip_op_slide_reduce_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, ip, i32, ip, i32, C.POINTER(C.c_int64)]
    L.dinov2_hip_op_bank_bench.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, fp]
    L.dinov2_hip_op_clock_probe.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.dinov2_hip_op_clock_slots.argtypes = [C.POINTER(C.c_uint64)]
    L.dinov2_hip_op_probe_tr16.argtypes = [C.POINTER(C.c_int16)]
    L.dinov2_hip_op_preprocess_u8.argtypes = [i32, vp, i32, i32, i32, i32, vp]
    L.dinov2_hip_op_gemm_bench.argtypes = [i32] * 6
    L.dinov2_hip_op_gemm_bench.restype = C.c_float
    L.dinov2_hip_op_attention_bench.argtypes = [i32] * 6
    L.dinov2_hip_op_attention_bench.restype = C.c_float
    L.dinov2_hip_op_set_tuning.argtypes = [cp, i32]
    L.dinov2_hip_op_get_tuning.argtypes = [cp]
    L.dinov2_hip_op_gemm_plan.argtypes = [i32, i32, i32, i32, i32, C.c_char_p, i32]
    L.dinov2_hip_op_gemm_plan_strided.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.c_char_p, i32]
    L.dinov2_hip_op_gemm_plan_parts.argtypes =[i32, i32, i32, i32, i32, C.POINTER(C.c_int64), i32]
    L.dinov2_hip_op_stream_delay.argtypes = [vp, i32]
    i64p = C.POINTER(C.c_int64)
    L.dinov2_hip_op_device_memory.argtypes = [i64p, i64p]
    L.dinov2_hip_op_gemm_far.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.c_uint64, C.c_uint64, fp, fp, fp, i32, C.c_float, i64p, i32, fp,
                                         i64p]
    L.dinov2_hip_op_attention_far.argtypes = [i32, i32, i32, i32, C.c_uint64, i32, i64p, i32, fp, i64p]
    L.dinov2_hip_op_rows_fill.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, i32, fp, i32, i32, C.c_uint64, i64p, C.POINTER(i32), i32]
    _lib = L
    return L


def _errbuf(size: int = 512):
    return C.create_string_buffer(size)


def _call(fn, *args):
    """One call of a C-ABI function whose last two parameters are (err, errlen): a non-zero status raises DinoError with the library's text."""
    err = _errbuf()
    rc = fn(*args, err, len(err))
    if rc != 0:
        raise DinoError(rc, err.value.decode(errors="replace"))


class _Handle:
    """Owner of one C-ABI handle, `_h`; the subclass names the function that frees it.  close() and free() are the same call."""
    _free = None
    _h = None

    def close(self):
        if self._h:
            getattr(lib(), self._free)(self._h)
            self._h = None

    free = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


U8_BGR_HWC = 2


def preprocess_size(mode: int, h: int, w: int, patch: int = 14) -> tuple[int, int]:
    oh, ow = C.c_int32(), C.c_int32()
    if lib().dinov2_hip_preprocess_size(mode, h, w, patch, C.byref(oh), C.byref(ow)) != 0:
        raise DinoError(4, "preprocess_size")
    return oh.value, ow.value


def dino_preprocess(img_bgr_u8: np.ndarray, patch: int = 14) -> np.ndarray:
    """dino_preprocess (dinov2.cpp:135-156) on the host: [h, w, 3] uint8 BGR -> f32 BGR [(h/p+1)*p, (w/p+1)*p, 3]."""
    return _preprocess(0, img_bgr_u8, patch)


def dino_classify_preprocess(img_bgr_u8: np.ndarray, patch: int = 14) -> np.ndarray:
    """dino_classify_preprocess (dinov2.cpp:106-132): resize to 256x256 ignoring aspect, centre-crop 224, normalise."""
    return _preprocess(1, img_bgr_u8, patch)


def _preprocess(mode, img, patch):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3
    oh, ow = preprocess_size(mode, img.shape[0], img.shape[1], patch)
    out = np.empty((oh, ow, 3), np.float32)
    if lib().dinov2_hip_preprocess(mode, img.ctypes.data, img.shape[0], img.shape[1], patch, out.ctypes.data) != 0:
        raise DinoError(4, "preprocess")
    return out


class Model(_Handle):
    """dino_model counterpart (owning handle)."""
    _free = "dinov2_hip_model_free"

    def __init__(self, path: str, *, device: int = 0, dtype: int = F16, classify: bool = True,
                 skip_tensor_data: bool = False, pool_const_divisor: bool = True, pool_includes_registers: bool = True,
                 batch_invariant: bool = True, ln_fold: int = 0, patch_stride: int = 0):
        """ln_fold: 0 = the library's choice, 1 = LayerNorm folded into the neighbouring GEMMs, -1 = separate LayerNorm launches.
        patch_stride: pixels from one patch to the next, 0 = patch_size, else a divisor of it (overlapping patches: a denser token grid)."""
        L = lib()
        o = LoadOpts()
        L.dinov2_hip_default_load_opts(C.byref(o))
        o.device, o.compute_dtype, o.classify = device, dtype, int(classify)
        o.skip_tensor_data = int(skip_tensor_data)
        o.quirk_pool_const_divisor, o.quirk_pool_includes_registers = int(pool_const_divisor), int(pool_includes_registers)
        o.batch_invariant = int(batch_invariant)
        o.ln_fold = int(ln_fold)
        o.patch_stride = int(patch_stride)
        h = C.c_void_p()
        _call(L.dinov2_hip_model_load, path.encode(), C.byref(o), C.byref(h))
        self._h = h
        hp = HParams()
        L.dinov2_hip_model_hparams(h, C.byref(hp))
        self.patch_stride = hp.patch_stride = int(L.dinov2_hip_model_patch_stride(h))  # resolved: never 0
        self.hparams = hp
        self.device = device

    def label(self, i: int) -> str | None:
        s = lib().dinov2_hip_model_label(self._h, i)
        return s.decode() if s is not None else None

    def arena(self) -> tuple[int, int]:
        p, n = C.c_void_p(), C.c_size_t()
        lib().dinov2_hip_model_arena(self._h, C.byref(p), C.byref(n))
        return int(p.value or 0), int(n.value)

    def workspace_bytes(self, batch, h, w) -> int:
        return int(lib().dinov2_hip_workspace_bytes(self._h, batch, h, w))

    def interpolate_pos_embed(self, h_new, w_new) -> np.ndarray:
        out = np.empty((1 + h_new * w_new, self.hparams.hidden_size), np.float32)
        rc = lib().dinov2_hip_interpolate_pos_embed(self._h, h_new, w_new, out.ctypes.data)
        if rc != 0:
            raise DinoError(rc, "interpolate_pos_embed")
        return out

    def grid(self, h, w) -> tuple[int, int]:
        """(h0, w0): the patch grid of a NETWORK input size h x w (dinov2_hip_model_grid), or the refusal a predict of it would give."""
        h0, w0 = C.c_int32(), C.c_int32()
        _call(lib().dinov2_hip_model_grid, self._h, int(h), int(w), C.byref(h0), C.byref(w0))
        return h0.value, w0.value

    def slide_windows(self, h, w, crop, stride):
        """(y1, x1): the window starts of sliding-window inference over an h x w image (dinov2_hip_slide_windows; no device), int32 arrays;
        window k = iy * len(x1) + ix.  crop and stride: one number or (h, w).  Raises the refusal predict_dense_slide would give."""
        (ch, cw), (sh, sw) = _pair(crop), _pair(stride)
        sl = Slide(ch, cw, sh, sw)
        ny, nx = C.c_int32(), C.c_int32()
        y1, x1 = np.zeros(8192, np.int32), np.zeros(8192, np.int32)
        ip = C.POINTER(C.c_int32)
        _call(lib().dinov2_hip_slide_windows, self._h, int(h), int(w), C.byref(sl), C.byref(ny), C.byref(nx), y1.ctypes.data_as(ip),
              x1.ctypes.data_as(ip))
        return y1[:ny.value].copy(), x1[:nx.value].copy()

    def tokens(self, h, w):
        h0, w0 = _grid_dims(self.hparams, h, w)
        return 1 + self.hparams.num_register_tokens + h0 * w0


def _images(images, layout, dtype=None):
    """The image argument of every predict as the C-ABI takes it: (img, B, hh, ww), img contiguous [B, 3, hh, ww] (RGB_CHW) or [B, hh, ww, 3],
    uint8 for U8_BGR_HWC and float32 otherwise unless `dtype` says so; one image becomes a batch of one.  Any other shape is refused here:
    the library reads B * 3 * hh * ww elements whatever the array holds."""
    img = np.ascontiguousarray(images, dtype=dtype or (np.uint8 if layout == U8_BGR_HWC else np.float32))
    if img.ndim == 3:
        img = img[None]
    if img.ndim != 4 or (img.shape[1] if layout == RGB_CHW else img.shape[3]) != 3:
        raise ValueError(f"expected [B, 3, H, W] (RGB_CHW) or [B, H, W, 3] images, got shape {img.shape}")
    hh, ww = (img.shape[2], img.shape[3]) if layout == RGB_CHW else (img.shape[1], img.shape[2])
    return img, img.shape[0], hh, ww


def _grid_dims(hp, h, w):
    """(h0, w0): the patch grid of a network input size h x w -- patches of hp.patch_size pixels every hp.patch_stride pixels (absent or 0:
    the patch size).  THE definition on the Python side (csrc/kernels.h: grid_dim); nothing else here divides by the patch size for a grid
    or a row count."""
    p = hp.patch_size
    s = getattr(hp, "patch_stride", 0) or p
    return (0 if h < p else (h - p) // s + 1), (0 if w < p else (w - p) // s + 1)


def _grid(hp, hh, ww, layout, classify):
    """(nh, nw, P): the network input size of an hh x ww image (raw 8-bit input: after the preprocessing) and its number of patches."""
    nh, nw = preprocess_size(1 if classify else 0, hh, ww, hp.patch_size) if layout == U8_BGR_HWC else (hh, ww)
    h0, w0 = _grid_dims(hp, nh, nw)
    return nh, nw, h0 * w0


def _device_output(cls_ptr, patch_ptr, logits_ptr, probs_ptr):
    """The Output of the *_device calls: raw device pointers, 0 = not wanted; no top-k on the device."""
    return Output(cls_ptr or None, patch_ptr or None, logits_ptr or None, probs_ptr or None, None, None, 0, 1)


def _alloc_outputs(hp, B, hh, ww, layout, classify, topk, want):
    """Host output arrays + the filled Output struct for a predict of B images (shared by Session and Group)."""
    Hd, R = hp.hidden_size, hp.num_register_tokens
    P = _grid(hp, hh, ww, layout, classify)[2]
    out = {}
    o = Output()
    if "cls" in want:
        out["cls"] = np.empty((B, Hd), np.float32)
        o.cls = out["cls"].ctypes.data
    if "patch_tokens" in want:
        out["patch_tokens"] = np.empty((B, P + (R if classify else 0), Hd), np.float32)
        o.patch_tokens = out["patch_tokens"].ctypes.data
    if classify:
        Cn = hp.num_classes
        if "logits" in want:
            out["logits"] = np.empty((B, Cn), np.float32)
            o.logits = out["logits"].ctypes.data
        if "probs" in want:
            out["probs"] = np.empty((B, Cn), np.float32)
            o.probs = out["probs"].ctypes.data
        if topk > 0:
            out["topk_ids"] = np.empty((B, topk), np.int32)
            out["topk_probs"] = np.empty((B, topk), np.float32)
            o.topk_ids, o.topk_probs, o.topk = out["topk_ids"].ctypes.data, out["topk_probs"].ctypes.data, topk
    return out, o


def _image_list(ptrs, sizes, layout, on_device):
    """(ImageList, the ctypes arrays it points into: kept alive by the caller) of n images at `ptrs` with `sizes` = [(h, w)]."""
    n = len(ptrs)
    data = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in ptrs])
    hs = (C.c_int32 * max(n, 1))(*[int(s[0]) for s in sizes])
    ws = (C.c_int32 * max(n, 1))(*[int(s[1]) for s in sizes])
    il = ImageList(C.cast(data, C.POINTER(C.c_void_p)), C.cast(hs, C.POINTER(C.c_int32)), C.cast(ws, C.POINTER(C.c_int32)), n, int(layout),
                   int(on_device))
    return il, (data, hs, ws)


def list_rows(model: "Model", sizes, *, classify: bool = False, layout: int = RGB_CHW) -> np.ndarray:
    """offsets [n + 1] (dinov2_hip_list_rows; no device): image i of a predict_list of images of these `sizes` = [(h, w)] (RAW sizes for
    U8_BGR_HWC) owns rows offsets[i] .. offsets[i + 1] of the packed patch tokens."""
    il, keep = _image_list([0] * len(sizes), sizes, layout, 0)
    il.data = None
    offsets = np.zeros(len(sizes) + 1, np.int64)
    _call(lib().dinov2_hip_list_rows, model._h, C.byref(il), CLASSIFY if classify else 0, _ptr(offsets))
    del keep
    return offsets


def pinned_empty(shape, dtype=np.float32) -> np.ndarray:
    """numpy array over page-locked host memory (dinov2_hip_host_alloc): host <-> device copies of such buffers run at the full
    PCIe rate.  The memory is released when the array (and every view of it) is garbage-collected."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = lib().dinov2_hip_host_alloc(max(n, 1))
    if not ptr:
        raise MemoryError(f"dinov2_hip_host_alloc({n}) failed")
    buf = (C.c_char * max(n, 1)).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    import weakref
    weakref.finalize(buf, lib().dinov2_hip_host_free, ptr)
    return arr


class DeviceArray:
    """A float32 array in device memory for the *_device calls, for hosts that have no torch in the process: plain hipMalloc / hipMemcpy
    through the HIP runtime the library itself is linked against, on HIP device `device` (the model's: Model.device).  `ptr` is the raw
    device pointer.  free() waits for the device first: a session's stream may still be writing into the buffer."""
    _hip = None

    @classmethod
    def _rt(cls):
        if cls._hip is None:
            lib()  # the library has the runtime loaded: dlopen by SONAME hands back that copy
            for name in ("libamdhip64.so.7", "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
                try:
                    cls._hip = C.CDLL(name)
                    break
                except OSError:
                    continue
            else:
                raise HipLibraryMissing("libamdhip64 not found")
            cls._hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            cls._hip.hipFree.argtypes = [C.c_void_p]
            cls._hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            cls._hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            cls._hip.hipSetDevice.argtypes = [C.c_int]
            cls._hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            cls._hip.hipStreamDestroy.argtypes = [C.c_void_p]
            cls._hip.hipStreamQuery.argtypes = [C.c_void_p]
            cls._hip.hipStreamSynchronize.argtypes = [C.c_void_p]
            cls._hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        return cls._hip

    def _select(self):
        if self._rt().hipSetDevice(self.device) != 0:
            raise RuntimeError(f"hipSetDevice({self.device}) failed")
        return self._hip

    def __init__(self, shape, fill_nan: bool = False, device: int = 0):
        self.shape = tuple(int(v) for v in shape)
        self.nbytes = 4 * int(np.prod(self.shape))
        self.device = int(device)
        p = C.c_void_p()
        if self._select().hipMalloc(C.byref(p), max(self.nbytes, 16)) != 0:
            raise MemoryError(f"hipMalloc({self.nbytes}) failed")
        self.ptr = int(p.value)
        if fill_nan and (self._rt().hipMemset(self.ptr, 0xff, self.nbytes) != 0 or self._rt().hipDeviceSynchronize() != 0):
            raise RuntimeError("hipMemset failed")  # (synchronised: a session's stream is not ordered after the null stream)

    @classmethod
    def from_host(cls, a: np.ndarray, device: int = 0):
        a = np.ascontiguousarray(a, np.float32)
        d = cls(a.shape, device=device)
        if d._select().hipMemcpy(d.ptr, a.ctypes.data, d.nbytes, 1) != 0:  # hipMemcpyHostToDevice (synchronous)
            raise RuntimeError("hipMemcpy to the device failed")
        return d

    def to_host(self) -> np.ndarray:
        out = np.empty(self.shape, np.float32)
        if self._select().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) != 0:  # hipMemcpyDeviceToHost
            raise RuntimeError("hipMemcpy to the host failed")
        return out

    def free(self):
        if getattr(self, "ptr", 0):
            self._select().hipDeviceSynchronize()
            self._hip.hipFree(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def stream_delay(stream, ms):
    """Testing aid (dinov2_hip_op_stream_delay): one kernel on `stream` (a Stream or a raw hipStream_t) that keeps it busy for `ms`
    milliseconds, 1 .. 100 -- a bounded wait, never a hang; returns at once.  ValueError for the null stream or ms out of range."""
    h = int(getattr(stream, "handle", stream) or 0)
    ms = int(ms)
    rc = lib().dinov2_hip_op_stream_delay(C.c_void_p(h) if h else None, ms if -2**31 <= ms < 2**31 else 0)
    if rc == 4:
        raise ValueError(f"stream_delay: stream = {h:#x}, ms = {ms}: needs a stream of its own and 1 <= ms <= 100")
    if rc != 0:
        raise RuntimeError(f"dinov2_hip_op_stream_delay failed ({rc})")


class Stream:
    """A non-blocking HIP stream of the caller's, for hosts that have no torch in the process (Session(model, stream=s.handle)): created,
    queried, synchronised and destroyed through the runtime handle DeviceArray holds, on HIP device `device`."""
    NOT_READY = 600  # hipErrorNotReady

    def __init__(self, device: int = 0, handle: int | None = None):
        """handle: an existing hipStream_t to look at (Session.stream) instead of a new stream; it stays its owner's to destroy."""
        self.device, self.handle, self.owned = int(device), int(handle or 0), handle is None
        if not self.owned:
            return
        rt = DeviceArray._rt()
        h = C.c_void_p()
        if rt.hipSetDevice(self.device) != 0 or rt.hipStreamCreateWithFlags(C.byref(h), 1) != 0:  # hipStreamNonBlocking
            raise RuntimeError("hipStreamCreateWithFlags failed")
        self.handle = int(h.value)

    def copy(self, dst, src, nbytes: int | None = None):
        """Device-to-device copy on this stream; dst / src: DeviceArrays or raw device pointers (then `nbytes` is needed)."""
        n = int(nbytes if nbytes is not None else min(getattr(dst, "nbytes", 1 << 62), getattr(src, "nbytes", 1 << 62)))
        if DeviceArray._rt().hipMemcpyAsync(int(getattr(dst, "ptr", dst)), int(getattr(src, "ptr", src)), n, 3, self.handle) != 0:
            raise RuntimeError("hipMemcpyAsync (device to device) failed")

    def query(self) -> bool:
        """True when everything queued on the stream has finished.  A "not ready" answer is cleared from the runtime's last-error slot,
        so that the library's next launch check does not report it."""
        rt = DeviceArray._rt()
        rc = rt.hipStreamQuery(self.handle)
        if rc == self.NOT_READY:
            rt.hipGetLastError()
            return False
        if rc != 0:
            raise RuntimeError(f"hipStreamQuery failed ({rc})")
        return True

    def synchronize(self):
        if DeviceArray._rt().hipStreamSynchronize(self.handle) != 0:
            raise RuntimeError("hipStreamSynchronize failed")

    def destroy(self):
        if self.handle and self.owned:
            DeviceArray._rt().hipStreamDestroy(self.handle)
        self.handle = 0

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Bank(_Handle):
    """dinov2_hip_bank: a device-resident bank of unit-length f16 rows and its top-k cosine search (include/dinov2_hip.h).  Rows come from
    host arrays, DeviceArrays, or -- source="last_cls" / "last_patches" -- from the session's last un-split predict without leaving the device."""
    _free = "dinov2_hip_bank_free"

    def __init__(self, model: "Model", H: int, capacity: int):
        h = C.c_void_p()
        _call(lib().dinov2_hip_bank_create, model._h, int(H), int(capacity), C.byref(h))
        self._h = h
        self.H, self.capacity = int(H), int(capacity)

    def _rows(self, sess, rows, source, image, n):
        """(Rows struct, the array it points into: kept alive by the caller)."""
        if source is None:
            source = "given" if rows is not None else None
        if source not in _ROWS_SOURCE or (source == "given") != (rows is not None):
            raise ValueError("bank: give rows, or source = 'last_cls' / 'last_patches' without rows")
        if source != "given":
            if n is None:  # what the session's last Session.predict left behind (n=...: after another kind of predict)
                n = getattr(sess, "_last_rows", {}).get(source, 0)
            return Rows(_ROWS_SOURCE[source], None, int(n), self.H, int(image), 0), None
        if isinstance(rows, DeviceArray):
            if len(rows.shape) != 2:
                raise ValueError("bank: rows must be [n, H]")
            return Rows(ROWS_GIVEN, rows.ptr, rows.shape[0], rows.shape[1], 0, 1), rows
        x = np.ascontiguousarray(rows, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("bank: rows must be [n, H]")
        return Rows(ROWS_GIVEN, x.ctypes.data, x.shape[0], x.shape[1], 0, 0), x

    def add(self, sess: "Session", rows=None, *, source=None, image: int = 0, n: int | None = None) -> int:
        """Normalises rows into the bank and returns the index of the first one.  rows: [n, H] host array or DeviceArray; or rows=None with
        source="last_cls" (the CLS row of every image of the session's last predict; n = that batch) or "last_patches" (the patch rows of
        image `image`; n = P); `n` is taken from the session's last predict() unless given."""
        r, keep = self._rows(sess, rows, source, image, n)
        first = C.c_int32(-1)
        _call(lib().dinov2_hip_bank_add, sess._h, self._h, C.byref(r), C.byref(first))
        return int(first.value)

    def topk(self, sess: "Session", queries=None, k: int = 1, *, source=None, image: int = 0, n: int | None = None) -> dict:
        """The k most similar bank rows of every query, best first: dict of idx [nq, k] int32 (insertion indices; -1 past the bank's count)
        and sim [nq, k] f32 (-inf there).  queries as the rows of add()."""
        r, keep = self._rows(sess, queries, source, image, n)
        nq = max(int(r.n), 0)
        out = {"idx": np.empty((nq, int(k)), np.int32), "sim": np.empty((nq, int(k)), np.float32)}
        t = TopK(r, int(k), out["idx"].ctypes.data, out["sim"].ctypes.data)
        _call(lib().dinov2_hip_bank_topk, sess._h, self._h, C.byref(t))
        return out

    def keep(self, sess: "Session", idx) -> np.ndarray:
        """Compacts the bank to the rows `idx` (dinov2_hip_bank_keep): distinct indices in [0, count), in any order.  They are sorted; the
        sorted array is returned, so that new row j is old row result[j] (e.g. the picks of Session.coreset(bank=...))."""
        a = np.asarray(idx)
        if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("bank.keep: idx must be a non-empty 1-D integer array")
        a = np.sort(a.astype(np.int64))
        if a[0] < 0 or a[-1] >= self.count or (np.diff(a) == 0).any():
            raise ValueError(f"bank.keep: indices must be distinct and inside [0, {self.count})")
        a = np.ascontiguousarray(a, np.int32)
        _call(lib().dinov2_hip_bank_keep, sess._h, self._h, _ptr(a), len(a))
        return a

    @property
    def count(self) -> int:
        return int(lib().dinov2_hip_bank_count(self._h))

    def clear(self):
        lib().dinov2_hip_bank_clear(self._h)


class PropMemory(_Handle):
    """dinov2_hip_propmem: a device-resident memory of `frames` slots of one patch grid (unit-length f16 rows and f32 label vectors of
    `channels` channels per patch) and label propagation from it (include/dinov2_hip.h, dinov2_hip_propagate).  Rows come from host arrays,
    DeviceArrays, or -- source="last_patches" -- from the session's last un-split predict without leaving the device."""
    _free = "dinov2_hip_propmem_free"
    OUTPUTS = ("labels", "argmax", "idx", "sim")

    def __init__(self, model: "Model", H: int, grid, frames: int, channels: int):
        h = C.c_void_p()
        h0, w0 = int(grid[0]), int(grid[1])
        _call(lib().dinov2_hip_propmem_create, model._h, int(H), h0, w0, int(frames), int(channels), C.byref(h))
        self._h = h
        self.H, self.grid, self.P, self.frames, self.channels = int(H), (h0, w0), h0 * w0, int(frames), int(channels)

    def _rows(self, rows, source, image):
        """(Rows struct, the array it points into: kept alive by the caller)."""
        if source is None:
            source = "given" if rows is not None else None
        if source not in _ROWS_SOURCE or (source == "given") != (rows is not None):
            raise ValueError("propagate: give rows, or source = 'last_patches' without rows")
        if source != "given":
            return Rows(_ROWS_SOURCE[source], None, self.P, self.H, int(image), 0), None
        if isinstance(rows, DeviceArray):
            if len(rows.shape) != 2:
                raise ValueError("propagate: rows must be [P, H]")
            return Rows(ROWS_GIVEN, rows.ptr, rows.shape[0], rows.shape[1], 0, 1), rows
        x = np.ascontiguousarray(rows, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("propagate: rows must be [P, H]")
        return Rows(ROWS_GIVEN, x.ctypes.data, x.shape[0], x.shape[1], 0, 0), x

    def set(self, sess: "Session", slot: int, rows=None, labels=None, *, source=None, image: int = 0):
        """Fills slot `slot`: rows [P, H] (host array or DeviceArray), or rows=None with source="last_patches" (the patch rows of image
        `image` of the session's last predict); labels [P, channels] (host array or DeviceArray), or None: the result the last
        propagate(keep=True) left in this memory."""
        r, keep = self._rows(rows, source, image)
        lab, on_dev = None, 0
        if isinstance(labels, DeviceArray):
            lab, on_dev = labels.ptr, 1
        elif labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.float32)
            if labels.shape != (self.P, self.channels):
                raise ValueError(f"propagate: labels must be [{self.P}, {self.channels}]")
            lab = labels.ctypes.data
        _call(lib().dinov2_hip_propmem_set, sess._h, self._h, int(slot), C.byref(r), lab, on_dev)

    def drop(self, slot: int):
        if lib().dinov2_hip_propmem_drop(self._h, int(slot)) != 0:
            raise ValueError(f"propagate: slot {slot} outside 0 .. {self.frames - 1}")

    def propagate(self, sess: "Session", queries=None, *, slots, radius: int = -1, k: int = 5, temperature: float = 0.1, keep: bool = False,
                  want=OUTPUTS, source=None, image: int = 0) -> dict:
        """Propagates the labels of the slots `slots` (a mask or a list of slot numbers) to the P queries (as the rows of set()): dict of
        the outputs named in `want` -- labels [P, channels] f32, argmax [P] int32, idx / sim [P, k] (index = slot * P + patch; -1 / -inf past
        a short window).  keep: the result also stays in the memory for the next set(labels=None)."""
        bad = [w for w in want if w not in self.OUTPUTS]
        if bad:
            raise ValueError(f"propagate: unknown outputs {bad}")
        r, alive = self._rows(queries, source, image)
        k = int(k)
        shapes = {"labels": ((self.P, self.channels), np.float32), "argmax": ((self.P,), np.int32), "idx": ((self.P, k), np.int32),
                  "sim": ((self.P, k), np.float32)}
        out = {w: np.empty(tuple(max(d, 0) for d in shapes[w][0]), shapes[w][1]) for w in want}
        ptr = {w: (out[w].ctypes.data if w in out else None) for w in self.OUTPUTS}
        req = PropagateReq(r, _slot_mask(slots), int(radius), k, float(temperature), int(bool(keep)), ptr["labels"], ptr["argmax"], ptr["idx"],
                           ptr["sim"])
        _call(lib().dinov2_hip_propagate, sess._h, self._h, C.byref(req))
        return out


class DenseHead(_Handle):
    """dinov2_hip_dense_head: a resident linear segmentation (reduce="argmax") or depth (reduce="bins") head over the patch tokens of `layers`
    (include/dinov2_hip.h).  weight [C, K], K = len(layers) * H * (1 + concat_cls), column order layer-major, patch then cls; a BatchNorm in
    front of it is folded first (fold_batchnorm)."""
    _free = "dinov2_hip_dense_head_free"

    def __init__(self, model: "Model", layers, weight, bias=None, *, norm: bool = True, concat_cls: bool = False, reduce: str = "argmax",
                 bin_centers=None, bins_eps: float = 0.1):
        ids = [int(v) for v in layers]
        W = np.ascontiguousarray(weight, dtype=np.float32)
        hp = model.hparams
        K = len(ids) * int(hp.hidden_size) * (2 if concat_cls else 1)
        if W.ndim != 2 or W.shape[1] != K:
            raise ValueError(f"DenseHead: weight must be [C, {K}]")
        b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
        cen = np.ascontiguousarray(bin_centers, dtype=np.float32) if bin_centers is not None else None
        if (b is not None and b.shape != (W.shape[0],)) or (cen is not None and cen.shape != (W.shape[0],)):
            raise ValueError("DenseHead: bias and bin_centers must be [C]")
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        d = DenseDesc(arr, len(ids), int(bool(norm)), int(bool(concat_cls)), W.shape[0], W.ctypes.data, b.ctypes.data if b is not None else None,
                      _DENSE_REDUCE[reduce], cen.ctypes.data if cen is not None else None, float(bins_eps))
        h = C.c_void_p()
        _call(lib().dinov2_hip_dense_head_create, model._h, C.byref(d), C.byref(h))
        self._h = h
        self.layers, self.num_classes, self.reduce, self.K = ids, int(W.shape[0]), reduce, K


class Group(_Handle):
    """dinov2_hip_group: N devices behind one handle -- host threads + sessions per device inside the library (two lanes per
    device by default: one lane's PCIe copies run under the other's kernels), the global batch split contiguously, outputs
    landing at the shard offsets of the caller's arrays."""
    _free = "dinov2_hip_group_free"

    def __init__(self, path: str, devices=None, *, dtype: int = F16, classify: bool = True, broadcast: bool = True,
                 batch_invariant: bool = True, streams_per_device: int = 2, patch_stride: int = 0):
        L = lib()
        o = GroupOpts()
        L.dinov2_hip_default_group_opts(C.byref(o))
        o.load.compute_dtype, o.load.classify = dtype, int(classify)
        o.load.patch_stride = int(patch_stride)
        o.load.batch_invariant = int(batch_invariant)
        o.broadcast = int(broadcast)
        o.streams_per_device = int(streams_per_device)
        if devices is not None:
            self._devs = (C.c_int32 * len(devices))(*devices)
            o.n_devices, o.devices = len(devices), self._devs
        h = C.c_void_p()
        _call(L.dinov2_hip_group_create, path.encode(), C.byref(o), C.byref(h))
        self._h = h
        self.size = int(L.dinov2_hip_group_size(h))
        self.hparams = HParams()
        L.dinov2_hip_model_hparams(L.dinov2_hip_group_model(h, 0), C.byref(self.hparams))
        self.patch_stride = self.hparams.patch_stride = int(L.dinov2_hip_model_patch_stride(L.dinov2_hip_group_model(h, 0)))
        self.broadcast_ms = float(L.dinov2_hip_group_broadcast_ms(h))
        buf = C.create_string_buffer(8192)
        self.topology = buf.value.decode().splitlines() if L.dinov2_hip_group_describe(h, buf, len(buf)) == 0 else []

    def predict(self, images: np.ndarray, *, classify: bool = False, layout: int = RGB_CHW, topk: int = 0,
                want=("cls", "patch_tokens", "logits", "probs")) -> dict:
        img, B, hh, ww = _images(images, layout)
        out, o = _alloc_outputs(self.hparams, B, hh, ww, layout, classify, topk, want)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        _call(lib().dinov2_hip_group_predict, self._h, C.byref(i), C.byref(o), CLASSIFY if classify else 0)
        return out

    def submit(self, images: np.ndarray, *, classify: bool = False, layout: int = RGB_CHW, topk: int = 0,
               want=("cls", "patch_tokens", "logits", "probs")):
        """First half of predict (dinov2_hip_group_submit): returns a pending-job handle at once; up to `streams_per_device` jobs
        may be in flight.  `images` must not be modified until wait() has returned for the handle."""
        img, B, hh, ww = _images(images, layout)
        out, o = _alloc_outputs(self.hparams, B, hh, ww, layout, classify, topk, want)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        t = C.c_int64(-1)
        _call(lib().dinov2_hip_group_submit, self._h, C.byref(i), C.byref(o), CLASSIFY if classify else 0, C.byref(t))
        return (t.value, img, out)  # the handle keeps the input and output arrays alive

    def wait(self, handle) -> dict:
        """Second half: blocks until the job's results are in the arrays; handles are waited for in submission order."""
        _call(lib().dinov2_hip_group_wait, self._h, handle[0])
        return handle[2]


class Session(_Handle):
    """ggml_gallocr_t counterpart: stream + workspace, reusable across predicts."""
    _free = "dinov2_hip_session_free"

    def __init__(self, model: Model, stream: int | None = None):
        self.model = model
        h = C.c_void_p()
        _call(lib().dinov2_hip_session_create, model._h, C.c_void_p(stream) if stream else None, C.byref(h))
        self._h = h

    def predict(self, images: np.ndarray, *, classify: bool = False, layout: int = RGB_CHW, topk: int = 0,
                want=("cls", "patch_tokens", "logits", "probs")) -> dict:
        """images: f32 host array [B,3,H,W] (RGB_CHW) or [B,H,W,3] (BGR_HWC), or RAW uint8 [B,h,w,3] BGR with
        layout=U8_BGR_HWC (preprocessed on the device).  Returns host numpy outputs."""
        img, B, hh, ww = _images(images, layout)
        out, o = _alloc_outputs(self.model.hparams, B, hh, ww, layout, classify, topk, want)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        _call(lib().dinov2_hip_predict, self._h, C.byref(i), C.byref(o), CLASSIFY if classify else 0)
        # the resident rows a Bank may name: one CLS row per image, P patch rows per image
        nh, nw, P = _grid(self.model.hparams, hh, ww, layout, classify)
        self._last_rows = {"last_cls": B, "last_patches": P}
        self._last_grid = _grid_dims(self.model.hparams, nh, nw)  # (Session.tokencut's reshape)
        return out

    def predict_device(self, img_ptr: int, B: int, hh: int, ww: int, *, classify: bool, layout: int = RGB_CHW,
                       logits_ptr: int = 0, probs_ptr: int = 0, cls_ptr: int = 0, patch_ptr: int = 0):
        """Asynchronous predict on device-resident input/outputs (raw device pointers)."""
        i = Input(img_ptr, B, hh, ww, layout, 1)
        o = _device_output(cls_ptr, patch_ptr, logits_ptr, probs_ptr)
        _call(lib().dinov2_hip_predict, self._h, C.byref(i), C.byref(o), CLASSIFY if classify else 0)

    def predict_list(self, images, *, classify: bool = False, layout: int = RGB_CHW, topk: int = 0,
                     want=("cls", "patch_tokens", "logits", "probs")) -> dict:
        """Images of different sizes in ONE forward (dinov2_hip_predict_list): `images` = a list of f32 arrays [3, h, w] (RGB_CHW) or [h, w, 3]
        (BGR_HWC), or RAW uint8 [h, w, 3] with layout=U8_BGR_HWC.  Image i has, bit for bit, the outputs of predict() on it alone.  Returns
        cls [n, H], logits / probs [n, C], topk_* [n, topk] as predict() does, and the patch tokens three ways: "patch_packed" [offsets[n], H],
        "offsets" [n + 1], and "patch_tokens" = a list of views into the packed array, one [P_i (+ R), H] per image."""
        imgs = [np.ascontiguousarray(a, dtype=np.uint8 if layout == U8_BGR_HWC else np.float32) for a in images]
        for a in imgs:
            if a.ndim != 3 or (a.shape[0] if layout == RGB_CHW else a.shape[2]) != 3:
                raise ValueError(f"expected [3, h, w] (RGB_CHW) or [h, w, 3] images, got shape {a.shape}")
        sizes = [(a.shape[1], a.shape[2]) if layout == RGB_CHW else (a.shape[0], a.shape[1]) for a in imgs]
        il, keep = _image_list([a.ctypes.data for a in imgs], sizes, layout, 0)
        hp, n = self.model.hparams, len(imgs)
        offsets = np.zeros(n + 1, np.int64)
        _call(lib().dinov2_hip_list_rows, self.model._h, C.byref(il), CLASSIFY if classify else 0, _ptr(offsets))
        out, o = _alloc_outputs(hp, n, 0, 0, RGB_CHW, classify, topk, [k for k in want if k != "patch_tokens"])
        if "patch_tokens" in want:
            out["patch_packed"] = np.empty((int(offsets[-1]), hp.hidden_size), np.float32)
            o.patch_tokens = out["patch_packed"].ctypes.data
            out["patch_tokens"] = [out["patch_packed"][offsets[i]:offsets[i + 1]] for i in range(n)]
        out["offsets"] = offsets
        _call(lib().dinov2_hip_predict_list, self._h, C.byref(il), C.byref(o), CLASSIFY if classify else 0)
        self._last_rows = {}  # a list forward leaves nothing resident for a Bank to name
        del keep
        return out

    def predict_list_device(self, img_ptrs, sizes, *, classify: bool, layout: int = RGB_CHW, logits_ptr: int = 0, probs_ptr: int = 0,
                            cls_ptr: int = 0, patch_ptr: int = 0):
        """Asynchronous predict_list on device-resident inputs / outputs (raw device pointers): img_ptrs [n], sizes [(h, w)] as the layout
        takes them; patch_ptr receives the packed rows (list_rows gives their offsets)."""
        il, keep = _image_list(img_ptrs, sizes, layout, 1)
        o = _device_output(cls_ptr, patch_ptr, logits_ptr, probs_ptr)
        _call(lib().dinov2_hip_predict_list, self._h, C.byref(il), C.byref(o), CLASSIFY if classify else 0)
        self._last_rows = {}
        del keep

    def _layer_list(self, layers):
        """`layers` as the C-ABI wants it: ascending numbers of blocks applied; an int n = the last n layers, as upstream."""
        L = int(self.model.hparams.num_hidden_layers)
        if isinstance(layers, (int, np.integer)):
            if not 1 <= int(layers) <= L:
                raise ValueError(f"layers = {layers}: the last n layers, 1 <= n <= {L}")
            return list(range(L - int(layers) + 1, L + 1))
        return [int(v) for v in layers]

    def predict_layers(self, images: np.ndarray, layers, *, norm: bool = True, reshape: bool = False, return_class_token: bool = False,
                       return_registers: bool = False, classify: bool = False, layout: int = RGB_CHW, topk: int = 0,
                       want=("cls", "patch_tokens", "logits", "probs")) -> dict:
        """predict() plus the outputs of chosen layers from the same forward (dinov2_hip_predict_layers; upstream DINOv2's
        get_intermediate_layers).  `layers`: ascending list of layer numbers = blocks applied (0 = embeddings, L = the last block; upstream
        block index i is layer i + 1, HuggingFace hidden_states[k] is layer k), or an int n = the last n layers.  norm: through the model's
        final LayerNorm; reshape: patch tokens as [B, H, h0, w0] instead of [B, P, H].  Returns predict's dict plus "layers": one dict per
        requested layer with "layer", "patch_tokens" and, if asked for, "cls" [B, H] and "registers" [B, R, H]."""
        img, B, hh, ww = _images(images, layout)
        hp = self.model.hparams
        out, o = _alloc_outputs(hp, B, hh, ww, layout, classify, topk, want)
        ids = self._layer_list(layers)
        n, Hd, R = len(ids), hp.hidden_size, hp.num_register_tokens
        nh, nw, _ = _grid(hp, hh, ww, layout, classify)
        h0, w0 = _grid_dims(hp, nh, nw)
        arr = (C.c_int32 * max(n, 1))(*ids)
        patch = np.empty((n, B, Hd, h0, w0) if reshape else (n, B, h0 * w0, Hd), np.float32)
        cls = np.empty((n, B, Hd), np.float32) if return_class_token else None
        reg = np.empty((n, B, R, Hd), np.float32) if return_registers else None
        ly = Layers(arr, n, int(bool(norm)), LAYERS_CHW if reshape else LAYERS_TOKENS, patch.ctypes.data,
                    cls.ctypes.data if cls is not None else None, reg.ctypes.data if reg is not None else None, 0)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        _call(lib().dinov2_hip_predict_layers, self._h, C.byref(i), C.byref(o), C.byref(ly), CLASSIFY if classify else 0)
        out["layers"] = []
        for k, layer in enumerate(ids):
            d = {"layer": layer, "patch_tokens": patch[k]}
            if cls is not None:
                d["cls"] = cls[k]
            if reg is not None:
                d["registers"] = reg[k]
            out["layers"].append(d)
        return out

    def predict_layers_device(self, img_ptr: int, B: int, hh: int, ww: int, layers, *, norm: bool = True, reshape: bool = False,
                              classify: bool = False, layout: int = RGB_CHW, layer_patch_ptr: int = 0, layer_cls_ptr: int = 0,
                              layer_reg_ptr: int = 0, logits_ptr: int = 0, probs_ptr: int = 0, cls_ptr: int = 0, patch_ptr: int = 0):
        """Asynchronous predict_layers on device-resident input and outputs (raw device pointers): the tap kernel writes straight into
        layer_patch_ptr [n, B, P, H] (reshape: [n, B, H, h0, w0]), layer_cls_ptr [n, B, H] and layer_reg_ptr [n, B, R, H]."""
        ids = self._layer_list(layers)
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        ly = Layers(arr, len(ids), int(bool(norm)), LAYERS_CHW if reshape else LAYERS_TOKENS, layer_patch_ptr or None,
                    layer_cls_ptr or None, layer_reg_ptr or None, 1)
        i = Input(img_ptr, B, hh, ww, layout, 1)
        o = _device_output(cls_ptr, patch_ptr, logits_ptr, probs_ptr)
        _call(lib().dinov2_hip_predict_layers, self._h, C.byref(i), C.byref(o), C.byref(ly), CLASSIFY if classify else 0)

    def predict_dense(self, images: np.ndarray, head: "DenseHead", out_size=None, want=("labels", "value", "logits"), *, classify: bool = False,
                      layout: int = RGB_CHW, topk: int = 0, predict_want=()) -> dict:
        """One forward plus a linear dense head (dinov2_hip_predict_dense): dict of "labels" [B, oh, ow] uint8 (argmax heads), "value"
        [B, oh, ow] f32 (the winning logit, or the bins' expectation) and "logits" [B, P, C] f32, whichever of `want` the head has, plus
        "predict": predict()'s outputs named in `predict_want`, if any.  out_size: (out_h, out_w), None = the network input size."""
        img, B, hh, ww = _images(images, layout)
        hp = self.model.hparams
        nh, nw, P = _grid(hp, hh, ww, layout, classify)
        oh, ow = (nh, nw) if out_size is None else (int(out_size[0]), int(out_size[1]))
        res = {}
        if "labels" in want and head.reduce == "argmax":
            res["labels"] = np.empty((B, oh, ow), np.uint8)
        if "value" in want:
            res["value"] = np.empty((B, oh, ow), np.float32)
        if "logits" in want:
            res["logits"] = np.empty((B, P, head.num_classes), np.float32)
        ptr = lambda k: res[k].ctypes.data if k in res else None
        do = DenseOut(0 if out_size is None else oh, 0 if out_size is None else ow, ptr("labels"), ptr("value"), ptr("logits"), 0)
        out, o = _alloc_outputs(hp, B, hh, ww, layout, classify, topk, predict_want) if predict_want else ({}, None)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        _call(lib().dinov2_hip_predict_dense, self._h, C.byref(i), C.byref(o) if o is not None else None, head._h, C.byref(do),
              CLASSIFY if classify else 0)
        self._last_rows = {"last_cls": B, "last_patches": P}
        if predict_want:
            res["predict"] = out
        return res

    def predict_dense_device(self, img_ptr: int, B: int, hh: int, ww: int, head: "DenseHead", out_size=None, *, labels_ptr: int = 0,
                             value_ptr: int = 0, logits_ptr: int = 0, classify: bool = False, layout: int = RGB_CHW):
        """Asynchronous predict_dense on device-resident input and outputs (raw device pointers, 16-byte aligned): labels [B, oh, ow] uint8,
        value [B, oh, ow] f32, logits [B, P, C] f32, any of them 0."""
        oh, ow = (0, 0) if out_size is None else (int(out_size[0]), int(out_size[1]))
        do = DenseOut(oh, ow, labels_ptr or None, value_ptr or None, logits_ptr or None, 1)
        i = Input(img_ptr, B, hh, ww, layout, 1)
        _call(lib().dinov2_hip_predict_dense, self._h, C.byref(i), None, head._h, C.byref(do), CLASSIFY if classify else 0)

    def predict_dense_slide(self, images: np.ndarray, head: "DenseHead", crop, stride, want=("labels", "value", "logits"), *,
                            layout: int = RGB_CHW) -> dict:
        """Sliding-window inference with a linear dense head (dinov2_hip_predict_dense_slide) over images [B, 3, h, w] larger than the crop:
        dict of "labels" [B, h, w] uint8 (argmax heads), "value" [B, h, w] f32 and "logits" [B, windows, P, C] f32 (the low-resolution
        logits per window), whichever of `want` the head has.  crop and stride: one number or (h, w)."""
        img, B, hh, ww = _images(images, layout)
        (ch, cw), (sh, sw) = _pair(crop), _pair(stride)
        y1, x1 = self.model.slide_windows(hh, ww, (ch, cw), (sh, sw))
        h0, w0 = _grid_dims(self.model.hparams, ch, cw)
        res = {}
        if "labels" in want and head.reduce == "argmax":
            res["labels"] = np.empty((B, hh, ww), np.uint8)
        if "value" in want:
            res["value"] = np.empty((B, hh, ww), np.float32)
        if "logits" in want:
            res["logits"] = np.empty((B, len(y1) * len(x1), h0 * w0, head.num_classes), np.float32)
        ptr = lambda k: res[k].ctypes.data if k in res else None
        do = DenseOut(0, 0, ptr("labels"), ptr("value"), ptr("logits"), 0)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        sl = Slide(ch, cw, sh, sw)
        _call(lib().dinov2_hip_predict_dense_slide, self._h, C.byref(i), head._h, C.byref(sl), C.byref(do))
        self._last_rows = {}  # the session holds windows afterwards: nothing resident for a Bank to name
        return res

    def predict_dense_slide_device(self, img_ptr: int, B: int, hh: int, ww: int, head: "DenseHead", crop, stride, *, labels_ptr: int = 0,
                                   value_ptr: int = 0, logits_ptr: int = 0, layout: int = RGB_CHW):
        """Asynchronous predict_dense_slide on device-resident input and outputs (raw device pointers, the outputs 16-byte aligned): labels
        [B, h, w] uint8, value [B, h, w] f32, logits [B, windows, P, C] f32, any of them 0."""
        (ch, cw), (sh, sw) = _pair(crop), _pair(stride)
        do = DenseOut(0, 0, labels_ptr or None, value_ptr or None, logits_ptr or None, 1)
        i = Input(img_ptr, B, hh, ww, layout, 1)
        sl = Slide(ch, cw, sh, sw)
        _call(lib().dinov2_hip_predict_dense_slide, self._h, C.byref(i), head._h, C.byref(sl), C.byref(do))
        self._last_rows = {}

    def _attention_request(self, layers, queries, keys):
        """(layer ids, their C array, query ids, their C array or None, keys value) of a dinov2_hip_attention."""
        if keys not in _ATTN_KEYS:
            raise ValueError(f"keys = {keys!r}: 'all' or 'patches'")
        ids = [int(layers)] if isinstance(layers, (int, np.integer)) else [int(v) for v in layers]
        qs = [] if queries is None else [int(v) for v in queries]
        return ids, (C.c_int32 * max(len(ids), 1))(*ids), qs, ((C.c_int32 * len(qs))(*qs) if qs else None), _ATTN_KEYS[keys]

    def predict_attention(self, images: np.ndarray, layers, queries=None, keys: str = "all", taps=None, *, classify: bool = False,
                          layout: int = RGB_CHW, topk: int = 0, want=("cls", "patch_tokens", "logits", "probs"), norm: bool = True,
                          return_outputs: bool = False):
        """Softmax rows of chosen query tokens from the same forward as predict() (dinov2_hip_predict_attention; upstream DINOv2's
        get_last_selfattention, HuggingFace's output_attentions).  `layers`: ascending list of k (or one k) = the attention inside block k,
        1 .. L (HuggingFace attentions[k - 1]).  `queries`: ascending token indices (0 CLS, 1 .. R registers, then patches row-major); None: the
        CLS row.  keys: "all" (T columns) or "patches" (the P patch columns, the same bits, not re-normalised).  Returns [n, B, heads, Q, T | P]
        float32.  taps: a list of layer numbers for predict_layers' patch tokens [n_taps, B, P, H] (through the final LayerNorm if `norm`) from
        the same forward.  With taps or return_outputs the result is (rows, dict): predict's outputs, plus "layers" when taps were asked for."""
        img, B, hh, ww = _images(images, layout)
        hp = self.model.hparams
        out, o = _alloc_outputs(hp, B, hh, ww, layout, classify, topk, want)
        R, Hd = hp.num_register_tokens, hp.hidden_size
        P = _grid(hp, hh, ww, layout, classify)[2]
        ids, arr, qs, qarr, kv = self._attention_request(layers, queries, keys)
        rows = np.empty((len(ids), B, hp.num_attention_heads, max(1, len(qs)), P if kv == ATTN_KEYS_PATCHES else 1 + R + P), np.float32)
        at = Attention(arr, len(ids), qarr, len(qs), kv, rows.ctypes.data, 0)
        ly, patch = None, None
        if taps is not None:
            tids = self._layer_list(taps)
            tarr = (C.c_int32 * max(len(tids), 1))(*tids)
            patch = np.empty((len(tids), B, P, Hd), np.float32)
            ly = Layers(tarr, len(tids), int(bool(norm)), LAYERS_TOKENS, patch.ctypes.data, None, None, 0)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        _call(lib().dinov2_hip_predict_attention, self._h, C.byref(i), C.byref(o), C.byref(ly) if ly is not None else None, C.byref(at),
              CLASSIFY if classify else 0)
        if ly is not None:
            out["layers"] = [{"layer": layer, "patch_tokens": patch[k]} for k, layer in enumerate(tids)]
        return (rows, out) if (ly is not None or return_outputs) else rows

    def predict_attention_device(self, img_ptr: int, B: int, hh: int, ww: int, layers, probs: "DeviceArray", queries=None, keys: str = "all", *,
                                 classify: bool = False, layout: int = RGB_CHW, logits_ptr: int = 0, probs_ptr: int = 0, cls_ptr: int = 0,
                                 patch_ptr: int = 0):
        """Asynchronous predict_attention on device-resident input: attn_rows_kernel writes straight into `probs`, a DeviceArray (or a raw
        device pointer, 16-byte aligned) of [n, B, heads, Q, T | P] float32, on the session's stream."""
        ids, arr, qs, qarr, kv = self._attention_request(layers, queries, keys)
        at = Attention(arr, len(ids), qarr, len(qs), kv, int(getattr(probs, "ptr", probs)) or None, 1)
        i = Input(img_ptr, B, hh, ww, layout, 1)
        o = _device_output(cls_ptr, patch_ptr, logits_ptr, probs_ptr)
        _call(lib().dinov2_hip_predict_attention, self._h, C.byref(i), C.byref(o), None, C.byref(at), CLASSIFY if classify else 0)

    def debug_hidden(self, images: np.ndarray, layer: int, layout: int = RGB_CHW) -> np.ndarray:
        img, B, hh, ww = _images(images, layout, np.float32)  # (no preprocess step here: float32 whatever the layout)
        T = self.model.tokens(hh, ww)
        out = np.empty((B, T, self.model.hparams.hidden_size), np.float32)
        i = Input(img.ctypes.data, B, hh, ww, layout, 0)
        _call(lib().dinov2_hip_debug_hidden, self._h, C.byref(i), layer, out.ctypes.data)
        return out

    def pca3(self, tokens: np.ndarray | None = None, shape: tuple[int, int] | None = None):
        """Top-3 PCA of a [P, H] token matrix (cv::PCA(DATA_AS_ROW, 3) + project, inference.cpp:76-81), on the device: means,
        covariance (one MFMA GEMM), block iteration for the eigenvectors, projection.  `tokens=None` works on the patch tokens
        the last predict() left on the device (image 0; `shape` = their (P, H)) without moving them.
        Returns (components [3, H], mean [H], projection [P, 3])."""
        if tokens is None:
            P, H = shape
            ptr = None
        else:
            x = np.ascontiguousarray(tokens, dtype=np.float32)
            if x.ndim != 2:
                raise ValueError("pca3: tokens must be [P, H]")
            P, H = x.shape
            ptr = x.ctypes.data
        comp, mean, proj = np.empty((3, H), np.float32), np.empty(H, np.float32), np.empty((P, 3), np.float32)
        _call(lib().dinov2_hip_pca3, self._h, ptr, P, H, 0, comp.ctypes.data, mean.ctypes.data, proj.ctypes.data)
        return comp, mean, proj

    def match(self, a=None, b=None, *, image_a: int = 0, image_b: int = 1, shape: tuple[int, int] | None = None):
        """Nearest rows by cosine similarity in both directions (dinov2_hip_match_tokens): for every row of a [na, H] the most similar row of
        b [nb, H] and the reverse, from one pass over the similarity matrix on the device (never written, never moved).  A side left None is
        the patch tokens of image `image_a` / `image_b` of the session's last un-split predict, which stay on the device; `shape` = their
        (P, H), needed only when both sides are None.  The sides that are given are both numpy arrays or both DeviceArrays.
        Returns a dict: idx_ab, sim_ab [na], idx_ba, sim_ba [nb] and mutual [na] bool = (idx_ba[idx_ab[i]] == i)."""
        given = [x for x in (a, b) if x is not None]
        dev = [isinstance(x, DeviceArray) for x in given]
        if any(dev) and not all(dev):
            raise ValueError("match: a and b must both be host arrays or both DeviceArrays")
        on_device = bool(dev) and all(dev)
        if not on_device:
            given = [np.ascontiguousarray(x, dtype=np.float32) for x in given]
        if any(len(x.shape) != 2 for x in given):
            raise ValueError("match: a and b must be [n, H]")
        if not given and shape is None:
            raise ValueError("match: with both sides resident, give shape = (P, H) of the last predict's patch tokens")
        res = tuple(int(v) for v in shape) if shape is not None else (int(given[0].shape[0]), int(given[0].shape[1]))
        it = iter(given)
        xa = next(it) if a is not None else None
        xb = next(it) if b is not None else None
        (na, Ha), (nb, Hb) = (res if x is None else (int(x.shape[0]), int(x.shape[1])) for x in (xa, xb))
        if Ha != Hb:
            raise ValueError(f"match: a has H = {Ha}, b has H = {Hb}")
        ptr = (lambda x: None if x is None else int(x.ptr)) if on_device else (lambda x: None if x is None else x.ctypes.data)
        out = {"idx_ab": np.empty(na, np.int32), "sim_ab": np.empty(na, np.float32), "idx_ba": np.empty(nb, np.int32),
               "sim_ba": np.empty(nb, np.float32)}
        m = Match(ptr(xa), ptr(xb), na, nb, Ha, int(image_a), int(image_b), int(on_device), out["idx_ab"].ctypes.data, out["sim_ab"].ctypes.data,
                  out["idx_ba"].ctypes.data, out["sim_ba"].ctypes.data)
        _call(lib().dinov2_hip_match_tokens, self._h, C.byref(m))
        out["mutual"] = out["idx_ba"][out["idx_ab"]] == np.arange(na, dtype=np.int32)
        return out

    def _rows_request(self, who, rows, source, image, all_images, n, H):
        """(Rows struct, the array it points into: kept alive by the caller) of the rows arguments of kmeans and coreset."""
        if source is None:
            source = "given" if rows is not None else None
        if source not in _ROWS_SOURCE or (source == "given") != (rows is not None):
            raise ValueError(f"{who}: give rows, or source = 'last_cls' / 'last_patches' without rows")
        if source != "given":
            last = getattr(self, "_last_rows", {})
            if n is None:
                n = last.get(source, 0) * (last.get("last_cls", 0) if all_images else 1)
            return Rows(_ROWS_SOURCE[source], None, int(n), int(H if H is not None else self.model.hparams.hidden_size), int(image), 0), None
        if isinstance(rows, DeviceArray):
            if len(rows.shape) != 2:
                raise ValueError(f"{who}: rows must be [n, H]")
            return Rows(ROWS_GIVEN, rows.ptr, rows.shape[0], rows.shape[1], 0, 1), rows
        keep = np.ascontiguousarray(rows, dtype=np.float32)
        if keep.ndim != 2:
            raise ValueError(f"{who}: rows must be [n, H]")
        return Rows(ROWS_GIVEN, keep.ctypes.data, keep.shape[0], keep.shape[1], 0, 0), keep

    def coreset(self, rows=None, m: int | None = None, first: int = 0, stop_sim: float | None = None, *, source=None, image: int = 0,
                all_images: bool = False, bank: "Bank | None" = None, n: int | None = None, H: int | None = None) -> dict:
        """Greedy k-center (farthest-point) selection of m rows by cosine similarity on the device (dinov2_hip_coreset_tokens).  The rows
        as in kmeans(); or bank=: the rows of a Bank where they lie (Bank.keep(sess, result["idx"][:result["selected"]]) then thins it).
        first: the first pick.  stop_sim: stop once every unselected row has a pick at least this similar (None: never).
        Returns a dict: idx [m] int32 picks in selection order (-1 past `selected`), cover [m] f32 (the similarity of each pick to the picks
        before it when it was chosen; -inf for the first, +inf past `selected`), selected, nearest [n] int32 (position of each row's most
        similar pick) and near_sim [n] f32."""
        if m is None:
            raise ValueError("coreset: m, the number of rows to select, is required")
        if bank is not None:
            if rows is not None or source is not None:
                raise ValueError("coreset: give bank=, or rows / source, not both")
            r, keep, nn = Rows(), None, bank.count
        else:
            r, keep = self._rows_request("coreset", rows, source, image, all_images, n, H)
            nn = max(int(r.n), 0)
        out = _coreset_out(nn, max(int(m), 0))
        sel = C.c_int32(-1)
        c = Coreset(r, int(bool(all_images)), None if bank is None else bank._h.value, int(m), int(first), float(np.inf if stop_sim is None else stop_sim),
                    out["idx"].ctypes.data, out["cover"].ctypes.data, C.addressof(sel), out["nearest"].ctypes.data, out["near_sim"].ctypes.data)
        _call(lib().dinov2_hip_coreset_tokens, self._h, C.byref(c))
        out["selected"] = int(sel.value)
        return out

    def kmeans(self, rows=None, K: int = 8, max_iter: int = 20, init=None, seed: int = 0, *, source=None, image: int = 0,
               all_images: bool = False, n: int | None = None, H: int | None = None):
        """Spherical k-means on the device (dinov2_hip_kmeans_tokens).  rows: [n, H] host array or DeviceArray; or rows=None with
        source="last_patches" (the patch rows of image `image` of the last un-split predict, or of every image with all_images=True) or
        "last_cls"; `n` and `H` are taken from the session's last predict() unless given.  init: None (K distinct rows drawn by
        numpy.random.default_rng(seed), sorted), "maximin" (the K picks of Session.coreset from row seed % n on: with a resident source only
        K indices cross PCIe), [K] row indices or [K, H] centre vectors.  max_iter=0 only assigns.
        Returns a dict: labels [n] int32, sim [n] f32, centers [K, H] f32 (cluster sums: right direction, not unit length), counts [K],
        iterations, converged."""
        r, keep = self._rows_request("kmeans", rows, source, image, all_images, n, H)
        nn, HH, K = max(int(r.n), 0), int(r.H), int(K)
        if isinstance(init, str):
            if init != "maximin":
                raise ValueError("kmeans: init must be None, 'maximin', [K] row indices or [K, H] centre vectors")
            init = self.coreset(rows, m=K, first=int(seed) % max(nn, 1), source=source, image=image, all_images=all_images, n=n, H=H)["idx"]
        kind, cen, idx = _kmeans_init(init, nn, K, HH, seed)
        out = _kmeans_out(nn, max(K, 0), HH)
        it, conv = C.c_int32(-1), C.c_int32(-1)
        km = KMeans(r, int(bool(all_images)), K, int(max_iter), kind, None if cen is None else cen.ctypes.data,
                    None if idx is None else idx.ctypes.data, out["labels"].ctypes.data, out["sim"].ctypes.data, out["centers"].ctypes.data,
                    out["counts"].ctypes.data, C.addressof(it), C.addressof(conv))
        _call(lib().dinov2_hip_kmeans_tokens, self._h, C.byref(km))
        out.update(iterations=int(it.value), converged=bool(conv.value))
        return out

    def ncut(self, rows=None, n_eig: int = 4, affinity="threshold", tau: float = 0.2, floor: float = 1e-5, max_iter: int = 1000,
             tol: float = 1e-4, *, source=None, image: int = 0, all_images: bool = False, n: int | None = None, H: int | None = None):
        """Spectral embedding on the device (dinov2_hip_ncut_tokens): the n_eig smallest eigen-pairs of (D - W) z = lambda D z over the
        rows' affinity graph.  rows: [n, H] host array or DeviceArray; or rows=None with source="last_patches" (the patch rows of image
        `image` of the last un-split predict, or of every image with all_images=True) or "last_cls"; `n` and `H` as in Session.kmeans.
        affinity: "threshold" (w = s > tau ? 1 : floor), "relu" or "exp" (w = exp((s - 1) / tau)).
        Returns a dict: values [n_eig] ascending, vectors [n_eig, n] (unit length, largest entry positive), degree [n], residual [n_eig],
        iterations, converged."""
        if source is None:
            source = "given" if rows is not None else None
        if source not in _ROWS_SOURCE or (source == "given") != (rows is not None):
            raise ValueError("ncut: give rows, or source = 'last_cls' / 'last_patches' without rows")
        if source != "given":
            last = getattr(self, "_last_rows", {})
            if n is None:
                n = last.get(source, 0) * (last.get("last_cls", 0) if all_images else 1)
            r = Rows(_ROWS_SOURCE[source], None, int(n), int(H if H is not None else self.model.hparams.hidden_size), int(image), 0)
            keep = None
        elif isinstance(rows, DeviceArray):
            if len(rows.shape) != 2:
                raise ValueError("ncut: rows must be [n, H]")
            r, keep = Rows(ROWS_GIVEN, rows.ptr, rows.shape[0], rows.shape[1], 0, 1), rows
        else:
            keep = np.ascontiguousarray(rows, dtype=np.float32)
            if keep.ndim != 2:
                raise ValueError("ncut: rows must be [n, H]")
            r = Rows(ROWS_GIVEN, keep.ctypes.data, keep.shape[0], keep.shape[1], 0, 0)
        out = _ncut_out(r.n, n_eig)
        it, conv = C.c_int32(-1), C.c_int32(-1)
        nc = NCut(r, int(bool(all_images)), _ncut_affinity(affinity), float(tau), float(floor), int(n_eig), int(max_iter), float(tol),
                  out["values"].ctypes.data, out["vectors"].ctypes.data, out["degree"].ctypes.data, out["residual"].ctypes.data,
                  C.addressof(it), C.addressof(conv))
        _call(lib().dinov2_hip_ncut_tokens, self._h, C.byref(nc))
        del keep
        out.update(iterations=int(it.value), converged=bool(conv.value))
        return out

    def tokencut(self, image: int = 0, tau: float = 0.2, *, grid=None):
        """TokenCut on the patch tokens of image `image` of the last un-split predict: the second eigenvector of Session.ncut(affinity=
        "threshold", tau, floor=1e-5) reshaped to the patch grid (`grid`: (h0, w0), by default that of the last Session.predict), and the
        boolean mask v > mean(v) -- flipped where needed so that the foreground is the side that holds the entry of largest magnitude."""
        res = self.ncut(n_eig=2, affinity="threshold", tau=tau, floor=1e-5, source="last_patches", image=image)
        h0, w0 = grid if grid is not None else getattr(self, "_last_grid", (0, 0))
        v = res["vectors"][1]
        if h0 * w0 != v.size:
            raise ValueError(f"tokencut: the patch grid {h0} x {w0} does not hold {v.size} patches")
        return v.reshape(h0, w0), tokencut_mask(v).reshape(h0, w0)

    def vlad(self, rows=None, centers=None, *, source=None, image: int = 0, all_images: bool = False, offsets=None, intra_norm: bool = True,
             l2_norm: bool = True, want=("vlad", "counts"), n: int | None = None, H: int | None = None):
        """VLAD descriptors on the device (dinov2_hip_vlad_tokens).  rows: [n, H] host array or DeviceArray, cut into segments by offsets
        [n_seg + 1] (None: one segment); or rows=None with source="last_patches": the patch rows of image `image` of the last un-split
        predict, or one segment per image with all_images=True.  `n` and `H` (as in Session.kmeans) override the row count and width that
        are otherwise taken from the session's last predict(): needed only after a predict of another kind.
        centers: [K, H] vectors of any length, e.g. Session.kmeans(...)["centers"].  want: which of "vlad" [n_seg, K, H], "counts"
        [n_seg, K], "labels" [n], "sim" [n] to fetch.  Returns a dict of those."""
        if source is None:
            source = "given" if rows is not None else None
        if source not in _ROWS_SOURCE or (source == "given") != (rows is not None):
            raise ValueError("vlad: give rows, or source = 'last_patches' without rows")
        if centers is None:
            raise ValueError("vlad: centers are required")
        cen = np.ascontiguousarray(centers, dtype=np.float32)
        if cen.ndim != 2:
            raise ValueError("vlad: centers must be [K, H]")
        n_seg, off = 1, None
        if source != "given":
            last = getattr(self, "_last_rows", {})
            if all_images:
                n_seg = max(int(last.get("last_cls", 0)), 1)
            if n is None:
                n = last.get(source, 0) * (last.get("last_cls", 0) if all_images else 1)
            r = Rows(_ROWS_SOURCE[source], None, int(n), int(H if H is not None else self.model.hparams.hidden_size), int(image), 0)
            keep = None
            if offsets is not None:
                off = np.ascontiguousarray(offsets, np.int32)  # (the library refuses it)
        else:
            if isinstance(rows, DeviceArray):
                if len(rows.shape) != 2:
                    raise ValueError("vlad: rows must be [n, H]")
                r, keep = Rows(ROWS_GIVEN, rows.ptr, rows.shape[0], rows.shape[1], 0, 1), rows
            else:
                keep = np.ascontiguousarray(rows, dtype=np.float32)
                if keep.ndim != 2:
                    raise ValueError("vlad: rows must be [n, H]")
                r = Rows(ROWS_GIVEN, keep.ctypes.data, keep.shape[0], keep.shape[1], 0, 0)
            if offsets is not None:
                off = np.ascontiguousarray(offsets, np.int32)
                if off.ndim != 1 or len(off) < 2:
                    raise ValueError("vlad: offsets must be [n_seg + 1]")
                n_seg = len(off) - 1
        nn, HH, K = max(int(r.n), 0), int(r.H), int(cen.shape[0])
        if cen.shape[1] != HH:
            raise ValueError(f"vlad: centers are [K, {cen.shape[1]}], the rows have H = {HH}")
        unknown = set(want) - {"vlad", "counts", "labels", "sim"}
        if unknown:
            raise ValueError(f"vlad: unknown outputs {sorted(unknown)}")
        shapes = {"vlad": ((n_seg, K, HH), np.float32), "counts": ((n_seg, K), np.int32), "labels": ((nn,), np.int32), "sim": ((nn,), np.float32)}
        out = {k: np.full(shapes[k][0], -7 if shapes[k][1] is np.int32 else np.nan, shapes[k][1]) for k in shapes if k in want}
        ptr = lambda k: out[k].ctypes.data if k in out else None
        v = Vlad(r, int(bool(all_images)), None if off is None else off.ctypes.data, n_seg, K, cen.ctypes.data,
                 (VLAD_INTRA_NORM if intra_norm else 0) | (VLAD_L2_NORM if l2_norm else 0), ptr("vlad"), ptr("counts"), ptr("labels"), ptr("sim"))
        _call(lib().dinov2_hip_vlad_tokens, self._h, C.byref(v))
        return out

    def sync(self):
        lib().dinov2_hip_session_sync(self._h)

    @property
    def stream(self) -> int:
        return int(lib().dinov2_hip_session_stream(self._h) or 0)

    def profile(self, enable: bool):
        lib().dinov2_hip_session_profile(self._h, int(enable))

    def profile_read(self) -> dict:
        n = 32
        names = (C.c_char_p * n)()
        ms = (C.c_float * n)()
        cnt = (C.c_int32 * n)()
        k = lib().dinov2_hip_session_profile_read(self._h, n, names, ms, cnt)
        return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(k)}


# ------------------------------------------------------------------------------------------------
# Mirror of the reference's host API (dinov2.h)
# ------------------------------------------------------------------------------------------------
@dataclass
class dino_params:  # dinov2.h:57-68
    seed: int = 42
    topk: int = 5
    enable_flash_attn: bool = False  # accepted and ignored: attention here is always fused and exact-masked
    camera_id: int = 0
    n_threads: int = 4               # meaningless on the GPU path; kept for signature parity
    classify: bool = False
    model: str = "../ggml-model-f16.gguf"
    fname_inp: str = "../assets/tench.jpg"
    image_out: str = "pca_visual.jpg"
    eps: float = 1e-6


@dataclass
class dino_output:  # dinov2.h:85-88
    preds: list | None = None            # top-k class ids (the reference stores uint32(prob) == 0, dinov2.cpp:975)
    probs: np.ndarray | None = None      # top-k probabilities
    patch_tokens: np.ndarray | None = None  # [P, H] f32, row = y*w0 + x  (cv::Mat of dinov2.cpp:979-992)


@dataclass
class dino_model:  # dinov2.h:49-55
    hparams: HParams | None = None
    handle: Model | None = None
    session: Session | None = None
    id2label: dict = field(default_factory=dict)


def dino_model_load(img_size, fname: str, model: dino_model, params: dino_params, *, device: int = 0,
                    dtype: int = F16, patch_stride: int = 0) -> bool:
    """dinov2.h:98-99.  `img_size` is unused, as in the reference (dinov2.cpp:309-324).  Returns False and prints to
    stderr when the file cannot be opened (dinov2.cpp:269-272); other errors raise DinoError instead of asserting.
    patch_stride (no field of the reference's dino_params): Model's option of that name."""
    import sys
    try:
        model.handle = Model(fname, device=device, dtype=dtype, classify=params.classify, patch_stride=patch_stride)
    except DinoError as e:
        if e.status == 1:
            print(f"dino_model_load: failed to open '{fname}'", file=sys.stderr)
            return False
        raise
    model.hparams = model.handle.hparams
    model.session = Session(model.handle)
    if params.classify and model.hparams.has_classifier:
        model.id2label = {i: model.handle.label(i) for i in range(model.hparams.num_classes)}
    return True


def dino_predict(model: dino_model, img: np.ndarray, params: dino_params, allocr: Session | None = None):
    """dinov2.h:111-112.  `img`: preprocessed CV_32FC3-compatible array [H, W, 3], BGR interleaved (what
    dino_preprocess returns).  `allocr` plays the role of the reusable ggml_gallocr_t.  Prints the top-k lines the
    reference prints (dinov2.cpp:972-974) and returns a dino_output (None on failure, like the empty unique_ptr)."""
    sess = allocr or model.session
    try:
        r = sess.predict(img[None], classify=params.classify, layout=BGR_HWC, topk=params.topk if params.classify else 0,
                         want=("probs",) if params.classify else ("patch_tokens",))
    except DinoError as e:
        import sys
        print(f"dino_predict: {e}", file=sys.stderr)
        return None
    out = dino_output()
    if params.classify:
        ids, pr = r["topk_ids"][0], r["topk_probs"][0]
        for i, p in zip(ids, pr):
            if i >= 0:
                print(f" > {model.id2label.get(int(i), str(int(i)))} : {p:.2f}")
        out.preds, out.probs = [int(i) for i in ids if i >= 0], pr
    else:
        out.patch_tokens = r["patch_tokens"][0]
    return out
