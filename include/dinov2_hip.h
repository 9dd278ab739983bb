/*
 * dinov2_hip.h -- C-ABI of the MI355X-native DINOv2 forward (libdinov2_hip.so).
 *
 * Drop-in boundary for the hot path of lavaman131/dinov2.cpp: everything the reference does between
 * `dino_model_load` and the return of `dino_predict`.  Plain pointers and sizes only: no ggml, OpenCV,
 * torch or C++ types cross this boundary.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference repo).  Status codes, never abort/assert/throw (the reference mixes
 * bool / empty unique_ptr / assert / exceptions: dinov2.cpp:58,269-272,945-948).
 *
 * Threading: a model is immutable after load and may be shared by any number of sessions; one session
 * = one HIP stream + one workspace and is used by one host thread at a time (the role the caller-owned
 * `ggml_gallocr_t allocr` plays in dinov2.h:111-112).
 */
#ifndef DINOV2_HIP_H
#define DINOV2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DINOV2_HIP_ABI_VERSION 1

typedef struct dinov2_hip_model dinov2_hip_model;     /* replaces `struct dino_model`     dinov2.h:49-55   */
typedef struct dinov2_hip_session dinov2_hip_session; /* replaces `ggml_gallocr_t allocr` dinov2.h:111-112 */

enum dinov2_hip_status {
    DINOV2_HIP_OK = 0,
    DINOV2_HIP_ERR_IO = 1,          /* file cannot be opened / short read   (dinov2.cpp:269-272 returns false) */
    DINOV2_HIP_ERR_FORMAT = 2,      /* not GGUF, missing KV or tensor       (dinov2.cpp:58 asserts)            */
    DINOV2_HIP_ERR_UNSUPPORTED = 3, /* tensor type / shape outside the DINOv2 family                            */
    DINOV2_HIP_ERR_INVALID = 4,     /* bad argument                                                             */
    DINOV2_HIP_ERR_HIP = 5,         /* HIP runtime error (message carries hipGetErrorString)                    */
    DINOV2_HIP_ERR_NO_HEAD = 6      /* classify requested on a model loaded without a classifier                */
};

enum dinov2_hip_dtype { DINOV2_HIP_F16 = 0, DINOV2_HIP_BF16 = 1 };

/* Input image memory layouts accepted by dinov2_hip_predict. */
enum dinov2_hip_layout {
    DINOV2_HIP_BGR_HWC = 0, /* continuous CV_32FC3 cv::Mat as handed to dino_predict (dinov2.cpp:900, 914-931) */
    DINOV2_HIP_RGB_CHW = 1, /* the planar "input" tensor dino_predict uploads        (dinov2.cpp:629-631, 933) */
    DINOV2_HIP_U8_BGR_HWC = 2 /* RAW 8-bit BGR images [B, h, w, 3] as cv::imread returns them (inference.cpp:36): the library
                                 runs dino_preprocess (or dino_classify_preprocess with DINOV2_HIP_CLASSIFY) on the device
                                 first (dinov2.cpp:106-156); `data` points to uint8_t, height/width are the RAW size */
};

/* predict flags */
#define DINOV2_HIP_CLASSIFY 1u /* dino_params.classify (dinov2.h:63): run forward_head, patch view includes registers */

typedef struct dinov2_hip_load_opts {
    int32_t device;        /* HIP device ordinal (the reference picks its backend by #ifdef, dinov2.cpp:241-261)   */
    int32_t compute_dtype; /* enum dinov2_hip_dtype: MFMA input type of every weight GEMM and of attention          */
    int32_t classify;      /* dino_params.classify at load: read labels + classifier (dinov2.cpp:297-305)           */
    int32_t skip_tensor_data; /* 1: parse metadata and allocate the arena but leave it unfilled -- for ranks that
                                 receive the arena by RCCL broadcast (dinov2_hip_model_arena)                        */
    int32_t quirk_pool_const_divisor;      /* 1 (default): pooled = sum / (img_size/patch)^2  (dinov2.cpp:794,800-803) */
    int32_t quirk_pool_includes_registers; /* 1 (default): register tokens are pooled too      (dinov2.cpp:772-776)     */
    int32_t batch_invariant; /* kept for ABI compatibility; the value is ignored.  EVERY plan is batch-invariant: all kernels sum K in
                                one order, so B images == B independent forwards BIT FOR BIT, whatever the batch size, the chunking
                                of an over-long batch or the number of devices a dinov2_hip_group shards it over.  (Round 2 / early
                                round 3 had an opt-in mode, 0, that split K at tiny batches; the small-tile plans that replaced it are
                                faster than it was and keep the bits: profiles/r03_small_m_gemm.md.)                              */
    int32_t ln_fold; /* LayerNorm folded into the GEMMs on either side of it: 0 = the library's choice, 1 = on
                        (where the model allows it: hidden % 128 == 0 and <= 1 536), -1 = off: separate LayerNorm launches that round
                        f16(LN(x)) exactly where ggml does.  On: the residual epilogues emit f16(gamma x) + row statistics and the QKV /
                        FFN-in epilogues apply mean, rstd and beta -- 2 of 7 launches per layer less; the activation is rounded BEFORE the
                        normalisation instead of after it (same 2^-11 relative rounding per element; parity numbers: profiles/r06_*).      */
    int32_t patch_stride; /* pixels from one patch to the next (took reserved[0]: size and ABI version unchanged).  0 = patch_size: the
                        reference's non-overlapping patches, the same launches and bits as ever.  A smaller value s must DIVIDE patch_size
                        (patch 14: 1, 2, 7) and gives overlapping patches, the dense grids of the "deep ViT features" line of work
                        (stride 7 for patch 14): an image of h x w has h0 = (h - patch_size) / s + 1 rows of w0 = (w - patch_size) / s + 1
                        patches, the position embedding is interpolated to (h0, w0), patch_tokens row = y * w0 + x; CLS, registers, head and
                        the pooling quirks are untouched.  Inputs: h >= patch_size and (h - patch_size) % s == 0, likewise w -- every
                        multiple of patch_size passes, so dinov2_hip_preprocess_size and raw 8-bit input work as they are.  The stride is the
                        model's: one per load, not per call.  dinov2_hip_model_grid gives the grid of a size.          */
    int32_t reserved[7];
} dinov2_hip_load_opts;

/* dino_hparams (dinov2.h:25-47) plus what the loader derives from the tensor list. */
typedef struct dinov2_hip_hparams {
    uint32_t hidden_size, num_hidden_layers, num_attention_heads, num_classes;
    uint32_t num_register_tokens, patch_size, img_size, ftype;
    float eps;             /* 1e-6 (dinov2.h:33; dino_params.eps is unused by the reference) */
    uint32_t ffn_hidden;   /* fc1 rows, or weights_out columns for SwiGLU                                */
    uint32_t swiglu;       /* reference selects by num_hidden_layers == 40 (dinov2.cpp:740); here: tensor presence */
    uint32_t has_classifier;
    uint32_t weight_type;  /* ggml type id of the 2-D weights as stored in the file (1 f16, 8 q8_0, ...)  */
    uint32_t compute_dtype;
} dinov2_hip_hparams;

typedef struct dinov2_hip_input {
    const float *data; /* [batch] images, f32, already preprocessed (dino_preprocess output)               */
    int32_t batch;     /* the reference is batch 1 (dinov2.cpp:630); B images = B independent forwards     */
    int32_t height;    /* multiples of patch_size, like img.size() in dinov2.cpp:908 (patch_stride: see there) */
    int32_t width;
    int32_t layout;    /* enum dinov2_hip_layout                                                           */
    int32_t on_device; /* 0: host memory (copied H2D each call); 1: device memory on the model's device.
                          Device inputs must be COMPLETE before the call: a session created with stream = NULL runs on
                          its own non-blocking stream, which is not ordered after work the caller queued on another
                          stream (e.g. the kernel that produced the images) -- synchronise that stream first, or hand
                          the producer's stream to dinov2_hip_session_create.  Same for on_device outputs: read them
                          after dinov2_hip_session_sync (or on the session's stream).
                          HOST inputs (on_device = 0) are read ON THE SESSION'S STREAM: when the call returns asynchronously
                          -- out == NULL, or out->on_device = 1 -- the copy of `data` may still be in flight, and `data` must
                          stay valid and unchanged until dinov2_hip_session_sync or until a later call on the session that
                          returns host outputs.  That holds for pageable memory as well as for dinov2_hip_host_alloc
                          buffers (the runtime usually has staged a pageable buffer by the time the call returns; nothing
                          here promises it).  A call that returns host outputs has read its input when it returns.     */
} dinov2_hip_input;

/* Caller-allocated outputs; any pointer may be NULL.  Printing top-k stays in the caller. */
typedef struct dinov2_hip_output {
    float *cls;          /* [B, H]            "cls_token"    dinov2.cpp:764-768                                   */
    float *patch_tokens; /* [B, P, H] features; [B, R+P, H] with CLASSIFY ("patch_tokens", dinov2.cpp:770-789);
                            row = patch index y*w0+x like the cv::Mat of dinov2.cpp:979-992                        */
    float *logits;       /* [B, C]            unnamed tensor of dinov2.cpp:811-812 (CLASSIFY only)                */
    float *probs;        /* [B, C]            "probs"        dinov2.cpp:815-820  (CLASSIFY only)                  */
    int32_t *topk_ids;   /* [B, topk]         sorted descending like dinov2.cpp:961-965 (CLASSIFY only)           */
    float *topk_probs;   /* [B, topk]         (the reference's preds[] holds uint32(prob) == 0, dinov2.cpp:975)   */
    int32_t topk;        /* dino_params.topk (dinov2.h:59)                                                        */
    int32_t on_device;   /* 0: host pointers (call returns after the copy-out); 1: device pointers, async         */
} dinov2_hip_output;

/* -- load (replaces dino_model_load, dinov2.h:98-99 / dinov2.cpp:239-352) ---------------------------- */
void dinov2_hip_default_load_opts(dinov2_hip_load_opts *opts);
/* Supported geometry.  A model is either refused here with DINOV2_HIP_ERR_UNSUPPORTED and a message that names the hparam, its value and
 * the limit, or every forward entry point runs it (tests/geometry_cases.py sweeps both sides of each limit):
 *   hidden_size = 64 * num_attention_heads (head dim 64), at most 2 048 (32 heads): the LayerNorm kernels keep a row in one wave;
 *   FFN width a multiple of 64 (GELU: any such width; SwiGLU: the width of weights_out, its x1 | x2 rows interleaved in blocks of 32);
 *   patch_size 1 .. 32 (the im2col tile of ten patches of 3 p^2 elements, padded to a multiple of 64, must fit 64 KiB of LDS);
 *   patch_stride 0 (= patch_size) or a divisor of patch_size; with a stride below the patch size the pair must also pass im2col_stride_ok
 *   (csrc/kernels.h: the strided im2col keeps a strip of 3 p image rows of ten patch widths in at most 64 KiB of LDS) -- every divisor of
 *   every patch size 1 .. 32 does;
 *   img_size >= patch_size; any number of layers, register tokens and classes; 2-D weights F32 / F16 / BF16 / Q4_0 / Q4_1 / Q5_0 /
 *   Q5_1 / Q8_0 (the patch-embedding kernel F32 / F16 / BF16), every other tensor F32.
 * ln_fold applies where hidden_size % 128 == 0 and hidden_size <= 1 536; elsewhere the model runs with separate LayerNorm launches.
 * A call, not a model, is refused (DINOV2_HIP_ERR_INVALID, before anything is launched) where its network input size is off the model's
 * grid: float input whose height or width is not patch_size plus a multiple of patch_stride, and raw 8-bit input with
 * DINOV2_HIP_CLASSIFY on a model whose grid does not hold 224 x 224 -- the classify preprocessing crops to 224 x 224 whatever the patch
 * size (patch 5: refused; every divisor of 224 and every patch_stride of the published patch 14: taken).
 * What has been RUN off the four published geometries: widths 64 .. 2 048 and patch sizes 1 .. 8, 14, 16 and 32 through
 * dinov2_hip_predict (with and without ln_fold); _predict_layers, _predict_attention and _predict_dense at widths 64, 320 and 2 048, the
 * first two at patch 1 as well; dinov2_hip_predict_list / _list_rows, _match_tokens, the bank, _kmeans_tokens and _pca3 on resident rows
 * at widths 64 .. 2 048 with 1, 2, 3, 5 and 32 heads, patch sizes 1, 3, 7, 8, 14, 16 and 32, 0 .. 4 registers, f16 and bf16;
 * _predict_dense and _predict_dense_slide at patch sizes 1, 3, 8 and 16; patch_stride below patch sizes 2, 3, 4, 6, 7, 8, 16 and 32; raw
 * 8-bit input at patch sizes 5 and 16; a one-device group at patch 16 (tests/test_gpu_geometry.py,
 * tests/test_gpu_geometry_entry_points.py, tests/test_gpu_stride.py). */
int dinov2_hip_model_load(const char *gguf_path, const dinov2_hip_load_opts *opts, dinov2_hip_model **out,
                          char *err, size_t errlen);
/* replaces the caller-side frees of inference.cpp:70-73 */
void dinov2_hip_model_free(dinov2_hip_model *model);
/* replaces reads of model.hparams (dinov2.cpp:276-299) */
int dinov2_hip_model_hparams(const dinov2_hip_model *model, dinov2_hip_hparams *out);
/* The resolved dinov2_hip_load_opts.patch_stride (never 0: patch_size where the option was 0). */
int dinov2_hip_model_patch_stride(const dinov2_hip_model *model);
/* The patch grid (h0 rows of w0 patches) of a NETWORK input size h x w, or the refusal a predict of such an image would give: a size that
 * is not patch_size plus a multiple of the stride, or an image with too many token rows for one pass (rows * widest activation row * 2
 * bytes must stay below 2^31; with stride 1 a 518 x 518 image has 255 030 rows, inside the limit for ViT-L, outside it for ViT-g). */
int dinov2_hip_model_grid(const dinov2_hip_model *model, int32_t h, int32_t w, int32_t *h0, int32_t *w0, char *err, size_t errlen);
/* replaces model.hparams.id2label.at(id) (dinov2.cpp:301-305, 972); NULL when out of range */
const char *dinov2_hip_model_label(const dinov2_hip_model *model, int32_t id);
/* The packed device weight arena (one allocation, like model.buffer of dinov2.cpp:341): lets a multi-GPU
 * host broadcast rank 0's converted weights over RCCL/xGMI instead of re-reading the GGUF 8 times. */
int dinov2_hip_model_arena(dinov2_hip_model *model, void **device_ptr, size_t *bytes);

/* -- session (replaces ggml_gallocr_new / reuse across calls, inference.cpp:63, realtime.cpp:62) ---- */
/* `stream`: a hipStream_t to run on, or NULL to let the session create its own.
 * Stream contract (held by tests/test_gpu_streams.py; every wait of the session code and what it protects: DESIGN.md section 10):
 *   1. Everything a session launches or copies runs on its ONE stream, in call order: a caller's stream handed in here orders the session
 *      behind the work queued on it before a call and ahead of the work queued after it; the stream stays the caller's, and usable, after
 *      dinov2_hip_session_free.
 *   2. A call whose outputs are all on the device (on_device = 1) or absent (out == NULL) is ASYNCHRONOUS in steady state: it returns once
 *      its work is queued.  Steady state: the input shape, the list's sizes, the attention query list and the scratch sizes are those of
 *      an earlier call; a call that sees one of them for the first time may wait for the stream (it restages or reallocates), and is right
 *      either way.  Outputs of earlier asynchronous calls are never disturbed by later calls.
 *   3. A call that returns HOST outputs returns after they are complete, whatever was queued on the stream before it.
 *   4. Host INPUTS of a call that returns asynchronously: see dinov2_hip_input.on_device.
 *   5. Sessions of one model on different streams share nothing mutable: neither waits for the other. */
int dinov2_hip_session_create(dinov2_hip_model *model, void *stream, dinov2_hip_session **out, char *err,
                              size_t errlen);
void dinov2_hip_session_free(dinov2_hip_session *session);
/* Bytes of device workspace one predict of this shape needs (cf. ggml_gallocr_alloc_graph, dinov2.cpp:910); height / width: the NETWORK
 * input size.  0 for an image with too many token rows for one pass, which every predict refuses (dinov2_hip_model_grid). */
size_t dinov2_hip_workspace_bytes(const dinov2_hip_model *model, int32_t batch, int32_t height, int32_t width);
/* Blocks until everything enqueued on the session's stream has finished (ggml_backend_synchronize,
 * inference.cpp:66). */
int dinov2_hip_session_sync(dinov2_hip_session *session);
void *dinov2_hip_session_stream(dinov2_hip_session *session);

/* -- predict (replaces dino_predict, dinov2.h:111-112 / dinov2.cpp:900-999) -------------------------- */
int dinov2_hip_predict(dinov2_hip_session *session, const dinov2_hip_input *in, dinov2_hip_output *out,
                       uint32_t flags, char *err, size_t errlen);

/* -- predict + intermediate layers (no reference counterpart: the backbone use of DINOv2 -- DPT / linear decoders read four intermediate
 *    blocks, the linear-probe recipe the CLS tokens of the last four; upstream DINOv2: get_intermediate_layers(x, n, reshape,
 *    return_class_token, norm), HuggingFace: output_hidden_states).  ONE ordinary forward; each requested layer costs one more kernel launch
 *    (layer_tap_kernel, csrc/kernels_misc.hip), which reads the f32 residual stream as it stands after that layer and writes the rows asked for.
 *    Index convention -- `layers[i]` is the NUMBER OF BLOCKS APPLIED:
 *        this library (and dinov2_hip_debug_hidden)   HuggingFace                 upstream DINOv2
 *        0                                            hidden_states[0]            (embeddings; no block index)
 *        k, 1 <= k <= L                               hidden_states[k]            get_intermediate_layers(n = [k - 1])
 *    so the usual ViT-L taps, upstream blocks 4, 11, 17, 23, are layers 5, 12, 18, 24. */
enum dinov2_hip_layers_layout { DINOV2_HIP_LAYERS_TOKENS = 0, DINOV2_HIP_LAYERS_CHW = 1 };

typedef struct dinov2_hip_layers {
    const int32_t *layers; /* [n_layers], strictly ascending, each in [0, L] (table above)                                              */
    int32_t n_layers;      /* 1 .. L + 1                                                                                               */
    int32_t norm;          /* 1: the model's FINAL LayerNorm (ln_w, ln_b, eps) applied to the tapped rows -- norm = True upstream -- with the
                              bits dinov2_hip_predict's own final LayerNorm gives (layer L, norm 1 IS predict's cls / patch_tokens);
                              0: the raw f32 residual stream                                                                           */
    int32_t layout;        /* of patch_tokens only: TOKENS [n, B, P, H];  CHW [n, B, H, h0, w0] (reshape = True upstream): element
                              (c, y, x) = channel c of patch y*w0 + x -- the same bits, permuted                                       */
    float *patch_tokens;   /* patch rows only (CLS and registers stripped, with or without DINOV2_HIP_CLASSIFY); any of the three
                              pointers may be NULL                                                                                     */
    float *cls;            /* [n, B, H]                                                                                                */
    float *registers;      /* [n, B, R, H] (DINOV2_HIP_ERR_INVALID if non-NULL on a model without registers)                            */
    int32_t on_device;     /* 0: host pointers (the call returns after the copy-out; staged through a session-owned device buffer);
                              1: device pointers, 16-byte aligned, written by the kernel itself, asynchronously on the session's stream */
    int32_t reserved[4];
} dinov2_hip_layers;

/* `out` (may be NULL) and `flags` as for dinov2_hip_predict: one call returns logits and taps.  Argument errors (NULL `layers` or list,
 * n_layers or a layer out of range, a list not strictly ascending, an unknown layout, registers from a register-free model, a device
 * pointer that is not 16-byte aligned), like those of dinov2_hip_predict itself, return their status before anything is launched,
 * allocated or copied.  Batches that dinov2_hip_predict splits into passes are split here too,
 * every pass writing its images at their offset.  Afterwards dinov2_hip_fetch and dinov2_hip_pca3(tokens = NULL) behave as after a
 * dinov2_hip_predict of the same shape.  Runs eagerly under DINOV2_HIP_GRAPHS=1 (the graph cache is not keyed by the caller's pointers). */
int dinov2_hip_predict_layers(dinov2_hip_session *session, const dinov2_hip_input *in, dinov2_hip_output *out,
                              const dinov2_hip_layers *layers, uint32_t flags, char *err, size_t errlen);

/* -- predict + attention rows (no reference counterpart: the CLS-to-patch maps of the last block are the model's signature visualisation,
 *    register papers plot what registers and patches give each other, token-pruning code reads CLS rows of several blocks; upstream DINOv2:
 *    get_last_selfattention, HuggingFace: output_attentions).  ONE ordinary forward -- the attention kernels of the forward are the same and
 *    keep their probabilities in registers; each requested block costs one more kernel launch (attn_rows_kernel, csrc/attn_rows.hip) right
 *    after that block's QKV GEMM, which reads the q of the chosen query tokens and every k from the qkv buffer and writes
 *        probs[l][b][head][i][j] = exp2(s_ij - m_i) / sum_{j' < T} exp2(s_ij'  - m_i),   s_ij = q[queries[i]] . k[j],  m_i = max_j s_ij
 *    (q carries 0.125 log2(e): this is softmax(q k^T / 8)).  Index convention -- `layers[i]` = k is the attention INSIDE block k, the numbering
 *    of dinov2_hip_predict_layers (number of blocks applied):
 *        this library        HuggingFace              upstream DINOv2
 *        k, 1 <= k <= L      attentions[k - 1]        blocks[k - 1].attn;  k = L: get_last_selfattention
 *    (there is no layer 0: no attention runs before block 1).  Token indices: 0 CLS, 1 .. R registers, 1 + R + y*w0 + x patches.
 *    Contract: the stored f16 / bf16 q and k are the operands (their products are exact in f32); scores, maximum, exponentials, sum,
 *    reciprocal and product are f32, in summation orders that depend on nothing but T -- so a row is bit-identical whether it is asked for
 *    alone or with every other token, in a batch of 1 or of 32, whole or split into passes, and whichever columns are kept.  These are NOT
 *    the bits of the P the flash-style attention kernel feeds its PV product (un-normalised, rounded to the compute type, under a deferred
 *    maximum): they are the f32 softmax of the same stored q and k.
 *    Cost: per requested block one read of that block's K (B T H 2 bytes) per 8 queries or part thereof, e.g. the CLS rows of
 *    all 24 blocks of ViT-L at 518 px; a full T x T map is T / 8 such reads (profiles/attention_rows.md).  In dinov2_hip_session_profile the
 *    launches are booked under "layer_tap" (a tap of the attention): that kind reads taps + attention layers.
 *    Out of scope: the device group (dinov2_hip_group_*) has no such call. */
enum dinov2_hip_attention_keys { DINOV2_HIP_ATTN_KEYS_ALL = 0, DINOV2_HIP_ATTN_KEYS_PATCHES = 1 };

typedef struct dinov2_hip_attention {
    const int32_t *layers;  /* [n_layers] strictly ascending, each in [1, L]: the attention INSIDE block k -- the index convention
                               of dinov2_hip_predict_layers (number of blocks applied), HuggingFace attentions[k - 1],
                               upstream blocks[k - 1]; L = get_last_selfattention */
    int32_t n_layers;       /* 1 .. L */
    const int32_t *queries; /* [n_queries] token indices, strictly ascending, in [0, T): 0 CLS, 1 .. R registers, 1 + R + y*w0 + x patches.
                               NULL with n_queries == 0: the CLS row alone */
    int32_t n_queries;      /* 0 (CLS) or 1 .. T */
    int32_t keys;           /* ALL: rows of T columns; PATCHES: the P = h0*w0 patch columns only (same bits, not re-normalised) */
    float *probs;           /* [n_layers, B, heads, Q, T or P], Q = max(1, n_queries) */
    int32_t on_device;      /* as in dinov2_hip_layers: 0 host (staged through a session-owned device buffer, one stream wait),
                               1 device pointer, 16-byte aligned, written by the kernel itself, asynchronously on the session's stream */
    int32_t reserved[4];
} dinov2_hip_attention;

/* `out` (may be NULL) and `flags` as for dinov2_hip_predict; `taps` (may be NULL) as for dinov2_hip_predict_layers: one call returns logits,
 * layer taps and attention rows of the same forward.  Argument errors (NULL `attn`, layer list or probs; n_layers or a layer out of range,
 * layer 0 among them; a layer or query list not strictly ascending; a query >= T for this input's shape; an unknown `keys`; a device pointer
 * that is not 16-byte aligned; those of `taps` and of dinov2_hip_predict) return their status before anything is launched, allocated or
 * copied.  Split batches, dinov2_hip_fetch, dinov2_hip_pca3(tokens = NULL) and DINOV2_HIP_GRAPHS=1 as for dinov2_hip_predict_layers.  The
 * query list is kept on the device from call to call; a call with another list waits for the session's stream first. */
int dinov2_hip_predict_attention(dinov2_hip_session *session, const dinov2_hip_input *in, dinov2_hip_output *out,
                                 const dinov2_hip_layers *taps /* may be NULL */, const dinov2_hip_attention *attn,
                                 uint32_t flags, char *err, size_t errlen);

/* Copy-out half of dinov2_hip_predict on its own: the outputs of the session's LAST predict (which may have been called with
 * out = NULL, i.e. forward only) into the caller's buffers.  Lets a host overlap the device -> host copy of batch k with the
 * forward of batch k + 1 on another session (this is what the group's lanes do).  Not available after a predict that had to
 * split an over-long batch into passes. */
int dinov2_hip_fetch(dinov2_hip_session *session, dinov2_hip_output *out, char *err, size_t errlen);

/* -- predict over a list of images of different sizes (no reference counterpart: dino_preprocess resizes every image to (dim / patch + 1) patch
 *    per side, so the network size follows the raw image, and a folder of photographs, a set of crops or the levels of a pyramid is a list of
 *    different sizes -- each its own batch-1 forward through dinov2_hip_predict.  Upstream DINOv2: forward_features_list with a block-diagonal
 *    attention mask).  ONE forward: the token rows of all images stand one after the other in the residual stream (M = sum T_i rows); the patch
 *    embedding and the head run once per run of consecutive images of one size, every per-row kernel (LayerNorm, the four GEMMs of a block)
 *    runs once over the M rows, and attention runs once per block over a work table of {first row, length, head, query block} -- the list
 *    form of the two attention kernels (csrc/attention.hip, launch_attention_list), which never stages a key of a neighbouring image.
 *    Contract: image i of a list has, BIT FOR BIT, the outputs dinov2_hip_predict gives for that image alone (every kernel plan is
 *    batch-invariant, and the order of the list and of the work table changes nothing).
 *    Outputs: the ordinary dinov2_hip_output with B = n -- cls [n, H], logits / probs [n, C], topk_* [n, topk] -- and patch_tokens PACKED,
 *    [offsets[n], H]: image i owns rows offsets[i] .. offsets[i + 1] (dinov2_hip_list_rows), P_i of them, or R + P_i with DINOV2_HIP_CLASSIFY,
 *    in dinov2_hip_predict's row order.  Host and device outputs as in dinov2_hip_predict.
 *    The position embeddings of up to DINOV2_HIP_LIST_POS_GRIDS distinct patch grids ((1 + P) H floats each: 5.6 MB for ViT-L at 518 px) stay on the device from call to call; a list that would
 *    take the cache past that clears it first (a single list may hold more distinct grids than that: it is served, and evicts the rest).
 *    Argument errors -- n <= 0, a NULL array or image pointer, a size dinov2_hip_predict would refuse for that image, classify without a
 *    head, device top-k, a list with too many rows for one pass -- return their status, naming the image, before anything is allocated, copied
 *    or launched.
 *    Afterwards there is no "last un-split forward": until the next dinov2_hip_predict, dinov2_hip_fetch, dinov2_hip_pca3(tokens = NULL),
 *    dinov2_hip_match_tokens on resident tokens and the bank's LAST_CLS / LAST_PATCHES are refused as they are before the first predict.
 *    Out of scope: lists longer than one pass (rows * max(3 H, ffn, patch K) * 2 >= 2^31 bytes: refused, not split); layer taps, attention
 *    rows and dense heads on a list; the device group; graph capture (a list call runs eagerly); masks (upstream's masks_list); list forms
 *    of the attention variants that are never auto-selected (DINOV2_HIP_ATTN_V=3|4 make the call fail; DINOV2_HIP_ATTN_NWV is not looked at).
 *    Times against batch-1 calls: profiles/predict_list.md. */
#define DINOV2_HIP_LIST_POS_GRIDS 64
typedef struct dinov2_hip_image_list {
    const void *const *data; /* [n] one pointer per image: f32, or uint8_t for DINOV2_HIP_U8_BGR_HWC                                  */
    const int32_t *height;   /* [n] as dinov2_hip_input.height: the network size, or the RAW size for DINOV2_HIP_U8_BGR_HWC (each image
                                is then preprocessed on the device to its own network size)                                           */
    const int32_t *width;    /* [n]                                                                                                   */
    int32_t n;               /* >= 1                                                                                                  */
    int32_t layout;          /* enum dinov2_hip_layout, one for the whole list                                                        */
    int32_t on_device;       /* as dinov2_hip_input.on_device, one for the whole list.  Device images of equal size that already stand
                                one after the other in memory are read in place; others are gathered with device copies              */
} dinov2_hip_image_list;
/* rows of out->patch_tokens that image i occupies: offsets[i] .. offsets[i + 1]; offsets has n + 1 entries.  Needs no device; `data` may be NULL. */
int dinov2_hip_list_rows(const dinov2_hip_model *model, const dinov2_hip_image_list *list, uint32_t flags, int64_t *offsets, char *err,
                         size_t errlen);
int dinov2_hip_predict_list(dinov2_hip_session *session, const dinov2_hip_image_list *list, dinov2_hip_output *out, uint32_t flags,
                            char *err, size_t errlen);

/* -- multi-device group (no reference counterpart: the reference is one backend, batch 1) -----------------
 *    Host threads + sessions per device inside the library; dinov2_hip_group_predict splits the caller's global batch
 *    contiguously (device g owns images [g*B/G, (g+1)*B/G), remainder to the low ranks) and every device writes its results
 *    into the caller's HOST buffers at its shard offset.  Images are independent forwards: no data-path collective.  With
 *    `broadcast` = 1 (default) only device 0 parses / dequantises the GGUF; the packed weight arena reaches the others by ONE
 *    RCCL broadcast over xGMI (single-process ncclCommInitAll + ncclBroadcast; librccl is dlopen'ed on first use).  A device
 *    list that names a device twice (two sessions on one GPU) makes every entry read the file itself. */
typedef struct dinov2_hip_group dinov2_hip_group;
typedef struct dinov2_hip_group_opts {
    dinov2_hip_load_opts load; /* compute dtype, classify, quirks; `device` and `skip_tensor_data` are set per rank          */
    int32_t n_devices;         /* 0: every visible device                                                                     */
    const int32_t *devices;    /* [n_devices] HIP ordinals, or NULL for 0 .. n_devices-1                                      */
    int32_t broadcast;         /* 1: rank 0 loads, RCCL broadcast of the arena; 0: every rank loads the file                  */
    int32_t streams_per_device; /* lanes (host thread + stream + workspace) per device, 1..4; default 2 = the number of jobs
                                   dinov2_hip_group_submit accepts before one must be waited for.  Results do not depend on it.
                                   A lane allocates its workspace (dinov2_hip_workspace_bytes of its shard) and input staging buffer
                                   when it first runs a job; a job goes to the lowest lane with nothing in flight, so callers of
                                   dinov2_hip_group_predict alone (one job in flight) only ever pay for lane 0.                    */
    int32_t reserved[7];
} dinov2_hip_group_opts;
void dinov2_hip_default_group_opts(dinov2_hip_group_opts *opts);
int dinov2_hip_group_create(const char *gguf_path, const dinov2_hip_group_opts *opts, dinov2_hip_group **out, char *err,
                            size_t errlen);
void dinov2_hip_group_free(dinov2_hip_group *group);
int dinov2_hip_group_size(const dinov2_hip_group *group);
/* the model of one rank (hparams / labels are the same on every rank); owned by the group */
dinov2_hip_model *dinov2_hip_group_model(dinov2_hip_group *group, int32_t rank);
/* wall time of the load-time arena broadcast in ms; negative when every rank read the file itself */
double dinov2_hip_group_broadcast_ms(const dinov2_hip_group *group);
/* Where the group's devices sit: one text line per device -- ordinal, PCI bus id, NUMA node, local CPUs (its worker threads are bound
 * to them; DINOV2_HIP_GROUP_NO_AFFINITY=1 turns that off), peer-to-peer reachability of the group's other devices (y / n), and whether
 * its weights came from the file or from the RCCL broadcast (a broadcast that cannot be set up degrades to file reads with a line on
 * stderr; DINOV2_HIP_GROUP_REQUIRE_RCCL=1 makes it an error instead). */
int dinov2_hip_group_describe(const dinov2_hip_group *group, char *out, size_t cap);
/* dino_predict over the whole group: host input [B, ...] (any dinov2_hip_layout), host outputs [B, ...]; returns when every
 * shard has landed.  B < G leaves the high ranks idle.  One call at a time per group; refused (DINOV2_HIP_ERR_INVALID, nothing
 * queued) while a ticket of dinov2_hip_group_submit has not been waited for.  Layout / height / width are checked before
 * anything is copied. */
int dinov2_hip_group_predict(dinov2_hip_group *group, const dinov2_hip_input *in, dinov2_hip_output *out, uint32_t flags,
                             char *err, size_t errlen);
/* The same call in two halves, so that ONE host thread can keep up to `streams_per_device` batches in flight: while a device
 * computes batch k, its other lane copies batch k + 1 in and batch k - 1 out (host -> device copy, forward and device -> host
 * copy are separate turnstiles per device, each passed in submission order).  `in` / `out` are copied; the buffers they point
 * to must stay valid (and unread) until the ticket has been waited for.  Tickets are waited for in submission order.  Results
 * are bit-identical to dinov2_hip_group_predict's.  Page-locked buffers (dinov2_hip_host_alloc) make the copies faster but are
 * not required. */
int dinov2_hip_group_submit(dinov2_hip_group *group, const dinov2_hip_input *in, const dinov2_hip_output *out, uint32_t flags,
                            int64_t *ticket, char *err, size_t errlen);
int dinov2_hip_group_wait(dinov2_hip_group *group, int64_t ticket, char *err, size_t errlen);

/* Page-locked host memory for images / results handed to dinov2_hip_predict or dinov2_hip_group_predict: copies to and from
 * such buffers run at the full PCIe rate and truly asynchronously (pageable memory is staged through bounce buffers by the
 * runtime, at roughly half the rate, and a copy into or out of it is usually finished when the copy call returns).  Plain malloc'ed
 * buffers remain valid inputs.  With a page-locked INPUT an asynchronous call really returns while the copy is in flight: leave the buffer
 * alone until dinov2_hip_session_sync (dinov2_hip_input.on_device).  NULL on failure. */
void *dinov2_hip_host_alloc(size_t bytes);
void dinov2_hip_host_free(void *ptr);

/* -- preprocessing (replaces dino_preprocess / dino_classify_preprocess, dinov2.h:93-96,
 *    dinov2.cpp:106-156, without OpenCV).  mode 0: resize to ((w/p)+1)*p x ((h/p)+1)*p; mode 1: resize to 256x256 ignoring
 *    aspect, centre-crop 224.  Input 8-bit BGR interleaved [h, w, 3]; output continuous f32 BGR [out_h, out_w, 3], /255,
 *    bicubic (cv::INTER_CUBIC), (c - mean) / std with the reference's BGR<->mean indexing.  Host implementation; the same
 *    arithmetic runs on the device for DINOV2_HIP_U8_BGR_HWC inputs. */
int dinov2_hip_preprocess_size(int32_t mode, int32_t height, int32_t width, int32_t patch, int32_t *out_h, int32_t *out_w);
int dinov2_hip_preprocess(int32_t mode, const uint8_t *bgr, int32_t height, int32_t width, int32_t patch, float *out);

/* -- feature post-processing (replaces cv::PCA(tokens, noArray(), DATA_AS_ROW, 3) + project of
 *    inference.cpp:76-81).  tokens: [P, H] f32 (P >= 4, 8 <= H <= 4096, |x| within the f16 range), a host pointer, a device
 *    pointer (on_device = 1), or NULL = the patch tokens of image 0 that the session's last dinov2_hip_predict left on the
 *    device (P and H must be theirs) -- the realtime loop's case: nothing but the [P, 3] projection crosses PCIe.
 *    On the device: column means, the H x H covariance (one MFMA GEMM of the centred, transposed f16 tokens with themselves),
 *    a block iteration (8 vectors, CholeskyQR, one launch per step) for the leading eigenvectors, and the projection; on the
 *    host only the 8 x 8 Rayleigh-Ritz problem.  Deterministic.  Outputs (host, any may be NULL): components [3, H] unit
 *    vectors sorted by variance, each oriented so that its largest loading is positive; mean [H]; projection [P, 3] =
 *    (tokens - mean) components^T. */
int dinov2_hip_pca3(dinov2_hip_session *session, const float *tokens, int32_t P, int32_t H, int32_t on_device,
                    float *components, float *mean, float *projection, char *err, size_t errlen);

/* -- dense correspondence (no reference counterpart: for every patch of image A the most similar patch of image B by cosine similarity, the
 *    reverse, and the mutual nearest neighbours kept -- the matching figure of the DINOv2 paper, the "sparse matching" notebooks built on
 *    upstream's get_intermediate_layers / x_norm_patchtokens; with CLS vectors as rows the same call is retrieval / k-NN with k = 1).  Either
 *    side is a caller's [n, H] f32 matrix (host or device) or, with a NULL pointer, the PATCH tokens of one image of the session's last
 *    un-split forward, which never leave the device: only the two index / similarity vectors cross PCIe.  On the device (csrc/match.hip): rows
 *    to unit length in f16, one pass over the 128 x 128 tiles of the na x nb similarity matrix on the matrix cores -- the matrix is never
 *    written; each tile's epilogue reduces its accumulators per row and per column -- and a fold of the per-tile partials.
 *    Contract:
 *    1. Normalisation.  Per row ss = sum x^2 in f32, r = 1.0f / sqrtf(ss) with a correctly rounded square root and division, x^ = f16(x r);
 *       a row with ss == 0 gives x^ = 0, so all its similarities are 0.  The operands are f16 whatever the model's compute type (like the
 *       covariance GEMM of dinov2_hip_pca3).  Inputs must be finite; the result for non-finite input is unspecified.
 *    2. Similarity.  sim(i, j) = sum_k a^_ik b^_jk: the f16 products are exact in f32, the accumulation is f32 on the matrix cores in an order
 *       that depends on H alone -- not on na, nb or the tile a pair falls in -- so sim_ab[i] is bit-identical whatever other rows travel
 *       with row i.
 *    3. Argmax over the real rows and columns only (padding never wins); equal f32 values (-0 and +0 are equal) go to the LOWEST index; the
 *       result depends neither on launch geometry nor on the order in which tiles finish.
 *    4. Both directions come from the SAME products, so sim_ab[i] == sim_ba[idx_ab[i]] bit for bit whenever the pair is mutual
 *       (idx_ba[idx_ab[i]] == i).
 *    Out of scope: k > 1 and ratio tests, a persistent normalised bank (both: dinov2_hip_bank_topk below), the device group, device-side
 *    outputs, bf16 operands.
 *    Times against the vendor GEMM + max: profiles/match.md. */
typedef struct dinov2_hip_match {
    const float *a;    /* [na, H] f32, or NULL = the PATCH tokens (rows 1 + R .. T - 1 of the final-LayerNorm tokens: never CLS or registers,
                          with or without DINOV2_HIP_CLASSIFY) of image `image_a` of the session's last un-split forward; then na must be P */
    const float *b;    /* [nb, H], or NULL likewise with `image_b` (a and b may name the same or different images, or one of them a
                          caller's buffer: matching the live frame against a stored template) */
    int32_t na, nb;    /* 1 .. 1 048 576 each */
    int32_t H;         /* 8 .. 4096; with a NULL side it must be the model's hidden size */
    int32_t image_a, image_b; /* in [0, last batch); read only for a NULL side */
    int32_t on_device; /* of the non-NULL a / b: 0 host, 1 device pointers (16-byte aligned) on the model's device */
    int32_t *idx_ab;   /* [na] argmax_j sim(a_i, b_j); HOST; any of the four may be NULL, not all */
    float   *sim_ab;   /* [na] that similarity */
    int32_t *idx_ba;   /* [nb] argmax_i sim(a_i, b_j) */
    float   *sim_ba;   /* [nb] */
    int32_t reserved[4];
} dinov2_hip_match;
/* Synchronous: returns after the copy-out, like dinov2_hip_pca3.  Argument errors (NULL session or `m`; na, nb or H out of range; all four
 * outputs NULL; a NULL side when the session holds no un-split forward -- none yet, or the last predict was split into passes; na / nb / H
 * that are not P / P / the hidden size for a NULL side; an image index outside the last batch; a device pointer that is not 16-byte aligned)
 * return DINOV2_HIP_ERR_INVALID before anything is launched, allocated or copied.  The scratch (the two f16 operands, (na + nb) rounded up to
 * tiles x H rounded up to 64 x 2 bytes, a host side's staging copy, at most 32 MiB of partials, the results) is a session-owned buffer
 * grown on demand; an allocation the device refuses returns DINOV2_HIP_ERR_HIP. */
int dinov2_hip_match_tokens(dinov2_hip_session *session, const dinov2_hip_match *m, char *err, size_t errlen);

/* -- a resident feature bank with top-k cosine search (no reference counterpart: k-NN classification -- the evaluation protocol of the
 *    DINOv2 paper, k = 10, 20, ... with votes weighted by exp(sim / 0.07) --, retrieval against a gallery, Lowe's ratio test (k = 2), template
 *    memories for the realtime loop).  The other half of dinov2_hip_match_tokens: the gallery is normalised ONCE into a device-resident f16
 *    bank, and every query batch gets its k best rows back; only the queries (unless they are resident too) and [nq, k] results cross PCIe.
 *    The bank is one device allocation on the model's device, made at create and never moved: f16 rows [capacity rounded up to the 128-row
 *    tile, H rounded up to 64], zeroed at create.  It keeps only the device ordinal, so it may outlive the model; a session of another device
 *    is refused.  One host thread at a time uses a bank.  On the device (csrc/bank.hip): dinov2_hip_match's normalisation kernel, then
 *    workgroups that each sweep one chunk of the bank's 128-column tiles for one 128-row tile of queries on the matrix cores, keeping a sorted
 *    list of k (value, index) pairs per query row in LDS, and a merge of the chunk lists.  The similarity matrix is never written.
 *    Contract:
 *    1. Normalisation.  Contract 1 of dinov2_hip_match, word for word: per row ss = sum x^2 in f32 in the same order, r = 1.0f / sqrtf(ss)
 *       with a correctly rounded square root and division, x^ = f16(x r); a row with ss == 0 gives x^ = 0, so all its similarities are 0.
 *       It is the same kernel.  Inputs must be finite.
 *    2. Similarity.  Contract 2 of dinov2_hip_match: the same MFMA shape with k-steps of 32 in ascending order, an order that depends on H
 *       alone.  Hence sim[i][0] and idx[i][0] equal sim_ab[i] and idx_ab[i] of dinov2_hip_match_tokens on the same rows bit for bit, and a
 *       row's result is independent of the queries that travel with it.
 *    3. Order.  One strict total order: the larger f32 value first (-0 is read as +0), among equal values the LOWEST index.  Row i of the
 *       result is the first k of the bank's `count` rows in that order, best first.  Indices are distinct, so this list is unique: it does not
 *       depend on launch geometry, on the chunking of the bank, on the insertion or merge order, or on which rows were added in which call.
 *       The index is the insertion index (what dinov2_hip_bank_add reported as `first`, counting on).  Rows past `count` never win: the sweep
 *       masks on count and assumes nothing about the memory behind it (dinov2_hip_bank_clear does not touch it).
 *    4. Short banks.  When k > count, slots count .. k - 1 hold idx = -1 and sim = -INFINITY.
 *    Out of scope: weighted voting -- a caller writes it from idx, sim and its own label array:
 *        for (j = 0; j < k && idx[i * k + j] >= 0; ++j)
 *            votes[label[idx[i * k + j]]] += expf(sim[i * k + j] / 0.07f);
 *        predicted[i] = argmax(votes);
 *    -- removal of rows other than by keeping an ascending subset (dinov2_hip_bank_keep below; dinov2_hip_coreset_tokens chooses one), bf16
 *    operands, the device group, device-side outputs, k > 64.
 *    Times: profiles/bank_topk.md. */
typedef struct dinov2_hip_bank dinov2_hip_bank;

enum dinov2_hip_rows_source { DINOV2_HIP_ROWS_GIVEN = 0, DINOV2_HIP_ROWS_LAST_CLS = 1, DINOV2_HIP_ROWS_LAST_PATCHES = 2 };
typedef struct dinov2_hip_rows {
    int32_t source;     /* GIVEN: `data` is [n, H] f32.  LAST_CLS: the final-LayerNorm CLS row of every image of the session's last
                           un-split forward (n must be that batch).  LAST_PATCHES: the patch rows 1 + R .. T - 1 of image `image`
                           (n must be P) -- the rows a NULL side of dinov2_hip_match stands for.  Resident rows never leave the device. */
    const float *data;  /* GIVEN only; host, or device (16-byte aligned) with on_device = 1 */
    int32_t n, H, image, on_device;
    int32_t reserved[4];
} dinov2_hip_rows;

/* 8 <= H <= 4096, 1 <= capacity <= 2^24 (16 777 216) rows, else DINOV2_HIP_ERR_INVALID.  An allocation the device refuses returns
 * DINOV2_HIP_ERR_HIP and leaves nothing behind for the next launch to report. */
int  dinov2_hip_bank_create(dinov2_hip_model *model, int32_t H, int32_t capacity, dinov2_hip_bank **out, char *err, size_t errlen);
/* waits for the device first: a session's stream may still be reading the rows */
void dinov2_hip_bank_free(dinov2_hip_bank *bank);
/* rows added since create / the last clear (0 for NULL) */
int  dinov2_hip_bank_count(const dinov2_hip_bank *bank);
/* count = 0; the memory is not touched */
int  dinov2_hip_bank_clear(dinov2_hip_bank *bank);
/* Normalises `rows` into rows [count, count + n) of the bank, reports *first = the old count (first may be NULL) and returns after the
 * stream has finished: a returned bank is always complete.  More rows than fit returns DINOV2_HIP_ERR_INVALID and changes nothing.
 * Argument errors (NULLs; n out of range; H unequal to the bank's; a resident source when the session holds no un-split forward -- none
 * yet, or the last predict was split into passes; n that is not the batch (LAST_CLS) or P (LAST_PATCHES); an image index outside the last
 * batch; an unknown source; a misaligned device pointer; a session of another device) return DINOV2_HIP_ERR_INVALID before anything is
 * launched, allocated or copied, with *first and the bank untouched.  Host rows are staged in a session-owned scratch grown on demand. */
int  dinov2_hip_bank_add(dinov2_hip_session *s, dinov2_hip_bank *bank, const dinov2_hip_rows *rows, int32_t *first, char *err, size_t errlen);

typedef struct dinov2_hip_topk {
    dinov2_hip_rows queries; /* 1 .. 1 048 576 rows */
    int32_t k;          /* 1 .. 64 */
    int32_t *idx;       /* [nq, k] HOST; either may be NULL, not both */
    float   *sim;       /* [nq, k] HOST */
    int32_t reserved[4];
} dinov2_hip_topk;
/* Synchronous: returns after the copy-out.  Argument errors (those of dinov2_hip_bank_add for `queries`; k out of range; both outputs NULL;
 * an empty bank) return DINOV2_HIP_ERR_INVALID before anything is launched, allocated or copied, with the outputs untouched.  The scratch
 * (the f16 queries, host queries' staging copy, the partial lists, the results) is the same session-owned buffer; the queries are walked
 * in passes of at most 4 096 and the bank in at most as many chunks that the partial lists of one pass stay within 32 MiB whatever nq,
 * count and k.  An allocation the device refuses returns DINOV2_HIP_ERR_HIP. */
int  dinov2_hip_bank_topk(dinov2_hip_session *s, const dinov2_hip_bank *bank, const dinov2_hip_topk *q, char *err, size_t errlen);
/* Compacts the bank to rows idx[0 .. m) in that order: idx (HOST) strictly ascending, each in [0, count), 1 <= m <= count.  New row j is old
 * row idx[j], bit for bit; count = m; the memory past row m is left as it is (it is masked).  In place on the device, in ascending chunks of
 * destination rows staged through at most 32 MiB of the session's bank scratch (idx[j] >= j, so no chunk overwrites a later chunk's
 * sources); returns after the stream has finished.  Hence dinov2_hip_bank_topk afterwards equals, bit for bit, the search of a fresh bank
 * to which the kept rows were added in that order.  Argument errors (NULLs; m out of range; an index out of range or not above the one
 * before it; a session of another device) return DINOV2_HIP_ERR_INVALID and change nothing. */
int  dinov2_hip_bank_keep(dinov2_hip_session *s, dinov2_hip_bank *bank, const int32_t *idx, int32_t m, char *err, size_t errlen);

/* -- spherical k-means of token rows (no reference counterpart: k-means over the patch tokens of one image for unsupervised part or object
 *    segments, over the patches of a whole batch for co-segmentation, and a fixed vocabulary of centres applied to new frames -- visual
 *    words, labels that stay consistent from frame to frame in the realtime loop).  The rows are a caller's matrix or resident tokens of
 *    the session's last un-split forward; only [n] labels and [K, H] centres cross PCIe.  On the device (csrc/kmeans.hip): the rows are
 *    normalised and transposed once; every iteration assigns each row to its most similar centre on the matrix cores (dinov2_hip_match's
 *    tile and K loop, the similarity matrix never written) and sums the members of every cluster with a second GEMM, X^T times the one-hot
 *    matrix of the labels, which is built in LDS and never exists in memory.
 *    Contract:
 *    1. Operands.  Rows and centre vectors go through contract 1 of dinov2_hip_match, the same kernel: f16 unit rows, a zero row stays zero.
 *       Inputs must be finite: the update multiplies rows by a one-hot operand on the matrix cores, so 0 x NaN makes one non-finite row
 *       poison every centre.
 *    2. Assignment.  label[i] = argmax_c sim(i, c) over the K real centres; sim is contract 2 of dinov2_hip_match (the same MFMA shape and
 *       operand roles, k-steps of 32 ascending, an order that depends on H alone); ties go to the LOWEST c, -0 equals +0.  Hence labels and
 *       sim equal idx_ab and sim_ab of dinov2_hip_match_tokens(rows, centre vectors) bit for bit, and a row's label does not depend on the
 *       rows that travel with it.
 *    3. Update.  For every cluster with at least one member, S_c[h] = sum over label[i] == c of x^_ih: the f16 values are exact in f32; the
 *       accumulation is f32 in an order fixed by a pure planner from (n, K, H) alone -- ascending rows within a chunk of rows, then the
 *       chunks ascending.  No atomics: the result is bit-reproducible run to run.  counts are exact integers.
 *    4. Centres.  The vector of centre c is S_c of the last update in which c had members, otherwise the vector it had before -- initially
 *       the init vector, verbatim in f32: an EMPTY cluster keeps its vector.  The f16 centre used for assignment is always
 *       normalise(vector).  `centers` returns these f32 vectors: they point in the right direction but are not unit length.  Passing them
 *       back as DINOV2_HIP_KMEANS_INIT_GIVEN with max_iter = 0 therefore reproduces labels and sim bit for bit.
 *    5. Loop.  c^0 = the init vectors.  Iteration t: labels^t = assign(c^(t-1)); changed = the labels that differ from labels^(t-1) (n at
 *       t = 1).  changed == 0: stop, converged, iterations = t - 1.  Otherwise update, giving c^t.  After max_iter updates one more
 *       assignment runs against c^max_iter (converged if it changes nothing).  The returned labels, sim and counts are always the assignment
 *       against the returned centers.  The host reads one 4-byte `changed` per iteration.
 *    Out of scope: Euclidean k-means; k-means++ seeding (the Python Session.kmeans offers a seeded sample of rows through
 *    DINOV2_HIP_KMEANS_INIT_ROWS, and maximin seeding as init="maximin": the K picks of dinov2_hip_coreset_tokens below, handed over as
 *    DINOV2_HIP_KMEANS_INIT_ROWS); re-seeding empty clusters; K > 1024; bf16 operands; the device group; device-side outputs; the rows of a
 *    list forward; dinov2_compat.hpp and the example programs.
 *    Times: profiles/kmeans.md. */
enum dinov2_hip_kmeans_init { DINOV2_HIP_KMEANS_INIT_GIVEN = 0, DINOV2_HIP_KMEANS_INIT_ROWS = 1 };
typedef struct dinov2_hip_kmeans {
    dinov2_hip_rows rows;     /* GIVEN (host / device), LAST_CLS, LAST_PATCHES of `rows.image`; 1 <= n <= 1 048 576, 8 <= H <= 4096 */
    int32_t all_images;       /* 1 with LAST_PATCHES: the patch rows of EVERY image of the last un-split forward, image-major;
                                 rows.image is ignored and rows.n must be last_b * P.  Must be 0 for the other sources. */
    int32_t K;                /* 1 .. 1024 */
    int32_t max_iter;         /* 0 .. 1000; 0 = assign only (a stored vocabulary applied to new rows) */
    int32_t init;             /* GIVEN: init_centers [K, H] f32 HOST.  ROWS: init_rows [K] HOST indices in [0, n): centre j starts as row init_rows[j] */
    const float   *init_centers;
    const int32_t *init_rows;
    int32_t *labels;          /* [n] HOST; any output may be NULL, not all */
    float   *sim;             /* [n] cosine of each row to its centre */
    float   *centers;         /* [K, H] f32, see contract 4 */
    int32_t *counts;          /* [K] */
    int32_t *iterations;      /* updates performed */
    int32_t *converged;       /* 1 if the loop ended because no label changed */
    int32_t reserved[4];
} dinov2_hip_kmeans;
/* Synchronous: returns after the copy-out, like dinov2_hip_match_tokens.  Argument errors (NULL session or request; n, H, K or max_iter out
 * of range; an unknown init or its pointer NULL; an init_rows entry outside [0, n); all_images with a source other than LAST_PATCHES; all
 * outputs NULL; the resident-source errors of dinov2_hip_bank_add; a misaligned device pointer) return DINOV2_HIP_ERR_INVALID before anything
 * is launched, allocated or copied, with the outputs untouched.  The scratch (host rows' staging copy, X^ and X^T in f16, the centres, at
 * most 32 MiB of partial sums, the results) is a session-owned buffer grown on demand; an allocation the device refuses returns
 * DINOV2_HIP_ERR_HIP.  The session's last forward stays what it was. */
int dinov2_hip_kmeans_tokens(dinov2_hip_session *s, const dinov2_hip_kmeans *km, char *err, size_t errlen);

/* -- greedy k-center selection of rows (no reference counterpart: thinning a memory bank of nominal patch tokens to the 1 - 10 % that cover
 *    the rest -- the coreset step of memory-bank anomaly detection, PatchCore and AnomalyDINO, whose other steps are dinov2_hip_predict,
 *    dinov2_hip_bank_add from resident patches and dinov2_hip_bank_topk with k = 1 --, and maximin seeding of dinov2_hip_kmeans_tokens).
 *    Farthest-point selection by cosine similarity: the next pick is the row least similar to everything picked so far.  The rows are a
 *    caller's matrix, resident tokens of the session's last un-split forward, or the rows of a bank where they lie; only [m] picks and, if
 *    asked for, [n] assignments cross PCIe.  On the device (csrc/coreset.hip): one launch per pick sweeps the n x hpad f16 rows once --
 *    every row's similarity to the picked row against its best so far, and each workgroup's unselected rows folded to one (smallest value,
 *    lowest index) partial; every workgroup of the next launch folds the partials to the next pick itself, so the picked row's index never
 *    travels to the host between picks.  Stream order between the launches is the only synchronisation: no grid-wide barrier, no
 *    cooperative launch, no workgroup waits for another.
 *    Contract:
 *    1. Operands.  Contract 1 of dinov2_hip_match, the same kernel: f16 unit rows, a zero row stays zero.  A bank's rows are used as they
 *       are (they went through that kernel when they were added).  Inputs must be finite.
 *    2. Similarity.  sim(i, c) is contract 2 of dinov2_hip_match: one chain of hpad / 32 16x16x32 f16 MFMA k-steps, ascending, from a zero
 *       accumulator, the same operand roles (csrc/sim_tile.h) -- the bits it has in match, bank top-k and k-means.  A row's values do not
 *       depend on the rows that travel with it, and selecting from a bank equals selecting from the rows that were added to it.
 *    3. Greedy rule.  idx[0] = first, cover[0] = -INFINITY.  After picks 0 .. t - 1, s(i) is the largest sim(i, idx[u]) over u < t and
 *       nearest(i) the LOWEST such u among equal values; -0 is read as +0.  A row's own pick takes part like any other pick.  Pick t is the
 *       not-yet-selected row with the SMALLEST s, among equal values the LOWEST row index, and cover[t] is that s (before pick t changes
 *       it).  cover[1 ..] is therefore non-decreasing: s never falls and the rows to choose from only get fewer.  A selected row is never
 *       selected again, whatever its s (a zero row has s = 0 to itself).  Rows >= n never take part.
 *    4. Stop.  If before pick t >= 1 the smallest s is >= stop_sim, selection ends with selected = t; slots t .. m - 1 then hold idx = -1
 *       and cover = +INFINITY.  nearest / near_sim are always against exactly the `selected` picks, the last one included.
 *    5. Determinism.  The result depends on the rows, first, m and stop_sim alone -- not on launch geometry, on how the rows are split over
 *       workgroups (a pure planner fixes that from (n, H)), or on how often the host looks at the stop flag (a 4-byte read every 256 picks,
 *       none with stop_sim = +INFINITY; a launch that finds the flag set returns at once).  No atomics.
 *    Out of scope: Euclidean distance; the random-projection speed-up of PatchCore (a caller passes projected rows: H >= 8 is accepted); a
 *    choice of `first` by the library; warm starts from an existing selection; bf16 operands; the device group; device-side outputs; the
 *    rows of a list forward; dinov2_compat.hpp and the example programs.
 *    Times: profiles/coreset.md. */
typedef struct dinov2_hip_coreset {
    dinov2_hip_rows rows;         /* GIVEN (host / device), LAST_CLS, LAST_PATCHES of `rows.image`; 1 <= n <= 1 048 576, 8 <= H <= 4096 */
    int32_t all_images;           /* as in dinov2_hip_kmeans */
    const dinov2_hip_bank *bank;  /* non-NULL: the rows are rows [0, count) of this bank, already normalised; `rows` and `all_images` are not
                                     read; n = count (up to 2^24), H = the bank's */
    int32_t m;                    /* rows to select, 1 .. n */
    int32_t first;                /* the first pick, in [0, n) */
    float   stop_sim;             /* stop once every unselected row has a selected row at least this similar; +INFINITY = never; NaN refused */
    int32_t *idx;                 /* [m] HOST: picks in selection order; -1 past `selected`.  Any output may be NULL, not all */
    float   *cover;               /* [m] see contract 3 */
    int32_t *selected;            /* picks made, 1 .. m */
    int32_t *nearest;             /* [n] position in 0 .. selected - 1 of the most similar pick */
    float   *near_sim;            /* [n] that similarity */
    int32_t reserved[4];
} dinov2_hip_coreset;
/* Synchronous: returns after the copy-out, like dinov2_hip_kmeans_tokens.  Argument errors (NULL session or request; n or H out of range;
 * m > n or m < 1; first outside [0, n); a NaN stop_sim; all outputs NULL; all_images with a source other than LAST_PATCHES or an n that is
 * not last_b * P; the resident-source errors of dinov2_hip_bank_add; an empty bank; a bank or session of another device; a misaligned
 * device pointer) return DINOV2_HIP_ERR_INVALID before anything is launched, allocated or copied, with the outputs untouched.  The scratch
 * (host rows' staging copy, the f16 rows unless they are a bank's, 9 bytes of state per row, 16 KiB of partials, the results) is a
 * session-owned buffer grown on demand; an allocation the device refuses returns DINOV2_HIP_ERR_HIP.  The session's last forward stays
 * what it was, and a bank is only read. */
int dinov2_hip_coreset_tokens(dinov2_hip_session *s, const dinov2_hip_coreset *c, char *err, size_t errlen);

/* -- VLAD descriptors of row segments (no reference counterpart: one vector per image for place recognition and image retrieval from
 *    frozen patch tokens -- every token is assigned to the nearest centre of a k-means vocabulary, the residuals are summed per centre,
 *    each centre's sum is normalised, then the whole; the recipe of AnyLoc).  The last step of forward -> vocabulary
 *    (dinov2_hip_kmeans_tokens) -> descriptor -> search.  The rows are a caller's matrix cut into segments by `offsets`, or resident patch
 *    tokens of the session's last un-split forward, one segment per image; only [n_seg, K, H] descriptors cross PCIe, not the tokens.  On
 *    the device (csrc/vlad.hip): every segment is normalised into a block of its own, padded to whole 128-row tiles; k-means' assignment
 *    walk and its one-hot GEMM then run per segment, and one workgroup per (segment, centre) forms the residual and its norm.
 *    Contract:
 *    1. Operands.  Rows and centre vectors go through contract 1 of dinov2_hip_match, the same row code: x^, c^ (f16 unit rows; a zero
 *       row stays zero).  Inputs must be finite.
 *    2. Assignment.  Contract 2 of dinov2_hip_kmeans.  labels and sim equal those of dinov2_hip_kmeans_tokens(max_iter = 0) with the same
 *       centres and idx_ab / sim_ab of dinov2_hip_match_tokens(rows, centers) bit for bit.
 *    3. Sums.  For segment s and centre c, n_sc = the number of rows of s with label c (a zero row counts: the tie rule gives it centre
 *       0), S_sc[h] = the f32 sum of the members' x^_ih.  The order is fixed by a pure planner from (len_s, K, H) alone -- ascending rows
 *       within a chunk of rows of the segment, then the chunks ascending.  No atomics.  Hence a segment's descriptor, counts and labels
 *       have the same bits whatever segments travel with it and at whatever position: alone, first or last of a list, and as
 *       LAST_PATCHES of image i of a batch against GIVEN with the same rows.
 *    4. Residual.  R_sc[h] = S_sc[h] - n_sc * c^_c[h] in f32 (the product rounded, then the difference); c^ is the f16 unit centre the
 *       assignment used, not the caller's vector.  An empty cluster gives a zero row.
 *    5. Norms.  DINOV2_HIP_VLAD_INTRA_NORM: R_sc <- R_sc / sqrt(ss) per (s, c), ss = the f32 sum of the f32 squares in an order that
 *       depends on H alone; square root and division correctly rounded; ss == 0 stays zero.  DINOV2_HIP_VLAD_L2_NORM: the same over the
 *       K H values of segment s as they stand after INTRA (if set), in an order that depends on (K, H) alone.  Nothing is normalised
 *       across segments.  flags = 0 returns the raw R.
 *    Out of scope: soft assignment; descriptors written into a bank (they are K H wide, the bank stops at 4096); device-side outputs; PCA
 *    or whitening of descriptors; the device group; the rows of a list forward (GIVEN rows with `offsets` cover them); bf16 operands;
 *    dinov2_compat.hpp and the example programs.
 *    Times: profiles/vlad.md. */
enum dinov2_hip_vlad_flags { DINOV2_HIP_VLAD_INTRA_NORM = 1, DINOV2_HIP_VLAD_L2_NORM = 2 };
typedef struct dinov2_hip_vlad {
    dinov2_hip_rows rows;     /* GIVEN (host / device) or LAST_PATCHES of `rows.image`; LAST_CLS is refused.  1 <= n <= 1 048 576, 8 <= H <= 4096 */
    int32_t all_images;       /* as dinov2_hip_kmeans: 1 with LAST_PATCHES = one segment per image of the last un-split forward
                                 (rows.n = last_b * P, n_seg = last_b) */
    const int32_t *offsets;   /* GIVEN only, HOST, [n_seg + 1], strictly ascending, offsets[0] = 0, offsets[n_seg] = rows.n: segment i is
                                 rows [offsets[i], offsets[i + 1]).  NULL = one segment (n_seg must be 1).  Must be NULL for a resident source. */
    int32_t n_seg;            /* 1 .. 4096; LAST_PATCHES: 1, or last_b with all_images.  n_seg * K * H <= 2^28 */
    int32_t K;                /* 1 .. 1024 */
    const float *centers;     /* [K, H] f32 HOST: vectors of any length, e.g. what dinov2_hip_kmeans_tokens returned */
    uint32_t flags;           /* DINOV2_HIP_VLAD_INTRA_NORM | DINOV2_HIP_VLAD_L2_NORM; 0 = the raw residual sums */
    float   *vlad;            /* [n_seg, K, H] HOST; any output may be NULL, not all */
    int32_t *counts;          /* [n_seg, K] */
    int32_t *labels;          /* [rows.n] */
    float   *sim;             /* [rows.n] */
    int32_t reserved[4];
} dinov2_hip_vlad;
/* Synchronous: returns after the copy-out, like dinov2_hip_kmeans_tokens.  Argument errors (NULL session, request or centers; all outputs
 * NULL; rows, H, K, n_seg or n_seg * K * H out of range; offsets that do not ascend strictly from 0 to rows.n, or NULL with n_seg != 1;
 * offsets or all_images with a source they do not go with; LAST_CLS; n_seg or rows.n that are not the resident source's; the
 * resident-source errors of dinov2_hip_bank_add; a misaligned device pointer; unknown flag bits) return DINOV2_HIP_ERR_INVALID before
 * anything is launched, allocated or copied, with the outputs untouched.  The scratch (host rows' staging copy, X^ and X^T in f16 in the
 * padded layout, the centres, the tables, at most 32 MiB of partial sums -- the segments are walked in passes --, the results) is a
 * session-owned buffer grown on demand; an allocation the device refuses returns DINOV2_HIP_ERR_HIP.  The session's last forward stays
 * what it was. */
int dinov2_hip_vlad_tokens(dinov2_hip_session *s, const dinov2_hip_vlad *v, char *err, size_t errlen);

/* -- spectral embedding of token rows (no reference counterpart: the leading eigenvectors of the normalised patch-affinity graph,
 *    (D - W) z = lambda D z.  TokenCut cuts the second one of one image's patches at its mean: unsupervised object discovery; Deep Spectral
 *    Methods and the NCut visualisations feed the first few to k-means -- dinov2_hip_kmeans_tokens -- or show them as colours).  The rows
 *    are a caller's matrix or resident tokens of the session's last un-split forward; only [n_eig, n] vectors cross PCIe, and the n x n
 *    matrix W never exists: every step forms it tile by tile on the matrix cores (dinov2_hip_match's tile and K loop), maps the f32
 *    accumulators to affinities and multiplies them into an 8-column f64 block at once (csrc/ncut.hip; the loop: csrc/ncut.cpp).
 *    Contract:
 *    1. Operands.  Contract 1 of dinov2_hip_match, the same row code: f16 unit rows x^, a zero row stays zero.  Inputs must be finite.
 *    2. Similarity.  s_ij is contract 2 of dinov2_hip_match through the same tile code (csrc/sim_tile.h): the bits dinov2_hip_match_tokens,
 *       the bank and k-means give that pair.  The diagonal is a pair like any other.  Columns j >= n carry weight 0 whatever f(0) is.
 *    3. Affinity.  w_ij = f(s_ij) in f32 on the f32 similarity, -0 read as +0.  THRESHOLD: s > tau ? 1 : floor (strictly greater).  RELU:
 *       max(s, 0).  EXP: expf((s - 1) / tau), the difference and the correctly rounded quotient in f32, expf the device library's (at most
 *       1 ulp from the exact exponential of its argument).
 *    4. Degrees and operator.  d_i = sum_j w_ij; c_i = d_i > 0 ? 1 / sqrt(d_i) : 0 in f64, so a vertex of degree 0 has zero entries in every
 *       vector.  The iteration runs on A = 1/2 (I + C W C), C = diag(c): the shift keeps the spectrum in [0, 1], so an affinity that is not
 *       positive semi-definite (THRESHOLD) cannot make the iteration converge to the negative end.  Every sum over j is f64 (w_ij exact in
 *       f64, one fused multiply-add per term) in an order a pure planner fixes from (n, H) alone: within a chunk of column tiles every one
 *       of 8 accumulators per row (column j of the tile belongs to accumulator (j / 64) * 4 + (j % 16) / 4) adds its columns in ascending
 *       order, the accumulators fold as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)), then the chunks fold in ascending order.  No atomics
 *       anywhere: a call is bit-reproducible run to run.
 *    5. Iteration.  Block width 8, Y in f64 [n, 8].  Every step: Q = Y_prev R^-1 (CholeskyQR: R from the Gram matrix Y_prev^T Y_prev, the
 *       sum of per-workgroup partials -- 128 rows each, ascending -- in ascending order), then Y_next = A Q.  The start block is a fixed
 *       function of (n, d): column 0 is sqrt(d_i), the known top eigenvector of A; column c = 1 .. 7 is
 *       sin(0.37 (i + 1) (c + 1)) + (c == i % 8 ? 0.5 : 0); a row of degree 0 is zero.  Every 8 steps for the first 32, then every 16, the
 *       host does Rayleigh-Ritz from two 8 x 8 matrices, B = Q^T Y_next (symmetrised) and G = Y_next^T Y_next, both from per-workgroup
 *       partials: B v_k = theta_k v_k (theta descending), residual r_k^2 = v_k^T G v_k - theta_k^2 = ||A u_k - theta_k u_k||^2 for
 *       u_k = Q v_k.  The loop ends when r_k <= tol for every k < n_eig (converged = 1) or when at least max_iter steps are done;
 *       iterations = the steps done, max_iter rounded up to the check interval.  lambda_k = 2 (1 - theta_k).
 *    6. Vectors.  Formed once at the end on the host in f64 from the last Y_next: z_k = C (Y_next v_k), scaled to unit Euclidean length,
 *       the entry of largest magnitude positive (the lowest index at a tie), then rounded to f32.
 *    Out of scope: Nystrom and other sub-sampling; Lanczos or LOBPCG; exploiting the symmetry of W; a materialised W; n_eig > 6;
 *    device-side outputs; bf16 operands; the device group; the rows of a list forward; KNN-sparsified graphs; dinov2_compat.hpp and the
 *    example programs.
 *    Times: profiles/ncut.md. */
enum dinov2_hip_ncut_affinity { DINOV2_HIP_NCUT_THRESHOLD = 0, DINOV2_HIP_NCUT_RELU = 1, DINOV2_HIP_NCUT_EXP = 2 };
typedef struct dinov2_hip_ncut {
    dinov2_hip_rows rows;   /* GIVEN (host / device), LAST_CLS, LAST_PATCHES of rows.image; 16 <= n <= 131 072, 8 <= H <= 4096 */
    int32_t all_images;     /* as dinov2_hip_kmeans: 1 with LAST_PATCHES = the patch rows of every image of the last un-split forward */
    int32_t affinity;       /* THRESHOLD: w = s > tau ? 1 : floor (TokenCut: tau 0.2, floor 1e-5); RELU: w = max(s, 0); EXP: w = exp((s - 1) / tau) */
    float   tau, floor;     /* THRESHOLD: -1 <= tau < 1, 0 <= floor <= 1; EXP: 2^-6 <= tau <= 16; otherwise ignored */
    int32_t n_eig;          /* 1 .. 6 */
    int32_t max_iter;       /* 1 .. 10 000 steps (rounded up to the check interval) */
    float   tol;            /* 1e-6 .. 1e-1: stop when every residual ||A u_k - theta_k u_k|| <= tol, k < n_eig */
    float   *values;        /* [n_eig] HOST: lambda_k of (D - W) z = lambda D z, ascending (lambda_0 ~ 0); any output may be NULL, not all */
    float   *vectors;       /* [n_eig, n]: z_k = D^-1/2 u_k, unit Euclidean length, entry of largest magnitude positive (lowest index at a tie) */
    float   *degree;        /* [n] d_i = sum_j w_ij */
    float   *residual;      /* [n_eig] */
    int32_t *iterations, *converged;
    int32_t reserved[4];
} dinov2_hip_ncut;
/* Synchronous: returns after the copy-out, like dinov2_hip_kmeans_tokens; the host waits for the stream at the degrees and at every check.
 * Argument errors (NULL session or request; n, H, n_eig, max_iter, tol, tau or floor out of range; an unknown affinity; all outputs NULL;
 * all_images with a source other than LAST_PATCHES or an n that is not last_b * P; the resident-source errors of dinov2_hip_bank_add; a
 * misaligned device pointer) return DINOV2_HIP_ERR_INVALID before anything is launched, allocated or copied, with the outputs untouched.
 * Rows that are not finite are found at the first check and return DINOV2_HIP_ERR_INVALID too, outputs untouched.  The scratch (host
 * rows' staging copy, x^ in f16, two blocks, their 8 x 8 partials, d and c, at most 32 MiB of partial sums) is a session-owned buffer grown
 * on demand; an allocation the device refuses returns DINOV2_HIP_ERR_HIP.  The session's last forward stays what it was. */
int dinov2_hip_ncut_tokens(dinov2_hip_session *s, const dinov2_hip_ncut *nc, char *err, size_t errlen);

/* -- video label propagation over a frame memory (no reference counterpart: the label-propagation protocol of DINO's video-segmentation
 *    evaluation on DAVIS -- every patch of a new frame looks at the patches of a few remembered frames (the first one and the last few)
 *    inside a spatial window around its own cell, keeps its k most similar ones and takes the softmax-weighted mean of their label vectors.
 *    Masks, part labels, clicked points or a dense head's output on a key frame then follow a video at one forward per frame: forward,
 *    propagate with keep, set -- no token and no label crosses PCIe).  The memory is one device allocation on the model's device, made at
 *    create and never moved: f16 rows [frames][P rounded up to the 128-row tile][H rounded up to 64], zeroed at create, so that every slot
 *    owns whole tiles; f32 labels [frames][P][C]; the kept result [P][C]; a cell table.  All offsets are 64-bit.  It keeps only the device
 *    ordinal, so it may outlive the model; a session of another device is refused.  One host thread at a time uses a memory.  On the device
 *    (csrc/propagate.hip): dinov2_hip_match's normalisation kernel, a selection kernel with the tile of dinov2_hip_match and the per-row
 *    list of dinov2_hip_bank_topk (one source each: csrc/sim_tile.h, csrc/topk_list.h), the bank's merge kernel, and a combine kernel.  The
 *    affinity matrix is never written.
 *    Contract:
 *    1. Operands.  Contract 1 of dinov2_hip_match, the same row code (csrc/normalise_row.h): f16 unit rows, a zero row stays zero.  Inputs
 *       must be finite.
 *    2. Similarity.  Contract 2 of dinov2_hip_match: the same tile and K loop, so a pair has the bits it has in dinov2_hip_match_tokens and
 *       dinov2_hip_bank_topk.
 *    3. Candidates.  Query i sits at cell (i / w0, i % w0).  Column (f, p) -- patch p of slot f -- is a candidate iff bit f of `slots` is
 *       set and (radius < 0 or max(|qy - py|, |qx - px|) <= radius).  Rows P .. Ppad - 1 of a slot and unset slots never enter a list, and
 *       nothing is assumed about their memory (dinov2_hip_propmem_drop does not touch it).
 *    4. Selection.  The first k candidates in the strict total order of dinov2_hip_bank_topk: the larger f32 value first (-0 is read as
 *       +0), among equal values the LOWEST index, where index = f * P + p.  Slots beyond the number of candidates hold idx = -1 and
 *       sim = -INFINITY.  Hence with radius = -1 and slots 0 .. n - 1 set, idx and sim equal those of dinov2_hip_bank_topk on a bank that
 *       holds the same frames in slot order, bit for bit.  A query's result does not depend on the chunking, nor on which other queries
 *       travel with it.
 *    5. Weights.  w_j = expf((sim_j - sim_0) / T): an f32 subtraction, a correctly rounded f32 division, the device library's expf (not
 *       the fast intrinsic).  w_0 = 1 exactly; an empty slot weighs 0.
 *    6. Output.  out[c] = (sum_j w_j L[idx_j][c]) / (sum_j w_j): every product rounded to f32, both sums in f32 with j ascending, the
 *       division correctly rounded.  No atomics: the result is bit-reproducible run to run.  argmax[i] is the LOWEST c among the largest
 *       out[i][c].  With keep, out also stays in the memory for the next dinov2_hip_propmem_set with labels == NULL.  This is DINO's
 *       procedure (exp(sim / T) masked to the window, the top k per query, normalised, labels x affinity) wherever no tie sits on the
 *       k-th value; there the published code keeps ALL the tied entries, and this keeps those with the lowest indices.
 *    Out of scope: device-side outputs, the device group, the rows of a list forward, bf16 operands, k > 64, non-rectangular windows,
 *    upsampling of the result to pixels, dinov2_compat.hpp and the example programs.
 *    Times: profiles/propagate.md. */
typedef struct dinov2_hip_propmem dinov2_hip_propmem;   /* resident: F slots of one h0 x w0 patch grid */

/* 8 <= H <= 4096, 1 <= h0, w0 <= 256, 1 <= frames <= 64, frames * Ppad <= 2^24 (Ppad = h0 w0 rounded up to 128), 1 <= C <= 256, else
 * DINOV2_HIP_ERR_INVALID.  Every slot starts empty.  An allocation the device refuses returns DINOV2_HIP_ERR_HIP and leaves nothing
 * behind for the next launch to report. */
int  dinov2_hip_propmem_create(dinov2_hip_model *model, int32_t H, int32_t h0, int32_t w0, int32_t frames, int32_t C,
                               dinov2_hip_propmem **out, char *err, size_t errlen);
/* waits for the device first, like dinov2_hip_bank_free */
void dinov2_hip_propmem_free(dinov2_hip_propmem *mem);
/* Fills slot `slot` (0 .. frames - 1; a filled slot is overwritten): `rows` -- GIVEN (host or device, [P, H]) or LAST_PATCHES of one image
 * of the last un-split forward; LAST_CLS is refused; n must be P = h0 w0 -- are normalised into the slot, and `labels` [P, C] f32 (host,
 * or device with labels_on_device = 1) become its labels.  labels == NULL: the soft labels that the last dinov2_hip_propagate with
 * keep = 1 left in this memory (refused when there are none).  Returns after the stream has finished, like dinov2_hip_bank_add.
 * Argument errors (NULLs; a slot out of range; those of dinov2_hip_bank_add for `rows`, the resident-source errors included; H unequal
 * to the memory's; a misaligned device pointer; a session of another device) return DINOV2_HIP_ERR_INVALID
 * before anything is launched, allocated or copied, with the memory untouched. */
int  dinov2_hip_propmem_set(dinov2_hip_session *s, dinov2_hip_propmem *mem, int32_t slot, const dinov2_hip_rows *rows,
                            const float *labels, int32_t labels_on_device, char *err, size_t errlen);
/* the slot becomes empty; the memory is not touched.  DINOV2_HIP_ERR_INVALID for NULL or a slot out of range. */
int  dinov2_hip_propmem_drop(dinov2_hip_propmem *mem, int32_t slot);

typedef struct dinov2_hip_propagate_req {
    dinov2_hip_rows queries; /* GIVEN or LAST_PATCHES; n must be P */
    uint64_t slots;          /* bit f set: slot f is context.  Every set bit must be a filled slot; at least one must be set */
    int32_t radius;          /* Chebyshev radius in patch cells, 0 .. 255; -1: no window */
    int32_t k;               /* 1 .. 64 */
    float   temperature;     /* finite, 1e-3 .. 1e3 */
    int32_t keep;            /* 1: out also stays in the memory for the next dinov2_hip_propmem_set(labels = NULL); else 0 */
    float   *labels;         /* [P, C] HOST: out of contract 6.  Any output may be NULL, but not all of them with keep == 0 */
    int32_t *argmax;         /* [P] */
    int32_t *idx;            /* [P, k] */
    float   *sim;            /* [P, k] */
    int32_t reserved[4];
} dinov2_hip_propagate_req;
/* Synchronous: returns after the copy-out.  Argument errors (NULLs; those of dinov2_hip_propmem_set for `queries`; LAST_CLS; a set bit
 * that is no filled slot; no bit set; radius, k, temperature or keep out of range; nothing asked for) return DINOV2_HIP_ERR_INVALID
 * before anything is launched, allocated or copied, with the outputs and the memory untouched.  The scratch (the f16 queries, host queries'
 * staging copy, at most 32 MiB of partial lists, the results) is a session-owned buffer grown on demand; an allocation the device refuses
 * returns DINOV2_HIP_ERR_HIP. */
int  dinov2_hip_propagate(dinov2_hip_session *s, dinov2_hip_propmem *mem, const dinov2_hip_propagate_req *req, char *err, size_t errlen);

/* -- linear dense-prediction heads (no reference counterpart: semantic segmentation and depth estimation with a linear head on frozen
 *    patch features, two of the evaluation protocols of the DINOv2 paper; upstream: BNHead of
 *    dinov2/eval/segmentation/models/decode_heads/linear_head.py and of dinov2/eval/depth/models/decode_heads/linear_head.py).  A resident head
 *    -- a 1x1 convolution over the concatenated patch tokens of up to 8 layers -- and ONE call that runs the forward and returns a label map
 *    or a depth map [B, out_h, out_w]: the tapped tokens, the low-resolution logits and the resampling all stay on the device, and the
 *    full-resolution logit planes never exist.  On the device (csrc/dense.hip): at each requested layer one kernel writes the patch rows as
 *    f16 into their columns of the operand A [B P, K]; one plain GEMM on the matrix cores gives the low-resolution logits; one kernel
 *    interpolates them per output pixel and reduces over the classes.  The head is one device allocation made at create (f16 weight, bias,
 *    centres) and never moved; it keeps the device ordinal, the hidden size and the number of layers only, so it may outlive the model; one
 *    host thread at a time uses a session with it.
 *    BatchNorm (upstream's BNHead normalises the concatenated features before the convolution) is folded by the caller: with
 *        s = gamma / sqrt(var + eps)      (per input channel k)
 *        W' = W diag(s)                   W'[c][k] = W[c][k] s[k]
 *        b' = b + W (beta - mean * s)
 *    pass W' and b' (the Python binding has fold_batchnorm).
 *    Contract:
 *    1. Operands.  Row (b, p) of A is, per requested layer in list order, f16 (round to nearest even) of exactly the f32 bits
 *       dinov2_hip_predict_layers gives for that patch row with the same `norm`; with concat_cls that image's CLS row of the same layer
 *       follows (so K = n_layers * H * (1 + concat_cls), layer-major, patch then cls).  W^ = f16(W).  The operands are f16 whatever the
 *       model's compute type, as for dinov2_hip_pca3 and dinov2_hip_match.  Values must lie within the f16 range; outside it the result is
 *       unspecified.
 *    2. Low-resolution logits.  L[b][p][c] = sum_k A^ W^ + bias[c]: the products are exact in f32, the accumulation is f32 on the matrix
 *       cores in an order that depends on K alone, the bias is added last.  An image's logits are bit-identical whatever batch it travels
 *       in, and whether or not the batch is split into passes.
 *    3. Resampling.  Bilinear, half-pixel centres, PyTorch's align_corners=False, all in f32, per axis (n_in = h0 or w0, n_out = out_h or out_w):
 *           scale = (float)n_in / (float)n_out
 *           src   = max(scale * (dst + 0.5f) - 0.5f, 0)
 *           i0 = min((int)src, n_in - 1),  i1 = min(i0 + 1, n_in - 1),  lambda = src - i0
 *       and with the four neighbours v00 (y i0, x i0), v01 (y i0, x i1), v10, v11 of class c:
 *           t = (1 - lx) * v00 + lx * v01,   u = (1 - lx) * v10 + lx * v11,   val = (1 - ly) * t + ly * u
 *       Every multiplication and addition is rounded on its own; nothing is contracted into a fused multiply-add.  A numpy float32
 *       restatement gives the same bits (tests/dense_cases.py).
 *    4. ARGMAX.  labels = the argmax over c of val_c; equal values go to the LOWEST class (-0 equals +0); `value` is that val.  The argmax
 *       is taken after the interpolation, never before it.
 *    5. BINS.  r_c = max(val_c, 0) + eps,  S = sum_c r_c,  D = sum_c r_c * center_c, both sums in f32, sequential in ascending c (an order
 *       that depends on C alone), uncontracted;  value = D / S with a correctly rounded division.
 *    6. Independence.  A pixel's result does not depend on launch geometry, on how out_h x out_w is tiled, or on the other images.
 *    Out of scope: the device group (dinov2_hip_group_*); dinov2_compat.hpp; C > 256; softmax probabilities; the final scalar resize of a
 *    depth map to the image size (upstream reduces over the bins at 4 h0 x 4 w0: pass that as out_h, out_w); multi-scale
 *    inference (sliding-window inference is dinov2_hip_predict_dense_slide, below); reading head weights from GGUF or mmseg checkpoints; hidden sizes that are not a multiple of 64.
 *    Times: profiles/dense_head.md. */
enum dinov2_hip_dense_reduce { DINOV2_HIP_DENSE_ARGMAX = 0, DINOV2_HIP_DENSE_BINS = 1 };
typedef struct dinov2_hip_dense_head dinov2_hip_dense_head;
typedef struct dinov2_hip_dense_desc {
    const int32_t *layers;    /* as dinov2_hip_layers: strictly ascending, each in [0, L] (number of blocks applied) */
    int32_t n_layers;         /* 1 .. 8 */
    int32_t norm;             /* 1: the model's final LayerNorm on the tapped rows (upstream default) */
    int32_t concat_cls;       /* 1: every layer's block is [patch row ; CLS row of that image] (upstream's depth heads) */
    int32_t num_classes;      /* C, 2 .. 256 */
    const float *weight;      /* HOST [C, K] f32, K = n_layers * H * (1 + concat_cls); column order: layer-major, patch then cls */
    const float *bias;        /* HOST [C] or NULL */
    int32_t reduce;           /* DINOV2_HIP_DENSE_ARGMAX | DINOV2_HIP_DENSE_BINS */
    const float *bin_centers; /* HOST [C], BINS only */
    float bins_eps;           /* BINS only, > 0 (upstream 0.1) */
    int32_t reserved[6];
} dinov2_hip_dense_desc;
/* Copies what `desc` points to: the caller's arrays may go afterwards.  Argument errors (NULL model, desc, out, layer list or weight; a bad
 * layer list; num_classes out of range; an unknown reduce; BINS without centres or with bins_eps <= 0; a hidden size that is not a
 * multiple of 64) return DINOV2_HIP_ERR_INVALID before anything is launched, allocated or copied.  An allocation the device refuses returns
 * DINOV2_HIP_ERR_HIP. */
int  dinov2_hip_dense_head_create(dinov2_hip_model *model, const dinov2_hip_dense_desc *desc, dinov2_hip_dense_head **out, char *err,
                                  size_t errlen);
/* waits for the device first: a session's stream may still be reading the weight */
void dinov2_hip_dense_head_free(dinov2_hip_dense_head *head);

typedef struct dinov2_hip_dense_out {
    int32_t out_h, out_w;  /* the grid on which the reduction over C runs; 0, 0 = the network input size; otherwise each 1 .. 8192 */
    uint8_t *labels;       /* [B, out_h, out_w], ARGMAX only */
    float   *value;        /* [B, out_h, out_w]; ARGMAX: the winning interpolated logit, BINS: the expectation D / S */
    float   *logits;       /* [B, P, C] token-major low-resolution logits (contract 2); any of the three may be NULL, not all */
    int32_t on_device;     /* as dinov2_hip_layers: 0 host (staged in the session's scratch, one stream wait at the end), 1 device pointers,
                              16-byte aligned, written asynchronously on the session's stream */
    int32_t reserved[4];
} dinov2_hip_dense_out;
/* `out` (may be NULL) and `flags` as for dinov2_hip_predict: one call returns the classifier's logits and the dense prediction of the same
 * forward.  The patch rows are rows 1 + R .. T - 1, with or without DINOV2_HIP_CLASSIFY.  Argument errors (NULL session, input, head or
 * `dense`; out_h or out_w out of range, the network input size with 0, 0 included; `labels` requested from a BINS head; all three outputs
 * NULL; a device pointer that is not 16-byte aligned; a head created for a model with another hidden size or number of layers; a session
 * on another device than the head; those of dinov2_hip_predict) return their status before anything is launched, allocated or copied, with
 * the outputs untouched.  A batch that is split into passes runs the dense stage once per pass, each pass writing at its image offset.  The
 * call runs eagerly under DINOV2_HIP_GRAPHS=1.  dinov2_hip_fetch, dinov2_hip_pca3(tokens = NULL), dinov2_hip_match_tokens and the
 * dinov2_hip_bank_* calls behave afterwards as after a dinov2_hip_predict of the same shape.  The scratch (the f16 operand and the logits
 * of one pass, rows rounded up to 256, and host outputs' staging) is a session-owned buffer grown on demand; an allocation the device
 * refuses returns DINOV2_HIP_ERR_HIP.  In dinov2_hip_session_profile the packing launches are booked under "layer_tap", the GEMM and the
 * reduction under "head". */
int dinov2_hip_predict_dense(dinov2_hip_session *session, const dinov2_hip_input *in, dinov2_hip_output *out /* may be NULL */,
                             const dinov2_hip_dense_head *head, const dinov2_hip_dense_out *dense, uint32_t flags, char *err, size_t errlen);

/* -- sliding-window dense inference (no reference counterpart; mmsegmentation's slide_inference, test_cfg = dict(mode='slide', crop_size,
 *    stride): how the published linear-head numbers are produced, and the way to label an image larger than the size the head was trained
 *    at).  ONE call: the images are uploaded once, one kernel copies the windows into a window batch (csrc/slide.hip), the ordinary forward
 *    and head give every window's low-resolution logits (split into passes as usual), and one kernel averages, per pixel and class, the
 *    resampled logits of the windows that cover the pixel and reduces over the classes.  Neither the full-resolution logit planes nor the
 *    windows' resamplings ever exist in memory.
 *    Input: B f32 images of one size h x w, DINOV2_HIP_BGR_HWC or DINOV2_HIP_RGB_CHW, host or device; crop_h <= h <= 8192 and
 *    crop_w <= w <= 8192; h and w need not be multiples of the patch size.  DINOV2_HIP_U8_BGR_HWC is refused (raw preprocessing resizes to a
 *    network size, which is what sliding avoids).  Output: `dense` with out_h, out_w = 0, 0 (the image size); labels and value [B, h, w];
 *    logits [B, ny nx, P, C], the low-resolution logits per window, image-major, windows in index order; any of the three may be NULL, not
 *    all; on_device as for dinov2_hip_predict_dense.
 *    Contract (continuing that of dinov2_hip_predict_dense, whose items 3 - 5 it refers to):
 *    1. Windows.  Per axis (len = h or w, crop, stride):  n = max(len - crop + stride - 1, 0) / stride + 1  (integer division),
 *       start_i = max(min(i * stride + crop, len) - crop, 0): the last window is pulled back to end at the image edge.  Window
 *       k = iy * nx + ix covers rows [y1[iy], y1[iy] + crop_h) and columns [x1[ix], x1[ix] + crop_w).  dinov2_hip_slide_windows returns them.
 *    2. Window logits.  Window k of image b has, bit for bit, the `logits` dinov2_hip_predict_dense returns for that crop alone (batch
 *       invariance: the window batch goes through the ordinary forward, split into passes as usual).
 *    3. Per pixel (Y, X) and class c, over the windows that cover the pixel in ascending k:  val_c^k = item 3 of dinov2_hip_predict_dense
 *       with n_in = (h0, w0) of the crop's grid (dinov2_hip_model_grid), n_out = (crop_h, crop_w), dst = (Y - y1_k, X - x1_k);  acc_c starts as
 *       the first covering window's val and adds the following ones one at a time in f32, in that order;  mean_c = acc_c / (float)n with n
 *       the number of covering windows, a correctly rounded division.  Nothing is contracted into a fused multiply-add.
 *    4. Reduction.  ARGMAX and BINS are applied to mean_c exactly as items 4 and 5 of dinov2_hip_predict_dense: ties go to the lowest
 *       class, S and D are summed in ascending c.  The mean is taken BEFORE the argmax (upstream averages logits, then decides).
 *    5. One window.  With h == crop_h and w == crop_w there is one window, n = 1, and labels and value have the bits of
 *       dinov2_hip_predict_dense at out_h, out_w = 0, 0.
 *    6. Independence.  A pixel's result does not depend on launch geometry, on the tiling or the staging of the classes, on the other images,
 *       on the batch, or on how the windows were split into passes.
 *    Out of scope: multi-scale and flip augmentation (they average softmax probabilities); a final resize of the map; images smaller than
 *    the crop (dinov2_hip_predict_dense); raw 8-bit input; the classifier outputs of the window forwards; the device group;
 *    dinov2_compat.hpp; lists of images of different sizes; graph capture.  Times: profiles/dense_slide.md. */
#define DINOV2_HIP_SLIDE_COVER_MAX 16
typedef struct dinov2_hip_slide {
    int32_t crop_h, crop_w;      /* the window: a network input size of this model (dinov2_hip_model_grid accepts it) */
    int32_t stride_h, stride_w;  /* 1 .. crop_h, 1 .. crop_w; any integer, no relation to the patch size needed    */
    int32_t reserved[4];
} dinov2_hip_slide;
/* No device.  *ny, *nx and the window starts y1[ny], x1[nx] of contract 1 (either array may be NULL; 8192 entries always suffice); window
 * k = iy * nx + ix.  Refuses (DINOV2_HIP_ERR_INVALID, naming the value): a NULL model, `sl`, ny or nx; a crop that dinov2_hip_model_grid
 * refuses; a stride outside 1 .. crop; an image smaller than the crop or larger than 8192. */
int dinov2_hip_slide_windows(const dinov2_hip_model *model, int32_t h, int32_t w, const dinov2_hip_slide *sl,
                             int32_t *ny, int32_t *nx, int32_t *y1, int32_t *x1, char *err, size_t errlen);
/* Argument errors (a NULL argument or input data; a batch below 1; raw 8-bit or unknown layout; the refusals of dinov2_hip_slide_windows;
 * out_h, out_w other than 0, 0; `labels` from a BINS head; all outputs NULL; a device pointer that is not 16-byte aligned; the head / session
 * mismatches of dinov2_hip_predict_dense; B ny nx > 65 535; a pixel covered by more than DINOV2_HIP_SLIDE_COVER_MAX windows -- per axis the
 * cover is at most ceil(crop / stride) + 1, so stride >= crop / 3 always passes) return their status, naming the value, before anything is
 * allocated, copied or launched, and leave the outputs untouched.  Afterwards the session has no last un-split forward, exactly as after
 * dinov2_hip_predict_list: dinov2_hip_fetch, dinov2_hip_pca3(tokens = NULL), resident dinov2_hip_match_tokens and the bank's LAST_* sources
 * are refused until the next dinov2_hip_predict, which gives the bits it gives in a fresh session.  Device input with device outputs is
 * asynchronous on the session's stream in steady state; host outputs are complete on return (one stream wait at the end).  The call
 * runs eagerly under DINOV2_HIP_GRAPHS=1.  The scratch (a host input's images, the window table, the window batch, the logits of all windows and
 * host outputs' staging) is a session-owned buffer grown on demand, beside that of dinov2_hip_predict_dense for the window batch; an
 * allocation the device refuses returns DINOV2_HIP_ERR_HIP.  In dinov2_hip_session_profile the window gather is booked under "im2col" (the
 * kind of the input-side rearrangements; the raw 8-bit preprocessing launch is not booked at all) and the reduction under "head". */
int dinov2_hip_predict_dense_slide(dinov2_hip_session *session, const dinov2_hip_input *in,
                                   const dinov2_hip_dense_head *head, const dinov2_hip_slide *sl,
                                   const dinov2_hip_dense_out *dense, char *err, size_t errlen);

/* -- quantise a GGUF (replaces dino_model_quantize, dinov2.h:118 / dinov2.cpp:355-453).  Host only.
 *    itype: ggml type id 2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0.  2-D tensors named `*weight` are re-encoded, the rest copied. */
int dinov2_hip_quantize(const char *fname_inp, const char *fname_out, int32_t itype, char *err, size_t errlen);

/* Host helper, exposed for parity tests: interpolate_pos_embed (dinov2.h:101-103 / dinov2.cpp:159-225).
 * out: [(1 + h_new*w_new), H] f32. */
int dinov2_hip_interpolate_pos_embed(const dinov2_hip_model *model, int32_t h_new, int32_t w_new, float *out);

/* -- measurement hooks (no reference counterpart; the reference times the whole call, inference.cpp:64-68) */
/* Per-kernel-kind HIP-event timing of subsequent predicts on this session (adds two events per launch). */
int dinov2_hip_session_profile(dinov2_hip_session *session, int32_t enable);
/* Accumulated since enable: for kind k in [0, n): name, total ms, launches.  Returns n (<= max).  The kind "layer_tap" holds the launches of
 * dinov2_hip_predict_layers (one per layer) AND those of dinov2_hip_predict_attention (one per attention layer: a tap of the attention). */
int dinov2_hip_session_profile_read(dinov2_hip_session *session, int32_t max, const char **names, float *total_ms,
                                    int32_t *launches);
/* Debug/parity: copy the f32 token stream [B, T, H] as it stands after `layer` layers (0 = embeddings) of the
 * LAST predict with the same shape re-run up to that point.  Host pointer.  (Product code wants dinov2_hip_predict_layers.) */
int dinov2_hip_debug_hidden(dinov2_hip_session *session, const dinov2_hip_input *in, int32_t layer, float *out,
                            char *err, size_t errlen);

int dinov2_hip_abi_version(void);
/* the commit the library was built from ("<12 hex digits>[+dirty]", "unknown" outside a git checkout): measurements taken where there is
 * no repository next to the library (bench.py on a GPU box) stamp themselves with it */
const char *dinov2_hip_build_id(void);

/* -- Environment ----------------------------------------------------------------------------------------------------------
 * The library reads exactly seven environment variables; none is needed in normal use.
 *   DINOV2_HIP_GRAPHS=1      replay a captured hipGraph for a forward that repeats with the same session, input pointer, shape
 *                            and flags (second sighting is captured).  Off by default: the forward is kernel-bound and the
 *                            replay measured no faster on an idle host; it is there for hosts whose launch thread is contended.
 *   DINOV2_HIP_MAX_CHUNK=n   testing aid: split a predict call into passes of at most n images (the split that otherwise only
 *                            happens past 2^31 bytes of activations), to exercise that path at small sizes.
 *   The next four are testing aids that pick a kernel the library would otherwise choose by shape.  They are read ONCE, on first use
 *   (round 5; they used to be getenv() calls on every launch); a test that flips one inside a process uses dinov2_hip_op_set_tuning
 *   (include/dinov2_hip_ops.h), and dinov2_hip_op_gemm_plan reports which GEMM kernels a shape gets under the current setting.
 *   DINOV2_HIP_ATTN_V=1|2|3|4  force the throughput / the software-pipelined attention kernel (normally chosen by workgroup count; 3 and 4 =
 *                            the measured, never auto-selected 64-queries-per-wave variants: two waves per SIMD, and software-pipelined
 *                            with one wave per SIMD).  All give the same bits.
 *   DINOV2_HIP_ATTN_NWV=2|3|4  waves (32-query blocks) per workgroup of the software-pipelined attention kernel (normally 4; 2 for short
 *                            sequences); every size gives the same bits.
 *   DINOV2_HIP_GEMM_TILE=128|256   the small-tile kernel only / 256-row persistent tiles only.
 *   DINOV2_HIP_GEMM_GEN=2|4  which generation of the persistent GEMM runs the 256-row / mixed / one-tile-per-workgroup plans -- 2 = gemm2.hip
 *                            (eight waves, barrier-separated sections), 4 = gemm4.hip (four waves, hand-ordered K loop; the default for
 *                            K >= 1 024).  Both give every row the same bits.  (The LN-fold epilogues exist in gemm4.hip and the small-tile kernel only.)
 *   DINOV2_HIP_LIST_ORDER=1  (a fifth switch of that kind, "list_order") the attention work table of dinov2_hip_predict_list with the longest
 *                            images first instead of in list order; a measuring aid (profiles/predict_list.md), same bits.
 *   DINOV2_HIP_LN_FOLD=0|1   what dinov2_hip_load_opts.ln_fold = 0 ("the library's choice") resolves to; unset: off.
 *   DINOV2_HIP_GROUP_NO_AFFINITY=1  the group's worker threads are not bound to the CPUs local to their device.
 *   DINOV2_HIP_GROUP_REQUIRE_RCCL=1  dinov2_hip_group_create fails when librccl cannot be loaded instead of letting every device
 *                            read the GGUF itself.
 * (DINOV2_HIP_LIB, read by the Python binding only, points it at another build of this library.) */

#ifdef __cplusplus
}
#endif
#endif /* DINOV2_HIP_H */
