// Host-side model / session objects behind the C-ABI (include/dinov2_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/dinov2_hip.h"
#include "kernels.h"

namespace dinov2 {

struct LayerWeights {
    float *norm1_w, *norm1_b, *qkv_b, *o_b, *ls1, *norm2_w, *norm2_b, *fc1_b, *fc2_b, *ls2;
    void *qkv_w, *o_w, *fc1_w, *fc2_w;  // compute dtype, [N, K] row-major (ggml ne = [K, N])
    // LN fold (kernels.h): s[n] = sum_k gamma_k W[n, k], c[n] = bias[n] + sum_k beta_k W[n, k] of the QKV / FFN-in weights with the
    // LayerNorm in front of them; derived at load, part of the arena (so they travel with a weight broadcast)
    float *qkv_s = nullptr, *qkv_c = nullptr, *fc1_s = nullptr, *fc1_c = nullptr;
};

// A device allocation that a session owns and grows on demand through reserve() (host.h).
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    template <class T>
    T* as() const { return static_cast<T*>(ptr); }
};

// The side outputs of ONE pass of the forward.  Every run descriptor points at where image 0 of this pass goes; the distance from one requested
// layer's block to the next is that of the caller's WHOLE batch, so the passes of a split batch fill one set of buffers.  at_image(b0, ...) is
// the descriptor of the pass that starts at image b0 of the batch this one describes.  n == 0: off.

// The taps of dinov2_hip_predict_layers: device pointers into the first requested layer's block, and the strides (in floats) between blocks.
struct TapRun {
    const int32_t* layers = nullptr;  // [n] strictly ascending, each in [0, L]
    int n = 0;
    bool norm = false, chw = false;
    float *patch = nullptr, *cls = nullptr, *reg = nullptr;
    size_t patch_stride = 0, cls_stride = 0, reg_stride = 0;
    TapRun at_image(size_t b0, size_t P, size_t R, size_t H) const {  // an image is [P, H] / [H] / [R, H] of its layer's block
        TapRun t = *this;
        if (t.patch) t.patch += b0 * P * H;
        if (t.cls) t.cls += b0 * H;
        if (t.reg) t.reg += b0 * R * H;
        return t;
    }
};

// The attention rows of dinov2_hip_predict_attention: a device pointer into the first requested layer's block [B, heads, nq, nkeys], and the
// stride (in floats) between blocks.
struct AttnRun {
    const int32_t* layers = nullptr;   // [n] strictly ascending, each in [1, L]: the attention inside block layers[i]
    int n = 0;
    const int32_t* queries = nullptr;  // DEVICE [nq]
    int nq = 0, key0 = 0, nkeys = 0;
    float* probs = nullptr;
    size_t stride = 0;
    AttnRun at_image(size_t b0, size_t heads) const {
        AttnRun a = *this;
        if (a.probs) a.probs += b0 * heads * (size_t)nq * (size_t)nkeys;
        return a;
    }
};

// dinov2_hip_predict_dense.  During the forward, at requested layer i (slot i) dense_pack_kernel writes the f16 patch rows of this pass's images
// into columns [i * hblk, (i + 1) * hblk) of A [B P, K], hblk = H * (1 + concat_cls): the operand of the logits GEMM.  After it, dense_stage
// runs that GEMM into `lg` and reduces to the caller's outputs at image b0.  A, lg, lab and val are ONE pass's, in the session's dense scratch,
// reused by every pass; lab / val are where host labels / values are staged.
struct DenseRun {
    const dinov2_hip_dense_head* head = nullptr;
    const int32_t* layers = nullptr;  // the head's: [n] strictly ascending, each in [0, L]
    int n = 0;
    const dinov2_hip_dense_out* out = nullptr;
    size_t b0 = 0;  // first image of this pass within the caller's batch
    int oh = 0, ow = 0;
    _Float16* A = nullptr;
    float* lg = nullptr;
    uint8_t* lab = nullptr;
    float* val = nullptr;
    DenseRun at_image(size_t b) const {
        DenseRun d = *this;
        d.b0 += b;
        return d;
    }
};

struct PassExtras {
    TapRun taps;
    AttnRun attn;
    DenseRun dense;
    bool any() const { return taps.n > 0 || attn.n > 0 || dense.n > 0; }
    PassExtras at_image(size_t b0, size_t P, size_t R, size_t H, size_t heads) const {
        return PassExtras{taps.at_image(b0, P, R, H), attn.at_image(b0, heads), dense.at_image(b0)};
    }
};

// One run of a pass: B consecutive images of ONE network size h x w, embedded and pooled by one launch each.  A uniform batch is one run;
// a list (dinov2_hip_predict_list) has one per stretch of equal-sized images (list_plan).  The run owns rows [row0, row0 + B T) of the
// residual stream and of `fin`, rows [patch0, patch0 + B P) of `col`, and the slices of feat / logits / probs from image `image0` on.
struct PassRun {
    const float* img = nullptr;  // DEVICE: the run's images, contiguous
    int B = 0, h = 0, w = 0;
    const float* pos = nullptr;  // DEVICE: the position embedding [1 + P, H] of the run's patch grid
    int64_t row0 = 0, patch0 = 0;
    int image0 = 0;
    int P = 0, T = 0;  // patches and tokens (1 + R + P) of one image
};

// One pass of the forward: the runs, and what is the same for all of them.  Attention is the one launch that is not per row: without a work
// table it is launch_attention over runs[0] (a uniform batch), with one launch_attention_list over the table.  The extras are a uniform
// batch's only: forward() refuses a pass of several runs that carries any.
struct Pass {
    const PassRun* runs = nullptr;
    int nruns = 0;
    int M = 0;                        // token rows of all runs
    const AttnItem* items = nullptr;  // DEVICE: the list's attention work table (null: uniform over runs[0])
    int n_items = 0;
    int layout = 0;
    bool classify = false;
    int nlayers = 0;
    bool finalize = true;  // final LayerNorm (and the head with `classify`) after the layers
    PassExtras ex;
};

// The scratch buffers of a session, one DevBuf each in dinov2_hip_session::scratch: dinov2_hip_session_free frees them all.
enum Scratch : int {
    SCRATCH_WS = 0,  // the forward's workspace, carved into the views below
    SCRATCH_RAW,     // raw 8-bit images of DINOV2_HIP_U8_BGR_HWC host inputs
    SCRATCH_PCA,     // dinov2_hip_pca3
    SCRATCH_MATCH,   // dinov2_hip_match_tokens
    SCRATCH_BANK,    // dinov2_hip_bank_add / _topk / _keep (staged host rows, f16 queries, partials, results; the compaction's stage and indices)
    SCRATCH_DENSE,   // dinov2_hip_predict_dense (the f16 operand and the logits of one pass, host outputs' staging)
    SCRATCH_TAP,     // dinov2_hip_predict_layers with host outputs: where the tap kernel writes before the copy-out
    SCRATCH_ATTN,    // dinov2_hip_predict_attention with a host output: where attn_rows_kernel writes before the copy-out
    SCRATCH_ATTN_Q,  // the query list of the last dinov2_hip_predict_attention on the device (attn_q_host: what it holds)
    SCRATCH_LIST_POS,    // dinov2_hip_predict_list: the interpolated position embeddings of up to LIST_POS_GRIDS patch grids (list_pos: what it holds)
    SCRATCH_LIST_ITEMS,  // dinov2_hip_predict_list: the attention work table of the last list (list_items_host: what it holds)
    SCRATCH_KMEANS,      // dinov2_hip_kmeans_tokens (staged host rows, the f16 operands, the update's partials, the results)
    SCRATCH_SLIDE,       // dinov2_hip_predict_dense_slide (a host input's images, the window table, the window batch, every window's logits, host outputs' staging)
    SCRATCH_VLAD,        // dinov2_hip_vlad_tokens (staged host rows, the f16 operands, the tables, one pass's partials, the results)
    SCRATCH_PROPAGATE,   // dinov2_hip_propmem_set / dinov2_hip_propagate (staged host rows and labels, the f16 queries, the partial lists, the results)
    SCRATCH_NCUT,        // dinov2_hip_ncut_tokens (staged host rows, the f16 operand, the block and its partials, degrees)
    SCRATCH_CORESET,     // dinov2_hip_coreset_tokens (staged host rows, the f16 operand, s / nearest / marks, the partials, the results)
    SCRATCH_COUNT
};

}  // namespace dinov2

// replaces `struct dino_model` (/root/reference/dinov2.h:49-55): hparams + one device buffer + name->tensor map
struct dinov2_hip_model {
    dinov2_hip_hparams hp{};
    dinov2::DType dt = dinov2::DT_F16;
    int device = 0;
    bool quirk_const_div = true, quirk_pool_regs = true;
    bool ln_fold = false;      // LayerNorm 1 / 2 of every layer folded into the neighbouring GEMM epilogues (dinov2_hip_load_opts.ln_fold)
    int kpe = 0, kpe_pad = 0;  // patch-embed K (3*p*p) and its padding to a multiple of 64
    int patch_stride = 0;      // pixels from one patch to the next (dinov2_hip_load_opts.patch_stride, resolved: a divisor of patch_size)
    char* arena = nullptr;     // ONE allocation, like model.buffer (dinov2.cpp:341)
    size_t arena_bytes = 0;
    std::vector<dinov2::LayerWeights> layers;
    void* patch_w = nullptr;
    float *patch_b = nullptr, *cls = nullptr, *pos = nullptr, *reg = nullptr, *ln_w = nullptr, *ln_b = nullptr;
    void* head_w = nullptr;
    float* head_b = nullptr;
    std::vector<float> pos_host;  // the reference reads position_embeddings on the host every call (dinov2.cpp:935-938)
    std::vector<std::string> labels;
};

struct ProfRecord {
    int kind;
    hipEvent_t a, b;
};

// replaces the caller-owned ggml_gallocr_t (/root/reference/dinov2.h:111-112): stream + workspace + cached pos-embed
struct dinov2_hip_session {
    dinov2_hip_model* model = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    dinov2::DevBuf scratch[dinov2::SCRATCH_COUNT];  // every device allocation of the session, by dinov2::Scratch
    std::vector<int32_t> attn_q_host;               // what scratch[SCRATCH_ATTN_Q] holds
    int last_b = 0, last_h = 0, last_w = 0;  // shape of the last un-split forward (0: none): what dinov2_hip_fetch copies out
    bool last_classify = false;
    int last_first = 0, last_patches = 0;  // rows [last_first, last_first + last_patches) of image 0 in `fin`: its patch tokens
    int last_t = 0;  // tokens per image of that forward: image i of last_b starts at row i * last_t of `fin` (dinov2_hip_match_tokens)
    // carved views (valid for cur_* shape)
    int cur_b = 0, cur_h = 0, cur_w = 0;
    float *img = nullptr, *x = nullptr, *fin = nullptr, *feat = nullptr, *logits = nullptr, *probs = nullptr,
          *pos = nullptr;
    void *col = nullptr, *ln = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr;
    float* stats = nullptr;  // LN fold: [M][ln_stat_slots(H)][2] row statistics of the residual stream (slots past H / 64 stay zero)
    int pos_h = -1, pos_w = -1;  // grid the cached interpolated pos-embed in `pos` belongs to
    std::vector<float> pos_stage;
    // dinov2_hip_predict_list.  The workspace is carved by (pixels, patches, rows, images) instead of (B, h, w): list_key holds those four while
    // the carve is a list's (cur_b is then -1, so the next uniform predict carves anew), and is cleared by a uniform carve.
    int64_t list_key[4] = {0, 0, 0, 0};
    struct ListPos {  // one cached position embedding [1 + h0 w0, H] f32 at float offset `off` of scratch[SCRATCH_LIST_POS]
        int h0, w0;
        size_t off;
    };
    std::vector<ListPos> list_pos;
    size_t list_pos_used = 0;                      // floats of scratch[SCRATCH_LIST_POS] taken by list_pos
    std::vector<float> list_pos_stage;             // host side of the uploads (never rewritten while a copy from it may be in flight)
    std::vector<dinov2::AttnItem> list_items_host;  // what scratch[SCRATCH_LIST_ITEMS] holds
    std::vector<int> slide_tab_host;                // the window table at the front of scratch[SCRATCH_SLIDE] (dinov2_hip_predict_dense_slide)
    // hipGraph cache (the "allocr reuse" of the reference taken one step further): a forward that repeats with the same
    // shape, input pointer and workspace is captured once and replayed; 178 launches become one graph launch
    struct GraphEntry {
        const void* ws;
        const void* img;
        int b, h, w, layout, classify, uses;
        hipGraphExec_t exec;
    };
    std::vector<GraphEntry> graphs;
    // profiling
    bool profiling = false;
    std::vector<ProfRecord> records;
    std::vector<hipEvent_t> free_events;
    std::vector<double> prof_ms;
    std::vector<int> prof_n;
};

// A resident bank of normalised f16 rows (dinov2_hip_bank_*): one device allocation [cap_pad, hpad], never moved; rows [0, count) are valid.
// It keeps the device ordinal only, so it may outlive the model it was created with.
struct dinov2_hip_bank {
    int device = 0;
    int H = 0, hpad = 0, capacity = 0, cap_pad = 0, count = 0;
    _Float16* rows = nullptr;
};

// A resident memory of frames for label propagation (dinov2_hip_propmem_*, dinov2_hip_propagate): one device allocation laid out by
// dinov2::propmem_layout, made at create and never moved -- the f16 rows of `frames` slots of one h0 x w0 grid, each padded to whole tiles,
// their f32 labels, the kept result of the last propagate and the cell table.  `filled`: bit f = slot f holds a frame; has_kept: `kept` holds
// the result of a propagate with keep.  It keeps the device ordinal only, so it may outlive the model it was created with.
struct dinov2_hip_propmem {
    int device = 0;
    int H = 0, hpad = 0, h0 = 0, w0 = 0, P = 0, ppad = 0, frames = 0, C = 0;
    uint64_t filled = 0;
    bool has_kept = false;
    dinov2::PropMemLayout lay{};
    char* dev = nullptr;
};

// A resident linear dense-prediction head (dinov2_hip_dense_head_*): one device allocation made at create -- the f16 weight [cpad, K] with zero
// rows past C, the bias [cpad] (zeros without one) and the bin centres [cpad] -- never moved.  It keeps the device ordinal and the two sizes of
// the model it was created for, so it may outlive that model.
struct dinov2_hip_dense_head {
    int device = 0;
    int H = 0, L = 0;  // hidden size and number of blocks of the model it was created for
    int n_layers = 0;
    int32_t layers[dinov2::DENSE_LAYERS_MAX] = {};
    bool norm = false, concat_cls = false;
    int C = 0, cpad = 0, K = 0, reduce = 0;
    float eps = 0.0f;
    char* dev = nullptr;
    _Float16* w16 = nullptr;
    float *bias = nullptr, *centers = nullptr;
};

// Internal (not C-ABI) helpers shared by model.cpp and group.cpp (host.h has those of the other host files).
// Argument checks of dinov2_hip_predict that need no session: layout, batch, height / width against the patch size and stride.
int dinov2_check_input(const dinov2_hip_model* m, const dinov2_hip_input* in, char* err, size_t errlen);
// ... and, for raw 8-bit input, its network size under `flags` against the grid (224 x 224 with DINOV2_HIP_CLASSIFY, whatever the patch size)
int dinov2_check_input_grid(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen);
// After it: ONE image of `in` (at its network size under `flags`) must fit a pass -- token rows * widest activation row * 2 bytes below 2^31,
// the 32-bit staging cursors of the GEMMs and the attention.  dinov2_max_pass_batch only cuts a batch into images; an image is not cut.
int dinov2_check_pass_rows(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen);
// dinov2_check_input_grid, then dinov2_check_pass_rows: what every predict entry point checks of its input before anything is allocated or launched
int dinov2_check_input_rows(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen);
// Largest batch ONE pass of the forward takes at network input size h x w (32-bit activation offsets; DINOV2_HIP_MAX_CHUNK lowers it for
// tests): dinov2_hip_predict cuts longer batches into passes and leaves nothing for dinov2_hip_fetch.
size_t dinov2_max_pass_batch(const dinov2_hip_model* m, int h, int w);
