// Launcher interface of the hand-written gfx950 kernels (gemm.hip, attention.hip, kernels_misc.hip).
// All launchers enqueue on `stream` and return hipGetLastError(); none of them allocates or syncs.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace dinov2 {

enum DType : int { DT_F16 = 0, DT_BF16 = 1 };

// GEMM epilogues.  C[m,n] = sum_k A[m,k] * W[n,k] (f32 accumulate), then:
enum Epilogue : int {
    EPI_PATCH = 0,   // x[b*T + 1+R+p, n] = acc + bias[n] + pos[1+p, n]           (f32 out; m = b*P + p)
    EPI_QKV = 1,     // out[m, n] = T((acc + bias[n]) * (n < qcols ? qscale : 1))  (T out)
    EPI_RESID = 2,   // x[m, n] += ls[n] * (acc + bias[n])                         (f32 in/out)
    EPI_GELU = 3,    // out[m, n] = T(f16(gelu_tanh(f16(acc + bias[n]))))          (T out; ggml f16-LUT contract)
    EPI_SWIGLU = 4,  // out[m, j] = T(silu(h1) * h2), rows of W interleaved in 32-blocks x1|x2 (T out, width N/2)
    EPI_PLAIN_F32 = 5,  // out[m, n] = acc + bias[n]                                (f32 out; tests / head)
    // ---- LayerNorm folded into the GEMMs on either side of it ("LN fold"; replaces ggml_norm + mul + add,
    // /root/reference/dinov2.cpp:694-700, 722-728, as separate launches).  With LN(x) = gamma (x - mu) r + beta feeding a weight matmul,
    //     sum_k LN(x)[m,k] W[n,k] + b[n]  =  r_m (sum_k (gamma_k x[m,k]) W[n,k]  -  mu_m s[n]) + c[n],
    //     s[n] = sum_k gamma_k W[n,k],   c[n] = b[n] + sum_k beta_k W[n,k]           (both computed once, at load time)
    // so the PRODUCER of x (the residual epilogue) also writes the operand T(gamma x) and per-row partial sums, and the CONSUMER
    // (QKV / FFN-in) applies r_m, mu_m, s, c in its epilogue.
    EPI_RESID_LN = 6,   // EPI_RESID, plus: xg[m, n] = T(x[m, n] * ln_gamma[n]);  stats[m][n / 64] = (sum, sum of squares) of x[m, 64 g .. 64 g + 63]
    EPI_QKV_LN = 7,     // v = r_m * (acc - mu_m * ln_s[n]) + ln_c[n], then as EPI_QKV / EPI_GELU / EPI_SWIGLU with v in place of acc + bias[n]
    EPI_GELU_LN = 8,
    EPI_SWIGLU_LN = 9
};
// the epilogue an LN-fold variant specialises (dispatch decisions depend on this one only)
inline Epilogue epi_base(Epilogue e) {
    return e == EPI_RESID_LN ? EPI_RESID : e == EPI_QKV_LN ? EPI_QKV : e == EPI_GELU_LN ? EPI_GELU : e == EPI_SWIGLU_LN ? EPI_SWIGLU : e;
}
inline bool epi_ln_consumer(Epilogue e) { return e == EPI_QKV_LN || e == EPI_GELU_LN || e == EPI_SWIGLU_LN; }
constexpr int EPI_COUNT = 10;
constexpr int LN_GROUP = 64;      // columns per partial-sum group of EPI_RESID_LN's row statistics
constexpr int LN_MAX_GROUPS = 24; // hidden sizes up to 1 536 (ViT-g); larger models keep the LayerNorm launches
inline int ln_stat_slots(int hidden) { return hidden / LN_GROUP <= 12 ? 12 : 24; }  // slots per row of the statistics buffer (device_types.h, ln_row_load)

// ---- the geometry limits of the row kernels, stated once: the launchers below refuse what is outside them, and dinov2_hip_model_load refuses
// a model that would reach such a launch (include/dinov2_hip.h, "Supported geometry") ----
// LayerNorm, layer tap, ln_prepare and dense_pack keep one token row in the registers of one wave: at most 8 float4 per lane of 64.
constexpr int LN_MAX_WIDTH = 64 * 4 * 8;
// im2col lays IM2COL_CHUNK patches of Kpad two-byte elements out in LDS (64 KiB per workgroup), divides a pixel column by 3 through a
// multiplication that is exact below 32 768, and by the patch size through one that must be exact for every column of the chunk.
constexpr int IM2COL_CHUNK = 10;
inline bool im2col_patch_ok(int patch, int Kpad) {
    if (patch <= 0 || 3LL * IM2COL_CHUNK * patch >= 32768) return false;  // (first: the loader hands over any 32-bit patch_size)
    if (Kpad % 8 != 0 || (long long)Kpad < 3LL * patch * patch) return false;
    if ((size_t)IM2COL_CHUNK * Kpad * 2 > 64 * 1024) return false;
    for (unsigned x = 0, mg = 65536u / (unsigned)patch + 1u; x < (unsigned)(IM2COL_CHUNK * patch); ++x)
        if (((x * mg) >> 16) != x / (unsigned)patch) return false;
    return true;
}
// the largest patch size whose K = 3 p^2, padded to a multiple of 64 as the loader pads it, im2col takes (32: Kpad = 3 072, 60 KiB of LDS;
// 33 needs Kpad = 3 328, 65 KiB)
inline int im2col_max_patch() {
    int p = 0;
    while (im2col_patch_ok(p + 1, (3 * (p + 1) * (p + 1) + 63) / 64 * 64)) ++p;
    return p;
}
// ---- the patch grid of an image, stated once for the host and the kernels' launchers: patches of `patch` pixels every `stride` pixels
// (dinov2_hip_load_opts.patch_stride; stride == patch: the reference's conv_2d_sk_p0).  The callers check px >= patch and
// (px - patch) % stride == 0; with stride | patch every multiple of the patch size passes.
inline int grid_dim(int px, int patch, int stride) { return px < patch ? 0 : (px - patch) / stride + 1; }
// The strided im2col (launch_im2col_stride) stages the image strip under a run of patches of one grid row -- 3 patch image rows of
// (np - 1) stride + patch pixels -- in LDS and gathers every col row from it.  A run is as many patches as a strip of IM2COL_CHUNK patch
// widths covers (stride == patch: IM2COL_CHUNK patches; patch 14, stride 7: 19; stride 1: 127), so the strip, and the LDS it takes, do not
// depend on the stride.
inline int im2col_stride_run(int patch, int stride) { return (IM2COL_CHUNK - 1) * patch / stride + 1; }
// elements from one strip row to the next in LDS: the strip's width up to an ODD number of dwords, so that the strip rows which the
// consecutive 16-byte pieces of a col row walk (row k / patch, every `patch` elements a new one) start in different banks
inline int im2col_stride_pitch(int patch, int stride) {
    const int width = (im2col_stride_run(patch, stride) - 1) * stride + patch;
    return (((width + 1) / 2) | 1) * 2;
}
// What the strided kernel takes: stride divides patch (the option's rule: the strip then starts on a stride boundary whatever the run, and
// every multiple of the patch size is a valid input size); the strip fits the 64 KiB of LDS that need no attribute (the CU has 160 KiB; the
// existing kernel stays under 64 as well); an interleaved strip row divides its element index by 3 through a multiplication that is exact
// below 32 768; a col piece divides its first element index k < Kpad by the patch size through (k * magic) >> 20, which must be exact and
// stay inside 32 bits.
inline bool im2col_stride_ok(int patch, int stride, int Kpad) {
    if (patch <= 0 || stride <= 0 || stride > patch || patch % stride != 0) return false;
    if (3LL * IM2COL_CHUNK * patch >= 32768) return false;
    if (Kpad % 8 != 0 || (long long)Kpad < 3LL * patch * patch || Kpad > (1 << 20)) return false;
    if ((size_t)3 * patch * im2col_stride_pitch(patch, stride) * 2 > 64 * 1024) return false;
    const unsigned long long mg = (1ull << 20) / (unsigned)patch + 1ull;
    for (unsigned long long k = 0; k < (unsigned long long)Kpad; k += 8)
        if (k * mg >= (1ull << 32) || ((k * mg) >> 20) != k / (unsigned)patch) return false;
    return true;
}

struct GemmArgs {
    const void* A;      // [M, K]  T, row-major, K % 64 == 0
    const void* W;      // [N, K]  T, row-major (ggml ne = [K, N])
    const float* bias;  // [N] or nullptr
    void* out;
    const float* aux;   // EPI_PATCH: pos [1+P, N]; EPI_RESID: layer-scale lambda [N]
    int M, N, K;
    int lda, ldw;       // row strides of A and W in elements; 0 = K (dense)
    int ldo;            // leading dimension of out in elements
    int P, T, R;        // EPI_PATCH token mapping
    int qcols;          // EPI_QKV: columns [0, qcols) are multiplied by qscale
    float qscale;
    // The next four are written by the planner (gemm_plan), never read from the caller.  They stay members because this struct is the kernels'
    // parameter block and its layout is fixed.
    int small_only;     // unused (no kernel reads it); once steered launch_gemm's recursion.  Always 0 in a plan
    int nt_out;         // 2-byte outputs leave with non-temporal stores (set when the output is larger than the L2s); one value per logical output
    int sub;            // unused (no kernel reads it); once marked the parts of a split launch.  Always 0 in a plan
    int clk_slot;       // the clock-probe slot of the LOGICAL launch (device_types.h), decided before any split
    // ---- LN fold (EPI_RESID_LN and the *_LN consumers).  Row statistics: stats[(m * ln_gs + g) * 2 + {0, 1}] = sum / sum of squares
    // of x[m, 64 g .. 64 g + 63] (f32, a fixed pairwise tree over the 64 columns: every kernel produces the same bits); ln_gs = slots per
    // row = ln_stat_slots(hidden): 12 or 24, the slots past hidden / 64 zero (set once, never written)
    int ln_gs;
    const float* ln_gamma;  // EPI_RESID_LN: weight [N] of the LayerNorm that FOLLOWS this residual update
    void* xg;               // EPI_RESID_LN: [M, N] T, T(x * ln_gamma) -- the consumer's A operand
    float* stats;           // EPI_RESID_LN: written ([M][N / 64][2]); consumers: read ([M][K / 64][2])
    const float* ln_s;      // consumers: s[n] = sum_k gamma_k W[n, k]
    const float* ln_c;      // consumers: c[n] = bias[n] + sum_k beta_k W[n, k]   (`bias` is not read)
    float ln_eps;           // consumers: LayerNorm epsilon
};

using GemmKernelFn = void (*)(GemmArgs);             // a kernel of gemm.hip / gemm2.hip / gemm4.hip
using GemmKernelFn2 = void (*)(GemmArgs, GemmArgs);  // a two-height kernel (gemm2_mixed_kernel, gemm4_mixed_kernel)
// raises a kernel's dynamic-LDS limit (the *_init functions); a null kernel = an epilogue its family does not instantiate
inline hipError_t gemm_raise_lds(const void* kernel, size_t bytes) {
    return kernel ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) : hipSuccess;
}

// ---- the plan of one GEMM: which kernels run it and which part of the output each of them covers.  Plain data, filled by gemm_plan without
// touching the device; launch_gemm launches its steps in order, gemm_plan_describe prints them, tests/test_gemm_plans.py checks on the CPU
// that the parts tile the output exactly once.
enum GemmFamily : int {
    GEMM_SMALL = 0,    // gemm.hip, the small-tile kernel; `cfg` names the configuration
    GEMM2 = 1,         // gemm2.hip, `tile`-row tiles (256 | 192 persistent, 128 one per workgroup)
    GEMM2_MIXED = 2,   // gemm2.hip, 256-row tiles for args[0], then 192-row tiles for args[1], one launch
    GEMM4 = 3,         // gemm4.hip, 256-row tiles
    GEMM4_MIXED = 4,   // gemm4.hip, as GEMM2_MIXED (args[0] may be empty: 192-row tiles only)
    GEMM4_SHORT = 5    // gemm4.hip, `tile`-row tiles (64 | 96 | 128), one per workgroup
};
struct GemmStep {
    GemmFamily family;
    int tile;                    // tile height in rows (0 for GEMM_SMALL)
    int cfg;                     // GEMM_SMALL: index into gemm.hip's list of small-tile configurations
    int row0, rows, col0, cols;  // the rectangle of the output this step covers
    int rows0;                   // rows [row0, row0 + rows0) are args[0]; the rest, for the two-height kernels only, args[1]
    GemmArgs args[2];            // what the kernel is launched with: slices of GemmPlan::whole over those ranges
};
constexpr int GEMM_PLAN_MAX_STEPS = 4;  // the deepest plan has three: "gemm2<256>;small<..>;small<..>" (column split, then a row split of the first part)
struct GemmPlan {
    GemmArgs whole;  // the caller's arguments, validated, with nt_out / clk_slot / ln_gs decided once for all steps
    int nsteps;      // 0 for a refused shape
    GemmStep steps[GEMM_PLAN_MAX_STEPS];
};
// Launches nothing and calls no device API.  hipErrorInvalidValue for shapes launch_gemm refuses; check_pointers = false for plan queries,
// which carry no pointers (none is dereferenced either way; a null pointer stays null in every slice).
hipError_t gemm_plan(DType dt, Epilogue epi, const GemmArgs& a, bool check_pointers, GemmPlan* out);

// gemm_plan (with pointer checks), then its steps in order, stopping at the first error
hipError_t launch_gemm(DType dt, Epilogue epi, const GemmArgs& a, hipStream_t stream);
// must be called once per device before the first launch_gemm (raises the dynamic-LDS limit)
hipError_t gemm_init();
// Which kernel(s) launch_gemm would run for this problem: gemm_plan without pointer checks, the step names joined by ';', e.g.
// "gemm4_mixed<256+192>" or "gemm4<256>;small<64x128,w2x2,st3,ks1>".  Returns hipErrorInvalidValue and an empty text
// for shapes launch_gemm refuses.  The CPU-side coverage test enumerates the model shapes with it (tests/test_gemm_plans.py).
hipError_t gemm_plan_describe(DType dt, Epilogue epi, const GemmArgs& a, char* out, size_t cap);

// Testing aids that used to be read from the environment on every launch: read ONCE (first use), changed afterwards only through
// tune_set (dinov2_hip_op_set_tuning, include/dinov2_hip_ops.h).  0 = the library's own choice.
enum TuneKey : int {
    TUNE_GEMM_GEN = 0,   // DINOV2_HIP_GEMM_GEN: 2 | 4 = force that generation of the persistent GEMM wherever it can run
    TUNE_GEMM_TILE = 1,  // DINOV2_HIP_GEMM_TILE: 128 | 256 (tuning builds: 129 | 192)
    TUNE_ATTN_V = 2,     // DINOV2_HIP_ATTN_V: 1 .. 4
    TUNE_ATTN_NWV = 3,   // DINOV2_HIP_ATTN_NWV: 2 | 3 | 4
    TUNE_LIST_ORDER = 4, // DINOV2_HIP_LIST_ORDER: 1 = the attention table of dinov2_hip_predict_list with the longest images first (a measuring aid; same bits)
    TUNE_COUNT = 5
};
int tune_get(TuneKey k);
void tune_set(TuneKey k, int v);

// y[r, :] = T(((x - mean) * rsqrt(var + eps)) * w + b)     x f32 [rows, H]; one wave per row
hipError_t launch_layernorm(DType dt, const float* x, const float* w, const float* b, void* y, int rows, int H,
                            float eps, hipStream_t stream);
// same, f32 output (final layernorm)
hipError_t launch_layernorm_f32(const float* x, const float* w, const float* b, float* y, int rows, int H, float eps,
                                hipStream_t stream);
// Layer tap (dinov2_hip_predict_layers): tokens of the residual stream x [B*T, H] f32 to up to three destinations, any of them nullptr:
// cls_out [B, H] (token 0), reg_out [B, R, H] (tokens 1 .. R), patch_out (tokens 1 + R .. T - 1) as [B, P, H] or, `chw`, [B, H, P].
// `norm`: through LayerNorm (w, b, eps) with the bits of launch_layernorm_f32; otherwise the rows as they are.  H % 4 == 0, H <= 2 048, P >= 1.
hipError_t launch_layer_tap(const float* x, const float* w, const float* b, float eps, int B, int T, int R, int H, bool norm, bool chw,
                            float* patch_out, float* cls_out, float* reg_out, hipStream_t stream);
// LN fold (EPI_RESID_LN): what the residual epilogue leaves behind, computed from a residual stream no GEMM has written (before layer 0):
// xg [rows, H] T = T(x gamma), stats [rows][gs][2] = (sum, sum of squares) per 64 columns in the producers' summation order (gs = ln_stat_slots(H))
hipError_t launch_ln_prepare(DType dt, const float* x, const float* gamma, void* xg, float* stats, int gs, int rows, int H, hipStream_t stream);
// load time: s[n] = sum_k gamma[k] W[n, k], c[n] = bias[n] + sum_k beta[k] W[n, k]   (W [N, K] T, dense; bias may be nullptr)
hipError_t launch_ln_fold_vectors(DType dt, const void* W, const float* bias, const float* gamma, const float* beta, float* s, float* c, int N, int K,
                                  hipStream_t stream);
// fused multi-head attention over token-major qkv [B*T, 3H] (T dtype, q pre-scaled), out [B*T, H]; hd == 64.
// log2_scores: q was scaled by log2(e)/sqrt(hd) instead of 1/sqrt(hd), so softmax uses exp2 directly.
hipError_t launch_attention(DType dt, const void* qkv, void* out, int B, int T, int H, int nh, bool log2_scores,
                            hipStream_t stream);
// ---- a list of images of different sizes in one forward (dinov2_hip_predict_list; contract in include/dinov2_hip.h).  The residual stream
// holds the images' token rows one after the other: image i owns rows [row0, row0 + T).  Everything but attention works per row and takes
// M = sum T_i; attention runs over a device table with one entry per workgroup.
struct AttnItem {  // one workgroup of launch_attention_list: 128 queries [128 qb, 128 qb + 128) of head `head` of the image at rows [row0, row0 + T)
    int32_t row0, T, head, qb;
};
struct ListImage {
    int64_t row0;     // first row of the image in the residual stream
    int32_t T, P;     // tokens (1 + R + P) and patches (h0 w0)
    int32_t h0, w0;   // patch grid
};
struct ListRun {  // a run of consecutive images of one network size: embedded and pooled by one launch each, with B = count
    int32_t first, count;
};
constexpr int ATTN_LIST_QB = 128;  // queries per workgroup of the list kernels (four waves of 32)
// The sizes of a plan; list_plan fills the arrays the caller gives it (any may be null: counts only).  Launches nothing, needs no device.
struct ListPlan {
    int64_t M;        // total rows, sum T_i
    int64_t P;        // total patches
    int64_t pixels;   // sum h_i w_i (network sizes)
    int64_t units;    // attention work items = sum ceil(T_i / 128) nh
    int32_t nruns;
};
// h[i], w[i]: NETWORK sizes in pixels (the callers check them against `patch` and `stride`: grid_dim).  items: [units], images: [n], runs: [<= n].
// Table order: image-major, then head, then query block -- after xcd_remap over the table's length all query blocks of an (image, head) sit
// on one XCD, except where the boundary between two XCD ranges falls inside one.  The images come in list order (LIST_ORDER_AS_GIVEN) or by
// descending T, equal T in list order (LIST_ORDER_LONGEST_FIRST); the order changes no bit of any result.  The table holds row0 in 32 bits:
// ask for it only where M < 2^31 (one pass is far below).
enum ListOrder : int { LIST_ORDER_AS_GIVEN = 0, LIST_ORDER_LONGEST_FIRST = 1 };
inline ListPlan list_plan(int n, const int32_t* h, const int32_t* w, int patch, int stride, int R, int nh, int order, ListImage* images,
                          ListRun* runs, AttnItem* items) {
    ListPlan p{};
    std::vector<std::pair<int32_t, int64_t>> seg(items ? (size_t)n : 0);  // (T, row0) per image, for the table
    for (int i = 0; i < n; ++i) {
        const int h0 = grid_dim(h[i], patch, stride), w0 = grid_dim(w[i], patch, stride);
        const int P = h0 * w0, T = 1 + R + P;
        if (images) images[i] = ListImage{p.M, T, P, h0, w0};
        if (items) seg[(size_t)i] = {T, p.M};
        if (i == 0 || h[i] != h[i - 1] || w[i] != w[i - 1]) {
            if (runs) runs[p.nruns] = ListRun{i, 0};
            ++p.nruns;
        }
        if (runs) ++runs[p.nruns - 1].count;
        p.units += (int64_t)((T + ATTN_LIST_QB - 1) / ATTN_LIST_QB) * nh;
        p.M += T;
        p.P += P;
        p.pixels += (int64_t)h[i] * w[i];
    }
    if (!items) return p;
    if (order == LIST_ORDER_LONGEST_FIRST)
        std::stable_sort(seg.begin(), seg.end(), [](const std::pair<int32_t, int64_t>& a, const std::pair<int32_t, int64_t>& b) { return a.first > b.first; });
    AttnItem* it = items;
    for (const auto& s : seg) {
        const int nqb = (s.first + ATTN_LIST_QB - 1) / ATTN_LIST_QB;
        for (int hd = 0; hd < nh; ++hd)
            for (int qb = 0; qb < nqb; ++qb) *it++ = AttnItem{(int32_t)s.second, s.first, hd, qb};
    }
    return p;
}
// The list form of launch_attention: qkv [sum T_i, 3H], out [sum T_i, H]; items_dev: DEVICE table of n_items entries (list_plan); `units` =
// n_items picks the kernel as launch_attention does on its own count (version 2 up to 512, else 1; TUNE_ATTN_V forces 1 or 2, other values
// are refused: versions 3 and 4 and the 2- and 3-wave workgroups have no list form).  Each image is, bit for bit, launch_attention on its
// rows alone (B = 1).  The 32-bit staging cursors are relative to the image's first row: T_i 3H 2 < 2^32 per image (the caller checks).
hipError_t launch_attention_list(DType dt, const void* qkv, void* out, const AttnItem* items_dev, int n_items, long units, int H, int nh,
                                 bool log2_scores, hipStream_t stream);
// Attention rows (dinov2_hip_predict_attention; attn_rows.hip): out [B, nh, nq, nkeys] f32 = columns [key0, key0 + nkeys) of the softmax rows of
// the query tokens queries[0 .. nq) (DEVICE pointer, each in [0, T)), from the same token-major qkv (row stride ld elements, q pre-scaled by
// log2(e)/sqrt(hd): exp2).  The softmax runs over all T keys whatever the columns; a row's bits depend on T and on its own q and k only.
hipError_t launch_attn_rows(DType dt, const void* qkv, int ld, float* out, int B, int T, int H, int nh, const int32_t* queries, int nq, int key0,
                            int nkeys, hipStream_t stream);
// same with the LDS the scores may take (bytes) given by the caller: below 4 T the two-pass form runs (a testing aid; same bits)
hipError_t launch_attn_rows_budget(DType dt, const void* qkv, int ld, float* out, int B, int T, int H, int nh, const int32_t* queries, int nq,
                                   int key0, int nkeys, size_t lds_budget, hipStream_t stream);

// im2col of conv_2d_sk_p0: img f32 (layout 0 = BGR HWC interleaved, 1 = RGB CHW planar) -> col [B*P, Kpad] T,
// patch vector order (c_rgb, ky, kx), zero padded to Kpad
hipError_t launch_im2col(DType dt, const float* img, void* col, int B, int Hh, int Ww, int patch, int Kpad, int layout,
                         hipStream_t stream);
// the same with patches every `stride` pixels (dinov2_hip_load_opts.patch_stride): col [B * h0 * w0, Kpad], h0 = grid_dim(Hh, patch, stride),
// row = (b h0 + y) w0 + x, the same patch vector order, padding and single rounding.  im2col_stride_ok(patch, stride, Kpad), Hh, Ww >= patch.
hipError_t launch_im2col_stride(DType dt, const float* img, void* col, int B, int Hh, int Ww, int patch, int stride, int Kpad, int layout,
                                hipStream_t stream);
// dino_preprocess / dino_classify_preprocess on the device: u8 BGR [B,h,w,3] -> normalised f32 BGR [B,oh,ow,3]
// (bicubic to rh x rw, crop at (y0, x0))
hipError_t launch_preprocess_u8(const uint8_t* src, float* dst, int B, int h, int w, int rh, int rw, int y0, int x0, int oh,
                                int ow, hipStream_t stream);
// x[b*T + 0] = cls + pos[0]; x[b*T + 1 + r] = reg[r]
hipError_t launch_init_tokens(float* x, const float* cls, const float* pos, const float* reg, int B, int T, int R,
                              int H, hipStream_t stream);

// load-time conversion of one GGUF tensor: src (ggml type) rows [N, K] -> dst T [N, Kpad], zero padded.
// interleave32 > 0: destination row order x1|x2 interleaved in 32-row blocks (SwiGLU weights_in), value = F.
hipError_t launch_convert_weight(DType dt, const void* src, uint32_t ggml_type, void* dst, int N, int K, int Kpad,
                                 int interleaveF, hipStream_t stream);
// f32 vector copy with the same optional interleave (bias of weights_in)
hipError_t launch_permute_bias(const float* src, float* dst, int N, int interleaveF, hipStream_t stream);

// classifier head (forward_head): fin = final-LN tokens f32 [B, T, H]
//   pooled[b, h] = sum_{t in [first, T)} fin[b, t, h] * inv_div ; feat = [cls ; pooled] rounded to T
//   logits = W feat + bias ; probs = softmax(logits)
hipError_t launch_head(DType dt, const float* fin, const void* W, const float* bias, float* feat_scratch,
                       float* logits, float* probs, int B, int T, int H, int C, int first, float inv_div,
                       hipStream_t stream);

// PCA support: mean[h] = column mean of tok [P, H]; xt [H, Ppad] f16 = (tok - mean)^T, zero padded in P
hipError_t launch_pca_prepare(const float* tok, float* mean, void* xt, int P, int H, int Ppad, hipStream_t stream);
// Ppad: the K of the covariance GEMM, a multiple of 64 with an even K / 64
inline int pca_ppad(int P) { return (P + 127) / 128 * 128; }
// cov [H, H] f32 = Xt Xt^T (= P times the covariance): one plain GEMM whose two operands are the same [H, Ppad] f16 matrix
inline hipError_t launch_pca_cov(const void* xt, float* cov, int H, int Ppad, hipStream_t stream) {
    GemmArgs a{};
    a.A = xt; a.W = xt; a.out = cov; a.M = H; a.N = H; a.K = Ppad; a.ldo = H;
    return launch_gemm(DT_F16, EPI_PLAIN_F32, a, stream);
}

// Block iteration for the leading eigenvectors of cov [H, H] (see pca_power_kernel): block width, rows per workgroup, grid size
constexpr int PCA_NB = 8, PCA_ROWS = 16;
inline int pca_blocks(int H) { return (H + PCA_ROWS - 1) / PCA_ROWS; }
// g [8][8] = Y^T Y  ->  rinv [8][8] upper triangular with Y rinv orthonormal (g = R^T R).  A direction whose pivot falls below
// 1e-24 of the largest diagonal entry is dropped (its column of rinv is zero), so rank-deficient blocks stay finite.  Shared by
// the kernel and the host-side Rayleigh-Ritz step so that both see the same Q.
__host__ __device__ inline void pca_chol_rinv(const double* g, double* rinv) {
    double R[PCA_NB][PCA_NB];
    bool dead[PCA_NB];
    double big = 0.0;
    for (int a = 0; a < PCA_NB; ++a) big = g[a * PCA_NB + a] > big ? g[a * PCA_NB + a] : big;
    for (int a = 0; a < PCA_NB; ++a) {
        double d = g[a * PCA_NB + a];
        for (int k = 0; k < a; ++k) d -= R[k][a] * R[k][a];
        dead[a] = !(d > 1e-24 * big);
        const double inv = dead[a] ? 0.0 : 1.0 / sqrt(d);
        for (int b = 0; b < PCA_NB; ++b) R[a][b] = 0.0;
        if (dead[a]) continue;
        R[a][a] = d * inv;
        for (int b = a + 1; b < PCA_NB; ++b) {
            double v = g[a * PCA_NB + b];
            for (int k = 0; k < a; ++k) v -= R[k][a] * R[k][b];
            R[a][b] = v * inv;
        }
    }
    for (int a = 0; a < PCA_NB; ++a)
        for (int b = 0; b < PCA_NB; ++b) rinv[a * PCA_NB + b] = 0.0;
    for (int a = 0; a < PCA_NB; ++a) {
        if (dead[a]) continue;
        rinv[a * PCA_NB + a] = 1.0 / R[a][a];
        for (int b = a + 1; b < PCA_NB; ++b) {
            if (dead[b]) continue;
            double v = 0.0;
            for (int k = a; k < b; ++k) v += rinv[a * PCA_NB + k] * R[k][b];
            rinv[a * PCA_NB + b] = -v / R[b][b];
        }
    }
}
hipError_t launch_pca_power(const float* cov, const double* yprev, const double* gprev, double* ynext, double* gnext, int H,
                            hipStream_t stream);
hipError_t launch_pca_project(const float* tok, const float* mean, const float* comp, float* proj, int P, int H,
                              hipStream_t stream);

// Nearest rows by cosine similarity, both directions from one pass (csrc/match.hip; contract in include/dinov2_hip.h, dinov2_hip_match).
// Tile of match_kernel, and the tiles per side of one pass: a longer side is walked in passes of MATCH_PASS tiles, which bounds the
// partials at 2 * MATCH_PASS * (MATCH_PASS * 128) * 8 bytes = 32 MiB whatever na and nb.
constexpr int MATCH_TM = 128, MATCH_TN = 128, MATCH_PASS = 128;
// Where everything sits in the caller's workspace (256-byte aligned offsets; `bytes` = its size).  The four results are DEVICE arrays there.
struct MatchPlan {
    int na_pad, nb_pad, hpad;  // rows to whole tiles, H to a multiple of 64
    size_t a16, b16;           // normalised f16 operands [na_pad, hpad], [nb_pad, hpad]
    size_t prow_v, prow_i;     // per (column tile of the pass, row of the pass): best value / column
    size_t pcol_v, pcol_i;     // per (row tile of the pass, column of the pass): best value / row
    size_t idx_ab, sim_ab, idx_ba, sim_ba;  // [na], [na], [nb], [nb]
    size_t bytes;
};
inline MatchPlan match_plan(int na, int nb, int H) {
    MatchPlan p{};
    p.na_pad = (na + MATCH_TM - 1) / MATCH_TM * MATCH_TM;
    p.nb_pad = (nb + MATCH_TN - 1) / MATCH_TN * MATCH_TN;
    p.hpad = (H + 63) / 64 * 64;
    const size_t pr = (size_t)(p.na_pad < MATCH_PASS * MATCH_TM ? p.na_pad : MATCH_PASS * MATCH_TM);  // rows / columns of one pass
    const size_t pc = (size_t)(p.nb_pad < MATCH_PASS * MATCH_TN ? p.nb_pad : MATCH_PASS * MATCH_TN);
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    p.a16 = take((size_t)p.na_pad * p.hpad * 2);
    p.b16 = take((size_t)p.nb_pad * p.hpad * 2);
    p.prow_v = take(pc / MATCH_TN * pr * 4);
    p.prow_i = take(pc / MATCH_TN * pr * 4);
    p.pcol_v = take(pr / MATCH_TM * pc * 4);
    p.pcol_i = take(pr / MATCH_TM * pc * 4);
    p.idx_ab = take((size_t)na * 4);
    p.sim_ab = take((size_t)na * 4);
    p.idx_ba = take((size_t)nb * 4);
    p.sim_ba = take((size_t)nb * 4);
    p.bytes = need;
    return p;
}
// a [na, H] / b [nb, H]: DEVICE f32 rows with row strides lda / ldb (floats); ws: DEVICE workspace of plan.bytes (256-byte aligned).
// Normalises both sides, runs the tile grid pass by pass and folds the partials: afterwards ws + plan.idx_ab etc. hold the results.
hipError_t launch_match(const float* a, size_t lda, const float* b, size_t ldb, int na, int nb, int H, char* ws, const MatchPlan& plan,
                        hipStream_t stream);

// match_normalise_kernel on its own (contract 1 of dinov2_hip_match): rows [n] of x (row stride ld floats) -> out [nout, hpad] f16, rows n ..
// nout - 1 zero, rows >= nout not touched.  The one normaliser of match.hip and bank.hip.
hipError_t launch_match_normalise(const float* x, size_t ld, _Float16* out, int n, int nout, int H, int hpad, hipStream_t stream);

// Top-k rows of a resident f16 bank by cosine similarity (csrc/bank.hip; contract in include/dinov2_hip.h, dinov2_hip_bank_topk).
// bank_topk_kernel has match_kernel's tile; workgroup (x, y) walks the `chunk_tiles` column tiles of chunk x for query row tile y and leaves
// one sorted list of k (value, index) pairs per query row; bank_merge_kernel merges the lists of a row over the chunks.  The queries are
// walked in passes of at most BANK_PASS_TILES row tiles, and the chunk count is capped, so that the partials of one pass
// (chunks x rows of the pass x k x 8 bytes) never exceed BANK_PARTIAL_MAX whatever nq, count and k.
constexpr int BANK_K_MAX = 64, BANK_PASS_TILES = 32, BANK_TARGET_WGS = 256;
constexpr size_t BANK_PARTIAL_MAX = (size_t)32 << 20;
struct BankEntry {  // one element of a list; an empty slot is (-inf, INT_MAX)
    float v;
    int i;
};
struct BankTopkPlan {
    int nq_pad, hpad;            // queries to whole tiles, H to a multiple of 64
    int ntiles;                  // column tiles that hold rows < count
    int chunk_tiles, nchunks;    // column tiles per workgroup, workgroups per query row tile
    int pass_tiles;              // query row tiles per pass
    size_t q16;                  // normalised queries [nq_pad, hpad] f16
    size_t part;                 // BankEntry [nchunks][pass_tiles * 128][k]
    size_t idx, sim;             // results [nq, k]
    size_t bytes;
};
// chunk_tiles = 0: as many chunks as fill BANK_TARGET_WGS workgroups; a given value is raised where the partials would pass BANK_PARTIAL_MAX
inline BankTopkPlan bank_topk_plan(int nq, int count, int H, int k, int chunk_tiles) {
    BankTopkPlan p{};
    p.nq_pad = (nq + MATCH_TM - 1) / MATCH_TM * MATCH_TM;
    p.hpad = (H + 63) / 64 * 64;
    p.ntiles = (count + MATCH_TN - 1) / MATCH_TN;
    const int rt = p.nq_pad / MATCH_TM < BANK_PASS_TILES ? p.nq_pad / MATCH_TM : BANK_PASS_TILES;
    const int want = (BANK_TARGET_WGS + rt - 1) / rt;
    if (chunk_tiles <= 0) chunk_tiles = (p.ntiles + want - 1) / want;
    const size_t per_chunk_tile = (size_t)MATCH_TM * k * sizeof(BankEntry);  // partials of one (chunk, row tile)
    const int max_chunks = (int)(BANK_PARTIAL_MAX / per_chunk_tile);
    const int floor_tiles = (p.ntiles + max_chunks - 1) / max_chunks;
    if (chunk_tiles < floor_tiles) chunk_tiles = floor_tiles;
    if (chunk_tiles > p.ntiles) chunk_tiles = p.ntiles;
    p.chunk_tiles = chunk_tiles;
    p.nchunks = (p.ntiles + chunk_tiles - 1) / chunk_tiles;
    const int fit = (int)(BANK_PARTIAL_MAX / (per_chunk_tile * p.nchunks));
    p.pass_tiles = rt < fit ? rt : fit;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    p.q16 = take((size_t)p.nq_pad * p.hpad * 2);
    p.part = take(per_chunk_tile * p.nchunks * p.pass_tiles);
    p.idx = take((size_t)nq * k * 4);
    p.sim = take((size_t)nq * k * 4);
    p.bytes = need;
    return p;
}
// q [nq, H]: DEVICE f32 rows with row stride ldq (floats); bank: the normalised f16 rows [>= ntiles * 128, hpad], of which the first `count`
// are searched; ws: DEVICE workspace of plan.bytes.  Afterwards ws + plan.idx / plan.sim hold [nq, k]; slots past `count` are (-1, -inf).
// `floor_only`: the sweep without its selection epilogue (a measuring aid: the results are meaningless).
hipError_t launch_bank_topk(const float* q, size_t ldq, int nq, const _Float16* bank, int count, int H, int k, char* ws, const BankTopkPlan& plan,
                            bool floor_only, hipStream_t stream);
// bank_merge_kernel on its own, for propagate.hip: row r < nrows: the sorted lists part[(c * pass_rows + r) * k ..] of chunks c < nchunks
// merged into idx / sim [r * k ..], empty slots as (-1, -inf)
hipError_t launch_bank_merge(const BankEntry* part, int pass_rows, int nchunks, int k, int nrows, int* idx, float* sim, hipStream_t stream);
// dinov2_hip_bank_keep: out[j, :] = rows[idx[j], :] for j < count (DEVICE indices, f16 rows of hpad elements; 64-bit offsets); `out` must
// not overlap the rows read
constexpr size_t BANK_KEEP_STAGE = (size_t)32 << 20;  // bytes of session scratch one chunk of the compaction is staged through
hipError_t launch_bank_gather(const _Float16* rows, const int* idx, int count, int hpad, _Float16* out, hipStream_t stream);

// Label propagation over a frame memory (csrc/propagate.hip; contract in include/dinov2_hip.h, dinov2_hip_propagate).  The memory holds
// `frames` slots of one h0 x w0 patch grid, each P = h0 w0 rows padded to ppad (whole 128-row tiles), so a slot owns whole column tiles.
// propagate_topk_kernel is bank_topk_kernel with two changes: its columns are the ITEMS (active slot a, kept column tile t), a-major, and
// a candidate must lie within `radius` cells (Chebyshev) of its query.  Column tiles none of whose grid rows can reach a grid row of the
// query tile are not walked: for query tile y the kept tiles are the range propagate_tile_range gives, the same for every slot.  The items
// of a query tile are cut into chunks of chunk_tiles items, one workgroup each; a workgroup past a query tile's last item leaves empty
// lists.  All P queries are one pass, and the chunk count is capped so that the partials (chunks x ppad x k x 8 bytes) stay within
// BANK_PARTIAL_MAX.  bank_merge_kernel merges the chunks; propagate_combine_kernel forms the weights and the weighted label mean.
constexpr int PROP_FRAMES_MAX = 64, PROP_GRID_MAX = 256, PROP_C_MAX = 256, PROP_RADIUS_MAX = 255;
constexpr int PROP_ROWS_MAX = 1 << 24;  // frames * ppad
// The cell of patch p of the grid: y << 16 | x (the memory's cell table; entries P .. ppad - 1 are never read as cells of candidates)
inline uint32_t propagate_cell(int p, int w0) { return (uint32_t)(p / w0) << 16 | (uint32_t)(p % w0); }
// Column tiles [*t0, *t1) of a slot that can hold a candidate of query tile qt (queries [128 qt, 128 qt + 128) n [0, P)): those with a patch in
// grid rows [first query row - radius, last query row + radius].  radius < 0: all of them.
__host__ __device__ inline void propagate_tile_range(int qt, int P, int w0, int radius, int* t0, int* t1) {
    const int ntiles = (P + MATCH_TN - 1) / MATCH_TN;
    if (radius < 0) {
        *t0 = 0;
        *t1 = ntiles;
        return;
    }
    const int q0 = qt * MATCH_TM, q1 = q0 + MATCH_TM - 1 < P - 1 ? q0 + MATCH_TM - 1 : P - 1;
    const int h0 = P / w0;
    int y0 = q0 / w0 - radius, y1 = q1 / w0 + radius;
    if (y0 < 0) y0 = 0;
    if (y1 > h0 - 1) y1 = h0 - 1;
    *t0 = y0 * w0 / MATCH_TN;
    *t1 = ((y1 + 1) * w0 - 1) / MATCH_TN + 1;
}
// The a-th set bit of `slots` (a < popcount)
__host__ __device__ inline int propagate_slot_of(uint64_t slots, int a) {
    for (int f = 0; f < 64; ++f)
        if (slots >> f & 1) {
            if (a == 0) return f;
            --a;
        }
    return -1;
}
struct PropagatePlan {
    int P, ppad, hpad, qtiles;   // patches of the grid, padded to whole tiles; H to a multiple of 64; query (and per-slot column) tiles
    int nactive;                 // set bits of `slots`
    int max_items, kept_items;   // items (active slot x kept column tile) of the query tile that has most; of all query tiles together
    int chunk_tiles, nchunks;    // items per workgroup, workgroups per query tile
    size_t q16;                  // normalised queries [ppad, hpad] f16
    size_t part;                 // BankEntry [nchunks][ppad][k]
    size_t idx, sim;             // the merged lists [P, k]
    size_t out, argmax;          // f32 [P, C], int32 [P]
    size_t bytes;
};
// chunk_tiles = 0: as many chunks as fill BANK_TARGET_WGS workgroups; a given value is raised where the partials would pass BANK_PARTIAL_MAX
inline PropagatePlan propagate_plan(int h0, int w0, int H, int nactive, int radius, int k, int C, int chunk_tiles) {
    PropagatePlan p{};
    p.P = h0 * w0;
    p.ppad = (p.P + MATCH_TN - 1) / MATCH_TN * MATCH_TN;
    p.hpad = (H + 63) / 64 * 64;
    p.qtiles = p.ppad / MATCH_TM;
    p.nactive = nactive;
    for (int qt = 0; qt < p.qtiles; ++qt) {
        int t0, t1;
        propagate_tile_range(qt, p.P, w0, radius, &t0, &t1);
        const int items = nactive * (t1 - t0);
        p.kept_items += items;
        if (items > p.max_items) p.max_items = items;
    }
    const int want = (BANK_TARGET_WGS + p.qtiles - 1) / p.qtiles;
    if (chunk_tiles <= 0) chunk_tiles = (p.max_items + want - 1) / want;
    const size_t per_chunk = (size_t)p.ppad * k * sizeof(BankEntry);  // partials of one chunk of every query tile
    const int max_chunks = (int)(BANK_PARTIAL_MAX / per_chunk);      // >= 1: ppad <= 2^16, k <= 64
    const int floor_tiles = (p.max_items + max_chunks - 1) / max_chunks;
    if (chunk_tiles < floor_tiles) chunk_tiles = floor_tiles;
    if (chunk_tiles > p.max_items) chunk_tiles = p.max_items;
    p.chunk_tiles = chunk_tiles;
    p.nchunks = (p.max_items + chunk_tiles - 1) / chunk_tiles;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    p.q16 = take((size_t)p.ppad * p.hpad * 2);
    p.part = take(per_chunk * p.nchunks);
    p.idx = take((size_t)p.P * k * 4);
    p.sim = take((size_t)p.P * k * 4);
    p.out = take((size_t)p.P * C * 4);
    p.argmax = take((size_t)p.P * 4);
    p.bytes = need;
    return p;
}
// Where everything sits in the memory's one allocation (256-byte aligned offsets; 64-bit throughout)
struct PropMemLayout {
    size_t rows;    // f16 [frames][ppad][hpad]
    size_t labels;  // f32 [frames][P][C]
    size_t kept;    // f32 [P][C]: `out` of the last propagate with keep
    size_t cells;   // uint32 [ppad]: propagate_cell
    size_t bytes;
};
inline PropMemLayout propmem_layout(int frames, int P, int ppad, int hpad, int C) {
    PropMemLayout l{};
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    l.rows = take((size_t)frames * ppad * hpad * 2);
    l.labels = take((size_t)frames * P * C * 4);
    l.kept = take((size_t)P * C * 4);
    l.cells = take((size_t)ppad * 4);
    l.bytes = need;
    return l;
}
struct PropMemView {  // the device arrays of a memory
    const _Float16* rows;
    const float* labels;
    float* kept;
    const uint32_t* cells;
    int h0, w0, C;
};
// q [P, H]: DEVICE f32 rows with row stride ldq (floats); ws: DEVICE workspace of plan.bytes, where idx, sim, out and argmax are left.
// keep: `out` is also written to m.kept.  Every set bit of `slots` must be a slot below the memory's frames.  No wait.
hipError_t launch_propagate(const float* q, size_t ldq, int H, const PropMemView& m, uint64_t slots, int radius, int k, float temperature,
                            bool keep, char* ws, const PropagatePlan& plan, hipStream_t stream);

// Spherical k-means of token rows (csrc/kmeans.hip; contract in include/dinov2_hip.h, dinov2_hip_kmeans).  The assignment has match_kernel's
// tile; the update is a GEMM X^T [hpad128, npad] x one-hot [npad, kpad] with the same tile, its rows split into `nsplit` chunks (a multiple of
// 64 rows each, the last one possibly shorter) whose f32 partials [nsplit][kpad][hpad128] never exceed KMEANS_PARTIAL_MAX.
constexpr int KMEANS_K_MAX = 1024, KMEANS_ITER_MAX = 1000, KMEANS_N_MAX = 1 << 20, KMEANS_TARGET_WGS = 256;
constexpr size_t KMEANS_PARTIAL_MAX = (size_t)32 << 20;
struct KmeansPlan {
    int npad, kpad, hpad, hpad128;  // rows and centres to whole 128-tiles, H to a multiple of 64 (assignment) and of 128 (update)
    int chunk, nsplit;              // rows per chunk of the update, chunks: chunk i covers rows [i chunk, min((i + 1) chunk, npad))
    size_t x16, xt, c16;            // f16: X^ [npad, hpad], X^T [hpad128, npad], normalised centres [kpad, hpad]
    size_t cvec;                    // the centre vectors [K, H] f32
    size_t labels, sim;             // [npad] int32 (-1 on padding rows), [npad] f32
    size_t part, cpart, counts;     // f32 [nsplit][kpad][hpad128], int32 [nsplit][kpad], int32 [kpad]
    size_t chpart, changed;         // int32 [npad / 128], int32 [1]
    size_t init;                    // int32 [K]: the row indices of DINOV2_HIP_KMEANS_INIT_ROWS
    size_t part_bytes, bytes;
};
// nsplit = 0: as many chunks as bring the update grid to about KMEANS_TARGET_WGS workgroups; the chunk of a given value is raised where the
// partials would pass KMEANS_PARTIAL_MAX.  Pure: (n, K, H, nsplit) alone decide every summation order of the update.
inline KmeansPlan kmeans_plan(int n, int K, int H, int nsplit) {
    KmeansPlan p{};
    p.npad = (n + 127) / 128 * 128;
    p.kpad = (K + 127) / 128 * 128;
    p.hpad = (H + 63) / 64 * 64;
    p.hpad128 = (H + 127) / 128 * 128;
    const int nt = p.npad / 64;  // K-tiles of the update
    const int tiles = (p.hpad128 / 128) * (p.kpad / 128);
    const size_t per_split = (size_t)p.kpad * p.hpad128 * 4;  // <= 16 MiB
    if (nsplit <= 0) nsplit = (KMEANS_TARGET_WGS + tiles - 1) / tiles;
    const int cap = (int)(KMEANS_PARTIAL_MAX / per_split);
    if (nsplit > cap) nsplit = cap;
    if (nsplit > nt) nsplit = nt;
    const int chunk_tiles = (nt + nsplit - 1) / nsplit;
    p.chunk = chunk_tiles * 64;
    p.nsplit = (nt + chunk_tiles - 1) / chunk_tiles;  // no empty chunk
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    p.x16 = take((size_t)p.npad * p.hpad * 2);
    p.xt = take((size_t)p.hpad128 * p.npad * 2);
    p.c16 = take((size_t)p.kpad * p.hpad * 2);
    p.cvec = take((size_t)K * H * 4);
    p.labels = take((size_t)p.npad * 4);
    p.sim = take((size_t)p.npad * 4);
    p.part_bytes = per_split * p.nsplit;
    p.part = take(p.part_bytes);
    p.cpart = take((size_t)p.nsplit * p.kpad * 4);
    p.counts = take((size_t)p.kpad * 4);
    p.chpart = take((size_t)(p.npad / 128) * 4);
    p.changed = take(4);
    p.init = take((size_t)K * 4);
    p.bytes = need;
    return p;
}
struct KmeansBufs {  // the device arrays of one run: views of a workspace (kmeans_bufs) or buffers of their own
    _Float16 *x16, *xt, *c16;
    float* cvec;
    int* labels;
    float* sim;
    float* part;
    int *cpart, *counts, *chpart, *changed;
};
KmeansBufs kmeans_bufs(char* ws, const KmeansPlan& plan);
// x16 and c16 normalised (launch_match_normalise with nout = npad / kpad) -> labels [npad] (read unless `first`; padding rows -1), sim [n],
// *changed = the rows whose label differs from what labels held (`first`: n)
hipError_t launch_kmeans_assign(const KmeansBufs& b, int n, int K, const KmeansPlan& plan, bool first, hipStream_t stream);
// x16 -> xt, every element of it written
hipError_t launch_kmeans_transpose(const KmeansBufs& b, const KmeansPlan& plan, hipStream_t stream);
// xt, labels (values in [0, K) or -1) -> counts [K]; cvec rows of the clusters with members = their sums; c16 = normalise(cvec)
hipError_t launch_kmeans_update(const KmeansBufs& b, int K, int H, const KmeansPlan& plan, hipStream_t stream);
hipError_t launch_kmeans_count(const KmeansBufs& b, int K, const KmeansPlan& plan, hipStream_t stream);
// cvec [K, H] = rows idx[j] (DEVICE indices) of src, where row r lives at src + (r / per) * outer + (r % per) * ld floats
hipError_t launch_kmeans_gather(const float* src, int per, size_t outer, size_t ld, const int* idx, int K, int H, float* cvec, hipStream_t stream);
// The loop (contract 5): b.x16 = the normalised rows, b.cvec = the init vectors on entry; synchronises the stream once per assignment.
hipError_t kmeans_run(const KmeansBufs& b, int n, int K, int H, int max_iter, const KmeansPlan& plan, hipStream_t stream, int* iterations,
                      int* converged);

// Greedy k-center selection of rows (csrc/coreset.hip; contract in include/dinov2_hip.h, dinov2_hip_coreset).  One launch of
// coreset_sweep_kernel per pick: workgroup x owns rows [x rows_per_wg, +rows_per_wg) -- whole 128-row tiles -- and leaves one (smallest
// similarity, lowest row) partial over its unselected rows; the next launch's workgroups each fold the nparts partials themselves.  The
// partials are double-buffered ([2][CORESET_PARTS_MAX]), so a launch never reads what it writes.
constexpr int CORESET_N_MAX = 1 << 20, CORESET_BANK_N_MAX = 1 << 24, CORESET_PARTS_MAX = 1024;
constexpr int CORESET_POLL = 256;                    // picks between two reads of the stop flag by the host
constexpr size_t CORESET_WG_BYTES = (size_t)64 << 10;  // a workgroup's share of the f16 rows is at least this where that still leaves 512 workgroups
struct CoresetPlan {
    int npad, hpad;            // rows to whole tiles, H to a multiple of 64
    int rows_per_wg, nparts;   // rows per workgroup (a multiple of 128), workgroups = partials (<= CORESET_PARTS_MAX)
    size_t x16;                // normalised rows [npad, hpad] f16 (not used when the rows are a bank's)
    size_t sim, nearest, mark; // f32 [npad], int32 [npad], uint8 [npad]: s, the position of the most similar pick, 1 = selected
    size_t part;               // BankEntry [2][CORESET_PARTS_MAX]
    size_t head;               // int32 [4]: [0] the stop flag, [1] `selected`
    size_t idx, cover;         // int32 [m], f32 [m]
    size_t bytes;
};
// rows_per_wg = 0: one tile a workgroup; more where n needs it to stay within CORESET_PARTS_MAX partials, and where a tile is shorter than
// CORESET_WG_BYTES and 512 workgroups remain.  A given value is rounded up to whole tiles and raised to the first of these bounds.  Pure:
// (n, H) alone fix the geometry (m only sizes the two result arrays), and no result depends on it.
inline CoresetPlan coreset_plan(int n, int H, int m, int rows_per_wg, bool own_rows = true) {
    CoresetPlan p{};
    p.npad = (n + 127) / 128 * 128;
    p.hpad = (H + 63) / 64 * 64;
    const int tiles = p.npad / 128;
    const int floor_tiles = (tiles + CORESET_PARTS_MAX - 1) / CORESET_PARTS_MAX;
    int tpw = (rows_per_wg + 127) / 128;
    if (rows_per_wg <= 0) {
        const int want = (int)((CORESET_WG_BYTES + (size_t)128 * p.hpad * 2 - 1) / ((size_t)128 * p.hpad * 2));
        const int spare = tiles / 512;
        tpw = want < spare ? want : spare;
    }
    if (tpw < floor_tiles) tpw = floor_tiles;
    if (tpw < 1) tpw = 1;
    if (tpw > tiles) tpw = tiles;
    p.rows_per_wg = tpw * 128;
    p.nparts = (tiles + tpw - 1) / tpw;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    p.x16 = take(own_rows ? (size_t)p.npad * p.hpad * 2 : 0);
    p.sim = take((size_t)p.npad * 4);
    p.nearest = take((size_t)p.npad * 4);
    p.mark = take((size_t)p.npad);
    p.part = take((size_t)2 * CORESET_PARTS_MAX * sizeof(BankEntry));
    p.head = take(16);
    p.idx = take((size_t)m * 4);
    p.cover = take((size_t)m * 4);
    p.bytes = need;
    return p;
}
struct CoresetBufs {  // the device arrays of one run: views of a workspace (coreset_bufs) or buffers of their own
    const _Float16* x16;
    float* sim;
    int* nearest;
    unsigned char* mark;
    BankEntry* part;
    int* head;
    int* idx;
    float* cover;
};
CoresetBufs coreset_bufs(char* ws, const CoresetPlan& plan, const _Float16* bank_rows);
// Contracts 3 - 5 of dinov2_hip_coreset on the normalised rows b.x16 [>= n rounded up to 16 rows, hpad] (rows >= n are never looked at):
// once the stream has run what this enqueues, idx / cover [m], head[1] = selected, nearest / sim [n] hold the results on the device.
// Enqueues one init launch and one sweep per pick, and waits for the stream only every CORESET_POLL picks, to read the 4-byte stop flag
// (never when stop_sim is +inf); the picked rows' indices stay on the device.
hipError_t coreset_run(const CoresetBufs& b, int n, int m, int first, float stop_sim, const CoresetPlan& plan, hipStream_t stream);

// VLAD descriptors of row segments (csrc/vlad.hip; contract in include/dinov2_hip.h, dinov2_hip_vlad).  Every segment has a block of its own
// in the f16 operand, padded to whole 128-row tiles, so that an assignment tile belongs to one segment and the K-tiles of the cluster sums
// start at the segment's first row: what a segment's sums are made of, and in which order, never depends on its neighbours or its offset.
// The sums are k-means' one-hot GEMM over chunks of vlad_chunk_rows(K, H) rows of ONE segment; the chunks of all segments in ascending order
// are walked in passes of at most `cap` chunks, whose f32 partials [cap][kpad][hpad128] never exceed VLAD_PARTIAL_MAX.
constexpr int VLAD_SEG_MAX = 4096, VLAD_N_MAX = 1 << 20;
constexpr size_t VLAD_OUT_MAX = (size_t)1 << 28, VLAD_PARTIAL_MAX = (size_t)32 << 20;
enum VladFlags : unsigned { VLAD_INTRA_NORM = 1u, VLAD_L2_NORM = 2u };
struct VladSeg {  // one segment: rows [row0, row0 + pad) of the padded layout hold its `len` rows and zeros; chunks [chunk0, chunk0 + nchunks)
    int row0, len, chunk0, nchunks;
};
struct VladChunk {  // one workgroup layer of the sums: `ktiles` K-tiles of 64 rows from padded row `row0` on, all of segment `seg`
    int seg, row0, ktiles;
};
struct VladTile {  // one assignment tile: its first `valid` rows are real, and they are rows out0 .. of the caller's rows
    int valid, out0;
};
// rows of a segment's block: its length to whole 128-row tiles
inline int vlad_seg_pad(int len) { return (len + 127) / 128 * 128; }
// Rows per chunk: a multiple of 64 from (K, H) alone -- as many K-tiles as the sums have output tiles, between 4 and 32: few output tiles
// need many chunks to fill the device, many output tiles amortise their stores over a longer chunk.
inline int vlad_chunk_rows(int K, int H) {
    const int tiles = ((H + 127) / 128) * ((K + 127) / 128);
    return 64 * (tiles < 4 ? 4 : tiles > 32 ? 32 : tiles);
}
struct VladPlan {
    int kpad, hpad, hpad128;        // as KmeansPlan
    int chunk, cap;                 // rows per chunk; chunks per pass
    int npad, ntiles;               // rows of the padded layout (the sum of the segments' pads), its 128-row tiles
    int nchunks, npass;             // pass p = chunks [p cap, min((p + 1) cap, nchunks))
    size_t x16, xt, c16;            // f16: X^ [npad, hpad], X^T [hpad128, npad], unit centres [kpad, hpad]
    size_t cvec;                    // the caller's centre vectors [K, H] f32
    size_t labels;                  // int32 [npad], padded layout (-1 on padding rows)
    size_t labels_out, sim_out;     // int32 / f32 [n], the caller's order
    size_t part, cpart;             // f32 [cap'][kpad][hpad128], int32 [cap'][kpad], cap' = min(cap, nchunks)
    size_t vlad, counts, rowss;     // f32 [n_seg, K, H], int32 [n_seg, K], f32 [n_seg, K] (sum of squares of each written row)
    size_t segs, chunks, tiles;     // VladSeg [n_seg], VladChunk [nchunks], VladTile [ntiles]
    size_t part_bytes, bytes;
};
// offsets [n_seg + 1] strictly ascending from 0.  Pure: a segment's chunks follow from (its length, K, H) alone; the pass boundaries depend
// on the segments before it, and the fold of vlad_finish_kernel is the same left-to-right chain wherever a pass ends.  segs / chunks / tiles
// (any may be NULL) receive the three tables.
inline VladPlan vlad_plan(const int32_t* offsets, int n_seg, int K, int H, std::vector<VladSeg>* segs, std::vector<VladChunk>* chunks,
                          std::vector<VladTile>* tiles) {
    VladPlan p{};
    p.kpad = (K + 127) / 128 * 128;
    p.hpad = (H + 63) / 64 * 64;
    p.hpad128 = (H + 127) / 128 * 128;
    p.chunk = vlad_chunk_rows(K, H);
    const size_t per_chunk = (size_t)p.kpad * p.hpad128 * 4;  // <= 16 MiB
    p.cap = (int)(VLAD_PARTIAL_MAX / per_chunk);
    if (segs) segs->clear();
    if (chunks) chunks->clear();
    if (tiles) tiles->clear();
    for (int s = 0; s < n_seg; ++s) {
        const int len = offsets[s + 1] - offsets[s], pad = vlad_seg_pad(len), nch = (pad + p.chunk - 1) / p.chunk;
        if (segs) segs->push_back(VladSeg{p.npad, len, p.nchunks, nch});
        for (int j = 0; chunks && j < nch; ++j) {
            const int r0 = j * p.chunk, r1 = r0 + p.chunk < pad ? r0 + p.chunk : pad;
            chunks->push_back(VladChunk{s, p.npad + r0, (r1 - r0) / 64});
        }
        for (int t = 0; tiles && t < pad / 128; ++t) {
            const int left = len - t * 128;
            tiles->push_back(VladTile{left < 128 ? left : 128, offsets[s] + t * 128});
        }
        p.npad += pad;
        p.nchunks += nch;
    }
    p.ntiles = p.npad / 128;
    p.npass = (p.nchunks + p.cap - 1) / p.cap;
    const int n = offsets[n_seg], held = p.nchunks < p.cap ? p.nchunks : p.cap;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    p.x16 = take((size_t)p.npad * p.hpad * 2);
    p.xt = take((size_t)p.hpad128 * p.npad * 2);
    p.c16 = take((size_t)p.kpad * p.hpad * 2);
    p.cvec = take((size_t)K * H * 4);
    p.labels = take((size_t)p.npad * 4);
    p.labels_out = take((size_t)n * 4);
    p.sim_out = take((size_t)n * 4);
    p.part_bytes = per_chunk * held;
    p.part = take(p.part_bytes);
    p.cpart = take((size_t)held * p.kpad * 4);
    p.vlad = take((size_t)n_seg * K * H * 4);
    p.counts = take((size_t)n_seg * K * 4);
    p.rowss = take((size_t)n_seg * K * 4);
    p.segs = take((size_t)n_seg * sizeof(VladSeg));
    p.chunks = take((size_t)p.nchunks * sizeof(VladChunk));
    p.tiles = take((size_t)p.ntiles * sizeof(VladTile));
    p.bytes = need;
    return p;
}
struct VladBufs {  // the device arrays of one call: views of a workspace (vlad_bufs) or buffers of their own
    _Float16 *x16, *xt, *c16;
    float* cvec;
    int *labels, *labels_out;
    float *sim_out, *part;
    int* cpart;
    float* vlad;
    int* counts;
    float* rowss;
    VladSeg* segs;
    VladChunk* chunks;
    VladTile* tiles;
};
VladBufs vlad_bufs(char* ws, const VladPlan& plan);
// launch_match_normalise's rows, bit for bit (csrc/normalise_row.h), into a layout of `ntiles` 128-row tiles in ONE launch (VladPlan): row
// r of tile t of out is source row g = tiles[t].out0 + r where r < tiles[t].valid, zeros otherwise; source row g lives at x + (g / per) * outer + (g % per) * ld floats (the
// view of launch_kmeans_gather).  tiles: DEVICE.
hipError_t launch_vlad_normalise(const float* x, int per, size_t outer, size_t ld, const VladTile* tiles, int ntiles, _Float16* out, int H,
                                 int hpad, hipStream_t stream);
// Everything after the operands: b.x16 (every segment normalised into its block by launch_vlad_normalise), b.cvec and
// the three tables are in place; normalises the centres, assigns, transposes, then sums and finishes pass by pass (`chunks`: the host's copy
// of that table) and takes the L2 step.  Afterwards labels_out, sim_out, counts and vlad hold the results.  No wait.
hipError_t vlad_run(const VladBufs& b, int n_seg, int K, int H, unsigned flags, const VladPlan& plan, const VladChunk* chunks,
                    hipStream_t stream);
// the single steps, for the diagnostic ops' timings
hipError_t launch_vlad_assign(const VladBufs& b, int K, const VladPlan& plan, hipStream_t stream);
hipError_t launch_vlad_sums(const VladBufs& b, int n_seg, int K, int H, unsigned flags, const VladPlan& plan, const VladChunk* chunks,
                            hipStream_t stream);

// Dense linear heads (csrc/dense.hip; contract in include/dinov2_hip.h, dinov2_hip_predict_dense): dense_pack_kernel builds the f16 operand
// A [B P, K] of the logits GEMM straight from the residual stream at each tapped layer, launch_gemm(DT_F16, EPI_PLAIN_F32) gives the
// low-resolution logits [B P, Cpad] f32, dense_reduce_kernel resamples them to out_h x out_w and reduces over the classes per pixel.
constexpr int DENSE_C_MIN = 2, DENSE_C_MAX = 256, DENSE_LAYERS_MAX = 8, DENSE_OUT_MAX = 8192;
constexpr size_t DENSE_LDS_BUDGET = (size_t)64 << 10;  // what a workgroup of dense_reduce_kernel may take (the limit no attribute has to raise)
enum DenseReduce : int { DENSE_ARGMAX = 0, DENSE_BINS = 1 };
// columns of the logits the GEMM writes: the weight is stored [Cpad, K] with zero rows, so that every 128- or 256-column tile reads real memory
inline int dense_cpad(int C) { return (C + 127) / 128 * 128; }
// floats from one staged logit row to the next in LDS: C to a multiple of 4, then an ODD number of 16-byte units, so that up to 16 neighbouring
// rows start in 16 different 16-byte bank groups (256 classes: 260 floats)
inline int dense_pitch(int C) { return (((C + 3) / 4) | 1) * 4; }
// Contract 3, one axis: where output coordinate dst samples the n_in inputs.  scale = (float)n_in / (float)n_out, computed ONCE on the host.
// Every operation rounds on its own (nothing contracted); the one source of these bits for the kernel, the planner and the host.
__host__ __device__ inline void dense_axis(float scale, int dst, int n_in, int& i0, int& i1, float& lam) {
#pragma clang fp contract(off)
    const float t = scale * ((float)dst + 0.5f);
    float src = t - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    i0 = (int)src;
    i0 = i0 < n_in - 1 ? i0 : n_in - 1;
    i1 = i0 + 1 < n_in - 1 ? i0 + 1 : n_in - 1;
    lam = src - (float)i0;
}
// The launch geometry of dense_reduce_kernel, decided without the device: a workgroup owns tile_y x tile_x output pixels and stages the
// span_y x span_x low-resolution rows between the first pixel's i0 and the last pixel's i1 (per axis, the widest over all tiles) into LDS --
// the largest tile of the list whose rows, centres and label tile fit DENSE_LDS_BUDGET.  A 1 x 1 tile needs 2 x 2 rows: some tile always fits.
struct DenseReducePlan {
    int tile_y, tile_x;  // 0, 0: refused arguments
    int span_y, span_x;
    int pitch;
    int grid_x, grid_y;
    float scale_y, scale_x;
    size_t lds_bytes;
};
inline int dense_axis_span(float scale, int n_in, int n_out, int tile) {
    int span = 0;
    for (int d0 = 0; d0 < n_out; d0 += tile) {
        const int d1 = d0 + tile < n_out ? d0 + tile - 1 : n_out - 1;
        int lo, hi, t;
        float lam;
        dense_axis(scale, d0, n_in, lo, t, lam);
        dense_axis(scale, d1, n_in, t, hi, lam);
        span = hi - lo + 1 > span ? hi - lo + 1 : span;
    }
    return span;
}
inline DenseReducePlan dense_reduce_plan(int h0, int w0, int C, int out_h, int out_w) {
    DenseReducePlan p{};
    if (h0 < 1 || w0 < 1 || C < 1 || C > DENSE_C_MAX || out_h < 1 || out_w < 1 || out_h > DENSE_OUT_MAX || out_w > DENSE_OUT_MAX) return p;
    static const int tiles[8][2] = {{16, 64}, {16, 32}, {16, 16}, {8, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}};
    p.scale_y = (float)h0 / (float)out_h;
    p.scale_x = (float)w0 / (float)out_w;
    p.pitch = dense_pitch(C);
    for (const auto& t : tiles) {
        const int sy = dense_axis_span(p.scale_y, h0, out_h, t[0]), sx = dense_axis_span(p.scale_x, w0, out_w, t[1]);
        const size_t lds = (size_t)sy * sx * p.pitch * 4 + (size_t)(C + 3) / 4 * 16 + ((size_t)t[0] * t[1] + 15) / 16 * 16;
        if (lds > DENSE_LDS_BUDGET) continue;
        p.tile_y = t[0]; p.tile_x = t[1]; p.span_y = sy; p.span_x = sx; p.lds_bytes = lds;
        p.grid_y = (out_h + t[0] - 1) / t[0];
        p.grid_x = (out_w + t[1] - 1) / t[1];
        break;
    }
    return p;
}
// x [B*T, H] f32 (the residual stream): for every PATCH row (b, p) the f16 (round to nearest even) of the row launch_layer_tap gives with the
// same `norm` goes to A[(b P + p) lda + col0 .. + H), and with `concat_cls` that image's CLS row behind it (.. + 2 H).  16-byte stores:
// H, lda and col0 multiples of 8, A 16-byte aligned.  H <= 2 048.
hipError_t launch_dense_pack(const float* x, const float* w, const float* b, float eps, int B, int T, int R, int H, bool norm, bool concat_cls,
                             _Float16* A, size_t lda, int col0, hipStream_t stream);
// logits [B, h0 w0, ldl] f32 DEVICE (token-major, ldl % 4 == 0, 16-byte aligned) -> labels [B, out_h, out_w] u8 (ARGMAX only) and / or value
// [B, out_h, out_w] f32, either may be nullptr; centers [C] DEVICE (BINS).  plan = dense_reduce_plan(h0, w0, C, out_h, out_w).
hipError_t launch_dense_reduce(const float* logits, int ldl, int B, int h0, int w0, int C, int out_h, int out_w, int reduce, const float* centers,
                               float eps, uint8_t* labels, float* value, const DenseReducePlan& plan, hipStream_t stream);

// Sliding-window dense inference (csrc/slide.hip; contract in include/dinov2_hip.h, dinov2_hip_predict_dense_slide): slide_gather_kernel copies
// the windows out of the resident images into one window batch, the ordinary forward and head give every window's low-resolution logits,
// slide_reduce_kernel averages, per output pixel and class, the resampled logits of the windows that cover the pixel and reduces over the classes.
constexpr int SLIDE_COVER_MAX = 16, SLIDE_WINDOWS_MAX = 65535;
// Contract 1, one axis (mmsegmentation's slide_inference): the number of windows and where window i starts.
inline int slide_count(int len, int crop, int stride) {
    const int t = len - crop + stride - 1;
    return (t > 0 ? t : 0) / stride + 1;
}
inline int slide_start(int i, int len, int crop, int stride) {
    long long e = (long long)i * stride + crop;
    e = (e < len ? e : len) - crop;
    return e > 0 ? (int)e : 0;
}
// Window starts of one axis that the kernels accept: ascending, inside the image, and leaving no pixel uncovered.
inline bool slide_axis_valid(const int* st, int n, int crop, int len) {
    if (!st || n < 1 || crop < 1 || crop > len || st[0] != 0 || st[n - 1] + crop != len) return false;
    for (int i = 1; i < n; ++i)
        if (st[i] < st[i - 1] || st[i] > st[i - 1] + crop) return false;
    return true;
}
// the largest number of windows over one coordinate (valid starts); a pixel's cover is the product of its two axes'
inline int slide_axis_cover(const int* st, int n, int crop) {
    int best = 0;
    for (int i = 0, j = 0; i < n; ++i) {  // (the busiest coordinate is some window's first)
        while (st[j] + crop <= st[i]) ++j;
        best = i - j + 1 > best ? i - j + 1 : best;
    }
    return best;
}
// One axis cut into tiles of `tile` coordinates: per tile the first window that touches it and how many do (ranges[2 t], ranges[2 t + 1]; may
// be nullptr); over all tiles the largest such number (slots) and the most low-resolution rows one window has to stage for one tile (span):
// from the i0 of the tile's first coordinate inside the window to the i1 of its last.  The kernel computes the same rows by the same calls.
inline void slide_axis_tiles(const int* st, int n, int crop, int len, int n_in, float scale, int tile, int* ranges, int& slots, int& span) {
    slots = span = 0;
    for (int t = 0, p0 = 0, lo = 0; p0 < len; ++t, p0 += tile) {
        const int p1 = (p0 + tile < len ? p0 + tile : len) - 1;
        while (st[lo] + crop <= p0) ++lo;
        int hi = lo;
        while (hi + 1 < n && st[hi + 1] <= p1) ++hi;
        if (ranges) {
            ranges[2 * t] = lo;
            ranges[2 * t + 1] = hi - lo + 1;
        }
        slots = hi - lo + 1 > slots ? hi - lo + 1 : slots;
        for (int i = lo; i <= hi; ++i) {
            const int d0 = p0 > st[i] ? p0 - st[i] : 0, d1 = p1 - st[i] < crop - 1 ? p1 - st[i] : crop - 1;
            int a, b, u;
            float lam;
            dense_axis(scale, d0, n_in, a, u, lam);
            dense_axis(scale, d1, n_in, u, b, lam);
            span = b - a + 1 > span ? b - a + 1 : span;
        }
    }
}
// The launch geometry and LDS layout of slide_reduce_kernel, decided without the device.  A workgroup owns tile_y x tile_x output pixels (at
// most 256: one per thread) in IMAGE coordinates; up to slots_y x slots_x windows touch a tile, each stages up to span_y x span_x rows of
// `chunk` classes (a multiple of 4, pitch = dense_pitch(chunk)).  The classes go through LDS chunk by chunk when the rows of all C do not fit:
// a pixel's running argmax or sums stay in registers across the chunks, so the orders of contract 3 and 4 do not depend on the chunking.
// The largest tile of the list that holds all classes, or at least 32 of them per chunk, within DENSE_LDS_BUDGET; a 1 x 1 tile has at most
// SLIDE_COVER_MAX slots of 2 x 2 rows of 4 classes, 1 KiB: some tile always fits.
struct SlideReducePlan {
    int tile_y, tile_x;  // 0, 0: refused arguments
    int slots_y, slots_x, span_y, span_x;
    int chunk, pitch;
    int grid_x, grid_y;
    int cover;  // windows over the busiest pixel
    float scale_y, scale_x;
    size_t lds_bytes;
};
inline size_t slide_lds_bytes(int ty, int tx, int sy, int sx, int ny, int nx, int pitch, int C) {
    return (size_t)sy * sx * ny * nx * pitch * 4 + (size_t)(C + 3) / 4 * 16 + ((size_t)ty * sy + (size_t)tx * sx + sy + sx) * 16 +
           ((size_t)ty * tx + 15) / 16 * 16;
}
// (h0, w0): the crop's patch grid; y1 [ny], x1 [nx]: valid starts of windows of crop_h x crop_w in an image of h x w
inline SlideReducePlan slide_reduce_plan(int h0, int w0, int C, int crop_h, int crop_w, int h, int w, const int* y1, int ny, const int* x1, int nx) {
    SlideReducePlan p{};
    if (h0 < 1 || w0 < 1 || C < 1 || C > DENSE_C_MAX || h > DENSE_OUT_MAX || w > DENSE_OUT_MAX) return p;
    if (!slide_axis_valid(y1, ny, crop_h, h) || !slide_axis_valid(x1, nx, crop_w, w)) return p;
    const int cover = slide_axis_cover(y1, ny, crop_h) * slide_axis_cover(x1, nx, crop_w);
    if (cover > SLIDE_COVER_MAX) return p;
    static const int tiles[5][2] = {{16, 16}, {8, 8}, {4, 4}, {2, 2}, {1, 1}};
    p.scale_y = (float)h0 / (float)crop_h;
    p.scale_x = (float)w0 / (float)crop_w;
    p.cover = cover;
    const int C4 = (C + 3) / 4;
    for (const auto& t : tiles) {
        int sy, sx, ry, rx;
        slide_axis_tiles(y1, ny, crop_h, h, h0, p.scale_y, t[0], nullptr, sy, ry);
        slide_axis_tiles(x1, nx, crop_w, w, w0, p.scale_x, t[1], nullptr, sx, rx);
        int q = C4;  // classes per chunk in units of 4: the most whose pitch fits
        while (q > 1 && slide_lds_bytes(t[0], t[1], sy, sx, ry, rx, dense_pitch(4 * q), C) > DENSE_LDS_BUDGET) --q;
        if (slide_lds_bytes(t[0], t[1], sy, sx, ry, rx, dense_pitch(4 * q), C) > DENSE_LDS_BUDGET) continue;
        if (q < C4 && q < 8 && t[0] > 1) continue;
        p.tile_y = t[0]; p.tile_x = t[1]; p.slots_y = sy; p.slots_x = sx; p.span_y = ry; p.span_x = rx;
        p.chunk = 4 * q;
        p.pitch = dense_pitch(4 * q);
        p.lds_bytes = slide_lds_bytes(t[0], t[1], sy, sx, ry, rx, p.pitch, C);
        p.grid_y = (h + t[0] - 1) / t[0];
        p.grid_x = (w + t[1] - 1) / t[1];
        break;
    }
    return p;
}
// The window table both kernels read, in ints: y1 [ny] | x1 [nx] | per tile row (first window row, how many) [grid_y][2] | the same per tile
// column [grid_x][2].  slide_table_fill writes slide_table_ints(plan, ny, nx) of them.
inline size_t slide_table_ints(const SlideReducePlan& p, int ny, int nx) { return (size_t)ny + nx + 2 * ((size_t)p.grid_y + p.grid_x); }
inline void slide_table_fill(const SlideReducePlan& p, int h0, int w0, int crop_h, int crop_w, int h, int w, const int* y1, int ny, const int* x1,
                             int nx, int* tab) {
    for (int i = 0; i < ny; ++i) tab[i] = y1[i];
    for (int i = 0; i < nx; ++i) tab[ny + i] = x1[i];
    int slots, span;
    slide_axis_tiles(y1, ny, crop_h, h, h0, p.scale_y, p.tile_y, tab + ny + nx, slots, span);
    slide_axis_tiles(x1, nx, crop_w, w, w0, p.scale_x, p.tile_x, tab + ny + nx + 2 * p.grid_y, slots, span);
}
// img [B, 3, h, w] (layout 1, RGB_CHW) or [B, h, w, 3] (0, BGR_HWC) f32 DEVICE -> win [B ny nx, ...] the same layout at crop_h x crop_w, window
// (b, iy, ix) at index (b ny + iy) nx + ix: a copy, bit for bit.  tab: DEVICE, starts with y1 [ny] | x1 [nx].  B ny nx <= 65 535.
hipError_t launch_slide_gather(const float* img, float* win, const int* tab, int B, int h, int w, int ny, int nx, int crop_h, int crop_w, int layout,
                               hipStream_t stream);
// logits [B ny nx, h0 w0, ldl] f32 DEVICE (ldl >= C, any alignment of the rows) -> labels [B, h, w] u8 (ARGMAX only) and / or value [B, h, w] f32;
// tab: the DEVICE copy of slide_table_fill's table for `plan` = slide_reduce_plan of this problem; centers [C] DEVICE (BINS).
hipError_t launch_slide_reduce(const float* logits, int ldl, int B, int h0, int w0, int C, int crop_h, int crop_w, int h, int w, int ny, int nx,
                               const int* tab, int reduce, const float* centers, float eps, uint8_t* labels, float* value, const SlideReducePlan& plan,
                               hipStream_t stream);

// Spectral embedding of token rows (csrc/ncut.hip, csrc/ncut.cpp; contract in include/dinov2_hip.h, dinov2_hip_ncut).  ncut_apply_kernel has
// match_kernel's tile: workgroup (x, y) owns row tile x and the `chunk_tiles` column tiles of chunk y, forms the affinities of each tile on
// the accumulators and sums w_ij (scale_j q_j) over its columns in f64 for the NCUT_NB columns of the block; ncut_finish_kernel folds the
// chunks in ascending order.  The chunk count is capped so that the partials [nchunks][npad][NCUT_NB] f64 never exceed NCUT_PARTIAL_MAX.
constexpr int NCUT_NB = PCA_NB, NCUT_N_MIN = 16, NCUT_N_MAX = 1 << 17, NCUT_EIG_MAX = 6, NCUT_ITER_MAX = 10000, NCUT_TARGET_WGS = 256;
constexpr size_t NCUT_PARTIAL_MAX = (size_t)32 << 20;
enum NcutAffinity : int { NCUT_THRESHOLD = 0, NCUT_RELU = 1, NCUT_EXP = 2 };
// the steps between two Rayleigh-Ritz checks on the host, by the steps already taken
inline int ncut_check_interval(int steps_done) { return steps_done < 32 ? 8 : 16; }
struct NcutPlan {
    int npad, hpad;            // rows to whole tiles, H to a multiple of 64
    int ntiles;                // row tiles = column tiles = workgroups of ncut_finish_kernel
    int chunk_tiles, nchunks;  // column tiles per workgroup of ncut_apply_kernel, workgroups per row tile
    size_t x16;                // normalised rows [npad, hpad] f16
    size_t y[2];               // the block, f64 [npad][NCUT_NB], two slots (rows >= n zero)
    size_t gram[2];            // f64 [ntiles][64]: per-workgroup partials of Y^T Y of the block in the same slot
    size_t ritz;               // f64 [ntiles][64]: per-workgroup partials of Q^T Y_next of the last step
    size_t deg, cs;            // f64 [npad]: d_i, c_i (rows >= n zero)
    size_t part;               // f64 [nchunks][npad][NCUT_NB]
    size_t part_bytes, bytes;
};
// nchunks = 0: as many chunks as bring the grid to about NCUT_TARGET_WGS workgroups (never more than there are column tiles); a given value
// is lowered where the partials would pass NCUT_PARTIAL_MAX.  Pure: (n, H, nchunks) alone decide every summation order.
inline NcutPlan ncut_plan(int n, int H, int nchunks) {
    NcutPlan p{};
    p.npad = (n + MATCH_TM - 1) / MATCH_TM * MATCH_TM;
    p.hpad = (H + 63) / 64 * 64;
    p.ntiles = p.npad / MATCH_TM;
    const size_t per_chunk = (size_t)p.npad * NCUT_NB * 8;  // <= 8 MiB
    if (nchunks <= 0) nchunks = (NCUT_TARGET_WGS + p.ntiles - 1) / p.ntiles;
    const int cap = (int)(NCUT_PARTIAL_MAX / per_chunk);
    if (nchunks > cap) nchunks = cap;
    if (nchunks > p.ntiles) nchunks = p.ntiles;
    p.chunk_tiles = (p.ntiles + nchunks - 1) / nchunks;
    p.nchunks = (p.ntiles + p.chunk_tiles - 1) / p.chunk_tiles;  // no empty chunk
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += (bytes + 255) / 256 * 256; return off; };
    p.x16 = take((size_t)p.npad * p.hpad * 2);
    for (int k = 0; k < 2; ++k) p.y[k] = take((size_t)p.npad * NCUT_NB * 8);
    for (int k = 0; k < 2; ++k) p.gram[k] = take((size_t)p.ntiles * 64 * 8);
    p.ritz = take((size_t)p.ntiles * 64 * 8);
    p.deg = take((size_t)p.npad * 8);
    p.cs = take((size_t)p.npad * 8);
    p.part_bytes = per_chunk * p.nchunks;
    p.part = take(p.part_bytes);
    p.bytes = need;
    return p;
}
struct NcutBufs {  // the device arrays of one call: views of a workspace (ncut_bufs) or buffers of their own
    _Float16* x16;
    double *y[2], *gram[2], *ritz, *deg, *cs, *part;
};
NcutBufs ncut_bufs(char* ws, const NcutPlan& plan);
// part [nchunks][npad][NCUT_NB] = the chunk sums of sum_j w_ij (scale_j q_j): x16 normalised (launch_match_normalise with nout = npad), scale
// [npad] or nullptr = ones, q [npad][NCUT_NB] or nullptr = a ones column 0 beside seven zero columns (the degree pass).  Columns >= n weigh 0.
hipError_t launch_ncut_apply(const _Float16* x16, int n, int affinity, float tau, float floor, const double* scale, const double* q, double* part,
                             const NcutPlan& plan, hipStream_t stream);
// deg [npad] = the chunk partials' column 0 folded in ascending order, cs = deg > 0 ? 1 / sqrt(deg) : 0; rows >= n get 0 in both
hipError_t launch_ncut_degree(const double* part, int n, double* deg, double* cs, const NcutPlan& plan, hipStream_t stream);
// One step's second half: t = the chunk partials folded in ascending order, ynext = (1/2 (yprev + cs t)) R^-1 with R^-1 = pca_chol_rinv of the
// sum of gprev's ntiles partials; gnext [ntiles][64] and ritz [ntiles][64] = the per-workgroup partials of ynext^T ynext and (yprev R^-1)^T ynext.
// Rows >= n of ynext are written as zeros and contribute nothing.
hipError_t launch_ncut_finish(const double* part, const double* cs, const double* yprev, const double* gprev, int n, double* ynext, double* gnext,
                              double* ritz, const NcutPlan& plan, hipStream_t stream);

// clock probe (device_types.h): per translation unit, [CLK_SLOTS][4] = running sums of shader cycles and 100 MHz ticks of workgroup 0 over
// all launches of each kernel kind on the current device, the 100 MHz end stamp of the last one, the launch count
hipError_t gemm_clock_probe_read(unsigned long long* out);
hipError_t gemm4_clock_probe_read(unsigned long long* out);
hipError_t attention_clock_probe_read(unsigned long long* out);

// testing aid (dinov2_hip_op_stream_delay): one wave that keeps `stream` busy for `milliseconds` of the 100 MHz wall clock, or for a fixed
// number of polls if that comes first; touches no memory
hipError_t launch_stream_delay(int milliseconds, hipStream_t stream);

// debugging aid: what ds_read_b64_tr_b16 returns per lane for addr = lane*8 over an LDS image holding its own
// element index (out: [64][4] int16)
hipError_t launch_probe_tr16(int16_t* out, hipStream_t stream);

}  // namespace dinov2
