/*
 * dinov2_hip_ops.h -- diagnostic single-kernel entry points of libdinov2_hip.so.
 *
 * NOT part of the drop-in boundary (that is include/dinov2_hip.h).  These run one hand-written kernel on host f32
 * data (converted to the compute dtype on the way in, back to f32 on the way out) so the parity tests can check each
 * kernel against the oracle in isolation -- the per-op granularity the reference gets from ggml's own op tests and
 * that /root/reference itself never had (it holds no tests at all).  All return 0 on success, -1 on a HIP error
 * (the entry points with guard bands -- attention_ex, layer_tap, attn_rows, pca_prepare / pca_cov / pca_power / pca_project, dense_reduce,
 * dense_pack, slide_reduce, slide_gather, kmeans_assign / _update / kmeans, vlad, ncut_apply / _step / ncut -- also DINOV2_HIP_OP_GUARD_CHANGED).  Each family has its cases in tests/*_cases.py, CPU probes of those cases and a GPU file; for the
 * pca_* entry points: tests/pca_cases.py, tests/test_pca_probes.py, tests/test_gpu_pca_kernels.py.
 */
#ifndef DINOV2_HIP_OPS_H
#define DINOV2_HIP_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* epilogue ids (csrc/kernels.h): 0 patch-embed(+bias+pos, token scatter) 1 qkv(+bias, q scaled) 2 residual
 * (x += ls*(acc+bias)) 3 gelu 4 swiglu 5 plain f32 (6 .. 9: the LN-fold variants, through dinov2_hip_op_gemm_resid_ln / _ln_consumer).  Replaces ggml_mul_mat call sites of dinov2.cpp:471,546,561,570,
 * 582,608,636 with their trailing elementwise nodes.  `out` is [out_rows, ldo] f32, read first for epilogues 0/2/5. */
int dinov2_hip_op_gemm(int32_t dtype, int32_t epilogue, const float *A, const float *W, const float *bias,
                       const float *aux, int64_t aux_count, float *out, int32_t out_rows, int32_t ldo, int32_t M,
                       int32_t N, int32_t K, int32_t P, int32_t T, int32_t R, int32_t qcols, float qscale);

/* LN fold (csrc/kernels.h, epilogues 6 .. 9), each piece alone.  Statistics rows hold `gs` = 12 (hidden <= 768) or 24
 * slots of (sum, sum of squares) per 64 columns, the slots past hidden / 64 zero.
 *   gemm_resid_ln: x [M, N] f32 in/out += ls * (A W^T + bias); xg [M, N] = T(x gamma) (returned as f32); stats [M][gs][2]
 *   gemm_ln_consumer: epilogue 7 (qkv) | 8 (gelu) | 9 (swiglu) on v = r_m (acc - mean_m s[n]) + c[n], mean / r from `stats` [M][gs][2]
 *   ln_prepare: xg and stats of a residual stream no GEMM has written;  ln_fold_vectors: s[n] = sum_k gamma_k W[n,k], c[n] = bias[n] + sum_k beta_k W[n,k] */
int dinov2_hip_op_gemm_resid_ln(int32_t dtype, const float *A, const float *W, const float *bias, const float *ls, const float *gamma, float *x,
                                float *xg, float *stats, int32_t M, int32_t N, int32_t K);
int dinov2_hip_op_gemm_ln_consumer(int32_t dtype, int32_t epilogue, const float *A, const float *W, const float *ln_s, const float *ln_c,
                                   const float *stats, float eps, float *out, int32_t ldo, int32_t M, int32_t N, int32_t K, int32_t qcols,
                                   float qscale);
/* im2col of the patch embedding (ggml_conv_2d_sk_p0, /root/reference/dinov2.cpp:636): img f32, layout 1 = RGB planar [B,3,H,W], 0 = BGR interleaved
 * [B,H,W,3]; col [B * (H/patch) * (W/patch), Kpad] as f32 values of the compute type, k = c * patch^2 + ky * patch + kx, zero beyond 3 * patch^2 */
int dinov2_hip_op_im2col(int32_t dtype, const float *img, float *col, int32_t B, int32_t Hh, int32_t Ww, int32_t patch, int32_t Kpad, int32_t layout);
/* the same with patches every `stride` pixels (dinov2_hip_load_opts.patch_stride; csrc/kernels.h: im2col_stride_ok -- a pair outside it is refused):
 * col [B * h0 * w0, Kpad], h0 = (H - patch) / stride + 1, w0 likewise, row = (b * h0 + y) * w0 + x */
int dinov2_hip_op_im2col_stride(int32_t dtype, const float *img, float *col, int32_t B, int32_t Hh, int32_t Ww, int32_t patch, int32_t stride,
                                int32_t Kpad, int32_t layout);
int dinov2_hip_op_ln_prepare(int32_t dtype, const float *x, const float *gamma, float *xg, float *stats, int32_t rows, int32_t H);
int dinov2_hip_op_ln_fold_vectors(int32_t dtype, const float *W, const float *bias, const float *gamma, const float *beta, float *s_out,
                                  float *c_out, int32_t N, int32_t K);

/* fused attention over token-major qkv [B*T, 3H] (q already scaled) -> [B*T, H]; replaces dinov2.cpp:479-543 */
int dinov2_hip_op_attention(int32_t dtype, const float *qkv, float *out, int32_t B, int32_t T, int32_t H, int32_t nh);
/* the same with the forward's choice of score domain: log2_scores = 1 runs the instances the forward launches (q pre-scaled by
 * log2(e)/8 in the QKV epilogue, softmax on exp2, csrc/model.cpp), 0 the natural-exp ones (dinov2_hip_op_attention forwards with 0).
 * The kernel and its workgroup size follow the "attn_v" / "attn_nwv" switches exactly as in the forward.  The device output is
 * framed by DINOV2_HIP_OP_GUARD_ROWS rows on either side and the whole buffer starts as 0xffff (NaN in f16 and bf16): a row the
 * kernel did not write comes back as NaN, and a changed guard byte returns DINOV2_HIP_OP_GUARD_CHANGED instead of 0. */
#define DINOV2_HIP_OP_GUARD_ROWS 128
#define DINOV2_HIP_OP_GUARD_CHANGED (-2)
int dinov2_hip_op_attention_ex(int32_t dtype, const float *qkv, float *out, int32_t B, int32_t T, int32_t H, int32_t nh,
                               int32_t log2_scores);

/* Far operands: ONE launch of launch_gemm / launch_attention whose operands end just below the launchers' 32-bit byte-offset limits
 * (M * lda * 2, N * ldw * 2 and B * T * 3H * 2 < 2^32).  Cases, the numpy restatement of the pattern and the sampled rows: tests/far_cases.py;
 * tests/test_far_probes.py (CPU), tests/test_gpu_far.py.  The large operands are written ON THE DEVICE from far_value (csrc/far_pattern.h: a
 * multiple of 1/64 in [-1, 1), a pure function of (seed, row, col)); every device buffer starts as 0xff bytes, so the gap between a row's last
 * column and its stride reads as NaN; the output sits between guard bands of DINOV2_HIP_OP_GUARD_ROWS rows.  Everything is freed on return.
 * Returns 0, -1 (HIP error), DINOV2_HIP_OP_GUARD_CHANGED, DINOV2_HIP_OP_NO_MEMORY (an allocation was refused) or DINOV2_HIP_ERR_INVALID (bad
 * arguments, or a shape the launcher refuses: nothing is allocated or launched then).
 *   device_memory: hipMemGetInfo of the current device.
 *   gemm_far: A [M, K] at row stride lda = far_value(seed_a, m, k); W [N, K] (host f32, rounded as dinov2_hip_op_gemm rounds it; placed at row
 *             stride ldw when ldw > K), bias [N] and aux [N] from the host; epilogue 1 .. 5.  The output [M, ldo] starts as NaN, or, for
 *             epilogue 2, as the f32 values far_value(seed_out, m, n).  out_rows [nrows, N (N / 2 for epilogue 4)] = the output rows rows[i]
 *             as f32; *untouched = the payload elements that still hold their initial bits.
 *   attention_far: qkv [B * T, 3 * 64 * nh] = far_value(seed, row, col) (q counts as already scaled) -> out_rows [nrows, 64 * nh] = the rows
 *             rows[i] of out [B * T, 64 * nh]; the kernel follows "attn_v" / "attn_nwv" as in dinov2_hip_op_attention_ex. */
#define DINOV2_HIP_OP_NO_MEMORY (-3)
int dinov2_hip_op_device_memory(int64_t *free_bytes, int64_t *total_bytes);
int dinov2_hip_op_gemm_far(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldo,
                           uint64_t seed_a, uint64_t seed_out, const float *W, const float *bias, const float *aux, int32_t qcols, float qscale,
                           const int64_t *rows, int32_t nrows, float *out_rows, int64_t *untouched);
int dinov2_hip_op_attention_far(int32_t dtype, int32_t B, int32_t T, int32_t nh, uint64_t seed, int32_t log2_scores, const int64_t *rows,
                                int32_t nrows, float *out_rows, int64_t *untouched);

/* Far rows: the operands of the resident-rows entry points (dinov2_hip_match_tokens, dinov2_hip_bank_add / _topk, dinov2_hip_kmeans_tokens) at
 * the far end of their row offsets.  Cases, the numpy restatement of the selection rule and the exact expectations: tests/rows_far_cases.py;
 * tests/test_rows_far_probes.py (CPU), tests/test_gpu_rows_far.py.
 *   rows_fill: writes rows [row0, row0 + n) of a far operand into the CALLER's device buffer dst_dev as f32 [n, H] at row stride ld (floats,
 *             >= H; the gap H .. ld of a row is left as it is).  Row r of the operand is row far_rows_entry(seed, r, d_common, plants)
 *             (csrc/far_pattern.h) of the host dictionary dict [D, H]: a hash of the full 64-bit row index onto the common entries
 *             [0, d_common), overridden for the at most 256 planted rows (plant_rows strictly ascending, plant_entries[i] in [0, D)).  The caller
 *             owns dst_dev and answers for its size ((n - 1) * ld + H floats); the call touches nothing else, synchronises the device before it
 *             returns and frees what it staged.  A testing aid only: no entry point of include/dinov2_hip.h reaches it.
 *             Returns 0, -1 (HIP error) or DINOV2_HIP_ERR_INVALID (nothing is launched then). */
int dinov2_hip_op_rows_fill(float *dst_dev, int64_t ld, int64_t row0, int64_t n, int32_t H, const float *dict, int32_t D, int32_t d_common,
                            uint64_t seed, const int64_t *plant_rows, const int32_t *plant_entries, int32_t nplants);

/* dinov2_hip_predict_list (include/dinov2_hip.h).  Cases, the numpy restatement of the plan and the per-segment emulation: tests/list_cases.py;
 * tests/test_list_probes.py (CPU), tests/test_gpu_attention_list.py, tests/test_gpu_predict_list.py.
 * list_plan (no device; list_plan of csrc/kernels.h): n images of NETWORK size h[i] x w[i] pixels, `patch` pixels per patch side, R register
 *   tokens, nh heads; order 0 = the work table in list order, 1 = longest images first (equal lengths in list order).
 *   images [n][5] int64 = row0, T, P, h0, w0;  runs [n][2] int32 = first image, count of each run of consecutive images of one size (totals[4]
 *   of them are written);  items [cap_items][4] int32 = row0, T, head, query block (128 queries) of every workgroup of the attention launch,
 *   image-major, then head, then query block;  totals [5] = M (rows), patches, pixels, units (table entries), runs.  images / runs / items may
 *   be NULL.  DINOV2_HIP_ERR_INVALID for bad arguments, cap_items < units, or M >= 2^31.
 * attention_list: launch_attention_list on host data: qkv [sum T, 3H] (q already scaled), n segments of T[i] tokens one after the other ->
 *   out [sum T, H]; each segment is, bit for bit, dinov2_hip_op_attention_ex on it alone (B = 1).  The kernel follows "attn_v" (1 | 2; other
 *   forced values fail) and otherwise the forward's rule on the table's length; the table's order follows "list_order".  Guard bands and NaN
 *   fill as for attention_ex. */
int dinov2_hip_op_list_plan(int32_t n, const int32_t *h, const int32_t *w, int32_t patch, int32_t R, int32_t nh, int32_t order, int64_t *images,
                            int32_t *runs, int32_t *items, int64_t cap_items, int64_t *totals);
int dinov2_hip_op_attention_list(int32_t dtype, const float *qkv, float *out, int32_t n, const int32_t *T, int32_t H, int32_t nh,
                                 int32_t log2_scores);

/* ggml_norm * w + b (dinov2.cpp:694-700); dtype -1 = f32 output (final layernorm), 0/1 = f16/bf16 output */
int dinov2_hip_op_layernorm(int32_t dtype, const float *x, const float *w, const float *b, float *out, int32_t rows,
                            int32_t H, float eps);

/* layer_tap_kernel alone (the kernel behind dinov2_hip_predict_layers, csrc/kernels_misc.hip): x [B, T, H] f32, T = 1 + R + h0 * w0 ->
 * cls_out [B, H] (token 0), reg_out [B, R, H] (tokens 1 .. R), patch_out [B, P, H] (layout 0) or [B, H, h0, w0] (layout 1); any of the three
 * may be NULL.  norm = 1: LayerNorm (w, b, eps) with the bits of dinov2_hip_op_layernorm(dtype = -1); norm = 0: the rows as they are (w, b
 * may be NULL).  Every device output is framed by guard bands of DINOV2_HIP_OP_GUARD_ROWS * H floats and starts as NaN; a changed guard
 * returns DINOV2_HIP_OP_GUARD_CHANGED. */
int dinov2_hip_op_layer_tap(const float *x, const float *w, const float *b, float eps, int32_t B, int32_t T, int32_t R, int32_t H, int32_t h0,
                            int32_t w0, int32_t norm, int32_t layout, float *patch_out, float *cls_out, float *reg_out);

/* attn_rows_kernel alone (the kernel behind dinov2_hip_predict_attention, csrc/attn_rows.hip): qkv [B*T, 3H] host f32, rounded to the compute
 * type on the way in (q already scaled by log2(e)/8, as the forward's QKV epilogue leaves it); queries [nq] host, strictly ascending token
 * indices in [0, T) -> out [B, nh, nq, nkeys] f32 = columns [key0, key0 + nkeys) of the softmax rows over ALL T keys.  The device output is
 * framed by guard bands of DINOV2_HIP_OP_GUARD_ROWS * nkeys floats and starts as NaN; a changed guard returns DINOV2_HIP_OP_GUARD_CHANGED.
 * _ex: lds_budget = the bytes of LDS the scores may take; 0 = the library's own (what the forward uses).  Below 4 T bytes the two-pass form of
 * the kernel runs, which keeps no scores -- the path of sequences too long for the LDS, reachable at test sizes this way.  Same bits. */
int dinov2_hip_op_attn_rows(int32_t dtype, const float *qkv, int32_t B, int32_t T, int32_t H, int32_t nh, const int32_t *queries, int32_t nq,
                            int32_t key0, int32_t nkeys, float *out);
int dinov2_hip_op_attn_rows_ex(int32_t dtype, const float *qkv, int32_t B, int32_t T, int32_t H, int32_t nh, const int32_t *queries, int32_t nq,
                               int32_t key0, int32_t nkeys, float *out, int64_t lds_budget);

/* load-time tensor conversion / dequantisation (F32,F16,BF16,Q4_0,Q4_1,Q5_0,Q5_1,Q8_0 -> compute dtype).  interleaveF > 0: N = 2F rows
 * of a SwiGLU weights_in [x1 (F rows); x2 (F rows)] come out as alternating 32-row blocks x1 | x2 (csrc/model.cpp).  The output
 * starts as NaN (as do those of the layernorm, preprocess_u8, permute_bias and head entry points). */
int dinov2_hip_op_convert_weight(int32_t dtype, const void *src, uint64_t src_bytes, uint32_t ggml_type, float *out,
                                 int32_t N, int32_t K, int32_t Kpad, int32_t interleaveF);
/* the matching bias permutation (permute_bias_kernel): dst[n] = src[source row of weight row n]; interleaveF = 0 copies */
int dinov2_hip_op_permute_bias(const float *src, float *dst, int32_t N, int32_t interleaveF);

/* the classifier head (launch_head, as csrc/model.cpp runs it after the final LayerNorm; dinov2.cpp:792-821): fin [B, T, H] f32,
 * W [C, 2H] (rounded to the compute dtype on the way in), bias [C] -> feat [B, 2H] = [T(cls) ; T(f32(f32(sum_{t >= first} fin) * inv_div))]
 * as f32, logits [B, C], probs [B, C].  H % 4 == 0. */
int dinov2_hip_op_head(int32_t dtype, const float *fin, const float *W, const float *bias, float *feat, float *logits, float *probs,
                       int32_t B, int32_t T, int32_t H, int32_t C, int32_t first, float inv_div);

/* what ds_read_b64_tr_b16 hands each lane for addr = lane*8 over an LDS image of its own indices: out[64][4] */
int dinov2_hip_op_probe_tr16(int16_t *out256);

/* micro-benchmarks on device-resident uniform-random operands: average ms per launch over `iters` launches (HIP events),
 * negative on error.  Used by tools/kernel_bench.py to price one kernel against its roofline. */
float dinov2_hip_op_gemm_bench(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t iters);
float dinov2_hip_op_attention_bench(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t nh, int32_t iters);

/* preprocess_u8_kernel alone: raw 8-bit BGR [B, h, w, 3] -> normalised f32 BGR [B, oh, ow, 3] (mode 0 dino_preprocess,
 * 1 dino_classify_preprocess; sizes from dinov2_hip_preprocess_size).  Replaces dinov2.cpp:106-156 on the device. */
int dinov2_hip_op_preprocess_u8(int32_t mode, const uint8_t *bgr, int32_t B, int32_t h, int32_t w, int32_t patch, float *out);

/* Clock probe.  Workgroup 0 of every launch of the forward's five heavy kernel kinds adds the shader cycles (s_memtime) and the 100 MHz
 * wall-clock ticks (s_memrealtime) it spent in the kernel to running sums on the device: cycles / (ticks * 10 ns) over a window = the clock
 * the power-limited part sustained under that kernel's load.  The sums only grow; take differences.
 * dinov2_hip_op_clock_probe: the FFN-in GEMM (the roofline's dominant kernel).
 * dinov2_hip_op_clock_slots: out18[3 s] = cycles, out18[3 s + 1] = ticks, out18[3 s + 2] = launches, s = 0 QKV GEMM, 1 attn-out GEMM, 2 FFN-in
 * GEMM, 3 FFN-out GEMM, 4 attention (its first workgroup's own lifetime), 5 any other GEMM.  bench.py weights the kinds by their share of the
 * step (`effective_clock_ghz`, `kernel_clocks_ghz`). */
int dinov2_hip_op_clock_probe(uint64_t *cycles, uint64_t *ticks_100mhz);
int dinov2_hip_op_clock_slots(uint64_t *out18);

/* Testing aids.  The switches the library used to read from the environment on every launch (DINOV2_HIP_GEMM_GEN, DINOV2_HIP_GEMM_TILE,
 * DINOV2_HIP_ATTN_V, DINOV2_HIP_ATTN_NWV; include/dinov2_hip.h, "Environment") are read ONCE, on first use; a test that wants to flip one
 * inside a process calls the setter: key = "gemm_gen" | "gemm_tile" | "attn_v" | "attn_nwv" | "list_order", value 0 = the library's own choice,
 * a negative value = back to what the environment said when the library first looked (so a test leaves a `DINOV2_HIP_GEMM_GEN=2 pytest`
 * run as it found it).
 * Not thread-safe against concurrent forwards on other threads in the sense that they may see either value. */
int dinov2_hip_op_set_tuning(const char *key, int32_t value);
int dinov2_hip_op_get_tuning(const char *key); /* -1: unknown key */

/* Which kernel plan the GEMM planner (csrc/gemm.hip gemm_plan; launch_gemm launches it) picks for a shape, as text: ';'-separated leaves such as "gemm4_mixed<256+192>", "gemm2<128>",
 * "gemm4<256>;small<64x128,w2x2,st3,ks1>".  Needs no device (nothing is launched).  0 on success. */
int dinov2_hip_op_gemm_plan(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, char *out, int32_t cap);
/* The same for A and W at row strides lda and ldw (elements; 0 = K).  The plan of a strided call is the plan of (M, N, K); the strides enter the
 * refusals only (a multiple of 8, at least K, M * lda * 2 and N * ldw * 2 below 2^32). */
int dinov2_hip_op_gemm_plan_strided(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, char *out,
                                    int32_t cap);
/* The same plan as data: one record of DINOV2_HIP_PLAN_PART_FIELDS int64 per argument block a kernel of the plan is launched with (a step of
 * a two-height kernel has two, the first possibly empty), in launch order:
 *   0 step (index into the text's leaves)  1 part within the step  2 row0  3 rows  4 col0  5 cols: the rectangle of the output it covers
 *   6 M  7 N  8 K  9 ldo  10 qcols  11 nt_out  12 clk_slot  13 ln_gs: the block's own fields   14 .. 16 nt_out, clk_slot, ln_gs of the whole problem
 *   17 .. 26 byte offsets of the block's A, W, bias, aux, out, xg, stats, ln_gamma, ln_s, ln_c from the caller's pointers
 * Returns the number of records, or -1 for a refused shape or too small a buffer.  Needs no device. */
#define DINOV2_HIP_PLAN_PART_FIELDS 27
int dinov2_hip_op_gemm_plan_parts(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int64_t *out, int32_t cap_records);

/* host-only: the Rayleigh-Ritz step behind dinov2_hip_pca3.  yprev [H][8] (any full-rank block), gram [8][8] = yprev^T yprev,
 * ynext [H][8] = cov * (yprev R^-1) with gram = R^T R  ->  evals [3] largest Ritz values of cov on span(yprev), comp [3][H] their
 * unit Ritz vectors, each with its largest loading positive (H >= 8) */
int dinov2_hip_op_pca_ritz(const double *yprev, const double *ynext, const double *gram, int32_t H, double *evals, double *comp);

/* The device stages of dinov2_hip_pca3 (csrc/pca.cpp), one at a time and without a model or session, each through the launch function
 * the driver itself calls (csrc/kernels.h: launch_pca_prepare, launch_pca_cov, launch_pca_power, launch_pca_project).  P >= 4, 8 <= H <= 4096
 * as the driver requires.  Every device output is framed by guard bands of DINOV2_HIP_OP_GUARD_ROWS rows of its own row width and the whole
 * buffer starts as 0xff bytes (NaN in f16, f32 and f64); a changed guard returns DINOV2_HIP_OP_GUARD_CHANGED, bad arguments
 * DINOV2_HIP_ERR_INVALID.  Cases, emulations and bounds: tests/pca_cases.py; tests/test_pca_probes.py (CPU), tests/test_gpu_pca_kernels.py.
 *   pca_ppad / pca_blocks: Ppad (the padded token count, K of the covariance GEMM) and the power kernel's grid size, as the driver computes them
 *   pca_prepare: pca_mean_kernel + pca_center_transpose_kernel: tok [P, H] -> mean_out [H], xt_out [H, Ppad] = the f32 values of the f16 matrix
 *                (tok - mean)^T, the padded columns p >= P included (they must be 0)
 *   pca_cov:     prepare (into an xt that starts as NaN) + the covariance GEMM with A == W aliased: cov_out [H, H] = Xt Xt^T, f32
 *   pca_power:   one pca_power_kernel launch: cov [H, H] f32, yprev [H][8], gprev_parts [pca_blocks(H)][64] (partial Gram sums of yprev; only
 *                their sum matters) -> ynext [H][8] = cov (yprev R^-1), gnext_parts [pca_blocks(H)][64] = the Gram of each workgroup's 16 rows
 *   pca_project: pca_project_kernel: proj [P, 3] = (tok - mean) comp^T, comp [3, H]
 *   pca_chol_rinv (host-only): gram [8][8] -> rinv [8][8], the CholeskyQR factor shared by the power kernel and pca_ritz (csrc/kernels.h) */
int dinov2_hip_op_pca_ppad(int32_t P);
int dinov2_hip_op_pca_blocks(int32_t H);
int dinov2_hip_op_pca_prepare(const float *tok, int32_t P, int32_t H, float *mean_out, float *xt_out);
int dinov2_hip_op_pca_cov(const float *tok, int32_t P, int32_t H, float *cov_out);
int dinov2_hip_op_pca_power(const float *cov, const double *yprev, const double *gprev_parts, int32_t H, double *ynext, double *gnext_parts);
int dinov2_hip_op_pca_project(const float *tok, const float *mean, const float *comp, int32_t P, int32_t H, float *proj);
int dinov2_hip_op_pca_chol_rinv(const double *gram, double *rinv);

/* the three kernels behind dinov2_hip_match_tokens (csrc/match.hip) without a model or session: host a [na, H], b [nb, H] in; host idx_ab [na],
 * sim_ab [na], idx_ba [nb], sim_ba [nb] out (all four required).  Same ranges and contract as dinov2_hip_match.  The workspace is filled
 * with 0xff bytes first, so padding that the kernels fail to zero shows up as NaN. */
int dinov2_hip_op_match(const float *a, int32_t na, const float *b, int32_t nb, int32_t H, int32_t *idx_ab, float *sim_ab, int32_t *idx_ba,
                        float *sim_ba);

/* the two kernels behind dinov2_hip_bank_topk (csrc/bank.hip) and the shared normaliser, without a model or session: host q [nq, H] against
 * host b [nb, H] (all of them counted); host idx / sim [nq, k] out (both required).  1 <= nq <= 2^20, 1 <= nb <= 2^24, 8 <= H <= 4096,
 * 1 <= k <= 64.  chunk_tiles: column tiles per workgroup, 0 = the planner's choice (a value that would take the partial lists past their
 * bound is raised).  The workspace and the bank are filled with 0xff bytes first, so anything the kernels read without having written it
 * shows up as NaN. */
int dinov2_hip_op_bank_topk(const float *q, int32_t nq, const float *b, int32_t nb, int32_t H, int32_t k, int32_t chunk_tiles, int32_t *idx,
                            float *sim);
/* the plan of such a call (bank_topk_plan, csrc/kernels.h; no device): out[0 .. 5] = chunk_tiles, nchunks, pass_tiles, ntiles, bytes of the
 * partial lists, bytes of the whole workspace.  Returns 0, or DINOV2_HIP_ERR_INVALID for sizes out of range. */
int dinov2_hip_op_bank_plan(int32_t nq, int32_t nb, int32_t H, int32_t k, int32_t chunk_tiles, int64_t *out);
/* measuring aid (tools/bank_bench.py): DEVICE f32 queries q_dev [nq, H] against a bank built here from the DEVICE f32 rows b_dev [nb, H];
 * `warmup` + `iters` searches (normalise the queries, sweep, merge) on the null stream, the mean milliseconds of the timed ones by HIP events
 * in *ms.  floor_only = 1: the sweep with its selection epilogue compiled out (the kernel's own floor; its results mean nothing). */
int dinov2_hip_op_bank_bench(const float *q_dev, int32_t nq, const float *b_dev, int32_t nb, int32_t H, int32_t k, int32_t chunk_tiles,
                             int32_t warmup, int32_t iters, int32_t floor_only, float *ms);

/* the kernels behind dinov2_hip_propagate (csrc/propagate.hip) with the shared normaliser and the bank's merge, without a model or session:
 * host q [P, H] (P = h0 w0) against a memory built here from host rows [frames, P, H] and labels [frames, P, C] -- every slot is written,
 * `slots` says which ones are context (bits below `frames` only, at least one) -> out [P, C], argmax [P], idx / sim [P, k] (all required)
 * and, unless NULL, kept [P, C]: what a call with keep leaves in the memory.  Limits as dinov2_hip_propmem_create / dinov2_hip_propagate,
 * else DINOV2_HIP_ERR_INVALID.  chunk_tiles: items (active slot x kept column tile) per workgroup, 0 = the planner's choice (raised where
 * the partials would pass their bound).  The memory and the workspace are filled with 0xff bytes first, so the padding rows of a slot and
 * anything the kernels read without having written it are NaN.
 * propagate_plan (no device): propagate_plan of csrc/kernels.h for `nactive` set slots: out[0 .. 7] = chunk_tiles, nchunks, query tiles,
 *   the most items of a query tile, the items of all query tiles together, bytes of the partials, bytes of the workspace, bytes of a memory
 *   of nactive frames; ranges (may be NULL) [query tiles][2] = the kept column tiles [t0, t1) of every query tile.
 * propagate_bench (tools/propagate_bench.py): DEVICE q_dev [P, H] and rows_dev [frames, P, H], labels zero: *ms = one call's device work
 *   (normalise, select, merge, combine with keep), the mean of `iters` after `warmup`. */
int dinov2_hip_op_propagate(const float *q, const float *rows, const float *labels, int32_t h0, int32_t w0, int32_t H, int32_t frames, int32_t C,
                            uint64_t slots, int32_t radius, int32_t k, float temperature, int32_t chunk_tiles, float *out, int32_t *argmax,
                            int32_t *idx, float *sim, float *kept);
int dinov2_hip_op_propagate_plan(int32_t h0, int32_t w0, int32_t H, int32_t nactive, int32_t radius, int32_t k, int32_t C, int32_t chunk_tiles,
                                 int64_t *out, int32_t *ranges);
int dinov2_hip_op_propagate_bench(const float *q_dev, const float *rows_dev, int32_t h0, int32_t w0, int32_t H, int32_t frames, int32_t C,
                                  uint64_t slots, int32_t radius, int32_t k, float temperature, int32_t chunk_tiles, int32_t warmup, int32_t iters,
                                  float *ms);

/* the kernels behind dinov2_hip_kmeans_tokens (csrc/kmeans.hip) and the shared normaliser, without a model or session; cases, the numpy
 * restatement and the bounds: tests/kmeans_cases.py.  1 <= n <= 2^20, 1 <= K <= 1024, 8 <= H <= 4096, else DINOV2_HIP_ERR_INVALID.  Every
 * device buffer starts as 0xff bytes, so anything the kernels read without having written it shows up as NaN / -1; labels, sim, centres and
 * counts sit between guard bands: a changed one returns DINOV2_HIP_OP_GUARD_CHANGED.
 * kmeans_assign: host rows [n, H] against host centers [K, H] (vectors of any length) -> labels [n], sim [n] (both required): one
 *                kmeans_assign_kernel launch, contract 2.
 * kmeans_update: transpose, update and finish for GIVEN labels_in [n] in [0, K): centers_out [K, H] = prev_centers with the vector of every
 *                cluster that has members replaced by its sum S_c (contract 3 / 4), counts [K]; xhat_f16_as_f32 [n, H] (may be NULL) = the f32
 *                values of the f16 rows that were summed.  nsplit: chunks of rows, 0 = the planner's choice.
 * kmeans_plan (no device): out[0 .. 7] = npad, kpad, hpad, hpad128, chunk rows, nsplit, bytes of the partials, bytes of the workspace.
 * kmeans:        the whole loop of dinov2_hip_kmeans_tokens on host rows; init_centers [K, H] or (when it is NULL) init_rows [K]; any output
 *                may be NULL.
 * kmeans_bench (tools/kmeans_bench.py): DEVICE f32 rows_dev [n, H], centres = the first K rows: ms[0] = one assignment, ms[1] = one update
 *                (sweep, fold, normalise), ms[2] = the whole call (normalise, transpose, `max_iter` iterations with their 4-byte reads), each
 *                the mean of `iters` timed runs after `warmup`, by HIP events on the null stream. */
int dinov2_hip_op_kmeans_assign(const float *rows, int32_t n, const float *centers, int32_t K, int32_t H, int32_t *labels, float *sim);
int dinov2_hip_op_kmeans_update(const float *rows, int32_t n, const int32_t *labels_in, int32_t K, int32_t H, int32_t nsplit,
                                const float *prev_centers, float *centers_out, int32_t *counts, float *xhat_f16_as_f32);
int dinov2_hip_op_kmeans_plan(int32_t n, int32_t K, int32_t H, int32_t nsplit, int64_t *out);
int dinov2_hip_op_kmeans(const float *rows, int32_t n, int32_t K, int32_t H, int32_t max_iter, const float *init_centers,
                         const int32_t *init_rows, int32_t *labels, float *sim, float *centers, int32_t *counts, int32_t *iterations,
                         int32_t *converged);
int dinov2_hip_op_kmeans_bench(const float *rows_dev, int32_t n, int32_t K, int32_t H, int32_t nsplit, int32_t max_iter, int32_t warmup,
                               int32_t iters, float *ms);

/* the kernels behind dinov2_hip_coreset_tokens (csrc/coreset.hip) and the shared normaliser, without a model or session; cases and the numpy
 * restatement of the greedy rule: tests/coreset_cases.py.  1 <= n <= 2^20, 8 <= H <= 4096, 1 <= m <= n, 0 <= first < n, stop_sim not NaN,
 * rows_per_wg >= 0, else DINOV2_HIP_ERR_INVALID.
 * coreset:       host rows [n, H] -> idx [m], cover [m], *selected, nearest [n], near_sim [n] (any may be NULL).  rows_per_wg: rows per
 *                workgroup, 0 = the planner's choice (a value is rounded up to whole 128-row tiles and raised where n needs it).  The
 *                workspace is filled with 0xff bytes first, so anything the kernels read without having written it shows up as NaN / -1.
 * coreset_plan (no device): out[0 .. 4] = npad, hpad, rows per workgroup, partials (= workgroups), bytes of the workspace for m picks.
 * coreset_bench (tools/coreset_bench.py): DEVICE f32 rows_dev [n, H], first = 0, never stops: *us_per_pick = the time of `m` sweep
 *                launches in a row divided by m, the mean of `iters` timed chains after `warmup`, by HIP events on the null stream. */
int dinov2_hip_op_coreset(const float *rows, int32_t n, int32_t H, int32_t m, int32_t first, float stop_sim, int32_t rows_per_wg, int32_t *idx,
                          float *cover, int32_t *selected, int32_t *nearest, float *near_sim);
int dinov2_hip_op_coreset_plan(int32_t n, int32_t H, int32_t m, int32_t rows_per_wg, int64_t *out);
int dinov2_hip_op_coreset_bench(const float *rows_dev, int32_t n, int32_t H, int32_t m, int32_t rows_per_wg, int32_t warmup, int32_t iters,
                                float *us_per_pick);

/* the kernels behind dinov2_hip_ncut_tokens (csrc/ncut.hip), its loop (csrc/ncut.cpp) and the shared normaliser, without a model or session;
 * cases, the numpy restatement and the bounds: tests/ncut_cases.py.  16 <= n <= 131 072, 8 <= H <= 4096, affinity, tau and floor as in
 * dinov2_hip_ncut, else DINOV2_HIP_ERR_INVALID.  Every device buffer starts as 0xff bytes; the partials, both blocks, the 8 x 8 partials,
 * the degrees and c sit between guard bands: a changed one returns DINOV2_HIP_OP_GUARD_CHANGED.  The block width is 8 throughout.
 * ncut_plan (no device): out[0 .. 7] = npad, hpad, row tiles, column tiles per chunk, chunks, bytes of the partials, bytes of the workspace, 0.
 *             nchunk: chunks of column tiles, 0 = the planner's choice.
 * ncut_apply: host rows [n, H]; t_out [n, 8] f64 = the raw sums sum_j w_ij scale_j q_jc (scale [n] f64 or NULL = ones, q [n, 8] f64; the
 *             chunk partials of one ncut_apply_kernel launch folded in ascending order), degree_out [n] f64 = d_i (the degree pass and
 *             ncut_degree_kernel), xhat_f16_as_f32 [n, H] = the f32 values of the f16 rows.  Any output may be NULL, not all; t_out needs q.
 * ncut_step:  one full step of contract 5 from yprev [n, 8] f64 and the partials gprev_parts [row tiles, 64] f64 of its Gram matrix (their
 *             sum in ascending order is the matrix): the degree pass, ncut_apply_kernel on c and yprev, ncut_finish_kernel -> ynext [n, 8],
 *             gnext_parts and ritz_parts [row tiles, 64]: the per-workgroup partials of ynext^T ynext and (yprev R^-1)^T ynext.  All required.
 * ncut:       the whole of dinov2_hip_ncut_tokens on host rows; any output may be NULL.
 * ncut_bench (tools/ncut_bench.py): DEVICE f32 rows_dev [n, H]: ms[0] = one ncut_apply_kernel launch, ms[1] = one ncut_finish_kernel launch,
 *             ms[2] = the whole call (normalise, degrees, the loop with its checks, the vectors), each the mean of `iters` timed runs after
 *             `warmup`, by HIP events on the null stream; steps[0] = the steps the whole call took. */
int dinov2_hip_op_ncut_plan(int32_t n, int32_t H, int32_t nchunk, int64_t *out);
int dinov2_hip_op_ncut_apply(const float *rows, int32_t n, int32_t H, int32_t affinity, float tau, float floor, const double *scale,
                             const double *q, int32_t nchunk, double *t_out, double *degree_out, float *xhat_f16_as_f32);
int dinov2_hip_op_ncut_step(const float *rows, int32_t n, int32_t H, int32_t affinity, float tau, float floor, int32_t nchunk,
                            const double *yprev, const double *gprev_parts, double *ynext, double *gnext_parts, double *ritz_parts);
int dinov2_hip_op_ncut(const float *rows, int32_t n, int32_t H, int32_t affinity, float tau, float floor, int32_t n_eig, int32_t max_iter,
                       float tol, float *values, float *vectors, float *degree, float *residual, int32_t *iterations, int32_t *converged);
int dinov2_hip_op_ncut_bench(const float *rows_dev, int32_t n, int32_t H, int32_t affinity, float tau, float floor, int32_t nchunk,
                             int32_t n_eig, int32_t max_iter, float tol, int32_t warmup, int32_t iters, float *ms, int32_t *steps);

/* the kernels behind dinov2_hip_vlad_tokens (csrc/vlad.hip) with the shared normaliser and k-means' transpose, without a model or session;
 * cases, the numpy restatement and the bounds: tests/vlad_cases.py.  offsets [n_seg + 1] strictly ascending from 0 to at most 2^20,
 * 1 <= n_seg <= 4096, 1 <= K <= 1024, 8 <= H <= 4096, n_seg K H <= 2^28, flags within DINOV2_HIP_VLAD_INTRA_NORM | _L2_NORM, else
 * DINOV2_HIP_ERR_INVALID.  Every device buffer starts as 0xff bytes; labels (padded and the caller's order), sim, counts, the rows' sums
 * of squares and the descriptors sit between guard bands: a changed one returns DINOV2_HIP_OP_GUARD_CHANGED.
 * vlad_plan (no device): out[0 .. 11] = kpad, hpad, hpad128, chunk rows, chunks per pass, rows of the padded layout, its tiles, chunks,
 *             passes, bytes of the partials, bytes of the workspace, 0; segs [n_seg, 4] (may be NULL) = first padded row, length, first
 *             chunk, chunks of every segment; chunks [max_chunks, 3] (may be NULL; max_chunks below the plan's count is refused) =
 *             segment, first padded row, K-tiles of every chunk.
 * vlad:       host rows [offsets[n_seg], H] and centers [K, H] through the whole of the call's device work; any output may be NULL:
 *             labels, sim [n], counts [n_seg, K], vlad [n_seg, K, H], and the f32 values of the f16 operands xhat_f16_as_f32 [n, H],
 *             chat_f16_as_f32 [K, H].
 * vlad_bench (tools/vlad_bench.py): DEVICE rows_dev [n, H] and centers_dev [K, H]: ms[0] = the assignment, ms[1] = sums, finish and L2 step,
 *             ms[2] = the whole device work (normalise, assign, transpose, sums), each the mean of `iters` timed runs after `warmup`, by HIP
 *             events on the null stream. */
int dinov2_hip_op_vlad_plan(const int32_t *offsets, int32_t n_seg, int32_t K, int32_t H, int64_t *out, int32_t *segs, int32_t *chunks,
                            int32_t max_chunks);
int dinov2_hip_op_vlad(const float *rows, const int32_t *offsets, int32_t n_seg, const float *centers, int32_t K, int32_t H, uint32_t flags,
                       int32_t *labels, float *sim, int32_t *counts, float *vlad, float *xhat_f16_as_f32, float *chat_f16_as_f32);
int dinov2_hip_op_vlad_bench(const float *rows_dev, const int32_t *offsets, int32_t n_seg, const float *centers_dev, int32_t K, int32_t H,
                             uint32_t flags, int32_t warmup, int32_t iters, float *ms);

/* the two kernels of csrc/dense.hip (behind dinov2_hip_predict_dense) without a model or session; cases and the numpy restatement:
 * tests/dense_cases.py.
 * dense_reduce: host logits [h0 * w0, C] f32 (one image, token-major) -> labels [out_h, out_w] u8 (ARGMAX only; NULL otherwise) and / or value
 *               [out_h, out_w] f32, contracts 3 - 5 of dinov2_hip_predict_dense.  reduce 0 ARGMAX, 1 BINS (centers [C], eps > 0).  1 <= C <= 256,
 *               out_h, out_w 1 .. 8192.  Each device output is framed by guard bands of DINOV2_HIP_OP_GUARD_ROWS * out_w elements and starts as
 *               0xff bytes; a changed guard returns DINOV2_HIP_OP_GUARD_CHANGED.
 * dense_pack:   x [B, T, H] f32, T = 1 + R + P -> out_f16_as_f32 [B * P, nslots * H * (1 + concat_cls)]: the f32 values of the f16 operand after
 *               ONE dense_pack launch into column block `slot`; the other blocks come back as NaN (the operand starts as 0xff bytes and is
 *               framed by guard bands).  norm = 1: LayerNorm (w, b, eps); H % 8 == 0.
 * dense_reduce_plan (no device): out[0 .. 5] = tile_y, tile_x, span_y, span_x, pitch, LDS bytes of dense_reduce_plan (csrc/kernels.h). */
int dinov2_hip_op_dense_reduce(const float *logits, int32_t h0, int32_t w0, int32_t C, int32_t out_h, int32_t out_w, int32_t reduce,
                               const float *centers, float eps, uint8_t *labels, float *value);
int dinov2_hip_op_dense_pack(const float *x, const float *ln_w, const float *ln_b, float eps, int32_t B, int32_t T, int32_t R, int32_t H,
                             int32_t norm, int32_t concat_cls, int32_t slot, int32_t nslots, float *out_f16_as_f32);
int dinov2_hip_op_dense_reduce_plan(int32_t h0, int32_t w0, int32_t C, int32_t out_h, int32_t out_w, int64_t *out);

/* the two kernels of csrc/slide.hip (behind dinov2_hip_predict_dense_slide) without a model or session; cases and the numpy restatement:
 * tests/slide_cases.py.  y1 [ny], x1 [nx]: window starts -- ascending, inside the image, the first at 0, the last ending at the image edge, no
 * gap between neighbours (what dinov2_hip_slide_windows gives); anything else is DINOV2_HIP_ERR_INVALID, as is a cover above 16.
 * slide_reduce:  host logits [ny * nx, h0 * w0, C] f32 (one image's windows in index order, token-major) -> labels [h, w] u8 (ARGMAX only; NULL
 *                otherwise) and / or value [h, w] f32, contracts 3 and 4 of dinov2_hip_predict_dense_slide.  reduce, centers, eps as for
 *                dense_reduce.  Each device output is framed by guard bands of DINOV2_HIP_OP_GUARD_ROWS * w elements and starts as 0xff bytes; a
 *                changed guard returns DINOV2_HIP_OP_GUARD_CHANGED.
 * slide_gather:  host image [3, h, w] (layout DINOV2_HIP_RGB_CHW) or [h, w, 3] (DINOV2_HIP_BGR_HWC) f32 -> windows [ny * nx, ...] of crop_h x
 *                crop_w in the same layout, framed and pre-filled the same way (guard row: crop_w * 3 elements).
 * slide_reduce_plan (no device): out[0 .. 9] = tile_y, tile_x, slots_y, slots_x, span_y, span_x, classes per chunk, pitch, LDS bytes, cover of
 *                slide_reduce_plan (csrc/kernels.h). */
int dinov2_hip_op_slide_reduce(const float *logits, int32_t h0, int32_t w0, int32_t C, int32_t crop_h, int32_t crop_w, int32_t h, int32_t w,
                               const int32_t *y1, int32_t ny, const int32_t *x1, int32_t nx, int32_t reduce, const float *centers, float eps,
                               uint8_t *labels, float *value);
int dinov2_hip_op_slide_gather(const float *image, int32_t layout, int32_t h, int32_t w, int32_t crop_h, int32_t crop_w, const int32_t *y1,
                               int32_t ny, const int32_t *x1, int32_t nx, float *windows);
int dinov2_hip_op_slide_reduce_plan(int32_t h0, int32_t w0, int32_t C, int32_t crop_h, int32_t crop_w, int32_t h, int32_t w, const int32_t *y1,
                                    int32_t ny, const int32_t *x1, int32_t nx, int64_t *out);

/* A bounded stall for the stream-ordering tests (tests/stream_cases.py, DESIGN.md "Stream contract"): queues ONE kernel of one wave on
 * `stream` (a hipStream_t) that polls the 100 MHz wall clock, sleeping between polls, and ends after `milliseconds` or after a fixed number
 * of polls (65 536, a few hundred milliseconds), whichever comes first: a wait with an upper bound, never a hang.  It touches no memory.
 * Work queued on the stream behind it starts when it ends; the call itself returns at once.  milliseconds outside 1 .. 100 and
 * stream == NULL (the null stream would order every other stream behind the stall) return DINOV2_HIP_ERR_INVALID before any HIP call. */
int dinov2_hip_op_stream_delay(void *stream, int32_t milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* DINOV2_HIP_OPS_H */
