// rerank.hip -- row ranges of a bank scored against one query set (dinov2_hip_bank_rerank, include/dinov2_hip.h) for gfx950 (MI355X).
//
// No reference counterpart: the re-ranking step of retrieval on frozen patch tokens -- every query token against every token of each of a
// shortlist of candidates, a candidate scored by the sum of the per-token maxima (MaxSim / Chamfer) and by its mutual nearest neighbours.
// Two kernels:
//   rerank_tile_kernel  one workgroup per item (segment, 128-row query tile) of a work table: the query tile against the segment's 128-column
//                       tiles in ascending order, each a sim_tile.  The best column of a query row stays in registers over the walk and is
//                       folded over lanes and waves once, at the end; the best query row of a column is reduced per tile, as in
//                       match_kernel's epilogue, into one partial per (item, column).  A segment starts at any row of the bank, so its
//                       tiles are not the bank's: the B operand clamps its rows to the allocation (SimRowsClamped) and columns >= len are
//                       masked.  The similarity matrix is never written.
//   rerank_fold_kernel  one workgroup per segment: the column partials folded over the query tiles in ascending order, the winning query row
//                       of every column kept in LDS (16 bits each: n <= 16 384) for the mutual test; the four sums.
// The tile, the K order of a pair and the total order of "best" are sim_tile.h's.  No atomics.
#include "sim_tile.h"

namespace dinov2 {

// Q [nq_pad, hpad]: the normalised queries, rows >= n zero.  bank: rows 0 .. last_row of hpad f16.  Item (seg, qt):
// prow_*[(seg - seg0) * nq_pad + 128 qt + r] = best column (0 .. len - 1, relative to the segment) of query row 128 qt + r;
// pcol_*[segs[seg].pcol + qt * lpad + c] = best row among this tile's real query rows of the segment's column c.
__global__ __launch_bounds__(256) void rerank_tile_kernel(const _Float16* __restrict__ Q, const _Float16* __restrict__ bank, int last_row, int hpad,
                                                          int n, int nq_pad, const RerankItem* __restrict__ items,
                                                          const RerankSeg* __restrict__ segs, int seg0, float* __restrict__ prow_v,
                                                          int* __restrict__ prow_i, float* __restrict__ pcol_v, int* __restrict__ pcol_i) {
    __shared__ __attribute__((aligned(16))) char sA[SIM_TILE * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) char sB[SIM_TILE * SIM_ROWB];
    __shared__ float red_rv[2][SIM_TILE], red_cv[2][SIM_TILE];
    __shared__ int red_ri[2][SIM_TILE], red_ci[2][SIM_TILE];

    const SimPlace p;
    const RerankItem it = items[blockIdx.x];
    const RerankSeg sg = segs[it.seg];
    const int m0 = it.qt * SIM_TILE, lpad = (sg.len + SIM_TILE - 1) / SIM_TILE * SIM_TILE;
    const size_t col_out = (size_t)sg.pcol + (size_t)it.qt * lpad;
    SimRows opa(p, Q, m0, hpad);
    Best best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) best[i] = Best{-INFINITY, INT_MAX};
    for (int n0 = 0; n0 < lpad; n0 += SIM_TILE) {  // the segment's column tiles in ascending order
        SimRowsClamped opb(p, bank, sg.first + n0, last_row, hpad);
        f32x4 acc[4][4];
        sim_tile(p, sA, sB, hpad / 64, opa, opb, acc);
        // acc[i][j][r] = sim(row, col), row = m0 + 64 wm + 16 i + fr, col = n0 + 64 wn + 16 j + 4 fh + r of the segment; columns >= len masked
#pragma unroll
        for (int i = 0; i < 4; ++i) sim_row_fold(acc, i, n0 + p.wn * 64 + 4 * p.fh, sg.len, best[i]);
        // per column over this wave's 64 rows (rows >= n masked), then the two waves above each other
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Best b{-INFINITY, INT_MAX};
                sim_col_fold(acc, j, r, m0 + p.wm * 64 + p.fr, n, b);
                sim_col_share(p, j, r, b, red_cv, red_ci);
            }
        __syncthreads();  // (the next tile's sim_tile has two barriers before anything writes red_c* again)
        if (p.tid < SIM_TILE) {
            const Best b = sim_fold_waves(red_cv, red_ci, p.tid);
            pcol_v[col_out + n0 + p.tid] = b.v;
            pcol_i[col_out + n0 + p.tid] = b.i;
        }
    }
    // per row: the four lanes that share it, then the two waves side by side
#pragma unroll
    for (int i = 0; i < 4; ++i) sim_row_share(p, i, best[i], red_rv, red_ri);
    __syncthreads();
    if (p.tid < SIM_TILE) {
        const Best b = sim_fold_waves(red_rv, red_ri, p.tid);
        const size_t o = (size_t)(it.seg - seg0) * nq_pad + m0 + p.tid;
        prow_v[o] = b.v;
        prow_i[o] = b.i;
    }
}

// The sum of x over the 256 threads in a fixed tree: the lanes of a wave by xor 1, 2, 4, 8, 16, 32 (both partners add the same two values,
// and f32 addition commutes), then the four waves as (w0 + w1) + (w2 + w3).  Every thread returns the total.
template <typename T>
__device__ __forceinline__ T rerank_sum256(T x, T (&red)[4]) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off);
    __syncthreads();  // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Workgroup x = segment seg0 + x of the list.  Thread t owns columns t, t + 256, ... and, afterwards, query rows t, t + 256, ...: each
// thread sums its own in ascending order, then rerank_sum256.
__global__ __launch_bounds__(256) void rerank_fold_kernel(const RerankSeg* __restrict__ segs, int seg0, int n, int nq_pad, int qtiles,
                                                          float min_sim, const float* __restrict__ prow_v, const int* __restrict__ prow_i,
                                                          const float* __restrict__ pcol_v, const int* __restrict__ pcol_i,
                                                          float* __restrict__ score_q, float* __restrict__ score_b, int* __restrict__ mutual,
                                                          float* __restrict__ mutual_sim) {
    __shared__ unsigned short idx_b[RERANK_LEN_MAX];  // the best query row of every column of the segment
    __shared__ float red_f[4];
    __shared__ int red_n[4];
    const int tid = threadIdx.x, seg = seg0 + blockIdx.x;
    const RerankSeg sg = segs[seg];
    const int lpad = (sg.len + SIM_TILE - 1) / SIM_TILE * SIM_TILE;
    float sb = 0.0f;
    for (int j = tid; j < sg.len; j += 256) {
        Best b{-INFINITY, INT_MAX};
        for (int t = 0; t < qtiles; ++t) {  // query tiles in ascending order
            const size_t o = (size_t)sg.pcol + (size_t)t * lpad + j;
            fold(b, pcol_v[o], pcol_i[o]);
        }
        idx_b[j] = (unsigned short)b.i;
        sb += b.v;
    }
    __syncthreads();
    float sq = 0.0f, sm = 0.0f;
    int cnt = 0;
    for (int i = tid; i < n; i += 256) {
        const size_t o = (size_t)blockIdx.x * nq_pad + i;
        const float v = prow_v[o];
        const int c = prow_i[o];
        sq += v;
        if ((unsigned)c < (unsigned)sg.len && (int)idx_b[c] == i && v >= min_sim) {
            ++cnt;
            sm += v;
        }
    }
    sb = rerank_sum256(sb, red_f);
    sq = rerank_sum256(sq, red_f);
    sm = rerank_sum256(sm, red_f);
    cnt = rerank_sum256(cnt, red_n);
    if (tid == 0) {
        score_q[seg] = sq;
        score_b[seg] = sb;
        mutual[seg] = cnt;
        mutual_sim[seg] = sm;
    }
}

hipError_t launch_rerank(const float* q, size_t ldq, int n, int H, const _Float16* bank, int last_row, int n_seg, float min_sim, char* ws,
                         const RerankPlan& p, const RerankTables& t, hipStream_t st) {
    _Float16* const q16 = (_Float16*)(ws + p.q16);
    hipError_t e = launch_match_normalise(q, ldq, q16, n, p.nq_pad, H, p.hpad, st);
    if (e != hipSuccess) return e;
    RerankSeg* const segs = (RerankSeg*)(ws + p.segs);
    RerankItem* const items = (RerankItem*)(ws + p.items);
    float *prow_v = (float*)(ws + p.prow_v), *pcol_v = (float*)(ws + p.pcol_v);
    int *prow_i = (int*)(ws + p.prow_i), *pcol_i = (int*)(ws + p.pcol_i);
    e = hipMemcpyAsync(segs, t.segs.data(), (size_t)n_seg * sizeof(RerankSeg), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    for (const RerankPass& ps : t.passes) {
        const int n_items = ps.nseg * p.qtiles;
        // (stream order: the pass before has read the table by the time this copy runs)
        e = hipMemcpyAsync(items, t.items.data() + ps.item0, (size_t)n_items * sizeof(RerankItem), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(rerank_tile_kernel, dim3(n_items), dim3(256), 0, st, q16, bank, last_row, p.hpad, n, p.nq_pad, items, segs, ps.seg0,
                           prow_v, prow_i, pcol_v, pcol_i);
        hipLaunchKernelGGL(rerank_fold_kernel, dim3(ps.nseg), dim3(256), 0, st, segs, ps.seg0, n, p.nq_pad, p.qtiles, min_sim, prow_v, prow_i,
                           pcol_v, pcol_i, (float*)(ws + p.score_q), (float*)(ws + p.score_b), (int*)(ws + p.mutual),
                           (float*)(ws + p.mutual_sim));
    }
    return hipGetLastError();
}

}  // namespace dinov2
