// match.hip -- nearest rows by cosine similarity in both directions (dinov2_hip_match_tokens, include/dinov2_hip.h) for gfx950 (MI355X).
//
// No reference counterpart: the dense-correspondence figure of the DINOv2 paper (for every patch of image A the most similar patch of image
// B, and back; mutual nearest neighbours kept), k-NN / retrieval with k = 1 on CLS vectors.  Three kernels:
//   match_normalise_kernel  f32 rows -> unit rows in f16, [npad, hpad], padding rows and columns zero (one wave per row)
//   match_kernel            one workgroup per 128 x 128 tile of the na x nb similarity matrix: K loop over hpad through LDS into
//                           v_mfma_f32_16x16x32_f16 accumulators; the matrix is never written -- the epilogue reduces the accumulators per row
//                           (best value, lowest column) and per column (best value, lowest row) and stores one partial per (row, column
//                           tile) and one per (column, row tile)
//   match_reduce_kernel     folds the partials of a row (column) over the column (row) tiles
// Both directions come from the same accumulators.  The tile, the K order of a pair and the total order of "best" are sim_tile.h's.
#include "normalise_row.h"
#include "sim_tile.h"

namespace dinov2 {

// x: rows [n] of H floats, row stride ld.  out [nout, hpad] f16: match_normalise_row of every row, zeros for rows >= n; rows >= nout are
// not touched (the grid covers nout rounded up to 4).  Four rows per workgroup, one wave each.
__global__ __launch_bounds__(256) void match_normalise_kernel(const float* __restrict__ x, size_t ld, _Float16* __restrict__ out, int n,
                                                              int nout, int H, int hpad, int vec) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)nout) return;
    match_normalise_row(row < (size_t)n ? x + row * ld : nullptr, (f16x4*)(out + row * hpad), threadIdx.x & 63, H, hpad, vec);
}

// A [na_pad, hpad], B [nb_pad, hpad]: the normalised operands.  Workgroup (x, y) owns rows [row0 + 128 y, +128) and columns
// [col0 + 128 x, +128): one tile of sim_tile.h.  Rows >= na and columns >= nb are masked in the epilogue.
// prow_*[x * prow_ld + 128 y + r]: best column of row r among this tile's columns; pcol_*[y * pcol_ld + 128 x + c]: best row of column c.
__global__ __launch_bounds__(256) void match_kernel(const _Float16* __restrict__ A, const _Float16* __restrict__ B, int hpad, int na, int nb,
                                                    int row0, int col0, float* __restrict__ prow_v, int* __restrict__ prow_i, size_t prow_ld,
                                                    float* __restrict__ pcol_v, int* __restrict__ pcol_i, size_t pcol_ld) {
    constexpr int BM = MATCH_TM, BN = MATCH_TN;
    __shared__ __attribute__((aligned(16))) char sA[BM * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) char sB[BN * SIM_ROWB];
    __shared__ float red_rv[2][BM], red_cv[2][BN];
    __shared__ int red_ri[2][BM], red_ci[2][BN];

    const SimPlace p;
    const int m0 = row0 + blockIdx.y * BM, n0 = col0 + blockIdx.x * BN;
    SimRows opa(p, A, m0, hpad), opb(p, B, n0, hpad);
    f32x4 acc[4][4];
    sim_tile(p, sA, sB, hpad / 64, opa, opb, acc);

    // acc[i][j][r] = sim(row, col), row = m0 + 64 wm + 16 i + fr, col = n0 + 64 wn + 16 j + 4 fh + r.  (+ 0.0f: a -0 becomes +0)
    const int rowb = m0 + p.wm * 64 + p.fr, colb = n0 + p.wn * 64 + 4 * p.fh;
    // per row over this wave's 64 columns: a lane's 16 in ascending order, then the four lanes that share the row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        Best b{-INFINITY, INT_MAX};
        sim_row_fold(acc, i, colb, nb, b);
        sim_row_share(p, i, b, red_rv, red_ri);
    }
    // per column over this wave's 64 rows: a lane's 4 in ascending order, then the sixteen lanes that share the column
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Best b{-INFINITY, INT_MAX};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rowb + i * 16;
                if (row < na) fold(b, acc[i][j][r] + 0.0f, row);
            }
            fold_lane<1>(b);
            fold_lane<2>(b);
            fold_lane<4>(b);
            fold_lane<8>(b);
            if (p.fr == 0) {
                red_cv[p.wm][p.wn * 64 + j * 16 + 4 * p.fh + r] = b.v;
                red_ci[p.wm][p.wn * 64 + j * 16 + 4 * p.fh + r] = b.i;
            }
        }
    __syncthreads();
    if (p.tid < BM) {  // the two waves side by side
        const Best b = sim_fold_waves(red_rv, red_ri, p.tid);
        const size_t o = (size_t)blockIdx.x * prow_ld + (size_t)blockIdx.y * BM + p.tid;
        prow_v[o] = b.v;
        prow_i[o] = b.i;
    } else {  // the two waves above each other
        const int c = p.tid - BM;
        const Best b = sim_fold_waves(red_cv, red_ci, c);
        const size_t o = (size_t)blockIdx.y * pcol_ld + (size_t)blockIdx.x * BN + c;
        pcol_v[o] = b.v;
        pcol_i[o] = b.i;
    }
}

// element e < n of one side: fold the partials pv / pi [ntiles][ld] in ascending tile order into (sim[e], idx[e]); `first` = 0 continues
// from what an earlier pass left there
__global__ __launch_bounds__(256) void match_reduce_kernel(const float* __restrict__ pv, const int* __restrict__ pi, size_t ld, int ntiles, int n,
                                                           int* __restrict__ idx, float* __restrict__ sim, int first) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    Best b{-INFINITY, INT_MAX};
    if (!first) b = Best{sim[e], idx[e]};
    for (int t = 0; t < ntiles; ++t) fold(b, pv[(size_t)t * ld + e], pi[(size_t)t * ld + e]);
    sim[e] = b.v;
    idx[e] = b.i;
}

hipError_t launch_match_normalise(const float* x, size_t ld, _Float16* out, int n, int nout, int H, int hpad, hipStream_t st) {
    const int vec = H % 4 == 0 && ld % 4 == 0 && ((size_t)x & 15) == 0;
    hipLaunchKernelGGL(match_normalise_kernel, dim3((nout + 3) / 4), dim3(256), 0, st, x, ld, out, n, nout, H, hpad, vec);
    return hipGetLastError();
}

hipError_t launch_match(const float* a, size_t lda, const float* b, size_t ldb, int na, int nb, int H, char* ws, const MatchPlan& p,
                        hipStream_t st) {
    _Float16* const a16 = (_Float16*)(ws + p.a16);
    _Float16* const b16 = (_Float16*)(ws + p.b16);
    hipError_t e = launch_match_normalise(a, lda, a16, na, p.na_pad, H, p.hpad, st);
    if (e != hipSuccess) return e;
    e = launch_match_normalise(b, ldb, b16, nb, p.nb_pad, H, p.hpad, st);
    if (e != hipSuccess) return e;
    float *prow_v = (float*)(ws + p.prow_v), *pcol_v = (float*)(ws + p.pcol_v), *sim_ab = (float*)(ws + p.sim_ab), *sim_ba = (float*)(ws + p.sim_ba);
    int *prow_i = (int*)(ws + p.prow_i), *pcol_i = (int*)(ws + p.pcol_i), *idx_ab = (int*)(ws + p.idx_ab), *idx_ba = (int*)(ws + p.idx_ba);
    constexpr int PR = MATCH_PASS * MATCH_TM, PC = MATCH_PASS * MATCH_TN;
    for (int r0 = 0; r0 < p.na_pad; r0 += PR) {
        const int rows = p.na_pad - r0 < PR ? p.na_pad - r0 : PR;  // of this pass, padded / real
        const int rreal = na - r0 < rows ? na - r0 : rows;
        for (int c0 = 0; c0 < p.nb_pad; c0 += PC) {
            const int cols = p.nb_pad - c0 < PC ? p.nb_pad - c0 : PC;
            const int creal = nb - c0 < cols ? nb - c0 : cols;
            const int ntm = rows / MATCH_TM, ntn = cols / MATCH_TN;
            hipLaunchKernelGGL(match_kernel, dim3(ntn, ntm), dim3(256), 0, st, a16, b16, p.hpad, na, nb, r0, c0, prow_v, prow_i, (size_t)rows,
                               pcol_v, pcol_i, (size_t)cols);
            hipLaunchKernelGGL(match_reduce_kernel, dim3((rreal + 255) / 256), dim3(256), 0, st, prow_v, prow_i, (size_t)rows, ntn, rreal,
                               idx_ab + r0, sim_ab + r0, c0 == 0);
            hipLaunchKernelGGL(match_reduce_kernel, dim3((creal + 255) / 256), dim3(256), 0, st, pcol_v, pcol_i, (size_t)cols, ntm, creal,
                               idx_ba + c0, sim_ba + c0, r0 == 0);
        }
    }
    return hipGetLastError();
}

}  // namespace dinov2
