// ncut.hip -- the device half of dinov2_hip_ncut_tokens (include/dinov2_hip.h): the leading eigenvectors of the normalised patch-affinity
// graph of token rows for gfx950 (MI355X).  The driver and the host's Rayleigh-Ritz step are csrc/ncut.cpp.
//
// No reference counterpart: TokenCut's second eigenvector, the first few of Deep Spectral Methods.  Rows are normalised by match.hip's kernel
// (launch_match_normalise); the kernels here:
//   ncut_apply_kernel    workgroup (x, y): row tile x against the column tiles of chunk y, each a tile of sim_tile.h; the affinity map on the
//                        f32 accumulators, then t_i += sum_j w_ij (scale_j q_j) for the NCUT_NB columns of the block in f64 -- W never exists
//                        in memory.  Partials [chunk][npad][NCUT_NB].  The degree pass is the same kernel with scale = 1 and a ones column.
//   ncut_degree_kernel   folds column 0 of the chunk partials in ascending order: d_i, c_i = d_i > 0 ? 1 / sqrt(d_i) : 0
//   ncut_finish_kernel   folds the chunk partials in ascending order, y_i = (1/2 (y_prev_i + c_i t_i)) R^-1 (CholeskyQR: pca_chol_rinv of the
//                        Gram matrix rebuilt from the previous step's per-workgroup partials), and leaves the partials of Y_next^T Y_next
//                        and Q^T Y_next
// The similarity of a pair is sim_tile.h's.  No atomics anywhere: every sum has one fixed order.
#include "sim_tile.h"

namespace dinov2 {

// contract 3 of dinov2_hip_ncut: f32 on the f32 similarity, -0 read as +0
template <int AFF>
__device__ __forceinline__ float ncut_weight(float s, float tau, float floor) {
    s += 0.0f;
    if (AFF == NCUT_THRESHOLD) return s > tau ? 1.0f : floor;
    if (AFF == NCUT_RELU) return s > 0.0f ? s : 0.0f;
    return expf((s - 1.0f) / tau);
}

// X [npad, hpad]: the normalised rows, padded to whole tiles.  Workgroup (x, y): rows [128 x, +128), column tiles [y chunk_tiles,
// min((y + 1) chunk_tiles, ntiles)).  scale [npad] (nullptr: ones), q [npad][NCUT_NB] (nullptr: a ones column 0, zeros beside it).
// part [gridDim.y][npad][NCUT_NB].  The order of a row's sum: every lane adds the columns it owns in ascending order across the chunk's
// tiles (16 per tile: 64 wn + 16 j + 4 fh + r, j then r ascending), then the four lanes that share the row fold as (fh 0 + 1) + (2 + 3), then
// the two waves side by side as wn 0 + wn 1.
template <int AFF>
__global__ __launch_bounds__(256) void ncut_apply_kernel(const _Float16* __restrict__ X, int hpad, int n, int ntiles, int chunk_tiles, float tau,
                                                         float floor, const double* __restrict__ scale, const double* __restrict__ q,
                                                         double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) char sA[SIM_TILE * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) char sB[SIM_TILE * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) double sv[SIM_TILE][NCUT_NB];      // scale_j q_j of the tile's columns; zeros for columns >= n
    __shared__ __attribute__((aligned(16))) double red[2][SIM_TILE][NCUT_NB];  // the row sums of the two waves side by side

    const SimPlace p;
    const int m0 = blockIdx.x * SIM_TILE;
    const int t0 = blockIdx.y * chunk_tiles, t1 = t0 + chunk_tiles < ntiles ? t0 + chunk_tiles : ntiles;
    const int npad = ntiles * SIM_TILE;

    SimRows opa(p, X, m0, hpad);
    double sum[4][NCUT_NB];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < NCUT_NB; ++c) sum[i][c] = 0.0;

    for (int t = t0; t < t1; ++t) {
        const int n0 = t * SIM_TILE;
        __syncthreads();  // every wave is done reading the previous tile's sv
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = k * 256 + p.tid, col = e >> 3, c = e & 7;
            const int g = n0 + col;
            double v = 0.0;
            if (g < n) {
                v = q ? q[(size_t)g * NCUT_NB + c] : (c == 0 ? 1.0 : 0.0);
                if (scale) v *= scale[g];
            }
            sv[col][c] = v;
        }
        SimRows opb(p, X, n0, hpad);
        f32x4 acc[4][4];
        sim_tile(p, sA, sB, hpad / 64, opa, opb, acc);  // (its barriers publish sv)
        // acc[i][j][r] = sim(row, column), row = m0 + 64 wm + 16 i + fr, column = n0 + 64 wn + 16 j + 4 fh + r; columns >= n weigh 0
        const int colb = p.wn * 64 + 4 * p.fh;
        // the affinities in place first: the f64 products below then keep 64 sums and one column's eight values live, nothing of the map
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = ncut_weight<AFF>(acc[i][j][r], tau, floor);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = colb + j * 16 + r;
                const bool real = n0 + col < n;
                double v[NCUT_NB];
#pragma unroll
                for (int c = 0; c < NCUT_NB; c += 2) {
                    const double2 d = *(const double2*)&sv[col][c];
                    v[c] = d.x;
                    v[c + 1] = d.y;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double w = real ? (double)acc[i][j][r] : 0.0;
#pragma unroll
                    for (int c = 0; c < NCUT_NB; ++c) sum[i][c] = fma(w, v[c], sum[i][c]);
                }
            }
    }
    // the four lanes that share a row, then the two waves side by side
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < NCUT_NB; ++c) {
            double s = sum[i][c];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (p.fh == 0) red[p.wn][p.wm * 64 + i * 16 + p.fr][c] = s;
        }
    __syncthreads();
    double* const dst = part + ((size_t)blockIdx.y * npad + m0) * NCUT_NB;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = k * 256 + p.tid;
        dst[e] = red[0][e >> 3][e & 7] + red[1][e >> 3][e & 7];
    }
}

// row i < npad: deg = column 0 of the chunk partials in ascending chunk order; rows >= n: 0
__global__ __launch_bounds__(256) void ncut_degree_kernel(const double* __restrict__ part, int nchunks, int npad, int n, double* __restrict__ deg,
                                                          double* __restrict__ cs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double d = 0.0;
    if (i < n) {
        d = part[(size_t)i * NCUT_NB];
        for (int s = 1; s < nchunks; ++s) d += part[((size_t)s * npad + i) * NCUT_NB];
    }
    deg[i] = d;
    cs[i] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
}

// Workgroup x owns rows [128 x, +128); thread r < 128 owns a row.  gprev / gnext / ritz: [gridDim.x][64] per-workgroup partials; a partial is
// the sum over the workgroup's rows in ascending order, the Gram matrix the sum of the partials in ascending order.
__global__ __launch_bounds__(256) void ncut_finish_kernel(const double* __restrict__ part, int nchunks, int npad, int n,
                                                          const double* __restrict__ cs, const double* __restrict__ yprev,
                                                          const double* __restrict__ gprev, double* __restrict__ ynext,
                                                          double* __restrict__ gnext, double* __restrict__ ritz) {
    __shared__ double gs[64], rinv[64];
    __shared__ double ys[SIM_TILE][NCUT_NB + 1], qs[SIM_TILE][NCUT_NB + 1];
    const int t = threadIdx.x;
    if (t < 64) {
        double s = 0.0;
        for (int blk = 0; blk < (int)gridDim.x; ++blk) s += gprev[(size_t)blk * 64 + t];
        gs[t] = s;
    }
    __syncthreads();
    if (t == 0) pca_chol_rinv(gs, rinv);
    __syncthreads();
    if (t < SIM_TILE) {
        const int row = blockIdx.x * SIM_TILE + t;
        double z[NCUT_NB], yp[NCUT_NB];
        if (row < n) {
            const double c = cs[row];
#pragma unroll
            for (int a = 0; a < NCUT_NB; ++a) {
                double s = part[(size_t)row * NCUT_NB + a];
                for (int k = 1; k < nchunks; ++k) s += part[((size_t)k * npad + row) * NCUT_NB + a];
                yp[a] = yprev[(size_t)row * NCUT_NB + a];
                z[a] = 0.5 * (yp[a] + c * s);
            }
        } else {
#pragma unroll
            for (int a = 0; a < NCUT_NB; ++a) z[a] = yp[a] = 0.0;
        }
#pragma unroll
        for (int b = 0; b < NCUT_NB; ++b) {  // (v R^-1)[b] = sum_{a <= b} v[a] rinv[a][b]
            double y = 0.0, qv = 0.0;
#pragma unroll
            for (int a = 0; a <= b; ++a) {
                y = fma(z[a], rinv[a * NCUT_NB + b], y);
                qv = fma(yp[a], rinv[a * NCUT_NB + b], qv);
            }
            ynext[(size_t)row * NCUT_NB + b] = y;
            ys[t][b] = y;
            qs[t][b] = qv;
        }
    }
    __syncthreads();
    if (t < 128) {
        const int e = t & 63, a = e >> 3, b = e & 7;
        const double(*left)[NCUT_NB + 1] = t < 64 ? ys : qs;
        double s = 0.0;
        for (int r = 0; r < SIM_TILE; ++r) s = fma(left[r][a], ys[r][b], s);
        (t < 64 ? gnext : ritz)[(size_t)blockIdx.x * 64 + e] = s;
    }
}

NcutBufs ncut_bufs(char* ws, const NcutPlan& p) {
    NcutBufs b;
    b.x16 = (_Float16*)(ws + p.x16);
    for (int k = 0; k < 2; ++k) {
        b.y[k] = (double*)(ws + p.y[k]);
        b.gram[k] = (double*)(ws + p.gram[k]);
    }
    b.ritz = (double*)(ws + p.ritz);
    b.deg = (double*)(ws + p.deg);
    b.cs = (double*)(ws + p.cs);
    b.part = (double*)(ws + p.part);
    return b;
}

hipError_t launch_ncut_apply(const _Float16* x16, int n, int affinity, float tau, float floor, const double* scale, const double* q, double* part,
                             const NcutPlan& p, hipStream_t st) {
    const dim3 grid(p.ntiles, p.nchunks);
    if (n < 1 || n > p.npad) return hipErrorInvalidValue;
    switch (affinity) {
        case NCUT_THRESHOLD:
            hipLaunchKernelGGL(ncut_apply_kernel<NCUT_THRESHOLD>, grid, dim3(256), 0, st, x16, p.hpad, n, p.ntiles, p.chunk_tiles, tau, floor, scale, q,
                               part);
            break;
        case NCUT_RELU:
            hipLaunchKernelGGL(ncut_apply_kernel<NCUT_RELU>, grid, dim3(256), 0, st, x16, p.hpad, n, p.ntiles, p.chunk_tiles, tau, floor, scale, q, part);
            break;
        case NCUT_EXP:
            hipLaunchKernelGGL(ncut_apply_kernel<NCUT_EXP>, grid, dim3(256), 0, st, x16, p.hpad, n, p.ntiles, p.chunk_tiles, tau, floor, scale, q, part);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ncut_degree(const double* part, int n, double* deg, double* cs, const NcutPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(ncut_degree_kernel, dim3(p.npad / 256 + 1), dim3(256), 0, st, part, p.nchunks, p.npad, n, deg, cs);
    return hipGetLastError();
}

hipError_t launch_ncut_finish(const double* part, const double* cs, const double* yprev, const double* gprev, int n, double* ynext, double* gnext,
                              double* ritz, const NcutPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(ncut_finish_kernel, dim3(p.ntiles), dim3(256), 0, st, part, p.nchunks, p.npad, n, cs, yprev, gprev, ynext, gnext, ritz);
    return hipGetLastError();
}

}  // namespace dinov2
