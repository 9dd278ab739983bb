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
// Both directions come from the same accumulators.  "Best" is one total order everywhere -- the larger f32 value, among equal values (-0 == +0)
// the lower index -- so the result does not depend on which lane, wave, tile or pass met a pair first.  The K order of a pair depends on
// hpad alone: k steps of 32 in ascending order, whatever tile the pair falls in.
#include <climits>

#include "device_types.h"
#include "kernels.h"

namespace dinov2 {

namespace {

struct Best {
    float v;
    int i;
};
// the order of the whole file: larger value first, then lower index (an empty slot is (-inf, INT_MAX))
__device__ __forceinline__ bool better(float v, int i, const Best& b) { return v > b.v || (v == b.v && i < b.i); }
__device__ __forceinline__ void fold(Best& b, float v, int i) {
    if (better(v, i, b)) {
        b.v = v;
        b.i = i;
    }
}
template <int OFF>
__device__ __forceinline__ void fold_lane(Best& b) {
    const float v = __shfl_xor(b.v, OFF);
    const int i = __shfl_xor(b.i, OFF);
    fold(b, v, i);
}

}  // namespace

// x: rows [n] of H floats, row stride ld.  out [nout, hpad] f16: row / sqrt(sum of squares), 0 for an all-zero row, for rows >= n and for
// columns >= H; rows >= nout are not touched (the grid covers nout rounded up to 4).  Four rows per workgroup, one wave each; lane l owns the 4-float chunks l, l + 64, ... (16-byte loads when `vec`: H, ld
// multiples of 4 and an aligned base; the summation order is the same either way, so it depends on H alone).
__global__ __launch_bounds__(256) void match_normalise_kernel(const float* __restrict__ x, size_t ld, _Float16* __restrict__ out, int n,
                                                              int nout, int H, int hpad, int vec) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)nout) return;
    f16x4* const o = (f16x4*)(out + row * hpad);
    const int nch = hpad / 4;
    if (row >= (size_t)n) {
        for (int c = lane; c < nch; c += 64) o[c] = f16x4{0, 0, 0, 0};
        return;
    }
    const float* const src = x + row * ld;
    auto chunk = [&](int c) {
        float4 v;
        if (vec && 4 * c + 4 <= H) {
            v = *(const float4*)(src + 4 * c);
        } else {
            v.x = 4 * c + 0 < H ? src[4 * c + 0] : 0.0f;
            v.y = 4 * c + 1 < H ? src[4 * c + 1] : 0.0f;
            v.z = 4 * c + 2 < H ? src[4 * c + 2] : 0.0f;
            v.w = 4 * c + 3 < H ? src[4 * c + 3] : 0.0f;
        }
        return v;
    };
    float ss = 0.0f;
    for (int c = lane; c < nch; c += 64) {
        const float4 v = chunk(c);
        ss += v.x * v.x;
        ss += v.y * v.y;
        ss += v.z * v.z;
        ss += v.w * v.w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
    // correctly rounded square root and division (the compiler's default for f32; no v_rsq_f32): once per row
    const float r = ss > 0.0f ? 1.0f / sqrtf(ss) : 0.0f;
    for (int c = lane; c < nch; c += 64) {
        const float4 v = chunk(c);
        o[c] = f16x4{(_Float16)(v.x * r), (_Float16)(v.y * r), (_Float16)(v.z * r), (_Float16)(v.w * r)};
    }
}

// A [na_pad, hpad], B [nb_pad, hpad]: the normalised operands.  Workgroup (x, y) owns rows [row0 + 128 y, +128) and columns
// [col0 + 128 x, +128); four waves, 2 x 2, each 64 x 64 = 4 x 4 accumulator blocks of 16 x 16.  Operands are padded to whole tiles, so loads
// need no guards; rows >= na and columns >= nb are masked in the epilogue.  LDS image as in gemm.hip: [row][64 k] f16, 128-byte rows, 16-byte
// chunk c of row r at chunk c ^ ((r >> 1) & 7), which spreads every 16-lane ds_read_b128 group over 16 bank slots.
// prow_*[x * prow_ld + 128 y + r]: best column of row r among this tile's columns; pcol_*[y * pcol_ld + 128 x + c]: best row of column c.
__global__ __launch_bounds__(256) void match_kernel(const _Float16* __restrict__ A, const _Float16* __restrict__ B, int hpad, int na, int nb,
                                                    int row0, int col0, float* __restrict__ prow_v, int* __restrict__ prow_i, size_t prow_ld,
                                                    float* __restrict__ pcol_v, int* __restrict__ pcol_i, size_t pcol_ld) {
    using E = Elem<_Float16>;
    constexpr int BM = MATCH_TM, BN = MATCH_TN, ROWB = 128;
    __shared__ __attribute__((aligned(16))) char sA[BM * ROWB];
    __shared__ __attribute__((aligned(16))) char sB[BN * ROWB];
    __shared__ float red_rv[2][BM], red_cv[2][BN];
    __shared__ int red_ri[2][BM], red_ci[2][BN];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = row0 + blockIdx.y * BM, n0 = col0 + blockIdx.x * BN;

    // staging: 128 rows x 8 chunks of 16 bytes per operand = 4 chunks per thread; 8 neighbouring threads read one 128-byte row segment
    const char* asrc[4];
    const char* bsrc[4];
    int sdst[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = j * 256 + tid, row = q >> 3, c = q & 7;
        asrc[j] = (const char*)A + ((size_t)(m0 + row) * hpad) * 2 + c * 16;
        bsrc[j] = (const char*)B + ((size_t)(n0 + row) * hpad) * 2 + c * 16;
        sdst[j] = row * ROWB + ((c ^ ((row >> 1) & 7)) << 4);
    }
    u32x4 ar[4], br[4];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ar[j] = *(const u32x4*)(asrc[j] + (size_t)kt * ROWB);
            br[j] = *(const u32x4*)(bsrc[j] + (size_t)kt * ROWB);
        }
    };

    const int fr = lane & 15, fh = lane >> 4, sw = (fr >> 1) & 7;
    const int aoff = (wm * 64 + fr) * ROWB, boff = (wn * 64 + fr) * ROWB;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = hpad / 64;
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *(u32x4*)(sA + sdst[j]) = ar[j];
            *(u32x4*)(sB + sdst[j]) = br[j];
        }
        __syncthreads();
        if (kt + 1 < nk) fetch(kt + 1);  // in flight under the MFMAs below
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {  // k steps of 32 in ascending order
            const int ch = ((ks * 4 + fh) ^ sw) << 4;
            f16x8 af[4], bf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *(const f16x8*)(sA + aoff + i * 16 * ROWB + ch);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *(const f16x8*)(sB + boff + j * 16 * ROWB + ch);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = E::mfma16(bf[j], af[i], acc[i][j]);  // operand swap: a lane owns one row, four columns
        }
    }

    // acc[i][j][r] = sim(row, col), row = m0 + 64 wm + 16 i + fr, col = n0 + 64 wn + 16 j + 4 fh + r.  (+ 0.0f: a -0 becomes +0)
    const int rowb = m0 + wm * 64 + fr, colb = n0 + wn * 64 + 4 * fh;
    // per row over this wave's 64 columns: a lane's 16 in ascending order, then the four lanes that share the row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        Best b{-INFINITY, INT_MAX};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = colb + j * 16 + r;
                if (col < nb) fold(b, acc[i][j][r] + 0.0f, col);
            }
        fold_lane<16>(b);
        fold_lane<32>(b);
        if (fh == 0) {
            red_rv[wn][wm * 64 + i * 16 + fr] = b.v;
            red_ri[wn][wm * 64 + i * 16 + fr] = b.i;
        }
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
            if (fr == 0) {
                red_cv[wm][wn * 64 + j * 16 + 4 * fh + r] = b.v;
                red_ci[wm][wn * 64 + j * 16 + 4 * fh + r] = b.i;
            }
        }
    __syncthreads();
    if (tid < BM) {  // the two waves side by side
        Best b{red_rv[0][tid], red_ri[0][tid]};
        fold(b, red_rv[1][tid], red_ri[1][tid]);
        const size_t o = (size_t)blockIdx.x * prow_ld + (size_t)blockIdx.y * BM + tid;
        prow_v[o] = b.v;
        prow_i[o] = b.i;
    } else {  // the two waves above each other
        const int c = tid - BM;
        Best b{red_cv[0][c], red_ci[0][c]};
        fold(b, red_cv[1][c], red_ci[1][c]);
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
