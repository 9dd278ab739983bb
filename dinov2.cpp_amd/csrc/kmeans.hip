// kmeans.hip -- spherical k-means of token rows (dinov2_hip_kmeans_tokens, include/dinov2_hip.h) for gfx950 (MI355X).
//
// No reference counterpart: k-means over the patch tokens of one image or of a batch (unsupervised part segments, co-segmentation), a fixed
// vocabulary of centres applied to new frames (visual words).  Rows and centre vectors are normalised by match.hip's kernel
// (launch_match_normalise); the kernels here:
//   kmeans_assign_kernel     one workgroup per 128-row tile of X^ walks the centre tiles, each a tile of sim_tile.h, keeps the best (value,
//                            lowest centre) per row across the tiles and writes label, sim and the workgroup's count of rows whose label
//                            changed
//   kmeans_fold_kernel       the changed-count partials -> one int
//   kmeans_transpose_kernel  X^ [npad, hpad] -> X^T [hpad128, npad], once per call (padding rows of H written as zeros)
//   kmeans_update_kernel     D[h, c] = sum_i X^T[h, i] * (label[i] == c) on the matrix cores over one chunk of rows, as a tile of sim_tile.h
//                            whose one-hot operand is built straight into the LDS image from 64 labels per K-tile; f32 partials
//                            [chunk][c][h], exact counts
//   kmeans_finish_kernel     folds the partials in ascending chunk order over the centre vectors of the clusters that have members
//   kmeans_count_kernel      members per cluster of the labels as they stand (the exits on which no update follows the last assignment)
//   kmeans_gather_kernel     centre j = row init[j] of the source, verbatim
// The similarity of a pair and the total order of "best" are sim_tile.h's, so the label does not depend on which lane, wave or centre tile
// met a centre first.  No atomics anywhere: every sum has one fixed order.
#include "onehot_rows.h"
#include "sim_tile.h"

namespace dinov2 {

// X [npad, hpad], Cn [kpad, hpad]: the normalised operands, padded to whole tiles (padding rows zero).  Workgroup x owns rows [128 x, +128)
// and walks the centre tiles.  label [npad] is read (the previous labels) and written in place: rows >= n get -1.  sim [n].  chpart[x] =
// rows of this tile whose label changed (`first`: every real row counts).
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const _Float16* __restrict__ X, const _Float16* __restrict__ Cn, int hpad, int n, int K,
                                                            int kpad, int* __restrict__ label, float* __restrict__ sim, int* __restrict__ chpart,
                                                            int first) {
    __shared__ __attribute__((aligned(16))) char sA[SIM_TILE * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) char sB[SIM_TILE * SIM_ROWB];
    __shared__ float red_rv[2][SIM_TILE];
    __shared__ int red_ri[2][SIM_TILE];
    __shared__ int red_ch[2];

    const SimPlace p;
    const int m0 = blockIdx.x * SIM_TILE;
    const Best b = sim_best_of_rows(p, sA, sB, red_rv, red_ri, X, m0, Cn, K, kpad, hpad);
    if (p.tid < SIM_TILE) {  // waves 0 and 1, whole
        const int row = m0 + p.tid;
        int changed = 0;
        if (row < n) {
            changed = first || label[row] != b.i;
            label[row] = b.i;
            sim[row] = b.v;
        } else {
            label[row] = -1;
        }
        const unsigned long long m = __ballot(changed);
        if (p.lane == 0) red_ch[p.wid] = __popcll(m);
    }
    __syncthreads();
    if (p.tid == 0) chpart[blockIdx.x] = red_ch[0] + red_ch[1];
}

// out[0] = sum of part[0 .. count), in ascending order (integers: any order gives the same)
__global__ __launch_bounds__(64) void kmeans_fold_kernel(const int* __restrict__ part, int count, int* __restrict__ out) {
    int s = 0;
    for (int i = threadIdx.x; i < count; i += 64) s += part[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) out[0] = s;
}

// X [npad, hpad] -> XT [hpad128, npad]; rows h >= hpad of XT are written as zeros.  Workgroup (x, y): rows [64 x, +64) of X, columns [64 y, +64).
__global__ __launch_bounds__(256) void kmeans_transpose_kernel(const _Float16* __restrict__ X, _Float16* __restrict__ XT, int npad, int hpad) {
    __shared__ _Float16 t[64][66];
    const int i0 = blockIdx.x * 64, h0 = blockIdx.y * 64;
    const int c = threadIdx.x & 63, r4 = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = k * 4 + r4;
        t[r][c] = h0 + c < hpad ? X[(size_t)(i0 + r) * hpad + h0 + c] : (_Float16)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = k * 4 + r4;
        XT[(size_t)(h0 + r) * npad + i0 + c] = t[c][r];
    }
}

// XT [hpad128, npad], label [npad] (-1 on padding rows).  Workgroup (x, y, z): rows h [128 x, +128) of XT, centres [128 y, +128), the rows i
// of chunk z = [z chunk, min((z + 1) chunk, npad)) in K-tiles of 64, ascending.  part [nsplit][kpad][hpad128]: every element of the
// workgroup's tile is stored.  cpart [nsplit][kpad]: members of each centre in the chunk (workgroups x == 0).
__global__ __launch_bounds__(256) void kmeans_update_kernel(const _Float16* __restrict__ XT, const int* __restrict__ label, int npad, int chunk,
                                                            int kpad, int hpad128, float* __restrict__ part, int* __restrict__ cpart) {
    __shared__ __attribute__((aligned(16))) char sA[SIM_TILE * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) char sB[SIM_TILE * SIM_ROWB];

    const SimPlace p;
    const int m0 = blockIdx.x * SIM_TILE, n0 = blockIdx.y * SIM_TILE;
    const int i0 = blockIdx.z * chunk;
    const int i1 = i0 + chunk < npad ? i0 + chunk : npad;

    SimRows opa(p, XT, m0, npad, i0);
    OneHotRows opb{label + i0 + (p.tid & 7) * 8, n0 + (p.tid >> 3), {}, {}, {0, 0, 0, 0}};
    f32x4 acc[4][4];
    sim_tile(p, sA, sB, (i1 - i0) / 64, opa, opb, acc);

    // acc[i][j][r] = D(h, c), h = m0 + 64 wm + 16 i + fr, c = n0 + 64 wn + 16 j + 4 fh + r
    float* const dst = part + ((size_t)blockIdx.z * kpad) * hpad128;
    const int hb = m0 + p.wm * 64 + p.fr, cb = n0 + p.wn * 64 + 4 * p.fh;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(size_t)(cb + j * 16 + r) * hpad128 + hb + i * 16] = acc[i][j][r];
    if (blockIdx.x == 0) {  // the eight threads that share a row of the one-hot image
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int s = opb.cnt[j];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            if ((p.tid & 7) == 0) cpart[(size_t)blockIdx.z * kpad + opb.crow + 32 * j] = s;
        }
    }
}

// centre c < K (blockIdx.y), column h < H: counts[c] = sum over the chunks of cpart; where it is > 0, cvec[c, h] = the partials folded in
// ascending chunk order; an empty cluster keeps its vector.
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const float* __restrict__ part, const int* __restrict__ cpart, int nsplit, int kpad,
                                                            int hpad128, int H, float* __restrict__ cvec, int* __restrict__ counts) {
    const int c = blockIdx.y, h = blockIdx.x * 256 + threadIdx.x;
    int cnt = 0;
    for (int s = 0; s < nsplit; ++s) cnt += cpart[(size_t)s * kpad + c];
    if (h == 0) counts[c] = cnt;
    if (h >= H || cnt == 0) return;
    float v = part[(size_t)c * hpad128 + h];
    for (int s = 1; s < nsplit; ++s) v += part[((size_t)s * kpad + c) * hpad128 + h];
    cvec[(size_t)c * H + h] = v;
}

// counts[c] = rows whose label is c (workgroup c; padding rows hold -1)
__global__ __launch_bounds__(256) void kmeans_count_kernel(const int* __restrict__ label, int npad, int* __restrict__ counts) {
    __shared__ int red[4];
    const int c = blockIdx.x;
    int s = 0;
    for (int i = threadIdx.x; i < npad; i += 256) s += label[i] == c;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) counts[c] = red[0] + red[1] + red[2] + red[3];
}

// cvec[j, :] = row idx[j] of the source: row r lives at src + (r / per) * outer + (r % per) * ld
__global__ __launch_bounds__(256) void kmeans_gather_kernel(const float* __restrict__ src, int per, size_t outer, size_t ld, const int* __restrict__ idx,
                                                            int H, float* __restrict__ cvec) {
    const int r = idx[blockIdx.x];
    const float* const row = src + (size_t)(r / per) * outer + (size_t)(r % per) * ld;
    for (int h = threadIdx.x; h < H; h += 256) cvec[(size_t)blockIdx.x * H + h] = row[h];
}

KmeansBufs kmeans_bufs(char* ws, const KmeansPlan& p) {
    KmeansBufs b;
    b.x16 = (_Float16*)(ws + p.x16);
    b.xt = (_Float16*)(ws + p.xt);
    b.c16 = (_Float16*)(ws + p.c16);
    b.cvec = (float*)(ws + p.cvec);
    b.labels = (int*)(ws + p.labels);
    b.sim = (float*)(ws + p.sim);
    b.part = (float*)(ws + p.part);
    b.cpart = (int*)(ws + p.cpart);
    b.counts = (int*)(ws + p.counts);
    b.chpart = (int*)(ws + p.chpart);
    b.changed = (int*)(ws + p.changed);
    return b;
}

hipError_t launch_kmeans_assign(const KmeansBufs& b, int n, int K, const KmeansPlan& p, bool first, hipStream_t st) {
    const int tiles = p.npad / SIM_TILE;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(tiles), dim3(256), 0, st, b.x16, b.c16, p.hpad, n, K, p.kpad, b.labels, b.sim, b.chpart,
                       first ? 1 : 0);
    hipLaunchKernelGGL(kmeans_fold_kernel, dim3(1), dim3(64), 0, st, b.chpart, tiles, b.changed);
    return hipGetLastError();
}

hipError_t launch_kmeans_transpose(const KmeansBufs& b, const KmeansPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(kmeans_transpose_kernel, dim3(p.npad / 64, p.hpad128 / 64), dim3(256), 0, st, b.x16, b.xt, p.npad, p.hpad);
    return hipGetLastError();
}

hipError_t launch_kmeans_update(const KmeansBufs& b, int K, int H, const KmeansPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(p.hpad128 / SIM_TILE, p.kpad / SIM_TILE, p.nsplit), dim3(256), 0, st, b.xt, b.labels, p.npad, p.chunk,
                       p.kpad, p.hpad128, b.part, b.cpart);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((H + 255) / 256, K), dim3(256), 0, st, b.part, b.cpart, p.nsplit, p.kpad, p.hpad128, H, b.cvec,
                       b.counts);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_match_normalise(b.cvec, (size_t)H, b.c16, K, p.kpad, H, p.hpad, st);
}

hipError_t launch_kmeans_count(const KmeansBufs& b, int K, const KmeansPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(kmeans_count_kernel, dim3(K), dim3(256), 0, st, b.labels, p.npad, b.counts);
    return hipGetLastError();
}

hipError_t launch_kmeans_gather(const float* src, int per, size_t outer, size_t ld, const int* idx, int K, int H, float* cvec, hipStream_t st) {
    hipLaunchKernelGGL(kmeans_gather_kernel, dim3(K), dim3(256), 0, st, src, per, outer, ld, idx, H, cvec);
    return hipGetLastError();
}

// Contract 5 of dinov2_hip_kmeans.  b.x16 holds the normalised rows and b.cvec the init vectors; afterwards labels, sim, cvec and counts are
// the results.  One 4-byte read of `changed` per assignment.
hipError_t kmeans_run(const KmeansBufs& b, int n, int K, int H, int max_iter, const KmeansPlan& p, hipStream_t st, int* iterations,
                      int* converged) {
    hipError_t e = launch_match_normalise(b.cvec, (size_t)H, b.c16, K, p.kpad, H, p.hpad, st);
    if (e == hipSuccess && max_iter > 0) e = launch_kmeans_transpose(b, p, st);
    int it = 0, conv = 0;
    while (e == hipSuccess) {
        e = launch_kmeans_assign(b, n, K, p, it == 0, st);
        int changed = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&changed, b.changed, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        if (changed == 0) {  // (never after the first assignment: there every row counts)
            conv = 1;
            break;
        }
        if (it == max_iter) {  // the counts the last update left belong to the labels before this assignment
            e = launch_kmeans_count(b, K, p, st);
            break;
        }
        e = launch_kmeans_update(b, K, H, p, st);
        ++it;
    }
    *iterations = it;
    *converged = conv;
    return e;
}

}  // namespace dinov2
