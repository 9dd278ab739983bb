// kmeans.hip -- spherical k-means of token rows (dinov2_hip_kmeans_tokens, include/dinov2_hip.h) for gfx950 (MI355X).
//
// No reference counterpart: k-means over the patch tokens of one image or of a batch (unsupervised part segments, co-segmentation), a fixed
// vocabulary of centres applied to new frames (visual words).  Rows and centre vectors are normalised by match.hip's kernel
// (launch_match_normalise); the kernels here:
//   kmeans_assign_kernel     one workgroup per 128-row tile of X^ walks the centre tiles with match_kernel's staging, LDS image, K loop and
//                            operand swap, keeps the best (value, lowest centre) per row across the tiles and writes label, sim and the
//                            workgroup's count of rows whose label changed
//   kmeans_fold_kernel       the changed-count partials -> one int
//   kmeans_transpose_kernel  X^ [npad, hpad] -> X^T [hpad128, npad], once per call (padding rows of H written as zeros)
//   kmeans_update_kernel     D[h, c] = sum_i X^T[h, i] * (label[i] == c) on the matrix cores over one chunk of rows: the one-hot operand is
//                            built straight into the swizzled LDS image from 64 labels per K-tile; f32 partials [chunk][c][h], exact counts
//   kmeans_finish_kernel     folds the partials in ascending chunk order over the centre vectors of the clusters that have members
//   kmeans_count_kernel      members per cluster of the labels as they stand (the exits on which no update follows the last assignment)
//   kmeans_gather_kernel     centre j = row init[j] of the source, verbatim
// The similarity of a pair is match_kernel's, instruction for instruction in the K loop: k steps of 32 in ascending order, an order that
// depends on hpad alone.  "Best" is match.hip's total order -- the larger f32 value, among equal values (-0 == +0) the lower index -- so the
// label does not depend on which lane, wave or centre tile met a centre first.  No atomics anywhere: every sum has one fixed order.
#include <climits>

#include "device_types.h"
#include "kernels.h"

namespace dinov2 {

namespace {

struct Best {
    float v;
    int i;
};
// match.hip's order: larger value first, then lower index (an empty slot is (-inf, INT_MAX))
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

constexpr int TILE = 128, ROWB = 128;  // match_kernel's tile; bytes of one LDS row (64 k of f16)

}  // namespace

// X [npad, hpad], Cn [kpad, hpad]: the normalised operands, padded to whole tiles (padding rows zero).  Workgroup x owns rows [128 x, +128);
// four waves, 2 x 2, each 64 x 64 = 4 x 4 accumulator blocks of 16 x 16, as in match_kernel.  label [npad] is read (the previous labels) and
// written in place: rows >= n get -1.  sim [n].  chpart[x] = rows of this tile whose label changed (`first`: every real row counts).
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const _Float16* __restrict__ X, const _Float16* __restrict__ Cn, int hpad, int n, int K,
                                                            int kpad, int* __restrict__ label, float* __restrict__ sim, int* __restrict__ chpart,
                                                            int first) {
    using E = Elem<_Float16>;
    __shared__ __attribute__((aligned(16))) char sA[TILE * ROWB];
    __shared__ __attribute__((aligned(16))) char sB[TILE * ROWB];
    __shared__ float red_rv[2][TILE];
    __shared__ int red_ri[2][TILE];
    __shared__ int red_ch[2];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = blockIdx.x * TILE;

    // staging: 128 rows x 8 chunks of 16 bytes per operand = 4 chunks per thread; 8 neighbouring threads read one 128-byte row segment
    const char* asrc[4];
    size_t boff_g[4];
    int sdst[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = j * 256 + tid, row = q >> 3, c = q & 7;
        asrc[j] = (const char*)X + ((size_t)(m0 + row) * hpad) * 2 + c * 16;
        boff_g[j] = ((size_t)row * hpad) * 2 + c * 16;
        sdst[j] = row * ROWB + ((c ^ ((row >> 1) & 7)) << 4);
    }
    const int fr = lane & 15, fh = lane >> 4, sw = (fr >> 1) & 7;
    const int aoff = (wm * 64 + fr) * ROWB, boff = (wn * 64 + fr) * ROWB;
    const int nk = hpad / 64;

    Best best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) best[i] = Best{-INFINITY, INT_MAX};

    for (int n0 = 0; n0 < kpad; n0 += TILE) {  // the centre tiles in ascending order
        const char* const bbase = (const char*)Cn + ((size_t)n0 * hpad) * 2;
        u32x4 ar[4], br[4];
        auto fetch = [&](int kt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ar[j] = *(const u32x4*)(asrc[j] + (size_t)kt * ROWB);
                br[j] = *(const u32x4*)(bbase + boff_g[j] + (size_t)kt * ROWB);
            }
        };
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        // acc[i][j][r] = sim(row, centre), row = m0 + 64 wm + 16 i + fr, centre = n0 + 64 wn + 16 j + 4 fh + r.  (+ 0.0f: a -0 becomes +0)
        const int colb = n0 + wn * 64 + 4 * fh;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = colb + j * 16 + r;
                    if (col < K) fold(best[i], acc[i][j][r] + 0.0f, col);  // a lane's columns ascending; columns >= K masked
                }
    }
    // the four lanes that share a row, then the two waves side by side
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        Best b = best[i];
        fold_lane<16>(b);
        fold_lane<32>(b);
        if (fh == 0) {
            red_rv[wn][wm * 64 + i * 16 + fr] = b.v;
            red_ri[wn][wm * 64 + i * 16 + fr] = b.i;
        }
    }
    __syncthreads();
    if (tid < TILE) {  // waves 0 and 1, whole
        Best b{red_rv[0][tid], red_ri[0][tid]};
        fold(b, red_rv[1][tid], red_ri[1][tid]);
        const int row = m0 + tid;
        int changed = 0;
        if (row < n) {
            changed = first || label[row] != b.i;
            label[row] = b.i;
            sim[row] = b.v;
        } else {
            label[row] = -1;
        }
        const unsigned long long m = __ballot(changed);
        if (lane == 0) red_ch[wid] = __popcll(m);
    }
    __syncthreads();
    if (tid == 0) chpart[blockIdx.x] = red_ch[0] + red_ch[1];
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
// of chunk z = [z chunk, min((z + 1) chunk, npad)) in K-tiles of 64.  The A operand is staged as in match_kernel; the B operand [128 c][64 i] =
// (label[i] == 128 y + c) is written into the same swizzled image from the K-tile's 64 labels.  part [nsplit][kpad][hpad128]: every element
// of the workgroup's tile is stored.  cpart [nsplit][kpad]: members of each centre in the chunk (workgroups x == 0).
__global__ __launch_bounds__(256) void kmeans_update_kernel(const _Float16* __restrict__ XT, const int* __restrict__ label, int npad, int chunk,
                                                            int kpad, int hpad128, float* __restrict__ part, int* __restrict__ cpart) {
    using E = Elem<_Float16>;
    __shared__ __attribute__((aligned(16))) char sA[TILE * ROWB];
    __shared__ __attribute__((aligned(16))) char sB[TILE * ROWB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = blockIdx.x * TILE, n0 = blockIdx.y * TILE;
    const int i0 = blockIdx.z * chunk;
    const int i1 = i0 + chunk < npad ? i0 + chunk : npad;
    const int nk = (i1 - i0) / 64;

    const char* asrc[4];
    int sdst[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = j * 256 + tid, row = q >> 3, c = q & 7;
        asrc[j] = (const char*)XT + ((size_t)(m0 + row) * npad + i0) * 2 + c * 16;
        sdst[j] = row * ROWB + ((c ^ ((row >> 1) & 7)) << 4);
    }
    // the 8 labels of this thread's chunk of every K-tile (the chunk index q & 7 = tid & 7 is the same for its four rows)
    const int* const lsrc = label + i0 + (tid & 7) * 8;
    const int crow = n0 + (tid >> 3);  // the centre of its row j = 0; row j is 32 j further
    u32x4 ar[4];
    u32x4 l0, l1;  // (compared as unsigned: the -1 of a padding row equals no centre)
    auto fetch = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ar[j] = *(const u32x4*)(asrc[j] + (size_t)kt * ROWB);
        l0 = *(const u32x4*)(lsrc + kt * 64);
        l1 = *(const u32x4*)(lsrc + kt * 64 + 4);
    };

    const int fr = lane & 15, fh = lane >> 4, sw = (fr >> 1) & 7;
    const int aoff = (wm * 64 + fr) * ROWB, boff = (wn * 64 + fr) * ROWB;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int cnt[4] = {0, 0, 0, 0};

    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {  // rows ascending
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *(u32x4*)(sA + sdst[j]) = ar[j];
            const unsigned c = (unsigned)(crow + 32 * j);
            const unsigned lab[8] = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
            u32x4 oh;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned lo = lab[2 * e] == c, hi = lab[2 * e + 1] == c;
                oh[e] = lo * 0x3c00u | hi * 0x3c000000u;  // 1.0 in f16
                cnt[j] += (int)(lo + hi);
            }
            *(u32x4*)(sB + sdst[j]) = oh;
        }
        __syncthreads();
        if (kt + 1 < nk) fetch(kt + 1);
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
                for (int j = 0; j < 4; ++j) acc[i][j] = E::mfma16(bf[j], af[i], acc[i][j]);
        }
    }
    // acc[i][j][r] = D(h, c), h = m0 + 64 wm + 16 i + fr, c = n0 + 64 wn + 16 j + 4 fh + r
    float* const dst = part + ((size_t)blockIdx.z * kpad) * hpad128;
    const int hb = m0 + wm * 64 + fr, cb = n0 + wn * 64 + 4 * fh;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(size_t)(cb + j * 16 + r) * hpad128 + hb + i * 16] = acc[i][j][r];
    if (blockIdx.x == 0) {  // the eight threads that share a row of the one-hot image
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int s = cnt[j];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            if ((tid & 7) == 0) cpart[(size_t)blockIdx.z * kpad + crow + 32 * j] = s;
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
    const int tiles = p.npad / TILE;
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
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(p.hpad128 / TILE, p.kpad / TILE, p.nsplit), dim3(256), 0, st, b.xt, b.labels, p.npad, p.chunk,
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
