// vlad.hip -- VLAD descriptors of row segments (dinov2_hip_vlad_tokens, include/dinov2_hip.h) for gfx950 (MI355X).
//
// No reference counterpart: patch tokens assigned to the centres of a k-means vocabulary, the residuals summed per centre, normalised per
// centre and as a whole -- one vector per image for place recognition and retrieval.  The centre vectors are normalised by match.hip's
// kernel (launch_match_normalise); X^ is transposed by k-means' kernel (launch_kmeans_transpose).  The kernels here:
//   vlad_normalise_kernel  match's row normaliser (normalise_row.h) over a table of tiles: every segment into a block of its own, padded
//                       to whole 128-row tiles (VladPlan, kernels.h), in one launch
//   vlad_assign_kernel  kmeans_assign_kernel's walk (sim_best_of_rows, sim_tile.h) with a count of real rows per tile: one workgroup per
//                       128-row tile of X^ walks the centre tiles and writes the label into the padded layout (-1 on padding rows) and
//                       label and sim into the caller's order
//   vlad_update_kernel  kmeans_update_kernel driven by a table of chunks: D[h, c] = sum_i X^T[h, i] * (label[i] == c) over the K-tiles of one
//                       chunk of one segment, the one-hot operand built in LDS (onehot_rows.h); f32 partials [chunk][c][h], exact counts
//   vlad_finish_kernel  one workgroup per (segment, centre): folds the segment's partials of this pass in ascending chunk order onto what the
//                       passes before left, and behind the segment's last chunk forms the residual, its sum of squares and the row
//   vlad_l2_kernel      the descriptor of a segment over the sum of its rows' sums of squares
// No atomics anywhere: every sum has one fixed order, which depends on the segment's own length, K and H alone.
#include "normalise_row.h"
#include "onehot_rows.h"
#include "sim_tile.h"

namespace dinov2 {

// match's row normaliser (normalise_row.h) over the layout of 128-row tiles (VladPlan, kernels.h): row r of tile t of out is row
// g = tiles[t].out0 + r of the source where r < tiles[t].valid, a zero row otherwise; source row g lives at
// x + (g / per) * outer + (g % per) * ld floats.  32 workgroups per tile, four rows each, one wave a row.
__global__ __launch_bounds__(256) void vlad_normalise_kernel(const float* __restrict__ x, int per, size_t outer, size_t ld,
                                                             const VladTile* __restrict__ tiles, _Float16* __restrict__ out, int H, int hpad,
                                                             int vec) {
    const int t = blockIdx.x >> 5, r = (blockIdx.x & 31) * 4 + (threadIdx.x >> 6);
    const VladTile tl = tiles[t];
    const int g = tl.out0 + r;
    const float* const src = r < tl.valid ? x + (size_t)(g / per) * outer + (size_t)(g % per) * ld : nullptr;
    match_normalise_row(src, (f16x4*)(out + ((size_t)t * 128 + r) * hpad), threadIdx.x & 63, H, hpad, vec);
}

// X [npad, hpad], Cn [kpad, hpad]: the normalised operands.  Workgroup x owns rows [128 x, +128), all of one segment, of which the first
// tiles[x].valid are real: they are rows tiles[x].out0 .. of label_out / sim_out.  label [npad]: padding rows get -1.
__global__ __launch_bounds__(256) void vlad_assign_kernel(const _Float16* __restrict__ X, const _Float16* __restrict__ Cn, int hpad, int K, int kpad,
                                                          const VladTile* __restrict__ tiles, int* __restrict__ label,
                                                          int* __restrict__ label_out, float* __restrict__ sim_out) {
    __shared__ __attribute__((aligned(16))) char sA[SIM_TILE * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) char sB[SIM_TILE * SIM_ROWB];
    __shared__ float red_rv[2][SIM_TILE];
    __shared__ int red_ri[2][SIM_TILE];

    const SimPlace p;
    const int m0 = blockIdx.x * SIM_TILE;
    const Best b = sim_best_of_rows(p, sA, sB, red_rv, red_ri, X, m0, Cn, K, kpad, hpad);
    if (p.tid < SIM_TILE) {
        const VladTile t = tiles[blockIdx.x];
        if (p.tid < t.valid) {
            label[m0 + p.tid] = b.i;
            label_out[t.out0 + p.tid] = b.i;
            sim_out[t.out0 + p.tid] = b.v;
        } else {
            label[m0 + p.tid] = -1;
        }
    }
}

// XT [hpad128, npad], label [npad] (-1 on padding rows).  Workgroup (x, y, z): rows h [128 x, +128) of XT, centres [128 y, +128), chunk
// chunks[z]: its K-tiles of 64 rows in ascending order.  part [z][kpad][hpad128]: every element of the workgroup's tile is stored.
// cpart [z][kpad]: members of each centre in the chunk (workgroups x == 0).
__global__ __launch_bounds__(256) void vlad_update_kernel(const _Float16* __restrict__ XT, const int* __restrict__ label, int npad,
                                                          const VladChunk* __restrict__ chunks, int kpad, int hpad128, float* __restrict__ part,
                                                          int* __restrict__ cpart) {
    __shared__ __attribute__((aligned(16))) char sA[SIM_TILE * SIM_ROWB];
    __shared__ __attribute__((aligned(16))) char sB[SIM_TILE * SIM_ROWB];

    const SimPlace p;
    const int m0 = blockIdx.x * SIM_TILE, n0 = blockIdx.y * SIM_TILE;
    const VladChunk ch = chunks[blockIdx.z];

    SimRows opa(p, XT, m0, npad, ch.row0);
    OneHotRows opb{label + ch.row0 + (p.tid & 7) * 8, n0 + (p.tid >> 3), {}, {}, {0, 0, 0, 0}};
    f32x4 acc[4][4];
    sim_tile(p, sA, sB, ch.ktiles, opa, opb, acc);

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

namespace {
// The sum of v over the 256 threads in one order: the lanes of a wave by a butterfly, then the four waves ascending.  Every thread gets it.
__device__ __forceinline__ float vlad_block_sum(float v, float (&red)[4]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();  // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
}  // namespace

// Workgroup (c, y): centre c < K of segment s = seg0 + y; the pass holds chunks [c0, c1), chunk j at part[j - c0] / cpart[j - c0].  The
// segment's chunks inside the pass are folded in ascending order, starting from the first one (the segment starts in this pass) or from what
// the pass before left in vlad / counts.  Where the segment's last chunk is not in the pass the running sum and count go back there; else
// R[h] = S[h] - n c^[h], ss = sum of R^2 (thread t: h = t, t + 256, ... ascending, then vlad_block_sum: an order that depends on H alone),
// the row R or R / sqrt(ss) is written, and rowss = the sum of squares of the written row in the same order.
__global__ __launch_bounds__(256) void vlad_finish_kernel(const float* __restrict__ part, const int* __restrict__ cpart,
                                                          const VladSeg* __restrict__ segs, int seg0, int c0, int c1, int kpad, int hpad128, int K,
                                                          int H, const _Float16* __restrict__ Cn, int hpad, unsigned flags,
                                                          float* __restrict__ vlad, int* __restrict__ counts, float* __restrict__ rowss) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int c = blockIdx.x, s = seg0 + blockIdx.y, tid = threadIdx.x;
    const VladSeg sg = segs[s];
    const int a = sg.chunk0 > c0 ? sg.chunk0 : c0, end = sg.chunk0 + sg.nchunks, b = end < c1 ? end : c1;
    const bool first = a == sg.chunk0, last = b == end;
    float* const out = vlad + ((size_t)s * K + c) * H;

    int cnt = first ? 0 : counts[(size_t)s * K + c];
    for (int j = a; j < b; ++j) cnt += cpart[(size_t)(j - c0) * kpad + c];

    float r[16];  // H <= 4096
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int h = tid + 256 * k;
        r[k] = 0.0f;
        if (h < H) {
            const float* const src = part + ((size_t)(a - c0) * kpad + c) * hpad128 + h;
            float v = first ? src[0] : out[h];
            for (int j = first ? 1 : 0; j < b - a; ++j) v += src[(size_t)j * kpad * hpad128];
            r[k] = v;
        }
    }
    if (!last) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (tid + 256 * k < H) out[tid + 256 * k] = r[k];
        if (tid == 0) counts[(size_t)s * K + c] = cnt;
        return;
    }
    const float nf = (float)cnt;  // exact: at most 2^20 rows
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int h = tid + 256 * k;
        if (h < H) {
            r[k] = cnt > 0 ? r[k] - nf * (float)Cn[(size_t)c * hpad + h] : 0.0f;
            ss += r[k] * r[k];
        }
    }
    ss = vlad_block_sum(ss, red);
    if ((flags & VLAD_INTRA_NORM) && ss > 0.0f) {
        const float nrm = sqrtf(ss);  // correctly rounded, as the division below (the compiler's default for f32)
        ss = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (tid + 256 * k < H) {
                r[k] = r[k] / nrm;
                ss += r[k] * r[k];
            }
        ss = vlad_block_sum(ss, red);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (tid + 256 * k < H) out[tid + 256 * k] = r[k];
    if (tid == 0) {
        counts[(size_t)s * K + c] = cnt;
        rowss[(size_t)s * K + c] = ss;
    }
}

// Workgroup (x, s): elements [4096 x, +4096) of the K H values of segment s over sqrt(total), total = the rows' sums of squares (thread t:
// c = t, t + 256, ... ascending, then vlad_block_sum: an order that depends on K alone, on top of the rows' own, which depends on H alone).
// Every workgroup of a segment forms the same total; total == 0 leaves the zeros.
__global__ __launch_bounds__(256) void vlad_l2_kernel(float* __restrict__ vlad, const float* __restrict__ rowss, int K, int H) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int s = blockIdx.y;
    float t = 0.0f;
    for (int c = threadIdx.x; c < K; c += 256) t += rowss[(size_t)s * K + c];
    t = vlad_block_sum(t, red);
    if (!(t > 0.0f)) return;
    const float nrm = sqrtf(t);
    const size_t total = (size_t)K * H, i0 = (size_t)blockIdx.x * 4096;
    float* const v = vlad + (size_t)s * total;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const size_t i = i0 + threadIdx.x + 256 * k;
        if (i < total) v[i] = v[i] / nrm;
    }
}

VladBufs vlad_bufs(char* ws, const VladPlan& p) {
    VladBufs b;
    b.x16 = (_Float16*)(ws + p.x16);
    b.xt = (_Float16*)(ws + p.xt);
    b.c16 = (_Float16*)(ws + p.c16);
    b.cvec = (float*)(ws + p.cvec);
    b.labels = (int*)(ws + p.labels);
    b.labels_out = (int*)(ws + p.labels_out);
    b.sim_out = (float*)(ws + p.sim_out);
    b.part = (float*)(ws + p.part);
    b.cpart = (int*)(ws + p.cpart);
    b.vlad = (float*)(ws + p.vlad);
    b.counts = (int*)(ws + p.counts);
    b.rowss = (float*)(ws + p.rowss);
    b.segs = (VladSeg*)(ws + p.segs);
    b.chunks = (VladChunk*)(ws + p.chunks);
    b.tiles = (VladTile*)(ws + p.tiles);
    return b;
}

hipError_t launch_vlad_normalise(const float* x, int per, size_t outer, size_t ld, const VladTile* tiles, int ntiles, _Float16* out, int H,
                                 int hpad, hipStream_t st) {
    const int vec = H % 4 == 0 && ld % 4 == 0 && outer % 4 == 0 && ((size_t)x & 15) == 0;
    hipLaunchKernelGGL(vlad_normalise_kernel, dim3(ntiles * 32), dim3(256), 0, st, x, per, outer, ld, tiles, out, H, hpad, vec);
    return hipGetLastError();
}

hipError_t launch_vlad_assign(const VladBufs& b, int K, const VladPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(vlad_assign_kernel, dim3(p.ntiles), dim3(256), 0, st, b.x16, b.c16, p.hpad, K, p.kpad, b.tiles, b.labels, b.labels_out,
                       b.sim_out);
    return hipGetLastError();
}

hipError_t launch_vlad_sums(const VladBufs& b, int n_seg, int K, int H, unsigned flags, const VladPlan& p, const VladChunk* chunks,
                            hipStream_t st) {
    for (int c0 = 0; c0 < p.nchunks; c0 += p.cap) {  // the passes
        const int c1 = c0 + p.cap < p.nchunks ? c0 + p.cap : p.nchunks;
        const int seg0 = chunks[c0].seg, seg1 = chunks[c1 - 1].seg;
        hipLaunchKernelGGL(vlad_update_kernel, dim3(p.hpad128 / SIM_TILE, p.kpad / SIM_TILE, c1 - c0), dim3(256), 0, st, b.xt, b.labels, p.npad,
                           b.chunks + c0, p.kpad, p.hpad128, b.part, b.cpart);
        hipLaunchKernelGGL(vlad_finish_kernel, dim3(K, seg1 - seg0 + 1), dim3(256), 0, st, b.part, b.cpart, b.segs, seg0, c0, c1, p.kpad, p.hpad128,
                           K, H, b.c16, p.hpad, flags, b.vlad, b.counts, b.rowss);
    }
    if (flags & VLAD_L2_NORM)
        hipLaunchKernelGGL(vlad_l2_kernel, dim3((unsigned)(((size_t)K * H + 4095) / 4096), n_seg), dim3(256), 0, st, b.vlad, b.rowss, K, H);
    return hipGetLastError();
}

hipError_t vlad_run(const VladBufs& b, int n_seg, int K, int H, unsigned flags, const VladPlan& p, const VladChunk* chunks, hipStream_t st) {
    hipError_t e = launch_match_normalise(b.cvec, (size_t)H, b.c16, K, p.kpad, H, p.hpad, st);
    if (e == hipSuccess) e = launch_vlad_assign(b, K, p, st);
    if (e == hipSuccess) {  // k-means' transpose over the whole padded layout
        KmeansPlan kp{};
        kp.npad = p.npad, kp.hpad = p.hpad, kp.hpad128 = p.hpad128;
        KmeansBufs kb{};
        kb.x16 = b.x16, kb.xt = b.xt;
        e = launch_kmeans_transpose(kb, kp, st);
    }
    return e != hipSuccess ? e : launch_vlad_sums(b, n_seg, K, H, flags, p, chunks, st);
}

}  // namespace dinov2
