// coreset.hip -- greedy k-center (farthest-point) selection of rows (dinov2_hip_coreset_tokens, include/dinov2_hip.h) and the row gather
// of dinov2_hip_bank_keep, for gfx950 (MI355X).
//
// No reference counterpart: thinning a memory bank of patch tokens to the few per cent that cover the rest (PatchCore, AnomalyDINO), maximin
// seeding of k-means.  The rows are normalised by match.hip's kernel (launch_match_normalise) or are a bank's; the kernels here:
//   coreset_init_kernel   idx = -1, cover = +inf, the stop flag cleared, selected = m
//   coreset_sweep_kernel  launch t = pick t.  Every workgroup folds the previous launch's partials to the pick itself (launch 0: `first`)
//                         and takes the stop decision; workgroup 0 records idx[t] / cover[t].  Then one sweep over the workgroup's rows:
//                         each row's similarity to the picked row (sim_tile.h's one-column chain: the bits of match) against its s, s and
//                         nearest updated on a strictly greater value, and the workgroup's unselected rows folded to one (smallest s,
//                         lowest row) partial for the next launch.
//   bank_gather_kernel    out[j] = rows[idx[j]]
// Stream order between the launches is the only synchronisation: no atomics, no grid barrier, no workgroup waits for another.  The two
// partial buffers alternate, so a launch reads only what the launch before it wrote.  A row's selected mark is read and written by the
// workgroup that owns the row alone.  A launch that finds the stop flag set returns at once, so the host may run ahead of the flag.
#include "sim_tile.h"

namespace dinov2 {

__global__ __launch_bounds__(256) void coreset_init_kernel(int* __restrict__ idx, float* __restrict__ cover, int* __restrict__ head, int m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        idx[i] = -1;
        cover[i] = INFINITY;
    }
    if (i == 0) {
        head[0] = 0;
        head[1] = m;
    }
}

// the farthest of the four waves' candidates, in every thread (red: one slot per wave)
__device__ __forceinline__ Best coreset_fold_workgroup(Best b, int lane, int wid, float (&red_v)[4], int (&red_i)[4]) {
    fold_far_lane<1>(b);
    fold_far_lane<2>(b);
    fold_far_lane<4>(b);
    fold_far_lane<8>(b);
    fold_far_lane<16>(b);
    fold_far_lane<32>(b);
    __syncthreads();  // the slots' readers of an earlier call are done
    if (lane == 0) {
        red_v[wid] = b.v;
        red_i[wid] = b.i;
    }
    __syncthreads();
    Best r{red_v[0], red_i[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w) fold_far(r, red_v[w], red_i[w]);
    return r;
}

// X [>= n up to 16 rows, hpad]: normalised rows.  Workgroup x: rows [x rows_per_wg, min(+rows_per_wg, n)), sixteen at a time per wave.
// part [2][CORESET_PARTS_MAX]: launch t reads half (t - 1) & 1 (nparts entries), writes entry x of half t & 1.
__global__ __launch_bounds__(256) void coreset_sweep_kernel(const _Float16* __restrict__ X, int hpad, int n, int rows_per_wg, int nparts, int t,
                                                            int first, float stop_sim, float* __restrict__ sim, int* __restrict__ nearest,
                                                            unsigned char* __restrict__ mark, BankEntry* __restrict__ part,
                                                            int* __restrict__ head, int* __restrict__ idx, float* __restrict__ cover) {
    __shared__ __attribute__((aligned(16))) char sCol[4096 * 2];
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ int stopped;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // One thread reads the flag for the workgroup: the launch that raises it may be this one (workgroup 0, below), and a flag that every
    // thread read for itself could part the workgroup before a barrier.  Either value ends this launch the same way.
    if (tid == 0) stopped = head[0];
    __syncthreads();
    if (stopped) return;

    int pick = first;
    if (t > 0) {
        const BankEntry* const prev = part + (size_t)((t - 1) & 1) * CORESET_PARTS_MAX;
        Best b{INFINITY, INT_MAX};
        for (int i = tid; i < nparts; i += 256) fold_far(b, prev[i].v, prev[i].i);
        b = coreset_fold_workgroup(b, lane, wid, red_v, red_i);
        if (b.v >= stop_sim) {  // (the same in every workgroup)
            if (blockIdx.x == 0 && tid == 0) {
                head[1] = t;
                head[0] = 1;
            }
            return;
        }
        pick = b.i;
        if (blockIdx.x == 0 && tid == 0) {
            idx[t] = pick;
            cover[t] = b.v;
        }
    } else if (blockIdx.x == 0 && tid == 0) {
        idx[0] = first;
        cover[0] = -INFINITY;
    }

    // the picked row: a plain image in LDS
    for (int c = tid; c < hpad / 8; c += 256) ((u32x4*)sCol)[c] = ((const u32x4*)(X + (size_t)pick * hpad))[c];
    __syncthreads();

    const int fr = lane & 15, fh = lane >> 4;
    const int r0 = blockIdx.x * rows_per_wg;
    const int r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
    Best far{INFINITY, INT_MAX};
    for (int g = r0 + wid * 16; g < r1; g += 64) {
        const int row = g + fr;
        const float v = sim_column(X + (size_t)row * hpad + 8 * fh, sCol, fr, fh, hpad / 32) + 0.0f;  // (+ 0.0f: a -0 becomes +0)
        if (fh == 0 && row < n) {
            float s = t > 0 ? sim[row] : -INFINITY;
            if (v > s) {
                s = v;
                sim[row] = v;
                nearest[row] = t;
            }
            const bool selected = row == pick || (t > 0 && mark[row] != 0);
            if (row == pick) mark[row] = 1;
            else if (t == 0) mark[row] = 0;
            if (!selected) fold_far(far, s, row);
        }
    }
    far = coreset_fold_workgroup(far, lane, wid, red_v, red_i);
    if (tid == 0) part[(size_t)(t & 1) * CORESET_PARTS_MAX + blockIdx.x] = far;
}

// out[j, :] = rows[idx[j], :]; one workgroup per row, 16 bytes a thread and turn
__global__ __launch_bounds__(256) void bank_gather_kernel(const _Float16* __restrict__ rows, const int* __restrict__ idx, int hpad,
                                                          _Float16* __restrict__ out) {
    const u32x4* const src = (const u32x4*)(rows + (size_t)idx[blockIdx.x] * hpad);
    u32x4* const dst = (u32x4*)(out + (size_t)blockIdx.x * hpad);
    for (int c = threadIdx.x; c < hpad / 8; c += 256) dst[c] = src[c];
}

hipError_t launch_bank_gather(const _Float16* rows, const int* idx, int count, int hpad, _Float16* out, hipStream_t st) {
    if (count < 1 || hpad < 64 || hpad % 64 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bank_gather_kernel, dim3(count), dim3(256), 0, st, rows, idx, hpad, out);
    return hipGetLastError();
}

CoresetBufs coreset_bufs(char* ws, const CoresetPlan& p, const _Float16* bank_rows) {
    CoresetBufs b;
    b.x16 = bank_rows ? bank_rows : (const _Float16*)(ws + p.x16);
    b.sim = (float*)(ws + p.sim);
    b.nearest = (int*)(ws + p.nearest);
    b.mark = (unsigned char*)(ws + p.mark);
    b.part = (BankEntry*)(ws + p.part);
    b.head = (int*)(ws + p.head);
    b.idx = (int*)(ws + p.idx);
    b.cover = (float*)(ws + p.cover);
    return b;
}

hipError_t coreset_run(const CoresetBufs& b, int n, int m, int first, float stop_sim, const CoresetPlan& p, hipStream_t st) {
    if (n < 1 || m < 1 || m > n || first < 0 || first >= n || stop_sim != stop_sim || p.nparts < 1 || p.nparts > CORESET_PARTS_MAX ||
        p.rows_per_wg % SIM_TILE != 0 || (long long)p.nparts * p.rows_per_wg < n || p.hpad > 4096)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(coreset_init_kernel, dim3((m + 255) / 256), dim3(256), 0, st, b.idx, b.cover, b.head, m);
    hipError_t e = hipGetLastError();
    const bool may_stop = stop_sim < INFINITY;
    for (int t = 0; t < m && e == hipSuccess; ++t) {
        hipLaunchKernelGGL(coreset_sweep_kernel, dim3(p.nparts), dim3(256), 0, st, b.x16, p.hpad, n, p.rows_per_wg, p.nparts, t, first, stop_sim,
                           b.sim, b.nearest, b.mark, b.part, b.head, b.idx, b.cover);
        e = hipGetLastError();
        if (e == hipSuccess && may_stop && (t + 1) % CORESET_POLL == 0 && t + 1 < m) {  // only to stop launching: the result is the device's
            int stopped = 0;
            e = hipMemcpyAsync(&stopped, b.head, 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (stopped) break;
        }
    }
    return e;
}

}  // namespace dinov2
