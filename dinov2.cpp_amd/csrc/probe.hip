// probe.hip -- the k most similar rows over the union of each query's OWN subset of row ranges of a bank (dinov2_hip_bank_topk_probe,
// include/dinov2_hip.h) for gfx950 (MI355X): the search step of an inverted file.
//
// No reference counterpart.  The probe table [n, n_probe] is inverted on the host (probe_plan, kernels.h) into items: one piece of a segment
// with the queries that probe the segment.  Three kernels:
//   probe_tile_kernel    the wide form, up to 128 queries an item: bank_topk_kernel's walk over the piece's column tiles, each a tile of
//                        sim_tile.h with the per-row lists and queue rounds of topk_list.h.  The A operand gathers its rows from the query
//                        matrix by the item's list (SimRowsGathered); the B operand starts at any row (SimRowsClamped); a candidate's index
//                        is its bank row; the lists leave through the scatter form of topk_list_write.
//   probe_narrow_kernel  the narrow form, up to 16 queries an item -- the case of a handful of queries against a huge bank, where a
//                        128-row tile would spend 7/8 of the matrix cores on padding and both operands would cross LDS.  The 16 query rows
//                        stay in LDS for the whole walk; the bank rows are streamed from global memory once, straight into the MFMA's
//                        first operand, 16 loads of 16 bytes a lane in flight.  Each wave keeps lists of its own, so the walk has no
//                        barrier; the four waves' lists are folded once at the end.  
//   probe_fill_kernel    every list of a pass empty, before the items write theirs: a query with fewer lists than the pass has slots
//   The lists of a query are folded by bank_merge_kernel (bank.hip), unchanged.
// A similarity is sim_tile.h's chain: hpad / 32 v_mfma_f32_16x16x32_f16 k steps in ascending order from a zero accumulator, the bank
// fragment first -- in the narrow form too, which issues the same instruction with the same operand roles (as sim_column does for one
// column).  The order of "best" is sim_tile.h's, inserts are wave_insert's: strict and total over distinct indices, so the first k of a
// query are one list whatever the form, the piece, the slot order and the pass.
#include "sim_tile.h"
#include "topk_list.h"

namespace dinov2 {

__global__ __launch_bounds__(256) void probe_fill_kernel(BankEntry* __restrict__ part, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) part[e] = BankEntry{-INFINITY, INT_MAX};
}

// Q [.., hpad]: the normalised queries; bank: rows 0 .. last_row of hpad f16.  Workgroup x = item x: queries rows_q[it.rows + r], r < it.nq,
// against bank rows [it.row0, +it.nrows); the list of r goes to part[rows_dst[it.rows + r] * k ..].  Dynamic LDS: BankEntry [128][k].
__global__ __launch_bounds__(256) void probe_tile_kernel(const _Float16* __restrict__ Q, const _Float16* __restrict__ bank, int last_row, int hpad,
                                                         int k, const ProbeItem* __restrict__ items, const int* __restrict__ rows_q,
                                                         const int* __restrict__ rows_dst, BankEntry* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) char sAB[2 * SIM_TILE * SIM_ROWB];  // operands in the K loop, the candidate queue after it
    __shared__ unsigned qmask[SIM_TILE];
    extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
    char* const sA = sAB;
    char* const sB = sAB + SIM_TILE * SIM_ROWB;
    BankEntry* const queue = (BankEntry*)sAB;
    BankEntry* const list = (BankEntry*)dyn_lds;

    const SimPlace p;
    const ProbeItem it = items[blockIdx.x];
    const int* const my_q = rows_q + it.rows;
    const int* const my_dst = rows_dst + it.rows;
    const int wn = p.wn, fh = p.fh;

    topk_list_init(p, list, qmask, k);
    SimRowsGathered opa(p, Q, my_q, it.nq, hpad);
    for (int n0 = 0; n0 < it.nrows; n0 += SIM_TILE) {  // the piece's column tiles in ascending order
        SimRowsClamped opb(p, bank, it.row0 + n0, last_row, hpad);
        f32x4 acc[4][4];
        sim_tile(p, sA, sB, hpad / 64, opa, opb, acc);  // (its first barrier: every wave is done with the queue of the previous tile)
        __syncthreads();                                // the operand image is free
        // the candidates: the item's real queries against the columns inside the piece, under their bank row
        topk_queue_rounds(p, acc, queue, qmask, list, k, [&](int, int rl, int j, int r) __attribute__((always_inline)) {
            const int col = n0 + wn * 64 + j * 16 + 4 * fh + r;
            return rl < it.nq && col < it.nrows ? it.row0 + col : -1;
        });
    }
    topk_list_scatter(p, list, k, it.nq, part, [&](int rl) __attribute__((always_inline)) { return my_dst[rl]; });
}

// ---- the narrow form ------------------------------------------------------------------------------------------------------------------------
// 256 threads = four waves.  The item's 16 query rows (rows >= it.nq repeat the last one and are masked) lie in LDS chunk-major:
// image[c][r] = the 16 bytes of k elements [8 c, 8 c + 8) of row r, so lane (fr, fh) finds its second MFMA operand of k step ks --
// row fr, elements 32 ks + 8 fh .. -- at byte 1024 ks + 16 lane: a wave's ds_read_b128 covers 1 KiB contiguously, every 16-lane group 256
// bytes = all 64 banks once.  The piece is cut into groups of 16 bank rows; wave w owns groups w, w + 4, w + 8, ..., PN_G of them at a
// time: lane (fr, fh) loads row fr of each group at elements 32 ks + 8 fh .. straight from global memory as the first operand (each
// element is used once: no LDS image), PN_U k steps ahead, and one LDS read feeds PN_G MFMAs.  acc[g][r] of lane (fr, fh) = sim(query fr,
// row 4 fh + r of group g).  Dynamic LDS: the image [hpad / 8][16][16 bytes], then BankEntry [4 waves][16][k].
constexpr int PN_G = 4, PN_U = 4;

template <int U>
__device__ __forceinline__ void probe_narrow_k(const char* const (&b)[PN_G], const char* img, int ks, f32x4 (&acc)[PN_G]) {
    using E = Elem<_Float16>;
    f16x8 bf[PN_G][U], af[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int g = 0; g < PN_G; ++g) bf[g][u] = *(const f16x8*)(b[g] + (size_t)(ks + u) * 64);
#pragma unroll
    for (int u = 0; u < U; ++u) af[u] = *(const f16x8*)(img + (size_t)(ks + u) * 1024);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int g = 0; g < PN_G; ++g) acc[g] = E::mfma16(bf[g][u], af[u], acc[g]);  // sim_tile_k's operand roles; k steps ascending per chain
}

__global__ __launch_bounds__(256) void probe_narrow_kernel(const _Float16* __restrict__ Q, const _Float16* __restrict__ bank, int hpad, int k,
                                                           const ProbeItem* __restrict__ items, const int* __restrict__ rows_q,
                                                           const int* __restrict__ rows_dst, BankEntry* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
    char* const img = dyn_lds;
    BankEntry* const lists = (BankEntry*)(dyn_lds + (size_t)PROBE_NARROW_ROWS * hpad * 2);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, fr = lane & 15, fh = lane >> 4;
    const ProbeItem it = items[blockIdx.x];
    const int* const my_q = rows_q + it.rows;
    const int* const my_dst = rows_dst + it.rows;
    BankEntry* const mine = lists + wid * PROBE_NARROW_ROWS * k;

    for (int e = tid; e < PROBE_NARROW_ROWS * (hpad / 8); e += 256) {  // e = 16 c + r
        const int r = (e & 15) < it.nq ? (e & 15) : it.nq - 1;
        *(u32x4*)(img + (size_t)e * 16) = *(const u32x4*)(Q + (size_t)my_q[r] * hpad + (e >> 4) * 8);
    }
    for (int e = tid; e < PROBE_NARROW_WAVES * PROBE_NARROW_ROWS * k; e += 256) lists[e] = BankEntry{-INFINITY, INT_MAX};
    __syncthreads();

    const int ngroups = (it.nrows + 15) / 16, nks = hpad / 32, last = it.row0 + it.nrows - 1;
    const char* const my_img = img + lane * 16;
    for (int g0 = wid; g0 < ngroups; g0 += PROBE_NARROW_WAVES * PN_G) {
        const char* b[PN_G];
#pragma unroll
        for (int g = 0; g < PN_G; ++g) {  // a group past the piece's end reads the piece's last row again: masked below
            const int row = it.row0 + (g0 + PROBE_NARROW_WAVES * g) * 16 + fr;
            b[g] = (const char*)(bank + (size_t)(row < last ? row : last) * hpad) + fh * 16;
        }
        f32x4 acc[PN_G];
#pragma unroll
        for (int g = 0; g < PN_G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        int ks = 0;
        for (; ks + PN_U <= nks; ks += PN_U) probe_narrow_k<PN_U>(b, my_img, ks, acc);
        for (; ks < nks; ks += 2) probe_narrow_k<2>(b, my_img, ks, acc);  // (nks is even: a K-tile of 64, as sim_tile_k)

        // the candidates of this wave's 16 x 64 similarities into its own lists: list `row` one entry per lane, inserted by wave_insert
#pragma unroll
        for (int g = 0; g < PN_G; ++g) {
            const int base = (g0 + PROBE_NARROW_WAVES * g) * 16;  // of the piece's rows
            if (base >= it.nrows) break;                          // (uniform)
            const BankEntry thr = mine[fr * k + k - 1];
            float v[4];
            int bits = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = base + 4 * fh + r;
                v[r] = acc[g][r] + 0.0f;  // a -0 becomes +0
                if (fr < it.nq && col < it.nrows && before(v[r], it.row0 + col, thr)) bits |= 1 << r;
            }
            unsigned long long todo = __ballot(bits != 0);
            while (todo) {
                const int row = (__ffsll((long long)todo) - 1) & 15;
                todo &= ~(0x0001000100010001ull << row);
                BankEntry e = lane < k ? mine[row * k + lane] : BankEntry{-INFINITY, INT_MAX};
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    int m = __builtin_amdgcn_readlane(bits, row + 16 * h);
                    while (m) {
                        const int r = __ffs(m) - 1;
                        m &= m - 1;
                        const float mv = r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3];
                        const float cv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mv), row + 16 * h));
                        wave_insert(e, BankEntry{cv, it.row0 + base + 4 * h + r}, k, lane);
                    }
                }
                if (lane < k) mine[row * k + lane] = e;
            }
        }
    }
    __syncthreads();
    // the four waves' lists of a query folded (bank_merge_kernel's step); wave w writes queries 4 w .. 4 w + 3
    for (int rr = 0; rr < PROBE_NARROW_ROWS / PROBE_NARROW_WAVES; ++rr) {
        const int row = wid * (PROBE_NARROW_ROWS / PROBE_NARROW_WAVES) + rr;
        if (row >= it.nq) break;
        BankEntry e = lane < k ? lists[row * k + lane] : BankEntry{-INFINITY, INT_MAX};
        for (int w = 1; w < PROBE_NARROW_WAVES; ++w) {
            const BankEntry x = lane < k ? lists[(w * PROBE_NARROW_ROWS + row) * k + lane] : BankEntry{-INFINITY, INT_MAX};
            for (int j = 0; j < k; ++j) {
                const BankEntry cand{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x.v), j)), __builtin_amdgcn_readlane(x.i, j)};
                const float kv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e.v), k - 1));
                const int ki = __builtin_amdgcn_readlane(e.i, k - 1);
                if (!before(cand.v, cand.i, BankEntry{kv, ki})) break;  // the rest of this sorted list comes after it
                wave_insert(e, cand, k, lane);
            }
        }
        if (lane < k) part[(size_t)my_dst[row] * k + lane] = e;
    }
}

hipError_t launch_probe(const float* q, size_t ldq, int n, int H, const _Float16* bank, int last_row, int k, char* ws, const ProbePlan& p,
                        const ProbeTables& t, hipStream_t st) {
    if (n < 1 || k < 1 || k > BANK_K_MAX || last_row < 0 || (p.n_narrow > 0 && p.narrow_lds == 0)) return hipErrorInvalidValue;
    _Float16* const q16 = (_Float16*)(ws + p.q16);
    BankEntry* const part = (BankEntry*)(ws + p.part);
    ProbeItem* const items = (ProbeItem*)(ws + p.items);
    int* const rows_q = (int*)(ws + p.rows_q);
    int* const rows_dst = (int*)(ws + p.rows_dst);
    int* const idx = (int*)(ws + p.idx);
    float* const sim = (float*)(ws + p.sim);
    hipError_t e = launch_match_normalise(q, ldq, q16, n, p.nq_pad, H, p.hpad, st);
    if (e != hipSuccess) return e;
    const size_t lds_wide = (size_t)SIM_TILE * k * sizeof(BankEntry);
    if (p.n_wide > 0) e = gemm_raise_lds((const void*)probe_tile_kernel, lds_wide);  // (per device; cheap enough to repeat)
    if (e == hipSuccess && p.n_narrow > 0) e = gemm_raise_lds((const void*)probe_narrow_kernel, p.narrow_lds);
    if (e != hipSuccess) return e;
    for (const ProbePass& ps : t.passes) {
        const int n_items = ps.n_wide + ps.n_narrow;
        if (n_items > 0) {  // (stream order: the pass before has read the tables by the time these copies run)
            e = hipMemcpyAsync(items, t.items.data() + ps.item0, (size_t)n_items * sizeof(ProbeItem), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(rows_q, t.rows_q.data() + ps.row0, (size_t)ps.nrows * 4, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(rows_dst, t.rows_dst.data() + ps.row0, (size_t)ps.nrows * 4, hipMemcpyHostToDevice, st);
            if (e != hipSuccess) return e;
            const size_t entries = (size_t)ps.slots * ps.nq * k;
            hipLaunchKernelGGL(probe_fill_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, part, entries);
        }
        if (ps.n_wide > 0)
            hipLaunchKernelGGL(probe_tile_kernel, dim3(ps.n_wide), dim3(256), lds_wide, st, q16, bank, last_row, p.hpad, k, items, rows_q, rows_dst,
                               part);
        if (ps.n_narrow > 0)
            hipLaunchKernelGGL(probe_narrow_kernel, dim3(ps.n_narrow), dim3(256), p.narrow_lds, st, q16, bank, p.hpad, k, items + ps.n_wide, rows_q,
                               rows_dst, part);
        e = launch_bank_merge(part, ps.nq, ps.slots, k, ps.nq, idx + (size_t)ps.q0 * k, sim + (size_t)ps.q0 * k, st);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace dinov2
