// sim_tile.h -- the 128 x 128 tile of A . B^T on the matrix cores that match_kernel (match.hip), bank_topk_kernel (bank.hip),
// kmeans_assign_kernel and kmeans_update_kernel (kmeans.hip) share, its one-column form for coreset_sweep_kernel (coreset.hip), and the
// total order of "best" that their results are chosen by.
//
// The contract: the similarity of a pair is one chain of hpad / 32 v_mfma_f32_16x16x32_f16 k steps in ascending order from a zero
// accumulator.  It depends on hpad alone -- not on the tile the pair falls in, nor on the kernel or the pass that computes it -- so a pair
// has the same bits in match, bank top-k, k-means and the coreset sweep (tests/test_gpu_bank.py::test_top1_is_match,
// tests/test_gpu_kmeans.py::test_assign_is_match_bit_for_bit_and_inside_its_tolerance, tests/test_gpu_coreset.py::test_one_pick_is_match).
// It holds because the staging, the LDS image and the K loops exist here only: the tile's (sim_tile) and the one column's (sim_column),
// which issues the same instruction with the same operand roles over the same k steps.
// "Best" is one strict total order -- the larger f32 value first (-0 == +0), among equal values the lower index -- so a result does not
// depend on which lane, wave, tile, chunk or pass met a candidate first.  "Farthest" (the coreset's next pick) is the same order with the
// values reversed: the smaller value first, among equal values still the lower index.
#pragma once
#include <climits>

#include "device_types.h"
#include "kernels.h"

namespace dinov2 {

// ---- the order -------------------------------------------------------------------------------------------------------------------------
using Best = BankEntry;  // (value, index); an empty slot is (-inf, INT_MAX), which comes after every candidate
// (v, i) comes before b.  The rule stands here once; B is how the caller holds b, and that alone decides what hipcc makes of the `||`.
// Through a reference (fold: the running best) the index is read only where the values tie -- branches, few registers: by value
// match_kernel needs 216 VGPRs for 168 and loses a wave per SIMD.  By value (bank.hip) both compares are made and joined by logic:
// through a reference bank_topk_kernel's queue rounds grow by 380 instructions of branches.  (profiles/sim_tile.md)
template <class B>
__device__ __forceinline__ bool before(float v, int i, const B b) { return v > b.v || (v == b.v && i < b.i); }
__device__ __forceinline__ void fold(Best& b, float v, int i) {
    if (before<const Best&>(v, i, b)) b = Best{v, i};
}
template <int OFF>
__device__ __forceinline__ void fold_lane(Best& b) {
    const float v = __shfl_xor(b.v, OFF);
    const int i = __shfl_xor(b.i, OFF);
    fold(b, v, i);
}
// "farthest": (v, i) comes before b when its value is smaller, among equal values when its index is lower; an empty slot is (+inf, INT_MAX)
__device__ __forceinline__ void fold_far(Best& b, float v, int i) {
    if (v < b.v || (v == b.v && i < b.i)) b = Best{v, i};
}
template <int OFF>
__device__ __forceinline__ void fold_far_lane(Best& b) {
    const float v = __shfl_xor(b.v, OFF);
    const int i = __shfl_xor(b.i, OFF);
    fold_far(b, v, i);
}

// ---- the tile--------------------------------------------------------------------------------------------------------------------------
// 256 threads = four waves, 2 x 2, each 64 x 64 = 4 x 4 accumulator blocks of 16 x 16.  LDS image of an operand as in gemm.hip: [row][64 k]
// f16, 128-byte rows, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7), which spreads every 16-lane ds_read_b128 group over 16 bank
// slots.  The caller declares the two images (bank_topk_kernel reuses them as its queue); nothing here owns shared memory.
constexpr int SIM_TILE = 128, SIM_ROWB = 128;  // rows of a tile; bytes of one LDS row
static_assert(MATCH_TM == SIM_TILE && MATCH_TN == SIM_TILE, "the plans in kernels.h pad to this tile");

// A thread's place in the tile.  Staging: 128 rows x 8 chunks of 16 bytes per operand = 4 chunks per thread, chunk sc of rows srow[0 .. 3];
// 8 neighbouring threads read one 128-byte row segment.  acc[i][j][r] of sim_tile_k belongs to row 64 wm + 16 i + fr and column
// 64 wn + 16 j + 4 fh + r of the tile (operand swap: a lane owns one row, four columns).
struct SimPlace {
    int tid, lane, wid, wm, wn;
    int srow[4], sc, sdst[4];  // sdst: byte offset of staging slot j in the swizzled image
    int fr, fh, sw, aoff, boff;
    __device__ __forceinline__ SimPlace() {
        tid = threadIdx.x;
        lane = tid & 63;
        wid = tid >> 6;
        wm = wid >> 1, wn = wid & 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = j * 256 + tid, row = q >> 3, c = q & 7;
            srow[j] = row;
            sc = c;
            sdst[j] = row * SIM_ROWB + ((c ^ ((row >> 1) & 7)) << 4);
        }
        fr = lane & 15, fh = lane >> 4, sw = (fr >> 1) & 7;
        aoff = (wm * 64 + fr) * SIM_ROWB, boff = (wn * 64 + fr) * SIM_ROWB;
    }
};

// An operand whose tile is 128 rows of a row-major f16 matrix: rows [row0, +128) of `base` (ld elements apart), K-tile kt at columns
// [k0 + 64 kt, +64).  Operands are padded to whole tiles, so loads need no guards.  fetch() brings a thread's four chunks into registers,
// store() writes them to the image.  An operand built differently (kmeans_update_kernel's one-hot B) offers the same two.
struct SimRows {
    const char* src[4];
    u32x4 r[4];
    __device__ __forceinline__ SimRows(const SimPlace& p, const _Float16* base, int row0, size_t ld, int k0 = 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) src[j] = (const char*)base + ((size_t)(row0 + p.srow[j]) * ld + k0) * 2 + p.sc * 16;
    }
    __device__ __forceinline__ void fetch(int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = *(const u32x4*)(src[j] + (size_t)kt * SIM_ROWB);
    }
    __device__ __forceinline__ void store(const SimPlace& p, char* s) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) *(u32x4*)(s + p.sdst[j]) = r[j];
    }
};

// One K-tile of arithmetic from the images: two k steps of 32 in ascending order, sixteen MFMAs each.
__device__ __forceinline__ void sim_tile_k(const SimPlace& p, const char* sA, const char* sB, f32x4 (&acc)[4][4]) {
    using E = Elem<_Float16>;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int ch = ((ks * 4 + p.fh) ^ p.sw) << 4;
        f16x8 af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = *(const f16x8*)(sA + p.aoff + i * 16 * SIM_ROWB + ch);
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = *(const f16x8*)(sB + p.boff + j * 16 * SIM_ROWB + ch);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = E::mfma16(bf[j], af[i], acc[i][j]);  // operand swap
    }
}

// The K loop: acc = A . B^T over nk K-tiles, register-staged -- the next K-tile's loads are in flight under the MFMAs of this one.  The
// first barrier also ends whatever the workgroup did with the images before the call.
template <class OperandB>
__device__ __forceinline__ void sim_tile(const SimPlace& p, char* sA, char* sB, int nk, SimRows& a, OperandB& b, f32x4 (&acc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    a.fetch(0);
    b.fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // every wave is done reading the previous K-tile
        a.store(p, sA);
        b.store(p, sB);
        __syncthreads();
        if (kt + 1 < nk) {
            a.fetch(kt + 1);
            b.fetch(kt + 1);
        }
        sim_tile_k(p, sA, sB, acc);
    }
}

// ---- the best column of a row (match_kernel, kmeans_assign_kernel) ----------------------------------------------------------------------
// A lane's 16 columns of accumulator row i in ascending order into b; colb = the tile's first column + 64 wn + 4 fh.  Columns >= ncols
// are masked.  (+ 0.0f: a -0 becomes +0)
__device__ __forceinline__ void sim_row_fold(const f32x4 (&acc)[4][4], int i, int colb, int ncols, Best& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = colb + j * 16 + r;
            if (col < ncols) fold(b, acc[i][j][r] + 0.0f, col);
        }
}
// b of accumulator row i over the four lanes that share the row, left in red[wn]; after a barrier sim_fold_waves folds the two waves
// side by side
__device__ __forceinline__ void sim_row_share(const SimPlace& p, int i, Best b, float (&red_v)[2][SIM_TILE], int (&red_i)[2][SIM_TILE]) {
    fold_lane<16>(b);
    fold_lane<32>(b);
    if (p.fh == 0) {
        red_v[p.wn][p.wm * 64 + i * 16 + p.fr] = b.v;
        red_i[p.wn][p.wm * 64 + i * 16 + p.fr] = b.i;
    }
}
__device__ __forceinline__ Best sim_fold_waves(const float (&red_v)[2][SIM_TILE], const int (&red_i)[2][SIM_TILE], int e) {
    Best b{red_v[0][e], red_i[0][e]};
    fold(b, red_v[1][e], red_i[1][e]);
    return b;
}

// ---- the best column of every row of one 128-row tile of A over all of B's tiles (kmeans_assign_kernel, vlad_assign_kernel) ----------------
// A [.., hpad], B [npad_b, hpad]: normalised operands padded to whole tiles.  The workgroup walks B's tiles in ascending order, each a
// sim_tile, keeps the best (value, lowest column) per row across the tiles (columns >= nb masked) and folds lanes and waves.  Afterwards
// thread tid < SIM_TILE holds the best of row m0 + tid; the other threads hold an empty slot.  The walk stands here once, so that k-means'
// assignment and VLAD's cannot drift apart.  The caller declares the images and the two fold arrays.
__device__ __forceinline__ Best sim_best_of_rows(const SimPlace& p, char* sA, char* sB, float (&red_v)[2][SIM_TILE], int (&red_i)[2][SIM_TILE],
                                                 const _Float16* A, int m0, const _Float16* B, int nb, int npad_b, int hpad) {
    SimRows opa(p, A, m0, hpad);
    Best best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) best[i] = Best{-INFINITY, INT_MAX};
    for (int n0 = 0; n0 < npad_b; n0 += SIM_TILE) {  // B's tiles in ascending order
        SimRows opb(p, B, n0, hpad);
        f32x4 acc[4][4];
        sim_tile(p, sA, sB, hpad / 64, opa, opb, acc);
        // acc[i][j][r] = sim(row, column), row = m0 + 64 wm + 16 i + fr, column = n0 + 64 wn + 16 j + 4 fh + r; columns >= nb masked
#pragma unroll
        for (int i = 0; i < 4; ++i) sim_row_fold(acc, i, n0 + p.wn * 64 + 4 * p.fh, nb, best[i]);
    }
    // the four lanes that share a row, then the two waves side by side
#pragma unroll
    for (int i = 0; i < 4; ++i) sim_row_share(p, i, best[i], red_v, red_i);
    __syncthreads();
    return p.tid < SIM_TILE ? sim_fold_waves(red_v, red_i, p.tid) : Best{-INFINITY, INT_MAX};
}

// ---- one column: 16 rows of A against ONE row of B (coreset_sweep_kernel) ----------------------------------------------------------------
// The chain of sim_tile for a single column: per k step the same MFMA with the same operand roles (the B fragment first), from a zero
// accumulator, k steps ascending -- so the value has the bits the tile gives the pair.  The B row is the only real row of its 16-row
// fragment: lanes fr != 0 hand in zeros, lane fr == 0 reads it from sCol, a plain hpad f16 image of the row in LDS.  The A rows are
// streamed from global memory (each element is used once: no LDS image): `a` = this lane's row (row0 + fr of a row-major [.., hpad]
// operand) at column 8 fh.  One wave, all 64 lanes; nks = hpad / 32 (even).  Afterwards lane fr of the lanes fh == 0 holds sim(row0 + fr,
// the column); the other lanes' values mean nothing.
// U k steps from step ks on: the U loads of A are requested together, then the MFMAs follow in ascending order
template <int U>
__device__ __forceinline__ void sim_column_k(const _Float16* a, const char* sCol, int fr, int fh, int ks, f32x4& acc) {
    using E = Elem<_Float16>;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    f16x8 af[U], bf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) af[u] = *(const f16x8*)(a + (size_t)(ks + u) * 32);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const f16x8 c = *(const f16x8*)(sCol + (((ks + u) * 4 + fh) << 4));
        bf[u] = fr == 0 ? c : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = E::mfma16(bf[u], af[u], acc);
}
__device__ __forceinline__ float sim_column(const _Float16* a, const char* sCol, int fr, int fh, int nks) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int ks = 0;
    for (; ks + 8 <= nks; ks += 8) sim_column_k<8>(a, sCol, fr, fh, ks, acc);  // eight 16-byte loads a lane in flight
    for (; ks < nks; ks += 2) sim_column_k<2>(a, sCol, fr, fh, ks, acc);        // a K-tile of 64, as sim_tile_k
    return acc[0];
}

}  // namespace dinov2
