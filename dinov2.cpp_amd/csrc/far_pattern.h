// The operand pattern of the far-offset diagnostic ops (csrc/ops_testing.cpp: dinov2_hip_op_gemm_far, dinov2_hip_op_attention_far): one pure
// function of (seed, row, col), evaluated on the device by the fill kernels and restated in numpy by tests/far_cases.py.  Host- and
// device-compilable and free of HIP, so that a plain C++ compiler builds it (tests/cpp/far_pattern_print.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FAR_PATTERN_HD __host__ __device__
#else
#define FAR_PATTERN_HD
#endif

namespace dinov2 {

// An integer in [-64, 64): the top 7 bits of a 64-bit mix of the arguments.  The row enters as a full 64-bit number and the mix is a
// bijection of the 64-bit word that row, col and seed are folded into, so the value has no period in `row`: two rows 2^31 or 2^32 BYTES
// apart (the aliases of a truncated or sign-flipped offset) hold unrelated data.
FAR_PATTERN_HD inline int far_value_q(uint64_t seed, uint64_t row, uint32_t col) {
    uint64_t h = row * 0x9E3779B97F4A7C15ull + ((uint64_t)col + 1u) * 0xC2B2AE3D27D4EB4Full + (seed + 1u) * 0x165667B19E3779F9ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    h *= 0x94D049BB133111EBull;
    h ^= h >> 29;
    return (int)(h >> 57) - 64;
}

// The operand value: a multiple of 1/64 in [-1, 1).  Exact in f16 and bf16 (7 significant bits); with both operands on this grid and
// K <= 4096 every product (a multiple of 2^-12, at most 1) and every partial sum of a GEMM (12 fraction bits, at most 12 integer bits) is
// exact in f32, in any order.
FAR_PATTERN_HD inline float far_value(uint64_t seed, uint64_t row, uint32_t col) { return (float)far_value_q(seed, row, col) * 0.015625f; }

// Far ROWS (dinov2_hip_op_rows_fill; tests/rows_far_cases.py restates both functions in numpy): row `row` of an operand is one entry of a small
// dictionary of rows.  The common entries [0, d_common) are drawn by a hash of the full 64-bit row index -- two far_value_q calls give 14 bits,
// reduced modulo d_common (1 .. 16384) -- so, like far_value, the choice has no period in `row`.
FAR_PATTERN_HD inline int far_rows_sel(uint64_t seed, uint64_t row, int d_common) {
    const int hi = far_value_q(seed, row, 0u) + 64, lo = far_value_q(seed, row, 1u) + 64;
    return (hi * 128 + lo) % d_common;
}

// The entry of a row: a short list of planted rows (plant_rows strictly ascending; plant_entries beside it) overrides the hash.
FAR_PATTERN_HD inline int far_rows_entry(uint64_t seed, uint64_t row, int d_common, const int64_t* plant_rows, const int32_t* plant_entries,
                                         int nplants) {
    int lo = 0, hi = nplants;  // the first plant whose row is >= row
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if ((uint64_t)plant_rows[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    if (lo < nplants && (uint64_t)plant_rows[lo] == row) return plant_entries[lo];
    return far_rows_sel(seed, row, d_common);
}

}  // namespace dinov2
