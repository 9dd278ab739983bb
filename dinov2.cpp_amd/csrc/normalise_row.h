// normalise_row.h -- contract 1 of dinov2_hip_match for one row: the one normaliser of match.hip (match_normalise_kernel: match, bank,
// k-means) and vlad.hip (vlad_normalise_kernel), written once so that a row has the same f16 bits through either.
#pragma once
#include "device_types.h"

namespace dinov2 {

// One row by one wave (contract 1 of dinov2_hip_match): o [hpad] f16 = src [H] / sqrt(sum of squares), 0 for an all-zero row, for
// src == nullptr (a padding row) and for columns >= H.  Lane l owns the 4-float chunks l, l + 64, ... (16-byte loads when `vec`: H and the
// row's address multiples of 4 floats; the summation order is the same either way, so it depends on H alone).  The one normaliser of
// match.hip, bank.hip, kmeans.hip and vlad.hip.
__device__ __forceinline__ void match_normalise_row(const float* __restrict__ src, f16x4* __restrict__ o, int lane, int H, int hpad, int vec) {
#pragma clang fp contract(off)
    const int nch = hpad / 4;
    if (!src) {
        for (int c = lane; c < nch; c += 64) o[c] = f16x4{0, 0, 0, 0};
        return;
    }
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

}  // namespace dinov2
