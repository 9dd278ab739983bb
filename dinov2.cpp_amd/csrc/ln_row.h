// ln_row.h -- the LayerNorm of ONE row held in the registers of one wave: the routine behind layernorm_kernel and the layer tap kernels
// (kernels_misc.hip) and behind dense_pack_kernel (dense.hip), written once so that all of them give a row the same bits.
// Rounding points, those of ggml's three graph nodes (norm, mul, add each store an f32 tensor): f32(v * scale), then f32(. * w), then
// f32(. + b).  Each piece carries its own `fp contract(off)`; all are inlined.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace dinov2 {

// Sum of a double over the 64 lanes of a wave, result in every lane.  DPP moves on the two 32-bit halves (quad swaps, half-row
// and row mirrors, then one readlane per 16-lane row) instead of six ds_bpermute round trips through the LDS pipe: the
// LayerNorm is two such reductions per row, and at batch 1 their latency was a third of the kernel.
static __device__ __forceinline__ double wave_sum_f64(double v) {
    auto dpp = [](double x, auto ctrl) {
        constexpr int C = decltype(ctrl)::value;
        const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
        const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)u, C, 0xF, 0xF, false);
        const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)(u >> 32), C, 0xF, 0xF, false);
        return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
    v += dpp(v, std::integral_constant<int, 0x141>{});  // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>{});  // row_mirror: every lane of a 16-lane row holds the row's sum
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, 16 * i), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), 16 * i);
        r[i] = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
    }
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// ln_row_load brings the row and the affine parameters into registers, ln_row_scale centres it in place and returns 1/sqrt(var + eps),
// LN_ROW_AFFINE is the three-rounding affine of one float4.
template <int MAXV>
static __device__ __forceinline__ void ln_row_load(const float4* __restrict__ xr, const float* __restrict__ w, const float* __restrict__ bta,
                                                   int nv, int lane, float4 (&v)[MAXV], float4 (&gw)[MAXV], float4 (&gb)[MAXV]) {
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {  // all loads of the row first: x, and the affine parameters needed only at the end
        const int i = lane + 64 * j;
        if (i < nv) {
            v[j] = xr[i];
            gw[j] = ((const float4*)w)[i];
            gb[j] = ((const float4*)bta)[i];
        }
    }
}

template <int MAXV>
static __device__ __forceinline__ float ln_row_scale(float4 (&v)[MAXV], int nv, int H, float eps, int lane) {
#pragma clang fp contract(off)  // ggml's rounding points (header above)
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int i = lane + 64 * j;
        if (i < nv) sum += (double)v[j].x + (double)v[j].y + (double)v[j].z + (double)v[j].w;
    }
    sum = wave_sum_f64(sum);
    const float mean = (float)(sum / H);
    double sq = 0.0;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int i = lane + 64 * j;
        if (i < nv) {
            v[j].x -= mean; v[j].y -= mean; v[j].z -= mean; v[j].w -= mean;
            sq += (double)(v[j].x * v[j].x) + (double)(v[j].y * v[j].y) + (double)(v[j].z * v[j].z) +
                  (double)(v[j].w * v[j].w);
        }
    }
    sq = wave_sum_f64(sq);
    const float var = (float)(sq / H);
    return 1.0f / sqrtf(var + eps);
}

// (a macro, not a function: through a function's arguments hipcc commutes the operands of the multiplies and adds -- the same bits, but not
// the instruction stream layernorm_kernel had.)  Assigns the four floats the CALLER declares; introduces no name of its own.
#define LN_ROW_AFFINE(r0, r1, r2, r3, c, scale, ww, bb)                                                             \
    do {                                                                                                             \
        r0 = (c).x * (scale) * (ww).x + (bb).x; r1 = (c).y * (scale) * (ww).y + (bb).y;                              \
        r2 = (c).z * (scale) * (ww).z + (bb).z; r3 = (c).w * (scale) * (ww).w + (bb).w;                              \
        /* f32 result first, f16 rounding second (ggml rounds at the NEXT mul_mat): block v_fma_mix*_f16 fusion */ \
        asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));                                                   \
    } while (0)

// one wave: row `xr` (H floats, nv = H / 4) into v, normalised (the bits of launch_layernorm_f32) or as it is
template <int MAXV, bool NORM>
static __device__ __forceinline__ void tap_row_to_registers(const float4* __restrict__ xr, const float* __restrict__ w,
                                                            const float* __restrict__ bta, int nv, int H, float eps, int lane,
                                                            float4 (&v)[MAXV]) {
#pragma clang fp contract(off)  // ggml's rounding points, as in layernorm_kernel
    if constexpr (NORM) {
        float4 gw[MAXV], gb[MAXV];
        ln_row_load<MAXV>(xr, w, bta, nv, lane, v, gw, gb);
        const float scale = ln_row_scale<MAXV>(v, nv, H, eps, lane);
#pragma unroll
        for (int j = 0; j < MAXV; ++j) {
            if (lane + 64 * j < nv) {
                const float4 ww = gw[j], bb = gb[j];
                float r0, r1, r2, r3;
                LN_ROW_AFFINE(r0, r1, r2, r3, v[j], scale, ww, bb);
                v[j] = make_float4(r0, r1, r2, r3);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < MAXV; ++j) {  // (every element defined: a partly written array does not stay in registers)
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane + 64 * j < nv) v[j] = xr[lane + 64 * j];
        }
    }
}

}  // namespace dinov2
