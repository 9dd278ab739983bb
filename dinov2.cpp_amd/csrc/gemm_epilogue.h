// gemm_epilogue.h -- the epilogue ARITHMETIC of the three GEMM kernel files (gemm.hip, gemm2.hip, gemm4.hip), written once.
//
// The planner may cut one logical output across any of the three kernels, and B images must give the bits of B independent forwards: every
// kernel has to turn an accumulator into an output element with the same operations, in the same order, rounded at the same points.  So
// each expression lives here and the kernels call it.  The helpers are value in / value out: they do not load, store, index accumulators
// or know tile shapes.  Device code only.  Two rules hold for all of them:
//   * `#pragma clang fp contract(off)`: no implicit mul + add -> fma contraction.  The unrolled epilogue instances would otherwise be
//     contracted differently, and an element's last f32 bit (after an f16 rounding, occasionally its value) would depend on WHERE its row
//     sits in a tile.  Where the contract wants a fused multiply-add (the LN fold) it is written as one.
//   * `asm("" : "+v"(x))` makes x a real f32 register value at that point.  hipcc otherwise fuses "f32 operation, then round to f16" into
//     v_fma_mixlo_f16 for SOME unrolled instances (one rounding instead of the reference's f32-then-f16 double rounding): the same effect.
// The packed (f32x2) forms run as v_pk_*_f32; their IEEE results are those of the scalar operations, so both forms agree bit for bit.
// Where one expression has two forms or shapes below, each is the one that keeps its callers' instruction streams as they were
// (profiles/gemm_epilogue_single_source.md).
#pragma once
#include "device_types.h"

namespace dinov2 {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
#define DINO_EPI static __device__ __forceinline__

// ---- the per-column term, V = float or f32x2, each pinned (a rounding to the element type follows) and `_raw` (operands that only feed
// further f32 arithmetic: nothing can be fused there, and the kernels never pinned them).  Plain: acc + bias, a real f32 sum
template <class V> DINO_EPI V epi_bias_raw(V acc, V bias) {
#pragma clang fp contract(off)
    return acc + bias;
}
template <class V> DINO_EPI V epi_bias(V acc, V bias) {
    V v = epi_bias_raw(acc, bias);
    asm("" : "+v"(v));
    return v;
}
// LN consumers (LN fold, kernels.h): r (acc - mean s[n]) + c[n] as two fused multiply-adds, fma(r, acc, fma(n, s[n], c[n])) with the row's
// r = 1 / sqrt(var + eps), n = -mean r and the column's s[n], c[n] (c contains the bias)
template <class V> DINO_EPI V epi_ln_raw(float r, float n, V acc, V s, V c) {
#pragma clang fp contract(off)
    const V d = __builtin_elementwise_fma((V)n, s, c);
    return __builtin_elementwise_fma((V)r, acc, d);
}
template <class V> DINO_EPI V epi_ln(float r, float n, V acc, V s, V c) {
    V v = epi_ln_raw(r, n, acc, s, c);
    asm("" : "+v"(v));
    return v;
}

// ---- GELU.  ggml semantics (ggml_gelu is an f16 lookup table): y = table[f16(x)], table[h] = f16(gelu_tanh(f32(h))).  0.5 x (1 + tanh u)
// == x / (1 + exp(-2 u)) with u = sqrt(2 / pi) x (1 + 0.044715 x^2), so -2 log2(e) u = x (GELU_C1 x^2 + GELU_C2) goes straight into
// v_exp_f32 (2^t).  The reference's x <= -10 -> 0 and x >= 10 -> x branches fall out of the formula after the f16 roundings (exp -> inf
// gives -0, exp -> 0 gives x), so no compares are needed.  A token must get the same bits from either form, whatever kernel and batch it
// arrives in.  Both return the table entry (an f16 value) as f32, for E::from_f32.
constexpr float GELU_C1 = -0.1029432397f;  // -2 log2(e) sqrt(2 / pi) 0.044715
constexpr float GELU_C2 = -2.302208199f;   // -2 log2(e) sqrt(2 / pi)
#if defined(DINO_PREC) && (DINO_PREC & 4)
// (tuning builds, profiles/r05_parity_attribution.md: the table entry from a double-precision tanh instead of v_exp_f32 / v_rcp_f32)
DINO_EPI float gelu_exact(float xr) {
    const double xd = (double)xr;
    return xd <= -10.0 ? 0.0f : xd >= 10.0 ? xr : (float)(0.5 * xd * (1.0 + tanh(0.79788456080286535587989211986876 * xd * (1.0 + 0.044715 * xd * xd))));
}
#endif
// two columns per instruction: x^2, the cubic, 1 + 2^t and the final product as v_pk_*_f32; v_exp / v_rcp per element, the f16 conversions
// as vector converts (one v_cvt_pk_f16_f32 + v_cvt_f32_f16 / its SDWA form instead of four scalar converts)
DINO_EPI f32x2 epi_gelu(f32x2 v) {
#pragma clang fp contract(off)
    const f32x2 xr = __builtin_convertvector(__builtin_convertvector(v, f16x2), f32x2);
    const f32x2 c1 = {GELU_C1, GELU_C1}, c2 = {GELU_C2, GELU_C2};
    const f32x2 t = xr * __builtin_elementwise_fma(xr * xr, c1, c2);  // -2 log2(e) u
    const f32x2 den = f32x2{1.0f, 1.0f} + f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
    f32x2 gl = xr * f32x2{__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
#if defined(DINO_PREC) && (DINO_PREC & 4)
    gl = f32x2{gelu_exact(xr[0]), gelu_exact(xr[1])};
#endif
    asm("" : "+v"(gl));
    return f32x2{(float)(_Float16)gl[0], (float)(_Float16)gl[1]};
}
// one column: the small-tile kernel's edge-guarded path only
DINO_EPI float epi_gelu(float v) {
#pragma clang fp contract(off)
    const float xr = (float)(_Float16)v;
    const float t = xr * __builtin_fmaf(xr * xr, GELU_C1, GELU_C2);  // -2 log2(e) u
    float g = xr * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
#if defined(DINO_PREC) && (DINO_PREC & 4)
    g = gelu_exact(xr);
#endif
    asm("" : "+v"(g));
    return (float)(_Float16)g;
}

// ---- QKV: the softmax scale on the q columns (qs = 1 elsewhere): f32 product first, then the rounding to the element type
DINO_EPI float epi_qkv_f32(float v, float qs) {
#pragma clang fp contract(off)
    float vq = v * qs;
    asm("" : "+v"(vq));
    return vq;
}
template <class E> DINO_EPI auto epi_qkv(float v, float qs) { return E::from_f32(epi_qkv_f32(v, qs)); }

// ---- SwiGLU: silu(x1) * x2 (the reference's dinov2.cpp:605), h1 / h2 = the per-column terms of the paired columns
DINO_EPI float epi_swiglu(float h1, float h2) {
#pragma clang fp contract(off)
    float sg = h1 * __builtin_amdgcn_rcpf(1.0f + __expf(-h1)) * h2;
    asm("" : "+v"(sg));
    return sg;
}

// ---- residual: x += ls (acc + bias) in two steps -- the LayerScale product of the per-column term (what gemm2.hip / gemm4.hip transpose
// through LDS) and the add to the residual stream's row -- three separately rounded f32 operations.  Scalar, and on the shapes gemm2.hip /
// gemm4.hip hold a lane's four consecutive columns in (per element: as whole-vector operations they compile to a different order).
DINO_EPI float epi_layerscale(float biased, float ls) {
#pragma clang fp contract(off)
    return biased * ls;
}
DINO_EPI float4 epi_layerscale(f32x4 acc, float4 bias, float4 ls) {
    return make_float4(epi_layerscale(epi_bias_raw(acc[0], bias.x), ls.x), epi_layerscale(epi_bias_raw(acc[1], bias.y), ls.y),
                       epi_layerscale(epi_bias_raw(acc[2], bias.z), ls.z), epi_layerscale(epi_bias_raw(acc[3], bias.w), ls.w));
}
DINO_EPI float epi_residual(float scaled, float x) {
#pragma clang fp contract(off)
    return scaled + x;
}
DINO_EPI float4 epi_residual(float4 scaled, float4 x) {
    return make_float4(epi_residual(scaled.x, x.x), epi_residual(scaled.y, x.y), epi_residual(scaled.z, x.z), epi_residual(scaled.w, x.w));
}

// ---- LN producers (EPI_RESID_LN): the next GEMM's operand xg = T(x gamma): f32 product first, then the rounding (as everywhere).  One
// column (gemm.hip), and a lane's four consecutive columns pinned in ONE statement (gemm4.hip); the same bits.
template <class E> DINO_EPI auto epi_xg(float x, float gamma) {
#pragma clang fp contract(off)
    float g = x * gamma;
    asm("" : "+v"(g));
    return E::from_f32(g);
}
template <class E> DINO_EPI typename E::vec4 epi_xg(float4 x, float4 gamma) {
#pragma clang fp contract(off)
    float g0 = x.x * gamma.x, g1 = x.y * gamma.y, g2 = x.z * gamma.z, g3 = x.w * gamma.w;
    asm("" : "+v"(g0), "+v"(g1), "+v"(g2), "+v"(g3));
    return typename E::vec4{E::from_f32(g0), E::from_f32(g1), E::from_f32(g2), E::from_f32(g3)};
}

// ---- 16-byte store of the 2-byte epilogues: NON-TEMPORAL when the launcher says so (GemmArgs::nt_out, decided and measured in gemm.hip,
// stamp_args: outputs larger than the chip's L2s would only push the operand panels out of them).  (A macro: behind a function's pointer
// argument the call sites' address arithmetic is canonicalised before inlining and compiles to a different instruction order.)
#define DINO_EPI_ST16(PTR, V, NT) { if (NT) __builtin_nontemporal_store((V), (PTR)); else *(PTR) = (V); }

}  // namespace dinov2
