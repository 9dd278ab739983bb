// Attention rows (dinov2_hip_predict_attention): the softmax probabilities of chosen query tokens, per image and head, computed from the
// token-major qkv buffer the QKV GEMM of a block has just written.  A separate small kernel: the attention kernels of the forward
// (attention.hip) are not involved and keep their probabilities in registers.
//
//   out[b][h][i][j - key0] = exp2(s_ij - m_i) / sum_{j' in [0, T)} exp2(s_ij' - m_i),   key0 <= j < key0 + nkeys
//   s_ij = sum_d q[queries[i]][d] k[j][d],   m_i = max_j s_ij
//
// q is already scaled by 0.125 log2(e) (the QKV epilogue), so the weights are powers of two of the scores.  The softmax always runs over
// all T keys; key0 / nkeys only select the columns that are written (a patch-only view is the same bits, not re-normalised).
//
// NUMERICS CONTRACT
//   * The stored T-typed (f16 | bf16) q and k are the operands.  A product of two f16 or two bf16 values is exact in f32, so fmaf(q, k, acc)
//     is "acc + q k" with ONE rounding, that of the sum.
//   * Scores, maximum, exponentials (exp2f), sum, reciprocal and quotient (p * (1 / l)) are f32.
//   * The summation orders are fixed and depend on nothing but T:
//       score:        8 slices of 8 consecutive d; inside a slice ascending d from 0; the 8 slice sums by the pairwise tree
//                     ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))
//       denominator:  256 slots; slot t sums p_j over j = t, t + 256, t + 512, ... in ascending order starting from 0; the 256 slot sums by the
//                     pairwise tree over neighbouring slots (1, 2, 4, ... 128 apart)
//     They do not depend on B, on nq, on which other queries were asked for, on key0 / nkeys, or on which of the instantiations below ran:
//     a row is bit-identical whether it is requested alone, with every other token, in a batch of 1 or of 32, or in a split batch.
//   * These are NOT claimed to be the bits of the P the flash-style kernel feeds its PV product: that P is un-normalised, rounded to T and
//     carries a deferred maximum.  They are the softmax of the same stored q and k, in f32.
//
// SHAPE.  One workgroup of 256 lanes per (image, head, block of QB queries).  A K row of one head is 128 contiguous bytes: 8 lanes read it with
// one 16-byte load each, so a wave covers 8 keys per load and the workgroup 32; four loads are in flight per lane.  Every lane keeps its
// 8-element slice of the QB queries in registers, so a block of queries shares the K reads.  The T scores of a query stay in LDS (QB T floats)
// between the three phases (scores + max, exponentials + sum, scaled store).  QB = 8 while 8 T floats fit the default 64 KiB (T <= 2 048),
// QB = 1 up to the device's LDS; past that the two-pass form, which keeps no scores and computes them again for the sum and for the store
// (same arithmetic, same orders, same bits).
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "kernels.h"

namespace dinov2 {

namespace {

constexpr int AR_THREADS = 256;
constexpr int AR_KEYS = 32;    // keys per workgroup per load: 4 waves x 8 keys
constexpr int AR_UNROLL = 4;   // loads in flight per lane
constexpr size_t AR_LDS_DEFAULT = 64 * 1024;
constexpr size_t AR_LDS_MAX = 160 * 1024 - 4096;  // dynamic part; the static reduction arrays and some slack stay out of it

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
    const typename Elem<T>::vec8 v = *reinterpret_cast<const typename Elem<T>::vec8*>(p);
#pragma unroll
    for (int d = 0; d < 8; ++d) f[d] = Elem<T>::to_f32(v[d]);
}

// the score of one key from the 8 lanes that hold its slices: every one of the 8 lanes ends up with the same bits
__device__ __forceinline__ float slice_dot(const float (&q)[8], const float (&k)[8]) {
    float acc = 0.0f;
#pragma unroll
    for (int d = 0; d < 8; ++d) acc = __builtin_fmaf(q[d], k[d], acc);
    acc += dpp_f32<0xB1>(acc);   // quad_perm [1, 0, 3, 2]: slices (0 + 1), (2 + 3), ...
    acc += dpp_f32<0x4E>(acc);   // quad_perm [2, 3, 0, 1]: (0 + 1) + (2 + 3), (4 + 5) + (6 + 7)
    acc += dpp_f32<0x141>(acc);  // row_half_mirror: the other quad of the 8 lanes
    return acc;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// pairwise tree over the 64 lanes, neighbours first; every lane gets the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// QB queries of one (image, head).  KEEP: the scores stay in LDS (QB * T floats of dynamic LDS); otherwise nothing is kept and the scores are
// computed three times (QB == 1 only).
template <typename T, int QB, bool KEEP>
__global__ __launch_bounds__(AR_THREADS) void attn_rows_kernel(const T* __restrict__ qkv, int ld, float* __restrict__ out, int Tn, int H, int nh,
                                                               const int32_t* __restrict__ queries, int nq, int key0, int nkeys) {
#pragma clang fp contract(off)
    static_assert(KEEP || QB == 1, "the two-pass form takes one query");
    extern __shared__ __attribute__((aligned(16))) char attn_rows_lds[];
    float* sc = reinterpret_cast<float*>(attn_rows_lds);  // [QB][Tn] when KEEP
    __shared__ float red[QB][4];
    __shared__ float slots[KEEP ? 1 : AR_THREADS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = lane & 7, g = lane >> 3;  // slice of the head dimension, key within the wave's 8
    const int q0 = blockIdx.x * QB, h = blockIdx.y, b = blockIdx.z;
    const T* base = qkv + (size_t)b * Tn * ld + (size_t)h * 64 + e * 8;
    const T* kbase = base + H;

    float qf[QB][8];
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        const int qi = q0 + i < nq ? q0 + i : nq - 1;  // (a ragged last block computes its last query again and stores it once)
        load8<T>(base + (size_t)queries[qi] * ld, qf[i]);
    }

    const int nsteps = (Tn + AR_KEYS * AR_UNROLL - 1) / (AR_KEYS * AR_UNROLL);
    // ---- phase 1: scores (kept or not) and their maximum
    float mx[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) mx[i] = -INFINITY;
    for (int st = 0; st < nsteps; ++st) {
        float kf[AR_UNROLL][8];
#pragma unroll
        for (int u = 0; u < AR_UNROLL; ++u) {
            const int j = (st * AR_UNROLL + u) * AR_KEYS + wave * 8 + g;
            load8<T>(kbase + (size_t)(j < Tn ? j : Tn - 1) * ld, kf[u]);
        }
#pragma unroll
        for (int u = 0; u < AR_UNROLL; ++u) {
            const int j = (st * AR_UNROLL + u) * AR_KEYS + wave * 8 + g;
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                const float s = slice_dot(qf[i], kf[u]);
                if (j < Tn) {
                    mx[i] = fmaxf(mx[i], s);
                    if (KEEP && e == (i & 7)) sc[(size_t)i * Tn + j] = s;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        const float m = wave_max(mx[i]);
        if (lane == 0) red[i][wave] = m;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < QB; ++i) mx[i] = fmaxf(fmaxf(red[i][0], red[i][1]), fmaxf(red[i][2], red[i][3]));
    __syncthreads();

    // ---- phase 2: exponentials and the denominator.  Slot t (of 256) owns the keys j = t (mod 256), in ascending order.
    float part[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) part[i] = 0.0f;
    if (KEEP) {
        for (int j = tid; j < Tn; j += AR_THREADS) {
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                const float p = exp2f(sc[(size_t)i * Tn + j] - mx[i]);
                sc[(size_t)i * Tn + j] = p;
                part[i] += p;
            }
        }
    } else {
        // key j sits in the 8 lanes (wave, g) at load j / 32; the lane with e == (j / 32) % 8 adds it, so its sum is that of slot
        // ((j / 32) % 8) * 32 + wave * 8 + g = j % 256, in ascending j
        for (int st = 0; st < nsteps; ++st) {
            float kf[AR_UNROLL][8];
#pragma unroll
            for (int u = 0; u < AR_UNROLL; ++u) {
                const int j = (st * AR_UNROLL + u) * AR_KEYS + wave * 8 + g;
                load8<T>(kbase + (size_t)(j < Tn ? j : Tn - 1) * ld, kf[u]);
            }
#pragma unroll
            for (int u = 0; u < AR_UNROLL; ++u) {
                const int ld_i = st * AR_UNROLL + u, j = ld_i * AR_KEYS + wave * 8 + g;
                const float s = slice_dot(qf[0], kf[u]);
                if (j < Tn && e == (ld_i & 7)) part[0] += exp2f(s - mx[0]);
            }
        }
        slots[e * 32 + wave * 8 + g] = part[0];
        __syncthreads();
        part[0] = slots[tid];
    }
    float inv[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        const float w = wave_sum(part[i]);
        if (lane == 0) red[i][wave] = w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < QB; ++i) inv[i] = 1.0f / ((red[i][0] + red[i][1]) + (red[i][2] + red[i][3]));

    // ---- phase 3: the requested columns
    float* orow = out + (((size_t)b * nh + h) * nq + q0) * (size_t)nkeys;
    if (KEEP) {
        for (int c = tid; c < nkeys; c += AR_THREADS) {
#pragma unroll
            for (int i = 0; i < QB; ++i)
                if (q0 + i < nq) orow[(size_t)i * nkeys + c] = sc[(size_t)i * Tn + key0 + c] * inv[i];
        }
    } else {
        for (int st = 0; st < nsteps; ++st) {
            float kf[AR_UNROLL][8];
#pragma unroll
            for (int u = 0; u < AR_UNROLL; ++u) {
                const int j = (st * AR_UNROLL + u) * AR_KEYS + wave * 8 + g;
                load8<T>(kbase + (size_t)(j < Tn ? j : Tn - 1) * ld, kf[u]);
            }
#pragma unroll
            for (int u = 0; u < AR_UNROLL; ++u) {
                const int j = (st * AR_UNROLL + u) * AR_KEYS + wave * 8 + g;
                const float s = slice_dot(qf[0], kf[u]);
                if (e == 0 && j >= key0 && j < key0 + nkeys && j < Tn) orow[j - key0] = exp2f(s - mx[0]) * inv[0];
            }
        }
    }
}

template <typename T, int QB, bool KEEP>
hipError_t launch_one(const void* qkv, int ld, float* out, int B, int Tn, int H, int nh, const int32_t* queries, int nq, int key0, int nkeys,
                      hipStream_t stream) {
    const size_t lds = KEEP ? sizeof(float) * QB * (size_t)Tn : 0;
    auto kern = attn_rows_kernel<T, QB, KEEP>;
    if (lds > AR_LDS_DEFAULT) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((nq + QB - 1) / QB), (unsigned)nh, (unsigned)B);
    hipLaunchKernelGGL(kern, grid, dim3(AR_THREADS), lds, stream, static_cast<const T*>(qkv), ld, out, Tn, H, nh, queries, nq, key0, nkeys);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_typed(const void* qkv, int ld, float* out, int B, int Tn, int H, int nh, const int32_t* queries, int nq, int key0, int nkeys,
                        size_t lds_budget, hipStream_t stream) {
    const size_t row = sizeof(float) * (size_t)Tn;
    if (nq >= 8 && 8 * row <= (lds_budget < AR_LDS_DEFAULT ? lds_budget : AR_LDS_DEFAULT))
        return launch_one<T, 8, true>(qkv, ld, out, B, Tn, H, nh, queries, nq, key0, nkeys, stream);
    if (row <= lds_budget) return launch_one<T, 1, true>(qkv, ld, out, B, Tn, H, nh, queries, nq, key0, nkeys, stream);
    return launch_one<T, 1, false>(qkv, ld, out, B, Tn, H, nh, queries, nq, key0, nkeys, stream);
}

}  // namespace

hipError_t launch_attn_rows_budget(DType dt, const void* qkv, int ld, float* out, int B, int T, int H, int nh, const int32_t* queries, int nq,
                                   int key0, int nkeys, size_t lds_budget, hipStream_t stream) {
    // (16-byte loads: every q / k slice starts at a multiple of 8 elements of a 16-byte aligned buffer)
    if (!qkv || !out || !queries || B < 1 || T < 1 || nh < 1 || H != nh * 64 || ld < 2 * H || (ld & 7) || nq < 1 || nq > T || key0 < 0 ||
        nkeys < 1 || key0 > T - nkeys || B > 65535 || nh > 65535 || (reinterpret_cast<uintptr_t>(qkv) & 15))
        return hipErrorInvalidValue;
    if (lds_budget > AR_LDS_MAX) lds_budget = AR_LDS_MAX;
    return dt == DT_BF16 ? launch_typed<__bf16>(qkv, ld, out, B, T, H, nh, queries, nq, key0, nkeys, lds_budget, stream)
                         : launch_typed<_Float16>(qkv, ld, out, B, T, H, nh, queries, nq, key0, nkeys, lds_budget, stream);
}

hipError_t launch_attn_rows(DType dt, const void* qkv, int ld, float* out, int B, int T, int H, int nh, const int32_t* queries, int nq, int key0,
                            int nkeys, hipStream_t stream) {
    return launch_attn_rows_budget(dt, qkv, ld, out, B, T, H, nh, queries, nq, key0, nkeys, AR_LDS_MAX, stream);
}

}  // namespace dinov2
