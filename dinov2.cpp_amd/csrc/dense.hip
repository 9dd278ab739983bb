// dense.hip -- linear dense-prediction heads on the patch tokens (dinov2_hip_predict_dense, include/dinov2_hip.h) for gfx950 (MI355X).
//
// No reference counterpart: semantic segmentation and depth with a linear head on frozen features (upstream DINOv2: BNHead of
// dinov2/eval/segmentation/models/decode_heads/linear_head.py and of dinov2/eval/depth/models/decode_heads/linear_head.py).  Two kernels
// around one plain GEMM (launch_gemm, EPI_PLAIN_F32):
//   dense_pack_kernel    one wave per patch row, at each tapped layer: the row through ln_row.h's routine (the bits of layer_tap_rows_kernel),
//                        rounded to f16 and stored 16 bytes a lane pair into its column block of the GEMM operand A [B P, K]; with concat_cls
//                        the image's CLS row behind it.  No f32 copy of the row is ever written.
//   dense_reduce_kernel  a workgroup owns a rectangle of output pixels, stages the low-resolution logit rows under it (token-major f32 [C],
//                        16-byte loads) into LDS, and every thread walks the classes of its pixels: bilinear interpolation of the four
//                        neighbouring rows, then the running argmax (ARGMAX) or the two running sums of the bins (BINS).  The full-resolution
//                        logit planes never exist.
// Everything the contract fixes bit for bit is written as separate f32 operations under `fp contract(off)`.
#include "device_types.h"
#include "kernels.h"
#include "ln_row.h"

namespace dinov2 {

namespace {

__device__ __forceinline__ unsigned pack_f16x2(float a, float b) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 p;
    p[0] = (_Float16)a;
    p[1] = (_Float16)b;
    return __builtin_bit_cast(unsigned, p);
}

// one wave: the row in v (float4 number lane + 64 j = columns 4 (lane + 64 j) ..) as f16 to dst; even lanes store their own four values and the
// next lane's, 16 bytes (nv is even: H % 8 == 0)
template <int MAXV>
__device__ __forceinline__ void store_row_f16(const float4 (&v)[MAXV], int nv, int lane, _Float16* __restrict__ dst) {
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const unsigned lo = pack_f16x2(v[j].x, v[j].y), hi = pack_f16x2(v[j].z, v[j].w);
        const unsigned nlo = __shfl_down(lo, 1), nhi = __shfl_down(hi, 1);  // (every lane takes part, whatever nv)
        const int i = lane + 64 * j;
        if (!(lane & 1) && i < nv) *(u32x4*)(dst + 4 * i) = u32x4{lo, hi, nlo, nhi};
    }
}

}  // namespace

template <int MAXV, bool NORM>
__global__ __launch_bounds__(256) void dense_pack_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bta,
                                                         _Float16* __restrict__ A, size_t lda, int col0, int B, int T, int R, int H, float eps,
                                                         int concat_cls) {
    const int lane = threadIdx.x & 63;
    const int P = T - 1 - R;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * P) return;
    const long long b = row / P;
    const int p = (int)(row - b * P);
    const int nv = H >> 2;
    _Float16* const dst = A + (size_t)row * lda + col0;
    float4 v[MAXV];
    tap_row_to_registers<MAXV, NORM>((const float4*)(x + (b * T + 1 + R + p) * H), w, bta, nv, H, eps, lane, v);
    store_row_f16<MAXV>(v, nv, lane, dst);
    if (concat_cls) {  // (uniform)
        tap_row_to_registers<MAXV, NORM>((const float4*)(x + b * T * H), w, bta, nv, H, eps, lane, v);
        store_row_f16<MAXV>(v, nv, lane, dst + H);
    }
}

template <int MAXV>
static hipError_t pack_dispatch(const float* x, const float* w, const float* b, float eps, int B, int T, int R, int H, bool norm, bool concat_cls,
                                _Float16* A, size_t lda, int col0, hipStream_t st) {
    const long long blocks = ((long long)B * (T - 1 - R) + 3) / 4;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    if (norm) hipLaunchKernelGGL((dense_pack_kernel<MAXV, true>), grid, block, 0, st, x, w, b, A, lda, col0, B, T, R, H, eps, (int)concat_cls);
    else hipLaunchKernelGGL((dense_pack_kernel<MAXV, false>), grid, block, 0, st, x, w, b, A, lda, col0, B, T, R, H, eps, (int)concat_cls);
    return hipGetLastError();
}

hipError_t launch_dense_pack(const float* x, const float* w, const float* b, float eps, int B, int T, int R, int H, bool norm, bool concat_cls,
                             _Float16* A, size_t lda, int col0, hipStream_t st) {
    if (H % 8 != 0 || H <= 0 || H > LN_MAX_WIDTH || B <= 0 || R < 0 || T < 2 + R) return hipErrorInvalidValue;  // ln_dispatch's widths; P >= 1
    if (!x || !A || (norm && (!w || !b))) return hipErrorInvalidValue;
    if (lda % 8 != 0 || col0 < 0 || col0 % 8 != 0 || ((size_t)A & 15) != 0 || (size_t)col0 + (size_t)H * (concat_cls ? 2 : 1) > lda)
        return hipErrorInvalidValue;
    const int nv = (H / 4 + 63) / 64;
    if (nv <= 2) return pack_dispatch<2>(x, w, b, eps, B, T, R, H, norm, concat_cls, A, lda, col0, st);
    if (nv <= 4) return pack_dispatch<4>(x, w, b, eps, B, T, R, H, norm, concat_cls, A, lda, col0, st);
    return pack_dispatch<8>(x, w, b, eps, B, T, R, H, norm, concat_cls, A, lda, col0, st);
}

// Workgroup (x, y, z): output pixels [y tile_y, +tile_y) x [x tile_x, +tile_x) of image z.  Dynamic LDS: the staged rows [max_rows][pitch]
// f32, the centres [C to a multiple of 4] f32, the tile's labels [tile_y][tile_x] u8.  Pixels go to threads row-major, so a wave's lanes
// are neighbours in x: they read the same few rows at the same class (a broadcast where the row is the same), and rows r, r + 1 sit in
// different bank groups (dense_pitch).  Classes ascend: the first of equal values stays (contract 4), S and D are summed in that order
// (contract 5).
template <int REDUCE>
__global__ __launch_bounds__(256) void dense_reduce_kernel(const float* __restrict__ L, int ldl, int h0, int w0, int C, int oh, int ow, float sy,
                                                           float sx, int ty, int tx, int pitch, int max_rows, const float* __restrict__ centers,
                                                           float eps, uint8_t* __restrict__ labels, float* __restrict__ value) {
#pragma clang fp contract(off)  // contract 3 - 5: every multiplication and addition rounds on its own
    extern __shared__ __attribute__((aligned(16))) float dense_lds[];
    const int tid = threadIdx.x;
    const int C4 = (C + 3) >> 2, pitch4 = pitch >> 2;  // (rows are addressed in 16-byte units: ds_read_b128 / ds_write_b128)
    float4* const lds4 = (float4*)dense_lds;
    float* const cen = dense_lds + (size_t)max_rows * pitch;
    uint8_t* const lab = (uint8_t*)(cen + 4 * C4);
    const int y_first = blockIdx.y * ty, x_first = blockIdx.x * tx;
    const int ny_px = oh - y_first < ty ? oh - y_first : ty, nx_px = ow - x_first < tx ? ow - x_first : tx;
    int ylo, yhi, xlo, xhi, unused;
    float lam_unused;
    dense_axis(sy, y_first, h0, ylo, unused, lam_unused);
    dense_axis(sy, y_first + ny_px - 1, h0, unused, yhi, lam_unused);
    dense_axis(sx, x_first, w0, xlo, unused, lam_unused);
    dense_axis(sx, x_first + nx_px - 1, w0, unused, xhi, lam_unused);
    const int ny = yhi - ylo + 1, nx = xhi - xlo + 1;
    if (ny * nx > max_rows) return;  // (uniform; the planner's spans cover every tile)
    const float* const Lb = L + (size_t)blockIdx.z * h0 * w0 * ldl;
    for (int i = tid; i < ny * nx * C4; i += 256) {
        const int r = i / C4, q = i - r * C4;
        const int ry = r / nx, rx = r - ry * nx;
        lds4[r * pitch4 + q] = *(const float4*)(Lb + ((size_t)(ylo + ry) * w0 + xlo + rx) * ldl + 4 * q);
    }
    if (REDUCE == DENSE_BINS)
        for (int i = tid; i < C; i += 256) cen[i] = centers[i];
    __syncthreads();

    const size_t img = (size_t)blockIdx.z * oh;
    for (int px = tid; px < ty * tx; px += 256) {
        const int ly = px / tx, lx = px - ly * tx;
        if (ly >= ny_px || lx >= nx_px) continue;
        int y0, y1, x0, x1;
        float ay, ax;
        dense_axis(sy, y_first + ly, h0, y0, y1, ay);
        dense_axis(sx, x_first + lx, w0, x0, x1, ax);
        const float by = 1.0f - ay, bx = 1.0f - ax;
        const float4* const r00 = lds4 + ((y0 - ylo) * nx + (x0 - xlo)) * pitch4;
        const float4* const r01 = lds4 + ((y0 - ylo) * nx + (x1 - xlo)) * pitch4;
        const float4* const r10 = lds4 + ((y1 - ylo) * nx + (x0 - xlo)) * pitch4;
        const float4* const r11 = lds4 + ((y1 - ylo) * nx + (x1 - xlo)) * pitch4;
        float best = 0.0f, S = 0.0f, D = 0.0f;
        int bi = 0;
        auto one = [&](int cls, float v00, float v01, float v10, float v11) {
            const float t = bx * v00 + ax * v01;
            const float u = bx * v10 + ax * v11;
            const float val = by * t + ay * u;
            if (REDUCE == DENSE_ARGMAX) {
                if (cls == 0 || val > best) {  // strictly greater: equal values (-0 and +0 among them) stay with the lowest class
                    best = val;
                    bi = cls;
                }
            } else {
                const float r = (val > 0.0f ? val : 0.0f) + eps;
                S = S + r;
                D = D + r * cen[cls];
            }
        };
        const int Cfull = C >> 2;
        for (int q = 0; q < Cfull; ++q) {  // four classes per 16-byte read of each neighbour row
            const float4 a = r00[q], b = r01[q], c = r10[q], d = r11[q];
            one(4 * q, a.x, b.x, c.x, d.x);
            one(4 * q + 1, a.y, b.y, c.y, d.y);
            one(4 * q + 2, a.z, b.z, c.z, d.z);
            one(4 * q + 3, a.w, b.w, c.w, d.w);
        }
        if (C & 3) {  // (uniform) the last one to three classes; what lies behind them in the row is never looked at
            const float4 a = r00[Cfull], b = r01[Cfull], c = r10[Cfull], d = r11[Cfull];
            one(4 * Cfull, a.x, b.x, c.x, d.x);
            if ((C & 3) > 1) one(4 * Cfull + 1, a.y, b.y, c.y, d.y);
            if ((C & 3) > 2) one(4 * Cfull + 2, a.z, b.z, c.z, d.z);
        }
        const size_t o = (img + y_first + ly) * ow + x_first + lx;
        if (REDUCE == DENSE_ARGMAX) {
            lab[px] = (uint8_t)bi;
            if (value) value[o] = best;
        } else {
            value[o] = D / S;
        }
    }
    if (REDUCE != DENSE_ARGMAX || !labels) return;  // (uniform)
    __syncthreads();
    // the tile's labels: every row's run of nx_px bytes leaves as aligned 32-bit words; the words that straddle its ends as single bytes
    const int words = (tx + 3) / 4 + 1;
    for (int i = tid; i < ny_px * words; i += 256) {
        const int ly = i / words, wi = i - ly * words;
        uint8_t* const g = labels + (img + y_first + ly) * ow + x_first;
        const int off = 4 * wi - (int)((uintptr_t)g & 3);  // of the word's first byte within the run: -3 .. nx_px + 3
        uint8_t* const wa = g + off;
        if (off >= 0 && off + 3 < nx_px) {
            const uint8_t* const s = lab + ly * tx + off;
            *(unsigned*)wa = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
        } else {
            for (int k = 0; k < 4; ++k)
                if (off + k >= 0 && off + k < nx_px) wa[k] = lab[ly * tx + off + k];
        }
    }
}

hipError_t launch_dense_reduce(const float* logits, int ldl, int B, int h0, int w0, int C, int out_h, int out_w, int reduce, const float* centers,
                               float eps, uint8_t* labels, float* value, const DenseReducePlan& p, hipStream_t st) {
    if (!logits || B < 1 || B > 65535 || ldl < C || ldl % 4 != 0 || ((size_t)logits & 15) != 0) return hipErrorInvalidValue;
    if (reduce != DENSE_ARGMAX && reduce != DENSE_BINS) return hipErrorInvalidValue;
    if (reduce == DENSE_BINS && (!centers || !value || labels || !(eps > 0.0f))) return hipErrorInvalidValue;
    if (reduce == DENSE_ARGMAX && !labels && !value) return hipErrorInvalidValue;
    const DenseReducePlan q = dense_reduce_plan(h0, w0, C, out_h, out_w);  // (the caller's plan must be THIS problem's: the kernel trusts its spans)
    if (q.tile_y == 0 || q.tile_y != p.tile_y || q.tile_x != p.tile_x || q.span_y != p.span_y || q.span_x != p.span_x || q.pitch != p.pitch ||
        q.lds_bytes != p.lds_bytes || p.lds_bytes > DENSE_LDS_BUDGET)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p.grid_x, (unsigned)p.grid_y, (unsigned)B), block(256);
    const int max_rows = p.span_y * p.span_x;
    if (reduce == DENSE_ARGMAX)
        hipLaunchKernelGGL(dense_reduce_kernel<DENSE_ARGMAX>, grid, block, p.lds_bytes, st, logits, ldl, h0, w0, C, out_h, out_w, p.scale_y, p.scale_x,
                           p.tile_y, p.tile_x, p.pitch, max_rows, centers, eps, labels, value);
    else
        hipLaunchKernelGGL(dense_reduce_kernel<DENSE_BINS>, grid, block, p.lds_bytes, st, logits, ldl, h0, w0, C, out_h, out_w, p.scale_y, p.scale_x,
                           p.tile_y, p.tile_x, p.pitch, max_rows, centers, eps, labels, value);
    return hipGetLastError();
}

}  // namespace dinov2
