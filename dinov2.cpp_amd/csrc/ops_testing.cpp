// Diagnostic entry points (include/dinov2_hip_ops.h): run ONE kernel on host-provided f32 data so that the parity
// tests can check each hand-written kernel against the oracle / numpy in isolation.  Not used by predict.
#include <chrono>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dinov2_hip.h"
#include "../../include/dinov2_hip_ops.h"
#include "device_types.h"
#include "kernels.h"

using namespace dinov2;

namespace {

template <typename T>
std::vector<T> to_t(const float* src, size_t n) {
    std::vector<T> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (T)src[i];
    return v;
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 16); }
};

#define OP_TRY(x)                          \
    do {                                   \
        if ((x) != hipSuccess) return -1;  \
    } while (0)

hipError_t upload_as(DType dt, const float* src, size_t n, DevBuf& d) {
    hipError_t e = d.alloc(n * 2);
    if (e != hipSuccess) return e;
    if (dt == DT_F16) {
        auto v = to_t<_Float16>(src, n);
        return hipMemcpy(d.p, v.data(), n * 2, hipMemcpyHostToDevice);
    }
    auto v = to_t<__bf16>(src, n);
    return hipMemcpy(d.p, v.data(), n * 2, hipMemcpyHostToDevice);
}

hipError_t download_as(DType dt, const void* dev, size_t n, float* dst) {
    std::vector<uint16_t> raw(n);
    hipError_t e = hipMemcpy(raw.data(), dev, n * 2, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t i = 0; i < n; ++i) {
        if (dt == DT_F16) {
            _Float16 h;
            std::memcpy(&h, &raw[i], 2);
            dst[i] = (float)h;
        } else {
            uint32_t u = (uint32_t)raw[i] << 16;
            std::memcpy(&dst[i], &u, 4);
        }
    }
    return hipSuccess;
}

}  // namespace

extern "C" int dinov2_hip_op_gemm(int32_t dtype, int32_t epilogue, const float* A, const float* W, const float* bias,
                                  const float* aux, int64_t aux_count, float* out, int32_t out_rows, int32_t ldo,
                                  int32_t M, int32_t N, int32_t K, int32_t P, int32_t T, int32_t R, int32_t qcols,
                                  float qscale) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    if (gemm_init() != hipSuccess) return -1;
    DevBuf dA, dW, dB, dX, dO;
    OP_TRY(upload_as(dt, A, (size_t)M * K, dA));
    OP_TRY(upload_as(dt, W, (size_t)N * K, dW));
    if (bias) {
        OP_TRY(dB.alloc(sizeof(float) * N));
        OP_TRY(hipMemcpy(dB.p, bias, sizeof(float) * N, hipMemcpyHostToDevice));
    }
    if (aux) {
        OP_TRY(dX.alloc(sizeof(float) * (size_t)aux_count));
        OP_TRY(hipMemcpy(dX.p, aux, sizeof(float) * (size_t)aux_count, hipMemcpyHostToDevice));
    }
    const bool f32out = epilogue == EPI_PATCH || epilogue == EPI_RESID || epilogue == EPI_PLAIN_F32;
    const size_t on = (size_t)out_rows * ldo;
    OP_TRY(dO.alloc(on * 4));
    if (f32out) OP_TRY(hipMemcpy(dO.p, out, on * 4, hipMemcpyHostToDevice));
    else OP_TRY(hipMemset(dO.p, 0, on * 4));
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.bias = (const float*)dB.p; a.out = dO.p; a.aux = (const float*)dX.p;
    a.M = M; a.N = N; a.K = K; a.ldo = ldo; a.P = P; a.T = T; a.R = R; a.qcols = qcols; a.qscale = qscale;
    OP_TRY(launch_gemm(dt, (Epilogue)epilogue, a, nullptr));
    OP_TRY(hipDeviceSynchronize());
    if (f32out) OP_TRY(hipMemcpy(out, dO.p, on * 4, hipMemcpyDeviceToHost));
    else OP_TRY(download_as(dt, dO.p, on, out));
    return 0;
}

// ---- LN fold (kernels.h): the producer epilogue, the consumer epilogues, the two small kernels, each alone ----
extern "C" int dinov2_hip_op_gemm_resid_ln(int32_t dtype, const float* A, const float* W, const float* bias, const float* ls, const float* gamma,
                                           float* x, float* xg, float* stats, int32_t M, int32_t N, int32_t K) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    if (gemm_init() != hipSuccess) return -1;
    const int gs = ln_stat_slots(N);
    DevBuf dA, dW, dV, dX, dG, dS;
    OP_TRY(upload_as(dt, A, (size_t)M * K, dA));
    OP_TRY(upload_as(dt, W, (size_t)N * K, dW));
    OP_TRY(dV.alloc(sizeof(float) * 3 * (size_t)N));
    float* v = (float*)dV.p;
    OP_TRY(hipMemcpy(v, bias, sizeof(float) * N, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(v + N, ls, sizeof(float) * N, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(v + 2 * N, gamma, sizeof(float) * N, hipMemcpyHostToDevice));
    OP_TRY(dX.alloc(sizeof(float) * (size_t)M * N));
    OP_TRY(hipMemcpy(dX.p, x, sizeof(float) * (size_t)M * N, hipMemcpyHostToDevice));
    OP_TRY(dG.alloc(2 * (size_t)M * N));
    OP_TRY(hipMemset(dG.p, 0, 2 * (size_t)M * N));
    OP_TRY(dS.alloc(sizeof(float) * 2 * (size_t)M * gs));
    OP_TRY(hipMemset(dS.p, 0, sizeof(float) * 2 * (size_t)M * gs));
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.bias = v; a.aux = v + N; a.ln_gamma = v + 2 * N; a.out = dX.p; a.xg = dG.p; a.stats = (float*)dS.p; a.ln_gs = gs;
    a.M = M; a.N = N; a.K = K; a.ldo = N;
    OP_TRY(launch_gemm(dt, EPI_RESID_LN, a, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(hipMemcpy(x, dX.p, sizeof(float) * (size_t)M * N, hipMemcpyDeviceToHost));
    OP_TRY(download_as(dt, dG.p, (size_t)M * N, xg));
    OP_TRY(hipMemcpy(stats, dS.p, sizeof(float) * 2 * (size_t)M * gs, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dinov2_hip_op_gemm_ln_consumer(int32_t dtype, int32_t epilogue, const float* A, const float* W, const float* ln_s, const float* ln_c,
                                              const float* stats, float eps, float* out, int32_t ldo, int32_t M, int32_t N, int32_t K,
                                              int32_t qcols, float qscale) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    if (gemm_init() != hipSuccess) return -1;
    if (!epi_ln_consumer((Epilogue)epilogue)) return -1;
    const int gs = ln_stat_slots(K);
    DevBuf dA, dW, dV, dS, dO;
    OP_TRY(upload_as(dt, A, (size_t)M * K, dA));
    OP_TRY(upload_as(dt, W, (size_t)N * K, dW));
    OP_TRY(dV.alloc(sizeof(float) * 2 * (size_t)N));
    float* v = (float*)dV.p;
    OP_TRY(hipMemcpy(v, ln_s, sizeof(float) * N, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(v + N, ln_c, sizeof(float) * N, hipMemcpyHostToDevice));
    OP_TRY(dS.alloc(sizeof(float) * 2 * (size_t)M * gs));
    OP_TRY(hipMemcpy(dS.p, stats, sizeof(float) * 2 * (size_t)M * gs, hipMemcpyHostToDevice));
    const size_t on = (size_t)M * ldo;
    OP_TRY(dO.alloc(on * 2));
    OP_TRY(hipMemset(dO.p, 0, on * 2));
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.ln_s = v; a.ln_c = v + N; a.stats = (float*)dS.p; a.ln_gs = gs; a.ln_eps = eps; a.out = dO.p;
    a.M = M; a.N = N; a.K = K; a.ldo = ldo; a.qcols = qcols; a.qscale = qscale;
    OP_TRY(launch_gemm(dt, (Epilogue)epilogue, a, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(download_as(dt, dO.p, on, out));
    return 0;
}

extern "C" int dinov2_hip_op_ln_prepare(int32_t dtype, const float* x, const float* gamma, float* xg, float* stats, int32_t rows, int32_t H) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    const int gs = ln_stat_slots(H);
    DevBuf dX, dV, dG, dS;
    OP_TRY(dX.alloc(sizeof(float) * (size_t)rows * H));
    OP_TRY(hipMemcpy(dX.p, x, sizeof(float) * (size_t)rows * H, hipMemcpyHostToDevice));
    OP_TRY(dV.alloc(sizeof(float) * (size_t)H));
    OP_TRY(hipMemcpy(dV.p, gamma, sizeof(float) * (size_t)H, hipMemcpyHostToDevice));
    OP_TRY(dG.alloc(2 * (size_t)rows * H));
    OP_TRY(dS.alloc(sizeof(float) * 2 * (size_t)rows * gs));
    OP_TRY(hipMemset(dS.p, 0, sizeof(float) * 2 * (size_t)rows * gs));
    OP_TRY(launch_ln_prepare(dt, (const float*)dX.p, (const float*)dV.p, dG.p, (float*)dS.p, gs, rows, H, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(download_as(dt, dG.p, (size_t)rows * H, xg));
    OP_TRY(hipMemcpy(stats, dS.p, sizeof(float) * 2 * (size_t)rows * gs, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dinov2_hip_op_im2col(int32_t dtype, const float* img, float* col, int32_t B, int32_t Hh, int32_t Ww, int32_t patch, int32_t Kpad,
                                    int32_t layout) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    if (B <= 0 || Hh <= 0 || Ww <= 0 || patch <= 0) return -1;
    const size_t npix = (size_t)B * 3 * Hh * Ww, rows = (size_t)B * (Hh / patch) * (Ww / patch);
    DevBuf dI, dC;
    OP_TRY(dI.alloc(sizeof(float) * npix));
    OP_TRY(hipMemcpy(dI.p, img, sizeof(float) * npix, hipMemcpyHostToDevice));
    OP_TRY(dC.alloc(2 * rows * (size_t)Kpad));
    OP_TRY(hipMemset(dC.p, 0xff, 2 * rows * (size_t)Kpad));  // (a NaN pattern: every element must be written)
    OP_TRY(launch_im2col(dt, (const float*)dI.p, dC.p, B, Hh, Ww, patch, Kpad, layout, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(download_as(dt, dC.p, rows * (size_t)Kpad, col));
    return 0;
}

extern "C" int dinov2_hip_op_ln_fold_vectors(int32_t dtype, const float* W, const float* bias, const float* gamma, const float* beta, float* s_out,
                                             float* c_out, int32_t N, int32_t K) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    DevBuf dW, dV;
    OP_TRY(upload_as(dt, W, (size_t)N * K, dW));
    OP_TRY(dV.alloc(sizeof(float) * (3 * (size_t)N + 2 * (size_t)K)));
    float* v = (float*)dV.p;
    OP_TRY(hipMemcpy(v, bias, sizeof(float) * N, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(v + 3 * (size_t)N, gamma, sizeof(float) * K, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(v + 3 * (size_t)N + K, beta, sizeof(float) * K, hipMemcpyHostToDevice));
    OP_TRY(launch_ln_fold_vectors(dt, dW.p, v, v + 3 * (size_t)N, v + 3 * (size_t)N + K, v + N, v + 2 * (size_t)N, N, K, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(hipMemcpy(s_out, v + N, sizeof(float) * N, hipMemcpyDeviceToHost));
    OP_TRY(hipMemcpy(c_out, v + 2 * (size_t)N, sizeof(float) * N, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dinov2_hip_op_attention(int32_t dtype, const float* qkv, float* out, int32_t B, int32_t T, int32_t H,
                                       int32_t nh) {
    return dinov2_hip_op_attention_ex(dtype, qkv, out, B, T, H, nh, 0);
}

extern "C" int dinov2_hip_op_attention_ex(int32_t dtype, const float* qkv, float* out, int32_t B, int32_t T, int32_t H,
                                          int32_t nh, int32_t log2_scores) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    if (B <= 0 || T <= 0 || H <= 0) return -1;
    // the output sits between two guard bands of DINOV2_HIP_OP_GUARD_ROWS rows; the whole buffer starts as 0xffff, a NaN in f16
    // and in bf16, so a row the kernel never wrote comes back as NaN and a write outside [0, B*T) rows changes a guard byte
    constexpr size_t G = DINOV2_HIP_OP_GUARD_ROWS;
    DevBuf dQ, dO;
    const size_t nq = (size_t)B * T * 3 * H, no = (size_t)B * T * H, ng = G * (size_t)H;
    const size_t nall = no + 2 * ng;
    OP_TRY(upload_as(dt, qkv, nq, dQ));
    OP_TRY(dO.alloc(nall * 2));
    OP_TRY(hipMemset(dO.p, 0xff, nall * 2));
    OP_TRY(launch_attention(dt, dQ.p, (uint16_t*)dO.p + ng, B, T, H, nh, log2_scores != 0, nullptr));
    OP_TRY(hipDeviceSynchronize());
    std::vector<uint16_t> raw(nall);
    OP_TRY(hipMemcpy(raw.data(), dO.p, nall * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nall; ++i) {
        const uint16_t h = raw[i];
        if (i < ng || i >= ng + no) {
            if (h != 0xffffu) return DINOV2_HIP_OP_GUARD_CHANGED;
            continue;
        }
        float f;
        if (dt == DT_F16) {
            _Float16 x;
            std::memcpy(&x, &h, 2);
            f = (float)x;
        } else {
            const uint32_t u = (uint32_t)h << 16;
            std::memcpy(&f, &u, 4);
        }
        out[i - ng] = f;
    }
    return 0;
}

extern "C" int dinov2_hip_op_layernorm(int32_t dtype, const float* x, const float* w, const float* b, float* out,
                                       int32_t rows, int32_t H, float eps) {
    DevBuf dX, dW, dB, dO;
    const size_t n = (size_t)rows * H;
    OP_TRY(dX.alloc(n * 4));
    OP_TRY(dW.alloc((size_t)H * 4));
    OP_TRY(dB.alloc((size_t)H * 4));
    OP_TRY(dO.alloc(n * 4));
    OP_TRY(hipMemset(dO.p, 0xff, n * 4));  // NaN in f32, f16 and bf16: an element the kernel never wrote comes back as NaN
    OP_TRY(hipMemcpy(dX.p, x, n * 4, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(dW.p, w, (size_t)H * 4, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(dB.p, b, (size_t)H * 4, hipMemcpyHostToDevice));
    if (dtype < 0) {
        OP_TRY(launch_layernorm_f32((const float*)dX.p, (const float*)dW.p, (const float*)dB.p, (float*)dO.p, rows, H, eps,
                                    nullptr));
        OP_TRY(hipDeviceSynchronize());
        OP_TRY(hipMemcpy(out, dO.p, n * 4, hipMemcpyDeviceToHost));
    } else {
        const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
        OP_TRY(launch_layernorm(dt, (const float*)dX.p, (const float*)dW.p, (const float*)dB.p, dO.p, rows, H, eps, nullptr));
        OP_TRY(hipDeviceSynchronize());
        OP_TRY(download_as(dt, dO.p, n, out));
    }
    return 0;
}

extern "C" int dinov2_hip_op_layer_tap(const float* x, const float* w, const float* b, float eps, int32_t B, int32_t T, int32_t R, int32_t H,
                                       int32_t h0, int32_t w0, int32_t norm, int32_t layout, float* patch_out, float* cls_out, float* reg_out) {
    if (B <= 0 || H <= 0 || R < 0 || h0 <= 0 || w0 <= 0 || T != 1 + R + h0 * w0 || (layout != 0 && layout != 1)) return -1;
    if (norm && (!w || !b)) return -1;
    const size_t P = (size_t)h0 * w0, n = (size_t)B * T * H, ng = (size_t)DINOV2_HIP_OP_GUARD_ROWS * H;
    // each output between two guard bands, the whole buffer 0xff bytes (NaN): an element the kernel never wrote comes back as NaN and a
    // write outside the output changes a guard
    const size_t counts[3] = {(size_t)B * P * H, (size_t)B * H, (size_t)B * R * H};
    float* const host[3] = {patch_out, cls_out, reg_out};
    DevBuf dX, dW, dB, dO[3];
    OP_TRY(dX.alloc(n * 4));
    OP_TRY(hipMemcpy(dX.p, x, n * 4, hipMemcpyHostToDevice));
    if (norm) {
        OP_TRY(dW.alloc((size_t)H * 4));
        OP_TRY(dB.alloc((size_t)H * 4));
        OP_TRY(hipMemcpy(dW.p, w, (size_t)H * 4, hipMemcpyHostToDevice));
        OP_TRY(hipMemcpy(dB.p, b, (size_t)H * 4, hipMemcpyHostToDevice));
    }
    float* dev[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; ++i) {
        if (!host[i]) continue;
        OP_TRY(dO[i].alloc((counts[i] + 2 * ng) * 4));
        OP_TRY(hipMemset(dO[i].p, 0xff, (counts[i] + 2 * ng) * 4));
        dev[i] = (float*)dO[i].p + ng;
    }
    OP_TRY(launch_layer_tap((const float*)dX.p, (const float*)dW.p, (const float*)dB.p, eps, B, T, R, H, norm != 0, layout == 1, dev[0], dev[1],
                            dev[2], nullptr));
    OP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 3; ++i) {
        if (!host[i]) continue;
        std::vector<uint32_t> raw(counts[i] + 2 * ng);
        OP_TRY(hipMemcpy(raw.data(), dO[i].p, raw.size() * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < ng; ++k)
            if (raw[k] != 0xffffffffu || raw[ng + counts[i] + k] != 0xffffffffu) return DINOV2_HIP_OP_GUARD_CHANGED;
        std::memcpy(host[i], raw.data() + ng, counts[i] * 4);
    }
    return 0;
}

extern "C" int dinov2_hip_op_attn_rows_ex(int32_t dtype, const float* qkv, int32_t B, int32_t T, int32_t H, int32_t nh, const int32_t* queries,
                                          int32_t nq, int32_t key0, int32_t nkeys, float* out, int64_t lds_budget) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    if (!qkv || !queries || !out || B <= 0 || T <= 0 || nh <= 0 || H != nh * 64 || nq < 1 || nq > T || key0 < 0 || nkeys < 1 || key0 > T - nkeys)
        return -1;
    for (int i = 0; i < nq; ++i)
        if (queries[i] < 0 || queries[i] >= T || (i > 0 && queries[i] <= queries[i - 1])) return -1;
    // the output between two guard bands, the whole buffer 0xff bytes (NaN): an element the kernel never wrote comes back as NaN and a write
    // outside the output changes a guard
    const size_t no = (size_t)B * nh * nq * nkeys, ng = (size_t)DINOV2_HIP_OP_GUARD_ROWS * nkeys;
    DevBuf dQ, dI, dO;
    OP_TRY(upload_as(dt, qkv, (size_t)B * T * 3 * H, dQ));
    OP_TRY(dI.alloc(sizeof(int32_t) * (size_t)nq));
    OP_TRY(hipMemcpy(dI.p, queries, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice));
    OP_TRY(dO.alloc((no + 2 * ng) * 4));
    OP_TRY(hipMemset(dO.p, 0xff, (no + 2 * ng) * 4));
    float* dev = (float*)dO.p + ng;
    if (lds_budget > 0)
        OP_TRY(launch_attn_rows_budget(dt, dQ.p, 3 * H, dev, B, T, H, nh, (const int32_t*)dI.p, nq, key0, nkeys, (size_t)lds_budget, nullptr));
    else
        OP_TRY(launch_attn_rows(dt, dQ.p, 3 * H, dev, B, T, H, nh, (const int32_t*)dI.p, nq, key0, nkeys, nullptr));
    OP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> raw(no + 2 * ng);
    OP_TRY(hipMemcpy(raw.data(), dO.p, raw.size() * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < ng; ++k)
        if (raw[k] != 0xffffffffu || raw[ng + no + k] != 0xffffffffu) return DINOV2_HIP_OP_GUARD_CHANGED;
    std::memcpy(out, raw.data() + ng, no * 4);
    return 0;
}

extern "C" int dinov2_hip_op_attn_rows(int32_t dtype, const float* qkv, int32_t B, int32_t T, int32_t H, int32_t nh, const int32_t* queries,
                                       int32_t nq, int32_t key0, int32_t nkeys, float* out) {
    return dinov2_hip_op_attn_rows_ex(dtype, qkv, B, T, H, nh, queries, nq, key0, nkeys, out, 0);
}

extern "C" int dinov2_hip_op_convert_weight(int32_t dtype, const void* src, uint64_t src_bytes, uint32_t ggml_type,
                                            float* out, int32_t N, int32_t K, int32_t Kpad, int32_t interleaveF) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    DevBuf dS, dO;
    OP_TRY(dS.alloc(src_bytes));
    OP_TRY(hipMemcpy(dS.p, src, src_bytes, hipMemcpyHostToDevice));
    OP_TRY(dO.alloc((size_t)N * Kpad * 2));
    OP_TRY(hipMemset(dO.p, 0xff, (size_t)N * Kpad * 2));  // NaN: an element the kernel never wrote comes back as NaN
    OP_TRY(launch_convert_weight(dt, dS.p, ggml_type, dO.p, N, K, Kpad, interleaveF, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(download_as(dt, dO.p, (size_t)N * Kpad, out));
    return 0;
}

extern "C" int dinov2_hip_op_permute_bias(const float* src, float* dst, int32_t N, int32_t interleaveF) {
    if (!src || !dst || N <= 0 || interleaveF < 0 || (interleaveF > 0 && N != 2 * interleaveF)) return -1;
    DevBuf dS, dD;
    OP_TRY(dS.alloc((size_t)N * 4));
    OP_TRY(dD.alloc((size_t)N * 4));
    OP_TRY(hipMemcpy(dS.p, src, (size_t)N * 4, hipMemcpyHostToDevice));
    OP_TRY(hipMemset(dD.p, 0xff, (size_t)N * 4));
    OP_TRY(launch_permute_bias((const float*)dS.p, (float*)dD.p, N, interleaveF, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(hipMemcpy(dst, dD.p, (size_t)N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_head as csrc/model.cpp runs it after the final LayerNorm, on host f32 data: W [C, 2H] rounded to the compute type as
// upload_as rounds it (nearest even), every output buffer NaN-filled first.
extern "C" int dinov2_hip_op_head(int32_t dtype, const float* fin, const float* W, const float* bias, float* feat, float* logits,
                                  float* probs, int32_t B, int32_t T, int32_t H, int32_t C, int32_t first, float inv_div) {
    // head_logits_kernel reads W and feat in 8-element pieces: 2H % 8 == 0
    if (!fin || !W || !bias || !feat || !logits || !probs || B <= 0 || T <= 0 || H <= 0 || H % 4 != 0 || C <= 0 || first < 0 || first > T)
        return -1;
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    DevBuf dF, dW, dB, dFeat, dL, dP;
    const size_t nf = (size_t)B * T * H, nfeat = (size_t)B * 2 * H, nl = (size_t)B * C;
    OP_TRY(dF.alloc(nf * 4));
    OP_TRY(hipMemcpy(dF.p, fin, nf * 4, hipMemcpyHostToDevice));
    OP_TRY(upload_as(dt, W, (size_t)C * 2 * H, dW));
    OP_TRY(dB.alloc((size_t)C * 4));
    OP_TRY(hipMemcpy(dB.p, bias, (size_t)C * 4, hipMemcpyHostToDevice));
    OP_TRY(dFeat.alloc(nfeat * 4));
    OP_TRY(dL.alloc(nl * 4));
    OP_TRY(dP.alloc(nl * 4));
    OP_TRY(hipMemset(dFeat.p, 0xff, nfeat * 4));
    OP_TRY(hipMemset(dL.p, 0xff, nl * 4));
    OP_TRY(hipMemset(dP.p, 0xff, nl * 4));
    OP_TRY(launch_head(dt, (const float*)dF.p, dW.p, (const float*)dB.p, (float*)dFeat.p, (float*)dL.p, (float*)dP.p, B, T, H, C, first,
                       inv_div, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(hipMemcpy(feat, dFeat.p, nfeat * 4, hipMemcpyDeviceToHost));
    OP_TRY(hipMemcpy(logits, dL.p, nl * 4, hipMemcpyDeviceToHost));
    OP_TRY(hipMemcpy(probs, dP.p, nl * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dinov2_hip_op_probe_tr16(int16_t* out256) {
    DevBuf d;
    OP_TRY(d.alloc(512));
    OP_TRY(launch_probe_tr16((int16_t*)d.p, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(hipMemcpy(out256, d.p, 512, hipMemcpyDeviceToHost));
    return 0;
}

// ---- micro-benchmarks: device-resident random operands, HIP-event timing around `iters` launches ----
namespace {
void fill_random_t(DType dt, void* dev, size_t n, unsigned seed, float scale) {
    std::vector<uint16_t> h(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        const float v = (((float)(s >> 8) / 8388608.0f) - 1.0f) * scale;  // uniform [-scale, scale): full-range random
        if (dt == DT_F16) {
            _Float16 x = (_Float16)v;
            std::memcpy(&h[i], &x, 2);
        } else {
            uint32_t u;
            std::memcpy(&u, &v, 4);
            h[i] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
    }
    (void)hipMemcpy(dev, h.data(), n * 2, hipMemcpyHostToDevice);
}
}  // namespace

extern "C" float dinov2_hip_op_gemm_bench(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t iters) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    if (gemm_init() != hipSuccess) return -1.f;
    DevBuf dA, dW, dB, dX, dO;
    // extra elements per row of A / W (row strides K + pad instead of the dense K): 0 in normal use; profiles/r02_gemm_kloop.md
    // measured 64 (= 128 bytes) as neutral, i.e. no power-of-two-stride channel conflict to pad away
    const int padA = 0, padW = 0;
    // EPI_PATCH writes token rows (image b, patch p) -> row b * T + 1 + R + p and reads the position embedding [1 + P, N]: shaped like the model
    // (P = 1369 patches, 4 registers) when M is a multiple of 1369, one "image" of M patches otherwise
    const int pP = epilogue == EPI_PATCH ? (M % 1369 == 0 ? 1369 : M) : 1, pR = epilogue == EPI_PATCH && M % 1369 == 0 ? 4 : 0;
    const int pT = pP + 1 + pR;
    const size_t out_elems = epilogue == EPI_PATCH ? (size_t)(M / pP) * pT * N : (size_t)M * N;
    const size_t aux_elems = epilogue == EPI_PATCH ? (size_t)(pP + 1) * N : (size_t)std::max(N, 4096) * 2;
    if (dA.alloc((size_t)M * (K + padA) * 2) != hipSuccess || dW.alloc((size_t)N * (K + padW) * 2) != hipSuccess ||
        dB.alloc((size_t)N * 4) != hipSuccess || dX.alloc(aux_elems * 4) != hipSuccess || dO.alloc(out_elems * 4) != hipSuccess)
        return -1.f;
    fill_random_t(dt, dA.p, (size_t)M * (K + padA), 1, 1.0f);
    fill_random_t(dt, dW.p, (size_t)N * (K + padW), 2, 0.05f);
    (void)hipMemset(dB.p, 0, (size_t)N * 4);
    (void)hipMemset(dX.p, 0, aux_elems * 4);
    (void)hipMemset(dO.p, 0, out_elems * 4);
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.bias = (const float*)dB.p; a.out = dO.p; a.aux = (const float*)dX.p;
    a.M = M; a.N = N; a.K = K; a.ldo = epilogue == EPI_SWIGLU ? N / 2 : N; a.P = 1; a.T = 2; a.R = 0;
    a.lda = K + padA; a.ldw = K + padW;
    a.qcols = N / 3; a.qscale = 0.125f;
    if (epilogue == EPI_PATCH) { a.P = pP; a.T = pT; a.R = pR; }
    DevBuf dSt, dXg, dV;
    if (epilogue >= EPI_RESID_LN) {  // LN fold: statistics of unit-variance rows, gamma = 1, s = 0, c = 0
        const int hc = epilogue == EPI_RESID_LN ? N : K;
        const int gs = ln_stat_slots(hc), groups = hc / LN_GROUP;
        std::vector<float> st((size_t)M * gs * 2, 0.f), ones((size_t)std::max(N, K), 1.0f);
        for (int m = 0; m < M; ++m)
            for (int g = 0; g < groups; ++g) st[((size_t)m * gs + g) * 2 + 1] = 64.0f;
        if (dSt.alloc(st.size() * 4) != hipSuccess || dXg.alloc((size_t)M * N * 2) != hipSuccess || dV.alloc(ones.size() * 4) != hipSuccess) return -1.f;
        (void)hipMemcpy(dSt.p, st.data(), st.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(dV.p, ones.data(), ones.size() * 4, hipMemcpyHostToDevice);
        a.stats = (float*)dSt.p; a.ln_gs = gs; a.ln_eps = 1e-6f;
        a.ln_gamma = (const float*)dV.p; a.xg = dXg.p;
        a.ln_s = (const float*)dB.p; a.ln_c = (const float*)dB.p;  // zeros
        if (epilogue == EPI_SWIGLU_LN) a.ldo = N / 2;
    }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (auto t0 = std::chrono::steady_clock::now(); std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(100);) {
        for (int i = 0; i < 10; ++i) (void)launch_gemm(dt, (Epilogue)epilogue, a, nullptr);  // ~100 ms warm-up (clock ramp)
        (void)hipDeviceSynchronize();
    }
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) (void)launch_gemm(dt, (Epilogue)epilogue, a, nullptr);
    (void)hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) != hipSuccess) return -1.f;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms / iters;
}

extern "C" float dinov2_hip_op_attention_bench(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t nh, int32_t iters) {
    const DType dt = dtype == 1 ? DT_BF16 : DT_F16;
    DevBuf dQ, dO;
    const size_t nq = (size_t)B * T * 3 * H, no = (size_t)B * T * H;
    if (dQ.alloc(nq * 2) != hipSuccess || dO.alloc(no * 2) != hipSuccess) return -1.f;
    fill_random_t(dt, dQ.p, nq, 3, 1.0f);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    // warm up for ~100 ms: a cold GPU runs the first milliseconds at a fraction of its sustained clock
    for (auto t0 = std::chrono::steady_clock::now(); std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(100);) {
        for (int i = 0; i < 10; ++i) (void)launch_attention(dt, dQ.p, dO.p, B, T, H, nh, true, nullptr);
        (void)hipDeviceSynchronize();
    }
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) (void)launch_attention(dt, dQ.p, dO.p, B, T, H, nh, true, nullptr);
    (void)hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) != hipSuccess) return -1.f;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms / iters;
}

// ---- testing aids: the tuning switches (read from the environment once) and the dispatcher's plan for a shape ----
extern "C" int dinov2_hip_op_set_tuning(const char* key, int32_t value) {
    static const char* const names[TUNE_COUNT] = {"gemm_gen", "gemm_tile", "attn_v", "attn_nwv"};
    if (!key) return DINOV2_HIP_ERR_INVALID;
    for (int k = 0; k < TUNE_COUNT; ++k)
        if (std::strcmp(key, names[k]) == 0) {
            tune_set((TuneKey)k, value);
            return DINOV2_HIP_OK;
        }
    return DINOV2_HIP_ERR_INVALID;
}
extern "C" int dinov2_hip_op_get_tuning(const char* key) {
    static const char* const names[TUNE_COUNT] = {"gemm_gen", "gemm_tile", "attn_v", "attn_nwv"};
    if (!key) return -1;
    for (int k = 0; k < TUNE_COUNT; ++k)
        if (std::strcmp(key, names[k]) == 0) return tune_get((TuneKey)k);
    return -1;
}
// no device needed: nothing is launched and no pointer is dereferenced
static GemmArgs plan_query_args(int32_t epilogue, int32_t M, int32_t N, int32_t K) {
    GemmArgs a{};
    a.M = M; a.N = N; a.K = K; a.ldo = epi_base((Epilogue)epilogue) == EPI_SWIGLU ? N / 2 : N;
    a.P = 1; a.T = 2;
    a.qcols = N / 3;
    return a;
}
extern "C" int dinov2_hip_op_gemm_plan(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, char* out, int32_t cap) {
    if (!out || cap <= 0 || epilogue < 0 || epilogue > EPI_SWIGLU_LN) return DINOV2_HIP_ERR_INVALID;
    const GemmArgs a = plan_query_args(epilogue, M, N, K);
    return gemm_plan_describe(dtype == 1 ? DT_BF16 : DT_F16, (Epilogue)epilogue, a, out, (size_t)cap) == hipSuccess ? DINOV2_HIP_OK : DINOV2_HIP_ERR_INVALID;
}
// The same plan as data.  Every pointer of the query is a distinct made-up address (never dereferenced), so that what a part's arguments add
// to the caller's pointers can be read back from the arguments the kernels would get.
extern "C" int dinov2_hip_op_gemm_plan_parts(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int64_t* out, int32_t cap_records) {
    if (!out || cap_records <= 0 || epilogue < 0 || epilogue > EPI_SWIGLU_LN) return -1;
    auto base = [](int k) { return (uintptr_t)(k + 1) << 40; };
    GemmArgs a = plan_query_args(epilogue, M, N, K);
    a.A = (const void*)base(0); a.W = (const void*)base(1); a.bias = (const float*)base(2); a.aux = (const float*)base(3); a.out = (void*)base(4);
    a.xg = (void*)base(5); a.stats = (float*)base(6); a.ln_gamma = (const float*)base(7); a.ln_s = (const float*)base(8); a.ln_c = (const float*)base(9);
    GemmPlan plan;
    if (gemm_plan(dtype == 1 ? DT_BF16 : DT_F16, (Epilogue)epilogue, a, false, &plan) != hipSuccess) return -1;
    int n = 0;
    for (int i = 0; i < plan.nsteps; ++i) {
        const GemmStep& s = plan.steps[i];
        for (int part = 0; part < (s.family == GEMM2_MIXED || s.family == GEMM4_MIXED ? 2 : 1); ++part, ++n) {
            if (n == cap_records) return -1;
            const GemmArgs& g = s.args[part];
            const uintptr_t ptr[10] = {(uintptr_t)g.A, (uintptr_t)g.W, (uintptr_t)g.bias, (uintptr_t)g.aux, (uintptr_t)g.out,
                                       (uintptr_t)g.xg, (uintptr_t)g.stats, (uintptr_t)g.ln_gamma, (uintptr_t)g.ln_s, (uintptr_t)g.ln_c};
            int64_t* r = out + (size_t)n * DINOV2_HIP_PLAN_PART_FIELDS;
            const int64_t head[17] = {i, part, part ? s.row0 + s.rows0 : s.row0, part ? s.rows - s.rows0 : s.rows0, s.col0, s.cols, g.M, g.N, g.K, g.ldo, g.qcols,
                                      g.nt_out, g.clk_slot, g.ln_gs, plan.whole.nt_out, plan.whole.clk_slot, plan.whole.ln_gs};
            for (int k = 0; k < 17; ++k) r[k] = head[k];
            for (int k = 0; k < 10; ++k) r[17 + k] = (int64_t)(ptr[k] - base(k));
        }
    }
    return n;
}

namespace dinov2 { void pca_ritz(const double* yprev, const double* ynext, const double* g_parts, int nparts, int H, double* evals, double* comp); }
// host-only: the Rayleigh-Ritz step behind dinov2_hip_pca3, for the CPU test-suite
// Clock probe (csrc/device_types.h): the per-translation-unit slot arrays hold running sums; a kernel kind may be served by more than one
// unit (gemm2.hip / gemm4.hip by shape), so the sums of all units are added.
static int read_clock_slots(unsigned long long out[CLK_SLOTS][4]) {
    unsigned long long a[3][CLK_SLOTS * 4] = {};
    if (hipDeviceSynchronize() != hipSuccess || dinov2::gemm_clock_probe_read(a[0]) != hipSuccess ||
        dinov2::gemm4_clock_probe_read(a[1]) != hipSuccess || dinov2::attention_clock_probe_read(a[2]) != hipSuccess)
        return DINOV2_HIP_ERR_HIP;
    for (int s = 0; s < CLK_SLOTS; ++s) {
        out[s][0] = out[s][1] = out[s][2] = out[s][3] = 0;
        for (int u = 0; u < 3; ++u) {
            out[s][0] += a[u][s * 4 + 0];
            out[s][1] += a[u][s * 4 + 1];
            out[s][2] = a[u][s * 4 + 2] > out[s][2] ? a[u][s * 4 + 2] : out[s][2];
            out[s][3] += a[u][s * 4 + 3];
        }
    }
    return DINOV2_HIP_OK;
}
// Running sums for the FFN-in GEMM (the roofline's dominant kernel): shader cycles and 100 MHz ticks of workgroup 0 over all its launches so
// far on the current device; callers take differences over a window.
extern "C" int dinov2_hip_op_clock_probe(uint64_t* cycles, uint64_t* ticks_100mhz) {
    unsigned long long v[CLK_SLOTS][4];
    const int rc = read_clock_slots(v);
    if (rc != DINOV2_HIP_OK) return rc;
    if (cycles) *cycles = v[CLK_FFN_IN][0];
    if (ticks_100mhz) *ticks_100mhz = v[CLK_FFN_IN][1];
    return DINOV2_HIP_OK;
}
// All slots: out18[3 s] = shader cycles, out18[3 s + 1] = 100 MHz ticks, out18[3 s + 2] = launches, running sums; slots 0 .. 5 = QKV, attn-out,
// FFN-in, FFN-out, attention, other GEMM
extern "C" int dinov2_hip_op_clock_slots(uint64_t* out18) {
    if (!out18) return DINOV2_HIP_ERR_INVALID;
    unsigned long long v[CLK_SLOTS][4];
    const int rc = read_clock_slots(v);
    if (rc != DINOV2_HIP_OK) return rc;
    for (int s = 0; s < CLK_SLOTS; ++s) {
        out18[3 * s] = v[s][0];
        out18[3 * s + 1] = v[s][1];
        out18[3 * s + 2] = v[s][3];
    }
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_op_pca_ritz(const double* yprev, const double* ynext, const double* gram, int32_t H, double* evals, double* comp) {
    if (!yprev || !ynext || !gram || !evals || H < 8) return DINOV2_HIP_ERR_INVALID;
    dinov2::pca_ritz(yprev, ynext, gram, 1, H, evals, comp);
    return DINOV2_HIP_OK;
}

// preprocess_u8_kernel alone (mode 0 = dino_preprocess, 1 = dino_classify_preprocess): raw BGR bytes [B, h, w, 3] in, the
// normalised f32 BGR image [B, oh, ow, 3] the forward would consume out -- so the kernel can be compared with
// oracle/preprocess_np.py directly instead of through a whole forward.
extern "C" int dinov2_hip_op_preprocess_u8(int32_t mode, const uint8_t* bgr, int32_t B, int32_t h, int32_t w, int32_t patch,
                                           float* out) {
    int32_t oh = 0, ow = 0;
    if (!bgr || !out || B <= 0 || dinov2_hip_preprocess_size(mode, h, w, patch, &oh, &ow) != DINOV2_HIP_OK) return -1;
    DevBuf dS, dD;
    const size_t nsrc = (size_t)B * h * w * 3, ndst = (size_t)B * oh * ow * 3;
    OP_TRY(dS.alloc(nsrc));
    OP_TRY(dD.alloc(ndst * sizeof(float)));
    OP_TRY(hipMemset(dD.p, 0xff, ndst * sizeof(float)));  // NaN: a pixel the kernel never wrote comes back as NaN
    OP_TRY(hipMemcpy(dS.p, bgr, nsrc, hipMemcpyHostToDevice));
    const int rh = mode == 1 ? 256 : oh, rw = mode == 1 ? 256 : ow;
    OP_TRY(launch_preprocess_u8((const uint8_t*)dS.p, (float*)dD.p, B, h, w, rh, rw, (rh - oh) / 2, (rw - ow) / 2, oh, ow, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(hipMemcpy(out, dD.p, ndst * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// match_normalise_kernel + match_kernel + match_reduce_kernel (csrc/match.hip) on host data, as dinov2_hip_match_tokens runs them
extern "C" int dinov2_hip_op_match(const float* a, int32_t na, const float* b, int32_t nb, int32_t H, int32_t* idx_ab, float* sim_ab,
                                   int32_t* idx_ba, float* sim_ba) {
    if (!a || !b || !idx_ab || !sim_ab || !idx_ba || !sim_ba || na < 1 || na > (1 << 20) || nb < 1 || nb > (1 << 20) || H < 8 || H > 4096)
        return DINOV2_HIP_ERR_INVALID;
    const MatchPlan plan = match_plan(na, nb, H);
    DevBuf dA, dB, dW;
    OP_TRY(dA.alloc((size_t)na * H * 4));
    OP_TRY(dB.alloc((size_t)nb * H * 4));
    OP_TRY(dW.alloc(plan.bytes));
    OP_TRY(hipMemset(dW.p, 0xff, plan.bytes));
    OP_TRY(hipMemcpy(dA.p, a, (size_t)na * H * 4, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(dB.p, b, (size_t)nb * H * 4, hipMemcpyHostToDevice));
    OP_TRY(launch_match((const float*)dA.p, (size_t)H, (const float*)dB.p, (size_t)H, na, nb, H, (char*)dW.p, plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    char* ws = (char*)dW.p;
    OP_TRY(hipMemcpy(idx_ab, ws + plan.idx_ab, (size_t)na * 4, hipMemcpyDeviceToHost));
    OP_TRY(hipMemcpy(sim_ab, ws + plan.sim_ab, (size_t)na * 4, hipMemcpyDeviceToHost));
    OP_TRY(hipMemcpy(idx_ba, ws + plan.idx_ba, (size_t)nb * 4, hipMemcpyDeviceToHost));
    OP_TRY(hipMemcpy(sim_ba, ws + plan.sim_ba, (size_t)nb * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- dinov2_hip_bank_topk's kernels (csrc/bank.hip) on host data: the bank is built by the shared normaliser, then swept and merged ----
namespace {
bool bank_shape_ok(int nq, int nb, int H, int k) {
    return nq >= 1 && nq <= (1 << 20) && nb >= 1 && nb <= (1 << 24) && H >= 8 && H <= 4096 && k >= 1 && k <= BANK_K_MAX;
}
}  // namespace
extern "C" int dinov2_hip_op_bank_plan(int32_t nq, int32_t nb, int32_t H, int32_t k, int32_t chunk_tiles, int64_t* out) {
    if (!out || !bank_shape_ok(nq, nb, H, k) || chunk_tiles < 0) return DINOV2_HIP_ERR_INVALID;
    const BankTopkPlan p = bank_topk_plan(nq, nb, H, k, chunk_tiles);
    out[0] = p.chunk_tiles;
    out[1] = p.nchunks;
    out[2] = p.pass_tiles;
    out[3] = p.ntiles;
    out[4] = (int64_t)((size_t)p.nchunks * p.pass_tiles * MATCH_TM * k * sizeof(BankEntry));
    out[5] = (int64_t)p.bytes;
    return 0;
}
extern "C" int dinov2_hip_op_bank_topk(const float* q, int32_t nq, const float* b, int32_t nb, int32_t H, int32_t k, int32_t chunk_tiles,
                                       int32_t* idx, float* sim) {
    if (!q || !b || !idx || !sim || !bank_shape_ok(nq, nb, H, k) || chunk_tiles < 0) return DINOV2_HIP_ERR_INVALID;
    const BankTopkPlan plan = bank_topk_plan(nq, nb, H, k, chunk_tiles);
    const size_t bank_bytes = (size_t)plan.ntiles * MATCH_TN * plan.hpad * 2;
    DevBuf dQ, dB, dBank, dW;
    OP_TRY(dQ.alloc((size_t)nq * H * 4));
    OP_TRY(dB.alloc((size_t)nb * H * 4));
    OP_TRY(dBank.alloc(bank_bytes));
    OP_TRY(dW.alloc(plan.bytes));
    OP_TRY(hipMemset(dBank.p, 0xff, bank_bytes));  // rows past nb stay NaN: the sweep must mask them
    OP_TRY(hipMemset(dW.p, 0xff, plan.bytes));
    OP_TRY(hipMemcpy(dQ.p, q, (size_t)nq * H * 4, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(dB.p, b, (size_t)nb * H * 4, hipMemcpyHostToDevice));
    OP_TRY(launch_match_normalise((const float*)dB.p, (size_t)H, (_Float16*)dBank.p, nb, nb, H, plan.hpad, nullptr));
    OP_TRY(launch_bank_topk((const float*)dQ.p, (size_t)H, nq, (const _Float16*)dBank.p, nb, H, k, (char*)dW.p, plan, false, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(hipMemcpy(idx, (char*)dW.p + plan.idx, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    OP_TRY(hipMemcpy(sim, (char*)dW.p + plan.sim, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int dinov2_hip_op_bank_bench(const float* q_dev, int32_t nq, const float* b_dev, int32_t nb, int32_t H, int32_t k,
                                        int32_t chunk_tiles, int32_t warmup, int32_t iters, int32_t floor_only, float* ms) {
    if (!q_dev || !b_dev || !ms || !bank_shape_ok(nq, nb, H, k) || chunk_tiles < 0 || warmup < 0 || iters < 1) return DINOV2_HIP_ERR_INVALID;
    const BankTopkPlan plan = bank_topk_plan(nq, nb, H, k, chunk_tiles);
    DevBuf dBank, dW;
    OP_TRY(dBank.alloc((size_t)plan.ntiles * MATCH_TN * plan.hpad * 2));
    OP_TRY(dW.alloc(plan.bytes));
    OP_TRY(hipMemset(dBank.p, 0, (size_t)plan.ntiles * MATCH_TN * plan.hpad * 2));
    OP_TRY(launch_match_normalise(b_dev, (size_t)H, (_Float16*)dBank.p, nb, nb, H, plan.hpad, nullptr));
    hipEvent_t e0, e1;
    OP_TRY(hipEventCreate(&e0));
    OP_TRY(hipEventCreate(&e1));
    int rc = 0;
    for (int i = 0; i < warmup + iters && rc == 0; ++i) {
        if (i == warmup && hipEventRecord(e0, nullptr) != hipSuccess) rc = -1;
        if (launch_bank_topk(q_dev, (size_t)H, nq, (const _Float16*)dBank.p, nb, H, k, (char*)dW.p, plan, floor_only != 0, nullptr) != hipSuccess)
            rc = -1;
    }
    float t = 0.0f;
    if (rc == 0 && (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                    hipEventElapsedTime(&t, e0, e1) != hipSuccess))
        rc = -1;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipDeviceSynchronize();
    *ms = t / (float)iters;
    return rc;
}

// ---- the device stages of dinov2_hip_pca3 (csrc/pca.cpp), each through the launch function the driver calls, on host data ----
namespace {
// A device output of n elements of esz bytes between two guard bands of DINOV2_HIP_OP_GUARD_ROWS rows of `row` elements; the whole buffer
// starts as 0xff bytes (NaN in f16, f32 and f64), so an element the kernel never wrote comes back as NaN and a write outside changes a guard.
struct Guarded {
    DevBuf d;
    size_t n = 0, ng = 0, esz = 0;
    hipError_t alloc(size_t n_, size_t row, size_t esz_) {
        n = n_; ng = (size_t)DINOV2_HIP_OP_GUARD_ROWS * row; esz = esz_;
        hipError_t e = d.alloc((n + 2 * ng) * esz);
        return e != hipSuccess ? e : hipMemset(d.p, 0xff, (n + 2 * ng) * esz);
    }
    void* ptr() const { return (char*)d.p + ng * esz; }
    // the payload to `host` (n * esz bytes): 0, -1 on a HIP error, DINOV2_HIP_OP_GUARD_CHANGED
    int fetch(void* host) const {
        std::vector<unsigned char> raw((n + 2 * ng) * esz);
        if (hipMemcpy(raw.data(), d.p, raw.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (size_t k = 0; k < ng * esz; ++k)
            if (raw[k] != 0xffu || raw[(ng + n) * esz + k] != 0xffu) return DINOV2_HIP_OP_GUARD_CHANGED;
        std::memcpy(host, raw.data() + ng * esz, n * esz);
        return 0;
    }
};
bool pca_shape_ok(int P, int H) { return P >= 4 && H >= 8 && H <= 4096; }  // the range dinov2_hip_pca3 accepts
hipError_t upload(const void* src, size_t bytes, DevBuf& d) {
    hipError_t e = d.alloc(bytes);
    return e != hipSuccess ? e : hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice);
}
}  // namespace

extern "C" int dinov2_hip_op_pca_ppad(int32_t P) { return pca_ppad(P); }
extern "C" int dinov2_hip_op_pca_blocks(int32_t H) { return pca_blocks(H); }

extern "C" int dinov2_hip_op_pca_prepare(const float* tok, int32_t P, int32_t H, float* mean_out, float* xt_out) {
    if (!tok || !mean_out || !xt_out || !pca_shape_ok(P, H)) return DINOV2_HIP_ERR_INVALID;
    const int Ppad = pca_ppad(P);
    const size_t nxt = (size_t)H * Ppad;
    DevBuf dT;
    Guarded gM, gX;
    OP_TRY(upload(tok, (size_t)P * H * 4, dT));
    OP_TRY(gM.alloc((size_t)H, (size_t)H, 4));
    OP_TRY(gX.alloc(nxt, (size_t)Ppad, 2));
    OP_TRY(launch_pca_prepare((const float*)dT.p, (float*)gM.ptr(), gX.ptr(), P, H, Ppad, nullptr));
    OP_TRY(hipDeviceSynchronize());
    int rc = gM.fetch(mean_out);
    if (rc != 0) return rc;
    std::vector<_Float16> raw(nxt);
    rc = gX.fetch(raw.data());
    if (rc != 0) return rc;
    for (size_t i = 0; i < nxt; ++i) xt_out[i] = (float)raw[i];
    return 0;
}

extern "C" int dinov2_hip_op_pca_cov(const float* tok, int32_t P, int32_t H, float* cov_out) {
    if (!tok || !cov_out || !pca_shape_ok(P, H)) return DINOV2_HIP_ERR_INVALID;
    if (gemm_init() != hipSuccess) return -1;
    const int Ppad = pca_ppad(P);
    DevBuf dT, dM, dX;
    Guarded gC;
    OP_TRY(upload(tok, (size_t)P * H * 4, dT));
    OP_TRY(dM.alloc((size_t)H * 4));
    OP_TRY(dX.alloc((size_t)H * Ppad * 2));
    OP_TRY(hipMemset(dX.p, 0xff, (size_t)H * Ppad * 2));  // (the driver's xt is reused scratch: whatever prepare leaves unwritten is read as it is)
    OP_TRY(gC.alloc((size_t)H * H, (size_t)H, 4));
    OP_TRY(launch_pca_prepare((const float*)dT.p, (float*)dM.p, dX.p, P, H, Ppad, nullptr));
    OP_TRY(launch_pca_cov(dX.p, (float*)gC.ptr(), H, Ppad, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return gC.fetch(cov_out);
}

extern "C" int dinov2_hip_op_pca_power(const float* cov, const double* yprev, const double* gprev_parts, int32_t H, double* ynext,
                                       double* gnext_parts) {
    if (!cov || !yprev || !gprev_parts || !ynext || !gnext_parts || H < 8 || H > 4096) return DINOV2_HIP_ERR_INVALID;
    const size_t ny = (size_t)H * PCA_NB, ng = (size_t)pca_blocks(H) * 64;
    DevBuf dC, dY, dG;
    Guarded gY, gG;
    OP_TRY(upload(cov, (size_t)H * H * 4, dC));
    OP_TRY(upload(yprev, ny * 8, dY));
    OP_TRY(upload(gprev_parts, ng * 8, dG));
    OP_TRY(gY.alloc(ny, PCA_NB, 8));
    OP_TRY(gG.alloc(ng, 64, 8));
    OP_TRY(launch_pca_power((const float*)dC.p, (const double*)dY.p, (const double*)dG.p, (double*)gY.ptr(), (double*)gG.ptr(), H, nullptr));
    OP_TRY(hipDeviceSynchronize());
    const int rc = gY.fetch(ynext);
    return rc != 0 ? rc : gG.fetch(gnext_parts);
}

extern "C" int dinov2_hip_op_pca_project(const float* tok, const float* mean, const float* comp, int32_t P, int32_t H, float* proj) {
    if (!tok || !mean || !comp || !proj || !pca_shape_ok(P, H)) return DINOV2_HIP_ERR_INVALID;
    DevBuf dT, dM, dC;
    Guarded gP;
    OP_TRY(upload(tok, (size_t)P * H * 4, dT));
    OP_TRY(upload(mean, (size_t)H * 4, dM));
    OP_TRY(upload(comp, (size_t)3 * H * 4, dC));
    OP_TRY(gP.alloc((size_t)P * 3, 3, 4));
    OP_TRY(launch_pca_project((const float*)dT.p, (const float*)dM.p, (const float*)dC.p, (float*)gP.ptr(), P, H, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return gP.fetch(proj);
}

// host-only: pca_chol_rinv (csrc/kernels.h), the factorisation the power kernel and pca_ritz share
extern "C" int dinov2_hip_op_pca_chol_rinv(const double* gram, double* rinv) {
    if (!gram || !rinv) return DINOV2_HIP_ERR_INVALID;
    pca_chol_rinv(gram, rinv);
    return DINOV2_HIP_OK;
}

// ---- the kernels of csrc/dense.hip (dinov2_hip_predict_dense) on host data ----
extern "C" int dinov2_hip_op_dense_reduce_plan(int32_t h0, int32_t w0, int32_t C, int32_t out_h, int32_t out_w, int64_t* out) {
    const DenseReducePlan p = dense_reduce_plan(h0, w0, C, out_h, out_w);
    if (!out || p.tile_y == 0) return DINOV2_HIP_ERR_INVALID;
    out[0] = p.tile_y;
    out[1] = p.tile_x;
    out[2] = p.span_y;
    out[3] = p.span_x;
    out[4] = p.pitch;
    out[5] = (int64_t)p.lds_bytes;
    return 0;
}
extern "C" int dinov2_hip_op_dense_reduce(const float* logits, int32_t h0, int32_t w0, int32_t C, int32_t out_h, int32_t out_w, int32_t reduce,
                                          const float* centers, float eps, uint8_t* labels, float* value) {
    const DenseReducePlan plan = dense_reduce_plan(h0, w0, C, out_h, out_w);
    if (!logits || plan.tile_y == 0 || (reduce != DENSE_ARGMAX && reduce != DENSE_BINS)) return DINOV2_HIP_ERR_INVALID;
    if (reduce == DENSE_BINS ? (!centers || !(eps > 0.0f) || labels || !value) : (!labels && !value)) return DINOV2_HIP_ERR_INVALID;
    const size_t P = (size_t)h0 * w0, ldl = (size_t)dense_cpad(C), npx = (size_t)out_h * out_w, ng = (size_t)DINOV2_HIP_OP_GUARD_ROWS * out_w;
    DevBuf dL, dC, dLab, dVal;
    OP_TRY(dL.alloc(P * ldl * 4));
    OP_TRY(hipMemset(dL.p, 0xff, P * ldl * 4));  // the columns past C stay NaN: the kernel must not let them into a result
    OP_TRY(hipMemcpy2D(dL.p, ldl * 4, logits, (size_t)C * 4, (size_t)C * 4, P, hipMemcpyHostToDevice));
    if (reduce == DENSE_BINS) {
        OP_TRY(dC.alloc((size_t)C * 4));
        OP_TRY(hipMemcpy(dC.p, centers, (size_t)C * 4, hipMemcpyHostToDevice));
    }
    if (labels) {
        OP_TRY(dLab.alloc(npx + 2 * ng));
        OP_TRY(hipMemset(dLab.p, 0xff, npx + 2 * ng));
    }
    if (value) {
        OP_TRY(dVal.alloc((npx + 2 * ng) * 4));
        OP_TRY(hipMemset(dVal.p, 0xff, (npx + 2 * ng) * 4));
    }
    OP_TRY(launch_dense_reduce((const float*)dL.p, (int)ldl, 1, h0, w0, C, out_h, out_w, reduce, (const float*)dC.p, eps,
                               labels ? (uint8_t*)dLab.p + ng : nullptr, value ? (float*)dVal.p + ng : nullptr, plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    if (labels) {
        std::vector<uint8_t> raw(npx + 2 * ng);
        OP_TRY(hipMemcpy(raw.data(), dLab.p, raw.size(), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < ng; ++k)
            if (raw[k] != 0xff || raw[ng + npx + k] != 0xff) return DINOV2_HIP_OP_GUARD_CHANGED;
        std::memcpy(labels, raw.data() + ng, npx);
    }
    if (value) {
        std::vector<uint32_t> raw(npx + 2 * ng);
        OP_TRY(hipMemcpy(raw.data(), dVal.p, raw.size() * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < ng; ++k)
            if (raw[k] != 0xffffffffu || raw[ng + npx + k] != 0xffffffffu) return DINOV2_HIP_OP_GUARD_CHANGED;
        std::memcpy(value, raw.data() + ng, npx * 4);
    }
    return 0;
}
extern "C" int dinov2_hip_op_dense_pack(const float* x, const float* ln_w, const float* ln_b, float eps, int32_t B, int32_t T, int32_t R, int32_t H,
                                        int32_t norm, int32_t concat_cls, int32_t slot, int32_t nslots, float* out) {
    if (!x || !out || B <= 0 || H <= 0 || H % 8 != 0 || R < 0 || T < 2 + R || nslots < 1 || nslots > DENSE_LAYERS_MAX || slot < 0 || slot >= nslots)
        return DINOV2_HIP_ERR_INVALID;
    if (norm && (!ln_w || !ln_b)) return DINOV2_HIP_ERR_INVALID;
    const size_t P = (size_t)(T - 1 - R), hblk = (size_t)H * (concat_cls ? 2 : 1), K = hblk * nslots, n = (size_t)B * P * K;
    const size_t nx = (size_t)B * T * H, ng = (size_t)DINOV2_HIP_OP_GUARD_ROWS * K;
    DevBuf dX, dW, dB, dA;
    OP_TRY(dX.alloc(nx * 4));
    OP_TRY(hipMemcpy(dX.p, x, nx * 4, hipMemcpyHostToDevice));
    if (norm) {
        OP_TRY(dW.alloc((size_t)H * 4));
        OP_TRY(dB.alloc((size_t)H * 4));
        OP_TRY(hipMemcpy(dW.p, ln_w, (size_t)H * 4, hipMemcpyHostToDevice));
        OP_TRY(hipMemcpy(dB.p, ln_b, (size_t)H * 4, hipMemcpyHostToDevice));
    }
    OP_TRY(dA.alloc((n + 2 * ng) * 2));
    OP_TRY(hipMemset(dA.p, 0xff, (n + 2 * ng) * 2));
    OP_TRY(launch_dense_pack((const float*)dX.p, (const float*)dW.p, (const float*)dB.p, eps, B, T, R, H, norm != 0, concat_cls != 0,
                             (_Float16*)dA.p + ng, K, (int)(slot * hblk), nullptr));
    OP_TRY(hipDeviceSynchronize());
    std::vector<uint16_t> raw(n + 2 * ng);
    OP_TRY(hipMemcpy(raw.data(), dA.p, raw.size() * 2, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < ng; ++k)
        if (raw[k] != 0xffffu || raw[ng + n + k] != 0xffffu) return DINOV2_HIP_OP_GUARD_CHANGED;
    for (size_t i = 0; i < n; ++i) {
        _Float16 hv;
        std::memcpy(&hv, &raw[ng + i], 2);
        out[i] = (float)hv;
    }
    return 0;
}
