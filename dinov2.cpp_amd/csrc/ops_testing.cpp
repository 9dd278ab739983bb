// Diagnostic entry points (include/dinov2_hip_ops.h): run ONE kernel on host-provided f32 data so that the parity
// tests can check each hand-written kernel against the oracle / numpy in isolation.  Not used by predict.
// Every entry point reads: validate, stage (OpBuf), launch, fetch.
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
#include "far_pattern.h"
#include "host.h"
#include "ops_frame.h"

using namespace dinov2;

namespace {

#define OP_TRY(x)                          \
    do {                                   \
        if ((x) != hipSuccess) return -1;  \
    } while (0)

struct OpBuf {
    // A device buffer of one diagnostic call, freed on return.  Inputs: upload / upload_as.  Outputs: alloc, then fetch / fetch_as.
    // An output starts as it is, as 0x00 bytes, as 0xff bytes (nans(): a NaN in f16, bf16, f32 and f64, so an element the kernel never wrote
    // comes back as NaN) or as a copy of host contents.  With guard_row > 0 it sits between two guard bands of DINOV2_HIP_OP_GUARD_ROWS rows
    // of guard_row elements, 0xff bytes too: a write outside the output changes one, and the fetch returns DINOV2_HIP_OP_GUARD_CHANGED.
    struct Fill {
        int byte;          // the byte every element starts as, -1 = none
        const void* host;  // or: n * esz bytes to start from
    };
    static Fill none() { return {-1, nullptr}; }
    static Fill zeros() { return {0x00, nullptr}; }
    static Fill nans() { return {0xff, nullptr}; }
    static Fill copy_of(const void* host) { return {-1, host}; }

    void* p = nullptr;  // the allocation: [ng | n | ng] elements of esz bytes
    size_t n = 0, ng = 0, esz = 1;

    OpBuf() = default;
    OpBuf(const OpBuf&) = delete;
    OpBuf& operator=(const OpBuf&) = delete;
    ~OpBuf() {
        if (p) (void)hipFree(p);
    }

    hipError_t alloc(size_t n_, size_t esz_, Fill fill, size_t guard_row = 0) {
        n = n_; esz = esz_; ng = (size_t)DINOV2_HIP_OP_GUARD_ROWS * guard_row;
        const size_t all = (n + 2 * ng) * esz;
        hipError_t e = hipMalloc(&p, all ? all : 16);
        if (e == hipSuccess && (ng || fill.byte == 0xff)) e = hipMemset(p, 0xff, all);  // the bands, and a NaN payload
        if (e == hipSuccess && fill.byte >= 0 && fill.byte != 0xff) e = hipMemset(as<void>(), fill.byte, n * esz);
        if (e == hipSuccess && fill.host) e = hipMemcpy(as<void>(), fill.host, n * esz, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t upload(const void* src, size_t bytes) { return alloc(bytes, 1, copy_of(src)); }
    static uint16_t round_to(DType dt, float f) {  // nearest even
        uint16_t u;
        if (dt == DT_F16) {
            const _Float16 h = (_Float16)f;
            std::memcpy(&u, &h, 2);
        } else {
            const __bf16 h = (__bf16)f;
            std::memcpy(&u, &h, 2);
        }
        return u;
    }
    // n f32 values rounded to the compute type
    hipError_t upload_as(DType dt, const float* src, size_t count) {
        std::vector<uint16_t> v(count);
        for (size_t i = 0; i < count; ++i) v[i] = round_to(dt, src[i]);
        return alloc(count, 2, copy_of(v.data()));
    }
    // a benchmark's operand: count uniform values in [-scale, scale) of the compute type.  Only the allocation is reported; the copy is not checked.
    hipError_t alloc_random(DType dt, size_t count, unsigned seed, float scale) {
        const hipError_t e = alloc(count, 2, none());
        if (e != hipSuccess) return e;
        std::vector<uint16_t> v(count);
        unsigned s = seed * 2654435761u + 12345u;
        for (size_t i = 0; i < count; ++i) {
            s = s * 1664525u + 1013904223u;
            v[i] = round_to(dt, (((float)(s >> 8) / 8388608.0f) - 1.0f) * scale);  // full-range random
        }
        (void)hipMemcpy(p, v.data(), count * 2, hipMemcpyHostToDevice);
        return hipSuccess;
    }

    // the payload (null for a buffer never allocated: an operand or output the call does without)
    template <typename T>
    T* as() const {
        return (T*)((char*)p + ng * esz);
    }

    // `bytes` of the payload from byte `off` on, the guards unchecked: pieces of a workspace
    hipError_t read(void* host, size_t off, size_t bytes) const { return hipMemcpy(host, as<char>() + off, bytes, hipMemcpyDeviceToHost); }
    // the payload to `host` (n * esz bytes): 0, -1 on a HIP error, DINOV2_HIP_OP_GUARD_CHANGED
    int fetch(void* host) const {
        if (!ng) return read(host, 0, n * esz) == hipSuccess ? 0 : -1;
        std::vector<unsigned char> raw;
        if (!pull(raw)) return -1;
        return frame_payload(raw.data(), n, ng, esz, host) ? 0 : DINOV2_HIP_OP_GUARD_CHANGED;
    }
    // the same for a payload of n two-byte values of type dt, widened to f32 straight from the frame
    int fetch_as(DType dt, float* host) const {
        std::vector<unsigned char> raw;
        if (!pull(raw)) return -1;
        if (!frame_intact(raw.data(), n, ng, esz)) return DINOV2_HIP_OP_GUARD_CHANGED;
        widen_to_f32(dt == DT_BF16, raw.data() + ng * esz, n, host);
        return 0;
    }

private:
    bool pull(std::vector<unsigned char>& raw) const {  // the whole allocation, bands included
        raw.resize((n + 2 * ng) * esz);
        return hipMemcpy(raw.data(), p, raw.size(), hipMemcpyDeviceToHost) == hipSuccess;
    }
};

#define OP_FETCH(x)                 \
    do {                            \
        const int rc__ = (x);       \
        if (rc__ != 0) return rc__; \
    } while (0)

DType dtype_of(int32_t dtype) { return dtype == 1 ? DT_BF16 : DT_F16; }

}  // namespace

extern "C" int dinov2_hip_op_gemm(int32_t dtype, int32_t epilogue, const float* A, const float* W, const float* bias,
                                  const float* aux, int64_t aux_count, float* out, int32_t out_rows, int32_t ldo,
                                  int32_t M, int32_t N, int32_t K, int32_t P, int32_t T, int32_t R, int32_t qcols,
                                  float qscale) {
    const DType dt = dtype_of(dtype);
    if (gemm_init() != hipSuccess) return -1;
    const bool f32out = epilogue == EPI_PATCH || epilogue == EPI_RESID || epilogue == EPI_PLAIN_F32;
    const size_t on = (size_t)out_rows * ldo;
    OpBuf dA, dW, dB, dX, dO;
    OP_TRY(dA.upload_as(dt, A, (size_t)M * K));
    OP_TRY(dW.upload_as(dt, W, (size_t)N * K));
    if (bias) OP_TRY(dB.upload(bias, sizeof(float) * N));
    if (aux) OP_TRY(dX.upload(aux, sizeof(float) * (size_t)aux_count));
    if (f32out) OP_TRY(dO.alloc(on, 4, OpBuf::copy_of(out)));
    else OP_TRY(dO.alloc(on, 2, OpBuf::zeros()));
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.bias = dB.as<float>(); a.out = dO.p; a.aux = dX.as<float>();
    a.M = M; a.N = N; a.K = K; a.ldo = ldo; a.P = P; a.T = T; a.R = R; a.qcols = qcols; a.qscale = qscale;
    OP_TRY(launch_gemm(dt, (Epilogue)epilogue, a, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return f32out ? dO.fetch(out) : dO.fetch_as(dt, out);
}

// ---- LN fold (kernels.h): the producer epilogue, the consumer epilogues, the two small kernels, each alone ----
extern "C" int dinov2_hip_op_gemm_resid_ln(int32_t dtype, const float* A, const float* W, const float* bias, const float* ls, const float* gamma,
                                           float* x, float* xg, float* stats, int32_t M, int32_t N, int32_t K) {
    const DType dt = dtype_of(dtype);
    if (gemm_init() != hipSuccess) return -1;
    const int gs = ln_stat_slots(N);
    OpBuf dA, dW, dBias, dLs, dGamma, dX, dG, dS;
    OP_TRY(dA.upload_as(dt, A, (size_t)M * K));
    OP_TRY(dW.upload_as(dt, W, (size_t)N * K));
    OP_TRY(dBias.upload(bias, sizeof(float) * N));
    OP_TRY(dLs.upload(ls, sizeof(float) * N));
    OP_TRY(dGamma.upload(gamma, sizeof(float) * N));
    OP_TRY(dX.alloc((size_t)M * N, 4, OpBuf::copy_of(x)));
    OP_TRY(dG.alloc((size_t)M * N, 2, OpBuf::zeros()));
    OP_TRY(dS.alloc(2 * (size_t)M * gs, 4, OpBuf::zeros()));
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.bias = dBias.as<float>(); a.aux = dLs.as<float>(); a.ln_gamma = dGamma.as<float>();
    a.out = dX.p; a.xg = dG.p; a.stats = dS.as<float>(); a.ln_gs = gs;
    a.M = M; a.N = N; a.K = K; a.ldo = N;
    OP_TRY(launch_gemm(dt, EPI_RESID_LN, a, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(dX.fetch(x));
    OP_FETCH(dG.fetch_as(dt, xg));
    return dS.fetch(stats);
}

extern "C" int dinov2_hip_op_gemm_ln_consumer(int32_t dtype, int32_t epilogue, const float* A, const float* W, const float* ln_s, const float* ln_c,
                                              const float* stats, float eps, float* out, int32_t ldo, int32_t M, int32_t N, int32_t K,
                                              int32_t qcols, float qscale) {
    const DType dt = dtype_of(dtype);
    if (gemm_init() != hipSuccess) return -1;
    if (!epi_ln_consumer((Epilogue)epilogue)) return -1;
    const int gs = ln_stat_slots(K);
    OpBuf dA, dW, dLnS, dLnC, dS, dO;
    OP_TRY(dA.upload_as(dt, A, (size_t)M * K));
    OP_TRY(dW.upload_as(dt, W, (size_t)N * K));
    OP_TRY(dLnS.upload(ln_s, sizeof(float) * N));
    OP_TRY(dLnC.upload(ln_c, sizeof(float) * N));
    OP_TRY(dS.upload(stats, sizeof(float) * 2 * (size_t)M * gs));
    OP_TRY(dO.alloc((size_t)M * ldo, 2, OpBuf::zeros()));
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.ln_s = dLnS.as<float>(); a.ln_c = dLnC.as<float>(); a.stats = dS.as<float>(); a.ln_gs = gs; a.ln_eps = eps;
    a.out = dO.p;
    a.M = M; a.N = N; a.K = K; a.ldo = ldo; a.qcols = qcols; a.qscale = qscale;
    OP_TRY(launch_gemm(dt, (Epilogue)epilogue, a, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dO.fetch_as(dt, out);
}

extern "C" int dinov2_hip_op_ln_prepare(int32_t dtype, const float* x, const float* gamma, float* xg, float* stats, int32_t rows, int32_t H) {
    const DType dt = dtype_of(dtype);
    const int gs = ln_stat_slots(H);
    OpBuf dX, dV, dG, dS;
    OP_TRY(dX.upload(x, sizeof(float) * (size_t)rows * H));
    OP_TRY(dV.upload(gamma, sizeof(float) * (size_t)H));
    OP_TRY(dG.alloc((size_t)rows * H, 2, OpBuf::none()));
    OP_TRY(dS.alloc(2 * (size_t)rows * gs, 4, OpBuf::zeros()));
    OP_TRY(launch_ln_prepare(dt, dX.as<float>(), dV.as<float>(), dG.p, dS.as<float>(), gs, rows, H, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(dG.fetch_as(dt, xg));
    return dS.fetch(stats);
}

extern "C" int dinov2_hip_op_im2col(int32_t dtype, const float* img, float* col, int32_t B, int32_t Hh, int32_t Ww, int32_t patch, int32_t Kpad,
                                    int32_t layout) {
    const DType dt = dtype_of(dtype);
    if (B <= 0 || Hh <= 0 || Ww <= 0 || patch <= 0) return -1;
    const size_t npix = (size_t)B * 3 * Hh * Ww, rows = (size_t)B * (Hh / patch) * (Ww / patch);
    OpBuf dI, dC;
    OP_TRY(dI.upload(img, sizeof(float) * npix));
    OP_TRY(dC.alloc(rows * (size_t)Kpad, 2, OpBuf::nans()));  // every element must be written
    OP_TRY(launch_im2col(dt, dI.as<float>(), dC.p, B, Hh, Ww, patch, Kpad, layout, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dC.fetch_as(dt, col);
}

extern "C" int dinov2_hip_op_im2col_stride(int32_t dtype, const float* img, float* col, int32_t B, int32_t Hh, int32_t Ww, int32_t patch,
                                           int32_t stride, int32_t Kpad, int32_t layout) {
    const DType dt = dtype_of(dtype);
    if (B <= 0 || patch <= 0 || stride <= 0 || Hh < patch || Ww < patch || Kpad <= 0) return -1;
    const size_t npix = (size_t)B * 3 * Hh * Ww, rows = (size_t)B * grid_dim(Hh, patch, stride) * grid_dim(Ww, patch, stride);
    OpBuf dI, dC;
    OP_TRY(dI.upload(img, sizeof(float) * npix));
    OP_TRY(dC.alloc(rows * (size_t)Kpad, 2, OpBuf::nans()));  // every element must be written
    OP_TRY(launch_im2col_stride(dt, dI.as<float>(), dC.p, B, Hh, Ww, patch, stride, Kpad, layout, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dC.fetch_as(dt, col);
}

extern "C" int dinov2_hip_op_ln_fold_vectors(int32_t dtype, const float* W, const float* bias, const float* gamma, const float* beta, float* s_out,
                                             float* c_out, int32_t N, int32_t K) {
    const DType dt = dtype_of(dtype);
    OpBuf dW, dBias, dGamma, dBeta, dS, dC;
    OP_TRY(dW.upload_as(dt, W, (size_t)N * K));
    OP_TRY(dBias.upload(bias, sizeof(float) * N));
    OP_TRY(dGamma.upload(gamma, sizeof(float) * K));
    OP_TRY(dBeta.upload(beta, sizeof(float) * K));
    OP_TRY(dS.alloc((size_t)N, 4, OpBuf::none()));
    OP_TRY(dC.alloc((size_t)N, 4, OpBuf::none()));
    OP_TRY(launch_ln_fold_vectors(dt, dW.p, dBias.as<float>(), dGamma.as<float>(), dBeta.as<float>(), dS.as<float>(), dC.as<float>(), N, K, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(dS.fetch(s_out));
    return dC.fetch(c_out);
}

extern "C" int dinov2_hip_op_attention(int32_t dtype, const float* qkv, float* out, int32_t B, int32_t T, int32_t H,
                                       int32_t nh) {
    return dinov2_hip_op_attention_ex(dtype, qkv, out, B, T, H, nh, 0);
}

extern "C" int dinov2_hip_op_attention_ex(int32_t dtype, const float* qkv, float* out, int32_t B, int32_t T, int32_t H,
                                          int32_t nh, int32_t log2_scores) {
    const DType dt = dtype_of(dtype);
    if (B <= 0 || T <= 0 || H <= 0) return -1;
    OpBuf dQ, dO;
    OP_TRY(dQ.upload_as(dt, qkv, (size_t)B * T * 3 * H));
    OP_TRY(dO.alloc((size_t)B * T * H, 2, OpBuf::nans(), (size_t)H));  // a write outside rows [0, B*T) changes a guard
    OP_TRY(launch_attention(dt, dQ.p, dO.as<void>(), B, T, H, nh, log2_scores != 0, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dO.fetch_as(dt, out);
}

// ---- dinov2_hip_predict_list: its plan (no device) and the list form of the attention kernels over segments of given lengths ----
extern "C" int dinov2_hip_op_list_plan(int32_t n, const int32_t* h, const int32_t* w, int32_t patch, int32_t R, int32_t nh, int32_t order,
                                       int64_t* images, int32_t* runs, int32_t* items, int64_t cap_items, int64_t* totals) {
    if (n <= 0 || !h || !w || patch <= 0 || R < 0 || nh <= 0 || !totals || (order != LIST_ORDER_AS_GIVEN && order != LIST_ORDER_LONGEST_FIRST))
        return DINOV2_HIP_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (h[i] < 0 || w[i] < 0) return DINOV2_HIP_ERR_INVALID;
    std::vector<ListImage> im((size_t)n);
    std::vector<ListRun> rn((size_t)n);
    const ListPlan p = list_plan(n, h, w, patch, patch, R, nh, order, im.data(), rn.data(), nullptr);
    totals[0] = p.M; totals[1] = p.P; totals[2] = p.pixels; totals[3] = p.units; totals[4] = p.nruns;
    if (p.M > (int64_t)INT32_MAX) return DINOV2_HIP_ERR_INVALID;  // (the table holds row0 in 32 bits)
    for (int i = 0; images && i < n; ++i) {
        const int64_t rec[5] = {im[(size_t)i].row0, im[(size_t)i].T, im[(size_t)i].P, im[(size_t)i].h0, im[(size_t)i].w0};
        std::copy(rec, rec + 5, images + (size_t)i * 5);
    }
    for (int r = 0; runs && r < p.nruns; ++r) {
        runs[2 * r] = rn[(size_t)r].first;
        runs[2 * r + 1] = rn[(size_t)r].count;
    }
    if (items) {
        if (cap_items < p.units) return DINOV2_HIP_ERR_INVALID;
        static_assert(sizeof(AttnItem) == 4 * sizeof(int32_t), "an item is four int32: row0, T, head, query block");
        (void)list_plan(n, h, w, patch, patch, R, nh, order, nullptr, nullptr, reinterpret_cast<AttnItem*>(items));
    }
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_op_attention_list(int32_t dtype, const float* qkv, float* out, int32_t n, const int32_t* T, int32_t H, int32_t nh,
                                            int32_t log2_scores) {
    const DType dt = dtype_of(dtype);
    if (!qkv || !out || n <= 0 || !T || nh <= 0 || H != nh * 64) return -1;
    // a segment of T tokens as a 1-pixel-patch image of (T - 1) x 1 patches without registers: the table is the forward's own
    std::vector<int32_t> hh((size_t)n), ww((size_t)n, 1);
    for (int i = 0; i < n; ++i) {
        if (T[i] <= 0 || (size_t)T[i] * 3 * H * 2 >= ((size_t)1 << 32)) return -1;  // the per-image bound of the 32-bit staging cursors
        hh[(size_t)i] = T[i] - 1;
    }
    const int order = tune_get(TUNE_LIST_ORDER) == 1 ? LIST_ORDER_LONGEST_FIRST : LIST_ORDER_AS_GIVEN;
    ListPlan p = list_plan(n, hh.data(), ww.data(), 1, 1, 0, nh, order, nullptr, nullptr, nullptr);
    if (p.M > (int64_t)INT32_MAX) return -1;
    std::vector<AttnItem> items((size_t)p.units);
    p = list_plan(n, hh.data(), ww.data(), 1, 1, 0, nh, order, nullptr, nullptr, items.data());
    OpBuf dQ, dI, dO;
    OP_TRY(dQ.upload_as(dt, qkv, (size_t)p.M * 3 * H));
    OP_TRY(dI.upload(items.data(), items.size() * sizeof(AttnItem)));
    OP_TRY(dO.alloc((size_t)p.M * H, 2, OpBuf::nans(), (size_t)H));  // a write outside rows [0, sum T) changes a guard
    OP_TRY(launch_attention_list(dt, dQ.p, dO.as<void>(), dI.as<AttnItem>(), (int)items.size(), (long)p.units, H, nh, log2_scores != 0, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dO.fetch_as(dt, out);
}

extern "C" int dinov2_hip_op_layernorm(int32_t dtype, const float* x, const float* w, const float* b, float* out,
                                       int32_t rows, int32_t H, float eps) {
    const size_t n = (size_t)rows * H;
    OpBuf dX, dW, dB, dO;
    OP_TRY(dX.upload(x, n * 4));
    OP_TRY(dW.upload(w, (size_t)H * 4));
    OP_TRY(dB.upload(b, (size_t)H * 4));
    OP_TRY(dO.alloc(n, dtype < 0 ? 4 : 2, OpBuf::nans()));
    if (dtype < 0) {
        OP_TRY(launch_layernorm_f32(dX.as<float>(), dW.as<float>(), dB.as<float>(), dO.as<float>(), rows, H, eps, nullptr));
        OP_TRY(hipDeviceSynchronize());
        return dO.fetch(out);
    }
    const DType dt = dtype_of(dtype);
    OP_TRY(launch_layernorm(dt, dX.as<float>(), dW.as<float>(), dB.as<float>(), dO.p, rows, H, eps, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dO.fetch_as(dt, out);
}

extern "C" int dinov2_hip_op_layer_tap(const float* x, const float* w, const float* b, float eps, int32_t B, int32_t T, int32_t R, int32_t H,
                                       int32_t h0, int32_t w0, int32_t norm, int32_t layout, float* patch_out, float* cls_out, float* reg_out) {
    if (B <= 0 || H <= 0 || R < 0 || h0 <= 0 || w0 <= 0 || T != 1 + R + h0 * w0 || (layout != 0 && layout != 1)) return -1;
    if (norm && (!w || !b)) return -1;
    const size_t P = (size_t)h0 * w0;
    const size_t counts[3] = {(size_t)B * P * H, (size_t)B * H, (size_t)B * R * H};
    float* const host[3] = {patch_out, cls_out, reg_out};
    OpBuf dX, dW, dB, dO[3];
    OP_TRY(dX.upload(x, (size_t)B * T * H * 4));
    if (norm) {
        OP_TRY(dW.upload(w, (size_t)H * 4));
        OP_TRY(dB.upload(b, (size_t)H * 4));
    }
    for (int i = 0; i < 3; ++i)
        if (host[i]) OP_TRY(dO[i].alloc(counts[i], 4, OpBuf::nans(), (size_t)H));
    OP_TRY(launch_layer_tap(dX.as<float>(), dW.as<float>(), dB.as<float>(), eps, B, T, R, H, norm != 0, layout == 1, dO[0].as<float>(),
                            dO[1].as<float>(), dO[2].as<float>(), nullptr));
    OP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 3; ++i)
        if (host[i]) OP_FETCH(dO[i].fetch(host[i]));
    return 0;
}

extern "C" int dinov2_hip_op_attn_rows_ex(int32_t dtype, const float* qkv, int32_t B, int32_t T, int32_t H, int32_t nh, const int32_t* queries,
                                          int32_t nq, int32_t key0, int32_t nkeys, float* out, int64_t lds_budget) {
    const DType dt = dtype_of(dtype);
    if (!qkv || !queries || !out || B <= 0 || T <= 0 || nh <= 0 || H != nh * 64 || nq < 1 || nq > T || key0 < 0 || nkeys < 1 || key0 > T - nkeys)
        return -1;
    for (int i = 0; i < nq; ++i)
        if (queries[i] < 0 || queries[i] >= T || (i > 0 && queries[i] <= queries[i - 1])) return -1;
    OpBuf dQ, dI, dO;
    OP_TRY(dQ.upload_as(dt, qkv, (size_t)B * T * 3 * H));
    OP_TRY(dI.upload(queries, sizeof(int32_t) * (size_t)nq));
    OP_TRY(dO.alloc((size_t)B * nh * nq * nkeys, 4, OpBuf::nans(), (size_t)nkeys));
    if (lds_budget > 0)
        OP_TRY(launch_attn_rows_budget(dt, dQ.p, 3 * H, dO.as<float>(), B, T, H, nh, dI.as<int32_t>(), nq, key0, nkeys, (size_t)lds_budget, nullptr));
    else
        OP_TRY(launch_attn_rows(dt, dQ.p, 3 * H, dO.as<float>(), B, T, H, nh, dI.as<int32_t>(), nq, key0, nkeys, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dO.fetch(out);
}

extern "C" int dinov2_hip_op_attn_rows(int32_t dtype, const float* qkv, int32_t B, int32_t T, int32_t H, int32_t nh, const int32_t* queries,
                                       int32_t nq, int32_t key0, int32_t nkeys, float* out) {
    return dinov2_hip_op_attn_rows_ex(dtype, qkv, B, T, H, nh, queries, nq, key0, nkeys, out, 0);
}

extern "C" int dinov2_hip_op_convert_weight(int32_t dtype, const void* src, uint64_t src_bytes, uint32_t ggml_type,
                                            float* out, int32_t N, int32_t K, int32_t Kpad, int32_t interleaveF) {
    const DType dt = dtype_of(dtype);
    OpBuf dS, dO;
    OP_TRY(dS.upload(src, src_bytes));
    OP_TRY(dO.alloc((size_t)N * Kpad, 2, OpBuf::nans()));
    OP_TRY(launch_convert_weight(dt, dS.p, ggml_type, dO.p, N, K, Kpad, interleaveF, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dO.fetch_as(dt, out);
}

extern "C" int dinov2_hip_op_permute_bias(const float* src, float* dst, int32_t N, int32_t interleaveF) {
    if (!src || !dst || N <= 0 || interleaveF < 0 || (interleaveF > 0 && N != 2 * interleaveF)) return -1;
    OpBuf dS, dD;
    OP_TRY(dS.upload(src, (size_t)N * 4));
    OP_TRY(dD.alloc((size_t)N, 4, OpBuf::nans()));
    OP_TRY(launch_permute_bias(dS.as<float>(), dD.as<float>(), N, interleaveF, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dD.fetch(dst);
}

// launch_head as csrc/model.cpp runs it after the final LayerNorm, on host f32 data: W [C, 2H] rounded to the compute type as
// upload_as rounds it (nearest even), every output buffer NaN-filled first.
extern "C" int dinov2_hip_op_head(int32_t dtype, const float* fin, const float* W, const float* bias, float* feat, float* logits,
                                  float* probs, int32_t B, int32_t T, int32_t H, int32_t C, int32_t first, float inv_div) {
    // head_logits_kernel reads W and feat in 8-element pieces: 2H % 8 == 0
    if (!fin || !W || !bias || !feat || !logits || !probs || B <= 0 || T <= 0 || H <= 0 || H % 4 != 0 || C <= 0 || first < 0 || first > T)
        return -1;
    const DType dt = dtype_of(dtype);
    OpBuf dF, dW, dB, dFeat, dL, dP;
    OP_TRY(dF.upload(fin, (size_t)B * T * H * 4));
    OP_TRY(dW.upload_as(dt, W, (size_t)C * 2 * H));
    OP_TRY(dB.upload(bias, (size_t)C * 4));
    OP_TRY(dFeat.alloc((size_t)B * 2 * H, 4, OpBuf::nans()));
    OP_TRY(dL.alloc((size_t)B * C, 4, OpBuf::nans()));
    OP_TRY(dP.alloc((size_t)B * C, 4, OpBuf::nans()));
    OP_TRY(launch_head(dt, dF.as<float>(), dW.p, dB.as<float>(), dFeat.as<float>(), dL.as<float>(), dP.as<float>(), B, T, H, C, first, inv_div,
                       nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(dFeat.fetch(feat));
    OP_FETCH(dL.fetch(logits));
    return dP.fetch(probs);
}

extern "C" int dinov2_hip_op_probe_tr16(int16_t* out256) {
    OpBuf d;
    OP_TRY(d.alloc(256, 2, OpBuf::none()));
    OP_TRY(launch_probe_tr16(d.as<int16_t>(), nullptr));
    OP_TRY(hipDeviceSynchronize());
    return d.fetch(out256);
}

// ---- far operands: ONE launch of a GEMM or of attention whose operands end just below the launchers' 32-bit byte-offset limits.  Host
// operands of that size would take gigabytes and tens of seconds to round, so A / qkv (and a residual's initial contents) are written on the
// device from far_value (csrc/far_pattern.h); the caller gets the output rows it lists, the number of payload elements that still hold their
// initial bits, and DINOV2_HIP_OP_GUARD_CHANGED if a guard band changed -- all three found on the device. ----
namespace {

enum FarKind : int { FAR_F16 = 0, FAR_BF16 = 1, FAR_F32 = 2 };
constexpr int FAR_BLOCKS = 4096, FAR_THREADS = 256;

// p[r * ld + c] = far_value(seed, r, c) as `kind`, r < rows, c < cols; the gap cols .. ld of a row is left as it is
__global__ void far_fill_kernel(void* p, size_t rows, int cols, size_t ld, int kind, uint64_t seed) {
    const size_t n = rows * (size_t)cols, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const size_t r = i / (size_t)cols;
        const int c = (int)(i - r * (size_t)cols);
        const float v = far_value(seed, r, (uint32_t)c);
        const size_t at = r * ld + (size_t)c;
        if (kind == FAR_F32) {
            ((float*)p)[at] = v;
        } else if (kind == FAR_F16) {
            ((_Float16*)p)[at] = (_Float16)v;
        } else {
            ((uint16_t*)p)[at] = (uint16_t)(__float_as_uint(v) >> 16);  // exact: 7 significant bits
        }
    }
}

// *count += the payload elements (r < rows, c < cols at row stride ld) that still hold their initial bits: all-ones elements of esz bytes
// (pattern = 0), or the f32 pattern value of `seed` (pattern = 1, esz = 4)
__global__ void far_count_kernel(const void* p, size_t rows, int cols, size_t ld, int esz, int pattern, uint64_t seed, unsigned long long* count) {
    const size_t n = rows * (size_t)cols, step = (size_t)gridDim.x * blockDim.x;
    unsigned long long mine = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const size_t r = i / (size_t)cols;
        const int c = (int)(i - r * (size_t)cols);
        const size_t at = r * ld + (size_t)c;
        if (esz == 2) mine += ((const uint16_t*)p)[at] == 0xffffu;
        else if (!pattern) mine += ((const uint32_t*)p)[at] == 0xffffffffu;
        else mine += ((const uint32_t*)p)[at] == __float_as_uint(far_value(seed, r, (uint32_t)c));
    }
    if (mine) atomicAdd(count, mine);
}

// *count += the 32-bit words of [p, p + words) that are not all ones
__global__ void far_band_kernel(const uint32_t* p, size_t words, unsigned long long* count) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    unsigned long long mine = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += step) mine += p[i] != 0xffffffffu;
    if (mine) atomicAdd(count, mine);
}

// dst[i][0 .. units) = the first `units` two-byte units of row rows[i] of src (row stride ld_units two-byte units); one block per listed row
__global__ void far_gather_kernel(const uint16_t* src, size_t ld_units, const int64_t* rows, int units, uint16_t* dst) {
    const uint16_t* s = src + (size_t)rows[blockIdx.x] * ld_units;
    uint16_t* d = dst + (size_t)blockIdx.x * (size_t)units;
    for (int k = threadIdx.x; k < units; k += blockDim.x) d[k] = s[k];
}

// a refused allocation is an answer of its own (the caller asked hipMemGetInfo first and may skip on it), any other failure a HIP error
#define FAR_ALLOC(x)                                                          \
    do {                                                                      \
        const hipError_t e__ = (x);                                           \
        if (e__ == hipErrorOutOfMemory) {                                     \
            (void)hipGetLastError();                                          \
            return DINOV2_HIP_OP_NO_MEMORY;                                   \
        }                                                                     \
        if (e__ != hipSuccess) return -1;                                     \
    } while (0)

hipError_t far_fill(const OpBuf& b, size_t rows, int cols, size_t ld, int kind, uint64_t seed) {
    far_fill_kernel<<<FAR_BLOCKS, FAR_THREADS>>>(b.as<void>(), rows, cols, ld, kind, seed);
    return hipGetLastError();
}

// What both far ops end with.  out: [rows_all, ld] elements of esz bytes between guard bands, `width` payload columns.  0, -1,
// DINOV2_HIP_OP_GUARD_CHANGED; *untouched and the listed rows (widened to f32 when esz == 2) are written on 0 only.
int far_collect(const OpBuf& out, DType dt, size_t rows_all, int width, size_t ld, int pattern, uint64_t seed_o, const int64_t* rows, int nrows,
                float* out_rows, int64_t* untouched) {
    OpBuf dCnt, dRows, dG;
    OP_TRY(dCnt.alloc(2, 8, OpBuf::zeros()));
    unsigned long long* cnt = dCnt.as<unsigned long long>();
    const size_t band_words = out.ng * out.esz / 4;
    if (band_words) {
        far_band_kernel<<<FAR_BLOCKS, FAR_THREADS>>>((const uint32_t*)out.p, band_words, cnt);
        far_band_kernel<<<FAR_BLOCKS, FAR_THREADS>>>((const uint32_t*)(out.as<char>() + out.n * out.esz), band_words, cnt);
    }
    far_count_kernel<<<FAR_BLOCKS, FAR_THREADS>>>(out.as<void>(), rows_all, width, ld, (int)out.esz, pattern, seed_o, cnt + 1);
    OP_TRY(hipGetLastError());
    const int units = width * (int)out.esz / 2;
    OP_TRY(dRows.upload(rows, sizeof(int64_t) * (size_t)nrows));
    OP_TRY(dG.alloc((size_t)nrows * units, 2, OpBuf::nans()));
    far_gather_kernel<<<nrows, FAR_THREADS>>>(out.as<uint16_t>(), ld * out.esz / 2, dRows.as<int64_t>(), units, dG.as<uint16_t>());
    OP_TRY(hipGetLastError());
    OP_TRY(hipDeviceSynchronize());
    unsigned long long c[2] = {0, 0};
    OP_TRY(dCnt.read(c, 0, sizeof(c)));
    if (c[0]) return DINOV2_HIP_OP_GUARD_CHANGED;
    *untouched = (int64_t)c[1];
    if (out.esz == 4) return dG.fetch(out_rows);
    std::vector<uint16_t> raw((size_t)nrows * units);
    OP_FETCH(dG.fetch(raw.data()));
    widen_to_f32(dt == DT_BF16, raw.data(), raw.size(), out_rows);
    return 0;
}

bool far_rows_ok(const int64_t* rows, int nrows, int64_t limit) {
    if (!rows || nrows <= 0 || nrows > (1 << 20)) return false;
    for (int i = 0; i < nrows; ++i)
        if (rows[i] < 0 || rows[i] >= limit) return false;
    return true;
}

}  // namespace

extern "C" int dinov2_hip_op_device_memory(int64_t* free_bytes, int64_t* total_bytes) {
    size_t f = 0, t = 0;
    OP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return 0;
}

extern "C" int dinov2_hip_op_gemm_far(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldo,
                                      uint64_t seed_a, uint64_t seed_out, const float* W, const float* bias, const float* aux, int32_t qcols,
                                      float qscale, const int64_t* rows, int32_t nrows, float* out_rows, int64_t* untouched) {
    const DType dt = dtype_of(dtype);
    if (epilogue < EPI_QKV || epilogue > EPI_PLAIN_F32 || M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || !W || !out_rows || !untouched ||
        !far_rows_ok(rows, nrows, M))
        return DINOV2_HIP_ERR_INVALID;
    const int width = epilogue == EPI_SWIGLU ? N / 2 : N;
    if (ldo < width || (epilogue == EPI_RESID && !aux)) return DINOV2_HIP_ERR_INVALID;
    {  // the planner's own refusal (the strides included), before anything is allocated
        GemmArgs q{};
        q.M = M; q.N = N; q.K = K; q.lda = lda; q.ldw = ldw; q.ldo = ldo; q.P = 1; q.T = 2; q.qcols = qcols;
        GemmPlan plan;
        if (gemm_plan(dt, (Epilogue)epilogue, q, false, &plan) != hipSuccess) return DINOV2_HIP_ERR_INVALID;
    }
    if (gemm_init() != hipSuccess) return -1;
    const bool f32out = epilogue == EPI_RESID || epilogue == EPI_PLAIN_F32;
    OpBuf dA, dW, dB, dX, dO;
    FAR_ALLOC(dA.alloc((size_t)M * lda, 2, OpBuf::nans()));  // the gap K .. lda of every row stays NaN
    OP_TRY(far_fill(dA, (size_t)M, K, (size_t)lda, dt == DT_BF16 ? FAR_BF16 : FAR_F16, seed_a));
    if (ldw == K) {
        FAR_ALLOC(dW.upload_as(dt, W, (size_t)N * K));
    } else {
        std::vector<uint16_t> w((size_t)N * K);
        for (size_t i = 0; i < w.size(); ++i) w[i] = OpBuf::round_to(dt, W[i]);
        FAR_ALLOC(dW.alloc((size_t)N * ldw, 2, OpBuf::nans()));
        OP_TRY(hipMemcpy2D(dW.p, (size_t)ldw * 2, w.data(), (size_t)K * 2, (size_t)K * 2, (size_t)N, hipMemcpyHostToDevice));
    }
    if (bias) OP_TRY(dB.upload(bias, sizeof(float) * N));
    if (aux) OP_TRY(dX.upload(aux, sizeof(float) * N));
    FAR_ALLOC(dO.alloc((size_t)M * ldo, f32out ? 4 : 2, OpBuf::nans(), (size_t)ldo));
    if (epilogue == EPI_RESID) OP_TRY(far_fill(dO, (size_t)M, width, (size_t)ldo, FAR_F32, seed_out));
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.bias = dB.as<float>(); a.out = dO.as<void>(); a.aux = dX.as<float>();
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldo = ldo; a.P = 1; a.T = 2; a.qcols = qcols; a.qscale = qscale;
    OP_TRY(launch_gemm(dt, (Epilogue)epilogue, a, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return far_collect(dO, dt, (size_t)M, width, (size_t)ldo, epilogue == EPI_RESID, seed_out, rows, nrows, out_rows, untouched);
}

extern "C" int dinov2_hip_op_attention_far(int32_t dtype, int32_t B, int32_t T, int32_t nh, uint64_t seed, int32_t log2_scores, const int64_t* rows,
                                           int32_t nrows, float* out_rows, int64_t* untouched) {
    const DType dt = dtype_of(dtype);
    if (B <= 0 || T <= 0 || nh <= 0 || nh > 64 || !out_rows || !untouched || (int64_t)B * T > (int64_t)INT32_MAX ||
        !far_rows_ok(rows, nrows, (int64_t)B * T))
        return DINOV2_HIP_ERR_INVALID;
    const int H = 64 * nh;
    if ((size_t)B * T * 3 * H * 2 >= ((size_t)1 << 32)) return DINOV2_HIP_ERR_INVALID;  // launch_attention's own refusal, before anything is allocated
    const size_t M = (size_t)B * T;
    OpBuf dQ, dO;
    FAR_ALLOC(dQ.alloc(M * 3 * H, 2, OpBuf::nans()));
    OP_TRY(far_fill(dQ, M, 3 * H, (size_t)3 * H, dt == DT_BF16 ? FAR_BF16 : FAR_F16, seed));
    FAR_ALLOC(dO.alloc(M * H, 2, OpBuf::nans(), (size_t)H));
    OP_TRY(launch_attention(dt, dQ.p, dO.as<void>(), B, T, H, nh, log2_scores != 0, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return far_collect(dO, dt, M, H, (size_t)H, 0, 0, rows, nrows, out_rows, untouched);
}

// ---- far rows: rows [row0, row0 + n) of an operand whose row r is dictionary entry far_rows_entry(seed, r, ...) (csrc/far_pattern.h), written
// into the CALLER's device buffer, for the resident-rows entry points (match, bank, k-means) at the far end of their row offsets ----
namespace {

// dst[r * ld + c] = dict[entry(row0 + r) * H + c], r < n, c < H; one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void rows_fill_kernel(float* __restrict__ dst, size_t ld, uint64_t row0, size_t n, int H,
                                                        const float* __restrict__ dict, int d_common, uint64_t seed,
                                                        const int64_t* __restrict__ plant_rows, const int32_t* __restrict__ plant_entries,
                                                        int nplants) {
    const int lane = threadIdx.x & 63;
    const size_t step = (size_t)gridDim.x * 4;
    for (size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += step) {
        const int e = far_rows_entry(seed, row0 + r, d_common, plant_rows, plant_entries, nplants);
        const float* const src = dict + (size_t)e * (size_t)H;
        float* const out = dst + r * ld;
        for (int c = lane; c < H; c += 64) out[c] = src[c];
    }
}

}  // namespace

extern "C" int dinov2_hip_op_rows_fill(float* dst_dev, int64_t ld, int64_t row0, int64_t n, int32_t H, const float* dict, int32_t D,
                                       int32_t d_common, uint64_t seed, const int64_t* plant_rows, const int32_t* plant_entries,
                                       int32_t nplants) {
    if (!dst_dev || ((size_t)dst_dev & 3) != 0 || !dict || H < 1 || H > 4096 || ld < H || row0 < 0 || n < 1 || n > ((int64_t)1 << 32) ||
        D < 1 || D > 16384 || d_common < 1 || d_common > D || nplants < 0 || nplants > 256 || (nplants > 0 && (!plant_rows || !plant_entries)))
        return DINOV2_HIP_ERR_INVALID;
    for (int i = 0; i < nplants; ++i)
        if (plant_rows[i] < 0 || (i > 0 && plant_rows[i] <= plant_rows[i - 1]) || plant_entries[i] < 0 || plant_entries[i] >= D)
            return DINOV2_HIP_ERR_INVALID;
    OpBuf dD, dR, dE;
    OP_TRY(dD.upload(dict, sizeof(float) * (size_t)D * H));
    if (nplants > 0) {
        OP_TRY(dR.upload(plant_rows, sizeof(int64_t) * nplants));
        OP_TRY(dE.upload(plant_entries, sizeof(int32_t) * nplants));
    }
    const size_t groups = ((size_t)n + 3) / 4;
    const unsigned blocks = (unsigned)(groups < ((size_t)1 << 20) ? groups : ((size_t)1 << 20));
    rows_fill_kernel<<<blocks, 256>>>(dst_dev, (size_t)ld, (uint64_t)row0, (size_t)n, H, dD.as<float>(), d_common, seed, dR.as<int64_t>(),
                                      dE.as<int32_t>(), nplants);
    OP_TRY(hipGetLastError());
    OP_TRY(hipDeviceSynchronize());
    return 0;
}

// ---- micro-benchmarks: device-resident random operands, HIP-event timing around `iters` launches ----
namespace {
// the two events a timed loop sits between, destroyed on return
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() {
        const hipError_t e = hipEventCreate(&e0);
        return e != hipSuccess ? e : hipEventCreate(&e1);
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// ms per launch of `iters` launches after ~100 ms of them (a cold GPU runs the first milliseconds at a fraction of its sustained clock);
// -1 if the device reports an error at the end.  The launches themselves are not checked.
template <typename Launch>
float time_launches(int iters, Launch launch) {
    EventPair ev;
    (void)ev.create();
    for (auto t0 = std::chrono::steady_clock::now(); std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(100);) {
        for (int i = 0; i < 10; ++i) (void)launch();
        (void)hipDeviceSynchronize();
    }
    (void)hipEventRecord(ev.e0, nullptr);
    for (int i = 0; i < iters; ++i) (void)launch();
    (void)hipEventRecord(ev.e1, nullptr);
    if (hipEventSynchronize(ev.e1) != hipSuccess) return -1.f;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.e0, ev.e1);
    return ms / iters;
}
}  // namespace

extern "C" float dinov2_hip_op_gemm_bench(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t iters) {
    const DType dt = dtype_of(dtype);
    if (gemm_init() != hipSuccess) return -1.f;
    OpBuf dA, dW, dB, dX, dO;
    // extra elements per row of A / W (row strides K + pad instead of the dense K): 0 in normal use; profiles/r02_gemm_kloop.md
    // measured 64 (= 128 bytes) as neutral, i.e. no power-of-two-stride channel conflict to pad away
    const int padA = 0, padW = 0;
    // EPI_PATCH writes token rows (image b, patch p) -> row b * T + 1 + R + p and reads the position embedding [1 + P, N]: shaped like the model
    // (P = 1369 patches, 4 registers) when M is a multiple of 1369, one "image" of M patches otherwise
    const int pP = epilogue == EPI_PATCH ? (M % 1369 == 0 ? 1369 : M) : 1, pR = epilogue == EPI_PATCH && M % 1369 == 0 ? 4 : 0;
    const int pT = pP + 1 + pR;
    const size_t out_elems = epilogue == EPI_PATCH ? (size_t)(M / pP) * pT * N : (size_t)M * N;
    const size_t aux_elems = epilogue == EPI_PATCH ? (size_t)(pP + 1) * N : (size_t)std::max(N, 4096) * 2;
    if (dA.alloc_random(dt, (size_t)M * (K + padA), 1, 1.0f) != hipSuccess || dW.alloc_random(dt, (size_t)N * (K + padW), 2, 0.05f) != hipSuccess ||
        dB.alloc((size_t)N, 4, OpBuf::none()) != hipSuccess || dX.alloc(aux_elems, 4, OpBuf::none()) != hipSuccess ||
        dO.alloc(out_elems, 4, OpBuf::none()) != hipSuccess)
        return -1.f;
    (void)hipMemset(dB.p, 0, (size_t)N * 4);
    (void)hipMemset(dX.p, 0, aux_elems * 4);
    (void)hipMemset(dO.p, 0, out_elems * 4);
    GemmArgs a{};
    a.A = dA.p; a.W = dW.p; a.bias = dB.as<float>(); a.out = dO.p; a.aux = dX.as<float>();
    a.M = M; a.N = N; a.K = K; a.ldo = epilogue == EPI_SWIGLU ? N / 2 : N; a.P = 1; a.T = 2; a.R = 0;
    a.lda = K + padA; a.ldw = K + padW;
    a.qcols = N / 3; a.qscale = 0.125f;
    if (epilogue == EPI_PATCH) { a.P = pP; a.T = pT; a.R = pR; }
    OpBuf dSt, dXg, dV;
    if (epilogue >= EPI_RESID_LN) {  // LN fold: statistics of unit-variance rows, gamma = 1, s = 0, c = 0
        const int hc = epilogue == EPI_RESID_LN ? N : K;
        const int gs = ln_stat_slots(hc), groups = hc / LN_GROUP;
        std::vector<float> st((size_t)M * gs * 2, 0.f), ones((size_t)std::max(N, K), 1.0f);
        for (int m = 0; m < M; ++m)
            for (int g = 0; g < groups; ++g) st[((size_t)m * gs + g) * 2 + 1] = 64.0f;
        if (dSt.alloc(st.size(), 4, OpBuf::none()) != hipSuccess || dXg.alloc((size_t)M * N, 2, OpBuf::none()) != hipSuccess ||
            dV.alloc(ones.size(), 4, OpBuf::none()) != hipSuccess)
            return -1.f;
        (void)hipMemcpy(dSt.p, st.data(), st.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(dV.p, ones.data(), ones.size() * 4, hipMemcpyHostToDevice);
        a.stats = dSt.as<float>(); a.ln_gs = gs; a.ln_eps = 1e-6f;
        a.ln_gamma = dV.as<float>(); a.xg = dXg.p;
        a.ln_s = dB.as<float>(); a.ln_c = dB.as<float>();  // zeros
        if (epilogue == EPI_SWIGLU_LN) a.ldo = N / 2;
    }
    return time_launches(iters, [&] { return launch_gemm(dt, (Epilogue)epilogue, a, nullptr); });
}

extern "C" float dinov2_hip_op_attention_bench(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t nh, int32_t iters) {
    const DType dt = dtype_of(dtype);
    OpBuf dQ, dO;
    const size_t nq = (size_t)B * T * 3 * H, no = (size_t)B * T * H;
    if (dQ.alloc_random(dt, nq, 3, 1.0f) != hipSuccess || dO.alloc(no, 2, OpBuf::none()) != hipSuccess) return -1.f;
    return time_launches(iters, [&] { return launch_attention(dt, dQ.p, dO.p, B, T, H, nh, true, nullptr); });
}

// ---- testing aids: the tuning switches (read from the environment once) and the dispatcher's plan for a shape ----
namespace {
int tune_key(const char* key) {  // the TuneKey of a switch's name, -1 if there is none
    static const char* const names[TUNE_COUNT] = {"gemm_gen", "gemm_tile", "attn_v", "attn_nwv", "list_order"};
    for (int k = 0; key && k < TUNE_COUNT; ++k)
        if (std::strcmp(key, names[k]) == 0) return k;
    return -1;
}
}  // namespace
extern "C" int dinov2_hip_op_set_tuning(const char* key, int32_t value) {
    const int k = tune_key(key);
    if (k < 0) return DINOV2_HIP_ERR_INVALID;
    tune_set((TuneKey)k, value);
    return DINOV2_HIP_OK;
}
extern "C" int dinov2_hip_op_get_tuning(const char* key) {
    const int k = tune_key(key);
    return k < 0 ? -1 : tune_get((TuneKey)k);
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
    return gemm_plan_describe(dtype_of(dtype), (Epilogue)epilogue, a, out, (size_t)cap) == hipSuccess ? DINOV2_HIP_OK : DINOV2_HIP_ERR_INVALID;
}
// ... with row strides of A and W (0 = K): what stamp_args refuses of them is refused here
extern "C" int dinov2_hip_op_gemm_plan_strided(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, char* out,
                                               int32_t cap) {
    if (!out || cap <= 0 || epilogue < 0 || epilogue > EPI_SWIGLU_LN) return DINOV2_HIP_ERR_INVALID;
    GemmArgs a = plan_query_args(epilogue, M, N, K);
    a.lda = lda; a.ldw = ldw;
    return gemm_plan_describe(dtype_of(dtype), (Epilogue)epilogue, a, out, (size_t)cap) == hipSuccess ? DINOV2_HIP_OK : DINOV2_HIP_ERR_INVALID;
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
    if (gemm_plan(dtype_of(dtype), (Epilogue)epilogue, a, false, &plan) != hipSuccess) return -1;
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

// host-only: the Rayleigh-Ritz step behind dinov2_hip_pca3 (pca_ritz, csrc/pca.cpp), for the CPU test-suite
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
    OpBuf dS, dD;
    OP_TRY(dS.upload(bgr, (size_t)B * h * w * 3));
    OP_TRY(dD.alloc((size_t)B * oh * ow * 3, 4, OpBuf::nans()));
    const int rh = mode == 1 ? 256 : oh, rw = mode == 1 ? 256 : ow;
    OP_TRY(launch_preprocess_u8(dS.as<uint8_t>(), dD.as<float>(), B, h, w, rh, rw, (rh - oh) / 2, (rw - ow) / 2, oh, ow, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dD.fetch(out);
}

// match_normalise_kernel + match_kernel + match_reduce_kernel (csrc/match.hip) on host data, as dinov2_hip_match_tokens runs them
extern "C" int dinov2_hip_op_match(const float* a, int32_t na, const float* b, int32_t nb, int32_t H, int32_t* idx_ab, float* sim_ab,
                                   int32_t* idx_ba, float* sim_ba) {
    if (!a || !b || !idx_ab || !sim_ab || !idx_ba || !sim_ba || na < 1 || na > (1 << 20) || nb < 1 || nb > (1 << 20) || H < 8 || H > 4096)
        return DINOV2_HIP_ERR_INVALID;
    const MatchPlan plan = match_plan(na, nb, H);
    OpBuf dA, dB, dW;
    OP_TRY(dA.upload(a, (size_t)na * H * 4));
    OP_TRY(dB.upload(b, (size_t)nb * H * 4));
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::nans()));
    OP_TRY(launch_match(dA.as<float>(), (size_t)H, dB.as<float>(), (size_t)H, na, nb, H, dW.as<char>(), plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(dW.read(idx_ab, plan.idx_ab, (size_t)na * 4));
    OP_TRY(dW.read(sim_ab, plan.sim_ab, (size_t)na * 4));
    OP_TRY(dW.read(idx_ba, plan.idx_ba, (size_t)nb * 4));
    OP_TRY(dW.read(sim_ba, plan.sim_ba, (size_t)nb * 4));
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
    OpBuf dQ, dB, dBank, dW;
    OP_TRY(dQ.upload(q, (size_t)nq * H * 4));
    OP_TRY(dB.upload(b, (size_t)nb * H * 4));
    OP_TRY(dBank.alloc((size_t)plan.ntiles * MATCH_TN * plan.hpad, 2, OpBuf::nans()));  // rows past nb stay NaN: the sweep must mask them
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::nans()));
    OP_TRY(launch_match_normalise(dB.as<float>(), (size_t)H, dBank.as<_Float16>(), nb, nb, H, plan.hpad, nullptr));
    OP_TRY(launch_bank_topk(dQ.as<float>(), (size_t)H, nq, dBank.as<_Float16>(), nb, H, k, dW.as<char>(), plan, false, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(dW.read(idx, plan.idx, (size_t)nq * k * 4));
    OP_TRY(dW.read(sim, plan.sim, (size_t)nq * k * 4));
    return 0;
}
extern "C" int dinov2_hip_op_bank_bench(const float* q_dev, int32_t nq, const float* b_dev, int32_t nb, int32_t H, int32_t k,
                                        int32_t chunk_tiles, int32_t warmup, int32_t iters, int32_t floor_only, float* ms) {
    if (!q_dev || !b_dev || !ms || !bank_shape_ok(nq, nb, H, k) || chunk_tiles < 0 || warmup < 0 || iters < 1) return DINOV2_HIP_ERR_INVALID;
    const BankTopkPlan plan = bank_topk_plan(nq, nb, H, k, chunk_tiles);
    OpBuf dBank, dW;
    EventPair ev;
    OP_TRY(dBank.alloc((size_t)plan.ntiles * MATCH_TN * plan.hpad, 2, OpBuf::zeros()));
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::none()));
    OP_TRY(launch_match_normalise(b_dev, (size_t)H, dBank.as<_Float16>(), nb, nb, H, plan.hpad, nullptr));
    OP_TRY(ev.create());
    int rc = 0;
    for (int i = 0; i < warmup + iters && rc == 0; ++i) {
        if (i == warmup && hipEventRecord(ev.e0, nullptr) != hipSuccess) rc = -1;
        if (launch_bank_topk(q_dev, (size_t)H, nq, dBank.as<_Float16>(), nb, H, k, dW.as<char>(), plan, floor_only != 0, nullptr) != hipSuccess) rc = -1;
    }
    float t = 0.0f;
    if (rc == 0 && (hipEventRecord(ev.e1, nullptr) != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess ||
                    hipEventElapsedTime(&t, ev.e0, ev.e1) != hipSuccess))
        rc = -1;
    (void)hipDeviceSynchronize();
    *ms = t / (float)iters;
    return rc;
}

// ---- dinov2_hip_propagate's kernels (csrc/propagate.hip) on host data: a memory of `frames` slots is built by the shared normaliser, then
// ---- swept, merged and combined ----
namespace {
bool propagate_shape_ok(int h0, int w0, int H, int frames, int C, uint64_t slots, int radius, int k, float T) {
    if (h0 < 1 || h0 > PROP_GRID_MAX || w0 < 1 || w0 > PROP_GRID_MAX || H < 8 || H > 4096 || frames < 1 || frames > PROP_FRAMES_MAX || C < 1 ||
        C > PROP_C_MAX || k < 1 || k > BANK_K_MAX || radius < -1 || radius > PROP_RADIUS_MAX)
        return false;
    const int ppad = (h0 * w0 + MATCH_TN - 1) / MATCH_TN * MATCH_TN;
    if ((int64_t)frames * ppad > PROP_ROWS_MAX) return false;
    if (slots == 0 || (frames < 64 && (slots >> frames) != 0)) return false;
    return T >= 1e-3f && T <= 1e3f;
}
// The memory of one diagnostic call: `fill` bytes everywhere, then the cell table and the rows of every slot normalised into their places
// (the padding rows of a slot keep the fill)
struct PropOpMem {
    OpBuf dev;
    PropMemLayout lay{};
    PropMemView view{};
    hipError_t build(const float* rows_dev, const float* labels_host, int h0, int w0, int H, int frames, int C, const PropagatePlan& plan,
                     OpBuf::Fill fill) {
        const int P = plan.P;
        lay = propmem_layout(frames, P, plan.ppad, plan.hpad, C);
        hipError_t e = dev.alloc(lay.bytes, 1, fill);
        if (e != hipSuccess) return e;
        char* const d = dev.as<char>();
        std::vector<uint32_t> cells((size_t)plan.ppad, 0u);
        for (int p = 0; p < P; ++p) cells[p] = propagate_cell(p, w0);
        e = hipMemcpy(d + lay.cells, cells.data(), cells.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && labels_host) e = hipMemcpy(d + lay.labels, labels_host, (size_t)frames * P * C * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && !labels_host) e = hipMemset(d + lay.labels, 0, (size_t)frames * P * C * 4);
        for (int f = 0; f < frames && e == hipSuccess; ++f)
            e = launch_match_normalise(rows_dev + (size_t)f * P * H, (size_t)H, (_Float16*)(d + lay.rows) + (size_t)f * plan.ppad * plan.hpad, P, P, H,
                                       plan.hpad, nullptr);
        view = PropMemView{(const _Float16*)(d + lay.rows), (const float*)(d + lay.labels), (float*)(d + lay.kept), (const uint32_t*)(d + lay.cells),
                           h0, w0, C};
        return e;
    }
};
}  // namespace
extern "C" int dinov2_hip_op_propagate_plan(int32_t h0, int32_t w0, int32_t H, int32_t nactive, int32_t radius, int32_t k, int32_t C,
                                            int32_t chunk_tiles, int64_t* out, int32_t* ranges) {
    if (!out || nactive < 1 || nactive > PROP_FRAMES_MAX || chunk_tiles < 0 ||
        !propagate_shape_ok(h0, w0, H, nactive, C, 1, radius, k, 1.0f))
        return DINOV2_HIP_ERR_INVALID;
    const PropagatePlan p = propagate_plan(h0, w0, H, nactive, radius, k, C, chunk_tiles);
    out[0] = p.chunk_tiles;
    out[1] = p.nchunks;
    out[2] = p.qtiles;
    out[3] = p.max_items;
    out[4] = p.kept_items;
    out[5] = (int64_t)((size_t)p.nchunks * p.ppad * k * sizeof(BankEntry));
    out[6] = (int64_t)p.bytes;
    out[7] = (int64_t)propmem_layout(nactive, p.P, p.ppad, p.hpad, C).bytes;
    for (int qt = 0; ranges && qt < p.qtiles; ++qt) {
        int t0, t1;
        propagate_tile_range(qt, p.P, w0, radius, &t0, &t1);
        ranges[2 * qt] = t0;
        ranges[2 * qt + 1] = t1;
    }
    return 0;
}
extern "C" int dinov2_hip_op_propagate(const float* q, const float* rows, const float* labels, int32_t h0, int32_t w0, int32_t H, int32_t frames,
                                       int32_t C, uint64_t slots, int32_t radius, int32_t k, float temperature, int32_t chunk_tiles, float* out,
                                       int32_t* argmax, int32_t* idx, float* sim, float* kept) {
    if (!q || !rows || !labels || !out || !argmax || !idx || !sim || chunk_tiles < 0 ||
        !propagate_shape_ok(h0, w0, H, frames, C, slots, radius, k, temperature))
        return DINOV2_HIP_ERR_INVALID;
    const PropagatePlan plan = propagate_plan(h0, w0, H, __builtin_popcountll(slots), radius, k, C, chunk_tiles);
    const int P = plan.P;
    OpBuf dQ, dR, dW;
    PropOpMem mem;
    OP_TRY(dQ.upload(q, (size_t)P * H * 4));
    OP_TRY(dR.upload(rows, (size_t)frames * P * H * 4));
    OP_TRY(mem.build(dR.as<float>(), labels, h0, w0, H, frames, C, plan, OpBuf::nans()));  // padding rows stay NaN: the sweep must mask them
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::nans()));
    OP_TRY(launch_propagate(dQ.as<float>(), (size_t)H, H, mem.view, slots, radius, k, temperature, kept != nullptr, dW.as<char>(), plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_TRY(dW.read(out, plan.out, (size_t)P * C * 4));
    OP_TRY(dW.read(argmax, plan.argmax, (size_t)P * 4));
    OP_TRY(dW.read(idx, plan.idx, (size_t)P * k * 4));
    OP_TRY(dW.read(sim, plan.sim, (size_t)P * k * 4));
    if (kept) OP_TRY(mem.dev.read(kept, mem.lay.kept, (size_t)P * C * 4));
    return 0;
}
extern "C" int dinov2_hip_op_propagate_bench(const float* q_dev, const float* rows_dev, int32_t h0, int32_t w0, int32_t H, int32_t frames, int32_t C,
                                             uint64_t slots, int32_t radius, int32_t k, float temperature, int32_t chunk_tiles, int32_t warmup,
                                             int32_t iters, float* ms) {
    if (!q_dev || !rows_dev || !ms || chunk_tiles < 0 || warmup < 0 || iters < 1 ||
        !propagate_shape_ok(h0, w0, H, frames, C, slots, radius, k, temperature))
        return DINOV2_HIP_ERR_INVALID;
    const PropagatePlan plan = propagate_plan(h0, w0, H, __builtin_popcountll(slots), radius, k, C, chunk_tiles);
    OpBuf dW;
    PropOpMem mem;
    EventPair ev;
    OP_TRY(mem.build(rows_dev, nullptr, h0, w0, H, frames, C, plan, OpBuf::zeros()));
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::none()));
    OP_TRY(ev.create());
    int rc = 0;
    for (int i = 0; i < warmup + iters && rc == 0; ++i) {
        if (i == warmup && hipEventRecord(ev.e0, nullptr) != hipSuccess) rc = -1;
        if (launch_propagate(q_dev, (size_t)H, H, mem.view, slots, radius, k, temperature, true, dW.as<char>(), plan, nullptr) != hipSuccess) rc = -1;
    }
    float t = 0.0f;
    if (rc == 0 && (hipEventRecord(ev.e1, nullptr) != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess ||
                    hipEventElapsedTime(&t, ev.e0, ev.e1) != hipSuccess))
        rc = -1;
    (void)hipDeviceSynchronize();
    *ms = t / (float)iters;
    return rc;
}

// ---- dinov2_hip_kmeans_tokens' kernels (csrc/kmeans.hip) on host data ----
namespace {
bool kmeans_shape_ok(int n, int K, int H) { return n >= 1 && n <= KMEANS_N_MAX && K >= 1 && K <= KMEANS_K_MAX && H >= 8 && H <= 4096; }
// The buffers of one run, each an allocation of its own that starts as 0xff bytes; the four results between guard bands.
struct KmeansOpBufs {
    OpBuf x16, xt, c16, cvec, labels, sim, part, cpart, counts, chpart, changed;
    KmeansBufs b{};
    hipError_t alloc(int K, int H, const KmeansPlan& p) {
        const struct { OpBuf* buf; size_t n, esz, guard; } all[] = {
            {&x16, (size_t)p.npad * p.hpad, 2, 0}, {&xt, (size_t)p.hpad128 * p.npad, 2, 0}, {&c16, (size_t)p.kpad * p.hpad, 2, 0},
            {&cvec, (size_t)K * H, 4, (size_t)H}, {&labels, (size_t)p.npad, 4, 1}, {&sim, (size_t)p.npad, 4, 1},
            {&part, p.part_bytes / 4, 4, 0}, {&cpart, (size_t)p.nsplit * p.kpad, 4, 0}, {&counts, (size_t)p.kpad, 4, 1},
            {&chpart, (size_t)p.npad / 128, 4, 0}, {&changed, 1, 4, 0}};
        for (const auto& a : all) {
            const hipError_t e = a.buf->alloc(a.n, a.esz, OpBuf::nans(), a.guard);
            if (e != hipSuccess) return e;
        }
        b.x16 = x16.as<_Float16>(); b.xt = xt.as<_Float16>(); b.c16 = c16.as<_Float16>(); b.cvec = cvec.as<float>();
        b.labels = labels.as<int>(); b.sim = sim.as<float>(); b.part = part.as<float>(); b.cpart = cpart.as<int>();
        b.counts = counts.as<int>(); b.chpart = chpart.as<int>(); b.changed = changed.as<int>();
        return hipSuccess;
    }
    // the first `count` elements of a guarded buffer to `host` (nothing for a NULL host)
    template <typename T>
    static int head(const OpBuf& buf, T* host, size_t count) {
        if (!host) return 0;
        std::vector<T> all(buf.n);
        const int rc = buf.fetch(all.data());
        if (rc == 0) std::copy(all.begin(), all.begin() + count, host);
        return rc;
    }
};
}  // namespace

extern "C" int dinov2_hip_op_kmeans_plan(int32_t n, int32_t K, int32_t H, int32_t nsplit, int64_t* out) {
    if (!out || !kmeans_shape_ok(n, K, H) || nsplit < 0) return DINOV2_HIP_ERR_INVALID;
    const KmeansPlan p = kmeans_plan(n, K, H, nsplit);
    const int64_t v[8] = {p.npad, p.kpad, p.hpad, p.hpad128, p.chunk, p.nsplit, (int64_t)p.part_bytes, (int64_t)p.bytes};
    std::copy(v, v + 8, out);
    return 0;
}

extern "C" int dinov2_hip_op_kmeans_assign(const float* rows, int32_t n, const float* centers, int32_t K, int32_t H, int32_t* labels, float* sim) {
    if (!rows || !centers || !labels || !sim || !kmeans_shape_ok(n, K, H)) return DINOV2_HIP_ERR_INVALID;
    const KmeansPlan plan = kmeans_plan(n, K, H, 0);
    OpBuf dX, dC;
    KmeansOpBufs w;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(dC.upload(centers, (size_t)K * H * 4));
    OP_TRY(w.alloc(K, H, plan));
    OP_TRY(launch_match_normalise(dX.as<float>(), (size_t)H, w.b.x16, n, plan.npad, H, plan.hpad, nullptr));
    OP_TRY(launch_match_normalise(dC.as<float>(), (size_t)H, w.b.c16, K, plan.kpad, H, plan.hpad, nullptr));
    OP_TRY(launch_kmeans_assign(w.b, n, K, plan, true, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(KmeansOpBufs::head(w.labels, labels, (size_t)n));
    return KmeansOpBufs::head(w.sim, sim, (size_t)n);
}

extern "C" int dinov2_hip_op_kmeans_update(const float* rows, int32_t n, const int32_t* labels_in, int32_t K, int32_t H, int32_t nsplit,
                                           const float* prev_centers, float* centers_out, int32_t* counts, float* xhat_f16_as_f32) {
    if (!rows || !labels_in || !prev_centers || !centers_out || !counts || !kmeans_shape_ok(n, K, H) || nsplit < 0) return DINOV2_HIP_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (labels_in[i] < 0 || labels_in[i] >= K) return DINOV2_HIP_ERR_INVALID;
    const KmeansPlan plan = kmeans_plan(n, K, H, nsplit);
    OpBuf dX;
    KmeansOpBufs w;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(w.alloc(K, H, plan));
    std::vector<int32_t> lab((size_t)plan.npad, -1);  // as the assignment leaves them
    std::copy(labels_in, labels_in + n, lab.begin());
    OP_TRY(hipMemcpy(w.b.labels, lab.data(), lab.size() * 4, hipMemcpyHostToDevice));
    OP_TRY(hipMemcpy(w.b.cvec, prev_centers, (size_t)K * H * 4, hipMemcpyHostToDevice));
    OP_TRY(launch_match_normalise(dX.as<float>(), (size_t)H, w.b.x16, n, plan.npad, H, plan.hpad, nullptr));
    OP_TRY(launch_kmeans_transpose(w.b, plan, nullptr));
    OP_TRY(launch_kmeans_update(w.b, K, H, plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(w.cvec.fetch(centers_out));
    OP_FETCH(KmeansOpBufs::head(w.counts, counts, (size_t)K));
    OP_FETCH(w.labels.fetch(lab.data()));  // (its guards)
    if (xhat_f16_as_f32) {
        std::vector<uint16_t> x16((size_t)plan.npad * plan.hpad);
        OP_TRY(w.x16.read(x16.data(), 0, x16.size() * 2));
        for (int i = 0; i < n; ++i) widen_to_f32(false, (const unsigned char*)(x16.data() + (size_t)i * plan.hpad), (size_t)H, xhat_f16_as_f32 + (size_t)i * H);
    }
    return 0;
}

extern "C" int dinov2_hip_op_kmeans(const float* rows, int32_t n, int32_t K, int32_t H, int32_t max_iter, const float* init_centers,
                                    const int32_t* init_rows, int32_t* labels, float* sim, float* centers, int32_t* counts, int32_t* iterations,
                                    int32_t* converged) {
    if (!rows || (!init_centers && !init_rows) || !kmeans_shape_ok(n, K, H) || max_iter < 0 || max_iter > KMEANS_ITER_MAX) return DINOV2_HIP_ERR_INVALID;
    for (int j = 0; !init_centers && j < K; ++j)
        if (init_rows[j] < 0 || init_rows[j] >= n) return DINOV2_HIP_ERR_INVALID;
    const KmeansPlan plan = kmeans_plan(n, K, H, 0);
    OpBuf dX, dI;
    KmeansOpBufs w;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(w.alloc(K, H, plan));
    OP_TRY(launch_match_normalise(dX.as<float>(), (size_t)H, w.b.x16, n, plan.npad, H, plan.hpad, nullptr));
    if (init_centers) {
        OP_TRY(hipMemcpy(w.b.cvec, init_centers, (size_t)K * H * 4, hipMemcpyHostToDevice));
    } else {
        OP_TRY(dI.upload(init_rows, (size_t)K * 4));
        OP_TRY(launch_kmeans_gather(dX.as<float>(), n, 0, (size_t)H, dI.as<int>(), K, H, w.b.cvec, nullptr));
    }
    int it = 0, conv = 0;
    OP_TRY(kmeans_run(w.b, n, K, H, max_iter, plan, nullptr, &it, &conv));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(KmeansOpBufs::head(w.labels, labels, (size_t)n));
    OP_FETCH(KmeansOpBufs::head(w.sim, sim, (size_t)n));
    if (centers) OP_FETCH(w.cvec.fetch(centers));
    OP_FETCH(KmeansOpBufs::head(w.counts, counts, (size_t)K));
    if (iterations) *iterations = it;
    if (converged) *converged = conv;
    return 0;
}

extern "C" int dinov2_hip_op_kmeans_bench(const float* rows_dev, int32_t n, int32_t K, int32_t H, int32_t nsplit, int32_t max_iter, int32_t warmup,
                                          int32_t iters, float* ms) {
    if (!rows_dev || !ms || !kmeans_shape_ok(n, K, H) || K > n || nsplit < 0 || max_iter < 0 || max_iter > KMEANS_ITER_MAX || warmup < 0 || iters < 1)
        return DINOV2_HIP_ERR_INVALID;
    const KmeansPlan plan = kmeans_plan(n, K, H, nsplit);
    OpBuf dW;
    EventPair ev;
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::none()));
    OP_TRY(ev.create());
    const KmeansBufs b = kmeans_bufs(dW.as<char>(), plan);
    auto seed = [&] { return hipMemcpyAsync(b.cvec, rows_dev, (size_t)K * H * 4, hipMemcpyDeviceToDevice, nullptr); };
    auto whole = [&] {
        hipError_t e = launch_match_normalise(rows_dev, (size_t)H, b.x16, n, plan.npad, H, plan.hpad, nullptr);
        if (e == hipSuccess) e = seed();
        int it, conv;
        return e != hipSuccess ? e : kmeans_run(b, n, K, H, max_iter, plan, nullptr, &it, &conv);
    };
    OP_TRY(whole());  // leaves every buffer of the single steps in a real state
    OP_TRY(launch_kmeans_transpose(b, plan, nullptr));
    auto timed = [&](auto step, float* out) {
        int rc = 0;
        for (int i = 0; i < warmup + iters && rc == 0; ++i) {
            if (i == warmup && hipEventRecord(ev.e0, nullptr) != hipSuccess) rc = -1;
            if (step() != hipSuccess) rc = -1;
        }
        float t = 0.0f;
        if (rc == 0 && (hipEventRecord(ev.e1, nullptr) != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess ||
                        hipEventElapsedTime(&t, ev.e0, ev.e1) != hipSuccess))
            rc = -1;
        *out = t / (float)iters;
        return rc;
    };
    int rc = timed([&] { return launch_kmeans_assign(b, n, K, plan, true, nullptr); }, ms + 0);
    if (rc == 0) rc = timed([&] { return launch_kmeans_update(b, K, H, plan, nullptr); }, ms + 1);
    if (rc == 0) rc = timed(whole, ms + 2);
    (void)hipDeviceSynchronize();
    return rc;
}

// ---- dinov2_hip_coreset_tokens' kernels (csrc/coreset.hip) on host data ----
namespace {
bool coreset_args_ok(int n, int H, int m, int first, float stop_sim, int rows_per_wg) {
    return n >= 1 && n <= CORESET_N_MAX && H >= 8 && H <= 4096 && m >= 1 && m <= n && first >= 0 && first < n && stop_sim == stop_sim &&
           rows_per_wg >= 0;
}
}  // namespace

extern "C" int dinov2_hip_op_coreset_plan(int32_t n, int32_t H, int32_t m, int32_t rows_per_wg, int64_t* out) {
    if (!out || !coreset_args_ok(n, H, m, 0, 0.0f, rows_per_wg)) return DINOV2_HIP_ERR_INVALID;
    const CoresetPlan p = coreset_plan(n, H, m, rows_per_wg);
    const int64_t v[5] = {p.npad, p.hpad, p.rows_per_wg, p.nparts, (int64_t)p.bytes};
    std::copy(v, v + 5, out);
    return 0;
}

extern "C" int dinov2_hip_op_coreset(const float* rows, int32_t n, int32_t H, int32_t m, int32_t first, float stop_sim, int32_t rows_per_wg,
                                     int32_t* idx, float* cover, int32_t* selected, int32_t* nearest, float* near_sim) {
    if (!rows || !coreset_args_ok(n, H, m, first, stop_sim, rows_per_wg)) return DINOV2_HIP_ERR_INVALID;
    const CoresetPlan plan = coreset_plan(n, H, m, rows_per_wg);
    OpBuf dX, dW;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::nans()));
    const CoresetBufs b = coreset_bufs(dW.as<char>(), plan, nullptr);
    OP_TRY(launch_match_normalise(dX.as<float>(), (size_t)H, dW.as<_Float16>() + plan.x16 / 2, n, plan.npad, H, plan.hpad, nullptr));
    OP_TRY(coreset_run(b, n, m, first, stop_sim, plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    if (idx) OP_TRY(dW.read(idx, plan.idx, (size_t)m * 4));
    if (cover) OP_TRY(dW.read(cover, plan.cover, (size_t)m * 4));
    if (selected) OP_TRY(dW.read(selected, plan.head + 4, 4));
    if (nearest) OP_TRY(dW.read(nearest, plan.nearest, (size_t)n * 4));
    if (near_sim) OP_TRY(dW.read(near_sim, plan.sim, (size_t)n * 4));
    return 0;
}

extern "C" int dinov2_hip_op_coreset_bench(const float* rows_dev, int32_t n, int32_t H, int32_t m, int32_t rows_per_wg, int32_t warmup,
                                           int32_t iters, float* us_per_pick) {
    if (!rows_dev || !us_per_pick || !coreset_args_ok(n, H, m, 0, INFINITY, rows_per_wg) || warmup < 0 || iters < 1) return DINOV2_HIP_ERR_INVALID;
    const CoresetPlan plan = coreset_plan(n, H, m, rows_per_wg);
    OpBuf dW;
    EventPair ev;
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::none()));
    OP_TRY(ev.create());
    const CoresetBufs b = coreset_bufs(dW.as<char>(), plan, nullptr);
    OP_TRY(launch_match_normalise(rows_dev, (size_t)H, dW.as<_Float16>() + plan.x16 / 2, n, plan.npad, H, plan.hpad, nullptr));
    float total = 0.0f;
    for (int i = 0; i < warmup + iters; ++i) {
        float t = 0.0f;
        OP_TRY(hipEventRecord(ev.e0, nullptr));
        OP_TRY(coreset_run(b, n, m, 0, INFINITY, plan, nullptr));
        OP_TRY(hipEventRecord(ev.e1, nullptr));
        OP_TRY(hipEventSynchronize(ev.e1));
        OP_TRY(hipEventElapsedTime(&t, ev.e0, ev.e1));
        if (i >= warmup) total += t;
    }
    *us_per_pick = total * 1000.0f / ((float)iters * (float)m);
    return 0;
}

// ---- dinov2_hip_ncut_tokens' kernels (csrc/ncut.hip) and its loop (csrc/ncut.cpp) on host data ----
namespace {
bool ncut_shape_ok(int n, int H) { return n >= NCUT_N_MIN && n <= NCUT_N_MAX && H >= 8 && H <= 4096; }
bool ncut_affinity_ok(int n, int H, int affinity, float tau, float floor) { return ncut_args_ok(n, H, affinity, tau, floor, 1, 1, 1e-3f); }
// The buffers of one run, each an allocation of its own that starts as 0xff bytes; the partials, the blocks, the degrees and the 8 x 8
// partials between guard bands.
struct NcutOpBufs {
    OpBuf x16, y[2], gram[2], ritz, deg, cs, part;
    NcutBufs b{};
    hipError_t alloc(const NcutPlan& p) {
        const struct { OpBuf* buf; size_t n, esz, guard; } all[] = {
            {&x16, (size_t)p.npad * p.hpad, 2, 0}, {&y[0], (size_t)p.npad * NCUT_NB, 8, NCUT_NB}, {&y[1], (size_t)p.npad * NCUT_NB, 8, NCUT_NB},
            {&gram[0], (size_t)p.ntiles * 64, 8, 64}, {&gram[1], (size_t)p.ntiles * 64, 8, 64}, {&ritz, (size_t)p.ntiles * 64, 8, 64},
            {&deg, (size_t)p.npad, 8, 1}, {&cs, (size_t)p.npad, 8, 1}, {&part, p.part_bytes / 8, 8, NCUT_NB}};
        for (const auto& a : all) {
            const hipError_t e = a.buf->alloc(a.n, a.esz, OpBuf::nans(), a.guard);
            if (e != hipSuccess) return e;
        }
        b.x16 = x16.as<_Float16>(); b.ritz = ritz.as<double>(); b.deg = deg.as<double>(); b.cs = cs.as<double>(); b.part = part.as<double>();
        for (int k = 0; k < 2; ++k) { b.y[k] = y[k].as<double>(); b.gram[k] = gram[k].as<double>(); }
        return hipSuccess;
    }
    // every guarded buffer's bands
    int guards() const {
        for (const OpBuf* g : {&y[0], &y[1], &gram[0], &gram[1], &ritz, &deg, &cs, &part}) {
            std::vector<double> all(g->n);
            OP_FETCH(g->fetch(all.data()));
        }
        return 0;
    }
};
}  // namespace

extern "C" int dinov2_hip_op_ncut_plan(int32_t n, int32_t H, int32_t nchunk, int64_t* out) {
    if (!out || !ncut_shape_ok(n, H) || nchunk < 0) return DINOV2_HIP_ERR_INVALID;
    const NcutPlan p = ncut_plan(n, H, nchunk);
    const int64_t v[8] = {p.npad, p.hpad, p.ntiles, p.chunk_tiles, p.nchunks, (int64_t)p.part_bytes, (int64_t)p.bytes, 0};
    std::copy(v, v + 8, out);
    return 0;
}

extern "C" int dinov2_hip_op_ncut_apply(const float* rows, int32_t n, int32_t H, int32_t affinity, float tau, float floor, const double* scale,
                                        const double* q, int32_t nchunk, double* t_out, double* degree_out, float* xhat_f16_as_f32) {
    if (!rows || !ncut_shape_ok(n, H) || !ncut_affinity_ok(n, H, affinity, tau, floor) || nchunk < 0 || (t_out && !q) ||
        (!t_out && !degree_out && !xhat_f16_as_f32))
        return DINOV2_HIP_ERR_INVALID;
    const NcutPlan plan = ncut_plan(n, H, nchunk);
    OpBuf dX, dS, dQ;
    NcutOpBufs w;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(w.alloc(plan));
    OP_TRY(launch_match_normalise(dX.as<float>(), (size_t)H, w.b.x16, n, plan.npad, H, plan.hpad, nullptr));
    std::vector<double> part(plan.part_bytes / 8);
    auto fold = [&](int cols, double* out) {  // the chunks in ascending order, as ncut_degree_kernel and ncut_finish_kernel fold them
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < cols; ++c) {
                double s = part[(size_t)i * NCUT_NB + c];
                for (int k = 1; k < plan.nchunks; ++k) s += part[((size_t)k * plan.npad + i) * NCUT_NB + c];
                out[(size_t)i * cols + c] = s;
            }
    };
    if (degree_out) {
        OP_TRY(launch_ncut_apply(w.b.x16, n, affinity, tau, floor, nullptr, nullptr, w.b.part, plan, nullptr));
        OP_TRY(launch_ncut_degree(w.b.part, n, w.b.deg, w.b.cs, plan, nullptr));
        OP_TRY(hipDeviceSynchronize());
        std::vector<double> d((size_t)plan.npad);
        OP_FETCH(w.deg.fetch(d.data()));
        std::copy(d.begin(), d.begin() + n, degree_out);
        OP_FETCH(w.part.fetch(part.data()));  // (its guards)
    }
    if (t_out) {
        if (scale) OP_TRY(dS.upload(scale, (size_t)n * 8));
        OP_TRY(dQ.upload(q, (size_t)n * NCUT_NB * 8));
        OP_TRY(launch_ncut_apply(w.b.x16, n, affinity, tau, floor, scale ? dS.as<double>() : nullptr, dQ.as<double>(), w.b.part, plan, nullptr));
        OP_TRY(hipDeviceSynchronize());
        OP_FETCH(w.part.fetch(part.data()));
        fold(NCUT_NB, t_out);
    }
    if (xhat_f16_as_f32) {
        std::vector<uint16_t> x16((size_t)plan.npad * plan.hpad);
        OP_TRY(w.x16.read(x16.data(), 0, x16.size() * 2));
        for (int i = 0; i < n; ++i) widen_to_f32(false, (const unsigned char*)(x16.data() + (size_t)i * plan.hpad), (size_t)H, xhat_f16_as_f32 + (size_t)i * H);
    }
    return 0;
}

extern "C" int dinov2_hip_op_ncut_step(const float* rows, int32_t n, int32_t H, int32_t affinity, float tau, float floor, int32_t nchunk,
                                       const double* yprev, const double* gprev_parts, double* ynext, double* gnext_parts, double* ritz_parts) {
    if (!rows || !yprev || !gprev_parts || !ynext || !gnext_parts || !ritz_parts || !ncut_shape_ok(n, H) ||
        !ncut_affinity_ok(n, H, affinity, tau, floor) || nchunk < 0)
        return DINOV2_HIP_ERR_INVALID;
    const NcutPlan plan = ncut_plan(n, H, nchunk);
    OpBuf dX;
    NcutOpBufs w;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(w.alloc(plan));
    OP_TRY(launch_match_normalise(dX.as<float>(), (size_t)H, w.b.x16, n, plan.npad, H, plan.hpad, nullptr));
    OP_TRY(launch_ncut_apply(w.b.x16, n, affinity, tau, floor, nullptr, nullptr, w.b.part, plan, nullptr));
    OP_TRY(launch_ncut_degree(w.b.part, n, w.b.deg, w.b.cs, plan, nullptr));
    OP_TRY(hipMemcpy(w.b.y[0], yprev, (size_t)n * NCUT_NB * 8, hipMemcpyHostToDevice));  // (rows >= n stay NaN: the kernels do not read them)
    OP_TRY(hipMemcpy(w.b.gram[0], gprev_parts, (size_t)plan.ntiles * 64 * 8, hipMemcpyHostToDevice));
    OP_TRY(launch_ncut_apply(w.b.x16, n, affinity, tau, floor, w.b.cs, w.b.y[0], w.b.part, plan, nullptr));
    OP_TRY(launch_ncut_finish(w.b.part, w.b.cs, w.b.y[0], w.b.gram[0], n, w.b.y[1], w.b.gram[1], w.b.ritz, plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    std::vector<double> y((size_t)plan.npad * NCUT_NB);
    OP_FETCH(w.y[1].fetch(y.data()));
    for (size_t i = (size_t)n * NCUT_NB; i < y.size(); ++i)
        if (y[i] != 0.0) return -1;  // the rows >= n are written as zeros
    std::copy(y.begin(), y.begin() + (size_t)n * NCUT_NB, ynext);
    OP_FETCH(w.gram[1].fetch(gnext_parts));
    OP_FETCH(w.ritz.fetch(ritz_parts));
    return w.guards();
}

extern "C" int dinov2_hip_op_ncut(const float* rows, int32_t n, int32_t H, int32_t affinity, float tau, float floor, int32_t n_eig, int32_t max_iter,
                                  float tol, float* values, float* vectors, float* degree, float* residual, int32_t* iterations,
                                  int32_t* converged) {
    if (!rows || !ncut_args_ok(n, H, affinity, tau, floor, n_eig, max_iter, tol)) return DINOV2_HIP_ERR_INVALID;
    const NcutPlan plan = ncut_plan(n, H, 0);
    OpBuf dX;
    NcutOpBufs w;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(w.alloc(plan));
    OP_TRY(launch_match_normalise(dX.as<float>(), (size_t)H, w.b.x16, n, plan.npad, H, plan.hpad, nullptr));
    NcutResult res;
    OP_TRY(ncut_run(w.b, n, affinity, tau, floor, n_eig, max_iter, tol, plan, nullptr, &res));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(w.guards());
    if (!res.finite) return -1;
    if (values) std::copy(res.values.begin(), res.values.end(), values);
    if (vectors) std::copy(res.vectors.begin(), res.vectors.end(), vectors);
    if (degree) std::copy(res.degree.begin(), res.degree.end(), degree);
    if (residual) std::copy(res.residual.begin(), res.residual.end(), residual);
    if (iterations) *iterations = res.iterations;
    if (converged) *converged = res.converged;
    return 0;
}

extern "C" int dinov2_hip_op_ncut_bench(const float* rows_dev, int32_t n, int32_t H, int32_t affinity, float tau, float floor, int32_t nchunk,
                                        int32_t n_eig, int32_t max_iter, float tol, int32_t warmup, int32_t iters, float* ms, int32_t* steps) {
    if (!rows_dev || !ms || !steps || !ncut_args_ok(n, H, affinity, tau, floor, n_eig, max_iter, tol) || nchunk < 0 || warmup < 0 || iters < 1)
        return DINOV2_HIP_ERR_INVALID;
    const NcutPlan plan = ncut_plan(n, H, nchunk);
    OpBuf dW;
    EventPair ev;
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::none()));
    OP_TRY(ev.create());
    const NcutBufs b = ncut_bufs(dW.as<char>(), plan);
    NcutResult res;
    auto whole = [&] {
        const hipError_t e = launch_match_normalise(rows_dev, (size_t)H, b.x16, n, plan.npad, H, plan.hpad, nullptr);
        return e != hipSuccess ? e : ncut_run(b, n, affinity, tau, floor, n_eig, max_iter, tol, plan, nullptr, &res);
    };
    OP_TRY(whole());  // leaves every buffer of the single steps in a real state
    *steps = res.iterations;
    auto timed = [&](auto step, float* out) {
        int rc = 0;
        for (int i = 0; i < warmup + iters && rc == 0; ++i) {
            if (i == warmup && hipEventRecord(ev.e0, nullptr) != hipSuccess) rc = -1;
            if (step() != hipSuccess) rc = -1;
        }
        float t = 0.0f;
        if (rc == 0 && (hipEventRecord(ev.e1, nullptr) != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess ||
                        hipEventElapsedTime(&t, ev.e0, ev.e1) != hipSuccess))
            rc = -1;
        *out = t / (float)iters;
        return rc;
    };
    int rc = timed([&] { return launch_ncut_apply(b.x16, n, affinity, tau, floor, b.cs, b.y[0], b.part, plan, nullptr); }, ms + 0);
    if (rc == 0) rc = timed([&] { return launch_ncut_finish(b.part, b.cs, b.y[0], b.gram[0], n, b.y[1], b.gram[1], b.ritz, plan, nullptr); }, ms + 1);
    if (rc == 0) rc = timed(whole, ms + 2);
    (void)hipDeviceSynchronize();
    return rc;
}

// ---- dinov2_hip_vlad_tokens' kernels (csrc/vlad.hip) on host data ----
namespace {
bool vlad_shape_ok(const int32_t* offsets, int n_seg, int K, int H) {
    if (!offsets || n_seg < 1 || n_seg > VLAD_SEG_MAX || K < 1 || K > KMEANS_K_MAX || H < 8 || H > 4096 || offsets[0] != 0) return false;
    for (int i = 1; i <= n_seg; ++i)
        if (offsets[i] <= offsets[i - 1] || offsets[i] > VLAD_N_MAX) return false;
    return (uint64_t)n_seg * (uint64_t)K * (uint64_t)H <= VLAD_OUT_MAX;
}
// The buffers of one run, each an allocation of its own that starts as 0xff bytes; the four results between guard bands.
struct VladOpBufs {
    OpBuf x16, xt, c16, cvec, labels, labels_out, sim_out, part, cpart, vlad, counts, rowss, segs, chunks, tiles;
    VladBufs b{};
    hipError_t alloc(int n, int n_seg, int K, int H, const VladPlan& p) {
        const size_t held = (size_t)(p.nchunks < p.cap ? p.nchunks : p.cap);
        const struct { OpBuf* buf; size_t n, esz, guard; } all[] = {
            {&x16, (size_t)p.npad * p.hpad, 2, 0}, {&xt, (size_t)p.hpad128 * p.npad, 2, 0}, {&c16, (size_t)p.kpad * p.hpad, 2, 0},
            {&cvec, (size_t)K * H, 4, 0}, {&labels, (size_t)p.npad, 4, 1}, {&labels_out, (size_t)n, 4, 1}, {&sim_out, (size_t)n, 4, 1},
            {&part, p.part_bytes / 4, 4, 0}, {&cpart, held * p.kpad, 4, 0}, {&vlad, (size_t)n_seg * K * H, 4, (size_t)H},
            {&counts, (size_t)n_seg * K, 4, 1}, {&rowss, (size_t)n_seg * K, 4, 1}, {&segs, (size_t)n_seg * sizeof(VladSeg), 1, 0},
            {&chunks, (size_t)p.nchunks * sizeof(VladChunk), 1, 0}, {&tiles, (size_t)p.ntiles * sizeof(VladTile), 1, 0}};
        for (const auto& a : all) {
            const hipError_t e = a.buf->alloc(a.n, a.esz, OpBuf::nans(), a.guard);
            if (e != hipSuccess) return e;
        }
        b.x16 = x16.as<_Float16>(); b.xt = xt.as<_Float16>(); b.c16 = c16.as<_Float16>(); b.cvec = cvec.as<float>();
        b.labels = labels.as<int>(); b.labels_out = labels_out.as<int>(); b.sim_out = sim_out.as<float>(); b.part = part.as<float>();
        b.cpart = cpart.as<int>(); b.vlad = vlad.as<float>(); b.counts = counts.as<int>(); b.rowss = rowss.as<float>();
        b.segs = segs.as<VladSeg>(); b.chunks = chunks.as<VladChunk>(); b.tiles = tiles.as<VladTile>();
        return hipSuccess;
    }
};
struct VladTables {
    std::vector<VladSeg> segs;
    std::vector<VladChunk> chunks;
    std::vector<VladTile> tiles;
    hipError_t upload(const VladBufs& b) const {
        hipError_t e = hipMemcpy(b.segs, segs.data(), segs.size() * sizeof(VladSeg), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(b.chunks, chunks.data(), chunks.size() * sizeof(VladChunk), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(b.tiles, tiles.data(), tiles.size() * sizeof(VladTile), hipMemcpyHostToDevice);
        return e;
    }
};
// every segment of the device rows x [n, H] into its block of the padded layout (b.tiles uploaded)
hipError_t vlad_normalise_segments(const float* x, int n, int H, const VladBufs& b, const VladPlan& p) {
    return launch_vlad_normalise(x, n, 0, (size_t)H, b.tiles, p.ntiles, b.x16, H, p.hpad, nullptr);
}
}  // namespace

extern "C" int dinov2_hip_op_vlad_plan(const int32_t* offsets, int32_t n_seg, int32_t K, int32_t H, int64_t* out, int32_t* segs, int32_t* chunks,
                                       int32_t max_chunks) {
    if (!out || !vlad_shape_ok(offsets, n_seg, K, H)) return DINOV2_HIP_ERR_INVALID;
    VladTables t;
    const VladPlan p = vlad_plan(offsets, n_seg, K, H, &t.segs, &t.chunks, nullptr);
    if (chunks && max_chunks < p.nchunks) return DINOV2_HIP_ERR_INVALID;
    const int64_t v[12] = {p.kpad, p.hpad, p.hpad128, p.chunk, p.cap, p.npad, p.ntiles, p.nchunks, p.npass, (int64_t)p.part_bytes, (int64_t)p.bytes, 0};
    std::copy(v, v + 12, out);
    for (int i = 0; segs && i < n_seg; ++i) {
        const int32_t r[4] = {t.segs[i].row0, t.segs[i].len, t.segs[i].chunk0, t.segs[i].nchunks};
        std::copy(r, r + 4, segs + 4 * i);
    }
    for (int i = 0; chunks && i < p.nchunks; ++i) {
        const int32_t r[3] = {t.chunks[i].seg, t.chunks[i].row0, t.chunks[i].ktiles};
        std::copy(r, r + 3, chunks + 3 * i);
    }
    return 0;
}

extern "C" int dinov2_hip_op_vlad(const float* rows, const int32_t* offsets, int32_t n_seg, const float* centers, int32_t K, int32_t H, uint32_t flags,
                                  int32_t* labels, float* sim, int32_t* counts, float* vlad, float* xhat_f16_as_f32, float* chat_f16_as_f32) {
    if (!rows || !centers || !vlad_shape_ok(offsets, n_seg, K, H) || (flags & ~3u)) return DINOV2_HIP_ERR_INVALID;
    const int n = offsets[n_seg];
    VladTables t;
    const VladPlan plan = vlad_plan(offsets, n_seg, K, H, &t.segs, &t.chunks, &t.tiles);
    OpBuf dX;
    VladOpBufs w;
    OP_TRY(dX.upload(rows, (size_t)n * H * 4));
    OP_TRY(w.alloc(n, n_seg, K, H, plan));
    OP_TRY(t.upload(w.b));
    OP_TRY(hipMemcpy(w.b.cvec, centers, (size_t)K * H * 4, hipMemcpyHostToDevice));
    OP_TRY(vlad_normalise_segments(dX.as<float>(), n, H, w.b, plan));
    OP_TRY(vlad_run(w.b, n_seg, K, H, flags, plan, t.chunks.data(), nullptr));
    OP_TRY(hipDeviceSynchronize());
    std::vector<int32_t> li((size_t)n), ci((size_t)n_seg * K), lp((size_t)plan.npad);
    std::vector<float> sf((size_t)n), rs((size_t)n_seg * K), vf((size_t)n_seg * K * H);
    OP_FETCH(w.labels_out.fetch(li.data()));
    OP_FETCH(w.sim_out.fetch(sf.data()));
    OP_FETCH(w.counts.fetch(ci.data()));
    OP_FETCH(w.vlad.fetch(vf.data()));
    OP_FETCH(w.labels.fetch(lp.data()));  // (their guards)
    OP_FETCH(w.rowss.fetch(rs.data()));
    if (labels) std::copy(li.begin(), li.end(), labels);
    if (sim) std::copy(sf.begin(), sf.end(), sim);
    if (counts) std::copy(ci.begin(), ci.end(), counts);
    if (vlad) std::copy(vf.begin(), vf.end(), vlad);
    if (xhat_f16_as_f32) {
        std::vector<uint16_t> x16((size_t)plan.npad * plan.hpad);
        OP_TRY(w.x16.read(x16.data(), 0, x16.size() * 2));
        for (int s = 0; s < n_seg; ++s)
            for (int i = 0; i < t.segs[s].len; ++i)
                widen_to_f32(false, (const unsigned char*)(x16.data() + (size_t)(t.segs[s].row0 + i) * plan.hpad), (size_t)H,
                             xhat_f16_as_f32 + (size_t)(offsets[s] + i) * H);
    }
    if (chat_f16_as_f32) {
        std::vector<uint16_t> c16((size_t)plan.kpad * plan.hpad);
        OP_TRY(w.c16.read(c16.data(), 0, c16.size() * 2));
        for (int c = 0; c < K; ++c)
            widen_to_f32(false, (const unsigned char*)(c16.data() + (size_t)c * plan.hpad), (size_t)H, chat_f16_as_f32 + (size_t)c * H);
    }
    return 0;
}

extern "C" int dinov2_hip_op_vlad_bench(const float* rows_dev, const int32_t* offsets, int32_t n_seg, const float* centers_dev, int32_t K, int32_t H,
                                        uint32_t flags, int32_t warmup, int32_t iters, float* ms) {
    if (!rows_dev || !centers_dev || !ms || !vlad_shape_ok(offsets, n_seg, K, H) || (flags & ~3u) || warmup < 0 || iters < 1)
        return DINOV2_HIP_ERR_INVALID;
    VladTables t;
    const VladPlan plan = vlad_plan(offsets, n_seg, K, H, &t.segs, &t.chunks, &t.tiles);
    OpBuf dW;
    EventPair ev;
    OP_TRY(dW.alloc(plan.bytes, 1, OpBuf::none()));
    OP_TRY(ev.create());
    const VladBufs b = vlad_bufs(dW.as<char>(), plan);
    OP_TRY(t.upload(b));
    auto whole = [&] {
        hipError_t e = hipMemcpyAsync(b.cvec, centers_dev, (size_t)K * H * 4, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = vlad_normalise_segments(rows_dev, offsets[n_seg], H, b, plan);
        return e != hipSuccess ? e : vlad_run(b, n_seg, K, H, flags, plan, t.chunks.data(), nullptr);
    };
    OP_TRY(whole());  // leaves every buffer of the single steps in a real state
    auto timed = [&](auto step, float* out) {
        int rc = 0;
        for (int i = 0; i < warmup + iters && rc == 0; ++i) {
            if (i == warmup && hipEventRecord(ev.e0, nullptr) != hipSuccess) rc = -1;
            if (step() != hipSuccess) rc = -1;
        }
        float tm = 0.0f;
        if (rc == 0 && (hipEventRecord(ev.e1, nullptr) != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess ||
                        hipEventElapsedTime(&tm, ev.e0, ev.e1) != hipSuccess))
            rc = -1;
        *out = tm / (float)iters;
        return rc;
    };
    int rc = timed([&] { return launch_vlad_assign(b, K, plan, nullptr); }, ms + 0);
    if (rc == 0) rc = timed([&] { return launch_vlad_sums(b, n_seg, K, H, flags, plan, t.chunks.data(), nullptr); }, ms + 1);
    if (rc == 0) rc = timed(whole, ms + 2);
    (void)hipDeviceSynchronize();
    return rc;
}

// ---- the device stages of dinov2_hip_pca3 (csrc/pca.cpp), each through the launch function the driver calls, on host data ----
namespace {
bool pca_shape_ok(int P, int H) { return P >= 4 && H >= 8 && H <= 4096; }  // the range dinov2_hip_pca3 accepts
}  // namespace

extern "C" int dinov2_hip_op_pca_ppad(int32_t P) { return pca_ppad(P); }
extern "C" int dinov2_hip_op_pca_blocks(int32_t H) { return pca_blocks(H); }

extern "C" int dinov2_hip_op_pca_prepare(const float* tok, int32_t P, int32_t H, float* mean_out, float* xt_out) {
    if (!tok || !mean_out || !xt_out || !pca_shape_ok(P, H)) return DINOV2_HIP_ERR_INVALID;
    const int Ppad = pca_ppad(P);
    OpBuf dT, dM, dX;
    OP_TRY(dT.upload(tok, (size_t)P * H * 4));
    OP_TRY(dM.alloc((size_t)H, 4, OpBuf::nans(), (size_t)H));
    OP_TRY(dX.alloc((size_t)H * Ppad, 2, OpBuf::nans(), (size_t)Ppad));
    OP_TRY(launch_pca_prepare(dT.as<float>(), dM.as<float>(), dX.as<void>(), P, H, Ppad, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(dM.fetch(mean_out));
    return dX.fetch_as(DT_F16, xt_out);
}

extern "C" int dinov2_hip_op_pca_cov(const float* tok, int32_t P, int32_t H, float* cov_out) {
    if (!tok || !cov_out || !pca_shape_ok(P, H)) return DINOV2_HIP_ERR_INVALID;
    if (gemm_init() != hipSuccess) return -1;
    const int Ppad = pca_ppad(P);
    OpBuf dT, dM, dX, dC;
    OP_TRY(dT.upload(tok, (size_t)P * H * 4));
    OP_TRY(dM.alloc((size_t)H, 4, OpBuf::none()));
    OP_TRY(dX.alloc((size_t)H * Ppad, 2, OpBuf::nans()));  // (the driver's xt is reused scratch: whatever prepare leaves unwritten is read as it is)
    OP_TRY(dC.alloc((size_t)H * H, 4, OpBuf::nans(), (size_t)H));
    OP_TRY(launch_pca_prepare(dT.as<float>(), dM.as<float>(), dX.p, P, H, Ppad, nullptr));
    OP_TRY(launch_pca_cov(dX.p, dC.as<float>(), H, Ppad, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dC.fetch(cov_out);
}

extern "C" int dinov2_hip_op_pca_power(const float* cov, const double* yprev, const double* gprev_parts, int32_t H, double* ynext,
                                       double* gnext_parts) {
    if (!cov || !yprev || !gprev_parts || !ynext || !gnext_parts || H < 8 || H > 4096) return DINOV2_HIP_ERR_INVALID;
    const size_t ny = (size_t)H * PCA_NB, ngram = (size_t)pca_blocks(H) * 64;
    OpBuf dC, dY, dG, dYn, dGn;
    OP_TRY(dC.upload(cov, (size_t)H * H * 4));
    OP_TRY(dY.upload(yprev, ny * 8));
    OP_TRY(dG.upload(gprev_parts, ngram * 8));
    OP_TRY(dYn.alloc(ny, 8, OpBuf::nans(), PCA_NB));
    OP_TRY(dGn.alloc(ngram, 8, OpBuf::nans(), 64));
    OP_TRY(launch_pca_power(dC.as<float>(), dY.as<double>(), dG.as<double>(), dYn.as<double>(), dGn.as<double>(), H, nullptr));
    OP_TRY(hipDeviceSynchronize());
    OP_FETCH(dYn.fetch(ynext));
    return dGn.fetch(gnext_parts);
}

extern "C" int dinov2_hip_op_pca_project(const float* tok, const float* mean, const float* comp, int32_t P, int32_t H, float* proj) {
    if (!tok || !mean || !comp || !proj || !pca_shape_ok(P, H)) return DINOV2_HIP_ERR_INVALID;
    OpBuf dT, dM, dC, dP;
    OP_TRY(dT.upload(tok, (size_t)P * H * 4));
    OP_TRY(dM.upload(mean, (size_t)H * 4));
    OP_TRY(dC.upload(comp, (size_t)3 * H * 4));
    OP_TRY(dP.alloc((size_t)P * 3, 4, OpBuf::nans(), 3));
    OP_TRY(launch_pca_project(dT.as<float>(), dM.as<float>(), dC.as<float>(), dP.as<float>(), P, H, nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dP.fetch(proj);
}

// host-only: pca_chol_rinv (csrc/kernels.h), the factorisation the power kernel and pca_ritz share
extern "C" int dinov2_hip_op_pca_chol_rinv(const double* gram, double* rinv) {
    if (!gram || !rinv) return DINOV2_HIP_ERR_INVALID;
    pca_chol_rinv(gram, rinv);
    return DINOV2_HIP_OK;
}

// ---- a bounded stall of a caller's stream (tests/stream_cases.py): refusals first, before any HIP call ----
extern "C" int dinov2_hip_op_stream_delay(void* stream, int32_t milliseconds) {
    if (!stream || milliseconds < 1 || milliseconds > 100) return DINOV2_HIP_ERR_INVALID;
    return launch_stream_delay(milliseconds, (hipStream_t)stream) == hipSuccess ? DINOV2_HIP_OK : DINOV2_HIP_ERR_HIP;
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
    const size_t P = (size_t)h0 * w0, ldl = (size_t)dense_cpad(C), npx = (size_t)out_h * out_w;
    OpBuf dL, dC, dLab, dVal;
    OP_TRY(dL.alloc(P * ldl, 4, OpBuf::nans()));  // the columns past C stay NaN: the kernel must not let them into a result
    OP_TRY(hipMemcpy2D(dL.p, ldl * 4, logits, (size_t)C * 4, (size_t)C * 4, P, hipMemcpyHostToDevice));
    if (reduce == DENSE_BINS) OP_TRY(dC.upload(centers, (size_t)C * 4));
    if (labels) OP_TRY(dLab.alloc(npx, 1, OpBuf::nans(), (size_t)out_w));
    if (value) OP_TRY(dVal.alloc(npx, 4, OpBuf::nans(), (size_t)out_w));
    OP_TRY(launch_dense_reduce(dL.as<float>(), (int)ldl, 1, h0, w0, C, out_h, out_w, reduce, dC.as<float>(), eps, dLab.as<uint8_t>(),
                               dVal.as<float>(), plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    if (labels) OP_FETCH(dLab.fetch(labels));
    if (value) OP_FETCH(dVal.fetch(value));
    return 0;
}
extern "C" int dinov2_hip_op_dense_pack(const float* x, const float* ln_w, const float* ln_b, float eps, int32_t B, int32_t T, int32_t R, int32_t H,
                                        int32_t norm, int32_t concat_cls, int32_t slot, int32_t nslots, float* out) {
    if (!x || !out || B <= 0 || H <= 0 || H % 8 != 0 || R < 0 || T < 2 + R || nslots < 1 || nslots > DENSE_LAYERS_MAX || slot < 0 || slot >= nslots)
        return DINOV2_HIP_ERR_INVALID;
    if (norm && (!ln_w || !ln_b)) return DINOV2_HIP_ERR_INVALID;
    const size_t P = (size_t)(T - 1 - R), hblk = (size_t)H * (concat_cls ? 2 : 1), K = hblk * nslots;
    OpBuf dX, dW, dB, dA;
    OP_TRY(dX.upload(x, (size_t)B * T * H * 4));
    if (norm) {
        OP_TRY(dW.upload(ln_w, (size_t)H * 4));
        OP_TRY(dB.upload(ln_b, (size_t)H * 4));
    }
    OP_TRY(dA.alloc((size_t)B * P * K, 2, OpBuf::nans(), K));  // the column blocks of the other slots stay NaN
    OP_TRY(launch_dense_pack(dX.as<float>(), dW.as<float>(), dB.as<float>(), eps, B, T, R, H, norm != 0, concat_cls != 0, dA.as<_Float16>(), K,
                             (int)(slot * hblk), nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dA.fetch_as(DT_F16, out);
}

// ---- the kernels of csrc/slide.hip (dinov2_hip_predict_dense_slide) on host data ----
extern "C" int dinov2_hip_op_slide_reduce_plan(int32_t h0, int32_t w0, int32_t C, int32_t crop_h, int32_t crop_w, int32_t h, int32_t w,
                                               const int32_t* y1, int32_t ny, const int32_t* x1, int32_t nx, int64_t* out) {
    const SlideReducePlan p = slide_reduce_plan(h0, w0, C, crop_h, crop_w, h, w, y1, ny, x1, nx);
    if (!out || p.tile_y == 0) return DINOV2_HIP_ERR_INVALID;
    const int64_t v[10] = {p.tile_y, p.tile_x, p.slots_y, p.slots_x, p.span_y, p.span_x, p.chunk, p.pitch, (int64_t)p.lds_bytes, p.cover};
    std::copy(v, v + 10, out);
    return 0;
}
extern "C" int dinov2_hip_op_slide_reduce(const float* logits, int32_t h0, int32_t w0, int32_t C, int32_t crop_h, int32_t crop_w, int32_t h, int32_t w,
                                          const int32_t* y1, int32_t ny, const int32_t* x1, int32_t nx, int32_t reduce, const float* centers,
                                          float eps, uint8_t* labels, float* value) {
    const SlideReducePlan plan = slide_reduce_plan(h0, w0, C, crop_h, crop_w, h, w, y1, ny, x1, nx);
    if (!logits || plan.tile_y == 0 || (int64_t)ny * nx > SLIDE_WINDOWS_MAX || (reduce != DENSE_ARGMAX && reduce != DENSE_BINS))
        return DINOV2_HIP_ERR_INVALID;
    if (reduce == DENSE_BINS ? (!centers || !(eps > 0.0f) || labels || !value) : (!labels && !value)) return DINOV2_HIP_ERR_INVALID;
    const size_t rows = (size_t)ny * nx * h0 * w0, npx = (size_t)h * w;
    std::vector<int> tab(slide_table_ints(plan, ny, nx));
    slide_table_fill(plan, h0, w0, crop_h, crop_w, h, w, y1, ny, x1, nx, tab.data());
    OpBuf dL, dT, dC, dLab, dVal;
    OP_TRY(dL.upload(logits, rows * (size_t)C * 4));  // (rows of C floats back to back: no more than a float's alignment, as in the session)
    OP_TRY(dT.upload(tab.data(), tab.size() * sizeof(int)));
    if (reduce == DENSE_BINS) OP_TRY(dC.upload(centers, (size_t)C * 4));
    if (labels) OP_TRY(dLab.alloc(npx, 1, OpBuf::nans(), (size_t)w));
    if (value) OP_TRY(dVal.alloc(npx, 4, OpBuf::nans(), (size_t)w));
    OP_TRY(launch_slide_reduce(dL.as<float>(), C, 1, h0, w0, C, crop_h, crop_w, h, w, ny, nx, dT.as<int>(), reduce, dC.as<float>(), eps,
                               dLab.as<uint8_t>(), dVal.as<float>(), plan, nullptr));
    OP_TRY(hipDeviceSynchronize());
    if (labels) OP_FETCH(dLab.fetch(labels));
    if (value) OP_FETCH(dVal.fetch(value));
    return 0;
}
extern "C" int dinov2_hip_op_slide_gather(const float* image, int32_t layout, int32_t h, int32_t w, int32_t crop_h, int32_t crop_w, const int32_t* y1,
                                          int32_t ny, const int32_t* x1, int32_t nx, float* windows) {
    if (!image || !windows || (layout != DINOV2_HIP_BGR_HWC && layout != DINOV2_HIP_RGB_CHW) || h > DENSE_OUT_MAX || w > DENSE_OUT_MAX)
        return DINOV2_HIP_ERR_INVALID;
    if (!slide_axis_valid(y1, ny, crop_h, h) || !slide_axis_valid(x1, nx, crop_w, w) || (int64_t)ny * nx > SLIDE_WINDOWS_MAX)
        return DINOV2_HIP_ERR_INVALID;
    std::vector<int> tab(y1, y1 + ny);
    tab.insert(tab.end(), x1, x1 + nx);
    OpBuf dI, dT, dW;
    OP_TRY(dI.upload(image, (size_t)3 * h * w * 4));
    OP_TRY(dT.upload(tab.data(), tab.size() * sizeof(int)));
    OP_TRY(dW.alloc((size_t)ny * nx * 3 * crop_h * crop_w, 4, OpBuf::nans(), (size_t)crop_w * 3));
    OP_TRY(launch_slide_gather(dI.as<float>(), dW.as<float>(), dT.as<int>(), 1, h, w, ny, nx, crop_h, crop_w, layout == DINOV2_HIP_RGB_CHW ? 1 : 0,
                               nullptr));
    OP_TRY(hipDeviceSynchronize());
    return dW.fetch(windows);
}
