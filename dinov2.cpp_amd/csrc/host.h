// Internal helpers of the host files behind the C-ABI (load.cpp, model.cpp, extras.cpp, pca.cpp, resident.cpp, vlad.cpp, propagate.cpp, ncut.cpp, coreset.cpp): error text, HIP_TRY, sizes, the session's
// scratch buffers.  Not for group.cpp, which talks to the sessions through the C-ABI and has an error macro of its own.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "model.h"

namespace dinov2 {

inline void set_err(char* err, size_t n, const char* fmt, ...) {
    if (!err || n == 0) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, n, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            dinov2::set_err(err, errlen, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return DINOV2_HIP_ERR_HIP;                                                             \
        }                                                                                          \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Dims {
    int P, T, M;
};

// The patch grid of an image of network size h x w: THE definition on the host (kernels.h grid_dim: patches of patch_size pixels every
// patch_stride pixels).  Nothing outside the kernels divides by the patch size for a grid or a row count.
struct Grid {
    int h0, w0;
};
inline Grid grid_of(const dinov2_hip_model* m, int h, int w) {
    return Grid{grid_dim(h, (int)m->hp.patch_size, m->patch_stride), grid_dim(w, (int)m->hp.patch_size, m->patch_stride)};
}

inline Dims dims_of(const dinov2_hip_model* m, int B, int h, int w) {
    Dims d;
    const Grid g = grid_of(m, h, w);
    d.P = g.h0 * g.w0;
    d.T = 1 + (int)m->hp.num_register_tokens + d.P;
    d.M = B * d.T;
    return d;
}

// The runs of a pass (model.h), no device needed.  A uniform batch is one run that starts at row, patch and image 0 ...
inline PassRun uniform_run(const dinov2_hip_model* m, const float* img, int B, int h, int w, const float* pos) {
    const Dims d = dims_of(m, B, h, w);
    return PassRun{img, B, h, w, pos, 0, 0, 0, d.P, d.T};
}
// ... and a list has list_plan's runs, each behind the rows and patches of the runs before it (hs / ws: network sizes per image; the caller
// fills in img and pos)
inline void list_runs(const ListImage* im, const ListRun* lr, int nruns, const int32_t* hs, const int32_t* ws, PassRun* out) {
    int64_t patch0 = 0;
    for (int r = 0; r < nruns; ++r) {
        const int i0 = lr[r].first;
        out[r] = PassRun{nullptr, lr[r].count, hs[i0], ws[i0], nullptr, im[i0].row0, patch0, i0, im[i0].P, im[i0].T};
        patch0 += (int64_t)lr[r].count * im[i0].P;
    }
}

// load.cpp: the widest activation row of a forward in elements (qkv, the FFN hidden layer or the im2col matrix), and one image of network
// size h x w against the limit of a pass: token rows * widest_row * 2 bytes below 2^31 (model.h: dinov2_check_pass_rows words the refusal)
size_t widest_row(const dinov2_hip_model* m);
int check_rows_at(const dinov2_hip_model* m, int h, int w, char* err, size_t errlen);

// The im2col of the patch embedding: the default stride keeps the launch it always had, a smaller one goes to the strided kernel
inline hipError_t launch_patch_im2col(DType dt, const float* img, void* col, int B, int h, int w, int ps, int stride, int Kpad, int layout,
                                      hipStream_t st) {
    return stride == ps ? launch_im2col(dt, img, col, B, h, w, ps, Kpad, layout, st)
                        : launch_im2col_stride(dt, img, col, B, h, w, ps, stride, Kpad, layout, st);
}

// Session scratch `buf`, at least `need` bytes: the one place that allocates it (model.cpp).  Returns at once when it is large enough; otherwise
// waits for the session's stream (which may still be using the old allocation), frees it and allocates anew -- the contents are not kept.  A
// refused allocation leaves `buf` empty and HIP's last error cleared (not left behind for the next launch to report), and reports
// "<who>: <n> bytes of scratch refused: <hip error string>".
int reserve(dinov2_hip_session* s, DevBuf& buf, size_t need, const char* who, char* err, size_t errlen);

// A layer list has to be strictly ascending with every entry in [lo, hi].  0 when it is; otherwise *bad is the first offending entry and the
// return value says what is wrong with it -- entry by entry, the range before the order.  The callers word the refusal.
enum LayerListFault : int { LAYER_LIST_OK = 0, LAYER_OUT_OF_RANGE, LAYER_NOT_ASCENDING };
inline LayerListFault check_layer_list(const int32_t* layers, int n, int lo, int hi, int* bad) {
    for (int i = 0; i < n; ++i) {
        *bad = (int)layers[i];
        if (layers[i] < lo || layers[i] > hi) return LAYER_OUT_OF_RANGE;
        if (i > 0 && layers[i] <= layers[i - 1]) return LAYER_NOT_ASCENDING;
    }
    return LAYER_LIST_OK;
}

// resident.cpp, for vlad.cpp, propagate.cpp, ncut.cpp and coreset.cpp: its check of a dinov2_hip_rows of row width H against the session.  On success *src / *ld are the device view
// of a resident source (nullptr for DINOV2_HIP_ROWS_GIVEN).  Touches nothing.
int check_session_rows(const char* who, const dinov2_hip_session* s, int H, const dinov2_hip_rows* r, const float** src, size_t* ld, char* err,
                       size_t errlen);

// pca.cpp, for ops_testing.cpp: the Rayleigh-Ritz step of dinov2_hip_pca3 on the host
void pca_ritz(const double* yprev, const double* ynext, const double* g_parts, int nparts, int H, double* evals, double* comp);

// ncut.cpp, for ops_testing.cpp: the ranges of dinov2_hip_ncut, the start block, the host's Rayleigh-Ritz step and the loop of
// dinov2_hip_ncut_tokens from the normalised rows on (it waits for the stream; the results stay f64 until the caller narrows them)
struct NcutResult {
    std::vector<double> values, vectors, degree, residual;  // [n_eig], [n_eig][n], [n], [n_eig]; values and vectors empty unless finite
    int iterations = 0, converged = 0;
    bool finite = true;
};
bool ncut_args_ok(int n, int H, int affinity, float tau, float floor, int n_eig, int max_iter, float tol);
void ncut_start_block(const double* deg, int n, int npad, int nparts, double* y0, double* g0);
void ncut_ritz(const double* b_parts, const double* g_parts, int nparts, double* theta, double* V, double* resid);
hipError_t ncut_run(const NcutBufs& b, int n, int affinity, float tau, float floor, int n_eig, int max_iter, float tol, const NcutPlan& plan,
                    hipStream_t stream, NcutResult* out);

// interpolate_pos_embed of the reference (load.cpp).  pos: [1 + M*M, H]; out: [1 + h_new*w_new, H].
void interpolate_pos_embed(const float* pos, int M, int H, int h_new, int w_new, float* out);

// model.cpp, for extras.cpp: the argument checks of every predict (null session / dinov2_check_input / dinov2_check_pass_rows; classify without
// a head, top-k on the device), the network input size of `in` (raw 8-bit input: after the preprocessing), the passes themselves, and the copy-out of the last one.
int check_input(const dinov2_hip_session* s, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen);
int check_predict_args(const dinov2_hip_model* m, const dinov2_hip_output* out, uint32_t flags, char* err, size_t errlen);
void network_size(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, int* h, int* w);
int predict_impl(dinov2_hip_session* s, const dinov2_hip_input* in, dinov2_hip_output* out, uint32_t flags, const PassExtras& ex, char* err,
                 size_t errlen);
int fetch_outputs(dinov2_hip_session* s, dinov2_hip_output* out, char* err, size_t errlen);
// model.cpp, for slide.cpp: while it lives, what the session's stream runs is booked under the kind `kind` ("im2col", "head", ...) of
// dinov2_hip_session_profile, as the forward's own launches are; nothing while the session is not profiling
struct ProfileMark {
    ProfileMark(dinov2_hip_session* s, const char* kind);
    ~ProfileMark();
    ProfileMark(const ProfileMark&) = delete;
    ProfileMark& operator=(const ProfileMark&) = delete;
    void* scope = nullptr;
};

}  // namespace dinov2
