// ncut.cpp -- dinov2_hip_ncut_tokens (include/dinov2_hip.h): the host half of the spectral embedding of token rows -- the argument checks,
// the loop of contract 5 with its Rayleigh-Ritz step from 8 x 8 matrices, and the vectors of contract 6 (csrc/ncut.hip; no reference
// counterpart).  Beside resident.cpp, whose check of a rows source it shares (host.h check_session_rows).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "host.h"

using namespace dinov2;

namespace {
// The tables of a call are locals whose copies to and from the device are queued on the session's stream: a return before the wait that
// belongs to them drains the stream first.
struct DrainOnError {
    hipStream_t st;
    bool armed = true;
    ~DrainOnError() {
        if (armed) (void)hipStreamSynchronize(st);
    }
};
}  // namespace

namespace dinov2 {

bool ncut_args_ok(int n, int H, int affinity, float tau, float floor, int n_eig, int max_iter, float tol) {
    if (n < NCUT_N_MIN || n > NCUT_N_MAX || H < 8 || H > 4096) return false;
    if (affinity != NCUT_THRESHOLD && affinity != NCUT_RELU && affinity != NCUT_EXP) return false;
    if (affinity == NCUT_THRESHOLD && !(tau >= -1.0f && tau < 1.0f && floor >= 0.0f && floor <= 1.0f)) return false;
    if (affinity == NCUT_EXP && !(tau >= 0x1p-6f && tau <= 16.0f)) return false;
    if (n_eig < 1 || n_eig > NCUT_EIG_MAX || max_iter < 1 || max_iter > NCUT_ITER_MAX) return false;
    return tol >= 1e-6f && tol <= 1e-1f;
}

// Contract 5's start block, a fixed function of (n, d): column 0 is sqrt(d_i), the top eigenvector of A; column c >= 1 is PCA's pattern
// sin(0.37 (i + 1) (c + 1)) + (c == i % 8 ? 0.5 : 0); a row of degree 0 is zero (and stays zero: its c_i is 0).  y0 [npad][8] with the rows
// >= n zero; g0 [nparts][64] = its Gram matrix in partial 0, zeros in the others.
void ncut_start_block(const double* deg, int n, int npad, int nparts, double* y0, double* g0) {
    std::fill(y0, y0 + (size_t)npad * NCUT_NB, 0.0);
    std::fill(g0, g0 + (size_t)nparts * 64, 0.0);
    for (int i = 0; i < n; ++i) {
        if (!(deg[i] > 0.0)) continue;
        double* const y = y0 + (size_t)i * NCUT_NB;
        y[0] = std::sqrt(deg[i]);
        for (int c = 1; c < NCUT_NB; ++c) y[c] = std::sin(0.37 * (i + 1) * (c + 1)) + (c == i % NCUT_NB ? 0.5 : 0.0);
        for (int r = 0; r < NCUT_NB; ++r)
            for (int c = 0; c < NCUT_NB; ++c) g0[r * NCUT_NB + c] += y[r] * y[c];
    }
}

// The Rayleigh-Ritz step from 8 x 8 matrices only: B = Q^T Y_next = Q^T A Q (symmetrised) and G = Y_next^T Y_next = Q^T A^2 Q, each the sum
// of its nparts per-workgroup partials in ascending order.  theta [8]: the eigenvalues of B, descending; V [8][8]: column k = the unit
// eigenvector v_k; resid [8]: r_k = sqrt(max(v_k^T G v_k - theta_k^2, 0)) = ||A u_k - theta_k u_k|| for u_k = Q v_k.  (pca_ritz builds its
// 8 x 8 matrix from the whole blocks and keeps three pairs; the Jacobi sweep is the same and stands here again because pca.cpp's lines
// above its waits are pinned by tests/test_stream_cases.py.)
void ncut_ritz(const double* b_parts, const double* g_parts, int nparts, double* theta, double* V, double* resid) {
    constexpr int NB = NCUT_NB;
    double Bm[NB * NB], G[NB * NB], W[NB * NB] = {0};
    for (int t = 0; t < NB * NB; ++t) {
        double sb = 0.0, sg = 0.0;
        for (int blk = 0; blk < nparts; ++blk) {
            sb += b_parts[(size_t)blk * NB * NB + t];
            sg += g_parts[(size_t)blk * NB * NB + t];
        }
        Bm[t] = sb;
        G[t] = sg;
    }
    for (int r = 0; r < NB; ++r)
        for (int c = r + 1; c < NB; ++c) Bm[r * NB + c] = Bm[c * NB + r] = 0.5 * (Bm[r * NB + c] + Bm[c * NB + r]);
    for (int k = 0; k < NB; ++k) W[k * NB + k] = 1.0;
    for (int sweep = 0; sweep < 50; ++sweep) {  // cyclic Jacobi, as pca_ritz: eigenvalues on Bm's diagonal, eigenvectors in W's columns
        double off = 0, diag = 0;
        for (int r = 0; r < NB; ++r)
            for (int c = 0; c < NB; ++c) (r == c ? diag : off) += Bm[r * NB + c] * Bm[r * NB + c];
        if (!(off > 1e-30 * diag)) break;
        for (int p = 0; p < NB - 1; ++p)
            for (int q = p + 1; q < NB; ++q) {
                const double apq = Bm[p * NB + q];
                if (apq == 0.0) continue;
                const double th = 0.5 * std::atan2(2 * apq, Bm[q * NB + q] - Bm[p * NB + p]);
                const double c = std::cos(th), sn = std::sin(th);
                for (int k = 0; k < NB; ++k) {
                    const double x = Bm[k * NB + p], y = Bm[k * NB + q];
                    Bm[k * NB + p] = c * x - sn * y; Bm[k * NB + q] = sn * x + c * y;
                }
                for (int k = 0; k < NB; ++k) {
                    const double x = Bm[p * NB + k], y = Bm[q * NB + k];
                    Bm[p * NB + k] = c * x - sn * y; Bm[q * NB + k] = sn * x + c * y;
                }
                for (int k = 0; k < NB; ++k) {
                    const double x = W[k * NB + p], y = W[k * NB + q];
                    W[k * NB + p] = c * x - sn * y; W[k * NB + q] = sn * x + c * y;
                }
            }
    }
    int order[NB];
    for (int k = 0; k < NB; ++k) order[k] = k;
    std::stable_sort(order, order + NB, [&](int x, int y) { return Bm[x * NB + x] > Bm[y * NB + y]; });
    for (int k = 0; k < NB; ++k) {
        const int o = order[k];
        theta[k] = Bm[o * NB + o];
        double vgv = 0.0;
        for (int r = 0; r < NB; ++r) {
            V[r * NB + k] = W[r * NB + o];
            for (int c = 0; c < NB; ++c) vgv += W[r * NB + o] * G[r * NB + c] * W[c * NB + o];
        }
        const double r2 = vgv - theta[k] * theta[k];
        resid[k] = r2 > 0.0 ? std::sqrt(r2) : (r2 == r2 ? 0.0 : r2);
    }
}

// Contracts 4 - 6.  b.x16 holds the normalised rows.  Waits for the stream at the degrees, at every check and at the end.
hipError_t ncut_run(const NcutBufs& b, int n, int affinity, float tau, float floor, int n_eig, int max_iter, float tol, const NcutPlan& p,
                    hipStream_t st, NcutResult* out) {
    DrainOnError drain{st};
    hipError_t e = launch_ncut_apply(b.x16, n, affinity, tau, floor, nullptr, nullptr, b.part, p, st);
    if (e == hipSuccess) e = launch_ncut_degree(b.part, n, b.deg, b.cs, p, st);
    out->degree.assign((size_t)n, 0.0);
    std::vector<double> cs((size_t)n), y0((size_t)p.npad * NCUT_NB), g0((size_t)p.ntiles * 64), bp((size_t)p.ntiles * 64), gp((size_t)p.ntiles * 64);
    if (e == hipSuccess) e = hipMemcpyAsync(out->degree.data(), b.deg, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cs.data(), b.cs, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    ncut_start_block(out->degree.data(), n, p.npad, p.ntiles, y0.data(), g0.data());
    e = hipMemcpyAsync(b.y[0], y0.data(), y0.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b.gram[0], g0.data(), g0.size() * 8, hipMemcpyHostToDevice, st);
    double theta[NCUT_NB] = {0}, V[NCUT_NB * NCUT_NB] = {0}, resid[NCUT_NB] = {0};
    int steps = 0, src = 0, conv = 0;
    bool finite = true;
    while (e == hipSuccess && steps < max_iter) {
        const int check = ncut_check_interval(steps);
        for (int it = 0; it < check && e == hipSuccess; ++it) {
            const int dst = src ^ 1;
            e = launch_ncut_apply(b.x16, n, affinity, tau, floor, b.cs, b.y[src], b.part, p, st);
            if (e == hipSuccess) e = launch_ncut_finish(b.part, b.cs, b.y[src], b.gram[src], n, b.y[dst], b.gram[dst], b.ritz, p, st);
            src = dst;
        }
        // here: src = the slot of Y_next of the last step, b.ritz = the partials of its Q^T Y_next
        if (e == hipSuccess) e = hipMemcpyAsync(bp.data(), b.ritz, bp.size() * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(gp.data(), b.gram[src], gp.size() * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        steps += check;
        ncut_ritz(bp.data(), gp.data(), p.ntiles, theta, V, resid);
        bool done = true;
        for (int k = 0; k < n_eig; ++k) {
            finite = finite && std::isfinite(theta[k]) && std::isfinite(resid[k]);
            done = done && resid[k] <= (double)tol;
        }
        if (!finite) break;
        if (done) {
            conv = 1;
            break;
        }
    }
    if (e != hipSuccess) return e;
    out->finite = finite;
    out->iterations = steps;
    out->converged = conv;
    if (!finite) {
        drain.armed = false;  // (the last check waited)
        return hipSuccess;
    }
    // contract 6: z_k = C (Y_next v_k), unit length, the entry of largest magnitude positive (the lowest index at a tie)
    std::vector<double>& y = y0;
    e = hipMemcpyAsync(y.data(), b.y[src], (size_t)n * NCUT_NB * 8, hipMemcpyDeviceToHost, st);
    drain.armed = false;
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    out->values.assign((size_t)n_eig, 0.0);
    out->residual.assign((size_t)n_eig, 0.0);
    out->vectors.assign((size_t)n_eig * n, 0.0);
    for (int k = 0; k < n_eig; ++k) {
        out->values[k] = 2.0 * (1.0 - theta[k]);
        out->residual[k] = resid[k];
        double* const z = out->vectors.data() + (size_t)k * n;
        double nrm = 0.0;
        int big = 0;
        for (int i = 0; i < n; ++i) {
            double u = 0.0;
            for (int a = 0; a < NCUT_NB; ++a) u += y[(size_t)i * NCUT_NB + a] * V[a * NCUT_NB + k];
            z[i] = cs[i] * u;
            nrm += z[i] * z[i];
            if (std::fabs(z[i]) > std::fabs(z[big])) big = i;
        }
        const double sc = nrm > 0.0 ? (z[big] < 0.0 ? -1.0 : 1.0) / std::sqrt(nrm) : 0.0;
        for (int i = 0; i < n; ++i) z[i] *= sc;
    }
    return hipSuccess;
}

}  // namespace dinov2

extern "C" int dinov2_hip_ncut_tokens(dinov2_hip_session* s, const dinov2_hip_ncut* nc, char* err, size_t errlen) {
    if (!s || !nc) {
        set_err(err, errlen, "ncut: null session / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int n = nc->rows.n, H = nc->rows.H;
    if (n < NCUT_N_MIN || n > NCUT_N_MAX || H < 8 || H > 4096) {
        set_err(err, errlen, "ncut: need %d <= n <= %d and 8 <= H <= 4096", NCUT_N_MIN, NCUT_N_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (nc->affinity != DINOV2_HIP_NCUT_THRESHOLD && nc->affinity != DINOV2_HIP_NCUT_RELU && nc->affinity != DINOV2_HIP_NCUT_EXP) {
        set_err(err, errlen, "ncut: unknown affinity %d", (int)nc->affinity);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!ncut_args_ok(n, H, nc->affinity, nc->tau, nc->floor, nc->n_eig, nc->max_iter, nc->tol)) {
        set_err(err, errlen,
                "ncut: need 1 <= n_eig <= %d, 1 <= max_iter <= %d, 1e-6 <= tol <= 1e-1; THRESHOLD: -1 <= tau < 1 and 0 <= floor <= 1; EXP: 2^-6 <= "
                "tau <= 16",
                NCUT_EIG_MAX, NCUT_ITER_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!nc->values && !nc->vectors && !nc->degree && !nc->residual && !nc->iterations && !nc->converged) {
        set_err(err, errlen, "ncut: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (nc->all_images != 0 && (nc->all_images != 1 || nc->rows.source != DINOV2_HIP_ROWS_LAST_PATCHES)) {
        set_err(err, errlen, "ncut: all_images is 0, or 1 with DINOV2_HIP_ROWS_LAST_PATCHES");
        return DINOV2_HIP_ERR_INVALID;
    }
    // the view of the source: row r lives at src + (r / per) * outer + (r % per) * ld floats
    const float* src;
    size_t ld, outer = 0;
    int per = n;
    if (nc->all_images) {
        dinov2_hip_rows one = nc->rows;  // image 0's patch rows stand for the checks of the resident source
        one.image = 0;
        const int P = s->last_b > 0 ? s->last_t - 1 - (int)s->model->hp.num_register_tokens : 0;
        one.n = P > 0 ? P : 1;  // (no forward: the resident check below says so)
        const int rc = check_session_rows("ncut", s, H, &one, &src, &ld, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
        if ((int64_t)n != (int64_t)s->last_b * P) {
            set_err(err, errlen, "ncut: all_images has the %d patch rows of each of the last %d images: n must be %d", P, s->last_b, s->last_b * P);
            return DINOV2_HIP_ERR_INVALID;
        }
        per = P;
        outer = (size_t)s->last_t * H;
    } else {
        const int rc = check_session_rows("ncut", s, H, &nc->rows, &src, &ld, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
    }
    HIP_TRY(hipSetDevice(s->model->device));
    hipStream_t st = s->stream;
    const NcutPlan plan = ncut_plan(n, H, 0);
    const bool given = nc->rows.source == DINOV2_HIP_ROWS_GIVEN, stage = given && !nc->rows.on_device;
    const size_t n_x = (size_t)n * H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_NCUT], plan.bytes + align_up(stage ? n_x : 0, 256), "ncut", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_NCUT].as<char>();
    const NcutBufs b = ncut_bufs(buf, plan);
    NcutResult res;
    {
        DrainOnError drain{st};  // (the staging copy reads the caller's rows)
        if (given) {
            src = nc->rows.data;
            if (stage) {
                HIP_TRY(hipMemcpyAsync(buf + plan.bytes, nc->rows.data, n_x, hipMemcpyHostToDevice, st));
                src = (const float*)(buf + plan.bytes);
            }
        }
        if (nc->all_images) {  // the images' patch rows are not contiguous in the token stream: one launch per image, consecutive row blocks
            for (int i = 0; i < s->last_b; ++i) {
                const bool last = i == s->last_b - 1;
                HIP_TRY(launch_match_normalise(src + (size_t)i * outer, ld, b.x16 + (size_t)i * per * plan.hpad, per,
                                               last ? plan.npad - i * per : per, H, plan.hpad, st));
            }
        } else {
            HIP_TRY(launch_match_normalise(src, ld, b.x16, n, plan.npad, H, plan.hpad, st));
        }
        HIP_TRY(ncut_run(b, n, nc->affinity, nc->tau, nc->floor, nc->n_eig, nc->max_iter, nc->tol, plan, st, &res));
        drain.armed = false;  // (ncut_run's last wait)
    }
    if (!res.finite) {
        set_err(err, errlen, "ncut: non-finite Ritz values (rows that are not finite?)");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int ne = nc->n_eig;
    if (nc->values) std::copy(res.values.begin(), res.values.end(), nc->values);
    if (nc->vectors) std::copy(res.vectors.begin(), res.vectors.end(), nc->vectors);
    if (nc->degree) std::copy(res.degree.begin(), res.degree.end(), nc->degree);
    if (nc->residual) std::copy(res.residual.begin(), res.residual.begin() + ne, nc->residual);
    if (nc->iterations) *nc->iterations = res.iterations;
    if (nc->converged) *nc->converged = res.converged;
    return DINOV2_HIP_OK;
}
