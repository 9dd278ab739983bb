// rerank.cpp -- dinov2_hip_bank_rerank (include/dinov2_hip.h): row ranges of a bank scored against one query set on the device
// (csrc/rerank.hip; no reference counterpart).  Beside resident.cpp, whose check of a rows source it shares (host.h check_session_rows).
#include <cmath>

#include "host.h"

using namespace dinov2;

extern "C" int dinov2_hip_bank_rerank(dinov2_hip_session* s, const dinov2_hip_bank* b, const dinov2_hip_rerank* r, char* err, size_t errlen) {
    if (!s || !b || !r) {
        set_err(err, errlen, "bank_rerank: null session / bank / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (s->model->device != b->device) {
        set_err(err, errlen, "bank_rerank: the session is on device %d, the bank on device %d", s->model->device, b->device);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (r->queries.H != b->H) {
        set_err(err, errlen, "bank_rerank: rows have H = %d, the bank %d", r->queries.H, b->H);
        return DINOV2_HIP_ERR_INVALID;
    }
    const float* src;
    size_t ld;
    const int rc = check_session_rows("bank_rerank", s, b->H, &r->queries, &src, &ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const int n = r->queries.n, n_seg = r->n_seg;
    if (n > RERANK_N_MAX) {
        set_err(err, errlen, "bank_rerank: at most %d queries a call", RERANK_N_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (b->count < 1) {
        set_err(err, errlen, "bank_rerank: the bank is empty");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (n_seg < 1 || n_seg > RERANK_SEG_MAX || !r->first || !r->len) {
        set_err(err, errlen, "bank_rerank: need 1 <= n_seg <= %d and first / len", RERANK_SEG_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    for (int i = 0; i < n_seg; ++i)
        if (r->len[i] < 1 || r->len[i] > RERANK_LEN_MAX || r->first[i] < 0 || r->first[i] > b->count - r->len[i]) {
            set_err(err, errlen, "bank_rerank: segment %d is rows [%d, %d + %d): need 1 <= len <= %d inside the bank's %d rows", i, (int)r->first[i],
                    (int)r->first[i], (int)r->len[i], RERANK_LEN_MAX, b->count);
            return DINOV2_HIP_ERR_INVALID;
        }
    if (std::isnan(r->min_sim)) {
        set_err(err, errlen, "bank_rerank: min_sim is NaN (-INFINITY = every mutual pair counts)");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!r->score_q && !r->score_b && !r->mutual && !r->mutual_sim) {
        set_err(err, errlen, "bank_rerank: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;
    RerankTables tables;  // (lives until the wait below: the uploads read it)
    const RerankPlan plan = rerank_plan(n, b->H, n_seg, r->first, r->len, 0, &tables);
    const bool stage = r->queries.source == DINOV2_HIP_ROWS_GIVEN && !r->queries.on_device;
    const size_t n_q = (size_t)n * b->H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_RERANK], plan.bytes + align_up(stage ? n_q : 0, 256), "bank_rerank", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_RERANK].as<char>();
    if (r->queries.source == DINOV2_HIP_ROWS_GIVEN) {
        src = r->queries.data;
        if (stage) {
            HIP_TRY(hipMemcpyAsync(buf + plan.bytes, r->queries.data, n_q, hipMemcpyHostToDevice, st));
            src = (const float*)(buf + plan.bytes);
        }
    }
    hipError_t e = launch_rerank(src, ld, n, b->H, b->rows, b->cap_pad - 1, n_seg, r->min_sim, buf, plan, tables, st);
    const size_t bytes = (size_t)n_seg * 4;
    if (e == hipSuccess && r->score_q) e = hipMemcpyAsync(r->score_q, buf + plan.score_q, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && r->score_b) e = hipMemcpyAsync(r->score_b, buf + plan.score_b, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && r->mutual) e = hipMemcpyAsync(r->mutual, buf + plan.mutual, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && r->mutual_sim) e = hipMemcpyAsync(r->mutual_sim, buf + plan.mutual_sim, bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // (on an error too: the tables and the caller's arrays may be in flight)
    HIP_TRY(e);
    HIP_TRY(es);
    return DINOV2_HIP_OK;
}
