// probe.cpp -- dinov2_hip_bank_topk_probe (include/dinov2_hip.h): per query the k best rows over the union of its own subset of row ranges
// of a bank, on the device (csrc/probe.hip; no reference counterpart).  Beside rerank.cpp, whose shape it has; the check of a rows source is
// resident.cpp's (host.h check_session_rows), the check of the segments and the probe table kernels.h' probe_check.
#include "host.h"

using namespace dinov2;

extern "C" int dinov2_hip_bank_topk_probe(dinov2_hip_session* s, const dinov2_hip_bank* b, const dinov2_hip_topk_probe* p, char* err,
                                          size_t errlen) {
    if (!s || !b || !p) {
        set_err(err, errlen, "bank_topk_probe: null session / bank / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (s->model->device != b->device) {
        set_err(err, errlen, "bank_topk_probe: the session is on device %d, the bank on device %d", s->model->device, b->device);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (p->queries.H != b->H) {
        set_err(err, errlen, "bank_topk_probe: rows have H = %d, the bank %d", p->queries.H, b->H);
        return DINOV2_HIP_ERR_INVALID;
    }
    const float* src;
    size_t ld;
    const int rc = check_session_rows("bank_topk_probe", s, b->H, &p->queries, &src, &ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (!p->idx && !p->sim) {
        set_err(err, errlen, "bank_topk_probe: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int n = p->queries.n, k = p->k;
    char why[192];
    if (!probe_check(b->count, n, p->n_seg, p->first, p->len, p->n_probe, p->probe, k, why, sizeof(why))) {
        set_err(err, errlen, "bank_topk_probe: %s", why);
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;
    ProbeTables tables;  // (lives until the wait below: the uploads read it)
    const ProbePlan plan = probe_plan(n, b->H, k, p->n_seg, p->first, p->len, p->n_probe, p->probe, 0, 0, PROBE_FORM_AUTO, &tables);
    const bool stage = p->queries.source == DINOV2_HIP_ROWS_GIVEN && !p->queries.on_device;
    const size_t n_q = (size_t)n * b->H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_PROBE], plan.bytes + align_up(stage ? n_q : 0, 256), "bank_topk_probe", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_PROBE].as<char>();
    if (p->queries.source == DINOV2_HIP_ROWS_GIVEN) {
        src = p->queries.data;
        if (stage) {
            HIP_TRY(hipMemcpyAsync(buf + plan.bytes, p->queries.data, n_q, hipMemcpyHostToDevice, st));
            src = (const float*)(buf + plan.bytes);
        }
    }
    hipError_t e = launch_probe(src, ld, n, b->H, b->rows, b->cap_pad - 1, k, buf, plan, tables, st);
    const size_t bytes = (size_t)n * k * 4;
    if (e == hipSuccess && p->idx) e = hipMemcpyAsync(p->idx, buf + plan.idx, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && p->sim) e = hipMemcpyAsync(p->sim, buf + plan.sim, bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // (on an error too: the tables and the caller's arrays may be in flight)
    HIP_TRY(e);
    HIP_TRY(es);
    return DINOV2_HIP_OK;
}
