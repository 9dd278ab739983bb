// propagate.cpp -- dinov2_hip_propmem_* and dinov2_hip_propagate (include/dinov2_hip.h): a resident memory of frames and label propagation
// from it to the patches of a new frame (csrc/propagate.hip; no reference counterpart).  Beside resident.cpp, whose check of a rows source
// it shares (host.h check_session_rows).  Every call that launches has one wait, at its end.
#include <cmath>
#include <memory>
#include <vector>

#include "host.h"

using namespace dinov2;

extern "C" int dinov2_hip_propmem_create(dinov2_hip_model* model, int32_t H, int32_t h0, int32_t w0, int32_t frames, int32_t C,
                                         dinov2_hip_propmem** out, char* err, size_t errlen) {
    if (!model || !out) {
        set_err(err, errlen, "propmem_create: null model / out");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (H < 8 || H > 4096 || h0 < 1 || h0 > PROP_GRID_MAX || w0 < 1 || w0 > PROP_GRID_MAX || frames < 1 || frames > PROP_FRAMES_MAX || C < 1 ||
        C > PROP_C_MAX) {
        set_err(err, errlen, "propmem_create: need 8 <= H <= 4096, 1 <= h0, w0 <= %d, 1 <= frames <= %d and 1 <= C <= %d", PROP_GRID_MAX,
                PROP_FRAMES_MAX, PROP_C_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    const int P = h0 * w0, ppad = (P + MATCH_TN - 1) / MATCH_TN * MATCH_TN;
    if ((int64_t)frames * ppad > PROP_ROWS_MAX) {
        set_err(err, errlen, "propmem_create: frames * padded patches = %lld is above 2^24", (long long)frames * ppad);
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(model->device));
    std::unique_ptr<dinov2_hip_propmem> m(new dinov2_hip_propmem);
    m->device = model->device;
    m->H = H;
    m->hpad = (H + 63) / 64 * 64;
    m->h0 = h0;
    m->w0 = w0;
    m->P = P;
    m->ppad = ppad;
    m->frames = frames;
    m->C = C;
    m->lay = propmem_layout(frames, P, ppad, m->hpad, C);
    std::vector<uint32_t> cells((size_t)ppad, 0u);
    for (int p = 0; p < P; ++p) cells[p] = propagate_cell(p, w0);
    hipError_t e = hipMalloc((void**)&m->dev, m->lay.bytes);
    if (e == hipSuccess) {
        e = hipMemset(m->dev, 0, m->lay.bytes);
        if (e == hipSuccess) e = hipMemcpy(m->dev + m->lay.cells, cells.data(), cells.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) (void)hipFree(m->dev);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (not left behind for the next launch to report)
        set_err(err, errlen, "propmem_create: %zu bytes refused: %s", m->lay.bytes, hipGetErrorString(e));
        return DINOV2_HIP_ERR_HIP;
    }
    *out = m.release();
    return DINOV2_HIP_OK;
}

extern "C" void dinov2_hip_propmem_free(dinov2_hip_propmem* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();  // a session's stream may still be reading the rows
    if (m->dev) (void)hipFree(m->dev);
    delete m;
}

extern "C" int dinov2_hip_propmem_drop(dinov2_hip_propmem* m, int32_t slot) {
    if (!m || slot < 0 || slot >= m->frames) return DINOV2_HIP_ERR_INVALID;
    m->filled &= ~(1ull << slot);  // the memory stays as it is: the sweep walks the set slots only
    return DINOV2_HIP_OK;
}

namespace {
// The rows of a set or a propagate against the memory and the session: the device and H first, LAST_CLS refused, n == P.  On success *src /
// *ld are the device view of a resident source (nullptr for DINOV2_HIP_ROWS_GIVEN).  Touches nothing.
int check_rows(const char* who, const dinov2_hip_session* s, const dinov2_hip_propmem* m, const dinov2_hip_rows* r, const float** src, size_t* ld,
               char* err, size_t errlen) {
    *src = nullptr;
    *ld = (size_t)m->H;
    if (s->model->device != m->device) {
        set_err(err, errlen, "%s: the session is on device %d, the memory on device %d", who, s->model->device, m->device);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (r->H != m->H) {
        set_err(err, errlen, "%s: rows have H = %d, the memory %d", who, r->H, m->H);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (r->source == DINOV2_HIP_ROWS_LAST_CLS) {
        set_err(err, errlen, "%s: DINOV2_HIP_ROWS_LAST_CLS is no frame of patches: use GIVEN or LAST_PATCHES", who);
        return DINOV2_HIP_ERR_INVALID;
    }
    const int rc = check_session_rows(who, s, m->H, r, src, ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (r->n != m->P) {
        set_err(err, errlen, "%s: the memory's grid is %d x %d: n must be %d, not %d", who, m->h0, m->w0, m->P, r->n);
        return DINOV2_HIP_ERR_INVALID;
    }
    return DINOV2_HIP_OK;
}
}  // namespace

extern "C" int dinov2_hip_propmem_set(dinov2_hip_session* s, dinov2_hip_propmem* m, int32_t slot, const dinov2_hip_rows* rows, const float* labels,
                                      int32_t labels_on_device, char* err, size_t errlen) {
    if (!s || !m || !rows) {
        set_err(err, errlen, "propmem_set: null session / memory / rows");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (slot < 0 || slot >= m->frames) {
        set_err(err, errlen, "propmem_set: slot %d outside 0 .. %d", (int)slot, m->frames - 1);
        return DINOV2_HIP_ERR_INVALID;
    }
    const float* src;
    size_t ld;
    const int rc = check_rows("propmem_set", s, m, rows, &src, &ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (!labels && !m->has_kept) {
        set_err(err, errlen, "propmem_set: labels == NULL means the result the last propagate with keep left in this memory, and there is none");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (labels && labels_on_device && ((size_t)labels & 15) != 0) {
        set_err(err, errlen, "propmem_set: the device pointer of the labels is not 16-byte aligned");
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = s->stream;
    const int P = m->P;
    if (rows->source == DINOV2_HIP_ROWS_GIVEN) {
        src = rows->data;
        if (!rows->on_device) {
            const size_t bytes = (size_t)P * m->H * 4;
            const int rs = reserve(s, s->scratch[SCRATCH_PROPAGATE], align_up(bytes, 256), "propmem_set", err, errlen);
            if (rs != DINOV2_HIP_OK) return rs;
            HIP_TRY(hipMemcpyAsync(s->scratch[SCRATCH_PROPAGATE].ptr, rows->data, bytes, hipMemcpyHostToDevice, st));
            src = s->scratch[SCRATCH_PROPAGATE].as<float>();
        }
    }
    m->filled &= ~(1ull << slot);  // a call that fails half way leaves the slot empty
    // rows [0, P) of the slot only: its padding rows are not touched (they are masked, not assumed zero)
    _Float16* const dst = (_Float16*)(m->dev + m->lay.rows) + (size_t)slot * m->ppad * m->hpad;
    HIP_TRY(launch_match_normalise(src, ld, dst, P, P, m->H, m->hpad, st));
    const size_t lbytes = (size_t)P * m->C * 4;
    float* const ldst = (float*)(m->dev + m->lay.labels) + (size_t)slot * P * m->C;
    if (labels)
        HIP_TRY(hipMemcpyAsync(ldst, labels, lbytes, labels_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    else
        HIP_TRY(hipMemcpyAsync(ldst, m->dev + m->lay.kept, lbytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    m->filled |= 1ull << slot;
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_propagate(dinov2_hip_session* s, dinov2_hip_propmem* m, const dinov2_hip_propagate_req* q, char* err, size_t errlen) {
    if (!s || !m || !q) {
        set_err(err, errlen, "propagate: null session / memory / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (q->k < 1 || q->k > BANK_K_MAX || q->radius < -1 || q->radius > PROP_RADIUS_MAX) {
        set_err(err, errlen, "propagate: need 1 <= k <= %d and -1 <= radius <= %d", BANK_K_MAX, PROP_RADIUS_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!std::isfinite(q->temperature) || q->temperature < 1e-3f || q->temperature > 1e3f) {
        set_err(err, errlen, "propagate: the temperature must be finite and in 1e-3 .. 1e3");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (q->keep != 0 && q->keep != 1) {
        set_err(err, errlen, "propagate: keep is 0 or 1");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!q->keep && !q->labels && !q->argmax && !q->idx && !q->sim) {
        set_err(err, errlen, "propagate: no output requested and keep == 0");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (q->slots == 0 || (q->slots & ~m->filled) != 0) {
        set_err(err, errlen, "propagate: slots 0x%llx must name at least one slot and filled slots only (filled: 0x%llx)",
                (unsigned long long)q->slots, (unsigned long long)m->filled);
        return DINOV2_HIP_ERR_INVALID;
    }
    const float* src;
    size_t ld;
    const int rc = check_rows("propagate", s, m, &q->queries, &src, &ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = s->stream;
    const int P = m->P, k = q->k, C = m->C;
    const PropagatePlan plan = propagate_plan(m->h0, m->w0, m->H, __builtin_popcountll(q->slots), q->radius, k, C, 0);
    const bool stage = q->queries.source == DINOV2_HIP_ROWS_GIVEN && !q->queries.on_device;
    const size_t n_q = (size_t)P * m->H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_PROPAGATE], plan.bytes + align_up(stage ? n_q : 0, 256), "propagate", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_PROPAGATE].as<char>();
    if (q->queries.source == DINOV2_HIP_ROWS_GIVEN) {
        src = q->queries.data;
        if (stage) {
            HIP_TRY(hipMemcpyAsync(buf + plan.bytes, q->queries.data, n_q, hipMemcpyHostToDevice, st));
            src = (const float*)(buf + plan.bytes);
        }
    }
    const PropMemView view{(const _Float16*)(m->dev + m->lay.rows), (const float*)(m->dev + m->lay.labels), (float*)(m->dev + m->lay.kept),
                           (const uint32_t*)(m->dev + m->lay.cells), m->h0, m->w0, C};
    if (q->keep) m->has_kept = false;  // a call that fails half way leaves no kept result
    HIP_TRY(launch_propagate(src, ld, m->H, view, q->slots, q->radius, k, q->temperature, q->keep != 0, buf, plan, st));
    if (q->labels) HIP_TRY(hipMemcpyAsync(q->labels, buf + plan.out, (size_t)P * C * 4, hipMemcpyDeviceToHost, st));
    if (q->argmax) HIP_TRY(hipMemcpyAsync(q->argmax, buf + plan.argmax, (size_t)P * 4, hipMemcpyDeviceToHost, st));
    if (q->idx) HIP_TRY(hipMemcpyAsync(q->idx, buf + plan.idx, (size_t)P * k * 4, hipMemcpyDeviceToHost, st));
    if (q->sim) HIP_TRY(hipMemcpyAsync(q->sim, buf + plan.sim, (size_t)P * k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (q->keep) m->has_kept = true;
    return DINOV2_HIP_OK;
}
