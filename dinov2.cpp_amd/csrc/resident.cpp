// resident.cpp -- what works on rows that stay on the device between calls: nearest rows of two sets (dinov2_hip_match_tokens), the bank of
// normalised rows with its top-k search (dinov2_hip_bank_*), spherical k-means of rows (dinov2_hip_kmeans_tokens), and the lifetime of a dense-prediction head (dinov2_hip_dense_head_*; its
// forward, dinov2_hip_predict_dense, is in model.cpp).
#include <cstring>
#include <memory>

#include "host.h"

using namespace dinov2;

// =============================================================================================================
// nearest rows by cosine similarity, both directions (csrc/match.hip; no reference counterpart)
// =============================================================================================================
extern "C" int dinov2_hip_match_tokens(dinov2_hip_session* s, const dinov2_hip_match* m, char* err, size_t errlen) {
    if (!s || !m) {
        set_err(err, errlen, "match: null session / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    constexpr int NMAX = 1 << 20;
    if (m->na < 1 || m->na > NMAX || m->nb < 1 || m->nb > NMAX || m->H < 8 || m->H > 4096) {
        set_err(err, errlen, "match: need 1 <= na, nb <= %d and 8 <= H <= 4096", NMAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!m->idx_ab && !m->sim_ab && !m->idx_ba && !m->sim_ba) {
        set_err(err, errlen, "match: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int na = m->na, nb = m->nb, H = m->H;
    // a NULL side: the patch rows of one image of the last un-split forward -- rows 1 + R .. T - 1 whatever last_first says (under
    // DINOV2_HIP_CLASSIFY that one includes the registers)
    const int R = (int)s->model->hp.num_register_tokens;
    const int P = s->last_t - 1 - R;
    const struct { const float* p; int n, image; const char* name; } side[2] = {{m->a, na, m->image_a, "a"}, {m->b, nb, m->image_b, "b"}};
    for (const auto& sd : side) {
        if (sd.p) {
            if (m->on_device && ((size_t)sd.p & 15) != 0) {
                set_err(err, errlen, "match: device pointer %s is not 16-byte aligned", sd.name);
                return DINOV2_HIP_ERR_INVALID;
            }
            continue;
        }
        if (s->last_b <= 0 || !s->fin) {
            set_err(err, errlen, "match: %s == NULL means the patch tokens of the session's last un-split forward, and there is none", sd.name);
            return DINOV2_HIP_ERR_INVALID;
        }
        if (sd.n != P || H != (int)s->model->hp.hidden_size) {
            set_err(err, errlen, "match: %s == NULL means the last forward's patch tokens, which are [%d, %d]", sd.name, P,
                    (int)s->model->hp.hidden_size);
            return DINOV2_HIP_ERR_INVALID;
        }
        if (sd.image < 0 || sd.image >= s->last_b) {
            set_err(err, errlen, "match: image_%s %d outside the last batch of %d", sd.name, sd.image, s->last_b);
            return DINOV2_HIP_ERR_INVALID;
        }
    }
    HIP_TRY(hipSetDevice(s->model->device));
    hipStream_t st = s->stream;
    const MatchPlan plan = match_plan(na, nb, H);
    const bool stage_a = m->a && !m->on_device, stage_b = m->b && !m->on_device;
    const size_t n_a = (size_t)na * H * 4, n_b = (size_t)nb * H * 4;
    const size_t o_a = plan.bytes, o_b = o_a + align_up(stage_a ? n_a : 0, 256), need = o_b + align_up(stage_b ? n_b : 0, 256);
    const int rs = reserve(s, s->scratch[SCRATCH_MATCH], need, "match", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* buf = s->scratch[SCRATCH_MATCH].as<char>();
    const float* src[2];
    for (int k = 0; k < 2; ++k) {
        const auto& sd = side[k];
        if (!sd.p) {
            src[k] = s->fin + ((size_t)sd.image * s->last_t + 1 + R) * H;
        } else if (!m->on_device) {
            float* dst = (float*)(buf + (k == 0 ? o_a : o_b));
            HIP_TRY(hipMemcpyAsync(dst, sd.p, k == 0 ? n_a : n_b, hipMemcpyHostToDevice, st));
            src[k] = dst;
        } else {
            src[k] = sd.p;
        }
    }
    HIP_TRY(launch_match(src[0], (size_t)H, src[1], (size_t)H, na, nb, H, buf, plan, st));
    if (m->idx_ab) HIP_TRY(hipMemcpyAsync(m->idx_ab, buf + plan.idx_ab, (size_t)na * 4, hipMemcpyDeviceToHost, st));
    if (m->sim_ab) HIP_TRY(hipMemcpyAsync(m->sim_ab, buf + plan.sim_ab, (size_t)na * 4, hipMemcpyDeviceToHost, st));
    if (m->idx_ba) HIP_TRY(hipMemcpyAsync(m->idx_ba, buf + plan.idx_ba, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    if (m->sim_ba) HIP_TRY(hipMemcpyAsync(m->sim_ba, buf + plan.sim_ba, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DINOV2_HIP_OK;
}

// =============================================================================================================
// a resident bank of normalised rows and its top-k search (csrc/bank.hip; no reference counterpart)
// =============================================================================================================
extern "C" int dinov2_hip_bank_create(dinov2_hip_model* model, int32_t H, int32_t capacity, dinov2_hip_bank** out, char* err, size_t errlen) {
    if (!model || !out) {
        set_err(err, errlen, "bank_create: null model / out");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (H < 8 || H > 4096 || capacity < 1 || capacity > (1 << 24)) {
        set_err(err, errlen, "bank_create: need 8 <= H <= 4096 and 1 <= capacity <= %d", 1 << 24);
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(model->device));
    std::unique_ptr<dinov2_hip_bank> b(new dinov2_hip_bank);
    b->device = model->device;
    b->H = H;
    b->hpad = (H + 63) / 64 * 64;
    b->capacity = capacity;
    b->cap_pad = (capacity + MATCH_TN - 1) / MATCH_TN * MATCH_TN;
    const size_t bytes = (size_t)b->cap_pad * b->hpad * 2;
    hipError_t e = hipMalloc((void**)&b->rows, bytes);
    if (e == hipSuccess) {
        e = hipMemset(b->rows, 0, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) (void)hipFree(b->rows);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (not left behind for the next launch to report)
        set_err(err, errlen, "bank_create: %zu bytes refused: %s", bytes, hipGetErrorString(e));
        return DINOV2_HIP_ERR_HIP;
    }
    *out = b.release();
    return DINOV2_HIP_OK;
}

extern "C" void dinov2_hip_bank_free(dinov2_hip_bank* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();  // a session's stream may still be reading the rows
    if (b->rows) (void)hipFree(b->rows);
    delete b;
}

extern "C" int dinov2_hip_bank_count(const dinov2_hip_bank* b) { return b ? b->count : 0; }

extern "C" int dinov2_hip_bank_clear(dinov2_hip_bank* b) {
    if (!b) return DINOV2_HIP_ERR_INVALID;
    b->count = 0;  // the memory stays as it is: the sweep masks on count
    return DINOV2_HIP_OK;
}

namespace {
// Checks a dinov2_hip_rows of row width H against the session; on success *src / *ld are the device view of a resident source (nullptr for
// DINOV2_HIP_ROWS_GIVEN).  Touches nothing.
int check_rows(const char* who, const dinov2_hip_session* s, int H, const dinov2_hip_rows* r, const float** src, size_t* ld, char* err,
               size_t errlen) {
    *src = nullptr;
    *ld = (size_t)H;
    if (r->n < 1 || r->n > (1 << 24)) {
        set_err(err, errlen, "%s: need 1 <= n <= %d", who, 1 << 24);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (r->source == DINOV2_HIP_ROWS_GIVEN) {
        if (!r->data) {
            set_err(err, errlen, "%s: DINOV2_HIP_ROWS_GIVEN with data == NULL", who);
            return DINOV2_HIP_ERR_INVALID;
        }
        if (r->on_device && ((size_t)r->data & 15) != 0) {
            set_err(err, errlen, "%s: the device pointer is not 16-byte aligned", who);
            return DINOV2_HIP_ERR_INVALID;
        }
        return DINOV2_HIP_OK;
    }
    if (r->source != DINOV2_HIP_ROWS_LAST_CLS && r->source != DINOV2_HIP_ROWS_LAST_PATCHES) {
        set_err(err, errlen, "%s: unknown rows source %d", who, r->source);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (s->last_b <= 0 || !s->fin) {
        set_err(err, errlen, "%s: a resident source means rows of the session's last un-split forward, and there is none", who);
        return DINOV2_HIP_ERR_INVALID;
    }
    const int Hm = (int)s->model->hp.hidden_size, R = (int)s->model->hp.num_register_tokens, T = s->last_t, P = T - 1 - R;
    if (r->H != Hm) {
        set_err(err, errlen, "%s: a resident source has the model's hidden size %d, not %d", who, Hm, r->H);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (r->source == DINOV2_HIP_ROWS_LAST_CLS) {
        if (r->n != s->last_b) {
            set_err(err, errlen, "%s: LAST_CLS has one row per image of the last batch: n must be %d", who, s->last_b);
            return DINOV2_HIP_ERR_INVALID;
        }
        *src = s->fin;  // row 0 of every image
        *ld = (size_t)T * Hm;
    } else {
        if (r->n != P) {
            set_err(err, errlen, "%s: LAST_PATCHES has the last forward's %d patch rows: n must be %d", who, P, P);
            return DINOV2_HIP_ERR_INVALID;
        }
        if (r->image < 0 || r->image >= s->last_b) {
            set_err(err, errlen, "%s: image %d outside the last batch of %d", who, r->image, s->last_b);
            return DINOV2_HIP_ERR_INVALID;
        }
        *src = s->fin + ((size_t)r->image * T + 1 + R) * Hm;
        *ld = (size_t)Hm;
    }
    return DINOV2_HIP_OK;
}
// The same against a bank: its device and its H first.
int check_rows(const char* who, const dinov2_hip_session* s, const dinov2_hip_bank* b, const dinov2_hip_rows* r, const float** src, size_t* ld,
               char* err, size_t errlen) {
    *src = nullptr;
    *ld = (size_t)b->H;
    if (s->model->device != b->device) {
        set_err(err, errlen, "%s: the session is on device %d, the bank on device %d", who, s->model->device, b->device);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (r->H != b->H) {
        set_err(err, errlen, "%s: rows have H = %d, the bank %d", who, r->H, b->H);
        return DINOV2_HIP_ERR_INVALID;
    }
    return check_rows(who, s, b->H, r, src, ld, err, errlen);
}
}  // namespace

extern "C" int dinov2_hip_bank_add(dinov2_hip_session* s, dinov2_hip_bank* b, const dinov2_hip_rows* rows, int32_t* first, char* err,
                                   size_t errlen) {
    if (!s || !b || !rows) {
        set_err(err, errlen, "bank_add: null session / bank / rows");
        return DINOV2_HIP_ERR_INVALID;
    }
    const float* src;
    size_t ld;
    const int rc = check_rows("bank_add", s, b, rows, &src, &ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (rows->n > b->capacity - b->count) {
        set_err(err, errlen, "bank_add: %d rows do not fit: the bank holds %d of %d", rows->n, b->count, b->capacity);
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;
    const int n = rows->n;
    if (rows->source == DINOV2_HIP_ROWS_GIVEN) {
        src = rows->data;
        if (!rows->on_device) {
            const size_t bytes = (size_t)n * b->H * 4;
            const int rs = reserve(s, s->scratch[SCRATCH_BANK], align_up(bytes, 256), "bank_add", err, errlen);
            if (rs != DINOV2_HIP_OK) return rs;
            HIP_TRY(hipMemcpyAsync(s->scratch[SCRATCH_BANK].ptr, rows->data, bytes, hipMemcpyHostToDevice, st));
            src = s->scratch[SCRATCH_BANK].as<float>();
        }
    }
    // rows [count, count + n) only: what lies past them is not touched (it is masked, not assumed zero)
    HIP_TRY(launch_match_normalise(src, ld, b->rows + (size_t)b->count * b->hpad, n, n, b->H, b->hpad, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (first) *first = b->count;
    b->count += n;
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_bank_topk(dinov2_hip_session* s, const dinov2_hip_bank* b, const dinov2_hip_topk* q, char* err, size_t errlen) {
    if (!s || !b || !q) {
        set_err(err, errlen, "bank_topk: null session / bank / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (q->k < 1 || q->k > BANK_K_MAX) {
        set_err(err, errlen, "bank_topk: need 1 <= k <= %d", BANK_K_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!q->idx && !q->sim) {
        set_err(err, errlen, "bank_topk: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    const float* src;
    size_t ld;
    const int rc = check_rows("bank_topk", s, b, &q->queries, &src, &ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (q->queries.n > (1 << 20)) {
        set_err(err, errlen, "bank_topk: at most %d queries a call", 1 << 20);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (b->count < 1) {
        set_err(err, errlen, "bank_topk: the bank is empty");
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;
    const int nq = q->queries.n, k = q->k;
    const BankTopkPlan plan = bank_topk_plan(nq, b->count, b->H, k, 0);
    const bool stage = q->queries.source == DINOV2_HIP_ROWS_GIVEN && !q->queries.on_device;
    const size_t n_q = (size_t)nq * b->H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_BANK], plan.bytes + align_up(stage ? n_q : 0, 256), "bank_topk", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_BANK].as<char>();
    if (q->queries.source == DINOV2_HIP_ROWS_GIVEN) {
        src = q->queries.data;
        if (stage) {
            HIP_TRY(hipMemcpyAsync(buf + plan.bytes, q->queries.data, n_q, hipMemcpyHostToDevice, st));
            src = (const float*)(buf + plan.bytes);
        }
    }
    HIP_TRY(launch_bank_topk(src, ld, nq, b->rows, b->count, b->H, k, buf, plan, false, st));
    if (q->idx) HIP_TRY(hipMemcpyAsync(q->idx, buf + plan.idx, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    if (q->sim) HIP_TRY(hipMemcpyAsync(q->sim, buf + plan.sim, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return DINOV2_HIP_OK;
}

// =============================================================================================================
// spherical k-means of token rows (csrc/kmeans.hip; no reference counterpart)
// =============================================================================================================
extern "C" int dinov2_hip_kmeans_tokens(dinov2_hip_session* s, const dinov2_hip_kmeans* km, char* err, size_t errlen) {
    if (!s || !km) {
        set_err(err, errlen, "kmeans: null session / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int n = km->rows.n, H = km->rows.H, K = km->K;
    if (n < 1 || n > KMEANS_N_MAX || H < 8 || H > 4096) {
        set_err(err, errlen, "kmeans: need 1 <= n <= %d and 8 <= H <= 4096", KMEANS_N_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (K < 1 || K > KMEANS_K_MAX || km->max_iter < 0 || km->max_iter > KMEANS_ITER_MAX) {
        set_err(err, errlen, "kmeans: need 1 <= K <= %d and 0 <= max_iter <= %d", KMEANS_K_MAX, KMEANS_ITER_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (km->init != DINOV2_HIP_KMEANS_INIT_GIVEN && km->init != DINOV2_HIP_KMEANS_INIT_ROWS) {
        set_err(err, errlen, "kmeans: unknown init %d", (int)km->init);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (km->init == DINOV2_HIP_KMEANS_INIT_GIVEN ? !km->init_centers : !km->init_rows) {
        set_err(err, errlen, "kmeans: init %d without its %s", (int)km->init, km->init == DINOV2_HIP_KMEANS_INIT_GIVEN ? "init_centers" : "init_rows");
        return DINOV2_HIP_ERR_INVALID;
    }
    for (int j = 0; km->init == DINOV2_HIP_KMEANS_INIT_ROWS && j < K; ++j)
        if (km->init_rows[j] < 0 || km->init_rows[j] >= n) {
            set_err(err, errlen, "kmeans: init_rows[%d] = %d outside [0, %d)", j, (int)km->init_rows[j], n);
            return DINOV2_HIP_ERR_INVALID;
        }
    if (!km->labels && !km->sim && !km->centers && !km->counts && !km->iterations && !km->converged) {
        set_err(err, errlen, "kmeans: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (km->all_images != 0 && (km->all_images != 1 || km->rows.source != DINOV2_HIP_ROWS_LAST_PATCHES)) {
        set_err(err, errlen, "kmeans: all_images is 0, or 1 with DINOV2_HIP_ROWS_LAST_PATCHES");
        return DINOV2_HIP_ERR_INVALID;
    }
    // the view of the source: row r lives at src + (r / per) * outer + (r % per) * ld floats
    const float* src;
    size_t ld;
    int per = n;
    size_t outer = 0;
    if (km->all_images) {
        dinov2_hip_rows one = km->rows;  // image 0's patch rows stand for the checks of the resident source
        one.image = 0;
        const int P = s->last_b > 0 ? s->last_t - 1 - (int)s->model->hp.num_register_tokens : 0;
        one.n = P > 0 ? P : 1;  // (no forward: the resident check below says so)
        const int rc = check_rows("kmeans", s, H, &one, &src, &ld, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
        if ((int64_t)n != (int64_t)s->last_b * P) {
            set_err(err, errlen, "kmeans: all_images has the %d patch rows of each of the last %d images: n must be %d", P, s->last_b, s->last_b * P);
            return DINOV2_HIP_ERR_INVALID;
        }
        per = P;
        outer = (size_t)s->last_t * H;
    } else {
        const int rc = check_rows("kmeans", s, H, &km->rows, &src, &ld, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
        if (km->rows.source == DINOV2_HIP_ROWS_LAST_CLS) {  // one row per image
            per = 1;
            outer = ld;
        }
    }
    HIP_TRY(hipSetDevice(s->model->device));
    hipStream_t st = s->stream;
    const KmeansPlan plan = kmeans_plan(n, K, H, 0);
    const bool stage = km->rows.source == DINOV2_HIP_ROWS_GIVEN && !km->rows.on_device;
    const size_t n_x = (size_t)n * H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_KMEANS], plan.bytes + align_up(stage ? n_x : 0, 256), "kmeans", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_KMEANS].as<char>();
    const KmeansBufs b = kmeans_bufs(buf, plan);
    if (km->rows.source == DINOV2_HIP_ROWS_GIVEN) {
        src = km->rows.data;
        if (stage) {
            HIP_TRY(hipMemcpyAsync(buf + plan.bytes, km->rows.data, n_x, hipMemcpyHostToDevice, st));
            src = (const float*)(buf + plan.bytes);
        }
    }
    if (km->all_images) {  // the images' patch rows are not contiguous in the token stream: one launch per image, consecutive row blocks
        for (int i = 0; i < s->last_b; ++i) {
            const bool last = i == s->last_b - 1;
            HIP_TRY(launch_match_normalise(src + (size_t)i * outer, ld, b.x16 + (size_t)i * per * plan.hpad, per,
                                           last ? plan.npad - i * per : per, H, plan.hpad, st));
        }
    } else {
        HIP_TRY(launch_match_normalise(src, ld, b.x16, n, plan.npad, H, plan.hpad, st));
    }
    if (km->init == DINOV2_HIP_KMEANS_INIT_GIVEN) {
        HIP_TRY(hipMemcpyAsync(b.cvec, km->init_centers, (size_t)K * H * 4, hipMemcpyHostToDevice, st));
    } else {
        int* const idx = (int*)(buf + plan.init);
        HIP_TRY(hipMemcpyAsync(idx, km->init_rows, (size_t)K * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_kmeans_gather(src, per, outer, ld, idx, K, H, b.cvec, st));
    }
    int iterations = 0, converged = 0;
    HIP_TRY(kmeans_run(b, n, K, H, km->max_iter, plan, st, &iterations, &converged));
    if (km->labels) HIP_TRY(hipMemcpyAsync(km->labels, b.labels, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (km->sim) HIP_TRY(hipMemcpyAsync(km->sim, b.sim, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (km->centers) HIP_TRY(hipMemcpyAsync(km->centers, b.cvec, (size_t)K * H * 4, hipMemcpyDeviceToHost, st));
    if (km->counts) HIP_TRY(hipMemcpyAsync(km->counts, b.counts, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (km->iterations) *km->iterations = iterations;
    if (km->converged) *km->converged = converged;
    return DINOV2_HIP_OK;
}

// =============================================================================================================
// linear dense-prediction heads (csrc/dense.hip; no reference counterpart; upstream DINOv2: BNHead of eval/segmentation and eval/depth)
// =============================================================================================================
extern "C" int dinov2_hip_dense_head_create(dinov2_hip_model* model, const dinov2_hip_dense_desc* d, dinov2_hip_dense_head** out, char* err,
                                            size_t errlen) {
    if (!model || !d || !out || !d->layers || !d->weight) {
        set_err(err, errlen, "dense_head_create: null model / desc / out / layer list / weight");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int L = (int)model->hp.num_hidden_layers, H = (int)model->hp.hidden_size;
    if (d->n_layers < 1 || d->n_layers > DENSE_LAYERS_MAX) {
        set_err(err, errlen, "dense_head_create: n_layers %d outside 1 .. %d", (int)d->n_layers, DENSE_LAYERS_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (int bad; check_layer_list(d->layers, d->n_layers, 0, L, &bad) != LAYER_LIST_OK) {
        set_err(err, errlen, "dense_head_create: the layer list must be strictly ascending, each layer in 0 .. %d", L);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (d->num_classes < DENSE_C_MIN || d->num_classes > DENSE_C_MAX) {
        set_err(err, errlen, "dense_head_create: num_classes %d outside %d .. %d", (int)d->num_classes, DENSE_C_MIN, DENSE_C_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (d->reduce != DINOV2_HIP_DENSE_ARGMAX && d->reduce != DINOV2_HIP_DENSE_BINS) {
        set_err(err, errlen, "dense_head_create: unknown reduce %d", (int)d->reduce);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (d->reduce == DINOV2_HIP_DENSE_BINS && (!d->bin_centers || !(d->bins_eps > 0.0f))) {
        set_err(err, errlen, "dense_head_create: DINOV2_HIP_DENSE_BINS needs bin_centers and bins_eps > 0");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (H % 64 != 0 || H > 2048) {
        set_err(err, errlen, "dense_head_create: hidden size %d is not a multiple of 64 up to 2048", H);
        return DINOV2_HIP_ERR_INVALID;
    }
    std::unique_ptr<dinov2_hip_dense_head> hd(new dinov2_hip_dense_head);
    hd->device = model->device;
    hd->H = H;
    hd->L = L;
    hd->n_layers = d->n_layers;
    for (int i = 0; i < d->n_layers; ++i) hd->layers[i] = d->layers[i];
    hd->norm = d->norm != 0;
    hd->concat_cls = d->concat_cls != 0;
    hd->C = d->num_classes;
    hd->cpad = dense_cpad(hd->C);
    hd->K = d->n_layers * H * (hd->concat_cls ? 2 : 1);
    hd->reduce = d->reduce;
    hd->eps = d->reduce == DINOV2_HIP_DENSE_BINS ? d->bins_eps : 0.0f;
    const size_t C = (size_t)hd->C, cpad = (size_t)hd->cpad, K = (size_t)hd->K;
    const size_t wbytes = align_up(cpad * K * 2, 256), vbytes = align_up(cpad * 4, 256), bytes = wbytes + 2 * vbytes;
    std::vector<char> host(bytes, 0);  // rows past C of the weight, the bias and the centres stay zero
    _Float16* const w16 = (_Float16*)host.data();
    for (size_t i = 0; i < C * K; ++i) w16[i] = (_Float16)d->weight[i];  // round to nearest even
    if (d->bias) std::memcpy(host.data() + wbytes, d->bias, C * 4);
    if (d->reduce == DINOV2_HIP_DENSE_BINS) std::memcpy(host.data() + wbytes + vbytes, d->bin_centers, C * 4);
    HIP_TRY(hipSetDevice(model->device));
    hipError_t e = hipMalloc((void**)&hd->dev, bytes);
    if (e == hipSuccess) {
        e = hipMemcpy(hd->dev, host.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(hd->dev);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (not left behind for the next launch to report)
        set_err(err, errlen, "dense_head_create: %zu bytes refused: %s", bytes, hipGetErrorString(e));
        return DINOV2_HIP_ERR_HIP;
    }
    hd->w16 = (_Float16*)hd->dev;
    hd->bias = (float*)(hd->dev + wbytes);
    hd->centers = (float*)(hd->dev + wbytes + vbytes);
    *out = hd.release();
    return DINOV2_HIP_OK;
}

extern "C" void dinov2_hip_dense_head_free(dinov2_hip_dense_head* hd) {
    if (!hd) return;
    (void)hipSetDevice(hd->device);
    (void)hipDeviceSynchronize();  // a session's stream may still be reading the weight
    if (hd->dev) (void)hipFree(hd->dev);
    delete hd;
}

// =============================================================================================================
// check_rows for the host files beside this one (host.h; vlad.cpp)
// =============================================================================================================
int dinov2::check_session_rows(const char* who, const dinov2_hip_session* s, int H, const dinov2_hip_rows* r, const float** src, size_t* ld,
                               char* err, size_t errlen) {
    return check_rows(who, s, H, r, src, ld, err, errlen);
}
