// coreset.cpp -- dinov2_hip_coreset_tokens and dinov2_hip_bank_keep (include/dinov2_hip.h): greedy k-center selection of rows on the device
// and the compaction of a bank to a chosen subset (csrc/coreset.hip; no reference counterpart).  Beside resident.cpp, whose check of a rows
// source it shares (host.h check_session_rows).
#include <cmath>

#include "host.h"

using namespace dinov2;

namespace {
// A rows source together with dinov2_hip_kmeans' all_images, viewed on the device: row r lives at src + (r / per) * outer + (r % per) * ld
// floats (src is nullptr for DINOV2_HIP_ROWS_GIVEN: the caller fills it in); `blocks` = the runs of `per` rows that are contiguous.
struct RowsView {
    const float* src;
    size_t ld, outer;
    int per, blocks;
};
// The checks of dinov2_hip_kmeans_tokens for `rows` and `all_images`, word for word.  Touches nothing.
int check_rows_view(const dinov2_hip_session* s, const dinov2_hip_rows* rows, int all_images, RowsView* v, char* err, size_t errlen) {
    const int n = rows->n, H = rows->H;
    if (all_images != 0 && (all_images != 1 || rows->source != DINOV2_HIP_ROWS_LAST_PATCHES)) {
        set_err(err, errlen, "coreset: all_images is 0, or 1 with DINOV2_HIP_ROWS_LAST_PATCHES");
        return DINOV2_HIP_ERR_INVALID;
    }
    *v = RowsView{nullptr, (size_t)H, 0, n, 1};
    if (!all_images) return check_session_rows("coreset", s, H, rows, &v->src, &v->ld, err, errlen);
    dinov2_hip_rows one = *rows;  // image 0's patch rows stand for the checks of the resident source
    one.image = 0;
    const int P = s->last_b > 0 ? s->last_t - 1 - (int)s->model->hp.num_register_tokens : 0;
    one.n = P > 0 ? P : 1;  // (no forward: the resident check below says so)
    const int rc = check_session_rows("coreset", s, H, &one, &v->src, &v->ld, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if ((int64_t)n != (int64_t)s->last_b * P) {
        set_err(err, errlen, "coreset: all_images has the %d patch rows of each of the last %d images: n must be %d", P, s->last_b, s->last_b * P);
        return DINOV2_HIP_ERR_INVALID;
    }
    v->per = P;
    v->outer = (size_t)s->last_t * H;
    v->blocks = s->last_b;
    return DINOV2_HIP_OK;
}
// the n rows, in the caller's order, as match's f16 unit rows into x16 [npad, hpad], the padding rows zero
hipError_t normalise_rows_view(const RowsView& v, int n, _Float16* x16, int npad, int H, int hpad, hipStream_t st) {
    if (v.blocks == 1) return launch_match_normalise(v.src, v.ld, x16, n, npad, H, hpad, st);
    // the images' patch rows are not contiguous in the token stream: one launch per image, consecutive row blocks
    for (int i = 0; i < v.blocks; ++i) {
        const bool last = i == v.blocks - 1;
        const hipError_t e = launch_match_normalise(v.src + (size_t)i * v.outer, v.ld, x16 + (size_t)i * v.per * hpad, v.per,
                                                    last ? npad - i * v.per : v.per, H, hpad, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

extern "C" int dinov2_hip_coreset_tokens(dinov2_hip_session* s, const dinov2_hip_coreset* c, char* err, size_t errlen) {
    if (!s || !c) {
        set_err(err, errlen, "coreset: null session / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    const dinov2_hip_bank* const bank = c->bank;
    const int n = bank ? bank->count : c->rows.n, H = bank ? bank->H : c->rows.H;
    if (bank) {
        if (s->model->device != bank->device) {
            set_err(err, errlen, "coreset: the session is on device %d, the bank on device %d", s->model->device, bank->device);
            return DINOV2_HIP_ERR_INVALID;
        }
        if (n < 1) {
            set_err(err, errlen, "coreset: the bank is empty");
            return DINOV2_HIP_ERR_INVALID;
        }
    } else if (n < 1 || n > CORESET_N_MAX || H < 8 || H > 4096) {
        set_err(err, errlen, "coreset: need 1 <= n <= %d and 8 <= H <= 4096", CORESET_N_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (c->m < 1 || c->m > n || c->first < 0 || c->first >= n) {
        set_err(err, errlen, "coreset: need 1 <= m <= n and 0 <= first < n (n = %d)", n);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (std::isnan(c->stop_sim)) {
        set_err(err, errlen, "coreset: stop_sim is NaN (+INFINITY = never stop)");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!c->idx && !c->cover && !c->selected && !c->nearest && !c->near_sim) {
        set_err(err, errlen, "coreset: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    RowsView v{};
    if (!bank) {
        const int rc = check_rows_view(s, &c->rows, c->all_images, &v, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
    }
    HIP_TRY(hipSetDevice(s->model->device));
    hipStream_t st = s->stream;
    const int m = c->m;
    const CoresetPlan plan = coreset_plan(n, H, m, 0, !bank);  // (a bank's rows are swept where they are)
    const bool stage = !bank && c->rows.source == DINOV2_HIP_ROWS_GIVEN && !c->rows.on_device;
    const size_t n_x = (size_t)n * H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_CORESET], plan.bytes + align_up(stage ? n_x : 0, 256), "coreset", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_CORESET].as<char>();
    const CoresetBufs b = coreset_bufs(buf, plan, bank ? bank->rows : nullptr);
    if (!bank) {
        if (c->rows.source == DINOV2_HIP_ROWS_GIVEN) {
            v.src = c->rows.data;
            if (stage) {
                HIP_TRY(hipMemcpyAsync(buf + plan.bytes, c->rows.data, n_x, hipMemcpyHostToDevice, st));
                v.src = (const float*)(buf + plan.bytes);
            }
        }
        HIP_TRY(normalise_rows_view(v, n, (_Float16*)(buf + plan.x16), plan.npad, H, plan.hpad, st));
    }
    HIP_TRY(coreset_run(b, n, m, c->first, c->stop_sim, plan, st));
    int32_t selected = 0;
    if (c->idx) HIP_TRY(hipMemcpyAsync(c->idx, b.idx, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    if (c->cover) HIP_TRY(hipMemcpyAsync(c->cover, b.cover, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    if (c->selected) HIP_TRY(hipMemcpyAsync(&selected, b.head + 1, 4, hipMemcpyDeviceToHost, st));
    if (c->nearest) HIP_TRY(hipMemcpyAsync(c->nearest, b.nearest, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (c->near_sim) HIP_TRY(hipMemcpyAsync(c->near_sim, b.sim, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->selected) *c->selected = selected;
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_bank_keep(dinov2_hip_session* s, dinov2_hip_bank* b, const int32_t* idx, int32_t m, char* err, size_t errlen) {
    if (!s || !b || !idx) {
        set_err(err, errlen, "bank_keep: null session / bank / idx");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (s->model->device != b->device) {
        set_err(err, errlen, "bank_keep: the session is on device %d, the bank on device %d", s->model->device, b->device);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (m < 1 || m > b->count) {
        set_err(err, errlen, "bank_keep: need 1 <= m <= count = %d", b->count);
        return DINOV2_HIP_ERR_INVALID;
    }
    for (int j = 0; j < m; ++j)
        if (idx[j] < 0 || idx[j] >= b->count || (j > 0 && idx[j] <= idx[j - 1])) {
            set_err(err, errlen, "bank_keep: idx must ascend strictly inside [0, %d) (entry %d is %d)", b->count, j, (int)idx[j]);
            return DINOV2_HIP_ERR_INVALID;
        }
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;
    const size_t row_bytes = (size_t)b->hpad * 2;
    const int chunk = (int)(BANK_KEEP_STAGE / row_bytes);  // >= 4096 rows
    const size_t stage_bytes = align_up((size_t)(m < chunk ? m : chunk) * row_bytes, 256);
    const int rs = reserve(s, s->scratch[SCRATCH_BANK], stage_bytes + align_up((size_t)m * 4, 256), "bank_keep", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    _Float16* const stage = s->scratch[SCRATCH_BANK].as<_Float16>();
    int* const didx = (int*)(s->scratch[SCRATCH_BANK].as<char>() + stage_bytes);
    // In place, destination rows [j0, j1) chunk by chunk in ascending order, each gathered whole into the stage before it is written.  idx
    // ascends strictly from >= 0, so idx[j] >= j: the sources of every later chunk lie at rows >= j1, which no earlier chunk's write
    // (rows < j1) has touched; within a chunk the gather ends before the copy begins (stream order).
    hipError_t e = hipMemcpyAsync(didx, idx, (size_t)m * 4, hipMemcpyHostToDevice, st);
    for (int j0 = 0; j0 < m && e == hipSuccess; j0 += chunk) {
        const int cnt = m - j0 < chunk ? m - j0 : chunk;
        e = launch_bank_gather(b->rows, didx + j0, cnt, b->hpad, stage, st);
        if (e == hipSuccess) e = hipMemcpyAsync(b->rows + (size_t)j0 * b->hpad, stage, (size_t)cnt * row_bytes, hipMemcpyDeviceToDevice, st);
    }
    const hipError_t es = hipStreamSynchronize(st);  // (on an error too: idx is the caller's, and a returned bank is always complete)
    HIP_TRY(e);
    HIP_TRY(es);
    b->count = m;
    return DINOV2_HIP_OK;
}
