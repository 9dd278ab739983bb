// vlad.cpp -- dinov2_hip_vlad_tokens (include/dinov2_hip.h): VLAD descriptors of row segments on the device (csrc/vlad.hip; no reference
// counterpart).  Beside resident.cpp, whose check of a rows source it shares (host.h check_session_rows).
#include <vector>

#include "host.h"

using namespace dinov2;

namespace {
// The tables of a call are locals whose copies to the device are queued on the session's stream: a return before the call's one wait drains
// the stream first.
struct DrainOnError {
    hipStream_t st;
    bool armed = true;
    ~DrainOnError() {
        if (armed) (void)hipStreamSynchronize(st);
    }
};
}  // namespace

extern "C" int dinov2_hip_vlad_tokens(dinov2_hip_session* s, const dinov2_hip_vlad* v, char* err, size_t errlen) {
    if (!s || !v) {
        set_err(err, errlen, "vlad: null session / request");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int H = v->rows.H, K = v->K;
    if (H < 8 || H > 4096 || K < 1 || K > KMEANS_K_MAX) {
        set_err(err, errlen, "vlad: need 8 <= H <= 4096 and 1 <= K <= %d", KMEANS_K_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!v->centers) {
        set_err(err, errlen, "vlad: centers == NULL");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (v->flags & ~(uint32_t)(DINOV2_HIP_VLAD_INTRA_NORM | DINOV2_HIP_VLAD_L2_NORM)) {
        set_err(err, errlen, "vlad: unknown flag bits 0x%x", (unsigned)v->flags);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!v->vlad && !v->counts && !v->labels && !v->sim) {
        set_err(err, errlen, "vlad: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (v->rows.source == DINOV2_HIP_ROWS_LAST_CLS) {
        set_err(err, errlen, "vlad: DINOV2_HIP_ROWS_LAST_CLS is no source of segments: use GIVEN or LAST_PATCHES");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (v->all_images != 0 && (v->all_images != 1 || v->rows.source != DINOV2_HIP_ROWS_LAST_PATCHES)) {
        set_err(err, errlen, "vlad: all_images is 0, or 1 with DINOV2_HIP_ROWS_LAST_PATCHES");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int n = v->rows.n, n_seg = v->n_seg;
    if (n < 1 || n > VLAD_N_MAX || n_seg < 1 || n_seg > VLAD_SEG_MAX || n_seg > n) {
        set_err(err, errlen, "vlad: need 1 <= rows <= %d and 1 <= n_seg <= %d, no more segments than rows", VLAD_N_MAX, VLAD_SEG_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if ((uint64_t)n_seg * (uint64_t)K * (uint64_t)H > VLAD_OUT_MAX) {
        set_err(err, errlen, "vlad: n_seg * K * H = %llu is above 2^28", (unsigned long long)n_seg * K * H);
        return DINOV2_HIP_ERR_INVALID;
    }
    const bool given = v->rows.source == DINOV2_HIP_ROWS_GIVEN;
    if (!given && v->offsets) {
        set_err(err, errlen, "vlad: offsets go with DINOV2_HIP_ROWS_GIVEN only; a resident source has one segment per image");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (given && !v->offsets && n_seg != 1) {
        set_err(err, errlen, "vlad: offsets == NULL means one segment, not %d", n_seg);
        return DINOV2_HIP_ERR_INVALID;
    }
    for (int i = 0; v->offsets && i <= n_seg; ++i) {
        const bool ok = i == 0 ? v->offsets[0] == 0 : v->offsets[i] > v->offsets[i - 1] && v->offsets[i] <= n;
        if (!ok || (i == n_seg && v->offsets[i] != n)) {
            set_err(err, errlen, "vlad: offsets must ascend strictly from 0 to rows.n = %d (entry %d is %d)", n, i, (int)v->offsets[i]);
            return DINOV2_HIP_ERR_INVALID;
        }
    }
    // the view of the source: segment i starts at src + i * outer floats (resident) or at row offsets[i] of src (GIVEN); rows ld floats apart
    const float* src;
    size_t ld, outer = 0;
    std::vector<int32_t> off(n_seg + 1, 0);
    if (given) {
        const int rc = check_session_rows("vlad", s, H, &v->rows, &src, &ld, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
        for (int i = 0; i <= n_seg; ++i) off[i] = v->offsets ? v->offsets[i] : i * n;
    } else {
        dinov2_hip_rows one = v->rows;  // one image's patch rows stand for the checks of the resident source
        const int P = s->last_b > 0 ? s->last_t - 1 - (int)s->model->hp.num_register_tokens : 0;
        if (v->all_images) {
            one.image = 0;
            one.n = P > 0 ? P : 1;  // (no forward: the resident check below says so)
        }
        const int rc = check_session_rows("vlad", s, H, &one, &src, &ld, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
        const int want_seg = v->all_images ? s->last_b : 1;
        if (n_seg != want_seg || (int64_t)n != (int64_t)want_seg * P) {
            set_err(err, errlen, "vlad: this source has %d segment(s) of %d patch rows: n_seg must be %d and rows.n %d", want_seg, P, want_seg,
                    want_seg * P);
            return DINOV2_HIP_ERR_INVALID;
        }
        outer = (size_t)s->last_t * H;
        for (int i = 0; i <= n_seg; ++i) off[i] = i * P;
    }
    HIP_TRY(hipSetDevice(s->model->device));
    hipStream_t st = s->stream;
    std::vector<VladSeg> segs;
    std::vector<VladChunk> chunks;
    std::vector<VladTile> tiles;
    const VladPlan plan = vlad_plan(off.data(), n_seg, K, H, &segs, &chunks, &tiles);
    const bool stage = given && !v->rows.on_device;
    const size_t n_x = (size_t)n * H * 4;
    const int rs = reserve(s, s->scratch[SCRATCH_VLAD], plan.bytes + align_up(stage ? n_x : 0, 256), "vlad", err, errlen);
    if (rs != DINOV2_HIP_OK) return rs;
    char* const buf = s->scratch[SCRATCH_VLAD].as<char>();
    const VladBufs b = vlad_bufs(buf, plan);
    DrainOnError drain{st};
    HIP_TRY(hipMemcpyAsync(b.segs, segs.data(), segs.size() * sizeof(VladSeg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.chunks, chunks.data(), chunks.size() * sizeof(VladChunk), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.tiles, tiles.data(), tiles.size() * sizeof(VladTile), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.cvec, v->centers, (size_t)K * H * 4, hipMemcpyHostToDevice, st));
    if (given) {
        src = v->rows.data;
        if (stage) {
            HIP_TRY(hipMemcpyAsync(buf + plan.bytes, v->rows.data, n_x, hipMemcpyHostToDevice, st));
            src = (const float*)(buf + plan.bytes);
        }
    }
    // every segment into its own block of whole tiles, one launch: row g of the caller's order lives at src + (g / per) * outer + (g % per) * ld
    HIP_TRY(launch_vlad_normalise(src, given ? n : n / n_seg, outer, ld, b.tiles, plan.ntiles, b.x16, H, plan.hpad, st));
    HIP_TRY(vlad_run(b, n_seg, K, H, v->flags, plan, chunks.data(), st));
    if (v->vlad) HIP_TRY(hipMemcpyAsync(v->vlad, b.vlad, (size_t)n_seg * K * H * 4, hipMemcpyDeviceToHost, st));
    if (v->counts) HIP_TRY(hipMemcpyAsync(v->counts, b.counts, (size_t)n_seg * K * 4, hipMemcpyDeviceToHost, st));
    if (v->labels) HIP_TRY(hipMemcpyAsync(v->labels, b.labels_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (v->sim) HIP_TRY(hipMemcpyAsync(v->sim, b.sim_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    drain.armed = false;
    HIP_TRY(hipStreamSynchronize(st));
    return DINOV2_HIP_OK;
}
