// slide.cpp -- dinov2_hip_predict_dense_slide and dinov2_hip_slide_windows (contract in include/dinov2_hip.h): sliding-window inference layered on
// dinov2_hip_predict_dense.  The entry point checks its request, carves the session's slide scratch, copies the windows into one batch
// (slide_gather_kernel), hands that batch to dinov2_hip_predict_dense as a device input with only the low-resolution logits requested as a
// device output -- which splits over-long batches into passes and writes each pass's logits at its image offset -- and reduces them
// (slide_reduce_kernel, csrc/slide.hip).
#include <vector>

#include "host.h"

using namespace dinov2;

namespace {

struct Windows {
    int h0 = 0, w0 = 0;  // the crop's patch grid
    std::vector<int> y1, x1;
};

// the refusals of dinov2_hip_slide_windows; on success the starts of both axes (contract 1)
int slide_windows(const dinov2_hip_model* m, int h, int w, const dinov2_hip_slide* sl, Windows& win, char* err, size_t errlen) {
    if (!m || !sl) {
        set_err(err, errlen, "slide: null model / slide");
        return DINOV2_HIP_ERR_INVALID;
    }
    int32_t h0, w0;
    const int rc = dinov2_hip_model_grid(m, sl->crop_h, sl->crop_w, &h0, &w0, err, errlen);  // (names the crop it refuses)
    if (rc != DINOV2_HIP_OK) return rc;
    if (sl->stride_h < 1 || sl->stride_h > sl->crop_h || sl->stride_w < 1 || sl->stride_w > sl->crop_w) {
        set_err(err, errlen, "slide: stride %d x %d outside 1 .. crop (%d x %d)", (int)sl->stride_h, (int)sl->stride_w, (int)sl->crop_h,
                (int)sl->crop_w);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (h < sl->crop_h || w < sl->crop_w || h > DENSE_OUT_MAX || w > DENSE_OUT_MAX) {
        set_err(err, errlen, "slide: image %d x %d smaller than the crop %d x %d (use dinov2_hip_predict_dense) or larger than %d", h, w,
                (int)sl->crop_h, (int)sl->crop_w, DENSE_OUT_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    win.h0 = h0;
    win.w0 = w0;
    win.y1.resize((size_t)slide_count(h, sl->crop_h, sl->stride_h));
    win.x1.resize((size_t)slide_count(w, sl->crop_w, sl->stride_w));
    for (size_t i = 0; i < win.y1.size(); ++i) win.y1[i] = slide_start((int)i, h, sl->crop_h, sl->stride_h);
    for (size_t i = 0; i < win.x1.size(); ++i) win.x1[i] = slide_start((int)i, w, sl->crop_w, sl->stride_w);
    return DINOV2_HIP_OK;
}

}  // namespace

extern "C" int dinov2_hip_slide_windows(const dinov2_hip_model* m, int32_t h, int32_t w, const dinov2_hip_slide* sl, int32_t* ny, int32_t* nx,
                                        int32_t* y1, int32_t* x1, char* err, size_t errlen) {
    if (!ny || !nx) {
        set_err(err, errlen, "slide_windows: null ny / nx");
        return DINOV2_HIP_ERR_INVALID;
    }
    Windows win;
    const int rc = slide_windows(m, h, w, sl, win, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    *ny = (int32_t)win.y1.size();
    *nx = (int32_t)win.x1.size();
    if (y1) std::copy(win.y1.begin(), win.y1.end(), y1);
    if (x1) std::copy(win.x1.begin(), win.x1.end(), x1);
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_predict_dense_slide(dinov2_hip_session* s, const dinov2_hip_input* in, const dinov2_hip_dense_head* hd,
                                              const dinov2_hip_slide* sl, const dinov2_hip_dense_out* o, char* err, size_t errlen) {
    if (!s || !in || !in->data || !hd || !sl || !o) {
        set_err(err, errlen, "predict_dense_slide: null session / input / head / slide / outputs");
        return DINOV2_HIP_ERR_INVALID;
    }
    const dinov2_hip_model* m = s->model;
    if (in->layout == DINOV2_HIP_U8_BGR_HWC) {
        set_err(err, errlen, "predict_dense_slide takes f32 images (BGR_HWC or RGB_CHW): raw 8-bit input is resized to a network size, which sliding avoids");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (in->layout != DINOV2_HIP_BGR_HWC && in->layout != DINOV2_HIP_RGB_CHW) {
        set_err(err, errlen, "predict_dense_slide: unknown input layout %d", (int)in->layout);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (in->batch < 1) {
        set_err(err, errlen, "predict_dense_slide: batch %d below 1", (int)in->batch);
        return DINOV2_HIP_ERR_INVALID;
    }
    const int h = in->height, w = in->width, ch = sl->crop_h, cw = sl->crop_w;
    Windows win;
    int rc = slide_windows(m, h, w, sl, win, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (o->out_h != 0 || o->out_w != 0) {
        set_err(err, errlen, "predict_dense_slide: out_h, out_w %d, %d: must be 0, 0 (the image size)", (int)o->out_h, (int)o->out_w);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (hd->device != m->device) {
        set_err(err, errlen, "predict_dense_slide: the session is on device %d, the head on device %d", m->device, hd->device);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (hd->H != (int)m->hp.hidden_size || hd->L != (int)m->hp.num_hidden_layers) {
        set_err(err, errlen, "predict_dense_slide: the head was created for hidden size %d and %d layers, the session's model has %d and %d", hd->H,
                hd->L, (int)m->hp.hidden_size, (int)m->hp.num_hidden_layers);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!o->labels && !o->value && !o->logits) {
        set_err(err, errlen, "predict_dense_slide: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (o->labels && hd->reduce == DINOV2_HIP_DENSE_BINS) {
        set_err(err, errlen, "predict_dense_slide: labels requested from a DINOV2_HIP_DENSE_BINS head");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (o->on_device && ((reinterpret_cast<uintptr_t>(o->labels) | reinterpret_cast<uintptr_t>(o->value) | reinterpret_cast<uintptr_t>(o->logits)) & 15)) {
        set_err(err, errlen, "device pointers of dinov2_hip_dense_out must be 16-byte aligned");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int ny = (int)win.y1.size(), nx = (int)win.x1.size();
    const size_t B = (size_t)in->batch, nwin = (size_t)ny * nx, NW = B * nwin;
    if (NW > (size_t)SLIDE_WINDOWS_MAX) {
        set_err(err, errlen, "predict_dense_slide: %d images of %d x %d windows make %zu windows, above %d", (int)in->batch, ny, nx, NW,
                SLIDE_WINDOWS_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    const int cover = slide_axis_cover(win.y1.data(), ny, ch) * slide_axis_cover(win.x1.data(), nx, cw);
    if (cover > SLIDE_COVER_MAX) {
        set_err(err, errlen, "predict_dense_slide: stride %d x %d of crop %d x %d puts %d windows over one pixel, above DINOV2_HIP_SLIDE_COVER_MAX %d",
                (int)sl->stride_h, (int)sl->stride_w, ch, cw, cover, SLIDE_COVER_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    const SlideReducePlan plan = slide_reduce_plan(win.h0, win.w0, hd->C, ch, cw, h, w, win.y1.data(), ny, win.x1.data(), nx);
    if (plan.tile_y == 0) {  // (every accepted request has a plan: kernels.h)
        set_err(err, errlen, "predict_dense_slide: no launch plan for %d classes on a %d x %d grid", hd->C, win.h0, win.w0);
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(m->device));

    // the scratch: the window table first (its place never moves), then the images of a host input, the window batch, all logits, the staging
    std::vector<int> tab(slide_table_ints(plan, ny, nx));
    slide_table_fill(plan, win.h0, win.w0, ch, cw, h, w, win.y1.data(), ny, win.x1.data(), nx, tab.data());
    const size_t P = (size_t)win.h0 * win.w0, C = (size_t)hd->C, npx = (size_t)h * w, per_win = (size_t)3 * ch * cw;
    const bool reduce = o->labels || o->value, host_out = !o->on_device;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += align_up(bytes, 256); return off; };
    const size_t o_tab = take(sizeof(int) * ((size_t)2 * DENSE_OUT_MAX + 4 * (size_t)DENSE_OUT_MAX));  // (the largest table there is)
    const size_t o_img = take(in->on_device ? 0 : B * 3 * npx * 4), o_win = take(NW * per_win * 4), o_lg = take(NW * P * C * 4);
    const size_t o_lab = take(host_out && o->labels ? B * npx : 0), o_val = take(host_out && o->value ? B * npx * 4 : 0);
    const size_t before = s->scratch[SCRATCH_SLIDE].bytes;  // (reserve keeps nothing when it grows the buffer)
    rc = reserve(s, s->scratch[SCRATCH_SLIDE], need, "predict_dense_slide", err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    char* const buf = s->scratch[SCRATCH_SLIDE].as<char>();
    hipStream_t st = s->stream;
    int* const d_tab = (int*)(buf + o_tab);
    if (s->scratch[SCRATCH_SLIDE].bytes != before || s->slide_tab_host != tab) {
        // the table changes: a kernel in flight may still read the old one on the device, a copy in flight the old one on the host
        HIP_TRY(hipStreamSynchronize(st));
        s->slide_tab_host = tab;
        HIP_TRY(hipMemcpyAsync(d_tab, s->slide_tab_host.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, st));
    }
    const float* img = in->data;
    if (!in->on_device) {  // uploaded once, whatever the overlap of the windows
        HIP_TRY(hipMemcpyAsync(buf + o_img, in->data, B * 3 * npx * 4, hipMemcpyHostToDevice, st));
        img = (const float*)(buf + o_img);
    }
    float* const d_win = (float*)(buf + o_win);
    float* const d_lg = (float*)(buf + o_lg);
    {
        ProfileMark pm(s, "im2col");
        HIP_TRY(launch_slide_gather(img, d_win, d_tab, (int)B, h, w, ny, nx, ch, cw, in->layout == DINOV2_HIP_RGB_CHW ? 1 : 0, st));
    }
    dinov2_hip_input wi{};
    wi.data = d_win; wi.batch = (int32_t)NW; wi.height = ch; wi.width = cw; wi.layout = in->layout; wi.on_device = 1;
    dinov2_hip_dense_out lo{};
    lo.logits = d_lg; lo.on_device = 1;
    rc = dinov2_hip_predict_dense(s, &wi, nullptr, hd, &lo, 0, err, errlen);
    s->last_patches = 0;
    s->last_b = 0;  // the session holds windows, not the caller's images: no last un-split forward, as after dinov2_hip_predict_list
    if (rc != DINOV2_HIP_OK) return rc;
    const hipMemcpyKind kind = host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (o->logits) HIP_TRY(hipMemcpyAsync(o->logits, d_lg, NW * P * C * 4, kind, st));
    if (reduce) {
        uint8_t* const lab = o->labels ? (host_out ? (uint8_t*)(buf + o_lab) : o->labels) : nullptr;
        float* const val = o->value ? (host_out ? (float*)(buf + o_val) : o->value) : nullptr;
        {
            ProfileMark pm(s, "head");
            HIP_TRY(launch_slide_reduce(d_lg, (int)C, (int)B, win.h0, win.w0, hd->C, ch, cw, h, w, ny, nx, d_tab, hd->reduce, hd->centers, hd->eps, lab,
                                        val, plan, st));
        }
        if (host_out) {
            if (lab) HIP_TRY(hipMemcpyAsync(o->labels, lab, B * npx, hipMemcpyDeviceToHost, st));
            if (val) HIP_TRY(hipMemcpyAsync(o->value, val, B * npx * 4, hipMemcpyDeviceToHost, st));
        }
    }
    if (host_out) HIP_TRY(hipStreamSynchronize(st));  // host outputs are complete on return
    return DINOV2_HIP_OK;
}
