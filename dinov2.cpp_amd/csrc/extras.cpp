// extras.cpp -- the entry points whose forward carries side outputs (PassExtras, model.h): dinov2_hip_predict_layers, dinov2_hip_predict_attention
// and dinov2_hip_predict_dense.  Each checks its request, sizes the session scratch its outputs are staged in, fills the run descriptors and
// hands them to predict_impl (model.cpp), which runs the passes.
#include <algorithm>

#include "host.h"

using namespace dinov2;

namespace {

// the argument checks of a dinov2_hip_layers, before anything runs
int check_layers(const dinov2_hip_model* m, const dinov2_hip_layers* ly, char* err, size_t errlen) {
    const int L = (int)m->hp.num_hidden_layers, R = (int)m->hp.num_register_tokens;
    if (!ly || !ly->layers) {
        set_err(err, errlen, "null layers / layer list");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (ly->n_layers < 1 || ly->n_layers > L + 1) {
        set_err(err, errlen, "n_layers %d outside 1 .. %d", (int)ly->n_layers, L + 1);
        return DINOV2_HIP_ERR_INVALID;
    }
    int bad;
    if (const LayerListFault f = check_layer_list(ly->layers, ly->n_layers, 0, L, &bad)) {
        if (f == LAYER_OUT_OF_RANGE)
            set_err(err, errlen, "layer %d outside 0 .. %d (number of blocks applied; 0 = embeddings)", bad, L);
        else
            set_err(err, errlen, "the layer list must be strictly ascending");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (ly->layout != DINOV2_HIP_LAYERS_TOKENS && ly->layout != DINOV2_HIP_LAYERS_CHW) {
        set_err(err, errlen, "unknown layers layout %d", (int)ly->layout);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (ly->registers && R == 0) {
        set_err(err, errlen, "register tokens requested from a model without registers");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (ly->on_device) {  // the kernel stores 16 bytes at a time through these pointers
        const float* const ptrs[3] = {ly->patch_tokens, ly->cls, ly->registers};
        for (const float* p : ptrs)
            if (reinterpret_cast<uintptr_t>(p) & 15) {
                set_err(err, errlen, "device pointers of dinov2_hip_layers must be 16-byte aligned");
                return DINOV2_HIP_ERR_INVALID;
            }
    }
    return DINOV2_HIP_OK;
}

}  // namespace

// =============================================================================================================
// predict + intermediate layers (no reference counterpart; upstream DINOv2: get_intermediate_layers, HuggingFace: output_hidden_states)
// =============================================================================================================
// One forward with layer taps (`ly`) and / or attention rows (`at`), either of which may be nullptr; every argument has been checked.
static int predict_tapped(dinov2_hip_session* s, const dinov2_hip_input* in, dinov2_hip_output* out, const dinov2_hip_layers* ly,
                          const dinov2_hip_attention* at, uint32_t flags, char* err, size_t errlen) {
    const dinov2_hip_model* m = s->model;
    const int R = (int)m->hp.num_register_tokens;
    int h, w;
    network_size(m, in, flags, &h, &w);
    const Dims d1 = dims_of(m, 1, h, w);
    const size_t B = (size_t)in->batch, H = m->hp.hidden_size, P = (size_t)d1.P, nh = m->hp.num_attention_heads;
    HIP_TRY(hipSetDevice(m->device));
    PassExtras ex;
    TapRun& t = ex.taps;
    size_t np = 0, nc = 0, nr = 0;
    if (ly) {
        const size_t n = (size_t)ly->n_layers;
        t.layers = ly->layers;
        t.n = ly->n_layers;
        t.norm = ly->norm != 0;
        t.chw = ly->layout == DINOV2_HIP_LAYERS_CHW;
        t.patch_stride = B * P * H;
        t.cls_stride = B * H;
        t.reg_stride = B * (size_t)R * H;
        if (ly->on_device) {  // the kernel writes straight into the caller's buffers
            t.patch = ly->patch_tokens;
            t.cls = ly->cls;
            t.reg = ly->registers;
        } else {  // host outputs: the kernel writes into the session's tap scratch, which leaves by asynchronous copies
            np = ly->patch_tokens ? n * t.patch_stride : 0;
            nc = ly->cls ? n * t.cls_stride : 0;
            nr = ly->registers ? n * t.reg_stride : 0;
            const int rc = reserve(s, s->scratch[SCRATCH_TAP], sizeof(float) * (np + nc + nr), "predict_layers", err, errlen);
            if (rc != DINOV2_HIP_OK) return rc;
            float* const buf = s->scratch[SCRATCH_TAP].as<float>();
            if (np) t.patch = buf;  // (every block is a multiple of H floats, H % 4 == 0: all three stay 16-byte aligned)
            if (nc) t.cls = buf + np;
            if (nr) t.reg = buf + np + nc;
        }
    }
    AttnRun& a = ex.attn;
    size_t na = 0;
    if (at) {
        static const int32_t cls_only[1] = {0};
        const int32_t* q = at->n_queries ? at->queries : cls_only;
        const size_t nq = at->n_queries ? (size_t)at->n_queries : 1;
        a.layers = at->layers;
        a.n = at->n_layers;
        a.nq = (int)nq;
        a.key0 = at->keys == DINOV2_HIP_ATTN_KEYS_PATCHES ? 1 + R : 0;
        a.nkeys = d1.T - a.key0;
        a.stride = B * nh * nq * (size_t)a.nkeys;
        // the query list on the device: kept from call to call, replaced (after a wait: a forward in flight may be reading it) when it changes
        if (s->attn_q_host.size() != nq || !std::equal(q, q + nq, s->attn_q_host.begin())) {
            HIP_TRY(hipStreamSynchronize(s->stream));
            s->attn_q_host.clear();
            const int rc = reserve(s, s->scratch[SCRATCH_ATTN_Q], sizeof(int32_t) * nq, "predict_attention", err, errlen);
            if (rc != DINOV2_HIP_OK) return rc;
            HIP_TRY(hipMemcpy(s->scratch[SCRATCH_ATTN_Q].ptr, q, sizeof(int32_t) * nq, hipMemcpyHostToDevice));
            s->attn_q_host.assign(q, q + nq);
        }
        a.queries = s->scratch[SCRATCH_ATTN_Q].as<int32_t>();
        if (at->on_device) {
            a.probs = at->probs;
        } else {
            na = (size_t)at->n_layers * a.stride;
            const int rc = reserve(s, s->scratch[SCRATCH_ATTN], sizeof(float) * na, "predict_attention", err, errlen);
            if (rc != DINOV2_HIP_OK) return rc;
            a.probs = s->scratch[SCRATCH_ATTN].as<float>();
        }
    }
    if (np + nc + nr + na == 0) return predict_impl(s, in, out, flags, ex, err, errlen);  // nothing staged: asynchronous, as predict
    // One synchronise for the whole call: the forward alone first, then the staged copies, then `out`'s copies (fetch_outputs, which waits
    // when `out` is host memory).  A batch that is split into passes hands `out` to the passes instead, which wait once each.
    const bool split = B > dinov2_max_pass_batch(m, h, w);
    int rc = predict_impl(s, in, split ? out : nullptr, flags, ex, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (np) HIP_TRY(hipMemcpyAsync(ly->patch_tokens, t.patch, sizeof(float) * np, hipMemcpyDeviceToHost, s->stream));
    if (nc) HIP_TRY(hipMemcpyAsync(ly->cls, t.cls, sizeof(float) * nc, hipMemcpyDeviceToHost, s->stream));
    if (nr) HIP_TRY(hipMemcpyAsync(ly->registers, t.reg, sizeof(float) * nr, hipMemcpyDeviceToHost, s->stream));
    if (na) HIP_TRY(hipMemcpyAsync(at->probs, a.probs, sizeof(float) * na, hipMemcpyDeviceToHost, s->stream));
    if (out && !split) {
        rc = fetch_outputs(s, out, err, errlen);
        if (rc != DINOV2_HIP_OK || !out->on_device) return rc;  // (host `out`: fetch_outputs has waited for the stream)
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_predict_layers(dinov2_hip_session* s, const dinov2_hip_input* in, dinov2_hip_output* out,
                                         const dinov2_hip_layers* ly, uint32_t flags, char* err, size_t errlen) {
    int rc = check_input(s, in, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    rc = check_layers(s->model, ly, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    rc = check_predict_args(s->model, out, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    return predict_tapped(s, in, out, ly, nullptr, flags, err, errlen);
}

// =============================================================================================================
// predict + attention rows (no reference counterpart; upstream DINOv2: get_last_selfattention, HuggingFace: output_attentions)
// =============================================================================================================
extern "C" int dinov2_hip_predict_attention(dinov2_hip_session* s, const dinov2_hip_input* in, dinov2_hip_output* out,
                                            const dinov2_hip_layers* taps, const dinov2_hip_attention* at, uint32_t flags, char* err,
                                            size_t errlen) {
    int rc = check_input(s, in, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const dinov2_hip_model* m = s->model;
    const int L = (int)m->hp.num_hidden_layers;
    if (!at || !at->layers || !at->probs) {
        set_err(err, errlen, "null attention request / layer list / probs");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (at->n_layers < 1 || at->n_layers > L) {
        set_err(err, errlen, "attention n_layers %d outside 1 .. %d", (int)at->n_layers, L);
        return DINOV2_HIP_ERR_INVALID;
    }
    int bad;
    if (const LayerListFault f = check_layer_list(at->layers, at->n_layers, 1, L, &bad)) {
        if (f == LAYER_OUT_OF_RANGE)
            set_err(err, errlen, "attention layer %d outside 1 .. %d (k = the attention inside block k; there is none before block 1)", bad, L);
        else
            set_err(err, errlen, "the attention layer list must be strictly ascending");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (at->keys != DINOV2_HIP_ATTN_KEYS_ALL && at->keys != DINOV2_HIP_ATTN_KEYS_PATCHES) {
        set_err(err, errlen, "unknown attention keys value %d", (int)at->keys);
        return DINOV2_HIP_ERR_INVALID;
    }
    int h, w;
    network_size(m, in, flags, &h, &w);
    const int T = dims_of(m, 1, h, w).T;
    if (at->n_queries < 0 || at->n_queries > T || (at->n_queries > 0 && !at->queries)) {
        set_err(err, errlen, "n_queries %d outside 0 .. %d, or a null query list", (int)at->n_queries, T);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (const LayerListFault f = check_layer_list(at->queries, at->n_queries, 0, T - 1, &bad)) {  // (the same rule as for a layer list)
        if (f == LAYER_OUT_OF_RANGE)
            set_err(err, errlen, "query token %d outside 0 .. %d for this input", bad, T - 1);
        else
            set_err(err, errlen, "the query list must be strictly ascending");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (at->on_device && (reinterpret_cast<uintptr_t>(at->probs) & 15)) {
        set_err(err, errlen, "the device pointer of dinov2_hip_attention must be 16-byte aligned");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (taps) {
        rc = check_layers(m, taps, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
    }
    rc = check_predict_args(m, out, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    return predict_tapped(s, in, out, taps, at, flags, err, errlen);
}

// =============================================================================================================
// predict + a linear dense-prediction head (the head itself: resident.cpp)
// =============================================================================================================
extern "C" int dinov2_hip_predict_dense(dinov2_hip_session* s, const dinov2_hip_input* in, dinov2_hip_output* out,
                                        const dinov2_hip_dense_head* hd, const dinov2_hip_dense_out* o, uint32_t flags, char* err,
                                        size_t errlen) {
    int rc = check_input(s, in, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const dinov2_hip_model* m = s->model;
    if (!hd || !o) {
        set_err(err, errlen, "predict_dense: null head / outputs");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (hd->device != m->device) {
        set_err(err, errlen, "predict_dense: the session is on device %d, the head on device %d", m->device, hd->device);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (hd->H != (int)m->hp.hidden_size || hd->L != (int)m->hp.num_hidden_layers) {
        set_err(err, errlen, "predict_dense: the head was created for hidden size %d and %d layers, the session's model has %d and %d", hd->H, hd->L,
                (int)m->hp.hidden_size, (int)m->hp.num_hidden_layers);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!o->labels && !o->value && !o->logits) {
        set_err(err, errlen, "predict_dense: no output requested");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (o->labels && hd->reduce == DINOV2_HIP_DENSE_BINS) {
        set_err(err, errlen, "predict_dense: labels requested from a DINOV2_HIP_DENSE_BINS head");
        return DINOV2_HIP_ERR_INVALID;
    }
    int h, w;
    network_size(m, in, flags, &h, &w);
    const bool own_size = o->out_h == 0 && o->out_w == 0;
    const int oh = own_size ? h : o->out_h, ow = own_size ? w : o->out_w;
    if (oh < 1 || ow < 1 || oh > DENSE_OUT_MAX || ow > DENSE_OUT_MAX) {
        set_err(err, errlen, "predict_dense: output size %d x %d outside 1 .. %d (0, 0 = the network input size)", oh, ow, DENSE_OUT_MAX);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (o->on_device && ((reinterpret_cast<uintptr_t>(o->labels) | reinterpret_cast<uintptr_t>(o->value) | reinterpret_cast<uintptr_t>(o->logits)) & 15)) {
        set_err(err, errlen, "device pointers of dinov2_hip_dense_out must be 16-byte aligned");
        return DINOV2_HIP_ERR_INVALID;
    }
    rc = check_predict_args(m, out, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    HIP_TRY(hipSetDevice(m->device));
    // the scratch of ONE pass: operand, logits (rows to whole 256-row tiles), and what host outputs are staged in
    const Dims d1 = dims_of(m, 1, h, w);
    const size_t B = (size_t)in->batch, Bp = std::min(B, dinov2_max_pass_batch(m, h, w));
    const size_t rows = align_up(Bp * (size_t)d1.P, 256), npx = (size_t)oh * ow;
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t off = need; need += align_up(bytes, 256); return off; };
    const size_t o_a16 = take(rows * (size_t)hd->K * 2), o_lg = take(rows * (size_t)hd->cpad * 4);
    const size_t o_lab = take(!o->on_device && o->labels ? Bp * npx : 0), o_val = take(!o->on_device && o->value ? Bp * npx * 4 : 0);
    rc = reserve(s, s->scratch[SCRATCH_DENSE], need, "predict_dense", err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    char* const buf = s->scratch[SCRATCH_DENSE].as<char>();
    PassExtras ex;
    ex.dense = DenseRun{hd, hd->layers, hd->n_layers, o, 0, oh, ow, (_Float16*)(buf + o_a16), (float*)(buf + o_lg), (uint8_t*)(buf + o_lab),
                        (float*)(buf + o_val)};
    rc = predict_impl(s, in, out, flags, ex, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (!o->on_device) HIP_TRY(hipStreamSynchronize(s->stream));  // host outputs are complete on return
    return DINOV2_HIP_OK;
}
