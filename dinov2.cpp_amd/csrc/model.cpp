// model.cpp -- session, forward orchestration and the predict family of the C-ABI of libdinov2_hip.so (the loader is load.cpp).
//
// Replaces, from the reference (lavaman131/dinov2.cpp):
//   build_graph + dino_predict  /root/reference/dinov2.cpp:823-838, :900-999  -> forward() + dinov2_hip_predict
// There is no graph builder / allocator / backend scheduler here: the forward is a fixed sequence of ~8 fused
// kernel launches per layer on one HIP stream over a pre-carved workspace.
// dinov2_hip_predict_list (no reference counterpart) is here too: forward() takes a pass of runs (model.h), a uniform batch is one run and a
// list of images of different sizes one run per stretch of equal sizes; copy_out() hands out the results of either.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>

#include "host.h"

using namespace dinov2;

// =============================================================================================================
// argument checks shared by the predict family (and, the first, by group.cpp)
// =============================================================================================================
int dinov2_check_input(const dinov2_hip_model* m, const dinov2_hip_input* in, char* err, size_t errlen) {
    if (!m || !in || !in->data) {
        set_err(err, errlen, "null session / input");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int ps = (int)m->hp.patch_size, st = m->patch_stride;  // (st == ps: the sizes are the positive multiples of the patch size)
    if (in->layout == DINOV2_HIP_U8_BGR_HWC) {  // raw images: any size, preprocessed on the device
        if (in->batch <= 0 || in->height <= 0 || in->width <= 0) {
            set_err(err, errlen, "raw image input must have batch, height, width >= 1");
            return DINOV2_HIP_ERR_INVALID;
        }
        return DINOV2_HIP_OK;
    }
    if (in->layout != DINOV2_HIP_BGR_HWC && in->layout != DINOV2_HIP_RGB_CHW) {  // (raw u8 returned above)
        set_err(err, errlen, "unknown input layout %d", in->layout);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (in->batch <= 0 || in->height < ps || in->width < ps || (in->height - ps) % st || (in->width - ps) % st) {
        set_err(err, errlen, "input must be batch >= 1 and height/width = patch_size %d plus a multiple of patch_stride %d (got %d x %d x %d)",
                ps, st, in->batch, in->height, in->width);
        return DINOV2_HIP_ERR_INVALID;
    }
    return DINOV2_HIP_OK;
}

int dinov2::check_input(const dinov2_hip_session* s, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen) {
    return dinov2_check_input_rows(s ? s->model : nullptr, in, flags, err, errlen);
}

// dinov2_hip_predict's own argument checks; the calls that allocate or copy before they reach predict_impl make them first, too: nothing may run
// for a call that is refused
int dinov2::check_predict_args(const dinov2_hip_model* m, const dinov2_hip_output* out, uint32_t flags, char* err, size_t errlen) {
    if ((flags & DINOV2_HIP_CLASSIFY) != 0 && !m->hp.has_classifier) {
        set_err(err, errlen, "classify requested but the model was loaded without a classifier head");
        return DINOV2_HIP_ERR_NO_HEAD;
    }
    if (out && out->on_device && (out->topk_ids || out->topk_probs)) {
        set_err(err, errlen, "top-k outputs are host-only");
        return DINOV2_HIP_ERR_INVALID;
    }
    return DINOV2_HIP_OK;
}

// the network input size of `in`: for raw 8-bit input, the one dino_classify_preprocess | dino_preprocess decide (dinov2.cpp:106-156)
void dinov2::network_size(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, int* h, int* w) {
    *h = in->height;
    *w = in->width;
    if (in->layout == DINOV2_HIP_U8_BGR_HWC)
        dinov2_hip_preprocess_size((flags & DINOV2_HIP_CLASSIFY) ? 1 : 0, in->height, in->width, (int32_t)m->hp.patch_size, h, w);
}

// =============================================================================================================
// session
// =============================================================================================================
int dinov2::reserve(dinov2_hip_session* s, DevBuf& buf, size_t need, const char* who, char* err, size_t errlen) {
    if (need <= buf.bytes) return DINOV2_HIP_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (buf.ptr) HIP_TRY(hipFree(buf.ptr));
    buf = DevBuf{};
    const hipError_t e = hipMalloc(&buf.ptr, need);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        buf.ptr = nullptr;
        set_err(err, errlen, "%s: %zu bytes of scratch refused: %s", who, need, hipGetErrorString(e));
        return DINOV2_HIP_ERR_HIP;
    }
    buf.bytes = need;
    return DINOV2_HIP_OK;
}

namespace {

struct Carve {
    size_t img, col, x, ln, qkv, att, hid, fin, feat, logits, probs, pos, stats, stats_bytes, total;
};

// The workspace of one pass over `n` images with `pixels` pixels, `patches` patches and `M` token rows in all; pos_floats: the carve's own
// position embedding (a uniform batch has one; a list keeps its embeddings in scratch[SCRATCH_LIST_POS])
Carve carve_sizes(const dinov2_hip_model* m, size_t n, size_t pixels, size_t patches, size_t M, size_t pos_floats) {
    const size_t H = m->hp.hidden_size, F = m->hp.ffn_hidden, C = std::max<size_t>(m->hp.num_classes, 1);
    Carve c{};
    size_t off = 0;
    auto put = [&](size_t bytes) {
        const size_t o = off;
        off += align_up(bytes, 256);
        return o;
    };
    c.img = put(sizeof(float) * 3 * pixels);
    c.col = put(2 * patches * m->kpe_pad);
    c.x = put(sizeof(float) * M * H);
    c.ln = put(2 * M * H);
#if defined(DINO_PREC) && (DINO_PREC & 25)
    c.qkv = put(2 * M * 6 * H);  // (tuning build, profiles/r05_parity_attribution.md) second f16 word of q | k | v behind the first
#else
    c.qkv = put(2 * M * 3 * H);
#endif
    c.att = put(2 * M * H);
    c.hid = put(2 * M * F);
    c.fin = put(sizeof(float) * M * H);
    c.feat = put(sizeof(float) * n * 2 * H);
    c.logits = put(sizeof(float) * n * C);
    c.probs = put(sizeof(float) * n * C);
    c.pos = put(sizeof(float) * pos_floats);
    c.stats_bytes = m->ln_fold ? sizeof(float) * 2 * M * ln_stat_slots((int)H) : 0;
    c.stats = put(c.stats_bytes);
    c.total = off;
    return c;
}

Carve carve_of(const dinov2_hip_model* m, int B, int h, int w) {
    const Dims d = dims_of(m, B, h, w);
    return carve_sizes(m, (size_t)B, (size_t)B * h * w, (size_t)B * d.P, (size_t)d.M, (size_t)(1 + d.P) * m->hp.hidden_size);
}

// Makes the workspace at least c.total bytes (captured graphs point into the old one: gone before it is freed) and points the session's views
// into it.  The caller records what the carve is for (cur_b / cur_h / cur_w, list_key).
int apply_carve(dinov2_hip_session* s, const Carve& c, char* err, size_t errlen) {
    DevBuf& buf = s->scratch[SCRATCH_WS];
    if (c.total > buf.bytes) {
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (auto& g : s->graphs)
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
        s->graphs.clear();
        const int rc = reserve(s, buf, c.total, "workspace", err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
    }
    char* const ws = buf.as<char>();
    s->img = (float*)(ws + c.img);
    s->col = ws + c.col;
    s->x = (float*)(ws + c.x);
    s->ln = ws + c.ln;
    s->qkv = ws + c.qkv;
    s->att = ws + c.att;
    s->hid = ws + c.hid;
    s->fin = (float*)(ws + c.fin);
    s->feat = (float*)(ws + c.feat);
    s->logits = (float*)(ws + c.logits);
    s->probs = (float*)(ws + c.probs);
    s->pos = (float*)(ws + c.pos);
    s->stats = s->model->ln_fold ? (float*)(ws + c.stats) : nullptr;
    // (the slots past hidden / 64 of every statistics row are read by the consumers and written by nobody: zero them with the carve)
    if (c.stats_bytes) HIP_TRY(hipMemsetAsync(s->stats, 0, c.stats_bytes, s->stream));
    s->pos_h = s->pos_w = -1;  // the carve moved: re-upload the pos-embed
    return DINOV2_HIP_OK;
}

int ensure_workspace(dinov2_hip_session* s, int B, int h, int w, char* err, size_t errlen) {
    if (s->cur_b == B && s->cur_h == h && s->cur_w == w && s->scratch[SCRATCH_WS].ptr) return DINOV2_HIP_OK;
    s->cur_b = 0;  // (nothing valid while the carve moves)
    s->list_key[2] = 0;
    const int rc = apply_carve(s, carve_of(s->model, B, h, w), err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    s->cur_b = B;
    s->cur_h = h;
    s->cur_w = w;
    return DINOV2_HIP_OK;
}

// the same for a list (dinov2_hip_predict_list): carved by its totals; cur_b = -1 makes the next uniform predict carve anew
int ensure_workspace_list(dinov2_hip_session* s, const ListPlan& lp, int n, char* err, size_t errlen) {
    const int64_t key[4] = {lp.pixels, lp.P, lp.M, n};
    if (s->cur_b == -1 && std::equal(key, key + 4, s->list_key) && s->scratch[SCRATCH_WS].ptr) return DINOV2_HIP_OK;
    s->cur_b = 0;
    s->list_key[2] = 0;
    const int rc = apply_carve(s, carve_sizes(s->model, (size_t)n, (size_t)lp.pixels, (size_t)lp.P, (size_t)lp.M, 0), err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    s->cur_b = -1;
    s->cur_h = s->cur_w = 0;
    std::copy(key, key + 4, s->list_key);
    return DINOV2_HIP_OK;
}

enum Kind : int {
    K_IM2COL = 0, K_INIT, K_PATCH_GEMM, K_LAYERNORM, K_QKV_GEMM, K_ATTENTION, K_OPROJ_GEMM, K_FC1_GEMM, K_FC2_GEMM,
    K_FINAL_LN, K_HEAD, K_LAYER_TAP, K_COUNT, K_IM2COL_STRIDE = K_COUNT, K_SLOTS  // (only the profile of a patch_stride model lists the last kind)
};
const char* const kKindNames[K_SLOTS] = {"im2col", "init_tokens", "gemm_patch_embed", "layernorm", "gemm_qkv",
                                         "attention", "gemm_attn_out", "gemm_ffn_in", "gemm_ffn_out", "final_layernorm",
                                         "head", "layer_tap", "im2col_stride"};

struct Scope {  // optional per-launch event pair
    dinov2_hip_session* s;
    int kind;
    hipEvent_t a = nullptr, b = nullptr;
    Scope(dinov2_hip_session* s_, int kind_) : s(s_), kind(kind_) {
        if (!s->profiling) return;
        auto get = [&]() {
            hipEvent_t e = nullptr;
            if (!s->free_events.empty()) {
                e = s->free_events.back();
                s->free_events.pop_back();
            } else {
                (void)hipEventCreate(&e);
            }
            return e;
        };
        a = get();
        b = get();
        (void)hipEventRecord(a, s->stream);
    }
    ~Scope() {
        if (!s->profiling) return;
        (void)hipEventRecord(b, s->stream);
        s->records.push_back(ProfRecord{kind, a, b});
    }
};

void drain_profile(dinov2_hip_session* s) {
    if (s->prof_ms.empty()) {
        s->prof_ms.assign(K_SLOTS, 0.0);
        s->prof_n.assign(K_SLOTS, 0);
    }
    for (auto& r : s->records) {
        (void)hipEventSynchronize(r.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            s->prof_ms[(size_t)r.kind] += ms;
            s->prof_n[(size_t)r.kind] += 1;
        }
        s->free_events.push_back(r.a);
        s->free_events.push_back(r.b);
    }
    s->records.clear();
}

// The forward pass: forward_features (dinov2.cpp:616-790) [+ forward_head :792-821], `nlayers` <= L layers.
// pos-embed for this grid, cached per (h0, w0): the reference recomputes it on every call (dinov2.cpp:937).  Host work +
// synchronisation: the callers of forward() run it first, BEFORE a stream capture, never inside one.
int prepare_pos(dinov2_hip_session* s, int B, int h, int w, char* err, size_t errlen) {
    const dinov2_hip_model* m = s->model;
    const int H = (int)m->hp.hidden_size;
    const int h0 = grid_of(m, h, w).h0, w0 = grid_of(m, h, w).w0;
    if (s->pos_h == h0 && s->pos_w == w0) return DINOV2_HIP_OK;
    const Dims d = dims_of(m, B, h, w);
    hipStream_t st = s->stream;
    HIP_TRY(hipStreamSynchronize(st));  // pos_stage may still be in flight from a previous shape
    s->pos_stage.resize((size_t)(1 + d.P) * H);
    interpolate_pos_embed(m->pos_host.data(), (int)(m->hp.img_size / m->hp.patch_size), H, h0, w0, s->pos_stage.data());
    HIP_TRY(hipMemcpyAsync(s->pos, s->pos_stage.data(), sizeof(float) * s->pos_stage.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    s->pos_h = h0;
    s->pos_w = w0;
    return DINOV2_HIP_OK;
}

// The "is `layer` the next requested one" cursor over a run descriptor's strictly ascending layer list: its slot (and on to the next) or -1.
struct LayerCursor {
    const int32_t* layers;
    int n, next = 0;
    int take(int layer) { return next < n && layers[next] == layer ? next++ : -1; }
};

// One pass over `p.runs` (model.h): the residual stream holds the runs' token rows one after the other.  The embedding and the head run once
// per run with B = its length and its own position embedding and pooling divisor; every layer launch works per row and takes M = all rows;
// attention goes over runs[0] or over the list's work table.  The position embeddings (prepare_pos / prepare_pos_list) and the table
// (prepare_items_list) are there before the call: nothing here synchronises or allocates, so a pass can be captured into a graph.
// Leaves final-LN tokens in s->fin, logits / probs [images, C] in s->logits / s->probs.
// ex.taps (dinov2_hip_predict_layers): one layer_tap launch per requested layer, on x as it stands after that many layers.  ex.attn
// (dinov2_hip_predict_attention): one attn_rows launch per requested block, on that block's qkv right after its QKV GEMM (the next block
// overwrites qkv; attention only reads it).  ex.dense (dinov2_hip_predict_dense): one dense_pack launch per requested layer, beside the tap.
// Without any of them, the launches are those of a plain forward.
int forward(dinov2_hip_session* s, const Pass& p, char* err, size_t errlen) {
    const dinov2_hip_model* m = s->model;
    const int H = (int)m->hp.hidden_size, F = (int)m->hp.ffn_hidden, R = (int)m->hp.num_register_tokens;
    const int nh = (int)m->hp.num_attention_heads, ps = (int)m->hp.patch_size;
    const int M = p.M, nlayers = p.nlayers;
    const PassExtras& ex = p.ex;
    hipStream_t st = s->stream;
    const DType dt = m->dt;
    if (p.nruns < 1 || (p.nruns > 1 && (!p.items || ex.any()))) {
        set_err(err, errlen, "forward: a pass of %d runs needs an attention work table and takes no taps, attention rows or dense pack", p.nruns);
        return DINOV2_HIP_ERR_INVALID;
    }
    const int B = p.runs[0].B, T = p.runs[0].T;  // what the extras and the uniform attention go by

    for (const PassRun* r = p.runs; r != p.runs + p.nruns; ++r) {
        char* const col = (char*)s->col + (size_t)r->patch0 * (size_t)m->kpe_pad * 2;
        float* const x = s->x + (size_t)r->row0 * H;
        {
            Scope sc(s, m->patch_stride == ps ? K_IM2COL : K_IM2COL_STRIDE);
            HIP_TRY(launch_patch_im2col(dt, r->img, col, r->B, r->h, r->w, ps, m->patch_stride, m->kpe_pad, p.layout, st));
        }
        {
            Scope sc(s, K_INIT);
            HIP_TRY(launch_init_tokens(x, m->cls, r->pos, m->reg, r->B, r->T, R, H, st));
        }
        {
            Scope sc(s, K_PATCH_GEMM);
            GemmArgs a{};
            a.A = col; a.W = m->patch_w; a.bias = m->patch_b; a.out = x; a.aux = r->pos;
            a.M = r->B * r->P; a.N = H; a.K = m->kpe_pad; a.ldo = H; a.P = r->P; a.T = r->T; a.R = R;
            HIP_TRY(launch_gemm(dt, EPI_PATCH, a, st));
        }
    }
    const float eps = m->hp.eps;
    LayerCursor tap_at{ex.taps.layers, ex.taps.n}, pack_at{ex.dense.layers, ex.dense.n}, attn_at{ex.attn.layers, ex.attn.n};
    auto tap = [&](int layer) -> hipError_t {  // x holds the output of `layer` layers: hand it out if it was asked for
        const int slot = tap_at.take(layer);
        if (slot < 0) return hipSuccess;
        const TapRun& t = ex.taps;
        const size_t k = (size_t)slot;
        Scope sc(s, K_LAYER_TAP);
        return launch_layer_tap(s->x, m->ln_w, m->ln_b, eps, B, T, R, H, t.norm, t.chw, t.patch ? t.patch + k * t.patch_stride : nullptr,
                                t.cls ? t.cls + k * t.cls_stride : nullptr, t.reg ? t.reg + k * t.reg_stride : nullptr, st);
    };
    HIP_TRY(tap(0));
    auto pack = [&](int layer) -> hipError_t {  // the same point as `tap`: this layer's patch rows as f16 into their columns of the dense operand
        const int slot = pack_at.take(layer);
        if (slot < 0) return hipSuccess;
        const dinov2_hip_dense_head* hd = ex.dense.head;
        Scope sc(s, K_LAYER_TAP);
        return launch_dense_pack(s->x, m->ln_w, m->ln_b, eps, B, T, R, H, hd->norm, hd->concat_cls, ex.dense.A, (size_t)hd->K,
                                 slot * hd->H * (hd->concat_cls ? 2 : 1), st);
    };
    HIP_TRY(pack(0));
    // LN fold (dinov2_hip_load_opts.ln_fold; kernels.h EPI_RESID_LN): no LayerNorm launches inside the layers.  `ln` holds T(gamma x) for the
    // NEXT LayerNorm and `stats` the row sums behind it, both written by whoever wrote x last: ln_prepare before layer 0, the residual
    // epilogues afterwards; the QKV / FFN-in epilogues apply mean, rstd and beta.
    const bool fold = m->ln_fold;
    const int gs = ln_stat_slots(H);
    if (fold && nlayers > 0) {
        Scope sc(s, K_LAYERNORM);
        HIP_TRY(launch_ln_prepare(dt, s->x, m->layers[0].norm1_w, s->ln, s->stats, gs, M, H, st));
    }
    for (int il = 0; il < nlayers; ++il) {
        const LayerWeights& ly = m->layers[(size_t)il];
        if (!fold) {
            Scope sc(s, K_LAYERNORM);
            HIP_TRY(launch_layernorm(dt, s->x, ly.norm1_w, ly.norm1_b, s->ln, M, H, eps, st));
        }
        int ldq = 3 * H;
        {
            Scope sc(s, K_QKV_GEMM);
            GemmArgs a{};
            a.A = s->ln; a.W = ly.qkv_w; a.bias = ly.qkv_b; a.out = s->qkv;
            a.M = M; a.N = 3 * H; a.K = H; a.ldo = 3 * H; a.qcols = H;
#if defined(DINO_PREC) && (DINO_PREC & 25)
            a.ldo = 6 * H;
#endif
            a.qscale = 0.125f * 1.44269504088896340736f;  // 1/sqrt(64) (dinov2.cpp:626) x log2(e): softmax runs on exp2
            if (fold) {
                a.stats = s->stats; a.ln_gs = gs; a.ln_s = ly.qkv_s; a.ln_c = ly.qkv_c; a.ln_eps = eps;
            }
            HIP_TRY(launch_gemm(dt, fold ? EPI_QKV_LN : EPI_QKV, a, st));
            ldq = a.ldo;
        }
        if (const int slot = attn_at.take(il + 1); slot >= 0) {  // booked as a tap: a tap of the attention
            const AttnRun& at = ex.attn;
            Scope sc(s, K_LAYER_TAP);
            HIP_TRY(launch_attn_rows(dt, s->qkv, ldq, at.probs + (size_t)slot * at.stride, B, T, H, nh, at.queries, at.nq, at.key0, at.nkeys, st));
        }
        {
            Scope sc(s, K_ATTENTION);  // (the two launchers give the same bits; the uniform one is the faster where it applies)
            HIP_TRY(p.items ? launch_attention_list(dt, s->qkv, s->att, p.items, p.n_items, p.n_items, H, nh, true, st)
                            : launch_attention(dt, s->qkv, s->att, B, T, H, nh, true, st));
        }
        {
            Scope sc(s, K_OPROJ_GEMM);
            GemmArgs a{};
            a.A = s->att; a.W = ly.o_w; a.bias = ly.o_b; a.out = s->x; a.aux = ly.ls1;
            a.M = M; a.N = H; a.K = H; a.ldo = H;
            if (fold) {
                a.ln_gamma = ly.norm2_w; a.xg = s->ln; a.stats = s->stats; a.ln_gs = gs;
            }
            HIP_TRY(launch_gemm(dt, fold ? EPI_RESID_LN : EPI_RESID, a, st));
        }
        if (!fold) {
            Scope sc(s, K_LAYERNORM);
            HIP_TRY(launch_layernorm(dt, s->x, ly.norm2_w, ly.norm2_b, s->ln, M, H, eps, st));
        }
        {
            Scope sc(s, K_FC1_GEMM);
            GemmArgs a{};
            a.A = s->ln; a.W = ly.fc1_w; a.bias = ly.fc1_b; a.out = s->hid;
            a.M = M; a.N = m->hp.swiglu ? 2 * F : F; a.K = H; a.ldo = F;
            if (fold) {
                a.stats = s->stats; a.ln_gs = gs; a.ln_s = ly.fc1_s; a.ln_c = ly.fc1_c; a.ln_eps = eps;
            }
            HIP_TRY(launch_gemm(dt, m->hp.swiglu ? (fold ? EPI_SWIGLU_LN : EPI_SWIGLU) : (fold ? EPI_GELU_LN : EPI_GELU), a, st));
        }
        {
            Scope sc(s, K_FC2_GEMM);
            GemmArgs a{};
            a.A = s->hid; a.W = ly.fc2_w; a.bias = ly.fc2_b; a.out = s->x; a.aux = ly.ls2;
            a.M = M; a.N = H; a.K = F; a.ldo = H;
            const bool feeds_ln1 = fold && il + 1 < nlayers;  // (the last layer's x goes to the final LayerNorm kernel)
            if (feeds_ln1) {
                a.ln_gamma = m->layers[(size_t)il + 1].norm1_w; a.xg = s->ln; a.stats = s->stats; a.ln_gs = gs;
            }
            HIP_TRY(launch_gemm(dt, feeds_ln1 ? EPI_RESID_LN : EPI_RESID, a, st));
        }
        HIP_TRY(tap(il + 1));
        HIP_TRY(pack(il + 1));
    }
    if (!p.finalize) return DINOV2_HIP_OK;
    {
        Scope sc(s, K_FINAL_LN);
        HIP_TRY(launch_layernorm_f32(s->x, m->ln_w, m->ln_b, s->fin, M, H, eps, st));
    }
    if (!p.classify) return DINOV2_HIP_OK;
    const int first = m->quirk_pool_regs ? 1 : 1 + R;
    const int Mg = (int)(m->hp.img_size / m->hp.patch_size);
    const size_t C = m->hp.num_classes;
    for (const PassRun* r = p.runs; r != p.runs + p.nruns; ++r) {  // the pooling divisor is the run's own
        const float div = m->quirk_const_div ? (float)(Mg * Mg) : (float)(r->T - first);
        const size_t i0 = (size_t)r->image0;
        Scope sc(s, K_HEAD);
        HIP_TRY(launch_head(dt, s->fin + (size_t)r->row0 * H, m->head_w, m->head_b, s->feat + i0 * 2 * H, s->logits + i0 * C, s->probs + i0 * C,
                            r->B, r->T, H, (int)C, first, 1.0f / div, st));
    }
    return DINOV2_HIP_OK;
}

// ---- dinov2_hip_predict_list: images of different sizes in one forward ------------------------------------------------------------------
// The position embeddings of the list's patch grids, one per distinct (h0, w0), in scratch[SCRATCH_LIST_POS]; pos_of[i] = image i's (device).
// They stay from call to call, up to DINOV2_HIP_LIST_POS_GRIDS of them: a list that would take the cache past that, or past its allocation,
// clears it first (so a single list with more distinct grids than the bound is served, and evicts everything else).  Staging as in
// prepare_pos: the host buffer is rewritten only after a wait for the stream, and the call returns after the copy has landed.
int prepare_pos_list(dinov2_hip_session* s, const std::vector<ListImage>& im, std::vector<const float*>& pos_of, char* err, size_t errlen) {
    const dinov2_hip_model* m = s->model;
    const size_t H = m->hp.hidden_size;
    auto find = [&](int h0, int w0) {
        for (size_t k = 0; k < s->list_pos.size(); ++k)
            if (s->list_pos[k].h0 == h0 && s->list_pos[k].w0 == w0) return (long)k;
        return -1L;
    };
    auto missing_of = [&](std::vector<std::pair<int, int>>& miss) {  // the list's grids that are not cached, each once; their floats
        size_t floats = 0;
        miss.clear();
        for (const ListImage& g : im) {
            if (find(g.h0, g.w0) >= 0 || std::find(miss.begin(), miss.end(), std::make_pair(g.h0, g.w0)) != miss.end()) continue;
            miss.emplace_back(g.h0, g.w0);
            floats += (size_t)(1 + g.P) * H;
        }
        return floats;
    };
    std::vector<std::pair<int, int>> miss;
    size_t add = missing_of(miss);
    DevBuf& buf = s->scratch[SCRATCH_LIST_POS];
    if (!miss.empty() && (s->list_pos.size() + miss.size() > DINOV2_HIP_LIST_POS_GRIDS || (s->list_pos_used + add) * sizeof(float) > buf.bytes)) {
        s->list_pos.clear();  // full: cleared, not grown entry by entry (the launches that read the old entries are ahead of the copy on the stream)
        s->list_pos_used = 0;
        add = missing_of(miss);
        const int rc = reserve(s, buf, add * sizeof(float), "predict_list", err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
    }
    if (!miss.empty()) {
        hipStream_t st = s->stream;
        HIP_TRY(hipStreamSynchronize(st));  // list_pos_stage may still be in flight
        s->list_pos_stage.resize(add);
        size_t off = 0;
        for (const auto& g : miss) {
            interpolate_pos_embed(m->pos_host.data(), (int)(m->hp.img_size / m->hp.patch_size), (int)H, g.first, g.second, s->list_pos_stage.data() + off);
            s->list_pos.push_back({g.first, g.second, s->list_pos_used + off});
            off += (size_t)(1 + g.first * g.second) * H;
        }
        HIP_TRY(hipMemcpyAsync(buf.as<float>() + s->list_pos_used, s->list_pos_stage.data(), sizeof(float) * add, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        s->list_pos_used += add;
    }
    pos_of.resize(im.size());
    for (size_t i = 0; i < im.size(); ++i) pos_of[i] = buf.as<float>() + s->list_pos[(size_t)find(im[i].h0, im[i].w0)].off;
    return DINOV2_HIP_OK;
}

// The attention work table on the device; uploaded only when it differs from the one already there (a caller that repeats a list pays once).
int prepare_items_list(dinov2_hip_session* s, const std::vector<AttnItem>& items, char* err, size_t errlen) {
    const size_t bytes = items.size() * sizeof(AttnItem);
    DevBuf& buf = s->scratch[SCRATCH_LIST_ITEMS];
    if (buf.ptr && s->list_items_host.size() == items.size() && std::memcmp(s->list_items_host.data(), items.data(), bytes) == 0) return DINOV2_HIP_OK;
    s->list_items_host.clear();  // (nothing valid on the device until the copy below has been queued)
    const int rc = reserve(s, buf, bytes, "predict_list", err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));  // a copy from list_items_host may still be in flight
    s->list_items_host = items;
    HIP_TRY(hipMemcpyAsync(buf.ptr, s->list_items_host.data(), bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return DINOV2_HIP_OK;
}

// Opt-in (DINOV2_HIP_GRAPHS=1): second and later forwards with the same (workspace, input pointer, shape, flags) replay a
// captured hipGraph; the first occurrence runs eagerly (one-off shapes never pay for a capture), the second is captured.
// Off by default because it buys nothing on an idle host: the forward is kernel-bound (178 launches, mean gap 1.0 us in the
// rocprofv3 trace at batch 1), measured p50 3.07 ms with graphs vs 3.06 ms without.  It is there for hosts whose launch
// thread is contended.
int forward_maybe_graph(dinov2_hip_session* s, const Pass& p, char* err, size_t errlen) {
    static const bool enabled = [] {
        const char* e = getenv("DINOV2_HIP_GRAPHS");
        return e && atoi(e) != 0;
    }();
    auto eager = [&] { return forward(s, p, err, errlen); };
    if (!enabled || s->profiling) return eager();
    const PassRun& r = p.runs[0];  // (a uniform batch: its one run is the key)
    hipStream_t st = s->stream;
    dinov2_hip_session::GraphEntry* hit = nullptr;
    for (auto& g : s->graphs)
        if (g.ws == s->scratch[SCRATCH_WS].ptr && g.img == r.img && g.b == r.B && g.h == r.h && g.w == r.w && g.layout == p.layout &&
            g.classify == (int)p.classify)
            hit = &g;
    if (hit && hit->exec) {
        ++hit->uses;
        HIP_TRY(hipGraphLaunch(hit->exec, st));
        return DINOV2_HIP_OK;
    }
    if (hit && hit->uses < 0) return eager();  // capture failed before
    if (!hit) {  // first sighting: remember it, run eagerly
        if (s->graphs.size() >= 8) {  // evict the least used entry
            size_t v = 0;
            for (size_t i = 1; i < s->graphs.size(); ++i)
                if (s->graphs[i].uses < s->graphs[v].uses) v = i;
            if (s->graphs[v].exec) (void)hipGraphExecDestroy(s->graphs[v].exec);
            s->graphs.erase(s->graphs.begin() + (long)v);
        }
        s->graphs.push_back({s->scratch[SCRATCH_WS].ptr, r.img, r.B, r.h, r.w, p.layout, (int)p.classify, 0, nullptr});
        return eager();
    }
    // second sighting: capture.  Nothing in forward() synchronises or allocates.
    if (hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        return eager();
    }
    const int rc = eager();
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(st, &graph);
    if (rc != DINOV2_HIP_OK || ec != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        hit->uses = -1000000;  // do not try again for this key
        if (rc != DINOV2_HIP_OK) return rc;
        return eager();
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess || !exec) {
        (void)hipGetLastError();
        hit->uses = -1000000;
        return eager();
    }
    hit->exec = exec;
    hit->uses = 1;
    HIP_TRY(hipGraphLaunch(exec, st));
    return DINOV2_HIP_OK;
}

}  // namespace

// out->topk_ids / topk_probs [B, topk] from host probabilities [B, C]: descending sort of all classes like dinov2.cpp:961-965
static void topk_rows(const float* probs_host, int B, size_t C, dinov2_hip_output* out) {
    const int k = std::min<int>(out->topk, (int)C);
    std::vector<int> idx(C);
    for (int b = 0; b < B; ++b) {
        const float* p = probs_host + (size_t)b * C;
        std::iota(idx.begin(), idx.end(), 0);
        std::partial_sort(idx.begin(), idx.begin() + k, idx.end(),
                          [&](int a, int c2) { return p[a] > p[c2] || (p[a] == p[c2] && a < c2); });
        for (int i = 0; i < out->topk; ++i) {
            if (out->topk_ids) out->topk_ids[(size_t)b * out->topk + i] = i < k ? idx[(size_t)i] : -1;
            if (out->topk_probs) out->topk_probs[(size_t)b * out->topk + i] = i < k ? p[idx[(size_t)i]] : 0.f;
        }
    }
}

// Copy-out of a finished pass, run by run: the tail of dino_predict (dinov2.cpp:950-999).  cls [n, H]; the patch rows packed, one image after
// the other (a list's image i at rows [offsets[i], offsets[i + 1]) of dinov2_hip_list_rows); logits / probs [n, C].  Device outputs are only
// enqueued; host outputs are complete on return, after ONE wait.
static int copy_out(dinov2_hip_session* s, const PassRun* runs, int nruns, bool classify, dinov2_hip_output* out, char* err, size_t errlen) {
    const dinov2_hip_model* m = s->model;
    hipStream_t st = s->stream;
    const size_t H = m->hp.hidden_size, C = m->hp.num_classes;
    const int n = runs[nruns - 1].image0 + runs[nruns - 1].B;
    const int first = classify ? 1 : 1 + (int)m->hp.num_register_tokens;  // rows [1+R, T) for features, [1, T) when classifying (dinov2.cpp:770-789)
    const hipMemcpyKind kind = out->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    size_t orow = 0;
    for (const PassRun* r = runs; r != runs + nruns; ++r) {
        const float* fin = s->fin + (size_t)r->row0 * H;
        const size_t pitch = sizeof(float) * (size_t)r->T * H, wbytes = sizeof(float) * (size_t)(r->T - first) * H;
        if (out->cls)  // "cls_token" = final-LN row 0 (dinov2.cpp:764-768)
            HIP_TRY(hipMemcpy2DAsync(out->cls + (size_t)r->image0 * H, sizeof(float) * H, fin, pitch, sizeof(float) * H, (size_t)r->B, kind, st));
        if (out->patch_tokens)
            HIP_TRY(hipMemcpy2DAsync(out->patch_tokens + orow * H, wbytes, fin + (size_t)first * H, pitch, wbytes, (size_t)r->B, kind, st));
        orow += (size_t)r->B * (size_t)(r->T - first);
    }
    if (classify) {
        if (out->logits) HIP_TRY(hipMemcpyAsync(out->logits, s->logits, sizeof(float) * n * C, kind, st));
        if (out->probs) HIP_TRY(hipMemcpyAsync(out->probs, s->probs, sizeof(float) * n * C, kind, st));
    }
    if (out->on_device) return DINOV2_HIP_OK;

    std::vector<float> probs_host;
    const bool want_topk = classify && out->topk > 0 && (out->topk_ids || out->topk_probs);
    if (want_topk) {
        probs_host.resize((size_t)n * C);
        HIP_TRY(hipMemcpyAsync(probs_host.data(), s->probs, sizeof(float) * n * C, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (want_topk) topk_rows(probs_host.data(), n, C, out);
    return DINOV2_HIP_OK;
}

// ... of the session's last un-split forward (shape in s->last_*): one run
int dinov2::fetch_outputs(dinov2_hip_session* s, dinov2_hip_output* out, char* err, size_t errlen) {
    const PassRun run = uniform_run(s->model, nullptr, s->last_b, s->last_h, s->last_w, nullptr);
    return copy_out(s, &run, 1, s->last_classify, out, err, errlen);
}

extern "C" int dinov2_hip_session_create(dinov2_hip_model* m, void* stream, dinov2_hip_session** out, char* err,
                                         size_t errlen) {
    if (!m || !out) {
        set_err(err, errlen, "null argument");
        return DINOV2_HIP_ERR_INVALID;
    }
    *out = nullptr;
    HIP_TRY(hipSetDevice(m->device));
    std::unique_ptr<dinov2_hip_session> s(new dinov2_hip_session());
    s->model = m;
    if (stream) {
        s->stream = (hipStream_t)stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        s->own_stream = true;
    }
    *out = s.release();
    return DINOV2_HIP_OK;
}

extern "C" void dinov2_hip_session_free(dinov2_hip_session* s) {
    if (!s) return;
    (void)hipSetDevice(s->model->device);
    (void)hipStreamSynchronize(s->stream);
    drain_profile(s);
    for (auto e : s->free_events) (void)hipEventDestroy(e);
    for (auto& g : s->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    for (DevBuf& b : s->scratch)
        if (b.ptr) (void)hipFree(b.ptr);
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" size_t dinov2_hip_workspace_bytes(const dinov2_hip_model* m, int32_t batch, int32_t height, int32_t width) {
    if (!m || batch <= 0 || height <= 0 || width <= 0 || check_rows_at(m, height, width, nullptr, 0) != DINOV2_HIP_OK) return 0;
    return carve_of(m, batch, height, width).total;
}

extern "C" int dinov2_hip_session_sync(dinov2_hip_session* s) {
    if (!s) return DINOV2_HIP_ERR_INVALID;
    return hipStreamSynchronize(s->stream) == hipSuccess ? DINOV2_HIP_OK : DINOV2_HIP_ERR_HIP;
}

extern "C" void* dinov2_hip_session_stream(dinov2_hip_session* s) { return s ? (void*)s->stream : nullptr; }

extern "C" int dinov2_hip_session_profile(dinov2_hip_session* s, int32_t enable) {
    if (!s) return DINOV2_HIP_ERR_INVALID;
    (void)hipStreamSynchronize(s->stream);
    drain_profile(s);
    s->profiling = enable != 0;
    if (enable) {
        s->prof_ms.assign(K_SLOTS, 0.0);
        s->prof_n.assign(K_SLOTS, 0);
    }
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_session_profile_read(dinov2_hip_session* s, int32_t max, const char** names, float* total_ms,
                                               int32_t* launches) {
    if (!s) return 0;
    (void)hipStreamSynchronize(s->stream);
    drain_profile(s);
    const int n = std::min<int>(max, s->model->patch_stride == (int)s->model->hp.patch_size ? K_COUNT : K_SLOTS);
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = kKindNames[i];
        if (total_ms) total_ms[i] = (float)s->prof_ms[(size_t)i];
        if (launches) launches[i] = s->prof_n[(size_t)i];
    }
    return n;
}

size_t dinov2_max_pass_batch(const dinov2_hip_model* m, int h, int w) {
    // The kernels address activations with 32-bit offsets (staging cursors of the GEMMs and of the attention): the widest
    // activation buffer of one forward must stay below 2^31 bytes (ViT-L @518: 190 images per pass).
    const Dims d1 = dims_of(m, 1, h, w);
    // (an image whose own rows pass the limit is refused by every entry point before it gets here: dinov2_check_pass_rows)
    size_t bmax = std::max<size_t>(1, ((size_t)1 << 31) / ((size_t)d1.T * widest_row(m) * 2));
    if (const char* e = getenv("DINOV2_HIP_MAX_CHUNK"))  // testing aid: force the split at small sizes
        if (atoi(e) > 0) bmax = std::min<size_t>(bmax, (size_t)atoi(e));
    return bmax;
}

// =============================================================================================================
// predict
// =============================================================================================================
// The dense stage of one pass of B images at network input size h x w, after its forward: the logits GEMM over the packed operand, the
// copy-out of the low-resolution logits, the resampling reduction, each output at this pass's image offset.  Enqueues only.
static int dense_stage(dinov2_hip_session* s, const DenseRun& dr, int B, int h, int w, char* err, size_t errlen) {
    const dinov2_hip_model* m = s->model;
    const dinov2_hip_dense_head* hd = dr.head;
    const dinov2_hip_dense_out* o = dr.out;
    const int h0 = grid_of(m, h, w).h0, w0 = grid_of(m, h, w).w0;
    const size_t P = (size_t)h0 * w0, M = (size_t)B * P, K = (size_t)hd->K, C = (size_t)hd->C, cpad = (size_t)hd->cpad;
    hipStream_t st = s->stream;
    Scope sc(s, K_HEAD);
    // (the GEMM's staging cursors are 32-bit byte offsets from A: row chunks below 2^31 bytes.  A row's bits do not depend on the chunking.)
    const size_t chunk = std::max<size_t>(256, (((size_t)1 << 31) / (K * 2)) / 256 * 256);
    for (size_t r0 = 0; r0 < M; r0 += chunk) {
        GemmArgs a{};
        a.A = dr.A + r0 * K; a.W = hd->w16; a.bias = hd->bias; a.out = dr.lg + r0 * cpad;
        a.M = (int)std::min(chunk, M - r0); a.N = (int)cpad; a.K = (int)K; a.ldo = (int)cpad;
        HIP_TRY(launch_gemm(DT_F16, EPI_PLAIN_F32, a, st));
    }
    const hipMemcpyKind kind = o->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (o->logits)
        HIP_TRY(hipMemcpy2DAsync(o->logits + dr.b0 * P * C, C * 4, dr.lg, cpad * 4, C * 4, M, kind, st));
    if (!o->labels && !o->value) return DINOV2_HIP_OK;
    const size_t npx = (size_t)dr.oh * dr.ow;
    uint8_t* lab = o->labels ? (o->on_device ? o->labels + dr.b0 * npx : dr.lab) : nullptr;
    float* val = o->value ? (o->on_device ? o->value + dr.b0 * npx : dr.val) : nullptr;
    const DenseReducePlan plan = dense_reduce_plan(h0, w0, hd->C, dr.oh, dr.ow);
    HIP_TRY(launch_dense_reduce(dr.lg, (int)cpad, B, h0, w0, hd->C, dr.oh, dr.ow, hd->reduce, hd->centers, hd->eps, lab, val, plan, st));
    if (!o->on_device) {
        if (lab) HIP_TRY(hipMemcpyAsync(o->labels + dr.b0 * npx, lab, (size_t)B * npx, hipMemcpyDeviceToHost, st));
        if (val) HIP_TRY(hipMemcpyAsync(o->value + dr.b0 * npx, val, (size_t)B * npx * 4, hipMemcpyDeviceToHost, st));
    }
    return DINOV2_HIP_OK;
}

// The preprocessed f32 images of `in` on the device: where the caller has them, or host ones copied into the workspace (carved for them)
static int images_f32(dinov2_hip_session* s, const dinov2_hip_input* in, const float** img, char* err, size_t errlen) {
    *img = in->data;
    if (in->on_device) return DINOV2_HIP_OK;
    HIP_TRY(hipMemcpyAsync(s->img, in->data, sizeof(float) * 3 * (size_t)in->batch * in->height * in->width, hipMemcpyHostToDevice, s->stream));
    *img = s->img;
    return DINOV2_HIP_OK;
}

// `ex`: the layer taps of dinov2_hip_predict_layers, the attention rows of dinov2_hip_predict_attention (device pointers), the head and outputs
// of dinov2_hip_predict_dense (extras.cpp builds them); empty for a plain predict
int dinov2::predict_impl(dinov2_hip_session* s, const dinov2_hip_input* in, dinov2_hip_output* out, uint32_t flags, const PassExtras& ex,
                         char* err, size_t errlen) {
    int rc = check_input(s, in, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const dinov2_hip_model* m = s->model;
    rc = check_predict_args(m, out, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const bool classify = (flags & DINOV2_HIP_CLASSIFY) != 0;
    HIP_TRY(hipSetDevice(m->device));
    s->last_b = 0;  // nothing to fetch until this forward has succeeded (a failed or re-carving call must not leave the old shape behind)
    const int B = in->batch;
    const bool raw_u8 = in->layout == DINOV2_HIP_U8_BGR_HWC;
    const int layout = raw_u8 ? DINOV2_HIP_BGR_HWC : in->layout;  // (raw images are preprocessed into BGR_HWC below)
    int h, w;
    network_size(m, in, flags, &h, &w);
    {
        // Batches longer than one pass takes (dinov2_max_pass_batch) are split here, transparently -- B images are B independent
        // forwards, so the results do not change.  Passes run last chunk first, so the session ends up holding chunk 0
        // (dinov2_hip_pca3's "image 0 of the last predict").
        const Dims d1 = dims_of(m, 1, h, w);
        const size_t bmax = dinov2_max_pass_batch(m, h, w);
        if ((size_t)B > bmax) {
            const size_t H = m->hp.hidden_size, C = m->hp.num_classes, R = m->hp.num_register_tokens;
            const size_t tok_rows = (size_t)d1.T - (classify ? 1 : 1 + R);
            const size_t in_stride = raw_u8 ? (size_t)in->height * in->width * 3  /* bytes */
                                            : (size_t)3 * h * w * sizeof(float);
            const int nchunks = (int)(((size_t)B + bmax - 1) / bmax);
            for (int c = nchunks - 1; c >= 0; --c) {
                const size_t b0 = (size_t)c * bmax, bn = std::min<size_t>(bmax, (size_t)B - b0);
                dinov2_hip_input ci = *in;
                ci.data = reinterpret_cast<const float*>(reinterpret_cast<const char*>(in->data) + b0 * in_stride);
                ci.batch = (int32_t)bn;
                dinov2_hip_output co{};
                if (out) {
                    co = *out;
                    if (out->cls) co.cls = out->cls + b0 * H;
                    if (out->patch_tokens) co.patch_tokens = out->patch_tokens + b0 * tok_rows * H;
                    if (out->logits) co.logits = out->logits + b0 * C;
                    if (out->probs) co.probs = out->probs + b0 * C;
                    if (out->topk_ids) co.topk_ids = out->topk_ids + b0 * (size_t)out->topk;
                    if (out->topk_probs) co.topk_probs = out->topk_probs + b0 * (size_t)out->topk;
                }
                rc = predict_impl(s, &ci, out ? &co : nullptr, flags, ex.at_image(b0, (size_t)d1.P, R, H, m->hp.num_attention_heads), err,
                                  errlen);
                if (rc != DINOV2_HIP_OK) return rc;
            }
            s->last_b = 0;  // the workspace holds chunk 0 only: nothing for dinov2_hip_fetch
            return DINOV2_HIP_OK;
        }
    }
    rc = ensure_workspace(s, B, h, w, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    hipStream_t st = s->stream;

    const float* img = in->data;
    if (raw_u8) {
        const size_t nraw = (size_t)B * in->height * in->width * 3;
        const uint8_t* src = reinterpret_cast<const uint8_t*>(in->data);
        if (!in->on_device) {
            rc = reserve(s, s->scratch[SCRATCH_RAW], nraw, "predict", err, errlen);
            if (rc != DINOV2_HIP_OK) return rc;
            HIP_TRY(hipMemcpyAsync(s->scratch[SCRATCH_RAW].ptr, src, nraw, hipMemcpyHostToDevice, st));
            src = s->scratch[SCRATCH_RAW].as<uint8_t>();
        }
        const int rh = classify ? 256 : h, rw = classify ? 256 : w;
        HIP_TRY(launch_preprocess_u8(src, s->img, B, in->height, in->width, rh, rw, (rh - h) / 2, (rw - w) / 2, h, w, st));
        img = s->img;
    } else {
        rc = images_f32(s, in, &img, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
    }
    rc = prepare_pos(s, B, h, w, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const PassRun run = uniform_run(m, img, B, h, w, s->pos);
    const Pass pass{&run, 1, B * run.T, nullptr, 0, layout, classify, (int)m->hp.num_hidden_layers, true, ex};
    // (a tapped forward runs eagerly, past the graph cache: its key knows nothing of the caller's tap pointers)
    rc = ex.any() ? forward(s, pass, err, errlen) : forward_maybe_graph(s, pass, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (ex.dense.n) {
        rc = dense_stage(s, ex.dense, B, h, w, err, errlen);
        if (rc != DINOV2_HIP_OK) return rc;
    }
    // what dinov2_hip_pca3(tokens = NULL) works on: the patch rows of image 0 in `fin`
    s->last_first = classify ? 1 : 1 + (int)m->hp.num_register_tokens;
    s->last_patches = run.T - s->last_first;
    s->last_t = run.T;
    s->last_b = B;
    s->last_h = h;
    s->last_w = w;
    s->last_classify = classify;
    if (!out) return DINOV2_HIP_OK;
    return fetch_outputs(s, out, err, errlen);
}

extern "C" int dinov2_hip_predict(dinov2_hip_session* s, const dinov2_hip_input* in, dinov2_hip_output* out,
                                  uint32_t flags, char* err, size_t errlen) {
    return predict_impl(s, in, out, flags, PassExtras{}, err, errlen);
}

// =============================================================================================================
// predict_list
// =============================================================================================================
namespace {

// The order of the attention work table (kernels.h ListOrder).  Shipped: as given -- profiles/predict_list.md (c) has both times.
// DINOV2_HIP_LIST_ORDER=1 / the "list_order" switch picks the other (a measuring aid; the bits do not depend on it).
int list_table_order() { return tune_get(TUNE_LIST_ORDER) == 1 ? (int)LIST_ORDER_LONGEST_FIRST : (int)LIST_ORDER_AS_GIVEN; }

// The argument checks of dinov2_hip_list_rows and dinov2_hip_predict_list that need no device: every refusal names the image.  On success
// hs / ws hold the network sizes.  need_data: the image pointers are checked too.
int check_list(const dinov2_hip_model* m, const dinov2_hip_image_list* l, uint32_t flags, bool need_data, std::vector<int32_t>& hs,
               std::vector<int32_t>& ws, char* err, size_t errlen) {
    if (!m || !l) {
        set_err(err, errlen, "null session / model / list");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (l->n <= 0) {
        set_err(err, errlen, "an image list holds at least one image (n = %d)", l->n);
        return DINOV2_HIP_ERR_INVALID;
    }
    if (!l->height || !l->width || (need_data && !l->data)) {
        set_err(err, errlen, "null data / height / width array of the image list");
        return DINOV2_HIP_ERR_INVALID;
    }
    hs.resize((size_t)l->n);
    ws.resize((size_t)l->n);
    // one pass, as dinov2_max_pass_batch has it for a uniform batch: the widest activation buffer stays below 2^31 bytes
    const int64_t widest = (int64_t)widest_row(m);
    int64_t M = 0;
    int first_over = -1;
    for (int i = 0; i < l->n; ++i) {
        if (need_data && !l->data[i]) {
            set_err(err, errlen, "image %d: null data pointer", i);
            return DINOV2_HIP_ERR_INVALID;
        }
        dinov2_hip_input in{};
        in.data = reinterpret_cast<const float*>(need_data ? l->data[i] : (const void*)l);  // (never dereferenced here)
        in.batch = 1; in.height = l->height[i]; in.width = l->width[i]; in.layout = l->layout; in.on_device = l->on_device;
        char why[256] = "";
        const int rc = dinov2_check_input_grid(m, &in, flags, why, sizeof(why));
        if (rc != DINOV2_HIP_OK) {
            set_err(err, errlen, "image %d: %s", i, why);
            return rc;
        }
        int h, w;
        network_size(m, &in, flags, &h, &w);
        hs[(size_t)i] = h;
        ws[(size_t)i] = w;
        M += dims_of(m, 1, h, w).T;
        if (first_over < 0 && M * widest * 2 >= ((int64_t)1 << 31)) first_over = i;
    }
    if (first_over >= 0) {
        set_err(err, errlen, "image %d: with it the list has too many token rows for one pass (%lld in all; rows * %lld * 2 must stay below 2^31, "
                "the 32-bit activation offsets of dinov2_hip_predict's passes).  A list is refused, not split: hand it over in parts",
                first_over, (long long)M, (long long)widest);
        return DINOV2_HIP_ERR_INVALID;
    }
    return DINOV2_HIP_OK;
}

}  // namespace

extern "C" int dinov2_hip_list_rows(const dinov2_hip_model* m, const dinov2_hip_image_list* list, uint32_t flags, int64_t* offsets, char* err,
                                    size_t errlen) {
    std::vector<int32_t> hs, ws;
    const int rc = check_list(m, list, flags, false, hs, ws, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    if (!offsets) {
        set_err(err, errlen, "null offsets");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int skip = (flags & DINOV2_HIP_CLASSIFY) ? 1 : 1 + (int)m->hp.num_register_tokens;  // rows of an image that are not handed out
    offsets[0] = 0;
    for (int i = 0; i < list->n; ++i) offsets[i + 1] = offsets[i] + dims_of(m, 1, hs[(size_t)i], ws[(size_t)i]).T - skip;
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_predict_list(dinov2_hip_session* s, const dinov2_hip_image_list* list, dinov2_hip_output* out, uint32_t flags, char* err,
                                       size_t errlen) {
    std::vector<int32_t> hs, ws;
    int rc = check_list(s ? s->model : nullptr, list, flags, true, hs, ws, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const dinov2_hip_model* m = s->model;
    rc = check_predict_args(m, out, flags, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const bool classify = (flags & DINOV2_HIP_CLASSIFY) != 0;
    const int n = list->n, R = (int)m->hp.num_register_tokens, nh = (int)m->hp.num_attention_heads;
    HIP_TRY(hipSetDevice(m->device));
    // a list forward leaves no "last un-split forward": nothing for dinov2_hip_fetch, pca3(tokens = NULL), match / bank on resident tokens
    s->last_b = 0;
    s->last_patches = 0;
    s->last_t = 0;

    std::vector<ListImage> im((size_t)n);
    std::vector<ListRun> lruns((size_t)n);
    ListPlan lp = list_plan(n, hs.data(), ws.data(), (int)m->hp.patch_size, m->patch_stride, R, nh, list_table_order(), im.data(), lruns.data(), nullptr);
    std::vector<PassRun> runs((size_t)lp.nruns);
    list_runs(im.data(), lruns.data(), lp.nruns, hs.data(), ws.data(), runs.data());
    std::vector<AttnItem> items((size_t)lp.units);
    lp = list_plan(n, hs.data(), ws.data(), (int)m->hp.patch_size, m->patch_stride, R, nh, list_table_order(), nullptr, nullptr, items.data());

    rc = ensure_workspace_list(s, lp, n, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    hipStream_t st = s->stream;

    // the images, run by run contiguous on the device: where the caller's device images already are, they are read in place
    const bool raw_u8 = list->layout == DINOV2_HIP_U8_BGR_HWC;
    const int layout = raw_u8 ? DINOV2_HIP_BGR_HWC : list->layout;
    std::vector<size_t> pix((size_t)n + 1, 0);  // pixels before image i (network size): its place in s->img
    for (int i = 0; i < n; ++i) pix[(size_t)i + 1] = pix[(size_t)i] + (size_t)hs[(size_t)i] * ws[(size_t)i];
    if (raw_u8) {
        std::vector<const uint8_t*> src((size_t)n);
        for (int i = 0; i < n; ++i) src[(size_t)i] = static_cast<const uint8_t*>(list->data[i]);
        if (!list->on_device) {
            size_t nraw = 0;
            for (int i = 0; i < n; ++i) nraw += align_up((size_t)list->height[i] * list->width[i] * 3, 16);
            rc = reserve(s, s->scratch[SCRATCH_RAW], nraw, "predict_list", err, errlen);
            if (rc != DINOV2_HIP_OK) return rc;
            uint8_t* d = s->scratch[SCRATCH_RAW].as<uint8_t>();
            for (int i = 0; i < n; ++i) {
                const size_t bytes = (size_t)list->height[i] * list->width[i] * 3;
                HIP_TRY(hipMemcpyAsync(d, src[(size_t)i], bytes, hipMemcpyHostToDevice, st));
                src[(size_t)i] = d;
                d += align_up(bytes, 16);
            }
        }
        for (int i = 0; i < n; ++i) {  // each image to its own network size
            const int h = hs[(size_t)i], w = ws[(size_t)i], rh = classify ? 256 : h, rw = classify ? 256 : w;
            HIP_TRY(launch_preprocess_u8(src[(size_t)i], s->img + 3 * pix[(size_t)i], 1, list->height[i], list->width[i], rh, rw, (rh - h) / 2,
                                         (rw - w) / 2, h, w, st));
        }
        for (PassRun& r : runs) r.img = s->img + 3 * pix[(size_t)r.image0];
    } else {
        for (PassRun& r : runs) {
            const int i0 = r.image0, i1 = i0 + r.B;
            const size_t fl = 3 * (size_t)r.h * r.w;  // floats of one image of the run
            bool in_place = list->on_device != 0;
            for (int i = i0 + 1; i < i1 && in_place; ++i)
                in_place = static_cast<const float*>(list->data[i]) == static_cast<const float*>(list->data[i - 1]) + fl;
            if (in_place) {
                r.img = static_cast<const float*>(list->data[i0]);
                continue;
            }
            for (int i = i0; i < i1; ++i)
                HIP_TRY(hipMemcpyAsync(s->img + 3 * pix[(size_t)i], list->data[i], sizeof(float) * fl,
                                       list->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
            r.img = s->img + 3 * pix[(size_t)i0];
        }
    }
    std::vector<const float*> pos_of;
    rc = prepare_pos_list(s, im, pos_of, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    for (PassRun& r : runs) r.pos = pos_of[(size_t)r.image0];
    rc = prepare_items_list(s, items, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const Pass pass{runs.data(), lp.nruns, (int)lp.M, s->scratch[SCRATCH_LIST_ITEMS].as<AttnItem>(), (int)items.size(), layout, classify,
                    (int)m->hp.num_hidden_layers, true, PassExtras{}};
    rc = forward(s, pass, err, errlen);
    if (rc != DINOV2_HIP_OK || !out) return rc;
    return copy_out(s, runs.data(), lp.nruns, classify, out, err, errlen);
}

extern "C" int dinov2_hip_fetch(dinov2_hip_session* s, dinov2_hip_output* out, char* err, size_t errlen) {
    if (!s || !out) {
        set_err(err, errlen, "null session / output");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (s->last_b <= 0) {
        set_err(err, errlen, "no forward to fetch from (no predict yet, or the last one was split into passes: pass outputs to predict)");
        return DINOV2_HIP_ERR_INVALID;
    }
    const int rc = check_predict_args(s->model, out, 0, err, errlen);  // (no flags: only "top-k outputs are host-only" can fire)
    if (rc != DINOV2_HIP_OK) return rc;
    HIP_TRY(hipSetDevice(s->model->device));
    return fetch_outputs(s, out, err, errlen);
}

extern "C" int dinov2_hip_debug_hidden(dinov2_hip_session* s, const dinov2_hip_input* in, int32_t layer, float* out,
                                       char* err, size_t errlen) {
    int rc = check_input(s, in, 0, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const dinov2_hip_model* m = s->model;
    if (!out || layer < 0 || layer > (int)m->hp.num_hidden_layers) {
        set_err(err, errlen, "layer out of range");
        return DINOV2_HIP_ERR_INVALID;
    }
    if (in->layout == DINOV2_HIP_U8_BGR_HWC) {  // check_input accepts raw images of any size; this entry point has no preprocess step
        set_err(err, errlen, "debug_hidden takes preprocessed f32 images (BGR_HWC or RGB_CHW), not raw 8-bit input");
        return DINOV2_HIP_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(m->device));
    s->last_b = 0;  // this call overwrites the workspace: the previous predict's results are gone for dinov2_hip_fetch
    const int B = in->batch, h = in->height, w = in->width;
    rc = ensure_workspace(s, B, h, w, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const float* img = nullptr;
    rc = images_f32(s, in, &img, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    rc = prepare_pos(s, B, h, w, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const PassRun run = uniform_run(m, img, B, h, w, s->pos);
    const Pass pass{&run, 1, B * run.T, nullptr, 0, in->layout, false, layer, false, PassExtras{}};
    rc = forward(s, pass, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, s->x, sizeof(float) * (size_t)pass.M * m->hp.hidden_size, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return DINOV2_HIP_OK;
}

// For the entry points outside this file that launch kernels of their own (slide.cpp): an event pair around them, booked under the kind of
// that name in dinov2_hip_session_profile.  Nothing happens while the session is not profiling.
dinov2::ProfileMark::ProfileMark(dinov2_hip_session* s, const char* kind) {
    int k = 0;
    while (k < K_COUNT && strcmp(kKindNames[k], kind) != 0) ++k;
    if (k < K_COUNT) scope = new Scope(s, k);
}
dinov2::ProfileMark::~ProfileMark() { delete static_cast<Scope*>(scope); }
