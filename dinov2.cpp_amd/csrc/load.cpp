// load.cpp -- the GGUF loader and what belongs to a model rather than a session: the arena, the pos-embed resampler, page-locked host memory.
//
// Replaces, from the reference (lavaman131/dinov2.cpp):
//   dino_model_load        /root/reference/dinov2.cpp:239-352   -> dinov2_hip_model_load
//   interpolate_pos_embed  /root/reference/dinov2.cpp:159-225   -> interpolate_pos_embed() below (no OpenCV)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "gguf_reader.h"
#include "host.h"

using namespace dinov2;

namespace {

// ---- cv::resize(INTER_CUBIC) for CV_32F, restated without OpenCV: separable cubic convolution, A = -0.75,
// source coordinate (d + 0.5) * (src/dst) - 0.5, four taps floor-1..floor+2 clamped to the border, no antialias.
void cubic_taps(float t, float w[4]) {
    const float A = -0.75f;
    w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * (1.f - t) - (A + 3.f)) * (1.f - t) * (1.f - t) + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}

struct Axis {
    std::vector<int> idx;    // 4 per destination coordinate
    std::vector<float> wgt;  // 4 per destination coordinate
};

Axis make_axis(int src, int dst) {
    Axis a;
    a.idx.resize(4 * (size_t)dst);
    a.wgt.resize(4 * (size_t)dst);
    const float scale = (float)src / (float)dst;
    for (int d = 0; d < dst; ++d) {
        float f = ((float)d + 0.5f) * scale - 0.5f;
        const int s = (int)std::floor(f);
        f -= (float)s;
        cubic_taps(f, &a.wgt[4 * (size_t)d]);
        for (int k = 0; k < 4; ++k) a.idx[4 * (size_t)d + k] = std::min(std::max(s - 1 + k, 0), src - 1);
    }
    return a;
}

}  // namespace

// interpolate_pos_embed (dinov2.cpp:159-225).  pos: [1 + M*M, H]; out: [1 + h*w, H].  Identity when the patch
// COUNT matches (the reference compares counts, not shapes: dinov2.cpp:176-179).
void dinov2::interpolate_pos_embed(const float* pos, int M, int H, int h_new, int w_new, float* out) {
    std::memcpy(out, pos, sizeof(float) * (size_t)H);
    if (h_new * w_new == M * M) {
        std::memcpy(out + H, pos + H, sizeof(float) * (size_t)M * M * H);
        return;
    }
    const Axis ax = make_axis(M, w_new), ay = make_axis(M, h_new);
    std::vector<float> rowbuf((size_t)4 * H);
    for (int dy = 0; dy < h_new; ++dy) {
        const int* iy = &ay.idx[4 * (size_t)dy];
        const float* wy = &ay.wgt[4 * (size_t)dy];
        for (int dx = 0; dx < w_new; ++dx) {
            const int* ix = &ax.idx[4 * (size_t)dx];
            const float* wx = &ax.wgt[4 * (size_t)dx];
            float* o = out + (size_t)(1 + dy * w_new + dx) * H;
            for (int ky = 0; ky < 4; ++ky) {  // horizontal pass per source row, then vertical blend
                float* rb = &rowbuf[(size_t)ky * H];
                const float* r0 = pos + (size_t)(1 + iy[ky] * M + ix[0]) * H;
                const float* r1 = pos + (size_t)(1 + iy[ky] * M + ix[1]) * H;
                const float* r2 = pos + (size_t)(1 + iy[ky] * M + ix[2]) * H;
                const float* r3 = pos + (size_t)(1 + iy[ky] * M + ix[3]) * H;
                for (int c = 0; c < H; ++c) rb[c] = r0[c] * wx[0] + r1[c] * wx[1] + r2[c] * wx[2] + r3[c] * wx[3];
            }
            for (int c = 0; c < H; ++c)
                o[c] = rowbuf[c] * wy[0] + rowbuf[(size_t)H + c] * wy[1] + rowbuf[(size_t)2 * H + c] * wy[2] +
                       rowbuf[(size_t)3 * H + c] * wy[3];
        }
    }
}

namespace {

// ---- arena planning --------------------------------------------------------------------------------------
struct Plan {
    struct Item {
        std::string name;   // GGUF tensor name
        void** slot;        // where the device pointer goes
        bool matrix;        // 2-D weight converted to the compute dtype, else f32 vector copied as is
        int N, K, Kpad;     // matrix dims (rows, cols, padded cols)
        int interleaveF;    // SwiGLU weights_in row interleave (0 = off)
        size_t offset, bytes;
        bool derived;       // no GGUF tensor behind it: computed on the device after the upload (LN-fold vectors)
    };
    std::vector<Item> items;
    size_t total = 0;
    void add(const std::string& name, void** slot, bool matrix, int N, int K, int Kpad, int F, size_t bytes) {
        Item it{name, slot, matrix, N, K, Kpad, F, total, bytes, false};
        total += align_up(bytes, 256);
        items.push_back(it);
    }
    void add_derived(const std::string& name, float** slot, int count) {
        Item it{name, (void**)slot, false, count, 1, 1, 0, total, sizeof(float) * (size_t)count, true};
        total += align_up(it.bytes, 256);
        items.push_back(it);
    }
};

// dinov2_hip_load_opts.ln_fold == 0: what the library picks (profiles/r06_ln_fold.md)
constexpr bool kLnFoldDefault = false;

}  // namespace

extern "C" void dinov2_hip_default_load_opts(dinov2_hip_load_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->device = 0;
    o->compute_dtype = DINOV2_HIP_F16;
    o->classify = 1;
    o->skip_tensor_data = 0;
    o->quirk_pool_const_divisor = 1;
    o->quirk_pool_includes_registers = 1;
    o->batch_invariant = 1;
    o->ln_fold = 0;
    o->patch_stride = 0;
}

extern "C" int dinov2_hip_abi_version(void) { return DINOV2_HIP_ABI_VERSION; }

extern "C" void* dinov2_hip_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

extern "C" void dinov2_hip_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

extern "C" int dinov2_hip_model_load(const char* path, const dinov2_hip_load_opts* opts_in, dinov2_hip_model** out,
                                     char* err, size_t errlen) {
    if (!path || !out) {
        set_err(err, errlen, "null argument");
        return DINOV2_HIP_ERR_INVALID;
    }
    *out = nullptr;
    dinov2_hip_load_opts opts;
    if (opts_in) opts = *opts_in; else dinov2_hip_default_load_opts(&opts);
    if (opts.compute_dtype != DINOV2_HIP_F16 && opts.compute_dtype != DINOV2_HIP_BF16) {
        set_err(err, errlen, "compute_dtype must be F16 or BF16");
        return DINOV2_HIP_ERR_INVALID;
    }

    GgufFile gg;
    std::string msg;
    if (!gg.open(path, &msg)) {
        set_err(err, errlen, "%s", msg.c_str());
        const bool io = msg.rfind("failed to open", 0) == 0 || msg.rfind("mmap", 0) == 0;
        return io ? DINOV2_HIP_ERR_IO : DINOV2_HIP_ERR_FORMAT;
    }

    std::unique_ptr<dinov2_hip_model> m(new dinov2_hip_model());
    auto& hp = m->hp;
    // hparams: u32 KVs, every one required (the reference asserts on a missing key, dinov2.cpp:58)
    struct { const char* key; uint32_t* dst; bool required; } keys[] = {
        {"hidden_size", &hp.hidden_size, true},           {"num_hidden_layers", &hp.num_hidden_layers, true},
        {"num_attention_heads", &hp.num_attention_heads, true}, {"patch_size", &hp.patch_size, true},
        {"img_size", &hp.img_size, true},                 {"ftype", &hp.ftype, true},
        {"num_register_tokens", &hp.num_register_tokens, false}, {"num_classes", &hp.num_classes, false}};
    for (auto& k : keys) {
        *k.dst = 0;
        if (!gg.get_u32(k.key, k.dst) && k.required) {
            set_err(err, errlen, "GGUF key '%s' is missing", k.key);
            return DINOV2_HIP_ERR_FORMAT;
        }
    }
    hp.eps = 1e-6f;
    hp.compute_dtype = (uint32_t)opts.compute_dtype;
    m->dt = opts.compute_dtype == DINOV2_HIP_BF16 ? DT_BF16 : DT_F16;
    m->device = opts.device;
    m->quirk_const_div = opts.quirk_pool_const_divisor != 0;
    m->quirk_pool_regs = opts.quirk_pool_includes_registers != 0;
    {
        // LN fold: on request (ln_fold = 1, or DINOV2_HIP_LN_FOLD=1 while the option says "library's choice"), where the model allows it.
        // The library's own choice is in kLnFoldDefault.
        int want = opts.ln_fold;
        if (want == 0)
            if (const char* e = getenv("DINOV2_HIP_LN_FOLD")) want = atoi(e) != 0 ? 1 : -1;
        if (want == 0) want = kLnFoldDefault ? 1 : -1;
        const int Hh = (int)hp.hidden_size;
        m->ln_fold = want > 0 && Hh % 128 == 0 && Hh / LN_GROUP <= LN_MAX_GROUPS;
    }

    const int H = (int)hp.hidden_size, L = (int)hp.num_hidden_layers, nh = (int)hp.num_attention_heads;
    const int ps = (int)hp.patch_size, R = (int)hp.num_register_tokens;
    if (H <= 0 || L <= 0 || nh <= 0 || ps <= 0 || hp.img_size < hp.patch_size) {
        set_err(err, errlen, "invalid hparams in '%s'", path);
        return DINOV2_HIP_ERR_FORMAT;
    }
    if (H != nh * 64) {
        set_err(err, errlen, "unsupported head dim %d (the DINOv2 family and this build use 64)", H / std::max(nh, 1));
        return DINOV2_HIP_ERR_UNSUPPORTED;
    }
    if (H % 64 != 0) {
        set_err(err, errlen, "hidden_size %d is not a multiple of 64", H);
        return DINOV2_HIP_ERR_UNSUPPORTED;
    }
    // what the kernels behind the forward take (kernels.h): refused here, by name, rather than by a launch of the first forward
    if (H > LN_MAX_WIDTH) {
        set_err(err, errlen, "unsupported hidden_size %d: the LayerNorm kernels take rows of up to %d (num_attention_heads <= %d)", H,
                LN_MAX_WIDTH, LN_MAX_WIDTH / 64);
        return DINOV2_HIP_ERR_UNSUPPORTED;
    }
    if (!im2col_patch_ok(ps, (int)align_up((size_t)3 * ps * ps, 64))) {
        set_err(err, errlen, "unsupported patch_size %d: the patch-embedding im2col takes patch sizes up to %d", ps, im2col_max_patch());
        return DINOV2_HIP_ERR_UNSUPPORTED;
    }
    {
        // patch_stride: 0 = the patch size.  A divisor of it keeps every multiple of the patch size a valid network size (so the preprocessing
        // needs no change) and lets the strided kernel think in stride x stride cells.
        const int st = opts.patch_stride == 0 ? ps : opts.patch_stride;
        if (st < 1 || st > ps || ps % st != 0) {
            set_err(err, errlen, "unsupported patch_stride %d: it must divide patch_size %d (0 = the patch size)", opts.patch_stride, ps);
            return DINOV2_HIP_ERR_UNSUPPORTED;
        }
        if (st != ps && !im2col_stride_ok(ps, st, (int)align_up((size_t)3 * ps * ps, 64))) {
            set_err(err, errlen, "unsupported patch_size %d with patch_stride %d: outside the limits of the strided im2col (im2col_stride_ok)", ps, st);
            return DINOV2_HIP_ERR_UNSUPPORTED;
        }
        m->patch_stride = st;
    }
    const int Mgrid = (int)(hp.img_size / hp.patch_size);

    auto need = [&](const std::string& name, const GgufTensor** t) -> bool {
        *t = gg.tensor(name);
        if (!*t) set_err(err, errlen, "GGUF tensor '%s' is missing", name.c_str());
        return *t != nullptr;
    };

    // FFN flavour: by tensor presence (equivalent to the reference's `num_hidden_layers == 40`, dinov2.cpp:740)
    const bool swiglu = gg.tensor("encoder.layer.0.mlp.weights_in.weight") != nullptr;
    hp.swiglu = swiglu;
    const GgufTensor* t = nullptr;
    if (!need(swiglu ? "encoder.layer.0.mlp.weights_out.weight" : "encoder.layer.0.mlp.fc1.weight", &t))
        return DINOV2_HIP_ERR_FORMAT;
    if (t->ne.size() < 2) {
        set_err(err, errlen, "tensor '%s' is not 2-D", t->name.c_str());
        return DINOV2_HIP_ERR_FORMAT;
    }
    const int F = swiglu ? (int)t->ne[0] : (int)t->ne[1];
    hp.ffn_hidden = (uint32_t)F;
    if (F % 64 != 0) {
        set_err(err, errlen, "FFN hidden size %d is not a multiple of 64", F);
        return DINOV2_HIP_ERR_UNSUPPORTED;
    }
    if (!need("encoder.layer.0.attention.attention.qkv.weight", &t)) return DINOV2_HIP_ERR_FORMAT;
    hp.weight_type = t->type;

    const GgufTensor* head = gg.tensor("classifier.weight");
    const bool want_head = opts.classify != 0 && head != nullptr;
    hp.has_classifier = want_head;
    int C = 0;
    if (want_head) {
        C = (int)(head->ne.size() >= 2 ? head->ne[1] : 0);
        if (C <= 0 || (int)head->ne[0] != 2 * H) {
            set_err(err, errlen, "classifier.weight has unexpected shape");
            return DINOV2_HIP_ERR_FORMAT;
        }
        hp.num_classes = (uint32_t)C;
        m->labels.resize((size_t)C);
        for (int i = 0; i < C; ++i) {  // id2label string KVs "0".."C-1" (dinov2.cpp:301-305)
            const GgufValue* v = gg.find(std::to_string(i));
            m->labels[(size_t)i] = v ? v->s : std::string();
        }
    }

    // ---- plan the arena ----
    const size_t esz = 2;
    m->kpe = 3 * ps * ps;
    m->kpe_pad = (int)align_up((size_t)m->kpe, 64);
    m->layers.resize((size_t)L);
    Plan plan;
    auto vec = [&](const std::string& n, float** slot, int count, int F_il = 0) {
        plan.add(n, (void**)slot, false, count, 1, 1, F_il, sizeof(float) * (size_t)count);
    };
    auto mat = [&](const std::string& n, void** slot, int N, int K, int Kpad, int F_il = 0) {
        plan.add(n, slot, true, N, K, Kpad, F_il, esz * (size_t)N * Kpad);
    };
    vec("embeddings.cls_token", &m->cls, H);
    vec("embeddings.position_embeddings", &m->pos, (1 + Mgrid * Mgrid) * H);
    if (R > 0) vec("embeddings.register_tokens", &m->reg, R * H);
    mat("embeddings.patch_embeddings.projection.weight", &m->patch_w, H, m->kpe, m->kpe_pad);
    vec("embeddings.patch_embeddings.projection.bias", &m->patch_b, H);
    for (int i = 0; i < L; ++i) {
        const std::string b = "encoder.layer." + std::to_string(i) + ".";
        LayerWeights& ly = m->layers[(size_t)i];
        vec(b + "norm1.weight", &ly.norm1_w, H);
        vec(b + "norm1.bias", &ly.norm1_b, H);
        mat(b + "attention.attention.qkv.weight", &ly.qkv_w, 3 * H, H, H);
        vec(b + "attention.attention.qkv.bias", &ly.qkv_b, 3 * H);
        mat(b + "attention.output.dense.weight", &ly.o_w, H, H, H);
        vec(b + "attention.output.dense.bias", &ly.o_b, H);
        vec(b + "layer_scale1.lambda1", &ly.ls1, H);
        vec(b + "norm2.weight", &ly.norm2_w, H);
        vec(b + "norm2.bias", &ly.norm2_b, H);
        if (swiglu) {
            mat(b + "mlp.weights_in.weight", &ly.fc1_w, 2 * F, H, H, F);
            vec(b + "mlp.weights_in.bias", &ly.fc1_b, 2 * F, F);
            mat(b + "mlp.weights_out.weight", &ly.fc2_w, H, F, F);
            vec(b + "mlp.weights_out.bias", &ly.fc2_b, H);
        } else {
            mat(b + "mlp.fc1.weight", &ly.fc1_w, F, H, H);
            vec(b + "mlp.fc1.bias", &ly.fc1_b, F);
            mat(b + "mlp.fc2.weight", &ly.fc2_w, H, F, F);
            vec(b + "mlp.fc2.bias", &ly.fc2_b, H);
        }
        vec(b + "layer_scale2.lambda1", &ly.ls2, H);
        if (m->ln_fold) {
            const int nfc1 = swiglu ? 2 * F : F;
            plan.add_derived(b + "ln_fold.qkv_s", &ly.qkv_s, 3 * H);
            plan.add_derived(b + "ln_fold.qkv_c", &ly.qkv_c, 3 * H);
            plan.add_derived(b + "ln_fold.fc1_s", &ly.fc1_s, nfc1);
            plan.add_derived(b + "ln_fold.fc1_c", &ly.fc1_c, nfc1);
        }
    }
    vec("layernorm.weight", &m->ln_w, H);
    vec("layernorm.bias", &m->ln_b, H);
    if (want_head) {
        mat("classifier.weight", &m->head_w, C, 2 * H, 2 * H);
        vec("classifier.bias", &m->head_b, C);
    }

    // validate every tensor against the plan before touching the device
    size_t max_raw = 0;
    for (auto& it : plan.items) {
        if (it.derived) continue;
        const GgufTensor* gt = nullptr;
        if (!need(it.name, &gt)) return DINOV2_HIP_ERR_FORMAT;
        const uint64_t want = it.matrix ? (uint64_t)it.N * it.K : (uint64_t)it.N;
        if (gt->nelements() != want) {
            set_err(err, errlen, "tensor '%s' has %llu elements, expected %llu", it.name.c_str(),
                    (unsigned long long)gt->nelements(), (unsigned long long)want);
            return DINOV2_HIP_ERR_FORMAT;
        }
        if (it.matrix && (int)gt->ne[0] != it.K && it.name.find("patch_embeddings") == std::string::npos) {
            set_err(err, errlen, "tensor '%s' has row length %llu, expected %d", it.name.c_str(),
                    (unsigned long long)gt->ne[0], it.K);
            return DINOV2_HIP_ERR_FORMAT;
        }
        if (!it.matrix && gt->type != GGML_F32) {
            set_err(err, errlen, "tensor '%s' must be F32 (the converter writes 1-D / embedding tensors as F32)",
                    it.name.c_str());
            return DINOV2_HIP_ERR_UNSUPPORTED;
        }
        if (it.matrix && it.name.find("patch_embeddings") != std::string::npos && gt->type != GGML_F16 &&
            gt->type != GGML_F32 && gt->type != GGML_BF16) {
            set_err(err, errlen, "patch-embedding kernel must be F16/F32/BF16");
            return DINOV2_HIP_ERR_UNSUPPORTED;
        }
        max_raw = std::max(max_raw, (size_t)gt->nbytes);
    }

    // ---- device side ----
    HIP_TRY(hipSetDevice(opts.device));
    HIP_TRY(gemm_init());
    m->arena_bytes = plan.total;
    HIP_TRY(hipMalloc((void**)&m->arena, plan.total));
    // every early return below (HIP_TRY included) must give the arena back: the model struct has no destructor of its own
    struct ArenaGuard {
        dinov2_hip_model* m;
        ~ArenaGuard() {
            if (m && m->arena) {
                (void)hipFree(m->arena);
                m->arena = nullptr;
            }
        }
    } arena_guard{m.get()};
    for (auto& it : plan.items) *it.slot = m->arena + it.offset;

    // host copy of the position embeddings for per-resolution interpolation
    {
        const GgufTensor* pt = gg.tensor("embeddings.position_embeddings");
        m->pos_host.assign((const float*)pt->data, (const float*)pt->data + pt->nelements());
    }

    if (!opts.skip_tensor_data) {
        char* staging = nullptr;
        HIP_TRY(hipMalloc((void**)&staging, align_up(max_raw, 256)));
        int rc = DINOV2_HIP_OK;
        for (auto& it : plan.items) {
            if (it.derived) continue;
            const GgufTensor* gt = gg.tensor(it.name);
            hipError_t e = hipSuccess;
            if (!it.matrix && it.interleaveF == 0) {
                e = hipMemcpy(*it.slot, gt->data, gt->nbytes, hipMemcpyHostToDevice);
            } else {
                e = hipMemcpy(staging, gt->data, gt->nbytes, hipMemcpyHostToDevice);
                if (e == hipSuccess) {
                    if (it.matrix)
                        e = launch_convert_weight(m->dt, staging, gt->type, *it.slot, it.N, it.K, it.Kpad, it.interleaveF,
                                                  nullptr);
                    else
                        e = launch_permute_bias((const float*)staging, (float*)*it.slot, it.N, it.interleaveF, nullptr);
                }
                if (e == hipSuccess) e = hipDeviceSynchronize();  // staging is reused by the next tensor
            }
            if (e != hipSuccess) {
                set_err(err, errlen, "uploading '%s' failed: %s", it.name.c_str(), hipGetErrorString(e));
                rc = DINOV2_HIP_ERR_HIP;
                break;
            }
        }
        (void)hipFree(staging);
        if (rc != DINOV2_HIP_OK) return rc;
        if (m->ln_fold) {  // s / c of the QKV and FFN-in weights under the LayerNorm in front of them, from the converted weights
            for (int i = 0; i < L; ++i) {
                const LayerWeights& ly = m->layers[(size_t)i];
                HIP_TRY(launch_ln_fold_vectors(m->dt, ly.qkv_w, ly.qkv_b, ly.norm1_w, ly.norm1_b, ly.qkv_s, ly.qkv_c, 3 * H, H, nullptr));
                HIP_TRY(launch_ln_fold_vectors(m->dt, ly.fc1_w, ly.fc1_b, ly.norm2_w, ly.norm2_b, ly.fc1_s, ly.fc1_c, swiglu ? 2 * F : F, H, nullptr));
            }
            HIP_TRY(hipDeviceSynchronize());
        }
    }
    arena_guard.m = nullptr;  // success: the arena now belongs to the model (dinov2_hip_model_free)
    *out = m.release();
    return DINOV2_HIP_OK;
}

extern "C" void dinov2_hip_model_free(dinov2_hip_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->arena) (void)hipFree(m->arena);
    delete m;
}

extern "C" int dinov2_hip_model_hparams(const dinov2_hip_model* m, dinov2_hip_hparams* out) {
    if (!m || !out) return DINOV2_HIP_ERR_INVALID;
    *out = m->hp;
    return DINOV2_HIP_OK;
}

// ---- what one pass of the forward takes of ONE image (model.h: dinov2_check_pass_rows) ----
size_t dinov2::widest_row(const dinov2_hip_model* m) {
    return std::max<size_t>({3 * (size_t)m->hp.hidden_size, (size_t)m->hp.ffn_hidden, (size_t)m->kpe_pad});
}

int dinov2::check_rows_at(const dinov2_hip_model* m, int h, int w, char* err, size_t errlen) {
    const Grid g = grid_of(m, h, w);
    const int64_t T = 1 + (int64_t)m->hp.num_register_tokens + (int64_t)g.h0 * g.w0, widest = (int64_t)widest_row(m);
    if (T * widest * 2 >= ((int64_t)1 << 31)) {
        set_err(err, errlen, "an image of %d x %d has too many token rows for one pass (%lld at patch_size %d, patch_stride %d; rows * %lld * 2 must "
                "stay below 2^31, the 32-bit activation offsets of dinov2_hip_predict's passes).  An image is refused, not split",
                h, w, (long long)T, (int)m->hp.patch_size, m->patch_stride, (long long)widest);
        return DINOV2_HIP_ERR_INVALID;
    }
    return DINOV2_HIP_OK;
}

// dinov2_check_input, then raw 8-bit input against the grid at its network size: the classify preprocessing crops to 224 x 224 whatever the
// patch size, and a size the model's grid does not hold is refused as the same size handed over as floats is
int dinov2_check_input_grid(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen) {
    const int rc = dinov2_check_input(m, in, err, errlen);
    if (rc != DINOV2_HIP_OK || in->layout != DINOV2_HIP_U8_BGR_HWC) return rc;
    const int ps = (int)m->hp.patch_size, st = m->patch_stride;
    int h, w;
    network_size(m, in, flags, &h, &w);
    if (h < ps || w < ps || (h - ps) % st || (w - ps) % st) {
        set_err(err, errlen, "raw image input is preprocessed to %d x %d, which is not patch_size %d plus a multiple of patch_stride %d (the classify "
                "preprocessing crops to 224 x 224 whatever the patch size)", h, w, ps, st);
        return DINOV2_HIP_ERR_INVALID;
    }
    return DINOV2_HIP_OK;
}

int dinov2_check_pass_rows(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen) {
    int h, w;
    network_size(m, in, flags, &h, &w);
    return check_rows_at(m, h, w, err, errlen);
}

int dinov2_check_input_rows(const dinov2_hip_model* m, const dinov2_hip_input* in, uint32_t flags, char* err, size_t errlen) {
    const int rc = dinov2_check_input_grid(m, in, flags, err, errlen);
    return rc != DINOV2_HIP_OK ? rc : dinov2_check_pass_rows(m, in, flags, err, errlen);
}

extern "C" int dinov2_hip_model_patch_stride(const dinov2_hip_model* m) { return m ? m->patch_stride : 0; }

extern "C" int dinov2_hip_model_grid(const dinov2_hip_model* m, int32_t h, int32_t w, int32_t* h0, int32_t* w0, char* err, size_t errlen) {
    if (!m || !h0 || !w0) {
        set_err(err, errlen, "null model / h0 / w0");
        return DINOV2_HIP_ERR_INVALID;
    }
    dinov2_hip_input in{};
    in.data = reinterpret_cast<const float*>(m);  // (never dereferenced: the checks below read the sizes only)
    in.batch = 1; in.height = h; in.width = w; in.layout = DINOV2_HIP_RGB_CHW;
    const int rc = dinov2_check_input_rows(m, &in, 0, err, errlen);
    if (rc != DINOV2_HIP_OK) return rc;
    const Grid g = grid_of(m, h, w);
    *h0 = g.h0;
    *w0 = g.w0;
    return DINOV2_HIP_OK;
}

extern "C" const char* dinov2_hip_model_label(const dinov2_hip_model* m, int32_t id) {
    if (!m || id < 0 || (size_t)id >= m->labels.size()) return nullptr;
    return m->labels[(size_t)id].c_str();
}

extern "C" int dinov2_hip_model_arena(dinov2_hip_model* m, void** ptr, size_t* bytes) {
    if (!m || !ptr || !bytes) return DINOV2_HIP_ERR_INVALID;
    *ptr = m->arena;
    *bytes = m->arena_bytes;
    return DINOV2_HIP_OK;
}

extern "C" int dinov2_hip_interpolate_pos_embed(const dinov2_hip_model* m, int32_t h_new, int32_t w_new, float* out) {
    if (!m || !out || h_new <= 0 || w_new <= 0) return DINOV2_HIP_ERR_INVALID;
    interpolate_pos_embed(m->pos_host.data(), (int)(m->hp.img_size / m->hp.patch_size), (int)m->hp.hidden_size, h_new,
                          w_new, out);
    return DINOV2_HIP_OK;
}

