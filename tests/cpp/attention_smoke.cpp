// C++ caller of dino_get_attention (include/dinov2_compat.hpp): load -> synthetic preprocessed image -> the CLS rows of every block and a
// patch-only view of the last one.  Every row sums to 1, and the patch-only view is columns 1 + R .. of the full one, bit for bit.
// Usage: attention_smoke model.gguf
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dinov2_compat.hpp"

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s model.gguf\n", argv[0]);
        return 2;
    }
    dino_params params;
    params.model = argv[1];
    dino_model model;
    if (!dino_model_load(Size2i{70, 70}, params.model, model, params)) return 1;
    const int Hi = 70, Wi = 84, L = (int)model.hparams.num_hidden_layers, R = (int)model.hparams.num_register_tokens;
    std::vector<float> pix((size_t)Hi * Wi * 3);
    unsigned s = 42;
    for (auto& p : pix) {
        s = s * 1664525u + 1013904223u;
        p = ((float)(s >> 8) / 8388608.0f) - 1.0f;
    }
    Mat32f img;
    img.rows = Hi; img.cols = Wi; img.channels = 3; img.data = pix.data();
    if (!dino_get_attention(model, img, {0}).empty()) {  // there is no attention before block 1: refused, message on stderr
        fprintf(stderr, "layer 0 was accepted\n");
        return 1;
    }
    std::vector<int> all;
    for (int k = 1; k <= L; ++k) all.push_back(k);
    auto cls = dino_get_attention(model, img, all);
    auto two = dino_get_attention(model, img, {L}, {0, 1 + R}, true);
    auto full = dino_get_attention(model, img, {L}, {0, 1 + R});
    if ((int)cls.size() != L || two.size() != 1 || full.size() != 1) return 1;
    for (const auto& a : cls)
        for (int h = 0; h < a.heads; ++h) {
            double sum = 0;
            for (int j = 0; j < a.keys; ++j) sum += a.row(h, 0)[j];
            if (!(std::fabs(sum - 1.0) <= a.keys * std::ldexp(1.0, -23))) {
                fprintf(stderr, "layer %d head %d: CLS row sums to %.9f\n", a.layer, h, sum);
                return 1;
            }
        }
    const auto &p = two[0], &f = full[0];
    if (p.keys != p.grid_h * p.grid_w || f.keys != 1 + R + p.keys) return 1;
    for (int h = 0; h < p.heads; ++h)
        for (int q = 0; q < 2; ++q)
            if (std::memcmp(p.row(h, q), f.row(h, q) + 1 + R, sizeof(float) * (size_t)p.keys) != 0) {
                fprintf(stderr, "the patch-only view is not a slice of the full one (head %d query %d)\n", h, q);
                return 1;
            }
    if (std::memcmp(cls[(size_t)L - 1].row(0, 0), f.row(0, 0), sizeof(float) * (size_t)f.keys) != 0) {
        fprintf(stderr, "the CLS row asked alone differs from the one asked with a patch\n");
        return 1;
    }
    printf("attention: %zu layers, heads %d, keys %d; last layer patches only: %d queries x %d keys, grid %d x %d\n", cls.size(), cls[0].heads,
           cls[0].keys, p.queries, p.keys, p.grid_h, p.grid_w);
    return 0;
}
