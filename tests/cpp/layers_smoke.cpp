// C++ caller of dino_get_intermediate_layers (include/dinov2_compat.hpp): load -> synthetic preprocessed image -> the last layer normalised,
// as rows and reshaped, next to dino_predict.  The last layer through the final LayerNorm IS dino_predict's patch_tokens, bit for bit, and
// the reshaped form is its transpose.  Usage: layers_smoke model.gguf
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
    const int Hi = 70, Wi = 84, L = (int)model.hparams.num_hidden_layers;
    std::vector<float> pix((size_t)Hi * Wi * 3);
    unsigned s = 42;
    for (auto& p : pix) {
        s = s * 1664525u + 1013904223u;
        p = ((float)(s >> 8) / 8388608.0f) - 1.0f;
    }
    Mat32f img;
    img.rows = Hi; img.cols = Wi; img.channels = 3; img.data = pix.data();
    std::unique_ptr<dino_output> ref = dino_predict(model, img, params);
    if (!ref) return 1;
    if (!dino_get_intermediate_layers(model, img, {L, 1}).empty()) {  // not ascending: refused, message on stderr
        fprintf(stderr, "a descending layer list was accepted\n");
        return 1;
    }
    auto rows = dino_get_intermediate_layers(model, img, {1, L}, true, false, true);
    auto chw = dino_get_intermediate_layers(model, img, {1, L}, true, true);
    if (rows.size() != 2 || chw.size() != 2) return 1;
    const Mat32f &a = rows[1].patch_tokens, &c = chw[1].patch_tokens, &r = *ref->patch_tokens;
    if (a.rows != r.rows || a.cols != r.cols || c.rows != r.cols || c.cols != r.rows) return 1;
    if (std::memcmp(a.data, r.data, sizeof(float) * (size_t)a.rows * a.cols) != 0) {
        fprintf(stderr, "layer L differs from dino_predict\n");
        return 1;
    }
    for (int p = 0; p < a.rows; ++p)
        for (int h = 0; h < a.cols; ++h)
            if (std::memcmp(&c.data[(size_t)h * c.cols + p], &a.data[(size_t)p * a.cols + h], sizeof(float)) != 0) {
                fprintf(stderr, "reshape is not the transpose at (%d, %d)\n", p, h);
                return 1;
            }
    printf("layers: %zu, layer %d patch_tokens: %d x %d, grid %d x %d, cls: %zu, reshaped: %d x %d\n", rows.size(), rows[1].layer, a.rows, a.cols,
           rows[1].grid_h, rows[1].grid_w, rows[1].cls.size(), c.rows, c.cols);
    return 0;
}
