// csrc/ops_frame.h under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_ops_frame.py): the guard-band check of the diagnostic
// ops' device harness on exactly sized heap buffers, and the f16 / bf16 widening of all 65 536 bit patterns against a decode written here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dinov2.cpp_amd/csrc/ops_frame.h"

using namespace dinov2;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::fprintf(stderr, "FAILED %s: ", #cond);   \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, "\n");                   \
            return 1;                                     \
        }                                                 \
    } while (0)

// [ng | n | ng] elements of esz bytes: an untouched frame hands back the payload; one flipped bit in the first or the last byte of either band
// is "changed" and leaves the destination alone.  edge: the first and the last payload byte.
static int check_frame(size_t n, size_t ng, size_t esz, unsigned char edge) {
    const size_t nb = n * esz, gb = ng * esz;
    std::vector<unsigned char> raw(2 * gb + nb, 0xff), want(nb), got(nb, 0x5a);
    for (size_t i = 0; i < nb; ++i) want[i] = (unsigned char)(i * 131u + 7u);
    if (nb) want[0] = want[nb - 1] = edge;
    if (nb) std::memcpy(raw.data() + gb, want.data(), nb);
    CHECK(frame_payload(raw.data(), n, ng, esz, got.data()), "n=%zu ng=%zu esz=%zu: an untouched frame reads as changed", n, ng, esz);
    CHECK(got == want, "n=%zu ng=%zu esz=%zu: payload differs", n, ng, esz);
    CHECK(frame_intact(raw.data(), n, ng, esz), "n=%zu ng=%zu esz=%zu: frame_intact disagrees with frame_payload", n, ng, esz);
    if (!gb) return 0;
    const size_t at[4] = {0, gb - 1, gb + nb, 2 * gb + nb - 1};
    for (int c = 0; c < 4; ++c)
        for (int bit = 0; bit < 8; bit += 7) {
            std::vector<unsigned char> bad(raw), dst(nb, 0x5a);
            bad[at[c]] ^= (unsigned char)(1u << bit);
            CHECK(!frame_intact(bad.data(), n, ng, esz), "n=%zu ng=%zu esz=%zu: byte %zu changed, frame_intact did not notice", n, ng, esz, at[c]);
            CHECK(!frame_payload(bad.data(), n, ng, esz, dst.data()), "n=%zu ng=%zu esz=%zu: byte %zu changed, not noticed", n, ng, esz, at[c]);
            CHECK(dst == std::vector<unsigned char>(nb, 0x5a), "n=%zu ng=%zu esz=%zu: payload copied out of a changed frame", n, ng, esz);
        }
    return 0;
}

// the value of a sign / exponent / mantissa pattern with `mb` mantissa bits, `eb` exponent bits, from its definition
static float decode(uint16_t h, int eb, int mb) {
    const int bias = (1 << (eb - 1)) - 1, emax = (1 << eb) - 1;
    const int e = (h >> mb) & emax, m = h & ((1 << mb) - 1);
    float v;
    if (e == emax) v = m ? NAN : INFINITY;
    else if (e == 0) v = std::ldexp((float)m, 1 - bias - mb);
    else v = std::ldexp((float)((1 << mb) + m), e - bias - mb);
    return (h & 0x8000u) ? -v : v;
}

static int check_widen(bool bf16) {
    const size_t N = 65536;
    std::vector<unsigned char> src(2 * N + 1);  // the values start at an odd address
    for (size_t i = 0; i < N; ++i) {
        const uint16_t h = (uint16_t)i;
        std::memcpy(src.data() + 1 + 2 * i, &h, 2);
    }
    std::vector<float> got(N);
    widen_to_f32(bf16, src.data() + 1, N, got.data());
    for (size_t i = 0; i < N; ++i) {
        const float want = bf16 ? decode((uint16_t)i, 8, 7) : decode((uint16_t)i, 5, 10);
        if (std::isnan(want)) {
            CHECK(std::isnan(got[i]), "%s 0x%04zx: a NaN came out as %g", bf16 ? "bf16" : "f16", i, (double)got[i]);
            continue;
        }
        CHECK(std::memcmp(&got[i], &want, 4) == 0, "%s 0x%04zx: %a, expected %a", bf16 ? "bf16" : "f16", i, (double)got[i], (double)want);
    }
    widen_to_f32(bf16, nullptr, 0, nullptr);
    return 0;
}

int main() {
    int frames = 0;
    for (size_t esz : {1, 2, 4, 8})
        for (size_t n : {0, 1, 7, 4096})
            for (size_t ng : {0, 3, 5, 128 * 1, 128 * 37})
                for (unsigned edge : {0xffu, 0x00u, 0x7fu}) {
                    if (check_frame(n, ng, esz, (unsigned char)edge)) return 1;
                    ++frames;
                }
    if (check_widen(false) || check_widen(true)) return 1;
    std::printf("ops_frame: %d frames, 2 x 65536 values OK\n", frames);
    return 0;
}
