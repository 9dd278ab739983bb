// The two pure pieces of the diagnostic ops' device harness (csrc/ops_testing.cpp): the guard-band check of a framed output and the
// widening of two-byte values to f32.  Host-only and free of HIP, so that a plain C++ compiler builds it (tests/cpp/ops_frame_san.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace dinov2 {

// raw: the bytes of a device buffer of [ng | n | ng] elements of esz bytes that started as 0xff bytes everywhere outside the payload.
// frame_intact: both bands are still all 0xff bytes.
inline bool frame_intact(const unsigned char* raw, size_t n, size_t ng, size_t esz) {
    const unsigned char* back = raw + (ng + n) * esz;
    for (size_t k = 0; k < ng * esz; ++k)
        if (raw[k] != 0xffu || back[k] != 0xffu) return false;
    return true;
}
// frame_payload: an intact frame's payload (n * esz bytes) copied to `payload`, true; false otherwise, `payload` untouched.
inline bool frame_payload(const unsigned char* raw, size_t n, size_t ng, size_t esz, void* payload) {
    if (!frame_intact(raw, n, ng, esz)) return false;
    if (n) std::memcpy(payload, raw + ng * esz, n * esz);
    return true;
}

// One IEEE binary16 value; a signalling NaN comes out quiet, as from a hardware conversion.
inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    uint32_t u;
    if (exp == 0x1fu) {
        u = 0x7f800000u | (man ? 0x00400000u | (man << 13) : 0u);
    } else if (exp) {
        u = ((exp + 112u) << 23) | (man << 13);
    } else {
        const float f = (float)man * 0x1p-24f;  // zero and the subnormals: exact
        std::memcpy(&u, &f, 4);
    }
    u |= sign;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

inline float bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// n two-byte values at `src` (any alignment) to f32: bf16 if `bf16`, f16 otherwise
inline void widen_to_f32(bool bf16, const void* src, size_t n, float* dst) {
    const unsigned char* s = (const unsigned char*)src;
    for (size_t i = 0; i < n; ++i) {
        uint16_t h;
        std::memcpy(&h, s + 2 * i, 2);
        dst[i] = bf16 ? bf16_to_f32(h) : f16_to_f32(h);
    }
}

}  // namespace dinov2
