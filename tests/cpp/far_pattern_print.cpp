// csrc/far_pattern.h through a plain C++ compiler: prints far_value_q for the (seed, row, col) triples given on the command line as
// "seed:row:col", one integer per line.  tests/test_far_probes.py compares them with the numpy restatement (tests/far_cases.py).
#include <cstdio>
#include <cstdlib>

#include "../../dinov2.cpp_amd/csrc/far_pattern.h"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        char* end = nullptr;
        const unsigned long long seed = std::strtoull(argv[i], &end, 10);
        if (*end != ':') return 2;
        const unsigned long long row = std::strtoull(end + 1, &end, 10);
        if (*end != ':') return 2;
        const unsigned long long col = std::strtoull(end + 1, &end, 10);
        if (*end != '\0') return 2;
        const int q = dinov2::far_value_q(seed, row, (uint32_t)col);
        if (dinov2::far_value(seed, row, (uint32_t)col) * 64.0f != (float)q) return 3;
        std::printf("%d\n", q);
    }
    return 0;
}
