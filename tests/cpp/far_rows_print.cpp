// The row selection of csrc/far_pattern.h (far_rows_sel / far_rows_entry) through a plain C++ compiler.  Arguments: d_common, the plant list
// as "row:entry,row:entry,..." (rows ascending; "-" for none), then "seed:row" pairs; prints "sel entry" per pair, one line each.
// tests/test_rows_far_probes.py compares them with the numpy restatement (tests/rows_far_cases.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dinov2.cpp_amd/csrc/far_pattern.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int d_common = std::atoi(argv[1]);
    std::vector<int64_t> rows;
    std::vector<int32_t> entries;
    if (std::strcmp(argv[2], "-") != 0) {
        char* p = argv[2];
        while (*p) {
            char* end = nullptr;
            rows.push_back((int64_t)std::strtoull(p, &end, 10));
            if (*end != ':') return 2;
            entries.push_back((int32_t)std::strtol(end + 1, &end, 10));
            if (*end == ',') ++end;
            else if (*end != '\0') return 2;
            p = end;
        }
    }
    for (int i = 3; i < argc; ++i) {
        char* end = nullptr;
        const unsigned long long seed = std::strtoull(argv[i], &end, 10);
        if (*end != ':') return 2;
        const unsigned long long row = std::strtoull(end + 1, &end, 10);
        if (*end != '\0') return 2;
        std::printf("%d %d\n", dinov2::far_rows_sel(seed, row, d_common),
                    dinov2::far_rows_entry(seed, row, d_common, rows.data(), entries.data(), (int)rows.size()));
    }
    return 0;
}
