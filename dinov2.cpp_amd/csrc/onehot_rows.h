// onehot_rows.h -- the one-hot operand of the cluster-sum GEMMs (kmeans_update_kernel of kmeans.hip, vlad_update_kernel of vlad.hip): the
// matrix (label[i] == c) never exists in memory, a thread builds its part of the LDS image of sim_tile.h from the labels.
#pragma once
#include "sim_tile.h"

namespace dinov2 {

// The B operand of a cluster-sum tile for sim_tile: the image [128 c][64 i] = (label[i] == n0 + c) as 1.0 / 0.0 in f16, from the K-tile's 64
// labels.  A thread's four staging slots share the chunk index tid & 7, so its 8 labels serve all four; cnt[j] counts the ones it wrote
// for the centre of slot j.
struct OneHotRows {
    const int* lsrc;  // the 8 labels of this thread's chunk of K-tile 0
    int crow;         // the centre of its slot j = 0; slot j is 32 j further
    u32x4 l0, l1;     // (compared as unsigned: the -1 of a padding row equals no centre)
    int cnt[4];
    __device__ __forceinline__ void fetch(int kt) {
        l0 = *(const u32x4*)(lsrc + kt * 64);
        l1 = *(const u32x4*)(lsrc + kt * 64 + 4);
    }
    __device__ __forceinline__ void store(const SimPlace& p, char* s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned c = (unsigned)(crow + 32 * j);
            const unsigned lab[8] = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
            u32x4 oh;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned lo = lab[2 * e] == c, hi = lab[2 * e + 1] == c;
                oh[e] = lo * 0x3c00u | hi * 0x3c000000u;  // 1.0 in f16
                cnt[j] += (int)(lo + hi);
            }
            *(u32x4*)(s + p.sdst[j]) = oh;
        }
    }
};

}  // namespace dinov2
