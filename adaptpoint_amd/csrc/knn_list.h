// knn_list.h -- the running sorted list of a kNN search, kept in a wave's lanes: shared by csrc/knn.hip (dense batches)
// and csrc/pointops.hip (stacked clouds).  Rank r lives in register r / 64, lane r % 64; csrc/knn.hip's head describes
// the insertion.
#pragma once
#include "apn_common.h"

namespace apn {

// lane j <- lane j-1 (lane 0 keeps `v`): one DPP move, no LDS traffic
__device__ __forceinline__ int wave_shr1(int v) {
    return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

// one wave's 64 candidates (d, s: one per lane, ascending index with the lane) into the sorted list (ld, li)
template <int R>
__device__ __forceinline__ void knn_insert(float (&ld)[R], int (&li)[R], float d, int s, int tl, int lane) {
    float thr = readlane_f(ld[R - 1], tl);               // the kd-th distance: rank kd - 1 = (R - 1) * 64 + tl
    unsigned long long mask = __ballot(d < thr);
    while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float cd = readlane_f(d, l);
        if (!(cd < thr)) continue;                       // the kd-th distance has dropped below this candidate
        const int ci = __builtin_amdgcn_readlane(s, l);
#pragma unroll
        for (int j = R - 1; j >= 0; --j) {               // top down: register j - 1 is still the old one when j reads it
            // (wave-uniform) nothing at or below this register moves; the top one always does: its last entry >= thr > cd
            if (j < R - 1 && !(readlane_f(ld[j], 63) > cd)) break;
            float pd = __int_as_float(wave_shr1(__float_as_int(ld[j])));
            int pi = wave_shr1(li[j]);
            if (j > 0) {
                const float cdn = readlane_f(ld[j - 1], 63);
                const int cin = __builtin_amdgcn_readlane(li[j - 1], 63);
                if (lane == 0) { pd = cdn; pi = cin; }
            }
            if (ld[j] > cd) {                            // strictly greater entries move one rank up
                const bool prev = (j > 0 || lane > 0) && pd > cd;
                ld[j] = prev ? pd : cd;
                li[j] = prev ? pi : ci;
            }
        }
        thr = readlane_f(ld[R - 1], tl);
    }
}

}  // namespace apn
