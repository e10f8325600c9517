// lds_bitonic.h -- the in-place ascending bitonic sort over an LDS array, shared by RSMix's knn threshold
// (online_aug.hip, double keys) and the point shuffle of the cloud transform (cloud_transform.hip, 64-bit keys).
#pragma once
#include <hip/hip_runtime.h>

namespace apn {

// s[0, P), P a power of two; every thread of the workgroup (THREADS of them) must call it.  Pad with keys that compare
// greater than every real one.  A fixed network: the result does not depend on timing.
template <int THREADS, typename T>
__device__ __forceinline__ void lds_bitonic_sort(T *s, int P) {
    const int t = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (P >> 1); i += THREADS) {
                const int lo = 2 * j * (i / j) + (i % j), hi = lo + j;
                const T x = s[lo], y = s[hi];
                const bool up = (lo & k) == 0;
                if ((x > y) == up) { s[lo] = y; s[hi] = x; }
            }
            __syncthreads();
        }
    }
}

}  // namespace apn
