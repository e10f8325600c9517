// lds_bitonic.h -- the in-place ascending bitonic sort over an LDS array: by a workgroup for RSMix's knn threshold
// (online_aug.hip, double keys) and the point shuffle of the cloud transform (cloud_transform.hip, 64-bit keys), by one
// wave for the long reverse lists of a gather (sa_wide_glue.hip, int keys).
#pragma once
#include <hip/hip_runtime.h>

namespace apn {

// Pair i (of P / 2) of the stage at distance j inside the merges of size k: compare and exchange.  j is a power of two,
// so the pair's lower index 2 j (i / j) + i % j is a shift and a mask.
template <typename T>
__device__ __forceinline__ void bitonic_pair(T *s, int k, int j, int i) {
    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
    const T x = s[lo], y = s[hi];
    const bool up = (lo & k) == 0;
    if ((x > y) == up) { s[lo] = y; s[hi] = x; }
}

// s[0, P), P a power of two; every thread of the workgroup (THREADS of them) must call it.  Pad with keys that compare
// greater than every real one.  A fixed network: the result does not depend on timing.
template <int THREADS, typename T>
__device__ __forceinline__ void lds_bitonic_sort(T *s, int P) {
    const int t = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (P >> 1); i += THREADS) bitonic_pair(s, k, j, i);
            __syncthreads();
        }
    }
}

// The same network by ONE wave over a buffer that it alone owns (every lane calls it).  No barrier between the stages:
// the LDS operations of a wave execute in program order, so a stage reads what the stage before it wrote.
__device__ __forceinline__ void wave_lds_bitonic_sort(int *buf, int P, int lane) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
            for (int i = lane; i < (P >> 1); i += 64) bitonic_pair(buf, k, j, i);
}

}  // namespace apn
