// reverse_lists.h -- what the builders of a gather's reverse lists share (csrc/sa_wide_glue.hip over the tile map's rows,
// csrc/edge_conv.hip over the positions of a neighbour index): for every gathered point pcnt (how many rows gather it),
// poff (where its list starts) and the rows in ascending order -- a counting sort whose counts and cursors come from
// integer atomics (order-free) and whose lists are sorted afterwards, so the result is a pure function of the indices.
#pragma once
#include "apn_common.h"

namespace apn {

// {sum of mult, sum of mult * q} over a list.  Float sums: the ORDER of the add() calls and of the butterfly is part of
// the result (run-to-run and golden bit checks rest on it) -- a thread adds in ascending row order; a wave adds
// lane-strided, then wave_sum().
struct GeoSum {
    float occ = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    __device__ __forceinline__ void add(float mult, const float *__restrict__ q) {
        occ += mult;
        sx = __builtin_fmaf(mult, q[0], sx);
        sy = __builtin_fmaf(mult, q[1], sy);
        sz = __builtin_fmaf(mult, q[2], sz);
    }
    // every lane leaves with the wave's sums: xor butterfly at distances 1, 2, 4, ..., 32
    __device__ __forceinline__ void wave_sum() {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            occ += __shfl_xor(occ, d); sx += __shfl_xor(sx, d); sy += __shfl_xor(sy, d); sz += __shfl_xor(sz, d);
        }
    }
    __device__ __forceinline__ void store(float *__restrict__ geo4) const {
        *reinterpret_cast<float4 *>(geo4) = make_float4(occ, sx, sy, sz);
    }
};

// A thread's insertion sort of src[0, c) into dst[0], dst[STRIDE], ...; dst's first `sorted` entries are src's, in
// order already (in place: src == dst, STRIDE 1, sorted = 1).  A chain of dependent operations: for short lists only.
template <int STRIDE>
__device__ __forceinline__ void list_insertion_sort(const int *src, int *dst, int sorted, int c) {
    for (int i = sorted; i < c; ++i) {
        const int v = src[i];
        int j = i;
        for (; j > 0 && dst[(j - 1) * STRIDE] > v; --j) dst[j * STRIDE] = dst[(j - 1) * STRIDE];
        dst[j * STRIDE] = v;
    }
}

// Exclusive prefix sum of v over the 1024 threads of a workgroup (all of them must call it, once per kernel): inside a
// wave by lane exchanges, the sixteen wave totals by wave 0 -- two barriers (the Hillis-Steele form over LDS takes
// twenty: ~5 us of csr_cloud_kernel's 16).
__device__ __forceinline__ int block_exclusive_scan_1024(int v) {
    __shared__ int wtot[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        int w = lane < 16 ? wtot[lane] : 0;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const int u = __shfl_up(w, d);
            if (lane >= d) w += u;
        }
        if (lane < 16) wtot[lane] = w;
    }
    __syncthreads();
    return incl - v + (wave > 0 ? wtot[wave - 1] : 0);
}

// pcnt = 0 and (optional) fq = -1, one launch (a kernel, not hipMemsetAsync: the whole index stage must replay from a
// captured hipGraph, and a captured memset node aborted the replay here)
static __global__ __launch_bounds__(256) void csr_init_kernel(long long npts, int *__restrict__ pcnt, int *__restrict__ fq) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npts) return;
    pcnt[e] = 0;
    if (fq) fq[e] = -1;
}

// one block per cloud of n points: poff (and cursor, when given) = the cloud's first place + exclusive scan of pcnt.
// The first place is toff[cloud] * 32 (the first row of the cloud's first tile) when toff is given, cloud * stride
// otherwise.  (Every thread reaches the scan: its exchanges are over full waves.)
static __global__ __launch_bounds__(1024) void csr_scan_kernel(int n, const int *__restrict__ toff, int stride,
                                                               const int *__restrict__ pcnt, int *__restrict__ poff,
                                                               int *__restrict__ cursor) {
    const int t = threadIdx.x, cloud = blockIdx.x, per = (n + 1023) / 1024;
    const int *__restrict__ cnt = pcnt + (size_t)cloud * n;
    int s = 0;
    for (int i = 0; i < per; ++i) {
        const int k = t * per + i;
        if (k < n) s += cnt[k];
    }
    int run = (toff ? toff[cloud] * 32 : cloud * stride) + block_exclusive_scan_1024(s);
    for (int i = 0; i < per; ++i) {
        const int k = t * per + i;
        if (k < n) {
            poff[(size_t)cloud * n + k] = run;
            if (cursor) cursor[(size_t)cloud * n + k] = run;
            run += cnt[k];
        }
    }
}

}  // namespace apn
