// knn.hip -- exact brute-force k nearest neighbours of C-dimensional rows (apn_knn_query).
//
// Contract (include/adaptpoint_amd.h): for every query the k supports with the smallest key (d2, support index), in
// ascending key order, where
//
//      d2(q, s) = sum_c (q_c - s_c)^2       in fp32, by direct differences, accumulated over c = 0, 1, ..., C-1 as
//      t_c = q_c - s_c                      (one rounding)
//      a_0 = t_0 * t_0                      (one rounding)
//      a_c = fma(t_c, t_c, a_{c-1})         (one rounding per channel: the explicit fused multiply-add; the unit is
//                                            compiled with -ffp-contract=off, so nothing else contracts)
//
// The |q|^2 + |s|^2 - 2 q.s form is never used: it loses the near neighbours' digits.
//
// Shape of the kernel: a workgroup is KNN_WAVES waves and owns KNN_QPW queries per wave of one cloud.  The supports are
// staged through LDS in chunks, channel-major with a row pitch of chunk + 1 words, so that the transposing stores
// spread over the banks and a wave's 64 lanes read 64 consecutive words (one support per lane) of a channel.  The
// tile's queries lie in LDS as [channel][query]: a wave fetches its KNN_QPW query values of a channel with one
// broadcast 16-byte read, so one support word serves KNN_QPW subtract + fma pairs.
//
// The running top-k of a query lives in the wave's lanes: lane j holds the j-th smallest (d2, index) seen so far
// (+inf beyond what has been seen).  Supports are visited in ascending index order, so a candidate that ties an entry
// of the list has the larger index and goes BEHIND it: insertion shifts only the entries strictly greater than the
// candidate, and a candidate enters only when it is strictly below the k-th entry.  A ballot against that k-th
// distance gates the serial insertion; after the first few chunks almost no lane passes it.
#include "apn_common.h"

namespace apn {

constexpr int KNN_WAVES = 4;
constexpr int KNN_QPW = 4;                              // queries per wave (one float4 of query values per channel)
constexpr int KNN_TILE = KNN_WAVES * KNN_QPW;           // queries per workgroup
constexpr int KNN_THREADS = KNN_WAVES * APN_WAVE;
constexpr int KNN_CHUNK_WORDS = 8192;                   // support words staged per chunk (32 KiB)
constexpr int KNN_CHUNK_MAX = 1024;

// supports per chunk: a multiple of the wave width, chunk * c <= KNN_CHUNK_WORDS (c <= 128 -> at least 64)
__host__ __device__ inline int knn_chunk(int n, int c) {
    int ch = (KNN_CHUNK_WORDS / c) & ~(APN_WAVE - 1);
    if (ch > KNN_CHUNK_MAX) ch = KNN_CHUNK_MAX;
    const int need = (n + APN_WAVE - 1) & ~(APN_WAVE - 1);
    return ch < need ? ch : need;
}

// lane j <- lane j-1 (lane 0 keeps `v`): one DPP move, no LDS traffic
__device__ __forceinline__ int wave_shr1(int v) {
    return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

// one wave's 64 candidates (d, s: one per lane, ascending index with the lane) into the sorted list (ld, li)
__device__ __forceinline__ void knn_insert(float &ld, int &li, float d, int s, int k, int lane) {
    float thr = readlane_f(ld, k - 1);
    unsigned long long mask = __ballot(d < thr);
    while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float cd = readlane_f(d, l);
        if (!(cd < thr)) continue;                       // the k-th distance has dropped below this candidate
        const int ci = __builtin_amdgcn_readlane(s, l);
        const float pd = __int_as_float(wave_shr1(__float_as_int(ld)));
        const int pi = wave_shr1(li);
        if (ld > cd) {                                   // strictly greater entries move one lane up
            const bool prev = lane > 0 && pd > cd;
            ld = prev ? pd : cd;
            li = prev ? pi : ci;
        }
        thr = readlane_f(ld, k - 1);
    }
}

__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(int n, int m, int c, int k, int chunk,
                                                           const float *support, const float *query,   // may alias
                                                           int *__restrict__ idx,
                                                           float *__restrict__ dist2) {
    extern __shared__ __align__(16) float lds[];
    float *qs = lds;                                     // [c][KNN_TILE]
    float *ss = lds + c * KNN_TILE;                      // [c][chunk + 1]
    const int pitch = chunk + 1;
    const int tid = threadIdx.x;
    const int lane = tid & (APN_WAVE - 1);
    const int wave = tid / APN_WAVE;
    const int bi = blockIdx.y;
    const int q0 = blockIdx.x * KNN_TILE;
    const float *sup = support + (size_t)bi * n * c;
    const float *qry = query + (size_t)bi * m * c;

    // the tile's queries, transposed; rows past m repeat the last query (computed, never written)
    for (int e = tid; e < KNN_TILE * c; e += KNN_THREADS) {
        const int qi = e / c, ci = e - qi * c;
        int q = q0 + qi;
        q = q < m ? q : m - 1;
        qs[ci * KNN_TILE + qi] = qry[(size_t)q * c + ci];
    }

    float ld[KNN_QPW];
    int li[KNN_QPW];
#pragma unroll
    for (int t = 0; t < KNN_QPW; ++t) {
        ld[t] = __builtin_inff();
        li[t] = 0;
    }

    for (int s0 = 0; s0 < n; s0 += chunk) {
        const int cnt = n - s0 < chunk ? n - s0 : chunk;
        __syncthreads();                                 // the previous chunk has been read (and qs is written)
        const float *g = sup + (size_t)s0 * c;
        for (int e = tid; e < cnt * c; e += KNN_THREADS) {
            const int si = e / c, ci = e - si * c;
            ss[ci * pitch + si] = g[e];
        }
        __syncthreads();
        for (int sb = 0; sb < cnt; sb += APN_WAVE) {
            const int sl = sb + lane;
            const bool live = sl < cnt;
            const float *sp = ss + (live ? sl : 0);
            const float *qp = qs + wave * KNN_QPW;
            float acc[KNN_QPW];
            {
                const float sv = sp[0];
                const float4 qv = *reinterpret_cast<const float4 *>(qp);
                const float t0 = qv.x - sv, t1 = qv.y - sv, t2 = qv.z - sv, t3 = qv.w - sv;
                acc[0] = t0 * t0;
                acc[1] = t1 * t1;
                acc[2] = t2 * t2;
                acc[3] = t3 * t3;
            }
#pragma unroll 4
            for (int ci = 1; ci < c; ++ci) {
                const float sv = sp[ci * pitch];
                const float4 qv = *reinterpret_cast<const float4 *>(qp + ci * KNN_TILE);
                const float t0 = qv.x - sv, t1 = qv.y - sv, t2 = qv.z - sv, t3 = qv.w - sv;
                acc[0] = __builtin_fmaf(t0, t0, acc[0]);
                acc[1] = __builtin_fmaf(t1, t1, acc[1]);
                acc[2] = __builtin_fmaf(t2, t2, acc[2]);
                acc[3] = __builtin_fmaf(t3, t3, acc[3]);
            }
            const int s = s0 + sl;
#pragma unroll
            for (int t = 0; t < KNN_QPW; ++t)
                knn_insert(ld[t], li[t], live ? acc[t] : __builtin_inff(), s, k, lane);
        }
    }

    if (lane < k) {
#pragma unroll
        for (int t = 0; t < KNN_QPW; ++t) {
            const int q = q0 + wave * KNN_QPW + t;
            if (q < m) {
                const size_t o = ((size_t)bi * m + q) * k + lane;
                idx[o] = li[t];
                if (dist2) dist2[o] = ld[t];
            }
        }
    }
}

}  // namespace apn

extern "C" int apn_knn_query(int b, int n, int m, int c, int k, const float *support, const float *query, int *idx,
                             float *dist2, void *stream) {
    using namespace apn;
    if (b < 0 || n < 1 || m < 0 || c < 1 || c > 128 || k < 1 || k > 64 || k > n || b > 65535) return APN_EINVAL;
    if ((long long)b * (n > m ? n : m) >= (1ll << 24)) return APN_EINVAL;
    if (b == 0 || m == 0) return APN_OK;
    if (!support || !query || !idx) return APN_EINVAL;
    const int chunk = knn_chunk(n, c);
    const size_t lds = sizeof(float) * ((size_t)c * KNN_TILE + (size_t)c * (chunk + 1));      // <= 8 + 32.5 KiB
    dim3 grid((m + KNN_TILE - 1) / KNN_TILE, b);
    hipLaunchKernelGGL(knn_kernel, grid, dim3(KNN_THREADS), lds, (hipStream_t)stream, n, m, c, k, chunk, support, query,
                       idx, dist2);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
