// knn_wide.hip -- exact kNN to rank 256 with only the wanted ranks written (apn_knn_dilated): the graph of a DeepGCN
// block, the k*d nearest rows of every row thinned to k of them (openpoints/models/layers/graph_conv.py, DilatedKNN).
//
// The key, the distance arithmetic and the staging are knn.hip's, word for word: key (d2, support index) ascending,
//
//      t_c = q_c - s_c,  a_0 = t_0 * t_0,  a_c = fma(t_c, t_c, a_{c-1})   over c = 0, 1, ..., C-1
//
// supports staged through LDS in chunks, channel-major with a row pitch of chunk + 1 words, the tile's queries as
// [channel][query], KW_QPW queries per wave.
//
// The running list of a query is knn.hip's resident list widened to R = ceil(kd / 64) registers per lane: rank r lives in
// register r / 64, lane r % 64 (+inf beyond what has been seen).  Supports arrive in ascending index order, so a
// candidate that ties an entry goes BEHIND it: insertion moves only the entries strictly greater than the candidate one
// rank up -- a DPP shift inside a register, lane 63 of register j - 1 carried into lane 0 of register j -- and walks the
// registers from the top down, stopping at the first one whose last entry is not greater than the candidate (nothing
// below it moves).  A ballot against the kd-th distance (rank kd - 1, always in register R - 1) gates the serial
// insertion.  At the end lane j < k fetches rank slots[j] (clamped into [0, kd)) or j * dilation with one cross-lane
// read of the distance and one of the index per register: one launch, no global scratch, no atomics, a function of the
// inputs alone.
#include "apn_common.h"

namespace apn {

constexpr int KW_WAVES = 4;
constexpr int KW_QPW = 4;                               // queries per wave (one float4 of query values per channel)
constexpr int KW_TILE = KW_WAVES * KW_QPW;              // queries per workgroup
constexpr int KW_THREADS = KW_WAVES * APN_WAVE;
constexpr int KW_CHUNK_WORDS = 8192;                    // support words staged per chunk (32 KiB)
constexpr int KW_CHUNK_MAX = 1024;
constexpr int KW_KD_MAX = 256;

// supports per chunk: a multiple of the wave width, chunk * c <= KW_CHUNK_WORDS (c <= 128 -> at least 64)
static inline int kw_chunk(int n, int c) {
    int ch = (KW_CHUNK_WORDS / c) & ~(APN_WAVE - 1);
    if (ch > KW_CHUNK_MAX) ch = KW_CHUNK_MAX;
    const int need = (n + APN_WAVE - 1) & ~(APN_WAVE - 1);
    return ch < need ? ch : need;
}

// lane j <- lane j-1 (lane 0 keeps `v`): one DPP move, no LDS traffic
__device__ __forceinline__ int kw_shr1(int v) {
    return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

// one wave's 64 candidates (d, s: one per lane, ascending index with the lane) into the sorted list (ld, li)
template <int R>
__device__ __forceinline__ void kw_insert(float (&ld)[R], int (&li)[R], float d, int s, int tl, int lane) {
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
            if (!(readlane_f(ld[j], 63) > cd)) break;    // (wave-uniform) nothing at or below this register moves
            float pd = __int_as_float(kw_shr1(__float_as_int(ld[j])));
            int pi = kw_shr1(li[j]);
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

template <int R>
__global__ __launch_bounds__(KW_THREADS) void knn_wide_kernel(int n, int m, int c, int kd, int k, int dilation,
                                                               int chunk, const int *__restrict__ slots,
                                                               const float *support, const float *query,   // may alias
                                                               int *__restrict__ idx, float *__restrict__ dist2) {
    extern __shared__ __align__(16) float lds[];
    float *qs = lds;                                     // [c][KW_TILE]
    float *ss = lds + c * KW_TILE;                       // [c][chunk + 1]
    const int pitch = chunk + 1;
    const int tid = threadIdx.x;
    const int lane = tid & (APN_WAVE - 1);
    const int wave = tid / APN_WAVE;
    const int bi = blockIdx.y;
    const int q0 = blockIdx.x * KW_TILE;
    const int tl = (kd - 1) & (APN_WAVE - 1);
    const float *sup = support + (size_t)bi * n * c;
    const float *qry = query + (size_t)bi * m * c;

    // the tile's queries, transposed; rows past m repeat the last query (computed, never written)
    for (int e = tid; e < KW_TILE * c; e += KW_THREADS) {
        const int qi = e / c, ci = e - qi * c;
        int q = q0 + qi;
        q = q < m ? q : m - 1;
        qs[ci * KW_TILE + qi] = qry[(size_t)q * c + ci];
    }

    float ld[KW_QPW][R];
    int li[KW_QPW][R];
#pragma unroll
    for (int t = 0; t < KW_QPW; ++t) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            ld[t][j] = __builtin_inff();
            li[t][j] = 0;
        }
    }

    for (int s0 = 0; s0 < n; s0 += chunk) {
        const int cnt = n - s0 < chunk ? n - s0 : chunk;
        __syncthreads();                                 // the previous chunk has been read (and qs is written)
        const float *g = sup + (size_t)s0 * c;
        for (int e = tid; e < cnt * c; e += KW_THREADS) {
            const int si = e / c, ci = e - si * c;
            ss[ci * pitch + si] = g[e];
        }
        __syncthreads();
        for (int sb = 0; sb < cnt; sb += APN_WAVE) {
            const int sl = sb + lane;
            const bool live = sl < cnt;
            const float *sp = ss + (live ? sl : 0);
            const float *qp = qs + wave * KW_QPW;
            float acc[KW_QPW];
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
                const float4 qv = *reinterpret_cast<const float4 *>(qp + ci * KW_TILE);
                const float t0 = qv.x - sv, t1 = qv.y - sv, t2 = qv.z - sv, t3 = qv.w - sv;
                acc[0] = __builtin_fmaf(t0, t0, acc[0]);
                acc[1] = __builtin_fmaf(t1, t1, acc[1]);
                acc[2] = __builtin_fmaf(t2, t2, acc[2]);
                acc[3] = __builtin_fmaf(t3, t3, acc[3]);
            }
            const int s = s0 + sl;
#pragma unroll
            for (int t = 0; t < KW_QPW; ++t)
                kw_insert<R>(ld[t], li[t], live ? acc[t] : __builtin_inff(), s, tl, lane);
        }
    }

    // lane j < k takes rank r: the table's entry clamped into [0, kd), or j * dilation
    int r = 0;
    if (lane < k) r = slots ? slots[lane] : lane * dilation;
    r = r < 0 ? 0 : (r >= kd ? kd - 1 : r);
    const int rl = r & (APN_WAVE - 1), rj = r / APN_WAVE;
#pragma unroll
    for (int t = 0; t < KW_QPW; ++t) {
        float od = 0.0f;
        int oi = 0;
#pragma unroll
        for (int j = 0; j < R; ++j) {                    // (every lane takes part in the cross-lane reads)
            const float vd = __shfl(ld[t][j], rl, APN_WAVE);
            const int vi = __shfl(li[t][j], rl, APN_WAVE);
            if (rj == j) { od = vd; oi = vi; }
        }
        const int q = q0 + wave * KW_QPW + t;
        if (lane < k && q < m) {
            const size_t o = ((size_t)bi * m + q) * k + lane;
            idx[o] = oi;
            if (dist2) dist2[o] = od;
        }
    }
}

}  // namespace apn

extern "C" int apn_knn_dilated(int b, int n, int m, int c, int kd, int k, int dilation, const int *slots,
                               const float *support, const float *query, int *idx, float *dist2, void *stream) {
    using namespace apn;
    if (b < 0 || n < 1 || m < 0 || c < 1 || c > 128 || kd < 1 || kd > KW_KD_MAX || kd > n || k < 1 || k > 64 || k > kd ||
        b > 65535)
        return APN_EINVAL;
    if ((long long)b * (n > m ? n : m) >= (1ll << 24)) return APN_EINVAL;
    if (!slots && (dilation < 1 || (long long)(k - 1) * dilation >= kd)) return APN_EINVAL;
    if (b == 0 || m == 0) return APN_OK;
    if (!support || !query || !idx) return APN_EINVAL;
    const int chunk = kw_chunk(n, c);
    const size_t lds = sizeof(float) * ((size_t)c * KW_TILE + (size_t)c * (chunk + 1));       // <= 8 + 32.5 KiB
    const dim3 grid((m + KW_TILE - 1) / KW_TILE, b), block(KW_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define APN_KW(R)                                                                                                  \
    hipLaunchKernelGGL(knn_wide_kernel<R>, grid, block, lds, st, n, m, c, kd, k, dilation, chunk, slots, support,  \
                       query, idx, dist2)
    switch ((kd + APN_WAVE - 1) / APN_WAVE) {
        case 1: APN_KW(1); break;
        case 2: APN_KW(2); break;
        case 3: APN_KW(3); break;
        default: APN_KW(4); break;
    }
#undef APN_KW
    APN_LAUNCH_CHECK();
    return APN_OK;
}
