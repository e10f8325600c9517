// knn.hip -- exact brute-force k nearest neighbours of C-dimensional rows: apn_knn_query (the k nearest, k <= 64) and
// apn_knn_dilated (to rank 256 with only the wanted ranks written: the graph of a DeepGCN block, the k*d nearest rows of
// every row thinned to k of them -- openpoints/models/layers/graph_conv.py, DilatedKNN).  One kernel serves both.
//
// Contract (include/adaptpoint_amd.h): for every query the kd supports with the smallest key (d2, support index), in
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
// The running list of a query lives in the wave's lanes, R = ceil(kd / 64) registers per lane: rank r lives in register
// r / 64, lane r % 64 (+inf beyond what has been seen); apn_knn_query is R = 1, lane j holding the j-th smallest.
// Supports are visited in ascending index order, so a candidate that ties an entry of the list has the larger index and
// goes BEHIND it: insertion moves only the entries strictly greater than the candidate one rank up -- a DPP shift
// inside a register, lane 63 of register j - 1 carried into lane 0 of register j -- and walks the registers from the top
// down, stopping at the first one whose last entry is not greater than the candidate (nothing below it moves).  A
// candidate enters only when it is strictly below the kd-th entry (rank kd - 1, always in register R - 1): a ballot
// against that distance gates the serial insertion; after the first few chunks almost no lane passes it.  At the end
// lane j < k fetches rank slots[j] (clamped into [0, kd)) or j * dilation with one cross-lane read of the distance and
// one of the index per register: one launch, no global scratch, no atomics, a function of the inputs alone.
#include "apn_common.h"
#include "knn_list.h"

namespace apn {

constexpr int KNN_WAVES = 4;
constexpr int KNN_QPW = 4;                              // queries per wave (one float4 of query values per channel)
constexpr int KNN_TILE = KNN_WAVES * KNN_QPW;           // queries per workgroup
constexpr int KNN_THREADS = KNN_WAVES * APN_WAVE;
constexpr int KNN_CHUNK_WORDS = 8192;                   // support words staged per chunk (32 KiB)
constexpr int KNN_CHUNK_MAX = 1024;
constexpr int KNN_KD_MAX = 256;                         // ranks searched: at most 4 registers per lane

// supports per chunk: a multiple of the wave width, chunk * c <= KNN_CHUNK_WORDS (c <= 128 -> at least 64)
static inline int knn_chunk(int n, int c) {
    int ch = (KNN_CHUNK_WORDS / c) & ~(APN_WAVE - 1);
    if (ch > KNN_CHUNK_MAX) ch = KNN_CHUNK_MAX;
    const int need = (n + APN_WAVE - 1) & ~(APN_WAVE - 1);
    return ch < need ? ch : need;
}

template <int R>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(int n, int m, int c, int kd, int k, int dilation,
                                                           int chunk, const int *__restrict__ slots,
                                                           const float *support, const float *query,   // may alias
                                                           int *__restrict__ idx, float *__restrict__ dist2) {
    extern __shared__ __align__(16) float lds[];
    float *qs = lds;                                     // [c][KNN_TILE]
    float *ss = lds + c * KNN_TILE;                      // [c][chunk + 1]
    const int pitch = chunk + 1;
    const int tid = threadIdx.x;
    const int lane = tid & (APN_WAVE - 1);
    const int wave = tid / APN_WAVE;
    const int bi = blockIdx.y;
    const int q0 = blockIdx.x * KNN_TILE;
    const int tl = (kd - 1) & (APN_WAVE - 1);
    const float *sup = support + (size_t)bi * n * c;
    const float *qry = query + (size_t)bi * m * c;

    // the tile's queries, transposed; rows past m repeat the last query (computed, never written)
    for (int e = tid; e < KNN_TILE * c; e += KNN_THREADS) {
        const int qi = e / c, ci = e - qi * c;
        int q = q0 + qi;
        q = q < m ? q : m - 1;
        qs[ci * KNN_TILE + qi] = qry[(size_t)q * c + ci];
    }

    float ld[KNN_QPW][R];
    int li[KNN_QPW][R];
#pragma unroll
    for (int t = 0; t < KNN_QPW; ++t) {
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
                knn_insert<R>(ld[t], li[t], live ? acc[t] : __builtin_inff(), s, tl, lane);
        }
    }

    // lane j < k takes rank r: the table's entry clamped into [0, kd), or j * dilation
    int r = 0;
    if (lane < k) r = slots ? slots[lane] : lane * dilation;
    r = r < 0 ? 0 : (r >= kd ? kd - 1 : r);
    const int rl = r & (APN_WAVE - 1), rj = r / APN_WAVE;
#pragma unroll
    for (int t = 0; t < KNN_QPW; ++t) {
        float od = 0.0f;
        int oi = 0;
#pragma unroll
        for (int j = 0; j < R; ++j) {                    // (every lane takes part in the cross-lane reads)
            const float vd = __shfl(ld[t][j], rl, APN_WAVE);
            const int vi = __shfl(li[t][j], rl, APN_WAVE);
            if (rj == j) { od = vd; oi = vi; }
        }
        const int q = q0 + wave * KNN_QPW + t;
        if (lane < k && q < m) {
            const size_t o = ((size_t)bi * m + q) * k + lane;
            idx[o] = oi;
            if (dist2) dist2[o] = od;
        }
    }
}

}  // namespace apn

using namespace apn;

// what both entries ask of the sizes and the pointers, the empty-work return between them, and the launch
static int knn_launch(int b, int n, int m, int c, int kd, int k, int dilation, const int *slots, const float *support,
                      const float *query, int *idx, float *dist2, void *stream) {
    if (b < 0 || n < 1 || m < 0 || c < 1 || c > 128 || b > 65535) return APN_EINVAL;
    if ((long long)b * (n > m ? n : m) >= (1ll << 24)) return APN_EINVAL;
    if (b == 0 || m == 0) return APN_OK;
    if (!support || !query || !idx) return APN_EINVAL;
    const int chunk = knn_chunk(n, c);
    const size_t lds = sizeof(float) * ((size_t)c * KNN_TILE + (size_t)c * (chunk + 1));      // <= 8 + 32.5 KiB
    const dim3 grid((m + KNN_TILE - 1) / KNN_TILE, b), block(KNN_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define APN_KNN(R)                                                                                                 \
    hipLaunchKernelGGL(knn_kernel<R>, grid, block, lds, st, n, m, c, kd, k, dilation, chunk, slots, support, query, \
                       idx, dist2)
    switch ((kd + APN_WAVE - 1) / APN_WAVE) {
        case 1: APN_KNN(1); break;
        case 2: APN_KNN(2); break;
        case 3: APN_KNN(3); break;
        default: APN_KNN(4); break;
    }
#undef APN_KNN
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_knn_query(int b, int n, int m, int c, int k, const float *support, const float *query, int *idx,
                             float *dist2, void *stream) {
    if (k < 1 || k > 64 || k > n) return APN_EINVAL;
    return knn_launch(b, n, m, c, k, k, 1, nullptr, support, query, idx, dist2, stream);     // R = 1, ranks 0 .. k-1
}

extern "C" int apn_knn_dilated(int b, int n, int m, int c, int kd, int k, int dilation, const int *slots,
                               const float *support, const float *query, int *idx, float *dist2, void *stream) {
    if (kd < 1 || kd > KNN_KD_MAX || kd > n || k < 1 || k > 64 || k > kd) return APN_EINVAL;
    if (!slots && (dilation < 1 || (long long)(k - 1) * dilation >= kd)) return APN_EINVAL;
    return knn_launch(b, n, m, c, kd, k, dilation, slots, support, query, idx, dist2, stream);
}
