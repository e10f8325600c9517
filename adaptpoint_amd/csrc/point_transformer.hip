// point_transformer.hip -- Point Transformer's vector-attention layer behind its q/k/v projection, fused
// (openpoints/models/backbone/pointtransformer.py: PointTransformerLayer).  Contract: include/adaptpoint_amd.h;
// design notes: DESIGN.md section 7n.  C channels, C' = C / 8 attention weights, k <= 32 slots, j = idx[i,s]:
//
//      pr = W2 h + b2            r = (k_j - q_i) + pr         y = relu(sc1 r + sh1)          (C)
//      t  = W3 y + b3            z = relu(sc2 t + sh2)        l = W4 z + b4                  (C')
//      a  = softmax over the slots                             out_i[c] = sum_s (v_j[c] + pr[c]) a_is[c mod C']
//
// No (n,k,C) tensor exists in forward; backward writes one (dr).  Two thread layouts:
//
//   channel layout   a thread owns channel c = blockIdx.y * CL + lane (CL = min(C, 256); rel_bwd: C / CL channels per
//                    thread and one block column), the 256 / CL groups of a workgroup take whole queries, the workgroups
//                    stride over the queries.  Per-channel sums live in float64 registers from the first query to the
//                    last and leave as ONE partial row per workgroup.             rel_stats, mid_bwd, rel_bwd
//   tile layout      a workgroup stages a tile of positions (mid: 8192 / C of them, the y rows) or of whole queries
//                    (attend: 2048 / C, attend_bwd: 1024 / C) in LDS and every thread computes a fixed c' of it, so the
//                    C -> C' and C' -> C' products read their vectors from LDS and their matrix rows coalesced.
//
// Every sum has a fixed order (thread-sequential, then the groups of a workgroup ascending, then apn_pt_fold over the
// workgroups -- the fold is csrc/col_sums.hip's, at 16 lanes; list walks ascending): two runs give the same bits.  No
// atomics, no memset, every output element is written.  fp32 VALU arithmetic; the unit is built with
// -ffp-contract=off, the fma calls below are the only fused operations.
#include "apn_common.h"

namespace apn {

constexpr int PT_THREADS = 256;
constexpr int PT_K_MAX = 32;
constexpr int PT_ROWS_MAX = 2048;                    // workgroups (= partial rows) of a strided kernel
constexpr int PT_ROWS_LIMIT = 1 << 24;

// elementwise loops stay scalar: interleaved by two, their arithmetic becomes packed FP32 (build.py: NO_SLP's note)
#define APN_PT_SCALAR_LOOP _Pragma("clang loop vectorize(disable) interleave(disable)")

__host__ __device__ constexpr int pt_cl(int C) { return C < PT_THREADS ? C : PT_THREADS; }

// the weights' pack: W2 (C,3) | b2 (C) | W3^T (C,C') | b3 (C') | W4 (C',C') | b4 (C')
struct PtW {
    const float *W2, *b2, *W3T, *b3, *W4, *b4;
};
__host__ __device__ __forceinline__ PtW pt_w(const float *w, int C) {
    const int Cp = C / 8;
    PtW p;
    p.W2 = w;
    p.b2 = w + 3 * C;
    p.W3T = w + 4 * C;
    p.b3 = p.W3T + C * Cp;
    p.W4 = p.b3 + Cp;
    p.b4 = p.W4 + Cp * Cp;
    return p;
}
// the folded BatchNorms: sc1 (C) | sh1 (C) | sc2 (C') | sh2 (C'); the dense terms: D1 (C) | E1 (C) | D2 (C') | E2 (C')

__device__ __forceinline__ int pt_clamp(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }
__device__ __forceinline__ float pt_pr(const float *__restrict__ w2row, float b, float h0, float h1, float h2) {
    return __builtin_fmaf(w2row[2], h2, __builtin_fmaf(w2row[1], h1, __builtin_fmaf(w2row[0], h0, b)));
}
__device__ __forceinline__ float pt_pr(float w0, float w1, float w2, float b, float h0, float h1, float h2) {
    return __builtin_fmaf(w2, h2, __builtin_fmaf(w1, h1, __builtin_fmaf(w0, h0, b)));
}
__device__ __forceinline__ float pt_r(float kj, float qi, float pr) { return (kj - qi) + pr; }
__device__ __forceinline__ float pt_dt(float sc2, float g1, float D2, float t, float E2) {
    return __builtin_fmaf(sc2, g1, __builtin_fmaf(D2, t, E2));
}

// the sum of v over the G groups' threads that share lane `cl` (ascending group), valid in group 0
template <int CL>
__device__ __forceinline__ double pt_group_sum(double v, double *red, int tid) {
    constexpr int G = PT_THREADS / CL;
    if (G == 1) return v;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    if (tid < CL)
        for (int g = 1; g < G; ++g) v += red[g * CL + tid];
    return v;
}

// ------------------------------------------------------------------------------------------------- rel_stats
template <int C>
__global__ __launch_bounds__(PT_THREADS) void pt_rel_stats_kernel(int n, int k, const float *__restrict__ qkv, int ld,
                                                                  const float *__restrict__ h,
                                                                  const int *__restrict__ idx,
                                                                  const float *__restrict__ wts,
                                                                  double *__restrict__ part) {
    constexpr int CL = pt_cl(C), G = PT_THREADS / CL;
    __shared__ double red[PT_THREADS];
    const int tid = threadIdx.x, cl = tid % CL, g = tid / CL, c = blockIdx.y * CL + cl;
    const PtW w = pt_w(wts, C);
    const float w0 = w.W2[c * 3], w1 = w.W2[c * 3 + 1], w2 = w.W2[c * 3 + 2], bb = w.b2[c];
    const long long npos = (long long)n * k, step = (long long)gridDim.x * G;
    double s = 0.0, s2 = 0.0;
#pragma unroll 4
    for (long long pos = (long long)blockIdx.x * G + g; pos < npos; pos += step) {
        const int i = (int)(pos / k), j = pt_clamp(idx[pos], n);
        const float pr = pt_pr(w0, w1, w2, bb, h[pos * 3], h[pos * 3 + 1], h[pos * 3 + 2]);
        const float r = pt_r(qkv[(size_t)j * ld + C + c], qkv[(size_t)i * ld + c], pr);
        s += (double)r;
        s2 += (double)r * (double)r;
    }
    s = pt_group_sum<CL>(s, red, tid);
    s2 = pt_group_sum<CL>(s2, red, tid);
    if (tid < CL) {
        part[(size_t)blockIdx.x * 2 * C + c] = s;
        part[(size_t)blockIdx.x * 2 * C + C + c] = s2;
    }
}

// part[blockIdx.x][j] = the sum of src[r][j] over the rows r = blockIdx.x, blockIdx.x + gridDim.x, ... (ascending), in
// float64: the bias gradient of the q/k/v projection without a framework reduction (whose captured form holds a memset)
constexpr int PT_COLSUM_PER = 6;                     // columns per thread: width <= 3 * 512
__global__ __launch_bounds__(PT_THREADS) void pt_colsum_kernel(int n, int width, const float *__restrict__ src, int ld,
                                                               double *__restrict__ part) {
    double acc[PT_COLSUM_PER];
#pragma unroll
    for (int u = 0; u < PT_COLSUM_PER; ++u) acc[u] = 0.0;
#pragma unroll 4
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const float *row = src + (size_t)r * ld;
#pragma unroll
        for (int u = 0; u < PT_COLSUM_PER; ++u) {
            const int j = threadIdx.x + u * PT_THREADS;
            if (j < width) acc[u] += (double)row[j];
        }
    }
#pragma unroll
    for (int u = 0; u < PT_COLSUM_PER; ++u) {
        const int j = threadIdx.x + u * PT_THREADS;
        if (j < width) part[(size_t)blockIdx.x * width + j] = acc[u];
    }
}

// ------------------------------------------------------------------------------------------------------- mid
template <int C>
__global__ __launch_bounds__(PT_THREADS) void pt_mid_kernel(int n, int k, const float *__restrict__ qkv, int ld,
                                                            const float *__restrict__ h, const int *__restrict__ idx,
                                                            const float *__restrict__ wts,
                                                            const float *__restrict__ bn, float *__restrict__ t,
                                                            double *__restrict__ part) {
    constexpr int Cp = C / 8, P = 8192 / C, LDY = C + 1;       // P positions per tile: P * Cp = 1024 outputs
    constexpr int PSTEP = PT_THREADS / Cp;                     // positions between a thread's four outputs
    __shared__ float y[P * LDY];
    __shared__ double red[PT_THREADS];
    const int tid = threadIdx.x, cp = tid % Cp;
    const PtW w = pt_w(wts, C);
    const float *sc1 = bn, *sh1 = bn + C;
    const long long npos = (long long)n * k, ntiles = (npos + P - 1) / P;
    double s = 0.0, s2 = 0.0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long p0 = tile * P;
        __syncthreads();                                       // the previous tile has been read
        for (int e = tid; e < P * C; e += PT_THREADS) {
            const int pp = e / C, c = e % C;
            const long long pos = p0 + pp;
            float v = 0.0f;
            if (pos < npos) {
                const int i = (int)(pos / k), j = pt_clamp(idx[pos], n);
                const float pr = pt_pr(w.W2 + c * 3, w.b2[c], h[pos * 3], h[pos * 3 + 1], h[pos * 3 + 2]);
                const float r = pt_r(qkv[(size_t)j * ld + C + c], qkv[(size_t)i * ld + c], pr);
                v = fmaxf(__builtin_fmaf(sc1[c], r, sh1[c]), 0.0f);
            }
            y[pp * LDY + c] = v;
        }
        __syncthreads();
        const int pp0 = tid / Cp;
        float acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = w.b3[cp];
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const float wv = w.W3T[c * Cp + cp];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(wv, y[(pp0 + u * PSTEP) * LDY + c], acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long pos = p0 + pp0 + u * PSTEP;
            if (pos < npos) {
                t[pos * Cp + cp] = acc[u];
                s += (double)acc[u];
                s2 += (double)acc[u] * (double)acc[u];
            }
        }
    }
    if (part != nullptr) {                                     // (uniform) the threads of one c' in ascending order
        for (int q = 0; q < 2; ++q) {
            __syncthreads();
            red[tid] = q == 0 ? s : s2;
            __syncthreads();
            if (tid < Cp) {
                double v = red[tid];
                for (int j = 1; j < PT_THREADS / Cp; ++j) v += red[j * Cp + tid];
                part[(size_t)blockIdx.x * 2 * Cp + q * Cp + tid] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- attend
template <int C>
__global__ __launch_bounds__(PT_THREADS) void pt_attend_kernel(int n, int k, const float *__restrict__ qkv, int ld,
                                                               const float *__restrict__ h,
                                                               const int *__restrict__ idx,
                                                               const float *__restrict__ wts,
                                                               const float *__restrict__ bn,
                                                               const float *__restrict__ t, float *__restrict__ a,
                                                               float *__restrict__ out) {
    constexpr int Cp = C / 8, Q = 2048 / C;                    // Q queries per tile: Q * Cp = 256 (query, c') pairs
    __shared__ float al[Q * PT_K_MAX * Cp];
    const int tid = threadIdx.x;
    const PtW w = pt_w(wts, C);
    const float *sc2 = bn + 2 * C, *sh2 = bn + 2 * C + Cp;
    const int i0 = blockIdx.x * Q;
    {
        const int q = tid / Cp, cp = tid % Cp, i = i0 + q;
        if (i < n) {
            float *lrow = al + (size_t)q * k * Cp + cp;
            const float *w4 = w.W4 + cp * Cp;
            const float b4 = w.b4[cp];
            float mx = 0.0f;
            for (int s = 0; s < k; ++s) {
                const float *trow = t + ((size_t)i * k + s) * Cp;
                float l = b4;
#pragma unroll 8
                for (int e = 0; e < Cp; ++e)
                    l = __builtin_fmaf(w4[e], fmaxf(__builtin_fmaf(sc2[e], trow[e], sh2[e]), 0.0f), l);
                lrow[s * Cp] = l;
                mx = s == 0 ? l : fmaxf(mx, l);
            }
            float sum = 0.0f;
            for (int s = 0; s < k; ++s) {
                const float e = expf(lrow[s * Cp] - mx);
                lrow[s * Cp] = e;
                sum = s == 0 ? e : sum + e;
            }
            for (int s = 0; s < k; ++s) {
                const float v = lrow[s * Cp] / sum;
                lrow[s * Cp] = v;
                a[((size_t)i * k + s) * Cp + cp] = v;
            }
        }
    }
    __syncthreads();
    for (int o = tid; o < Q * C; o += PT_THREADS) {
        const int q = o / C, c = o % C, i = i0 + q;
        if (i >= n) break;
        const float w0 = w.W2[c * 3], w1 = w.W2[c * 3 + 1], w2 = w.W2[c * 3 + 2], bb = w.b2[c];
        const float *arow = al + (size_t)q * k * Cp + c % Cp;
        float acc = 0.0f;
        for (int s = 0; s < k; ++s) {
            const size_t pos = (size_t)i * k + s;
            const int j = pt_clamp(idx[pos], n);
            const float pr = pt_pr(w0, w1, w2, bb, h[pos * 3], h[pos * 3 + 1], h[pos * 3 + 2]);
            const float term = (qkv[(size_t)j * ld + 2 * C + c] + pr) * arow[s * Cp];
            acc = s == 0 ? term : acc + term;
        }
        out[(size_t)i * C + c] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ attend_bwd
template <int C>
__global__ __launch_bounds__(PT_THREADS) void pt_attend_bwd_kernel(int n, int k, const float *__restrict__ qkv, int ld,
                                                                   const float *__restrict__ h,
                                                                   const int *__restrict__ idx,
                                                                   const float *__restrict__ wts,
                                                                   const float *__restrict__ bn,
                                                                   const float *__restrict__ t,
                                                                   const float *__restrict__ a,
                                                                   const float *__restrict__ go,
                                                                   float *__restrict__ g1, double *__restrict__ part) {
    constexpr int Cp = C / 8, Q = 1024 / C, PAIRS = Q * Cp;    // 128 (query, c') pairs per tile
    constexpr int NE = Cp * Cp;                                // dW4's entries
    constexpr int NV = NE >= PT_THREADS ? NE / PT_THREADS : 1; // entries per thread
    constexpr int R = NE >= PT_THREADS ? 1 : PT_THREADS / NE;  // threads per entry (each a residue class of positions)
    constexpr int WIDTH = NE + 3 * Cp;
    __shared__ float dl[PAIRS * PT_K_MAX], zl[PAIRS * PT_K_MAX];
    __shared__ double red[PT_THREADS];
    const int tid = threadIdx.x;
    const PtW w = pt_w(wts, C);
    const float *sc2 = bn + 2 * C, *sh2 = bn + 2 * C + Cp;
    const int ntiles = (n + Q - 1) / Q, e_own = tid % Cp;
    double sdl = 0.0, sg = 0.0, sgt = 0.0, dw[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) dw[v] = 0.0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int i0 = tile * Q;
        __syncthreads();                                       // the previous tile has been read
        if (tid < PAIRS) {
            const int q = tid / Cp, cp = tid % Cp, i = i0 + q;
            float *drow = dl + (size_t)q * k * Cp + cp, *zrow = zl + (size_t)q * k * Cp + cp;
            if (i < n) {
                float dot = 0.0f;
                for (int s = 0; s < k; ++s) {
                    const size_t pos = (size_t)i * k + s;
                    const int j = pt_clamp(idx[pos], n);
                    const float h0 = h[pos * 3], h1 = h[pos * 3 + 1], h2 = h[pos * 3 + 2];
                    float da = 0.0f;
#pragma unroll
                    for (int m = 0; m < 8; ++m) {
                        const int c = cp + m * Cp;
                        const float term = go[(size_t)i * C + c] *
                                           (qkv[(size_t)j * ld + 2 * C + c] + pt_pr(w.W2 + c * 3, w.b2[c], h0, h1, h2));
                        da = m == 0 ? term : da + term;
                    }
                    drow[s * Cp] = da;
                    zrow[s * Cp] = fmaxf(__builtin_fmaf(sc2[cp], t[pos * Cp + cp], sh2[cp]), 0.0f);
                    const float ad = a[pos * Cp + cp] * da;
                    dot = s == 0 ? ad : dot + ad;
                }
                for (int s = 0; s < k; ++s) {
                    const float v = a[((size_t)i * k + s) * Cp + cp] * (drow[s * Cp] - dot);
                    drow[s * Cp] = v;
                    sdl += (double)v;
                }
            } else {
                for (int s = 0; s < k; ++s) {
                    drow[s * Cp] = 0.0f;
                    zrow[s * Cp] = 0.0f;
                }
            }
        }
        __syncthreads();
        const int npl = Q * k;                                 // positions of the tile
        for (int o = tid; o < npl * Cp; o += PT_THREADS) {     // g1 = (W4^T dl) [z > 0]; o % Cp == e_own
            const int pl = o / Cp, i = i0 + pl / k;
            if (i >= n) break;
            float g = 0.0f;
#pragma unroll 8
            for (int cp = 0; cp < Cp; ++cp) g = __builtin_fmaf(w.W4[cp * Cp + e_own], dl[pl * Cp + cp], g);
            g = zl[pl * Cp + e_own] > 0.0f ? g : 0.0f;
            const size_t pos = (size_t)i0 * k + pl;
            g1[pos * Cp + e_own] = g;
            sg += (double)g;
            sgt += (double)g * (double)t[pos * Cp + e_own];
        }
        if (R == 1) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int ent = tid + v * PT_THREADS, cp = ent / Cp, e = ent % Cp;
                double acc = dw[v];
                for (int pl = 0; pl < npl; ++pl) acc += (double)dl[pl * Cp + cp] * (double)zl[pl * Cp + e];
                dw[v] = acc;
            }
        } else {
            const int ent = tid % NE, cp = ent / Cp, e = ent % Cp;
            double acc = dw[0];
            for (int pl = tid / NE; pl < npl; pl += R) acc += (double)dl[pl * Cp + cp] * (double)zl[pl * Cp + e];
            dw[0] = acc;
        }
    }
    double *row = part + (size_t)blockIdx.x * WIDTH;
    // dW4: the R threads of an entry in ascending order
    if (R == 1) {
#pragma unroll
        for (int v = 0; v < NV; ++v) row[tid + v * PT_THREADS] = dw[v];
    } else {
        __syncthreads();
        red[tid] = dw[0];
        __syncthreads();
        if (tid < NE) {
            double v = red[tid];
            for (int j = 1; j < R; ++j) v += red[j * NE + tid];
            row[tid] = v;
        }
    }
    for (int q = 0; q < 3; ++q) {                              // db4 (the pair threads), sum g1, sum g1 t: per c'
        __syncthreads();
        red[tid] = q == 0 ? (tid < PAIRS ? sdl : 0.0) : (q == 1 ? sg : sgt);
        __syncthreads();
        if (tid < Cp) {
            double v = red[tid];
            for (int j = 1; j < PT_THREADS / Cp; ++j) v += red[j * Cp + tid];
            row[NE + q * Cp + tid] = v;
        }
    }
}

// --------------------------------------------------------------------------------------------------- mid_bwd
// stage dt = sc2 g1 + D2 t + E2 of query i (k * C' values) into a group's LDS row by its CL lanes; zeros past n
template <int C>
__device__ __forceinline__ void pt_stage_dt(float *row, int cl, int i, int n, int k, const float *__restrict__ bn,
                                            const float *__restrict__ de, const float *__restrict__ t,
                                            const float *__restrict__ g1) {
    constexpr int Cp = C / 8, CL = pt_cl(C);
    const float *sc2 = bn + 2 * C, *D2 = de + 2 * C, *E2 = de + 2 * C + Cp;
    APN_PT_SCALAR_LOOP
    for (int e = cl; e < k * Cp; e += CL) {
        const int cp = e % Cp;
        const size_t at = (size_t)i * k * Cp + e;
        row[e] = i < n ? pt_dt(sc2[cp], g1[at], D2[cp], t[at], E2[cp]) : 0.0f;
    }
}

template <int C>
__global__ __launch_bounds__(PT_THREADS) void pt_mid_bwd_kernel(int n, int k, const float *__restrict__ qkv, int ld,
                                                                const float *__restrict__ h,
                                                                const int *__restrict__ idx,
                                                                const float *__restrict__ wts,
                                                                const float *__restrict__ bn,
                                                                const float *__restrict__ de,
                                                                const float *__restrict__ t,
                                                                const float *__restrict__ g1,
                                                                double *__restrict__ part) {
    constexpr int Cp = C / 8, CL = pt_cl(C), G = PT_THREADS / CL, WIDTH = Cp * C + Cp + 2 * C;
    __shared__ float dtl[G * PT_K_MAX * Cp];
    __shared__ double red[PT_THREADS];
    const int tid = threadIdx.x, cl = tid % CL, g = tid / CL, c = blockIdx.y * CL + cl;
    const PtW w = pt_w(wts, C);
    const float w0 = w.W2[c * 3], w1 = w.W2[c * 3 + 1], w2 = w.W2[c * 3 + 2], bb = w.b2[c];
    const float sc1 = bn[c], sh1 = bn[C + c];
    float w3[Cp];
#pragma unroll
    for (int cp = 0; cp < Cp; ++cp) w3[cp] = w.W3T[c * Cp + cp];
    double acc[Cp], sg0 = 0.0, sg0r = 0.0, sdb = 0.0;
#pragma unroll
    for (int cp = 0; cp < Cp; ++cp) acc[cp] = 0.0;
    float *row = dtl + g * PT_K_MAX * Cp;
    const int stride = gridDim.x * G, iters = (n + stride - 1) / stride;
    const bool bias_owner = blockIdx.y == 0 && cl < Cp;
    for (int it = 0; it < iters; ++it) {
        const int i = it * stride + blockIdx.x * G + g;
        __syncthreads();                                       // the previous query has been read
        pt_stage_dt<C>(row, cl, i, n, k, bn, de, t, g1);
        __syncthreads();
        if (i >= n) continue;                                  // (the loop bound is uniform: every thread meets every barrier)
        const float qi = qkv[(size_t)i * ld + c];
        for (int s = 0; s < k; ++s) {
            const size_t pos = (size_t)i * k + s;
            const int j = pt_clamp(idx[pos], n);
            const float pr = pt_pr(w0, w1, w2, bb, h[pos * 3], h[pos * 3 + 1], h[pos * 3 + 2]);
            const float r = pt_r(qkv[(size_t)j * ld + C + c], qi, pr);
            const float pre = __builtin_fmaf(sc1, r, sh1), yv = fmaxf(pre, 0.0f);
            const float *dts = row + s * Cp;
            float g0 = 0.0f;
#pragma unroll
            for (int cp = 0; cp < Cp; ++cp) {
                const float d = dts[cp];
                g0 = __builtin_fmaf(w3[cp], d, g0);
                acc[cp] += (double)d * (double)yv;
            }
            g0 = pre > 0.0f ? g0 : 0.0f;
            sg0 += (double)g0;
            sg0r += (double)g0 * (double)r;
            if (bias_owner) sdb += (double)dts[cl];
        }
    }
    double *prow = part + (size_t)blockIdx.x * WIDTH;
#pragma unroll
    for (int cp = 0; cp < Cp; ++cp) {
        const double v = pt_group_sum<CL>(acc[cp], red, tid);
        if (tid < CL) prow[(size_t)cp * C + c] = v;
    }
    sg0 = pt_group_sum<CL>(sg0, red, tid);
    sg0r = pt_group_sum<CL>(sg0r, red, tid);
    sdb = pt_group_sum<CL>(sdb, red, tid);
    if (tid < CL) {
        prow[Cp * C + Cp + c] = sg0;
        prow[Cp * C + Cp + C + c] = sg0r;
        if (bias_owner) prow[Cp * C + cl] = sdb;
    }
}

// --------------------------------------------------------------------------------------------------- rel_bwd
// the sum of v over the lanes of a channel group inside one wave (W = min(CL, 64) lanes), in every lane
template <int W>
__device__ __forceinline__ float pt_lanes_sum(float v) {
#pragma unroll
    for (int off = 1; off < W; off <<= 1) v += __shfl_xor(v, off, APN_WAVE);
    return v;
}

template <int C>
__global__ __launch_bounds__(PT_THREADS) void pt_rel_bwd_kernel(int n, int k, const float *__restrict__ qkv, int ld,
                                                                const float *__restrict__ h,
                                                                const int *__restrict__ idx,
                                                                const float *__restrict__ wts,
                                                                const float *__restrict__ bn,
                                                                const float *__restrict__ de,
                                                                const float *__restrict__ t,
                                                                const float *__restrict__ g1,
                                                                const float *__restrict__ a,
                                                                const float *__restrict__ go, float *__restrict__ dr,
                                                                float *__restrict__ dh, float *__restrict__ dqkv,
                                                                int ldg, double *__restrict__ part) {
    constexpr int Cp = C / 8, CL = pt_cl(C), G = PT_THREADS / CL, NCH = C / CL, WIDTH = 4 * C;
    constexpr int LW = CL < APN_WAVE ? CL : APN_WAVE;          // lanes of a group inside one wave
    constexpr int WPG = CL / LW;                               // waves per group
    __shared__ float dtl[G * PT_K_MAX * Cp];
    __shared__ float dhx[G * PT_K_MAX * WPG * 3];
    __shared__ double red[PT_THREADS];
    const int tid = threadIdx.x, cl = tid % CL, g = tid / CL;
    const PtW w = pt_w(wts, C);
    float w20[NCH], w21[NCH], w22[NCH], bb[NCH], sc1[NCH], sh1[NCH], D1[NCH], E1[NCH], w3[NCH][Cp];
    double dW2[NCH][3], db2[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = cl + ch * CL;
        w20[ch] = w.W2[c * 3], w21[ch] = w.W2[c * 3 + 1], w22[ch] = w.W2[c * 3 + 2], bb[ch] = w.b2[c];
        sc1[ch] = bn[c], sh1[ch] = bn[C + c], D1[ch] = de[c], E1[ch] = de[C + c];
#pragma unroll
        for (int cp = 0; cp < Cp; ++cp) w3[ch][cp] = w.W3T[c * Cp + cp];
        dW2[ch][0] = dW2[ch][1] = dW2[ch][2] = db2[ch] = 0.0;
    }
    float *row = dtl + g * PT_K_MAX * Cp;
    float *xrow = dhx + g * PT_K_MAX * WPG * 3;
    const int stride = gridDim.x * G, iters = (n + stride - 1) / stride;
    for (int it = 0; it < iters; ++it) {
        const int i = it * stride + blockIdx.x * G + g;
        const bool live = i < n;
        const int ic = live ? i : n - 1;                       // a group past the end computes the last query, writes nothing
        __syncthreads();                                       // the previous query has been read
        pt_stage_dt<C>(row, cl, ic, n, k, bn, de, t, g1);
        __syncthreads();
        float qi[NCH], goi[NCH], dq[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            qi[ch] = qkv[(size_t)ic * ld + cl + ch * CL];
            goi[ch] = go[(size_t)ic * C + cl + ch * CL];
            dq[ch] = 0.0f;
        }
        for (int s = 0; s < k; ++s) {
            const size_t pos = (size_t)ic * k + s;
            const int j = pt_clamp(idx[pos], n);
            const float h0 = h[pos * 3], h1 = h[pos * 3 + 1], h2 = h[pos * 3 + 2];
            const float *dts = row + s * Cp;
            float ph0 = 0.0f, ph1 = 0.0f, ph2 = 0.0f;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int c = cl + ch * CL;
                const float pr = pt_pr(w20[ch], w21[ch], w22[ch], bb[ch], h0, h1, h2);
                const float r = pt_r(qkv[(size_t)j * ld + C + c], qi[ch], pr);
                const float pre = __builtin_fmaf(sc1[ch], r, sh1[ch]);
                float g0 = 0.0f;
#pragma unroll
                for (int cp = 0; cp < Cp; ++cp) g0 = __builtin_fmaf(w3[ch][cp], dts[cp], g0);
                g0 = pre > 0.0f ? g0 : 0.0f;
                const float d = __builtin_fmaf(sc1[ch], g0, __builtin_fmaf(D1[ch], r, E1[ch]));
                dq[ch] = s == 0 ? d : dq[ch] + d;
                const float dpr = d + goi[ch] * a[pos * Cp + c % Cp];
                if (live) {
                    dr[pos * C + c] = d;
                    dW2[ch][0] += (double)dpr * (double)h0;
                    dW2[ch][1] += (double)dpr * (double)h1;
                    dW2[ch][2] += (double)dpr * (double)h2;
                    db2[ch] += (double)dpr;
                }
                ph0 = ch == 0 ? w20[ch] * dpr : __builtin_fmaf(w20[ch], dpr, ph0);
                ph1 = ch == 0 ? w21[ch] * dpr : __builtin_fmaf(w21[ch], dpr, ph1);
                ph2 = ch == 0 ? w22[ch] * dpr : __builtin_fmaf(w22[ch], dpr, ph2);
            }
            ph0 = pt_lanes_sum<LW>(ph0);                       // dh = W2^T dpr: the group's lanes inside the wave ...
            ph1 = pt_lanes_sum<LW>(ph1);
            ph2 = pt_lanes_sum<LW>(ph2);
            if (WPG == 1) {
                if (live && cl == 0) {
                    dh[pos * 3] = ph0;
                    dh[pos * 3 + 1] = ph1;
                    dh[pos * 3 + 2] = ph2;
                }
            } else if (cl % LW == 0) {                         // ... then the group's waves, ascending, below
                float *x = xrow + (s * WPG + cl / LW) * 3;
                x[0] = ph0, x[1] = ph1, x[2] = ph2;
            }
        }
        if (live) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) dqkv[(size_t)i * ldg + cl + ch * CL] = -dq[ch];
        }
        if (WPG > 1) {
            __syncthreads();
            if (live && cl < k * 3) {
                const float *x = xrow + (cl / 3) * WPG * 3 + cl % 3;
                float v = x[0];
#pragma unroll
                for (int wv = 1; wv < WPG; ++wv) v += x[wv * 3];
                dh[(size_t)i * k * 3 + cl] = v;
            }
        }
    }
    double *prow = part + (size_t)blockIdx.x * WIDTH;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = cl + ch * CL;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double v = pt_group_sum<CL>(dW2[ch][d], red, tid);
            if (tid < CL) prow[c * 3 + d] = v;
        }
        const double v = pt_group_sum<CL>(db2[ch], red, tid);
        if (tid < CL) prow[3 * C + c] = v;
    }
}

// ----------------------------------------------------------------------------------------------- scatter_bwd
__global__ __launch_bounds__(PT_THREADS) void pt_scatter_bwd_kernel(long long total, int k, int C,
                                                                    const float *__restrict__ dr,
                                                                    const float *__restrict__ go,
                                                                    const float *__restrict__ a,
                                                                    const int *__restrict__ pcnt,
                                                                    const int *__restrict__ poff,
                                                                    const int *__restrict__ plist,
                                                                    float *__restrict__ dqkv, int ldg) {
    const long long e = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (e >= total) return;
    const int Cp = C / 8, j = (int)(e / C), c = (int)(e % C), cnt = pcnt[j];
    const int *list = plist + poff[j];
    float dk = 0.0f, dv = 0.0f;
    for (int u = 0; u < cnt; ++u) {
        const size_t pos = (size_t)list[u];
        const float d = dr[pos * C + c];
        const float v = go[(pos / k) * C + c] * a[pos * Cp + c % Cp];
        dk = u == 0 ? d : dk + d;
        dv = u == 0 ? v : dv + v;
    }
    dqkv[(size_t)j * ldg + C + c] = dk;
    dqkv[(size_t)j * ldg + 2 * C + c] = dv;
}

static bool pt_ok(int n, int k, int c) {
    return n >= 0 && n < PT_ROWS_LIMIT && k >= 1 && k <= PT_K_MAX &&
           (c == 32 || c == 64 || c == 128 || c == 256 || c == 512);
}

// workgroups of a strided kernel: one per 64 positions, up to eight per compute unit where the partial rows are small
// (c <= 64) -- the position loops are chains of dependent gathers, hidden by resident waves only --, fewer as the rows
// grow: at c = 512 a workgroup's registers fill a SIMD and its partial row is a quarter of a megabyte (128 rows: 35 MB)
static int pt_rows(int n, int k, int c) {
    const long long want = ((long long)n * k + 63) / 64;
    const int cap = c <= 64 ? PT_ROWS_MAX : (c == 128 ? PT_ROWS_MAX / 2 : (c == 256 ? PT_ROWS_MAX / 8 : PT_ROWS_MAX / 16));
    return n == 0 ? 0 : (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

}  // namespace apn

using namespace apn;

#define PT_DISPATCH(c, KERNEL, grid, ...)                                                                          \
    switch (c) {                                                                                                   \
    case 32: hipLaunchKernelGGL(KERNEL<32>, grid, dim3(PT_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;   \
    case 64: hipLaunchKernelGGL(KERNEL<64>, grid, dim3(PT_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;   \
    case 128: hipLaunchKernelGGL(KERNEL<128>, grid, dim3(PT_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    case 256: hipLaunchKernelGGL(KERNEL<256>, grid, dim3(PT_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(KERNEL<512>, grid, dim3(PT_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;  \
    }

// mid's workgroups: one per tile of 8192 / c positions, within pt_rows' cap (a workgroup without a tile would only write
// a zero partial row for the fold to read)
static int pt_mid_rows(int n, int k, int c) {
    const long long tile = 8192 / c, tiles = ((long long)n * k + tile - 1) / tile;
    const int cap = pt_rows(n, k, c);
    return tiles < cap ? (int)tiles : cap;
}

extern "C" int apn_pt_rows(int n, int k, int c) { return pt_ok(n, k, c) ? pt_rows(n, k, c) : 0; }
extern "C" int apn_pt_mid_rows(int n, int k, int c) { return pt_ok(n, k, c) ? pt_mid_rows(n, k, c) : 0; }

extern "C" int apn_pt_rel_stats(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                                const float *wts, double *part, void *stream) {
    if (!pt_ok(n, k, c) || ld < 3 * c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!qkv || !h || !idx || !wts || !part) return APN_EINVAL;
    const dim3 grid(pt_rows(n, k, c), c / pt_cl(c));
    PT_DISPATCH(c, pt_rel_stats_kernel, grid, n, k, qkv, ld, h, idx, wts, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_pt_fold(const double *part, int rows, int width, double *sums, void *stream) {
    if (rows < 0 || rows > PT_ROWS_MAX || width < 0 || width > (1 << 20)) return APN_EINVAL;
    if (width == 0) return APN_OK;
    if (!sums || (rows > 0 && !part)) return APN_EINVAL;
    return col_sums(part, rows, (size_t)width, 16, sums, -1.0, (hipStream_t)stream);
}

static int pt_colsum_rows(int n) {
    const int want = (n + 31) / 32;
    return want > PT_ROWS_MAX / 2 ? PT_ROWS_MAX / 2 : want;
}

extern "C" int apn_pt_colsum_rows(int n) { return n > 0 && n < PT_ROWS_LIMIT ? pt_colsum_rows(n) : 0; }

extern "C" int apn_pt_colsum(int n, int width, const float *src, int ld, double *part, void *stream) {
    if (n < 0 || n >= PT_ROWS_LIMIT || width < 1 || width > PT_COLSUM_PER * PT_THREADS || ld < width) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!src || !part) return APN_EINVAL;
    hipLaunchKernelGGL(pt_colsum_kernel, dim3(pt_colsum_rows(n)), dim3(PT_THREADS), 0, (hipStream_t)stream, n, width, src,
                       ld, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_pt_mid(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                          const float *wts, const float *bn, float *t, double *part, void *stream) {
    if (!pt_ok(n, k, c) || ld < 3 * c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!qkv || !h || !idx || !wts || !bn || !t) return APN_EINVAL;
    const dim3 grid(pt_mid_rows(n, k, c));
    PT_DISPATCH(c, pt_mid_kernel, grid, n, k, qkv, ld, h, idx, wts, bn, t, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_pt_attend(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                             const float *wts, const float *bn, const float *t, float *a, float *out, void *stream) {
    if (!pt_ok(n, k, c) || ld < 3 * c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!qkv || !h || !idx || !wts || !bn || !t || !a || !out) return APN_EINVAL;
    const int Q = 2048 / c;
    const dim3 grid((n + Q - 1) / Q);
    PT_DISPATCH(c, pt_attend_kernel, grid, n, k, qkv, ld, h, idx, wts, bn, t, a, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_pt_attend_bwd(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                                 const float *wts, const float *bn, const float *t, const float *a, const float *go,
                                 float *g1, double *part, void *stream) {
    if (!pt_ok(n, k, c) || ld < 3 * c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!qkv || !h || !idx || !wts || !bn || !t || !a || !go || !g1 || !part) return APN_EINVAL;
    const dim3 grid(pt_rows(n, k, c));
    PT_DISPATCH(c, pt_attend_bwd_kernel, grid, n, k, qkv, ld, h, idx, wts, bn, t, a, go, g1, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_pt_mid_bwd(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                              const float *wts, const float *bn, const float *de, const float *t, const float *g1,
                              double *part, void *stream) {
    if (!pt_ok(n, k, c) || ld < 3 * c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!qkv || !h || !idx || !wts || !bn || !de || !t || !g1 || !part) return APN_EINVAL;
    const dim3 grid(pt_rows(n, k, c), c / pt_cl(c));
    PT_DISPATCH(c, pt_mid_bwd_kernel, grid, n, k, qkv, ld, h, idx, wts, bn, de, t, g1, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_pt_rel_bwd(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                              const float *wts, const float *bn, const float *de, const float *t, const float *g1,
                              const float *a, const float *go, float *dr, float *dh, float *dqkv, int ldg,
                              double *part, void *stream) {
    if (!pt_ok(n, k, c) || ld < 3 * c || ldg < 3 * c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!qkv || !h || !idx || !wts || !bn || !de || !t || !g1 || !a || !go || !dr || !dh || !dqkv || !part)
        return APN_EINVAL;
    const dim3 grid(pt_rows(n, k, c));
    PT_DISPATCH(c, pt_rel_bwd_kernel, grid, n, k, qkv, ld, h, idx, wts, bn, de, t, g1, a, go, dr, dh, dqkv, ldg, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_pt_scatter_bwd(int n, int k, int c, const float *dr, const float *go, const float *a,
                                  const int *pcnt_poff, const int *plist, float *dqkv, int ldg, void *stream) {
    if (!pt_ok(n, k, c) || ldg < 3 * c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!dr || !go || !a || !pcnt_poff || !plist || !dqkv) return APN_EINVAL;
    const long long total = (long long)n * c;
    hipLaunchKernelGGL(pt_scatter_bwd_kernel, dim3((unsigned)((total + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS),
                       0, (hipStream_t)stream, total, k, c, dr, go, a, pcnt_poff, pcnt_poff + n, plist, dqkv, ldg);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
