// online_aug.hip -- the two non-learned point-cloud augmenters of the reference's online_aug/ on the device.
//
// PointWOLF (openpoints/online_aug/pointwolf.py:110-148): one thread per anchor turns the call's random draws into the
// per-anchor affine map the deformation kernel of augment.hip consumes (lin = R diag(s), off = t) and the per-cloud
// projection axes of the kernel regression:
//   angle = pi u_deg / 180 * keep[0],  scale = u_scale * keep[1] * axis (a 0 becomes 1),  t = u_trl * keep[2] * axis
// with R composed as the reference composes it (anchor_rotation.h).
//
// RSMix (openpoints/online_aug/rsmix_provider.py:161-222): per selection (2B of them: the erase set of cloud c around
// point i1[c], the add set of cloud perm[c] around point i2[c]) one workgroup computes numpy's expanded float64 squared
// distance d = (-2 q.x + |q|^2) + |x|^2_f32, finds the threshold (knn: the k-th smallest d by a bitonic sort in LDS;
// ball: r^2), and writes the first `nsample` members d <= threshold in ascending index order with a wave-ballot
// compaction.  Then one workgroup per output cloud: the kept points (stable compaction of the cloud without its erase
// set), followed by the picked points of the partner cloud moved by q1 - q2 in float64, and lambda.  Integer LDS
// counters only; no float atomics, so every output is the same bit for bit from run to run.
#include <hip/hip_runtime.h>

#include "../../include/adaptpoint_amd.h"
#include "anchor_rotation.h"
#include "apn_common.h"
#include "lds_bitonic.h"

namespace apn {

// ------------------------------------------------------------------------------------------------------------ PointWOLF
// draws: keep (b*m*3) | axis code (b*m) | degree (b*m*3) | scale (b*m*3) | translation (b*m*3) | kernel axis code (b),
// either the reference's values (uniform = 0) or U[0,1) numbers mapped here onto the same distributions (uniform = 1).
__global__ __launch_bounds__(64) void pointwolf_params_kernel(int b, int m, const float *__restrict__ draws, int uniform,
                                                              float r_range, float s_range, float t_range,
                                                              float *__restrict__ lin, float *__restrict__ off,
                                                              float *__restrict__ kaxes) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int n = b * m;
    if (i >= n) return;
    const float *keep = draws, *code = draws + (size_t)n * 3, *deg = code + n, *scl = deg + (size_t)n * 3,
                *trl = scl + (size_t)n * 3, *kcode = trl + (size_t)n * 3;
    float k[3], u_deg[3], u_scl[3], u_trl[3];
    int ac;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        k[c] = keep[(size_t)i * 3 + c];
        u_deg[c] = deg[(size_t)i * 3 + c];
        u_scl[c] = scl[(size_t)i * 3 + c];
        u_trl[c] = trl[(size_t)i * 3 + c];
    }
    ac = (int)code[i];
    if (uniform) {
        const float r = fabsf(r_range), t = fabsf(t_range);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            k[c] = k[c] < 0.5f ? 1.0f : 0.0f;                  // bernoulli(0.5)
            u_deg[c] = -r + (r + r) * u_deg[c];                // uniform_(-r, r)
            u_scl[c] = 1.0f + (s_range - 1.0f) * u_scl[c];     // uniform_(1, s)
            u_trl[c] = -t + (t + t) * u_trl[c];                // uniform_(-t, t)
        }
        ac = 1 + min((int)(code[i] * 7.0f), 6);                // randint(1, 8)
    }
    const float kpi = 3.14159265358979323846f;
    AnchorTerms a;
    float t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float ax = (float)((ac >> c) & 1);
        const float ang = kpi * u_deg[c] / 180.0f * k[0];
        a.sn[c] = sinf(ang);
        a.cs[c] = cosf(ang);
        const float s = u_scl[c] * k[1] * ax;
        a.s[c] = s == 0.0f ? 1.0f : s;
        t[c] = u_trl[c] * k[2] * ax;
    }
    float R[9];
    anchor_rotation(a, R);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) lin[(size_t)i * 9 + 3 * r + c] = R[3 * r + c] * a.s[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) off[(size_t)i * 3 + c] = t[c];
    if (i % m == 0) {
        const int cloud = i / m;
        int kc = (int)kcode[cloud];
        if (uniform) kc = 1 + min((int)(kcode[cloud] * 7.0f), 6);
#pragma unroll
        for (int c = 0; c < 3; ++c) kaxes[(size_t)cloud * 3 + c] = (float)((kc >> c) & 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------- RSMix
constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_MAXN = 8192;

// numpy's square_distance for one float32 point against a query held in float64 (rsmix_provider.py:136-138):
// -2 * matmul(q, x) + sum(q**2) + sum(x**2), the last sum in float32.  Products of two float32 values are exact in
// float64, so only the sums round; -ffp-contract=off keeps them as written.
__device__ __forceinline__ double rs_dist(const double (&q)[3], double qq, const float *p) {
    const float x = p[0], y = p[1], z = p[2];
    const double dot = (q[0] * (double)x + q[1] * (double)y) + q[2] * (double)z;
    const float xx = (x * x + y * y) + z * z;
    return (-2.0 * dot + qq) + (double)xx;
}

// exclusive prefix of `flag` over the workgroup in thread order; returns it and sets *total (all threads)
__device__ __forceinline__ int rs_block_prefix(bool flag, int *wcount, int *total) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long bal = __ballot(flag);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int in_wave = __popcll(bal & below);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) {
        const int c = wcount[w];
        before += w < wave ? c : 0;
        all += c;
    }
    __syncthreads();                                  // wcount is reused by the next call
    *total = all;
    return before + in_wave;
}

__global__ __launch_bounds__(RS_THREADS) void rsmix_select_kernel(int b, int n, int c, const float *__restrict__ points,
                                                                  const int *__restrict__ draws, double r2, int knn_k,
                                                                  int nsample, int *__restrict__ members,
                                                                  int *__restrict__ counts) {
    __shared__ double sd[RS_MAXN];
    __shared__ int wcount[RS_WAVES];
    const int s = blockIdx.x, t = threadIdx.x;
    const int *perm = draws, *i1 = draws + b, *i2 = draws + 2 * b;
    const int cloud = s < b ? s : perm[s - b];
    const int qi = s < b ? i1[s] : i2[s - b];
    const float *pc = points + (size_t)cloud * n * c;
    const double q[3] = {(double)pc[(size_t)qi * c + 0], (double)pc[(size_t)qi * c + 1], (double)pc[(size_t)qi * c + 2]};
    const double qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    double thr = r2;
    if (knn_k >= 0) {
        int P = 1;
        while (P < n) P <<= 1;
        for (int p = t; p < P; p += RS_THREADS) sd[p] = p < n ? rs_dist(q, qq, pc + (size_t)p * c) : INFINITY;
        __syncthreads();
        // bitonic sort, ascending: the k-th order statistic, ties and all, as np.sort gives it
        lds_bitonic_sort<RS_THREADS>(sd, P);
        thr = sd[knn_k];
    }
    int base = 0;
    int *out = members + (size_t)s * nsample;
    for (int start = 0; start < n; start += RS_THREADS) {
        const int p = start + t;
        const bool in = p < n && rs_dist(q, qq, pc + (size_t)p * c) <= thr;
        int total;
        const int pos = base + rs_block_prefix(in, wcount, &total);
        if (in && pos < nsample) out[pos] = p;
        base += total;
        if (base >= nsample) break;                    // uniform across the workgroup
    }
    const int cnt = base < nsample ? base : nsample;
    for (int j = cnt + t; j < nsample; j += RS_THREADS) out[j] = -1;
    if (t == 0) counts[s] = cnt;
}

// pick (b, nsample): per cloud, for its |E| appended rows, a position in the add list (|A| > 0) or, with an empty add
// list, a row of the cloud itself in [0, n - |E|) (rsmix_provider.py:199-200 indexes the original cloud there).
__global__ __launch_bounds__(RS_THREADS) void rsmix_mix_kernel(int b, int n, int c, int nsample,
                                                               const float *__restrict__ points,
                                                               const int *__restrict__ draws,
                                                               const int *__restrict__ members,
                                                               const int *__restrict__ counts,
                                                               const int *__restrict__ pick, float *__restrict__ out,
                                                               float *__restrict__ lam) {
    __shared__ unsigned char erased[RS_MAXN];
    __shared__ int wcount[RS_WAVES];
    const int cl = blockIdx.x, t = threadIdx.x;
    const int *perm = draws, *i1 = draws + b, *i2 = draws + 2 * b;
    const int ne = counts[cl], na = counts[b + cl];
    const float *src = points + (size_t)cl * n * c;
    float *dst = out + (size_t)cl * n * c;
    for (int p = t; p < n; p += RS_THREADS) erased[p] = 0;
    __syncthreads();
    for (int j = t; j < ne; j += RS_THREADS) erased[members[(size_t)cl * nsample + j]] = 1;
    __syncthreads();
    int base = 0;
    for (int start = 0; start < n; start += RS_THREADS) {
        const int p = start + t;
        const bool keep = p < n && !erased[p];
        int total;
        const int r = base + rs_block_prefix(keep, wcount, &total);
        if (keep)
            for (int ch = 0; ch < c; ++ch) dst[(size_t)r * c + ch] = src[(size_t)p * c + ch];
        base += total;
    }
    const int kept = n - ne;
    if (na == 0) {
        for (int j = t; j < ne; j += RS_THREADS) {
            const float *ps = src + (size_t)pick[(size_t)cl * nsample + j] * c;
            for (int ch = 0; ch < c; ++ch) dst[(size_t)(kept + j) * c + ch] = ps[ch];
        }
    } else {
        const int pc = perm[cl];
        const float *partner = points + (size_t)pc * n * c;
        const float *q1 = src + (size_t)i1[cl] * c, *q2 = partner + (size_t)i2[cl] * c;
        const double d[3] = {(double)q1[0] - (double)q2[0], (double)q1[1] - (double)q2[1], (double)q1[2] - (double)q2[2]};
        const int *add = members + (size_t)(b + cl) * nsample;
        for (int j = t; j < ne; j += RS_THREADS) {
            const float *ps = partner + (size_t)add[pick[(size_t)cl * nsample + j]] * c;
            float *pd = dst + (size_t)(kept + j) * c;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) pd[ch] = (float)(d[ch] + (double)ps[ch]);
            for (int ch = 3; ch < c; ++ch) pd[ch] = ps[ch];
        }
    }
    if (t == 0) lam[cl] = (ne == 0 || na == 0) ? 0.0f : (float)((double)ne / (double)n);
}

}  // namespace apn

extern "C" int apn_pointwolf_params(int b, int m, const float *draws, int uniform, float r_range, float s_range,
                                    float t_range, float *lin, float *off, float *kaxes, void *stream) {
    using namespace apn;
    if (b < 0 || m <= 0) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!draws || !lin || !off || !kaxes) return APN_EINVAL;
    const int n = b * m;
    hipLaunchKernelGGL(pointwolf_params_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, b, m, draws,
                       uniform, r_range, s_range, t_range, lin, off, kaxes);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_rsmix_select(int b, int n, int c, const float *points, const int *draws, double r2, int knn_k,
                                int nsample, int *members, int *counts, void *stream) {
    using namespace apn;
    if (b < 0 || n <= 0 || n > RS_MAXN || c < 3 || nsample <= 0 || nsample >= n || knn_k >= n) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!points || !draws || !members || !counts) return APN_EINVAL;
    hipLaunchKernelGGL(rsmix_select_kernel, dim3(2 * b), dim3(RS_THREADS), 0, (hipStream_t)stream, b, n, c, points, draws,
                       r2, knn_k, nsample, members, counts);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_rsmix_mix(int b, int n, int c, int nsample, const float *points, const int *draws, const int *members,
                             const int *counts, const int *pick, float *out, float *lam, void *stream) {
    using namespace apn;
    if (b < 0 || n <= 0 || n > RS_MAXN || c < 3 || nsample <= 0 || nsample >= n) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!points || !draws || !members || !counts || !pick || !out || !lam) return APN_EINVAL;
    hipLaunchKernelGGL(rsmix_mix_kernel, dim3(b), dim3(RS_THREADS), 0, (hipStream_t)stream, b, n, c, nsample, points, draws,
                       members, counts, pick, out, lam);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
