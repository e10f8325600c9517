// affine_group.hip -- PointMLP's geometric-affine grouping stage with its first convolution hoisted to the points.
//
// LocalGrouper(normalize="anchor", use_xyz=False) + PreExtraction.transfer's convolution is, per cloud, with j = idx[s,k]
// and a = fps_idx[s],
//     d[s,k,:] = x[j,:] - x[a,:],  sigma = unbiased std of all S K C entries of d,  r = 1 / (sigma + 1e-5)
//     y[s,k,:] = W [alpha d r + beta ; x[a,:]]
// y is linear in the grouped tensor, so with [P | Q] = x [W1 alpha | W2]^T over the N POINTS (the contraction kernel of
// csrc/pointwise.hip) and c0 = W1 beta
//     y[s,k,:] = r (P[j,:] - P[a,:]) + Q[a,:] + c0
// This file is everything around that product: the moments of d (no (B,S,K,C) tensor), the combine with BatchNorm's
// partial rows in the layout apn_pw_bn_act folds, its gradient per point through the reverse lists of idx and of fps_idx
// (apn_po_csr on flat rows), the gradient through sigma, and the tail of a PreExtraction -- add + ReLU + max over K --
// with its gradient.
//
// Layout: [P | Q] is kept as ROWS of 2 O floats per point (B, N, 2 O): a gathered neighbour is one contiguous row segment,
// 64 lanes on 64 channels.  y is wanted channels-first (B, O, S K): the tile of 64 channels x 128 positions goes through
// LDS, written by channel lanes, read back along positions, so both the gather and the store are contiguous.  The
// gradient arrives as rows (B, S K, O) (one tiled transpose of dL/dy, apn_pw_transpose) for the same reason.
//
// Every sum runs in an order fixed by the shapes: no float atomic, two runs give the same bits.  The fold of the float64
// partial rows (apn_ag_fold) is csrc/col_sums.hip's, at 4 lanes.  Every index read from idx / fps_idx is clamped into its
// cloud.
#include <hip/hip_runtime.h>

#include "apn_common.h"

namespace apn {

constexpr int AG_KMAX = 64;
constexpr int AG_T = 128;            // positions per tile: the statistics tile of apn_pw_bn_act (PW_T)
constexpr int AG_OC = 64;            // channels per workgroup of the combine
constexpr int AG_ROW = AG_T + 1;     // floats per LDS row: odd, so the channel lanes' writes and the position lanes' reads
                                     // both spread over the banks
constexpr int AG_THREADS = 256;
constexpr int AG_PTS = 4;            // points per wave of the per-point kernels (16 per workgroup)
constexpr int AG_MROWS = 64;         // at most this many workgroups per cloud in the moments
constexpr int AG_PS = 128;           // queries per workgroup of the pooled epilogue

__device__ __forceinline__ int ag_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// the wave's sum in a fixed tree (lane 0 holds it)
__device__ __forceinline__ double ag_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// ------------------------------------------------------------------------------------------------------ moments
// grid (rows, clouds); wave w of the cloud's 4 rows waves takes queries w, w + 4 rows, ...; lanes on channels.
// part [rows][B][2] = {sum d, sum d^2} of the workgroup's queries, float64.
__global__ __launch_bounds__(AG_THREADS) void ag_moments_kernel(int N, int S, int K, int C, const float *__restrict__ x,
                                                                const int *__restrict__ idx,
                                                                const int *__restrict__ fps_idx,
                                                                double *__restrict__ part) {
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const float *__restrict__ xb = x + (size_t)b * N * C;
    double s1 = 0.0, s2 = 0.0;
    for (int s = blockIdx.x * 4 + wave; s < S; s += 4 * gridDim.x) {
        const size_t q = (size_t)b * S + s;
        const int a = ag_clamp(fps_idx[q], N);
        const int *__restrict__ row = idx + q * K;          // (the same address for every lane: one broadcast read)
        for (int c = lane; c < C; c += 64) {
            const float xa = xb[(size_t)a * C + c];
            for (int k = 0; k < K; ++k) {
                const int j = ag_clamp(row[k], N);
                const float d = xb[(size_t)j * C + c] - xa;
                s1 += (double)d;
                s2 += (double)d * (double)d;
            }
        }
    }
    s1 = ag_wave_sum(s1);
    s2 = ag_wave_sum(s2);
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *r = red[threadIdx.x];
        part[((size_t)blockIdx.x * gridDim.y + b) * 2 + threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

// ---------------------------------------------------------------------------------------------- combine, forward
// grid (position tiles of 128, channel chunks of 64, clouds).  Gather: wave w takes the tile's positions w, w + 4, ...,
// lane = channel.  Store / statistics: as fp_blend_stats_kernel (csrc/feature_prop.hip).
// training == 0 (what adaptpoint_amd.affine_group.affine_group_bn_act runs in eval mode): scale, shift and ReLU from the
// running statistics in this launch, y written only when a backward pass will read it.
__global__ __launch_bounds__(AG_THREADS) void ag_combine_fwd_kernel(
    int N, int S, int K, int O, const float *__restrict__ pq, const int *__restrict__ idx,
    const int *__restrict__ fps_idx, const float *__restrict__ rr, const float *__restrict__ c0, float *__restrict__ y,
    float *__restrict__ part, int training, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ run_mean, const float *__restrict__ run_var, float eps, int relu, float *__restrict__ stat,
    float *__restrict__ out) {
    __shared__ float tile[AG_OC * AG_ROW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int SK = S * K;
    const int p0 = blockIdx.x * AG_T, o0 = blockIdx.y * AG_OC, b = blockIdx.z;
    const int nc = min(AG_OC, O - o0);                 // channels of this chunk (workgroup-uniform)
    {
        const int oc = o0 + (lane < nc ? lane : nc - 1);   // clamped: every load legal
        const float r = rr[b], cc = c0[oc];
        const float *__restrict__ pb = pq + (size_t)b * N * 2 * O + oc;
        const int *__restrict__ ib = idx + (size_t)b * SK;
        const int *__restrict__ fb = fps_idx + (size_t)b * S;
        constexpr int U = 4;
#pragma clang loop vectorize(disable) interleave(disable)
        for (int i0 = 0; i0 < AG_T / 4; i0 += U) {
            float pj[U], pa[U], qa[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int p = wave + 4 * (i0 + u);
                const int pos = min(p0 + p, SK - 1);
                const int j = ag_clamp(ib[pos], N), a = ag_clamp(fb[pos / K], N);
                pj[u] = pb[(size_t)j * 2 * O];
                pa[u] = pb[(size_t)a * 2 * O];
                qa[u] = pb[(size_t)a * 2 * O + O];
            }
            // (no vectorisation: the library keeps packed-FP32 arithmetic out of every unit but pointwise.hip, build.py)
#pragma clang loop unroll(full) vectorize(disable)
            for (int u = 0; u < U; ++u) {
                const int p = wave + 4 * (i0 + u);
                // the difference first, then the scale: r (P[j] - P[a]) + Q[a] + c0, each operation rounded
                tile[lane * AG_ROW + p] = (r * (pj[u] - pa[u]) + qa[u]) + cc;
            }
        }
    }
    __syncthreads();
    const int col = t & (AG_T - 1), half = t >> 7;
    const bool in = p0 + col < SK;
    const size_t ofs = ((size_t)b * O + o0) * SK + p0 + col;
    for (int o = half; o < nc; o += 2) {
        const float v = tile[o * AG_ROW + col];
        if (training) {
            if (in) y[ofs + (size_t)o * SK] = v;
        } else {
            if (in && y) y[ofs + (size_t)o * SK] = v;
            const float inv = 1.0f / sqrtf(run_var[o0 + o] + eps);
            const float sc = (gamma ? gamma[o0 + o] : 1.0f) * inv;
            const float sh = (beta ? beta[o0 + o] : 0.0f) - run_mean[o0 + o] * sc;
            const float e = __builtin_fmaf(v, sc, sh);
            if (in) out[ofs + (size_t)o * SK] = relu ? fmaxf(e, 0.0f) : e;
        }
    }
    if (!training) {
        // stat [4][O] = {mean, invstd, scale, shift}, as apn_pw_bn_act leaves it for the backward pass
        if (stat && blockIdx.x == 0 && b == 0 && t < nc) {
            const int c = o0 + t;
            const float inv = 1.0f / sqrtf(run_var[c] + eps);
            const float sc = (gamma ? gamma[c] : 1.0f) * inv;
            stat[c] = run_mean[c];
            stat[O + c] = inv;
            stat[2 * O + c] = sc;
            stat[3 * O + c] = (beta ? beta[c] : 0.0f) - run_mean[c] * sc;
        }
        return;
    }
    // statistics: thread (row = t >> 2, block w = t & 3) sums its row's columns 32 w .. 32 w + 31 around the shift
    // c = the block's first value, in ascending order; the four blocks of a row sit in four neighbouring lanes
    const int row = t >> 2, w = t & 3;
    int nw = SK - (p0 + 32 * w);
    nw = nw < 0 ? 0 : (nw > 32 ? 32 : nw);
    const float *src = tile + row * AG_ROW + 32 * w;
    const float c = src[0];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
        const float d = j < nw ? src[j] - c : 0.0f;
        s1 += d;
        s2 = __builtin_fmaf(d, d, s2);
    }
    // the four blocks' (count, mean, M2) to the row's first lane, combined there in float64 in block order
    // (the pairwise update of Chan et al.)
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int from = (t & 60) + k;                    // lane of the row's block k
        const float ck = __shfl(c, from), ak = __shfl(s1, from), bk = __shfl(s2, from);
        int nk = SK - (p0 + 32 * k);
        nk = nk < 0 ? 0 : (nk > 32 ? 32 : nk);
        if (nk > 0) {
            const double mk = (double)ck + (double)ak / nk, m2k = (double)bk - (double)ak * (double)ak / nk;
            const double tot = cnt + nk, delta = mk - mean;
            m2 += m2k + delta * delta * cnt * nk / tot;
            mean += delta * nk / tot;
            cnt = tot;
        }
    }
    if (w == 0 && row < nc) {
        float *dst = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * O + o0 + row;
        dst[0] = (float)(mean * cnt);
        dst[O] = (float)(m2 < 0.0 ? 0.0 : m2);
    }
}

// --------------------------------------------------------------------------------------------- combine, backward
// grid (ceil(N / 16), clouds): wave w takes the points 16 bx + 4 w .. + 3, lanes on channels (chunks of 64).
// gyt: dL/dy as rows (B, S K, O).  Lists: flat rows (apn_po_csr with n = B N, m = B S): list_i holds flat positions
// (b S + s) K + k, list_a flat queries b S + s.
__global__ __launch_bounds__(AG_THREADS) void ag_combine_bwd_kernel(
    int N, int S, int K, int O, const float *__restrict__ gyt, const float *__restrict__ rr,
    const float *__restrict__ pq, const int *__restrict__ pcnt_i, const int *__restrict__ poff_i,
    const int *__restrict__ plist_i, const int *__restrict__ pcnt_a, const int *__restrict__ poff_a,
    const int *__restrict__ plist_a, float *__restrict__ dpq, double *__restrict__ part_dr,
    double *__restrict__ part_c0) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int B = gridDim.y;
    const long long npos = (long long)B * S * K, nq = (long long)B * S;
    const float r = rr[b];
    double dr = 0.0;
    for (int o0 = 0; o0 < O; o0 += 64) {
        const int o = o0 + lane;
        const bool on = o < O;
        const int oc = on ? o : O - 1;
        double gsum = 0.0;
        for (int q = 0; q < AG_PTS; ++q) {
            const int i = blockIdx.x * (4 * AG_PTS) + wave * AG_PTS + q;
            if (i >= N) break;                              // (wave-uniform)
            const size_t pt = (size_t)b * N + i;
            const int cnt = pcnt_i[pt], cna = pcnt_a[pt];
            const int *__restrict__ li = plist_i + poff_i[pt];
            const int *__restrict__ la = plist_a + poff_a[pt];
            float A = 0.0f, G = 0.0f;
            for (int e = 0; e < cnt; ++e) {
                long long pos = li[e];
                pos = pos < 0 ? 0 : (pos >= npos ? npos - 1 : pos);   // (a damaged list is never followed out of the arrays)
                A += gyt[(size_t)pos * O + oc];
            }
            for (int e = 0; e < cna; ++e) {
                long long sq = la[e];
                sq = sq < 0 ? 0 : (sq >= nq ? nq - 1 : sq);
                const float *__restrict__ gr = gyt + (size_t)sq * K * O + oc;
                float g = gr[0];
                for (int k = 1; k < K; ++k) g += gr[(size_t)k * O];
                G += g;
            }
            if (on) {
                dpq[pt * 2 * O + o] = r * (A - G);
                dpq[pt * 2 * O + O + o] = G;
                dr += (double)pq[pt * 2 * O + o] * ((double)A - (double)G);
                gsum += (double)G;
            }
        }
        __syncthreads();                                    // (red is free again)
        red[wave][lane] = gsum;
        __syncthreads();
        if (wave == 0 && on)
            part_c0[((size_t)b * gridDim.x + blockIdx.x) * O + o] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    }
    dr = ag_wave_sum(dr);
    __syncthreads();
    if (lane == 0) red[wave][0] = dr;
    __syncthreads();
    if (threadIdx.x == 0)
        part_dr[(size_t)blockIdx.x * B + b] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
}

// ------------------------------------------------------------------------------------------------ sigma, backward
// dx[i] = kappa ( sum over i's list of (d[s,k] - mu)  -  sum over the queries anchored at i of sum_k (d[s,k] - mu) )
__global__ __launch_bounds__(AG_THREADS) void ag_sigma_bwd_kernel(
    int N, int S, int K, int C, const float *__restrict__ x, const int *__restrict__ idx,
    const int *__restrict__ fps_idx, const float *__restrict__ kappa, const float *__restrict__ mu,
    const int *__restrict__ pcnt_i, const int *__restrict__ poff_i, const int *__restrict__ plist_i,
    const int *__restrict__ pcnt_a, const int *__restrict__ poff_a, const int *__restrict__ plist_a,
    float *__restrict__ dx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const float kp = kappa[b], m = mu[b];
    const float *__restrict__ xb = x + (size_t)b * N * C;
    const long long q0 = (long long)b * S;
    for (int q = 0; q < AG_PTS; ++q) {
        const int i = blockIdx.x * (4 * AG_PTS) + wave * AG_PTS + q;
        if (i >= N) return;                                 // (wave-uniform; no barrier follows)
        const size_t pt = (size_t)b * N + i;
        const int cnt = pcnt_i[pt], cna = pcnt_a[pt];
        const int *__restrict__ li = plist_i + poff_i[pt];
        const int *__restrict__ la = plist_a + poff_a[pt];
        for (int c = lane; c < C; c += 64) {
            const float xi = xb[(size_t)i * C + c];
            float s1 = 0.0f, s2 = 0.0f;
            for (int e = 0; e < cnt; ++e) {
                long long sq = (long long)(li[e] / K) - q0;
                sq = sq < 0 ? 0 : (sq >= S ? S - 1 : sq);   // the query, inside this cloud
                const int a = ag_clamp(fps_idx[q0 + sq], N);
                s1 += (xi - xb[(size_t)a * C + c]) - m;
            }
            for (int e = 0; e < cna; ++e) {
                long long sq = (long long)la[e] - q0;
                sq = sq < 0 ? 0 : (sq >= S ? S - 1 : sq);
                const int *__restrict__ row = idx + (size_t)(q0 + sq) * K;
                for (int k = 0; k < K; ++k) {
                    const int j = ag_clamp(row[k], N);
                    s2 += (xb[(size_t)j * C + c] - xi) - m;
                }
            }
            dx[pt * C + c] = kp * (s1 - s2);
        }
    }
}

// ------------------------------------------------------------------------------------------ pooled residual epilogue
// out[b,o,s] = max_k relu(z + h), sel = the first maximum's slot (0 where nothing is positive).
// grid (ceil(S / 128), O, B): the workgroup's 128 K sums go through LDS (rows of K | 1 floats).
__global__ __launch_bounds__(AG_THREADS) void ag_res_relu_max_kernel(int O, int S, int K, const float *__restrict__ z,
                                                                     const float *__restrict__ h,
                                                                     float *__restrict__ out,
                                                                     unsigned char *__restrict__ sel) {
    __shared__ float v[AG_PS * (AG_KMAX + 1)];
    const int t = threadIdx.x, s0 = blockIdx.x * AG_PS, o = blockIdx.y, b = blockIdx.z;
    const int ns = min(AG_PS, S - s0), KP = K | 1;
    const size_t row = ((size_t)b * O + o) * S + s0;
    const float *__restrict__ zb = z + row * K;
    const float *__restrict__ hb = h + row * K;
#pragma clang loop vectorize(disable) interleave(disable)
    for (int e = t; e < ns * K; e += AG_THREADS) {
        const int sq = e / K;
        v[sq * KP + (e - sq * K)] = zb[e] + hb[e];
    }
    __syncthreads();
    if (t < ns) {
        float m = v[t * KP];
        int best = 0;
        for (int k = 1; k < K; ++k) {
            const float w = v[t * KP + k];
            if (w > m) { m = w; best = k; }                // strict: the first maximum stays
        }
        const bool pos = m > 0.0f;
        out[row + t] = pos ? m : 0.0f;
        sel[row + t] = (unsigned char)(pos ? best : 0);
    }
}

// every element of gz (and gh) written: g at the kept slot where the output is positive, 0 elsewhere
__global__ __launch_bounds__(AG_THREADS) void ag_res_relu_max_grad_kernel(long long total, int K,
                                                                          const float *__restrict__ g,
                                                                          const float *__restrict__ out,
                                                                          const unsigned char *__restrict__ sel,
                                                                          float *__restrict__ gz, float *__restrict__ gh) {
    for (long long e = (long long)blockIdx.x * AG_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * AG_THREADS) {
        const long long row = e / K;
        const int k = (int)(e - row * K);
        const float v = ((int)sel[row] == k && out[row] > 0.0f) ? g[row] : 0.0f;
        gz[e] = v;
        if (gh) gh[e] = v;
    }
}

}  // namespace apn

using namespace apn;

// b clouds of n points, s queries of k neighbours: what every grouped entry of this file accepts
static bool ag_sizes(int b, int n, int s, int k) {
    return b >= 0 && n >= 0 && s >= 0 && k >= 1 && k <= AG_KMAX && k <= n && b <= 65535 &&
           (long long)b * n < (1ll << 24) && (long long)b * s < (1ll << 24);
}

extern "C" int apn_ag_moment_rows(int s) {
    if (s <= 0) return 0;
    const int rows = (s + 3) / 4;
    return rows < AG_MROWS ? rows : AG_MROWS;
}

extern "C" int apn_ag_point_rows(int n) { return n <= 0 ? 0 : (n + 4 * AG_PTS - 1) / (4 * AG_PTS); }

extern "C" int apn_ag_moments(int b, int n, int s, int k, int c, const float *x, const int *idx, const int *fps_idx,
                              double *part, void *stream) {
    if (!ag_sizes(b, n, s, k) || c < 0) return APN_EINVAL;
    if (b == 0 || s == 0 || c == 0) return APN_OK;
    if (!x || !idx || !fps_idx || !part) return APN_EINVAL;
    hipLaunchKernelGGL(ag_moments_kernel, dim3(apn_ag_moment_rows(s), b), dim3(AG_THREADS), 0, (hipStream_t)stream, n, s, k,
                       c, x, idx, fps_idx, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ag_fold(int rows, int ncol, const double *part, double *out, void *stream) {
    if (rows < 0 || ncol < 0) return APN_EINVAL;
    if (ncol == 0) return APN_OK;
    if (!out || (rows > 0 && !part)) return APN_EINVAL;
    return col_sums(part, rows, (size_t)ncol, 4, out, -1.0, (hipStream_t)stream);
}

extern "C" int apn_ag_combine_fwd(int b, int n, int s, int k, int o, const float *pq, const int *idx, const int *fps_idx,
                                  const float *r, const float *c0, float *y, float *part, int training,
                                  const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                  float eps, int relu, float *stat, float *out, void *stream) {
    if (!ag_sizes(b, n, s, k) || o < 0) return APN_EINVAL;
    if (b == 0 || s == 0 || o == 0) return APN_OK;
    if (!pq || !idx || !fps_idx || !r || !c0) return APN_EINVAL;
    if (training ? (!y || !part) : (!out || !run_mean || !run_var)) return APN_EINVAL;
    const dim3 grid((s * k + AG_T - 1) / AG_T, (o + AG_OC - 1) / AG_OC, b);
    if (grid.y > 65535) return APN_EINVAL;
    hipLaunchKernelGGL(ag_combine_fwd_kernel, grid, dim3(AG_THREADS), 0, (hipStream_t)stream, n, s, k, o, pq, idx, fps_idx,
                       r, c0, y, part, training, gamma, beta, run_mean, run_var, eps, relu, stat, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ag_combine_bwd(int b, int n, int s, int k, int o, const float *gyt, const float *r, const float *pq,
                                  const int *pcnt_poff_i, const int *plist_i, const int *pcnt_poff_a, const int *plist_a,
                                  float *dpq, double *part_dr, double *part_c0, void *stream) {
    if (!ag_sizes(b, n, s, k) || o < 0) return APN_EINVAL;
    if (b == 0 || n == 0 || o == 0) return APN_OK;
    if (!r || !pq || !pcnt_poff_i || !pcnt_poff_a || !dpq || !part_dr || !part_c0) return APN_EINVAL;
    if (s > 0 && (!gyt || !plist_i || !plist_a)) return APN_EINVAL;
    const long long npts = (long long)b * n;
    hipLaunchKernelGGL(ag_combine_bwd_kernel, dim3(apn_ag_point_rows(n), b), dim3(AG_THREADS), 0, (hipStream_t)stream, n, s,
                       k, o, gyt, r, pq, pcnt_poff_i, pcnt_poff_i + npts, plist_i, pcnt_poff_a, pcnt_poff_a + npts, plist_a,
                       dpq, part_dr, part_c0);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ag_sigma_bwd(int b, int n, int s, int k, int c, const float *x, const int *idx, const int *fps_idx,
                                const float *kappa, const float *mu, const int *pcnt_poff_i, const int *plist_i,
                                const int *pcnt_poff_a, const int *plist_a, float *dx, void *stream) {
    if (!ag_sizes(b, n, s, k) || c < 0) return APN_EINVAL;
    if (b == 0 || n == 0 || c == 0) return APN_OK;
    if (!x || !kappa || !mu || !pcnt_poff_i || !pcnt_poff_a || !dx) return APN_EINVAL;
    if (s > 0 && (!idx || !fps_idx || !plist_i || !plist_a)) return APN_EINVAL;
    const long long npts = (long long)b * n;
    hipLaunchKernelGGL(ag_sigma_bwd_kernel, dim3(apn_ag_point_rows(n), b), dim3(AG_THREADS), 0, (hipStream_t)stream, n, s,
                       k, c, x, idx, fps_idx, kappa, mu, pcnt_poff_i, pcnt_poff_i + npts, plist_i, pcnt_poff_a,
                       pcnt_poff_a + npts, plist_a, dx);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

// b clouds, o channels, s queries, k slots: what the pooled epilogue accepts
static bool ag_pool_sizes(int b, int o, int s, int k) {
    return b >= 0 && o >= 0 && s >= 0 && k >= 1 && k <= AG_KMAX && b <= 65535 && o <= 65535 &&
           (long long)b * o * s < (1ll << 31);
}

extern "C" int apn_ag_res_relu_max(int b, int o, int s, int k, const float *z, const float *h, float *out, void *sel,
                                   void *stream) {
    if (!ag_pool_sizes(b, o, s, k)) return APN_EINVAL;
    if (b == 0 || o == 0 || s == 0) return APN_OK;
    if (!z || !h || !out || !sel) return APN_EINVAL;
    hipLaunchKernelGGL(ag_res_relu_max_kernel, dim3((s + AG_PS - 1) / AG_PS, o, b), dim3(AG_THREADS), 0,
                       (hipStream_t)stream, o, s, k, z, h, out, (unsigned char *)sel);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ag_res_relu_max_grad(int b, int o, int s, int k, const float *g, const float *out, const void *sel,
                                        float *gz, float *gh, void *stream) {
    if (!ag_pool_sizes(b, o, s, k)) return APN_EINVAL;
    if (b == 0 || o == 0 || s == 0) return APN_OK;
    if (!g || !out || !sel || !gz) return APN_EINVAL;
    const long long total = (long long)b * o * s * k;
    const long long blocks = (total + AG_THREADS - 1) / AG_THREADS;
    hipLaunchKernelGGL(ag_res_relu_max_grad_kernel, dim3((unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20))),
                       dim3(AG_THREADS), 0, (hipStream_t)stream, total, k, g, out, (const unsigned char *)sel, gz, gh);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
