// feature_prop.hip -- the feature-propagation decoder with its convolution hoisted to the coarse points.
//
// The block is  y = W [f1 ; blend(f2)]  followed by BatchNorm (+ ReLU), with blend() = three_interpolate: both linear, so
//     y = W[:, :C1] f1 + blend(W[:, C1:] f2)
// -- the coarse-level product runs on m < n points, and the interpolation on O channels instead of C2.  The two products
// are ONE launch of the contraction kernel (csrc/pointwise.hip, apn_pw_contract2); this file is what follows them:
//
//     y[b][o][i] = a[b][o][i] + sum_j weight[b][i][j] * u[b][o][idx[b][i][j]],  j < 3
//
// for a = W[:, :C1] f1 (B, O, n) (or none) and u = W[:, C1:] f2 (B, O, m), channels-first as the contraction writes them
// and as three_interpolate_kernel reads them: a lane's three neighbours are three 4-byte reads of a row of m floats
// that stays in L2.  In training mode the launch also leaves BatchNorm's batch statistics of y as the partial rows
// apn_pw_bn_act folds -- part[tile][2][O], tile = cloud * tx + column block of 128, {sum, M2 around the tile's own mean},
// formed exactly as pw_gemm_kernel's epilogue forms them (per 32 columns around a shift, the four blocks combined in
// float64: see the comment there) -- in eval mode scale, shift and ReLU are applied here and nothing follows.
// Every sum runs in a fixed order: no float atomic, bit-identical results from run to run.
//
// The conditioned form (apn_fp_blend_stats_cond) serves a block whose concatenation starts with a per-cloud vector
// repeated over the points, W [cond 1^T ; f1 ; blend(f2)]: the vector's share of the product is one number per (cloud,
// channel), cvec[b][o] = (W[:, :Cc] cond_b)[o], and the launch adds it LAST -- y = (a + blend(u)) + cvec -- before the
// statistics.  It is the same kernel with one more pointer (null: the unconditioned block, the same bits as before).
// Its gradient is the row sum gc[b][o] = sum_i gy[b][o][i] (fp_cond_grad_kernel, one wave per row, fixed order).
#include <hip/hip_runtime.h>

#include "apn_common.h"

namespace apn {

constexpr int FP_T = 128;          // columns per tile: the statistics tile of apn_pw_bn_act (PW_T)
constexpr int FP_OC = 64;          // channels per workgroup
constexpr int FP_ROW = FP_T + 4;   // floats per LDS row: four threads read a row's four 32-column blocks as float4s; the pad
                                   // keeps neighbouring rows apart in the banks (blocks 0 / 2 and 1 / 3 of a row still meet:
                                   // two passes per read, eight reads per thread -- not worth a staggered layout)
constexpr int FP_THREADS = 256;
constexpr int FP_U = 8;            // channels whose loads a thread has in flight together

// grid (column tiles, channel chunks, clouds); thread t: column t & 127, channels (t >> 7) + 2 k of the chunk
__global__ __launch_bounds__(FP_THREADS) void fp_blend_stats_kernel(
    int O, int m, int n, const float *a, const float *__restrict__ u, const int *__restrict__ idx,
    const float *__restrict__ weight, float *y, float *__restrict__ part, int training, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ run_mean, const float *__restrict__ run_var, float eps,
    int relu, float *__restrict__ stat, float *__restrict__ out, const float *__restrict__ cvec) {
    __shared__ __attribute__((aligned(16))) float tile[FP_OC * FP_ROW];
    const int t = threadIdx.x, col = t & (FP_T - 1), half = t >> 7;
    const int n0 = blockIdx.x * FP_T, o0 = blockIdx.y * FP_OC, b = blockIdx.z;
    const int nc = min(FP_OC, O - o0);                 // channels of this chunk (workgroup-uniform)
    const int i = n0 + col;
    const bool in = i < n;
    const int ic = in ? i : n - 1;                     // clamped: every load legal and unpredicated
    const size_t pt = ((size_t)b * n + ic) * 3;
    // the indices are trusted to lie in [0, m) as apn_three_interpolate trusts them; clamped all the same, so that a bad
    // index reads a wrong row element instead of memory outside u
    const int i0 = min(max(idx[pt], 0), m - 1), i1 = min(max(idx[pt + 1], 0), m - 1), i2 = min(max(idx[pt + 2], 0), m - 1);
    const float w0 = weight[pt], w1 = weight[pt + 1], w2 = weight[pt + 2];
    const float *ub = u + ((size_t)b * O + o0) * m;
    const float *ab = a ? a + ((size_t)b * O + o0) * n + ic : nullptr;
    float *yb = y ? y + ((size_t)b * O + o0) * n + i : nullptr;
    float *ob = out ? out + ((size_t)b * O + o0) * n + i : nullptr;
    const float *cb = cvec ? cvec + (size_t)b * O + o0 : nullptr;     // the cloud's conditioning bias (workgroup-uniform)
    for (int k0 = half; k0 < nc; k0 += 2 * FP_U) {
        float va[FP_U], v0[FP_U], v1[FP_U], v2[FP_U], vc[FP_U];
#pragma unroll
        for (int e = 0; e < FP_U; ++e) {
            const int o = k0 + 2 * e;
            const int oc = o < nc ? o : nc - 1;
            const float *ur = ub + (size_t)oc * m;
            v0[e] = ur[i0]; v1[e] = ur[i1]; v2[e] = ur[i2];
            va[e] = ab ? ab[(size_t)oc * n] : 0.0f;
            vc[e] = cb ? cb[oc] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < FP_U; ++e) {
            const int o = k0 + 2 * e;
            if (o < nc) {
                // the interpolation's own order (three_interpolate_kernel), then the skip product
                float v = __builtin_fmaf(w2, v2[e], __builtin_fmaf(w1, v1[e], w0 * v0[e]));
                v = va[e] + v;
                if (cb) v = v + vc[e];                      // (a + blend(u)) + cvec: the conditioning bias last
                if (training) {
                    tile[o * FP_ROW + col] = v;
                    if (in) yb[(size_t)o * n] = v;
                } else {
                    if (in && yb) yb[(size_t)o * n] = v;
                    const float inv = 1.0f / sqrtf(run_var[o0 + o] + eps);
                    const float sc = (gamma ? gamma[o0 + o] : 1.0f) * inv;
                    const float sh = (beta ? beta[o0 + o] : 0.0f) - run_mean[o0 + o] * sc;
                    const float r = __builtin_fmaf(v, sc, sh);
                    if (in) ob[(size_t)o * n] = relu ? fmaxf(r, 0.0f) : r;
                }
            }
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
    __syncthreads();
    // statistics: thread (row = t >> 2, block w = t & 3) sums its row's columns 32 w .. 32 w + 31 around the shift
    // c = the block's first value, in ascending order; the four blocks of a row sit in four neighbouring lanes
    const int row = t >> 2, w = t & 3;
    int nw = n - (n0 + 32 * w);
    nw = nw < 0 ? 0 : (nw > 32 ? 32 : nw);
    const float *src = tile + (row < nc ? row : 0) * FP_ROW + 32 * w;
    const float c = src[0];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 v = *reinterpret_cast<const float4 *>(src + 4 * j);
        const float d0 = 4 * j < nw ? v.x - c : 0.0f, d1 = 4 * j + 1 < nw ? v.y - c : 0.0f;
        const float d2 = 4 * j + 2 < nw ? v.z - c : 0.0f, d3 = 4 * j + 3 < nw ? v.w - c : 0.0f;
        s1 += d0; s2 = __builtin_fmaf(d0, d0, s2);
        s1 += d1; s2 = __builtin_fmaf(d1, d1, s2);
        s1 += d2; s2 = __builtin_fmaf(d2, d2, s2);
        s1 += d3; s2 = __builtin_fmaf(d3, d3, s2);
    }
    // the four blocks' (count, mean, M2) to the row's first lane, combined there in float64 in block order
    // (the pairwise update of Chan et al.)
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int from = (t & 60) + k;                    // lane of the row's block k
        const float ck = __shfl(c, from), ak = __shfl(s1, from), bk = __shfl(s2, from);
        int nk = n - (n0 + 32 * k);
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

constexpr int FP_GC_THREADS = 256;
constexpr int FP_GC_ROWS = FP_GC_THREADS / APN_WAVE;

// gc[row] = sum_i gy[row][i] for the rows = B * O rows of n floats: one wave per row.  Lane l adds its elements
// l, l + 64, ... in ascending order; the 64 lane sums then meet in a fixed xor butterfly (every lane ends with the same
// total: float addition commutes, and the pairing is fixed).  One owner per output, no atomic: the same bits on every run.
__global__ __launch_bounds__(FP_GC_THREADS) void fp_cond_grad_kernel(long long rows, int n, const float *__restrict__ gy,
                                                                     float *__restrict__ gc) {
    const int lane = threadIdx.x % APN_WAVE;
    const long long row = (long long)blockIdx.x * FP_GC_ROWS + threadIdx.x / APN_WAVE;
    if (row >= rows) return;                           // wave-uniform
    const float *src = gy + (size_t)row * n;
    float s = 0.0f;
    for (int i = lane; i < n; i += APN_WAVE) s += src[i];
#pragma unroll
    for (int k = APN_WAVE / 2; k > 0; k >>= 1) s += __shfl_xor(s, k, APN_WAVE);
    if (lane == 0) gc[row] = s;
}

static int fp_blend_launch(int b, int o, int m, int n, const float *a, const float *u, const int *idx, const float *weight,
                           float *y, float *part, int training, const float *gamma, const float *beta,
                           const float *run_mean, const float *run_var, float eps, int relu, float *stat, float *out,
                           const float *cvec, void *stream) {
    if (b < 0 || o < 0 || m < 0 || n < 0 || b > 65535) return APN_EINVAL;
    if (b == 0 || o == 0 || n == 0) return APN_OK;
    if (m == 0 || !u || !idx || !weight) return APN_EINVAL;
    if (training ? (!y || !part) : (!out || !run_mean || !run_var)) return APN_EINVAL;
    const dim3 grid((n + FP_T - 1) / FP_T, (o + FP_OC - 1) / FP_OC, b);
    if (grid.y > 65535) return APN_EINVAL;
    hipLaunchKernelGGL(fp_blend_stats_kernel, grid, dim3(FP_THREADS), 0, (hipStream_t)stream, o, m, n, a, u, idx, weight,
                       y, part, training, gamma, beta, run_mean, run_var, eps, relu, stat, out, cvec);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

}  // namespace apn

extern "C" int apn_fp_blend_stats(int b, int o, int m, int n, const float *a, const float *u, const int *idx,
                                  const float *weight, float *y, float *part, int training, const float *gamma,
                                  const float *beta, const float *run_mean, const float *run_var, float eps, int relu,
                                  float *stat, float *out, void *stream) {
    return apn::fp_blend_launch(b, o, m, n, a, u, idx, weight, y, part, training, gamma, beta, run_mean, run_var, eps, relu,
                                stat, out, nullptr, stream);
}

extern "C" int apn_fp_blend_stats_cond(int b, int o, int m, int n, const float *a, const float *u, const int *idx,
                                       const float *weight, const float *c, float *y, float *part, int training,
                                       const float *gamma, const float *beta, const float *run_mean,
                                       const float *run_var, float eps, int relu, float *stat, float *out, void *stream) {
    if (b < 0 || o < 0 || m < 0 || n < 0 || b > 65535) return APN_EINVAL;
    if (b == 0 || o == 0 || n == 0) return APN_OK;
    if (!c) return APN_EINVAL;
    return apn::fp_blend_launch(b, o, m, n, a, u, idx, weight, y, part, training, gamma, beta, run_mean, run_var, eps, relu,
                                stat, out, c, stream);
}

extern "C" int apn_fp_cond_grad(int b, int o, int n, const float *gy, float *gc, void *stream) {
    using namespace apn;
    if (b < 0 || o < 0 || n < 0 || b > 65535) return APN_EINVAL;
    if (b == 0 || o == 0) return APN_OK;
    if (!gc || (n > 0 && !gy)) return APN_EINVAL;
    const long long rows = (long long)b * o;
    const long long blocks = (rows + FP_GC_ROWS - 1) / FP_GC_ROWS;
    if (blocks > 2147483647LL) return APN_EINVAL;
    hipLaunchKernelGGL(fp_cond_grad_kernel, dim3((unsigned)blocks), dim3(FP_GC_THREADS), 0, (hipStream_t)stream, rows, n, gy,
                       gc);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
