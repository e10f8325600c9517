// randla.hip -- RandLA-Net's LocalSpatialEncoding + AttentivePooling as one layer (gfx950).
//
// The reference composes, per layer: a (B,10,N,K) encoding e = [p_n, p_j, p_n - p_j, dist], a 10 -> C convolution, a
// training-mode BatchNorm2d over (B,C,N,K), ReLU, a concatenation with the centre's features to (B,2C,N,K), a 2C x 2C
// linear layer per (point, neighbour) pair, a softmax over K and a weighted sum.  Two identities leave
//
//      h_k = relu(W' (e_k - mu) + b')              W', b': BatchNorm folded into the convolution, mu: the encoding's
//                                                  batch mean (apn_rl_fold; zero on running statistics)
//      pooled[c] = sum_k softmax_k((A_hh h_k)[c]) h_k[c]           A_hh: the top-left C x C block of the score weight
//
// and the BatchNorm statistics follow from the encoding's 10 sums and 55 products over all pairs (apn_rl_moments).
// No (B,C,N,K) tensor exists: e, h, the logits and the scores live in registers and LDS.
//
// A tile is 64 (point, neighbour) columns: K is padded to Kp, the next power of two, and a tile holds 64 / Kp points;
// lane l of every wave is column l (point l / Kp, neighbour l % Kp), wave g owns the channels [g C/4, (g+1) C/4).
// The contraction A_hh H is fp32 vector code: a lane reads its column of H from LDS (one read per input channel) and
// the weights are wave-uniform (scalar loads), C/4 accumulators per lane.  The softmax and the pooled sum are
// butterflies over the Kp lanes of a point (the same bits in every lane, an order fixed by Kp alone).
//
// Sums that cross workgroups are per-workgroup partial rows added by a second launch (the fold is csrc/col_sums.hip's,
// at 8 lanes, float64 out): no atomics, no memset, no workgroup waits for another; two runs give the same bits.
#include "apn_common.h"

namespace apn {

constexpr int RL_THREADS = 256;
constexpr int RL_TILE = 64;            // columns of a tile = lanes of a wave
constexpr int RL_E = 10;               // the encoding's width
constexpr int RL_MOM = 65;             // 10 sums + 55 products
constexpr int RL_K_MAX = 32;
constexpr int RL_MOM_ROWS_MAX = 512;
constexpr long long RL_POINTS_LIMIT = 1ll << 24;

__host__ __device__ constexpr int rl_tri(int i, int j) {          // i <= j: the product's place after the 10 sums
    return RL_E + i * RL_E - i * (i - 1) / 2 + (j - i);
}

// element (channel c, column j) of an LDS tile: groups of four columns are swizzled by the channel, so that lanes
// reading consecutive channels at one column group spread over the banks, 64 lanes reading one channel's 64 columns hit
// every bank twice, and four consecutive columns (j % 4 == 0) stay one aligned 16-byte read in their own order
__device__ __forceinline__ int rl_at(int c, int j) { return c * RL_TILE + (j ^ ((c & 7) << 2)); }
__device__ __forceinline__ float4 rl_at4(const float *tile, int c, int j4) {
    return *reinterpret_cast<const float4 *>(tile + rl_at(c, 4 * j4));
}

// The encoding of one (point, neighbour) pair.  idx is clamped into the cloud.
__device__ __forceinline__ void rl_encode(long long pt, int kk, int n, int k, const float *__restrict__ coords,
                                          const int *__restrict__ idx, const float *__restrict__ dist, int sqrt_dist,
                                          float e[RL_E]) {
    const long long b = pt / n;
    int j = idx[pt * k + kk];
    j = j < 0 ? 0 : (j >= n ? n - 1 : j);
    const float *ci = coords + pt * 3;
    const float *cj = coords + (b * n + j) * 3;
    float d = dist[pt * k + kk];
    if (sqrt_dist) d = __builtin_sqrtf(d > 0.0f ? d : 0.0f);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = ci[a], y = cj[a];
        e[a] = x;
        e[3 + a] = y;
        e[6 + a] = x - y;
    }
    e[9] = d;
}

// ------------------------------------------------------------------------------------------------ moments
// part[row][65] (float64): the row's share of {sum e_i, sum e_i e_j (i <= j)}; a thread takes the pairs
// row * 256 + t, + rows * 256, ... in ascending order, the lanes of a wave are added by a butterfly, the waves ascending.
__global__ __launch_bounds__(RL_THREADS) void rl_moments_kernel(long long pairs, int n, int k,
                                                                const float *__restrict__ coords,
                                                                const int *__restrict__ idx,
                                                                const float *__restrict__ dist, int sqrt_dist,
                                                                double *__restrict__ part) {
    __shared__ double red[RL_THREADS / 64][RL_MOM];
    double acc[RL_MOM];
#pragma unroll
    for (int i = 0; i < RL_MOM; ++i) acc[i] = 0.0;
    const long long step = (long long)gridDim.x * RL_THREADS;
    for (long long q = (long long)blockIdx.x * RL_THREADS + threadIdx.x; q < pairs; q += step) {
        float e[RL_E];
        const long long pt = q / k;
        rl_encode(pt, (int)(q - pt * k), n, k, coords, idx, dist, sqrt_dist, e);
#pragma unroll
        for (int i = 0; i < RL_E; ++i) {
            acc[i] += (double)e[i];
#pragma unroll
            for (int j = i; j < RL_E; ++j) acc[rl_tri(i, j)] += (double)e[i] * (double)e[j];
        }
    }
#pragma unroll
    for (int i = 0; i < RL_MOM; ++i) {
        double v = acc[i];
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
        acc[i] = v;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < RL_MOM; ++i) red[threadIdx.x >> 6][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < RL_MOM) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < RL_THREADS / 64; ++w) v += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * RL_MOM + threadIdx.x] = v;
    }
}

// BatchNorm folded into the convolution, one thread per channel.  Training: the batch mean / biased variance from the
// moments, the running buffers updated as nn.BatchNorm2d does; eval: the running buffers.
// wf[C][10] | wf[10 C + c] | wf[11 C + i] = W', b', mu (the encoding's batch mean in training, zeros in eval: the hidden
// value is relu(W' (e - mu) + b'), centred before it is scaled so that a constant encoding normalises to exactly zero);
// stat[c], [C + c], [2C + c] = the mean, the variance and 1 / sqrt(var + eps) used.
__global__ __launch_bounds__(128) void rl_fold_kernel(int c_n, const double *__restrict__ mom, double count,
                                                      const float *__restrict__ w, const float *__restrict__ bias,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      float eps, float momentum, int training, float *running_mean,
                                                      float *running_var, long long *num_batches_tracked,
                                                      float *__restrict__ wf, double *__restrict__ stat) {
    const int c = threadIdx.x;
    if (c < RL_E) wf[c_n * (RL_E + 1) + c] = training ? (float)(mom[c] / count) : 0.0f;
    if (c >= c_n) return;
    double wc[RL_E];
#pragma unroll
    for (int i = 0; i < RL_E; ++i) wc[i] = (double)w[c * RL_E + i];
    const double b = bias ? (double)bias[c] : 0.0;
    double mean, var, wmu = 0.0;
    if (training) {
        double mu[RL_E];
#pragma unroll
        for (int i = 0; i < RL_E; ++i) {
            mu[i] = mom[i] / count;
            wmu += wc[i] * mu[i];
        }
        var = 0.0;
#pragma unroll
        for (int i = 0; i < RL_E; ++i) {
#pragma unroll
            for (int j = i; j < RL_E; ++j) {
                const double s = mom[rl_tri(i, j)] / count - mu[i] * mu[j];
                var += (i == j ? 1.0 : 2.0) * wc[i] * wc[j] * s;
            }
        }
        var = var > 0.0 ? var : 0.0;
        mean = wmu + b;
        if (running_mean && running_var) {
            const double m = (double)momentum;
            const double unbiased = var * (count / (count > 1.0 ? count - 1.0 : 1.0));
            running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
            running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * unbiased);
            if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
        }
    } else {
        mean = (double)running_mean[c];
        var = (double)running_var[c];
    }
    const double rstd = 1.0 / __builtin_sqrt(var + (double)eps);
    const double sc = (gamma ? (double)gamma[c] : 1.0) * rstd;
#pragma unroll
    for (int i = 0; i < RL_E; ++i) wf[c * RL_E + i] = (float)(sc * wc[i]);
    const double be = beta ? (double)beta[c] : 0.0;
    wf[c_n * RL_E + c] = (float)(training ? be : be + sc * (b - mean));
    stat[c] = mean;
    stat[c_n + c] = var;
    stat[2 * c_n + c] = rstd;
}

// ------------------------------------------------------------------------------------------------ the layer
// What forward and backward share: the tile's columns, h into LDS and registers, the logits, the scores and the pooled
// value.  hreg / sreg / preg [C/4]: this lane's column, this wave's channels.
template <int C>
struct RlTile {
    static constexpr int CG = C / 4;
    bool valid, point_ok;
    long long pt;
    int kk;
    float e[RL_E];

    __device__ __forceinline__ void locate(long long tile, int kp_log2, int k, long long points, int lane) {
        pt = tile * (RL_TILE >> kp_log2) + (lane >> kp_log2);
        kk = lane & ((1 << kp_log2) - 1);
        point_ok = pt < points;
        valid = point_ok && kk < k;
    }

    __device__ __forceinline__ void hidden(int g, int lane, int n, int k, const float *__restrict__ coords,
                                           const int *__restrict__ idx, const float *__restrict__ dist, int sqrt_dist,
                                           const float *__restrict__ wf, float *H, float hreg[CG]) {
#pragma unroll
        for (int i = 0; i < RL_E; ++i) e[i] = 0.0f;
        if (valid) {
            rl_encode(pt, kk, n, k, coords, idx, dist, sqrt_dist, e);
#pragma unroll
            for (int i = 0; i < RL_E; ++i) e[i] -= wf[C * (RL_E + 1) + i];          // centred: e - mu
        }
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) {
            const int c = g * CG + ci;
            float acc = wf[C * RL_E + c];
#pragma unroll
            for (int i = 0; i < RL_E; ++i) acc = __builtin_fmaf(wf[c * RL_E + i], e[i], acc);
            const float h = valid ? (acc > 0.0f ? acc : 0.0f) : 0.0f;
            hreg[ci] = h;
            H[rl_at(c, lane)] = h;
        }
    }

    // logits of this wave's channels at this lane's column: at[c2][c] = A_hh[c][c2]
    __device__ __forceinline__ void logits(int g, int lane, const float *__restrict__ at, const float *H, float lg[CG]) {
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) lg[ci] = 0.0f;
#pragma unroll 4
        for (int c2 = 0; c2 < C; ++c2) {
            const float hv = H[rl_at(c2, lane)];
            const float *row = at + c2 * C + g * CG;
#pragma unroll
            for (int ci = 0; ci < CG; ++ci) lg[ci] = __builtin_fmaf(row[ci], hv, lg[ci]);
        }
    }

    // softmax over the point's Kp lanes and the pooled sum: the same bits in every lane of the point
    __device__ __forceinline__ void pool(int kp, float l, float h, float &s, float &p) const {
        float m = valid ? l : -__builtin_inff();
        for (int w = 1; w < kp; w <<= 1) m = __builtin_fmaxf(m, __shfl_xor(m, w));
        const float ex = valid ? expf(l - m) : 0.0f;
        float den = ex;
        for (int w = 1; w < kp; w <<= 1) den += __shfl_xor(den, w);
        s = valid ? ex / den : 0.0f;
        p = s * h;
        for (int w = 1; w < kp; w <<= 1) p += __shfl_xor(p, w);
    }
};

template <int C>
__global__ __launch_bounds__(RL_THREADS) void rl_fwd_kernel(long long points, int n, int k, int kp_log2,
                                                            const float *__restrict__ coords,
                                                            const int *__restrict__ idx, const float *__restrict__ dist,
                                                            int sqrt_dist, const float *__restrict__ wf,
                                                            const float *__restrict__ at, float *__restrict__ pooled) {
    constexpr int CG = C / 4;
    __shared__ float H[C * RL_TILE];
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    RlTile<C> t;
    t.locate((long long)blockIdx.x, kp_log2, k, points, lane);
    float hreg[CG], lg[CG];
    t.hidden(g, lane, n, k, coords, idx, dist, sqrt_dist, wf, H, hreg);
    __syncthreads();
    t.logits(g, lane, at, H, lg);
    const long long b = t.pt / n, pn = t.pt - b * n;
#pragma unroll
    for (int ci = 0; ci < CG; ++ci) {
        float s, p;
        t.pool(1 << kp_log2, lg[ci], hreg[ci], s, p);
        if (t.point_ok && t.kk == 0) pooled[(b * C + g * CG + ci) * n + pn] = p;
    }
}

// Backward: one pass that recomputes h, the logits and the scores per tile and leaves, per workgroup, a row
// part[row][C C + 11 C] (float32): the shares of dA_hh[c][c2] = sum dl[c] h[c2], and per channel of
// {sum dy (e - mu)_0..9, sum dy}, dy = dL/d(the BatchNorm's output).  A workgroup takes the tiles row, row + rows, ...
template <int C>
__global__ __launch_bounds__(RL_THREADS) void rl_bwd_kernel(long long points, long long tiles, int n, int k, int kp_log2,
                                                            const float *__restrict__ coords,
                                                            const int *__restrict__ idx, const float *__restrict__ dist,
                                                            int sqrt_dist, const float *__restrict__ wf,
                                                            const float *__restrict__ a, const float *__restrict__ at,
                                                            const float *__restrict__ dpooled, float *__restrict__ part) {
    constexpr int CG = C / 4;
    constexpr int TR = C >= 16 ? 16 : 8;        // threads per side of the dA_hh grid
    constexpr int R = C / TR;                   // channels per thread and side (strided by TR)
    constexpr int HROWS = C < RL_E + 1 ? RL_E + 1 : C;
    constexpr int SOUT = (C * (RL_E + 1) + RL_THREADS - 1) / RL_THREADS;
    constexpr int WIDTH = C * C + C * (RL_E + 1);
    __shared__ __attribute__((aligned(16))) float H[HROWS * RL_TILE];        // h; later the tile's encodings and a row of ones
    __shared__ __attribute__((aligned(16))) float D[C * RL_TILE];            // dl; later dy
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = threadIdx.x;
    const bool da_on = tid < TR * TR;
    const int bc = tid / TR, bc2 = tid % TR;
    float da[R][R], sacc[SOUT];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) da[i][j] = 0.0f;
#pragma unroll
    for (int r = 0; r < SOUT; ++r) sacc[r] = 0.0f;

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        RlTile<C> t;
        t.locate(tile, kp_log2, k, points, lane);
        float hreg[CG], lg[CG], dyd[CG];
        t.hidden(g, lane, n, k, coords, idx, dist, sqrt_dist, wf, H, hreg);
        __syncthreads();
        t.logits(g, lane, at, H, lg);
        const long long b = t.pt / n, pn = t.pt - b * n;
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) {
            float s, p;
            t.pool(1 << kp_log2, lg[ci], hreg[ci], s, p);
            const float go = t.point_ok ? dpooled[(b * C + g * CG + ci) * n + pn] : 0.0f;
            const float gs = go * s;
            D[rl_at(g * CG + ci, lane)] = gs * (hreg[ci] - p);          // dl = s go (h - pooled)
            dyd[ci] = gs;                                               // the direct term of dh
        }
        __syncthreads();
        if (da_on) {
#pragma unroll 2
            for (int j4 = 0; j4 < RL_TILE / 4; ++j4) {
                float4 dv[R], hv[R];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    dv[i] = rl_at4(D, i * TR + bc, j4);
                    hv[i] = rl_at4(H, i * TR + bc2, j4);
                }
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int i2 = 0; i2 < R; ++i2) {
                        float acc = da[i][i2];
                        acc = __builtin_fmaf(dv[i].x, hv[i2].x, acc);
                        acc = __builtin_fmaf(dv[i].y, hv[i2].y, acc);
                        acc = __builtin_fmaf(dv[i].z, hv[i2].z, acc);
                        da[i][i2] = __builtin_fmaf(dv[i].w, hv[i2].w, acc);
                    }
            }
        }
        float dh[CG];
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) dh[ci] = 0.0f;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {                                   // dh[c2] += sum_c A_hh[c][c2] dl[c]
            const float dv = D[rl_at(c, lane)];
            const float *row = a + c * C + g * CG;
#pragma unroll
            for (int ci = 0; ci < CG; ++ci) dh[ci] = __builtin_fmaf(row[ci], dv, dh[ci]);
        }
        __syncthreads();
#pragma unroll
        for (int ci = 0; ci < CG; ++ci)
            D[rl_at(g * CG + ci, lane)] = hreg[ci] > 0.0f ? dh[ci] + dyd[ci] : 0.0f;
        if (g == 0) {
#pragma unroll
            for (int i = 0; i < RL_E; ++i) H[i * RL_TILE + lane] = t.e[i];
            H[RL_E * RL_TILE + lane] = 1.0f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < SOUT; ++r) {
            const int o = tid + r * RL_THREADS;
            if (o < C * (RL_E + 1)) {
                const int c = o / (RL_E + 1), i = o - c * (RL_E + 1);
                float acc = sacc[r];
#pragma unroll 4
                for (int j4 = 0; j4 < RL_TILE / 4; ++j4) {
                    const float4 dv = rl_at4(D, c, j4);
                    const float4 ev = *reinterpret_cast<const float4 *>(H + i * RL_TILE + 4 * j4);
                    acc = __builtin_fmaf(dv.x, ev.x, acc);
                    acc = __builtin_fmaf(dv.y, ev.y, acc);
                    acc = __builtin_fmaf(dv.z, ev.z, acc);
                    acc = __builtin_fmaf(dv.w, ev.w, acc);
                }
                sacc[r] = acc;
            }
        }
        __syncthreads();
    }
    float *row = part + (size_t)blockIdx.x * WIDTH;
    if (da_on) {
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int i2 = 0; i2 < R; ++i2) row[(i * TR + bc) * C + i2 * TR + bc2] = da[i][i2];
    }
#pragma unroll
    for (int r = 0; r < SOUT; ++r) {
        const int o = tid + r * RL_THREADS;
        if (o < C * (RL_E + 1)) row[C * C + o] = sacc[r];
    }
}

// From the folded rows (sums, float64): the BatchNorm / convolution algebra of one layer,
// grads = dA_hh [C C] | dgamma [C] | dbeta [C] | dW1 [C 10] | db1 [C]  (float32).
__global__ __launch_bounds__(RL_THREADS) void rl_finalize_kernel(int c_n, const double *__restrict__ sums,
                                                                 const double *__restrict__ mom, double count,
                                                                 const float *__restrict__ w,
                                                                 const float *__restrict__ bias,
                                                                 const float *__restrict__ gamma,
                                                                 const double *__restrict__ stat, int training,
                                                                 float *__restrict__ grads) {
    const int cc = c_n * c_n;
    const int o = blockIdx.x * RL_THREADS + threadIdx.x;
    if (o < cc) {
        grads[o] = (float)sums[o];
        return;
    }
    const int c = o - cc;
    if (c >= c_n) return;
    double ge[RL_E + 1];
#pragma unroll
    for (int i = 0; i <= RL_E; ++i) ge[i] = sums[cc + c * (RL_E + 1) + i];
    const double sum_g = ge[RL_E];
    const double mean = stat[c], rstd = stat[2 * c_n + c];
    const double gm = gamma ? (double)gamma[c] : 1.0;
    double wc[RL_E], wge = 0.0;
#pragma unroll
    for (int i = 0; i < RL_E; ++i) {
        wc[i] = (double)w[c * RL_E + i];
        wge += wc[i] * ge[i];
    }
    float *dgamma = grads + cc, *dbeta = dgamma + c_n, *dw = dbeta + c_n, *db = dw + c_n * RL_E;
    dbeta[c] = (float)sum_g;
    if (training) {
        // ge = sum dy (e - mu);  xhat = rstd w.(e - mu): sum dy xhat = rstd w.ge;  sum xhat (e - mu)_i = count rstd (Sigma w)_i
        double mu[RL_E];
#pragma unroll
        for (int i = 0; i < RL_E; ++i) mu[i] = mom[i] / count;
        const double dg = rstd * wge;
        dgamma[c] = (float)dg;
#pragma unroll
        for (int i = 0; i < RL_E; ++i) {
            double sw = 0.0;
#pragma unroll
            for (int j = 0; j < RL_E; ++j) {
                const int t = i <= j ? rl_tri(i, j) : rl_tri(j, i);
                sw += (mom[t] / count - mu[i] * mu[j]) * wc[j];
            }
            dw[c * RL_E + i] = (float)(gm * rstd * (ge[i] - dg * rstd * sw));
        }
        db[c] = 0.0f;                    // a bias in front of a training-mode BatchNorm has no gradient
    } else {
        const double b = bias ? (double)bias[c] : 0.0;
        dgamma[c] = (float)(rstd * (wge + (b - mean) * sum_g));
#pragma unroll
        for (int i = 0; i < RL_E; ++i) dw[c * RL_E + i] = (float)(gm * rstd * ge[i]);
        db[c] = (float)(gm * rstd * sum_g);
    }
}

static bool rl_shape_ok(int b, int n, int k) {
    return b >= 0 && n >= 1 && k >= 1 && k <= RL_K_MAX && (long long)b * n < RL_POINTS_LIMIT;
}
static bool rl_width_ok(int c) { return c == 8 || c == 16 || c == 32 || c == 64 || c == 128; }

static int rl_kp_log2(int k) {
    int l = 0;
    while ((1 << l) < k) ++l;
    return l;
}
static long long rl_tiles(int b, int n, int k) {
    const long long per = RL_TILE >> rl_kp_log2(k);
    return ((long long)b * n + per - 1) / per;
}
static int rl_moment_rows(int b, int n, int k) {
    const long long want = ((long long)b * n * k + 8 * RL_THREADS - 1) / (8 * RL_THREADS);
    return (int)(want < 1 ? 1 : (want > RL_MOM_ROWS_MAX ? RL_MOM_ROWS_MAX : want));
}
// backward's workgroups: one per tile up to a cap that keeps the partial rows (C C + 11 C floats each) small
static int rl_bwd_rows(int b, int n, int k, int c) {
    const long long tiles = rl_tiles(b, n, k);
    const int cap = c <= 32 ? 1024 : (c == 64 ? 512 : 256);
    return (int)(tiles < cap ? tiles : cap);
}

}  // namespace apn

using namespace apn;

#define RL_DISPATCH(c, KERNEL, grid, ...)                                                                          \
    switch (c) {                                                                                                   \
    case 8: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(RL_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;     \
    case 16: hipLaunchKernelGGL(KERNEL<16>, grid, dim3(RL_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;   \
    case 32: hipLaunchKernelGGL(KERNEL<32>, grid, dim3(RL_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;   \
    case 64: hipLaunchKernelGGL(KERNEL<64>, grid, dim3(RL_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;   \
    default: hipLaunchKernelGGL(KERNEL<128>, grid, dim3(RL_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); break;  \
    }

extern "C" int apn_rl_moment_rows(int b, int n, int k) {
    return rl_shape_ok(b, n, k) && b > 0 ? rl_moment_rows(b, n, k) : 0;
}

extern "C" int apn_rl_bwd_rows(int b, int n, int k, int c) {
    return rl_shape_ok(b, n, k) && rl_width_ok(c) && b > 0 ? rl_bwd_rows(b, n, k, c) : 0;
}

extern "C" int apn_rl_moments(int b, int n, int k, const float *coords, const int *idx, const float *dist,
                              int sqrt_dist, double *part, double *mom, void *stream) {
    if (!rl_shape_ok(b, n, k)) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!coords || !idx || !dist || !part || !mom) return APN_EINVAL;
    const int rows = rl_moment_rows(b, n, k);
    hipLaunchKernelGGL(rl_moments_kernel, dim3(rows), dim3(RL_THREADS), 0, (hipStream_t)stream, (long long)b * n * k, n,
                       k, coords, idx, dist, sqrt_dist, part);
    APN_LAUNCH_CHECK();
    return col_sums((const double *)part, rows, (size_t)RL_MOM, 8, mom, -1.0, (hipStream_t)stream);
}

extern "C" int apn_rl_fold(int c, const double *mom, double count, const float *w, const float *bias,
                           const float *gamma, const float *beta, float eps, float momentum, int training,
                           float *running_mean, float *running_var, long long *num_batches_tracked, float *wf,
                           double *stat, void *stream) {
    if (!rl_width_ok(c) || !(count >= 1.0) || !(eps >= 0.0f)) return APN_EINVAL;
    if (!w || !wf || !stat) return APN_EINVAL;
    if (training ? !mom : (!running_mean || !running_var)) return APN_EINVAL;
    if ((running_mean == nullptr) != (running_var == nullptr)) return APN_EINVAL;
    hipLaunchKernelGGL(rl_fold_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, c, mom, count, w, bias, gamma, beta,
                       eps, momentum, training, running_mean, running_var, num_batches_tracked, wf, stat);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_rl_forward(int b, int n, int k, int c, const float *coords, const int *idx, const float *dist,
                              int sqrt_dist, const float *wf, const float *at, float *pooled, void *stream) {
    if (!rl_shape_ok(b, n, k) || !rl_width_ok(c)) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!coords || !idx || !dist || !wf || !at || !pooled) return APN_EINVAL;
    const dim3 grid((unsigned)rl_tiles(b, n, k));
    RL_DISPATCH(c, rl_fwd_kernel, grid, (long long)b * n, n, k, rl_kp_log2(k), coords, idx, dist, sqrt_dist, wf, at,
                pooled);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_rl_backward(int b, int n, int k, int c, const float *coords, const int *idx, const float *dist,
                               int sqrt_dist, const float *wf, const float *a, const float *at, const float *dpooled,
                               float *part, void *stream) {
    if (!rl_shape_ok(b, n, k) || !rl_width_ok(c)) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!coords || !idx || !dist || !wf || !a || !at || !dpooled || !part) return APN_EINVAL;
    const dim3 grid(rl_bwd_rows(b, n, k, c));
    RL_DISPATCH(c, rl_bwd_kernel, grid, (long long)b * n, rl_tiles(b, n, k), n, k, rl_kp_log2(k), coords, idx, dist,
                sqrt_dist, wf, a, at, dpooled, part);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_rl_finalize(int c, int rows, const float *part, const double *mom, double count, const float *w,
                               const float *bias, const float *gamma, const double *stat, int training, double *sums,
                               float *grads, void *stream) {
    if (!rl_width_ok(c) || rows < 0 || rows > 1024 || !(count >= 1.0)) return APN_EINVAL;
    if (!w || !stat || !sums || !grads || (rows > 0 && !part) || (training && !mom)) return APN_EINVAL;
    const int outs = c * c + c, width = c * c + c * (RL_E + 1);
    if (const int e = col_sums(part, rows, (size_t)width, 8, sums, -1.0, (hipStream_t)stream)) return e;
    hipLaunchKernelGGL(rl_finalize_kernel, dim3((outs + RL_THREADS - 1) / RL_THREADS), dim3(RL_THREADS), 0,
                       (hipStream_t)stream, c, (const double *)sums, mom, count, w, bias, gamma, stat, training, grads);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
