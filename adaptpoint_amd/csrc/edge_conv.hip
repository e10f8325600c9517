// edge_conv.hip -- the position-level work of a DGCNN EdgeConv block (openpoints/models/layers/graph_conv.py:38-51),
//
//     out[b,:,i] = act(bn(max_k W [x_i ; x_j(i,k) - x_i])),   W = [Wa | Wb] (H x 2C),  act = LeakyReLU(slope)
//     (slope == 0, ReLU, and a residual behind the activation through apn_ec_out_res / apn_ec_bwd_prep_act: DeepGCN)
//
// The convolution is linear in [x_i ; x_j - x_i], so it is hoisted to the points: u = (Wa - Wb) x, v = Wb x (one
// contraction, csrc/pointwise.hip, rows [u | v] of pitch ld >= 2H), y[i,k] = u_i + v_j(i,k).  BatchNorm + LeakyReLU
// is monotone per channel with the sign of gamma (slope >= 0: non-decreasing is enough), so the extremum over K commutes with them:
//
//     out[b,c,i] = act(scale_c ext_k y[i,k][c] + shift_c),   ext = max (gamma_c >= 0) | min
//
// No (B,2C,N,K) or (B,H,N,K) tensor exists, forward or backward.
//
//   ec_pool_fwd   one wave per query, a lane per VEC consecutive channels: the extremum of y over the query's K
//                 neighbours (every slot counts, repeated neighbours once per occurrence -- as in the composed path)
//                 and the slot that holds it (the FIRST slot among equals, as torch.max), and -- training --
//                 ysum[i] = sum_k y[i,k] and the query's share of sum y^2: float32 over the query's K positions,
//                 float64 across queries, one float64 partial row per workgroup (apn_la_stats_fold adds them).
//   ec_out        out (B,H,N) = act(scale ext + shift), channels first, through an LDS tile.
//   ec_bwd_prep   g (B,H,N; any strides) through the activation's slope -> gsel (B,N,H) = g act' scale, and
//                 partS = {sum g act', sum g act' yhat_sel} rows (apn_sa_wide_consts2's input).
//   ec_csr_*      the reverse-neighbour lists of idx (B,N,K): pcnt / poff per point, plist = the positions
//                 (b N + i) K + k that gather the point, ASCENDING.  Counts and cursors by integer atomics
//                 (order-free); every list is then ranked into place by its point's wave, so the result is a pure
//                 function of idx.  Kernels only (no memset): the index step replays from a captured hipGraph.
//   ec_pool_bwd   one wave per point j.  With dL/dy[i,k] = gsel_i [k == sel_i] + D y[i,k] + E (BatchNorm's dense
//                 term, D = E = 0 in eval mode):
//                     du_i = gsel_i + D ysum_i + K E
//                     dv_j = sum over the list of j { gsel_i [k == sel_i] } + D (sum over the list u_i + cnt_j v_j) + cnt_j E
//                 both sums in list order (fixed): no float atomics, bit-identical from run to run.  Written as rows
//                 [du | dv] of pitch 2H: dL/dx = [Wa - Wb ; Wb]^T [du | dv]^T and the weight gradients are
//                 contractions of that one buffer.
#include "apn_common.h"
#include "reverse_lists.h"

namespace apn {

constexpr int EC_QPB = 64;        // queries per workgroup of the forward pass (16 per wave)
constexpr int EC_KMAX = 64;       // neighbours per query: one idx row per wave

template <int VEC>
__device__ __forceinline__ void ec_load(const float *__restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC >= 4) {
#pragma unroll
        for (int j = 0; j < VEC / 4; ++j) {
            const float4 t = reinterpret_cast<const float4 *>(p)[j];
            v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
        }
    } else if constexpr (VEC == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        v[0] = t.x; v[1] = t.y;
    } else {
        v[0] = *p;
    }
}

template <int VEC>
__device__ __forceinline__ void ec_store(float *__restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC >= 4) {
#pragma unroll
        for (int j = 0; j < VEC / 4; ++j)
            reinterpret_cast<float4 *>(p)[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else {
        *p = v[0];
    }
}

// H = 64 VEC channels.  Grid: ceil(B N / 64) workgroups of 4 waves.  uv: rows [u (H) | v (H)] of pitch ld.
template <int VEC>
__global__ __launch_bounds__(256) void ec_pool_fwd_kernel(long long nq, int n, int K, const float *__restrict__ uv,
                                                          int ld, const int *__restrict__ idx,
                                                          const float *__restrict__ gamma, float *__restrict__ ext,
                                                          unsigned char *__restrict__ sel, float *__restrict__ ysum,
                                                          double *__restrict__ part) {
    constexpr int H = 64 * VEC;
    __shared__ double red[4][2 * H];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * VEC;
    float sg[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) sg[j] = (!gamma || gamma[c0 + j] >= 0.0f) ? 1.0f : -1.0f;
    double acc1[VEC], acc2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { acc1[j] = 0.0; acc2[j] = 0.0; }
    const long long q0 = (long long)blockIdx.x * EC_QPB + wave * (EC_QPB / 4);
    for (int qi = 0; qi < EC_QPB / 4; ++qi) {
        const long long gq = q0 + qi;
        if (gq >= nq) break;                                   // (wave-uniform)
        const long long base = (gq / n) * n;                   // the cloud's first point
        int nb = lane < K ? idx[gq * K + lane] : 0;
        nb = nb < 0 ? 0 : (nb >= n ? n - 1 : nb);              // (an index outside the cloud is never followed)
        float u[VEC], best[VEC], s1[VEC], s2[VEC];
        unsigned char bs[VEC];
        ec_load<VEC>(uv + gq * ld + c0, u);
        constexpr int G = VEC >= 8 ? 2 : 4;                    // rows in flight per step
        for (int k = 0; k < K; k += G) {
            float v[G][VEC];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const long long pt = base + __builtin_amdgcn_readlane(nb, k + g < K ? k + g : K - 1);
                ec_load<VEC>(uv + pt * ld + H + c0, v[g]);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (k + g >= K) break;                         // (wave-uniform)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float y = u[j] + v[g][j];
                    const float t = y * sg[j];
                    if (k + g == 0) {
                        best[j] = t; bs[j] = 0; s1[j] = y; s2[j] = y * y;
                    } else {
                        if (t > best[j]) { best[j] = t; bs[j] = (unsigned char)(k + g); }
                        s1[j] += y;
                        s2[j] = __builtin_fmaf(y, y, s2[j]);
                    }
                }
            }
        }
        float e[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            e[j] = best[j] * sg[j];
            sel[gq * H + c0 + j] = bs[j];
            acc1[j] += (double)s1[j];
            acc2[j] += (double)s2[j];
        }
        ec_store<VEC>(ext + gq * H + c0, e);
        if (ysum) ec_store<VEC>(ysum + gq * H + c0, s1);
    }
    if (!part) return;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        red[wave][c0 + j] = acc1[j];
        red[wave][H + c0 + j] = acc2[j];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < 2 * H; col += 256)
        part[(size_t)blockIdx.x * 2 * H + col] = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

__device__ __forceinline__ float ec_act_slope(float z, float slope) { return z > 0.0f ? 1.0f : slope; }

// out (B,H,N) = act(scale ext + shift) [+ res] from ext (B,N,H).  Block = 64 points x 64 channels through an LDS
// tile.  RES: res (B,H,N; element strides rs_*) is added after the activation (a ResDynBlock's `body(x) + x`).
template <bool RES>
__global__ __launch_bounds__(256) void ec_out_kernel(int n, int H, const float *__restrict__ ext,
                                                     const float *__restrict__ pack, float slope,
                                                     const float *__restrict__ res, long long rs_b, long long rs_c,
                                                     long long rs_n, float *__restrict__ out) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const float sc = pack[c0 + tx], sh = pack[H + c0 + tx];
    for (int pp = ty; pp < 64; pp += 4) {          // tile[point][channel]: coalesced along the channels
        const int p = p0 + pp;
        if (p < n) {
            const float z = __builtin_fmaf(sc, ext[((size_t)b * n + p) * H + c0 + tx], sh);
            tile[pp][tx] = z * ec_act_slope(z, slope);
        }
    }
    __syncthreads();
    const int p = p0 + tx;
    if (p < n)
        for (int cc = ty; cc < 64; cc += 4) {
            float o = tile[tx][cc];
            if constexpr (RES) {
                float r = res[b * rs_b + (long long)(c0 + cc) * rs_c + p * rs_n];
                asm volatile("" : "+v"(r));        // (one scalar add per element: the unrolled loop's adds are not paired)
                o += r;
            }
            out[((size_t)b * H + c0 + cc) * n + p] = o;
        }
}

// g (B,H,N; strides gs_*) -> gsel (B,N,H) = g act'(z) scale, z = scale ext + shift, and
// partS[b * tiles + tile][2H] = {sum g act', sum g act' yhat_sel}, yhat_sel = (ext - mean) invstd.
__global__ __launch_bounds__(256) void ec_bwd_prep_kernel(int n, int H, const float *__restrict__ g, long long gs_b,
                                                          long long gs_c, long long gs_n,
                                                          const float *__restrict__ ext,
                                                          const float *__restrict__ pack, float slope,
                                                          float *__restrict__ gsel, float *__restrict__ partS) {
    __shared__ float tile[64][65];
    __shared__ float red[2][4][64];
    const int b = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int cc = ty; cc < 64; cc += 4) {          // tile[c][point]: coalesced along the points
        const int p = p0 + tx;
        tile[cc][tx] = p < n ? g[b * gs_b + (long long)(c0 + cc) * gs_c + p * gs_n] : 0.0f;
    }
    __syncthreads();
    const int c = c0 + tx;
    const float sc = pack[c], sh = pack[H + c], mu = pack[2 * H + c], iv = pack[3 * H + c];
    float s1 = 0.0f, s2 = 0.0f;
    for (int pp = ty; pp < 64; pp += 4) {
        const int p = p0 + pp;
        if (p < n) {
            const size_t o = ((size_t)b * n + p) * H + c;
            const float e = ext[o];
            const float gv = tile[tx][pp] * ec_act_slope(__builtin_fmaf(sc, e, sh), slope);
            gsel[o] = gv * sc;
            s1 += gv;
            s2 = __builtin_fmaf(gv, (e - mu) * iv, s2);
        }
    }
    red[0][ty][tx] = s1;
    red[1][ty][tx] = s2;
    __syncthreads();
    if (ty == 0) {
        const size_t row = (size_t)b * gridDim.x + blockIdx.x;
        partS[row * 2 * H + c] = (red[0][0][tx] + red[0][1][tx]) + (red[0][2][tx] + red[0][3][tx]);
        partS[row * 2 * H + H + c] = (red[1][0][tx] + red[1][1][tx]) + (red[1][2][tx] + red[1][3][tx]);
    }
}

// ------------------------------------------------------------------------------------------ reverse neighbours
// (the init and scan kernels: csrc/reverse_lists.h)
// mq: gathering rows per cloud (n for the EdgeConv graph; apn_po_csr: all m rows gather from one set of n)
__device__ __forceinline__ long long ec_target(const int *__restrict__ idx, long long pos, int n, int mq, int K) {
    int nb = idx[pos];
    nb = nb < 0 ? 0 : (nb >= n ? n - 1 : nb);                  // the clamp of ec_pool_fwd
    return ((pos / K) / mq) * n + nb;
}

// one thread per position.  fill = 0: count; fill = 1: write the position behind its point's cursor.
__global__ __launch_bounds__(256) void ec_csr_count_fill_kernel(long long npos, int n, int mq, int K, int fill,
                                                                const int *__restrict__ idx, int *__restrict__ pcnt,
                                                                int *__restrict__ cursor, int *__restrict__ tmp) {
    const long long pos = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pos >= npos) return;
    const long long gj = ec_target(idx, pos, n, mq, K);
    if (!fill) atomicAdd(pcnt + gj, 1);
    else tmp[atomicAdd(cursor + gj, 1)] = (int)pos;
}

// one wave per point: the list's entries (distinct positions, in the order the fill's atomics ran) ranked into place
__global__ __launch_bounds__(256) void ec_csr_sort_kernel(long long npts, const int *__restrict__ pcnt,
                                                          const int *__restrict__ poff, const int *__restrict__ tmp,
                                                          int *__restrict__ plist) {
    const int lane = threadIdx.x & 63;
    const long long pt = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pt >= npts) return;
    const int cnt = pcnt[pt];
    const int *__restrict__ src = tmp + poff[pt];
    int *__restrict__ dst = plist + poff[pt];
    if (cnt <= 64) {
        const int e = lane < cnt ? src[lane] : 0x7fffffff;
        int rank = 0;
        for (int t = 0; t < cnt; ++t) rank += __builtin_amdgcn_readlane(e, t) < e ? 1 : 0;
        if (lane < cnt) dst[rank] = e;
        return;
    }
    for (int i = lane; i < cnt; i += 64) {
        const int e = src[i];
        int rank = 0;
        for (int t = 0; t < cnt; ++t) rank += src[t] < e ? 1 : 0;
        dst[rank] = e;
    }
}

// One wave per point.  uv: rows [u | v] of pitch ld; de = {D[H], E[H]}; duv: rows [du | dv] of pitch 2H.
template <int VEC>
__global__ __launch_bounds__(256) void ec_pool_bwd_kernel(long long npts, int K, const float *__restrict__ gsel,
                                                          const unsigned char *__restrict__ sel,
                                                          const int *__restrict__ pcnt, const int *__restrict__ poff,
                                                          const int *__restrict__ plist, const float *__restrict__ uv,
                                                          int ld, const float *__restrict__ ysum,
                                                          const float *__restrict__ de, float *__restrict__ duv) {
    constexpr int H = 64 * VEC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * VEC;
    const long long pt = (long long)blockIdx.x * 4 + wave;
    if (pt >= npts) return;
    const int cnt = pcnt[pt];
    const int *__restrict__ list = plist + poff[pt];
    const bool dense = ysum != nullptr;                          // training: BatchNorm's dense term
    float acc[VEC], us[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { acc[j] = 0.0f; us[j] = 0.0f; }
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int chunk = cnt - i0 < 64 ? cnt - i0 : 64;
        int q = 0, slot = 0;
        if (lane < chunk) {
            const int pos = list[i0 + lane];
            q = pos / K;
            slot = pos - q * K;
        }
        q = q < 0 ? 0 : ((long long)q >= npts ? (int)(npts - 1) : q);   // (a damaged list is never followed out of the arrays)
        constexpr int G = VEC >= 8 ? 2 : 4;
        for (int j = 0; j < chunk; j += G) {
            float g[G][VEC], u[G][VEC];
            unsigned char sb[G][VEC];
            int sj[G];
#pragma unroll
            for (int t = 0; t < G; ++t) {
                const int jj = j + t < chunk ? j + t : chunk - 1;
                const long long qj = (long long)__builtin_amdgcn_readlane(q, jj);
                sj[t] = __builtin_amdgcn_readlane(slot, jj);
                ec_load<VEC>(gsel + qj * H + c0, g[t]);
                if (dense) ec_load<VEC>(uv + qj * ld + c0, u[t]);
#pragma unroll
                for (int e = 0; e < VEC; ++e) sb[t][e] = sel[qj * H + c0 + e];
            }
#pragma unroll
            for (int t = 0; t < G; ++t) {
                if (j + t >= chunk) break;                     // (wave-uniform)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    acc[e] += (int)sb[t][e] == sj[t] ? g[t][e] : 0.0f;
                    if (dense) us[e] += u[t][e];
                }
            }
        }
    }
    float v[VEC], gown[VEC], ys[VEC], du[VEC], dv[VEC];
    ec_load<VEC>(uv + pt * ld + H + c0, v);
    ec_load<VEC>(gsel + pt * H + c0, gown);
    if (dense) {
        ec_load<VEC>(ysum + pt * H + c0, ys);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) ys[e] = 0.0f;
    }
    const float fc = (float)cnt;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const float D = de[c0 + e], E = de[H + c0 + e];
        du[e] = gown[e] + __builtin_fmaf(D, ys[e], (float)K * E);
        dv[e] = acc[e] + __builtin_fmaf(D, __builtin_fmaf(fc, v[e], us[e]), fc * E);
    }
    ec_store<VEC>(duv + pt * 2 * H + c0, du);
    ec_store<VEC>(duv + pt * 2 * H + H + c0, dv);
}

}  // namespace apn

using namespace apn;

static bool ec_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

// b clouds of n points, k neighbours: what every entry of this file accepts
static bool ec_sizes(int b, int n, int k) {
    return b >= 0 && n >= 0 && k >= 1 && k <= EC_KMAX && b <= 65535 && (long long)b * n < (1ll << 24);
}

extern "C" int apn_ec_pool_rows(int b, int n) {
    if (b <= 0 || n <= 0) return 0;
    return (int)(((long long)b * n + EC_QPB - 1) / EC_QPB);
}

extern "C" int apn_ec_pool_fwd(int b, int n, int c, int k, const float *uv, int ld, const int *idx, const float *gamma,
                               float *ext, void *sel, float *ysum, double *part, void *stream) {
    if (!ec_sizes(b, n, k) || !ec_width(c) || ld < 2 * c || (ld % 4)) return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!uv || !idx || !ext || !sel || ((ysum != nullptr) != (part != nullptr))) return APN_EINVAL;
    const long long nq = (long long)b * n;
    const dim3 grid((unsigned)((nq + EC_QPB - 1) / EC_QPB)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define APN_EC_FWD(VEC)                                                                                      \
    hipLaunchKernelGGL(ec_pool_fwd_kernel<VEC>, grid, block, 0, st, nq, n, k, uv, ld, idx, gamma, ext,       \
                       (unsigned char *)sel, ysum, part)
    switch (c / 64) {
        case 1: APN_EC_FWD(1); break;
        case 2: APN_EC_FWD(2); break;
        case 4: APN_EC_FWD(4); break;
        default: APN_EC_FWD(8); break;
    }
#undef APN_EC_FWD
    APN_LAUNCH_CHECK();
    return APN_OK;
}

// The output stage behind its entries' slope guards: sizes, the empty-work return, pointers, the launch
static int ec_out_launch(int b, int n, int c, const float *ext, const float *pack, float slope, const float *res,
                         long long rs_b, long long rs_c, long long rs_n, float *out, void *stream) {
    if (b < 0 || n < 0 || b > 65535 || c <= 0 || (c % 64) || c / 64 > 65535) return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!ext || !pack || !out) return APN_EINVAL;
    const dim3 grid((n + 63) / 64, c / 64, b);
    if (res)
        hipLaunchKernelGGL(ec_out_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, n, c, ext, pack, slope, res, rs_b,
                           rs_c, rs_n, out);
    else
        hipLaunchKernelGGL(ec_out_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, n, c, ext, pack, slope, nullptr,
                           0ll, 0ll, 0ll, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ec_out(int b, int n, int c, const float *ext, const float *pack, float slope, float *out,
                          void *stream) {
    if (!(slope > 0.0f)) return APN_EINVAL;
    return ec_out_launch(b, n, c, ext, pack, slope, nullptr, 0ll, 0ll, 0ll, out, stream);
}

// apn_ec_out with ReLU (slope == 0) allowed and an optional residual added behind the activation
extern "C" int apn_ec_out_res(int b, int n, int c, const float *ext, const float *pack, float slope, const float *res,
                              long long rs_b, long long rs_c, long long rs_n, float *out, void *stream) {
    if (!(slope >= 0.0f)) return APN_EINVAL;
    return ec_out_launch(b, n, c, ext, pack, slope, res, rs_b, rs_c, rs_n, out, stream);
}

extern "C" int apn_ec_bwd_prep_rows(int b, int n) { return (b <= 0 || n <= 0) ? 0 : b * ((n + 63) / 64); }

// The backward pass's first stage behind its entries' slope guards, as ec_out_launch
static int ec_bwd_prep_launch(int b, int n, int c, const float *g, long long gs_b, long long gs_c, long long gs_n,
                              const float *ext, const float *pack, float slope, float *gsel, float *part_s,
                              void *stream) {
    if (b < 0 || n < 0 || b > 65535 || c <= 0 || (c % 64) || c / 64 > 65535) return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!g || !ext || !pack || !gsel || !part_s) return APN_EINVAL;
    hipLaunchKernelGGL(ec_bwd_prep_kernel, dim3((n + 63) / 64, c / 64, b), dim3(256), 0, (hipStream_t)stream, n, c, g,
                       gs_b, gs_c, gs_n, ext, pack, slope, gsel, part_s);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ec_bwd_prep(int b, int n, int c, const float *g, long long gs_b, long long gs_c, long long gs_n,
                               const float *ext, const float *pack, float slope, float *gsel, float *part_s,
                               void *stream) {
    if (!(slope > 0.0f)) return APN_EINVAL;
    return ec_bwd_prep_launch(b, n, c, g, gs_b, gs_c, gs_n, ext, pack, slope, gsel, part_s, stream);
}

// apn_ec_bwd_prep with ReLU (slope == 0) allowed: act' is recomputed from ext and pack, so a residual added behind the
// activation needs nothing here (its gradient is g itself)
extern "C" int apn_ec_bwd_prep_act(int b, int n, int c, const float *g, long long gs_b, long long gs_c, long long gs_n,
                                   const float *ext, const float *pack, float slope, float *gsel, float *part_s,
                                   void *stream) {
    if (!(slope >= 0.0f)) return APN_EINVAL;
    return ec_bwd_prep_launch(b, n, c, g, gs_b, gs_c, gs_n, ext, pack, slope, gsel, part_s, stream);
}

// The reverse lists of `clouds` sets of n points, each gathered by the mq k positions of its own rows: five launches.
// scratch: clouds n + clouds mq k ints.  No position (mq == 0): every list is empty.
static int ec_csr_launch(int clouds, int n, int mq, int k, const int *idx, int *pcnt_poff, int *plist, int *scratch,
                         hipStream_t st) {
    const long long npts = (long long)clouds * n, npos = (long long)clouds * mq * k;
    int *pcnt = pcnt_poff, *poff = pcnt_poff + npts;
    int *cursor = scratch, *tmp = scratch + npts;
    const unsigned pb = (unsigned)((npos + 255) / 256);
    if (npos == 0) {
        hipLaunchKernelGGL(csr_init_kernel, dim3((unsigned)((2 * npts + 255) / 256)), dim3(256), 0, st, 2 * npts, pcnt,
                           (int *)nullptr);
        APN_LAUNCH_CHECK();
        return APN_OK;
    }
    hipLaunchKernelGGL(csr_init_kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, st, npts, pcnt, (int *)nullptr);
    hipLaunchKernelGGL(ec_csr_count_fill_kernel, dim3(pb), dim3(256), 0, st, npos, n, mq, k, 0, idx, pcnt, cursor, tmp);
    hipLaunchKernelGGL(csr_scan_kernel, dim3(clouds), dim3(1024), 0, st, n, (const int *)nullptr, mq * k, pcnt, poff, cursor);
    hipLaunchKernelGGL(ec_csr_count_fill_kernel, dim3(pb), dim3(256), 0, st, npos, n, mq, k, 1, idx, pcnt, cursor, tmp);
    hipLaunchKernelGGL(ec_csr_sort_kernel, dim3((unsigned)((npts + 3) / 4)), dim3(256), 0, st, npts, pcnt, poff, tmp,
                       plist);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ec_csr(int b, int n, int k, const int *idx, int *pcnt_poff, int *plist, int *scratch, void *stream) {
    if (!ec_sizes(b, n, k)) return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!idx || !pcnt_poff || !plist || !scratch) return APN_EINVAL;
    return ec_csr_launch(b, n, n, k, idx, pcnt_poff, plist, scratch, (hipStream_t)stream);       // b n k < 2^30
}

// The reverse lists of an (m, k) index into n rows (the stacked-cloud operators of csrc/pointops.hip): one "cloud" of
// n rows gathered by m k positions; scratch: n + m k ints.  m == 0: every list is empty.
extern "C" int apn_po_csr(int n, int m, int k, const int *idx, int *pcnt_poff, int *plist, int *scratch, void *stream) {
    if (n < 0 || m < 0 || n >= (1 << 24) || m >= (1 << 24) || k < 1 || (long long)m * k >= (1ll << 31)) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!idx || !pcnt_poff || !plist || !scratch) return APN_EINVAL;
    return ec_csr_launch(1, n, m, k, idx, pcnt_poff, plist, scratch, (hipStream_t)stream);
}

extern "C" int apn_ec_pool_bwd(int b, int n, int c, int k, const float *gsel, const void *sel, const int *pcnt_poff,
                               const int *plist, const float *uv, int ld, const float *ysum, const float *de,
                               float *duv, void *stream) {
    if (!ec_sizes(b, n, k) || !ec_width(c) || ld < 2 * c || (ld % 4)) return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!gsel || !sel || !pcnt_poff || !plist || !uv || !de || !duv) return APN_EINVAL;
    const long long npts = (long long)b * n;
    const dim3 grid((unsigned)((npts + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define APN_EC_BWD(VEC)                                                                                          \
    hipLaunchKernelGGL(ec_pool_bwd_kernel<VEC>, grid, block, 0, st, npts, k, gsel, (const unsigned char *)sel,   \
                       pcnt_poff, pcnt_poff + npts, plist, uv, ld, ysum, de, duv)
    switch (c / 64) {
        case 1: APN_EC_BWD(1); break;
        case 2: APN_EC_BWD(2); break;
        case 4: APN_EC_BWD(4); break;
        default: APN_EC_BWD(8); break;
    }
#undef APN_EC_BWD
    APN_LAUNCH_CHECK();
    return APN_OK;
}
