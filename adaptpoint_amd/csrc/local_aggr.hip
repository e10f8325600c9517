// local_aggr.hip -- the position-level work of a PointNeXt LocalAggregation with ONE grouped convolution
// (openpoints/models/backbone/pointnext.py:27-78 as InvResMLP builds it, :246): p grouped around p itself,
//
//     out[b,c,q] = relu(bn(max_k conv([ (p[idx[q,k]] - p[q]) / r ; f[idx[q,k]] ])))
//
// The feature part of the convolution is hoisted to the points (adaptpoint_amd/fused_wide.py): U[n] = Wf f[n], so that
// y[q,k] = U[idx[q,k]] + Wp (p[idx[q,k]] - p[q]) / r -- the three coordinate columns are applied to the relative
// position itself, formed as the composed path forms it (no difference of two large hoisted terms when r is small).
// BatchNorm + ReLU is monotone per channel with the sign of gamma, so the max over K commutes with them:
//
//     out[b,c,q] = relu(scale_c ext_k y[q,k][c] + shift_c),   ext = max (gamma_c >= 0) | min
//
// and the whole pass over the B*N*K positions is a gather-extremum over each query's DISTINCT neighbours (a ball
// query pads slots cnt..31 with copies of slot 0: ball_query_gpu.cu:41-48).  No MFMA, no grouped tensor.
//
//   la_pool_fwd   one wave per query, a lane per VEC consecutive channels (a row of U is one coalesced read of the
//                 wave): the extremum and the slot that holds it, and -- training -- ysum[q] = sum_k y[q,k] (the
//                 backward pass and BatchNorm's mean need it) and the query's share of sum y^2, multiplicity-weighted,
//                 float32 over the query's 32 positions, float64 across queries.  One float64 partial row per
//                 workgroup; apn_la_stats_fold adds them with the {count, 1} tail apn_sa_bn_fold takes (the fold is
//                 csrc/col_sums.hip's, at 4 lanes).
//   la_pool_bwd   one wave per point n: dL/dU[n] = the gradients of the (query, channel) pairs that selected n --
//                 its rows walked through the index stage's inverse map (pcnt / poff / plist, ascending: a fixed
//                 order, no float atomics) -- plus BatchNorm's dense term D y + E summed over the positions that
//                 gather n (a function of the occurrence count and the gathering queries' coordinate sum, `geo`);
//                 dT[n] = dL/dU[n] - sum_k dL/dy[n,k]: what multiplies Wp p[n] / r, so that dL/dWp = dT^T p / r and
//                 (optionally, formed here) dL/dp[n] = dT[n] Wp / r.
//
// The layout change of the output, BatchNorm's fold and its backward constants are the width-generic block's own
// entries (apn_sa_wide_out, apn_sa_bn_fold, apn_sa_wide_bwd_prep, apn_sa_wide_consts2); the dense products run on
// csrc/pointwise.hip's contraction kernel.
#include "apn_common.h"
#include "tile_map.h"

namespace apn {

constexpr int LA_K = 32;          // neighbours per query (the tile map's row width)
constexpr int LA_QPB = 64;        // queries per workgroup of the forward pass (16 per wave)

// VEC consecutive floats at p (16-byte pieces for VEC >= 4)
template <int VEC>
__device__ __forceinline__ void la_load(const float *__restrict__ p, float (&v)[VEC]) {
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
__device__ __forceinline__ void la_store(float *__restrict__ p, const float (&v)[VEC]) {
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

// H = 64 VEC channels.  Grid: ceil(B N / 64) workgroups of 4 waves.  wp: the convolution's coordinate columns (H
// rows of stride ldw); radius: what relative positions are divided by (1 when the grouper does not normalise).
template <int VEC>
__global__ __launch_bounds__(256) void la_pool_fwd_kernel(long long nq, int n, float radius, const float *__restrict__ U,
                                                          const float *__restrict__ xyz, const float *__restrict__ wp,
                                                          int ldw, const int *__restrict__ idx,
                                                          const float *__restrict__ gamma, float *__restrict__ ext,
                                                          unsigned char *__restrict__ sel, float *__restrict__ ysum,
                                                          double *__restrict__ part) {
    constexpr int H = 64 * VEC;
    __shared__ double red[4][2 * H];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * VEC;
    float sg[VEC], w0[VEC], w1[VEC], w2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        sg[j] = (!gamma || gamma[c0 + j] >= 0.0f) ? 1.0f : -1.0f;
        w0[j] = wp[(size_t)(c0 + j) * ldw];
        w1[j] = wp[(size_t)(c0 + j) * ldw + 1];
        w2[j] = wp[(size_t)(c0 + j) * ldw + 2];
    }
    double acc1[VEC], acc2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { acc1[j] = 0.0; acc2[j] = 0.0; }
    const long long q0 = (long long)blockIdx.x * LA_QPB + wave * (LA_QPB / 4);
    for (int qi = 0; qi < LA_QPB / 4; ++qi) {
        const long long gq = q0 + qi;
        if (gq >= nq) break;                                   // (wave-uniform)
        const long long base = (gq / n) * n;                   // the cloud's first point
        int nb = idx[gq * LA_K + (lane & 31)];
        nb = nb < 0 ? 0 : (nb >= n ? n - 1 : nb);              // (an index outside the cloud is never followed)
        const int first = __builtin_amdgcn_readlane(nb, 0);
        const unsigned differ = (unsigned)__ballot(lane < 32 && nb != first);
        const int c = __popc(differ) + 1;
        // the ball query's structure (the differing slots are exactly 1..c-1); any other row is kept whole
        const bool folded = differ == ((c >= 32 ? 0xffffffffu : ((1u << c) - 1u)) & ~1u);
        const int rows = folded ? c : LA_K;
        const float mult0 = folded ? (float)(LA_K + 1 - c) : 1.0f;
        const float qx = xyz[gq * 3], qy = xyz[gq * 3 + 1], qz = xyz[gq * 3 + 2];
        float best[VEC], s1[VEC], s2[VEC];
        unsigned char bs[VEC];
        // G rows in flight per step (independent loads; the slots past the last row re-read it and are dropped)
        constexpr int G = VEC >= 8 ? 2 : 4;
        for (int k = 0; k < rows; k += G) {
            float u[G][VEC], dx[G], dy[G], dz[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const long long pt = base + __builtin_amdgcn_readlane(nb, k + g < rows ? k + g : rows - 1);
                la_load<VEC>(U + pt * H + c0, u[g]);
                dx[g] = xyz[pt * 3]; dy[g] = xyz[pt * 3 + 1]; dz[g] = xyz[pt * 3 + 2];
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (k + g >= rows) break;                      // (wave-uniform)
                const float rx = (dx[g] - qx) / radius, ry = (dy[g] - qy) / radius, rz = (dz[g] - qz) / radius;
                const float m = k + g == 0 ? mult0 : 1.0f;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float y = u[g][j] + __builtin_fmaf(rz, w2[j], __builtin_fmaf(ry, w1[j], rx * w0[j]));
                    const float t = y * sg[j], my = m * y;
                    if (k + g == 0) {
                        best[j] = t; bs[j] = 0; s1[j] = my; s2[j] = my * y;
                    } else {
                        if (t > best[j]) { best[j] = t; bs[j] = (unsigned char)(k + g); }
                        s1[j] += my;
                        s2[j] = __builtin_fmaf(my, y, s2[j]);
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
        la_store<VEC>(ext + gq * H + c0, e);
        if (ysum) la_store<VEC>(ysum + gq * H + c0, s1);
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

__device__ __forceinline__ float la_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per point.  gsel (B,N,H) = the upstream gradient times BatchNorm's scale (through the ReLU), sel the
// winning slots; tmap = the tile map (tq0 at +4, rowinfo behind it: csrc/sa_wide_glue.hip); de = {D[H], E[H]}:
// BatchNorm's dense term dL/dy = D y + E; wp = the convolution's three coordinate columns (row stride ldw).
// Sum of y over the positions that gather n: occ U[n] + Wp (occ p[n] - SP[n]) / r, geo[n] = {occ, SP}.
template <int VEC>
__global__ __launch_bounds__(256) void la_pool_bwd_kernel(long long npts, int n, float inv_r,
                                                          const float *__restrict__ gsel,
                                                          const unsigned char *__restrict__ sel,
                                                          const int *__restrict__ tq0,
                                                          const unsigned *__restrict__ rowinfo,
                                                          const int *__restrict__ pcnt, const int *__restrict__ poff,
                                                          const int *__restrict__ plist, const float *__restrict__ geo,
                                                          const float *__restrict__ U, const float *__restrict__ xyz,
                                                          const float *__restrict__ ysum, const float *__restrict__ de,
                                                          const float *__restrict__ wp, int ldw, float *__restrict__ dU,
                                                          float *__restrict__ dT, float *__restrict__ dp) {
    constexpr int H = 64 * VEC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * VEC;
    const long long pt = (long long)blockIdx.x * 4 + wave;
    if (pt >= npts) return;
    const int cnt = pcnt[pt];
    const int *__restrict__ list = plist + poff[pt];
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.0f;
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int chunk = cnt - i0 < 64 ? cnt - i0 : 64;
        long long q = 0;
        int slot = 0;
        if (lane < chunk) {
            const int row = list[i0 + lane];
            const unsigned info = rowinfo[row];
            q = (long long)tq0[row >> 5] + (int)(info & 0xffu);
            slot = (int)((info >> 8) & 0xffu);
        }
        q = q < 0 ? 0 : (q >= npts ? npts - 1 : q);              // (a damaged map is never followed out of the arrays)
        const int qlo = (int)q;
        constexpr int G = VEC >= 8 ? 2 : 4;
        for (int j = 0; j < chunk; j += G) {
            float g[G][VEC];
            unsigned char sb[G][VEC];
            int sj[G];
#pragma unroll
            for (int t = 0; t < G; ++t) {
                const int jj = j + t < chunk ? j + t : chunk - 1;
                const long long qj = (long long)__builtin_amdgcn_readlane(qlo, jj);
                sj[t] = __builtin_amdgcn_readlane(slot, jj);
                la_load<VEC>(gsel + qj * H + c0, g[t]);
#pragma unroll
                for (int e = 0; e < VEC; ++e) sb[t][e] = sel[qj * H + c0 + e];
            }
#pragma unroll
            for (int t = 0; t < G; ++t) {
                if (j + t >= chunk) break;                     // (wave-uniform)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += (int)sb[t][e] == sj[t] ? g[t][e] : 0.0f;
            }
        }
    }
    const float4 ge = *reinterpret_cast<const float4 *>(geo + pt * 4);
    const float px = xyz[pt * 3], py = xyz[pt * 3 + 1], pz = xyz[pt * 3 + 2];
    // occ p[n] - SP[n]: the gathered relative positions, summed
    const float rx = (ge.x * px - ge.y) * inv_r, ry = (ge.x * py - ge.z) * inv_r, rz = (ge.x * pz - ge.w) * inv_r;
    float u[VEC], gown[VEC], ys[VEC], du[VEC], dt[VEC];
    la_load<VEC>(U + pt * H + c0, u);
    la_load<VEC>(gsel + pt * H + c0, gown);
    if (ysum) {
        la_load<VEC>(ysum + pt * H + c0, ys);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) ys[e] = 0.0f;
    }
    float tp0 = 0.0f, tp1 = 0.0f, tp2 = 0.0f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int c = c0 + e;
        const float D = de[c], E = de[H + c];
        const float w0 = wp[(size_t)c * ldw], w1 = wp[(size_t)c * ldw + 1], w2 = wp[(size_t)c * ldw + 2];
        const float ygath = __builtin_fmaf(ge.x, u[e], __builtin_fmaf(rz, w2, __builtin_fmaf(ry, w1, rx * w0)));
        du[e] = acc[e] + __builtin_fmaf(D, ygath, ge.x * E);
        dt[e] = du[e] - (gown[e] + __builtin_fmaf(D, ys[e], (float)LA_K * E));
        tp0 = __builtin_fmaf(dt[e], w0, tp0);
        tp1 = __builtin_fmaf(dt[e], w1, tp1);
        tp2 = __builtin_fmaf(dt[e], w2, tp2);
    }
    la_store<VEC>(dU + pt * H + c0, du);
    la_store<VEC>(dT + pt * H + c0, dt);
    if (dp) {
        tp0 = la_wave_sum(tp0);
        tp1 = la_wave_sum(tp1);
        tp2 = la_wave_sum(tp2);
        if (lane < 3) dp[pt * 3 + lane] = (lane == 0 ? tp0 : (lane == 1 ? tp1 : tp2)) * inv_r;
    }
}

}  // namespace apn

using namespace apn;

static bool la_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

extern "C" int apn_la_pool_rows(int b, int n) {
    if (b <= 0 || n <= 0) return 0;
    return (int)(((long long)b * n + LA_QPB - 1) / LA_QPB);
}

extern "C" int apn_la_pool_fwd(int b, int n, int c, int nsample, float radius, const float *U, const float *xyz,
                               const float *wp, int ldw, const int *idx, const float *gamma, float *ext, void *sel,
                               float *ysum, double *part, void *stream) {
    if (b < 0 || n < 0 || !la_width(c) || nsample != LA_K || (long long)b * n > 0x7fffffffLL / 64 || ldw < 3 ||
        !(radius > 0.0f))
        return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!U || !xyz || !wp || !idx || !ext || !sel || ((ysum != nullptr) != (part != nullptr))) return APN_EINVAL;
    const long long nq = (long long)b * n;
    const dim3 grid((unsigned)((nq + LA_QPB - 1) / LA_QPB)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define APN_LA_FWD(VEC)                                                                                           \
    hipLaunchKernelGGL(la_pool_fwd_kernel<VEC>, grid, block, 0, st, nq, n, radius, U, xyz, wp, ldw, idx, gamma, ext, \
                       (unsigned char *)sel, ysum, part)
    switch (c / 64) {
        case 1: APN_LA_FWD(1); break;
        case 2: APN_LA_FWD(2); break;
        case 4: APN_LA_FWD(4); break;
        default: APN_LA_FWD(8); break;
    }
#undef APN_LA_FWD
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_la_stats_fold(const double *part, int rows, int c, double count, double *sums, void *stream) {
    if (rows < 0 || c <= 0 || !(count >= 0.0)) return APN_EINVAL;
    if (rows == 0) return APN_OK;
    if (!part || !sums) return APN_EINVAL;
    return col_sums(part, rows, (size_t)2 * c, 4, sums, count, (hipStream_t)stream);
}

extern "C" int apn_la_pool_bwd(int b, int n, int c, int nsample, float radius, const float *gsel, const void *sel,
                               const int *tmap, const int *pcnt_poff, const int *plist, const float *geo,
                               const float *U, const float *xyz, const float *ysum, const float *de, const float *wp,
                               int ldw, float *dU, float *dT, float *dp, void *stream) {
    if (b < 0 || n < 0 || !la_width(c) || nsample != LA_K || (long long)b * n > 0x7fffffffLL / 64 || ldw < 3 ||
        !(radius > 0.0f))
        return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!gsel || !sel || !tmap || !pcnt_poff || !plist || !geo || !U || !xyz || !de || !wp || !dU || !dT)
        return APN_EINVAL;
    const long long npts = (long long)b * n;
    const TileMapView tm(tmap, (int)npts, b);           // (every point is a query: the map of b n queries)
    const dim3 grid((unsigned)((npts + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define APN_LA_BWD(VEC)                                                                                               \
    hipLaunchKernelGGL(la_pool_bwd_kernel<VEC>, grid, block, 0, st, npts, n, 1.0f / radius, gsel,                     \
                       (const unsigned char *)sel, tm.tq0, tm.rowinfo, pcnt_poff, pcnt_poff + npts, plist, geo, U, xyz,   \
                       ysum, de, wp, ldw, dU, dT, dp)
    switch (c / 64) {
        case 1: APN_LA_BWD(1); break;
        case 2: APN_LA_BWD(2); break;
        case 4: APN_LA_BWD(4); break;
        default: APN_LA_BWD(8); break;
    }
#undef APN_LA_BWD
    APN_LAUNCH_CHECK();
    return APN_OK;
}
