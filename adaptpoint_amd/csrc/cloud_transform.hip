// cloud_transform.hip -- the ScanObjectNN dataset side of a training batch on the device: per cloud the slice and row
// shuffle of ScanObjectNNHardest.__getitem__ (openpoints/dataset/scanobjectnn/scanobjectnn.py:79-97), the cfg chain
// PointCloudScaling -> PointCloudCenterAndNormalize -> PointCloudRotation (openpoints/transforms/
// point_transformer_gpu.py), and the height channel, written as out (b, n, 4) = [pos, heights].
//
// One workgroup per cloud.  The cloud is read through the permutation straight from global memory into registers (at
// most CT_PTS points per thread); LDS holds only the sort keys of the device-drawn shuffle and the per-wave partials
// of the reductions.  Stages, each switched by a flag (APN_CT_* in include/adaptpoint_amd.h):
//   source    raw[rows[c], :n] (or raw[c, :n]); a row outside [0, s) makes the whole cloud NaN
//   permute   src[perm[i]]; with device draws perm is the order of the per-point uniforms, found by an LDS bitonic
//             sort of (uniform bits << 32 | i) keys -- distinct, so there are no ties
//   scale     p *= s (3 factors; mirror and scale_xyz already folded in)
//   heights   h = g - min(g) on the gravity axis, of the scaled points when CenterAndNormalize is in the chain and of
//             the unscaled ones otherwise (the dataset's fallback reads its own unscaled array)
//   centre    p -= mean(p), the mean summed in float64 in a fixed order and rounded once to float32
//   normalise p = p / max |p|, |p| = sqrt((x*x + y*y) + z*z), square root and division rounded to nearest
//   rotate    p @ R^T, each row summed in float64 from exact products and rounded once
// Every reduction has a fixed order, so the output is the same bit for bit from run to run.
#include <hip/hip_runtime.h>

#include "../../include/adaptpoint_amd.h"
#include "apn_common.h"
#include "lds_bitonic.h"

namespace apn {

constexpr int CT_THREADS = 1024;
constexpr int CT_WAVES = CT_THREADS / 64;
constexpr int CT_MAXN = 8192;
constexpr int CT_PTS = CT_MAXN / CT_THREADS;
constexpr int CT_CLOUD_U = 10;      // per-cloud uniforms: scale (3) | mirror (3) | angle (3) | axis order (1)
constexpr int CT_PARAMS = 12;       // per-cloud parameters: scale (3) | R row-major (9)

// R_axis(theta) = expm of the skew matrix of theta * e_axis (point_transformer_gpu.py:272-274), in closed form; selects
// rather than indexing, so that a run-time axis keeps the matrix in registers
__device__ __forceinline__ void ct_axis_rotation(int axis, double theta, double (&M)[9]) {
    const double c = cos(theta), s = sin(theta);
    const int i = (axis + 1) % 3, j = (axis + 2) % 3;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            M[3 * r + q] = r == q ? (r == axis ? 1.0 : c) : (r == i && q == j) ? -s : (r == j && q == i) ? s : 0.0;
}

__device__ __forceinline__ void ct_matmul3(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// the device-draw mapping of one cloud's uniforms u (CT_CLOUD_U) onto PointCloudScaling's and PointCloudRotation's
// distributions.  cfg (double): scale_lo, scale_hi, mirror (3), scale_xyz (3, 0 = off), angle bounds (3, NaN = None).
__device__ __forceinline__ void ct_device_params(const double *cfg, const float *u, int flags, float (&sc)[3],
                                                 float (&R)[9]) {
    if (flags & APN_CT_SCALE) {
        const float lo = (float)cfg[0], hi = (float)cfg[1], d = hi - lo;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sc[c] = ((flags & APN_CT_ANISOTROPIC) ? u[c] : u[0]) * d + lo;
            if (flags & APN_CT_MIRROR) sc[c] *= (double)u[3 + c] > cfg[2 + c] ? 1.0f : -1.0f;
            if (cfg[5 + c] == 0.0) sc[c] = 1.0f;
        }
    }
    if (flags & APN_CT_ROTATE) {
        // the k-th of the 6 orders of the three axis matrices, lexicographic: (0,1,2), (0,2,1), (1,0,2), ...
        const int k = min((int)(u[9] * 6.0f), 5);
        const int o0 = k >> 1;
        int o1 = o0 == 0 ? 1 : 0, o2 = o0 == 2 ? 1 : 2;
        if (k & 1) {
            const int tmp = o1;
            o1 = o2;
            o2 = tmp;
        }
        double th[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double bound = cfg[8 + c];
            th[c] = bound != bound ? 0.0 : -bound + (bound + bound) * (double)u[6 + c];
        }
        double M0[9], M1[9], M2[9];
        ct_axis_rotation(o0, o0 == 0 ? th[0] : o0 == 1 ? th[1] : th[2], M0);
        ct_axis_rotation(o1, o1 == 0 ? th[0] : o1 == 1 ? th[1] : th[2], M1);
        ct_axis_rotation(o2, o2 == 0 ? th[0] : o2 == 1 ? th[1] : th[2], M2);
        double A[9], Rd[9];
        ct_matmul3(M0, M1, A);
        ct_matmul3(A, M2, Rd);
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = (float)Rd[e];
    }
}

// sqrt(a), a >= 0, rounded to nearest: the hardware square root (within 1 ulp) moved to the neighbour its midpoint test
// picks.  The midpoint of two float32 neighbours has 25 significant bits, so its square is exact in float64 and never
// equals a float32 value.
__device__ __forceinline__ float ct_sqrt_rn(float a) {
    float s = sqrtf(a);
    if (!(s > 0.0f) || isinf(s)) return s;
    const double ad = a;
    const float up = __int_as_float(__float_as_int(s) + 1);
    const double mu = 0.5 * ((double)s + (double)up);
    if (mu * mu < ad) s = up;
    const float dn = __int_as_float(__float_as_int(s) - 1);
    const double md = 0.5 * ((double)s + (double)dn);
    if (md * md > ad) s = dn;
    return s;
}

__device__ __forceinline__ float ct_coord(int axis, float x, float y, float z) { return axis == 0 ? x : axis == 1 ? y : z; }

__global__ __launch_bounds__(CT_THREADS) void cloud_transform_kernel(
    int n, int n_raw, int s, const float *__restrict__ raw, const int *__restrict__ rows, int flags, int gdim,
    const double *__restrict__ cfg, const int *__restrict__ perm, const float *__restrict__ params,
    const float *__restrict__ u_cloud, const float *__restrict__ u_point, int *__restrict__ perm_out,
    float *__restrict__ params_out, float *__restrict__ out) {
    __shared__ unsigned long long keys[CT_MAXN];
    __shared__ double part_sum[3][CT_WAVES];
    __shared__ float part_min[CT_WAVES], part_max[CT_WAVES];
    const int cl = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float *dst = out + (size_t)cl * n * 4;
    const int row = rows ? rows[cl] : cl;
    if (row < 0 || row >= s) {                         // uniform across the workgroup
        const float q = __int_as_float(0x7fc00000);
        for (int i = t; i < n; i += CT_THREADS) {
            *reinterpret_cast<float4 *>(dst + (size_t)i * 4) = make_float4(q, q, q, q);
            if (perm_out) perm_out[(size_t)cl * n + i] = -1;
        }
        if (params_out && t < CT_PARAMS) params_out[(size_t)cl * CT_PARAMS + t] = q;
        return;
    }
    const bool uniform = flags & APN_CT_UNIFORM, permute = flags & APN_CT_PERMUTE;

    float sc[3] = {1.0f, 1.0f, 1.0f}, R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (uniform) {
        ct_device_params(cfg, u_cloud + (size_t)cl * CT_CLOUD_U, flags, sc, R);
    } else {
        const float *pp = params + (size_t)cl * CT_PARAMS;
        if (flags & APN_CT_SCALE)
#pragma unroll
            for (int c = 0; c < 3; ++c) sc[c] = pp[c];
        if (flags & APN_CT_ROTATE)
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = pp[3 + e];
    }
    if (params_out && t == 0) {
        float *po = params_out + (size_t)cl * CT_PARAMS;
#pragma unroll
        for (int c = 0; c < 3; ++c) po[c] = sc[c];
#pragma unroll
        for (int e = 0; e < 9; ++e) po[3 + e] = R[e];
    }

    if (uniform && permute) {
        const float *pu = u_point + (size_t)cl * n;
        int P = 1;
        while (P < n) P <<= 1;
        for (int i = t; i < P; i += CT_THREADS)
            keys[i] = i < n ? ((unsigned long long)__float_as_uint(pu[i]) << 32) | (unsigned)i : ~0ull;
        __syncthreads();
        lds_bitonic_sort<CT_THREADS>(keys, P);
    }

    // ---- gather through the permutation, scale; the gravity coordinate for the heights
    const float *src = raw + (size_t)row * n_raw * 3;
    const bool hscaled = flags & APN_CT_HEIGHTS_SCALED;
    float px[CT_PTS], py[CT_PTS], pz[CT_PTS], pg[CT_PTS];
    float tmin = INFINITY;
    double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < CT_PTS; ++k) {
        const int i = k * CT_THREADS + t;
        px[k] = py[k] = pz[k] = pg[k] = 0.0f;
        if (i < n) {
            int pi = i;
            if (permute) pi = uniform ? (int)(unsigned)(keys[i] & 0xffffffffull) : perm[(size_t)cl * n + i];
            if (perm_out) perm_out[(size_t)cl * n + i] = pi;
            float x = __int_as_float(0x7fc00000), y = x, z = x;
            if ((unsigned)pi < (unsigned)n) {           // a host permutation is checked too: never read out of bounds
                x = src[(size_t)pi * 3 + 0];
                y = src[(size_t)pi * 3 + 1];
                z = src[(size_t)pi * 3 + 2];
            }
            float g = ct_coord(gdim, x, y, z);
            x *= sc[0];
            y *= sc[1];
            z *= sc[2];
            if (hscaled) g = ct_coord(gdim, x, y, z);
            px[k] = x;
            py[k] = y;
            pz[k] = z;
            pg[k] = g;
            tmin = fminf(tmin, g);
            sum[0] += (double)x;
            sum[1] += (double)y;
            sum[2] += (double)z;
        }
    }

    // ---- heights' minimum and the centre: wave butterflies, then the waves' partials in wave order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tmin = fminf(tmin, __shfl_xor(tmin, o));
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += __shfl_xor(sum[c], o);
    }
    if (lane == 0) {
        part_min[wave] = tmin;
#pragma unroll
        for (int c = 0; c < 3; ++c) part_sum[c][wave] = sum[c];
    }
    __syncthreads();
    float hmin = INFINITY;
    double tot[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < CT_WAVES; ++w) {
        hmin = fminf(hmin, part_min[w]);
#pragma unroll
        for (int c = 0; c < 3; ++c) tot[c] += part_sum[c][w];
    }
    if (flags & APN_CT_CENTER) {
        const float mx = (float)(tot[0] / (double)n), my = (float)(tot[1] / (double)n), mz = (float)(tot[2] / (double)n);
#pragma unroll
        for (int k = 0; k < CT_PTS; ++k) {
            px[k] -= mx;
            py[k] -= my;
            pz[k] -= mz;
        }
    }

    // ---- normalise by the largest norm
    if (flags & APN_CT_NORMALIZE) {
        float tmax = 0.0f;
#pragma unroll
        for (int k = 0; k < CT_PTS; ++k)
            if (k * CT_THREADS + t < n) tmax = fmaxf(tmax, ct_sqrt_rn((px[k] * px[k] + py[k] * py[k]) + pz[k] * pz[k]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, o));
        if (lane == 0) part_max[wave] = tmax;
        __syncthreads();
        float m = 0.0f;
#pragma unroll
        for (int w = 0; w < CT_WAVES; ++w) m = fmaxf(m, part_max[w]);
#pragma unroll
        for (int k = 0; k < CT_PTS; ++k) {
            px[k] = __fdiv_rn(px[k], m);
            py[k] = __fdiv_rn(py[k], m);
            pz[k] = __fdiv_rn(pz[k], m);
        }
    }

    // ---- rotate and write [pos, heights]
    const bool rotate = flags & APN_CT_ROTATE;
#pragma unroll
    for (int k = 0; k < CT_PTS; ++k) {
        const int i = k * CT_THREADS + t;
        if (i >= n) continue;
        float o[3] = {px[k], py[k], pz[k]};
        if (rotate) {
            const double x = px[k], y = py[k], z = pz[k];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                o[r] = (float)((x * (double)R[3 * r] + y * (double)R[3 * r + 1]) + z * (double)R[3 * r + 2]);
        }
        *reinterpret_cast<float4 *>(dst + (size_t)i * 4) = make_float4(o[0], o[1], o[2], pg[k] - hmin);
    }
}

}  // namespace apn

extern "C" int apn_cloud_transform(int b, int n, int n_raw, int s, const float *raw, const int *rows, int flags,
                                   int gravity_dim, const double *cfg, const int *perm, const float *params,
                                   const float *uniforms, int *perm_out, float *params_out, float *out, void *stream) {
    using namespace apn;
    if (b < 0 || n <= 0 || n > CT_MAXN || n_raw < n || s <= 0 || gravity_dim < 0 || gravity_dim > 2) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!raw || !out || (!rows && s < b)) return APN_EINVAL;
    const float *u_cloud = nullptr, *u_point = nullptr;
    if (flags & APN_CT_UNIFORM) {
        if (!uniforms || !cfg) return APN_EINVAL;
        u_cloud = uniforms;
        u_point = uniforms + (size_t)b * CT_CLOUD_U;
    } else {
        if ((flags & APN_CT_PERMUTE) && !perm) return APN_EINVAL;
        if ((flags & (APN_CT_SCALE | APN_CT_ROTATE)) && !params) return APN_EINVAL;
    }
    hipLaunchKernelGGL(cloud_transform_kernel, dim3(b), dim3(CT_THREADS), 0, (hipStream_t)stream, n, n_raw, s, raw, rows,
                       flags, gravity_dim, cfg, perm, params, u_cloud, u_point, perm_out, params_out, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
