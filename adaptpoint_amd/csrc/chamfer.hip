// chamfer.hip -- Chamfer distance: exact nearest point in both directions and its ordered, atomic-free gradient
// (apn_chamfer_forward / apn_chamfer_backward; the contract is in include/adaptpoint_amd.h).
//
// Forward: for every point of one cloud the nearest point of the other, d = fma(tz, tz, fma(ty, ty, tx * tx)) with
// t = target - source in fp32 (apn_knn_query's form at c = 3; the unit is compiled with -ffp-contract=off), the running
// (best, index) kept under strict `<` while the targets go by in ascending index: the smallest index that attains the
// minimum wins, with no tie code.  Both directions run in ONE launch: a workgroup (general path) or a wave (small path)
// is handed a (cloud, direction) and sees only "sources" and "targets".
//
//   small path, max(n, m) <= 64 (the masked autoencoder's per-patch loss: thousands of 32-point clouds): one wave per
//     (cloud, direction), four waves per workgroup.  Lane i owns source i; lane j also holds target j in registers and
//     v_readlane broadcasts it: no LDS, no barrier.
//   general path: a workgroup owns 64 sources of one cloud (lane = source in every wave) and stages the targets through
//     LDS in structure-of-arrays chunks of 1024; each of its four waves takes a quarter of every chunk, reading four
//     targets of a coordinate with one 16-byte read at a wave-uniform address (a broadcast: no bank conflict) -- the four
//     distances are independent of each other --, and the four (best, index) pairs of a source are merged by (distance,
//     index) at the end.  The quarter per wave is what fills the chip: 65536 sources are 1024 waves of sources, one per
//     SIMD, and the loop waits on LDS latency at that occupancy (measured with 256 sources per workgroup, one per lane:
//     40 us against 25 at (32,1024,1024), 283 against 229 at (8,8192,8192), the launch under hipGraph replay).
//
// Backward: the lane that owns point i starts from its own term and then walks the OTHER direction's index array of
// its cloud in ascending j (LDS chunks, broadcast reads; registers on the small path), subtracting j's term when
// idx[j] == i.  Ascending order is the loop order, so the sum is one fixed sequence of separately rounded fp32
// operations: no float atomic, no list, no scratch, and the case of every source choosing one target costs what any
// other case costs (n m integer compares per cloud and direction).  Every output element is written by its owner.
//
// Grids are one-dimensional and flattened over (cloud, direction, tile): there is no 65535 limit on b.
#include "apn_common.h"

namespace apn {

constexpr int CH_MAX_POINTS = 65536;                    // apn_chamfer_max_points()
constexpr int CH_SMALL = APN_WAVE;                      // max(n, m) up to here: the one-wave path
constexpr int CH_THREADS = 256;
constexpr int CH_WAVES = CH_THREADS / APN_WAVE;
constexpr int CH_SRC = APN_WAVE;                        // sources per workgroup of the general forward (one per lane)
constexpr int CH_CHUNK = 1024;                          // targets staged per chunk (12 KiB forward, 20 KiB backward)

// one target against the lane's source: strict `<`, targets in ascending j
__device__ __forceinline__ void ch_step(float sx, float sy, float sz, float tx, float ty, float tz, int j, float &best,
                                        int &bi) {
    const float d = dist2(ty - sy, tx - sx, tz - sz);   // fma(tz, tz, fma(ty, ty, tx * tx)) (apn_common.h argument order)
    const bool lt = d < best;
    best = lt ? d : best;
    bi = lt ? j : bi;
}

// what a (cloud, direction) sees of the forward's arguments
struct ChSide {
    int ns, nt;                 // sources, targets
    const float *src, *tgt;
    size_t out;                 // offset of the cloud's first source in dist / idx
    bool rev;                   // direction 2 -> 1
};

__device__ __forceinline__ ChSide ch_side(int cloud, bool rev, int n, int m, const float *xyz1, const float *xyz2) {
    ChSide s;
    s.rev = rev;
    s.ns = rev ? m : n;
    s.nt = rev ? n : m;
    s.src = (rev ? xyz2 : xyz1) + (size_t)cloud * s.ns * 3;
    s.tgt = (rev ? xyz1 : xyz2) + (size_t)cloud * s.nt * 3;
    s.out = (size_t)cloud * s.ns;
    return s;
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_fwd_small_kernel(int b, int n, int m, const float *__restrict__ xyz1,
                                                                       const float *__restrict__ xyz2,
                                                                       float *__restrict__ dist1, float *__restrict__ dist2,
                                                                       int *__restrict__ idx1, int *__restrict__ idx2) {
    const int lane = threadIdx.x & (APN_WAVE - 1);
    const int gw = blockIdx.x * CH_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / APN_WAVE);   // (cloud, direction)
    if (gw >= 2 * b) return;
    const ChSide s = ch_side(gw >> 1, gw & 1, n, m, xyz1, xyz2);
    const int ls = lane < s.ns ? lane : s.ns - 1, lt = lane < s.nt ? lane : s.nt - 1;
    const float sx = s.src[ls * 3], sy = s.src[ls * 3 + 1], sz = s.src[ls * 3 + 2];
    const float tx = s.tgt[lt * 3], ty = s.tgt[lt * 3 + 1], tz = s.tgt[lt * 3 + 2];
    float best = __builtin_inff();
    int bi = 0;
    for (int j = 0; j < s.nt; ++j)
        ch_step(sx, sy, sz, readlane_f(tx, j), readlane_f(ty, j), readlane_f(tz, j), j, best, bi);
    if (lane < s.ns) {
        (s.rev ? dist2 : dist1)[s.out + lane] = best;
        (s.rev ? idx2 : idx1)[s.out + lane] = bi;
    }
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_fwd_kernel(int n, int m, int tiles1, int tiles2,
                                                                 const float *__restrict__ xyz1,
                                                                 const float *__restrict__ xyz2, float *__restrict__ dist1,
                                                                 float *__restrict__ dist2, int *__restrict__ idx1,
                                                                 int *__restrict__ idx2) {
    __shared__ __align__(16) float ts[3][CH_CHUNK];
    __shared__ float wbest[CH_WAVES][APN_WAVE];
    __shared__ int wbi[CH_WAVES][APN_WAVE];
    const int tid = threadIdx.x;
    const int lane = tid & (APN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / APN_WAVE);
    const int per = tiles1 + tiles2;
    const int cloud = blockIdx.x / per;
    int tile = blockIdx.x - cloud * per;
    const bool rev = tile >= tiles1;
    if (rev) tile -= tiles1;
    const ChSide s = ch_side(cloud, rev, n, m, xyz1, xyz2);
    const int i = tile * CH_SRC + lane;
    const int ic = i < s.ns ? i : s.ns - 1;              // rows past the cloud repeat the last source (never written)
    const float sx = s.src[ic * 3], sy = s.src[ic * 3 + 1], sz = s.src[ic * 3 + 2];
    float best = __builtin_inff();
    int bi = 0;
    for (int j0 = 0; j0 < s.nt; j0 += CH_CHUNK) {
        const int cnt = s.nt - j0 < CH_CHUNK ? s.nt - j0 : CH_CHUNK;
        const int padded = (cnt + 3) & ~3;               // the pad is +inf: its distance is +inf and never `<` best
        __syncthreads();                                 // the previous chunk has been read
        const float *g = s.tgt + (size_t)j0 * 3;
        for (int e = tid; e < padded * 3; e += CH_THREADS) {
            const int j = e / 3, c = e - j * 3;
            ts[c][j] = j < cnt ? g[e] : __builtin_inff();
        }
        __syncthreads();
        const int share = ((padded / 4 + CH_WAVES - 1) / CH_WAVES) * 4;      // this wave's run of the chunk, whole float4s
        const int lo = wave * share, hi = lo + share < padded ? lo + share : padded;
#pragma unroll 2
        for (int j = lo; j < hi; j += 4) {
            const float4 tx = *reinterpret_cast<const float4 *>(&ts[0][j]);
            const float4 ty = *reinterpret_cast<const float4 *>(&ts[1][j]);
            const float4 tz = *reinterpret_cast<const float4 *>(&ts[2][j]);
            ch_step(sx, sy, sz, tx.x, ty.x, tz.x, j0 + j, best, bi);
            ch_step(sx, sy, sz, tx.y, ty.y, tz.y, j0 + j + 1, best, bi);
            ch_step(sx, sy, sz, tx.z, ty.z, tz.z, j0 + j + 2, best, bi);
            ch_step(sx, sy, sz, tx.w, ty.w, tz.w, j0 + j + 3, best, bi);
        }
    }
    // a wave holds the smallest index that attains ITS minimum; the waves' runs interleave over the chunks, so the merge
    // orders the four candidates by (distance, index)
    wbest[wave][lane] = best;
    wbi[wave][lane] = bi;
    __syncthreads();
    if (wave == 0 && i < s.ns) {
#pragma unroll
        for (int w = 1; w < CH_WAVES; ++w) {
            const float d = wbest[w][lane];
            const int k = wbi[w][lane];
            const bool take = d < best || (d == best && k < bi);
            best = take ? d : best;
            bi = take ? k : bi;
        }
        (rev ? dist2 : dist1)[s.out + i] = best;
        (rev ? idx2 : idx1)[s.out + i] = bi;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// what a (cloud, direction) sees of the backward's arguments: the "own" cloud receives the gradient
struct ChGradSide {
    int no, nt;                 // own points, the other cloud's points
    const float *own, *oth;     // coordinates
    const int *oidx, *tidx;     // own nearest (into the other cloud), the other cloud's nearest (into the own one)
    const float *og, *tg;       // grad_dist of the own / the other direction
    float *out;                 // the own cloud's gradient rows
};

__device__ __forceinline__ ChGradSide ch_grad_side(int cloud, bool rev, int n, int m, const float *xyz1, const float *xyz2,
                                                   const int *idx1, const int *idx2, const float *g1, const float *g2,
                                                   float *gx1, float *gx2) {
    ChGradSide s;
    s.no = rev ? m : n;
    s.nt = rev ? n : m;
    const size_t oo = (size_t)cloud * s.no, ot = (size_t)cloud * s.nt;
    s.own = (rev ? xyz2 : xyz1) + oo * 3;
    s.oth = (rev ? xyz1 : xyz2) + ot * 3;
    s.oidx = (rev ? idx2 : idx1) + oo;
    s.tidx = (rev ? idx1 : idx2) + ot;
    s.og = (rev ? g2 : g1) + oo;
    s.tg = (rev ? g1 : g2) + ot;
    s.out = (rev ? gx2 : gx1) + oo * 3;
    return s;
}

__device__ __forceinline__ int ch_clamp(int v, int count) { return v < 0 ? 0 : (v < count ? v : count - 1); }

// acc = acc - (g * 2) * (t - o): three separately rounded operations per component
__device__ __forceinline__ void ch_sub_term(float &ax, float &ay, float &az, float g, float tx, float ty, float tz, float ox,
                                            float oy, float oz) {
    const float g2 = g * 2.0f;
    ax = ax - g2 * (tx - ox);
    ay = ay - g2 * (ty - oy);
    az = az - g2 * (tz - oz);
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_bwd_small_kernel(int b, int n, int m, const float *__restrict__ xyz1,
                                                                       const float *__restrict__ xyz2,
                                                                       const int *__restrict__ idx1,
                                                                       const int *__restrict__ idx2,
                                                                       const float *__restrict__ g1,
                                                                       const float *__restrict__ g2, float *__restrict__ gx1,
                                                                       float *__restrict__ gx2) {
    const int lane = threadIdx.x & (APN_WAVE - 1);
    const int gw = blockIdx.x * CH_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / APN_WAVE);   // (cloud, direction)
    if (gw >= 2 * b) return;
    const ChGradSide s = ch_grad_side(gw >> 1, gw & 1, n, m, xyz1, xyz2, idx1, idx2, g1, g2, gx1, gx2);
    const int lo = lane < s.no ? lane : s.no - 1, lt = lane < s.nt ? lane : s.nt - 1;
    const float ox = s.own[lo * 3], oy = s.own[lo * 3 + 1], oz = s.own[lo * 3 + 2];
    const float tx = s.oth[lt * 3], ty = s.oth[lt * 3 + 1], tz = s.oth[lt * 3 + 2];
    const float tg = s.tg[lt];
    const int ti = ch_clamp(s.tidx[lt], s.no);
    const int k = ch_clamp(s.oidx[lo], s.nt);
    const float go = s.og[lo] * 2.0f;
    float ax = go * (ox - __shfl(tx, k, APN_WAVE));
    float ay = go * (oy - __shfl(ty, k, APN_WAVE));
    float az = go * (oz - __shfl(tz, k, APN_WAVE));
    for (int j = 0; j < s.nt; ++j) {
        if (__builtin_amdgcn_readlane(ti, j) == lane)
            ch_sub_term(ax, ay, az, readlane_f(tg, j), readlane_f(tx, j), readlane_f(ty, j), readlane_f(tz, j), ox, oy, oz);
    }
    if (lane < s.no) {
        s.out[lane * 3] = ax;
        s.out[lane * 3 + 1] = ay;
        s.out[lane * 3 + 2] = az;
    }
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_bwd_kernel(int n, int m, int tiles1, int tiles2,
                                                                 const float *__restrict__ xyz1,
                                                                 const float *__restrict__ xyz2,
                                                                 const int *__restrict__ idx1, const int *__restrict__ idx2,
                                                                 const float *__restrict__ g1, const float *__restrict__ g2,
                                                                 float *__restrict__ gx1, float *__restrict__ gx2) {
    __shared__ __align__(16) int ti[CH_CHUNK];
    __shared__ float ts[3][CH_CHUNK];
    __shared__ float tg[CH_CHUNK];
    const int tid = threadIdx.x;
    const int per = tiles1 + tiles2;
    const int cloud = blockIdx.x / per;
    int tile = blockIdx.x - cloud * per;
    const bool rev = tile >= tiles1;
    if (rev) tile -= tiles1;
    const ChGradSide s = ch_grad_side(cloud, rev, n, m, xyz1, xyz2, idx1, idx2, g1, g2, gx1, gx2);
    const int i = tile * CH_THREADS + tid;               // rows past the cloud match no index and are never written
    const int ic = i < s.no ? i : s.no - 1;
    const float ox = s.own[ic * 3], oy = s.own[ic * 3 + 1], oz = s.own[ic * 3 + 2];
    const int k = ch_clamp(s.oidx[ic], s.nt);
    const float go = s.og[ic] * 2.0f;
    float ax = go * (ox - s.oth[k * 3]);
    float ay = go * (oy - s.oth[k * 3 + 1]);
    float az = go * (oz - s.oth[k * 3 + 2]);
    for (int j0 = 0; j0 < s.nt; j0 += CH_CHUNK) {
        const int cnt = s.nt - j0 < CH_CHUNK ? s.nt - j0 : CH_CHUNK;
        const int padded = (cnt + 15) & ~15;
        __syncthreads();                                 // the previous chunk has been read
        const float *g = s.oth + (size_t)j0 * 3;
        for (int e = tid; e < cnt * 3; e += CH_THREADS) {
            const int j = e / 3, c = e - j * 3;
            ts[c][j] = g[e];
        }
        for (int j = tid; j < padded; j += CH_THREADS) {
            ti[j] = j < cnt ? ch_clamp(s.tidx[j0 + j], s.no) : -1;      // the pad matches nobody
            if (j < cnt) tg[j] = s.tg[j0 + j];
        }
        __syncthreads();
        for (int j = 0; j < padded; j += 16) {
            int4 t[4];                                   // sixteen indices, wave-uniform addresses: four broadcasts
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = *reinterpret_cast<const int4 *>(&ti[j + 4 * q]);
            bool any = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) any |= (t[q].x == i) | (t[q].y == i) | (t[q].z == i) | (t[q].w == i);
            if (any) {                                   // in ascending j: the order of the sum
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = j + 4 * q;
                    if (t[q].x == i) ch_sub_term(ax, ay, az, tg[r], ts[0][r], ts[1][r], ts[2][r], ox, oy, oz);
                    if (t[q].y == i) ch_sub_term(ax, ay, az, tg[r + 1], ts[0][r + 1], ts[1][r + 1], ts[2][r + 1], ox, oy, oz);
                    if (t[q].z == i) ch_sub_term(ax, ay, az, tg[r + 2], ts[0][r + 2], ts[1][r + 2], ts[2][r + 2], ox, oy, oz);
                    if (t[q].w == i) ch_sub_term(ax, ay, az, tg[r + 3], ts[0][r + 3], ts[1][r + 3], ts[2][r + 3], ox, oy, oz);
                }
            }
        }
    }
    if (i < s.no) {
        s.out[(size_t)i * 3] = ax;
        s.out[(size_t)i * 3 + 1] = ay;
        s.out[(size_t)i * 3 + 2] = az;
    }
}

// 0: refuse, 1: nothing to do, 2: launch
static int chamfer_check(int b, int n, int m) {
    if (b < 0 || n < 1 || m < 1 || n > CH_MAX_POINTS || m > CH_MAX_POINTS) return 0;
    if ((long long)b * (n > m ? n : m) >= (1ll << 24)) return 0;
    return b == 0 ? 1 : 2;
}

}  // namespace apn

extern "C" int apn_chamfer_max_points(void) { return apn::CH_MAX_POINTS; }

extern "C" int apn_chamfer_forward(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1, float *dist2,
                                   int *idx1, int *idx2, void *stream) {
    using namespace apn;
    const int what = chamfer_check(b, n, m);
    if (what == 0) return APN_EINVAL;
    if (what == 1) return APN_OK;
    if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2) return APN_EINVAL;
    if ((n > m ? n : m) <= CH_SMALL) {
        const unsigned grid = (unsigned)((2ll * b + CH_WAVES - 1) / CH_WAVES);
        hipLaunchKernelGGL(chamfer_fwd_small_kernel, dim3(grid), dim3(CH_THREADS), 0, (hipStream_t)stream, b, n, m, xyz1,
                           xyz2, dist1, dist2, idx1, idx2);
    } else {
        const int tiles1 = (n + CH_SRC - 1) / CH_SRC, tiles2 = (m + CH_SRC - 1) / CH_SRC;
        const unsigned grid = (unsigned)((long long)b * (tiles1 + tiles2));          // <= 2 (2^24 / 64 + b) < 2^20
        hipLaunchKernelGGL(chamfer_fwd_kernel, dim3(grid), dim3(CH_THREADS), 0, (hipStream_t)stream, n, m, tiles1, tiles2,
                           xyz1, xyz2, dist1, dist2, idx1, idx2);
    }
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_chamfer_backward(int b, int n, int m, const float *xyz1, const float *xyz2, const int *idx1,
                                    const int *idx2, const float *grad_dist1, const float *grad_dist2, float *grad_xyz1,
                                    float *grad_xyz2, void *stream) {
    using namespace apn;
    const int what = chamfer_check(b, n, m);
    if (what == 0) return APN_EINVAL;
    if (what == 1) return APN_OK;
    if (!xyz1 || !xyz2 || !idx1 || !idx2 || !grad_dist1 || !grad_dist2 || !grad_xyz1 || !grad_xyz2) return APN_EINVAL;
    if ((n > m ? n : m) <= CH_SMALL) {
        const unsigned grid = (unsigned)((2ll * b + CH_WAVES - 1) / CH_WAVES);
        hipLaunchKernelGGL(chamfer_bwd_small_kernel, dim3(grid), dim3(CH_THREADS), 0, (hipStream_t)stream, b, n, m, xyz1,
                           xyz2, idx1, idx2, grad_dist1, grad_dist2, grad_xyz1, grad_xyz2);
    } else {
        const int tiles1 = (n + CH_THREADS - 1) / CH_THREADS, tiles2 = (m + CH_THREADS - 1) / CH_THREADS;
        const unsigned grid = (unsigned)((long long)b * (tiles1 + tiles2));
        hipLaunchKernelGGL(chamfer_bwd_kernel, dim3(grid), dim3(CH_THREADS), 0, (hipStream_t)stream, n, m, tiles1, tiles2,
                           xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2, grad_xyz1, grad_xyz2);
    }
    APN_LAUNCH_CHECK();
    return APN_OK;
}
