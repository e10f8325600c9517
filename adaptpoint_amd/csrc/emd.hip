// emd.hip -- approximate earth mover's distance (the reference's `emd_cuda` module) without the (b,m,n) tensor on the hot
// path: apn_emd_ratios / apn_emd_match / apn_emd_cost / apn_emd_cost_grad; the contract is in include/adaptpoint_amd.h.
//
// The reference's `match` is a sum over ten annealing levels of weights e_q(d[l,k]) ratioL_q[k] ratioR_q[l], so the two
// tables ratio_l (b,10,n) and ratio_r (b,10,m) determine it.  The iteration that makes them needs O(n + m) state per
// cloud; `match` is written once at the end by a kernel with no dependence between its elements (apn_emd_match), and the
// cost and its gradient recompute each match[l,k] from the tables in registers (ten v_exp_f32 per pair) instead of
// reading 4 bytes of a tensor that would have to be written first.
//
// Every pass of a level is a ROW sum -- suml and the remainL update run per k over l, sumr per l over k -- so a row has
// one owner and nothing is reduced across workgroups.  Two shapes of the iteration:
//   one launch, max(n, m) <= EMD_ONE_MAX: a workgroup per cloud, thread = row, both clouds and the remainders in LDS,
//     __syncthreads between the passes; the columns go by in ascending order, four per 16-byte LDS broadcast.
//   split, beyond it: a workgroup owns 64 rows (lane = row in each of its W waves; W = 8 from max(n, m) = 256 on, 4
//     below), stages the columns through LDS in chunks of 1024 and gives each wave an equal run of every chunk; a
//     row's sum is the waves' sums added in wave order.  Kernel boundaries are the only seams between the passes: no
//     grid barrier, no flag.  remainR is final after a level's second pass, so the third pass of level q and the first
//     of level q + 1 share one sweep (one distance, two exponentials): 20 launches.
// The pair kernels (match, cost, gradient) have the split form's geometry for every shape.
//
// Arithmetic: plain scalar fp32, one rounding per operation (the unit is built with -ffp-contract=off); the only fma
// is the distance's; no float atomics.  emd_exp is the one exponential of this file.
#include "apn_common.h"

namespace apn {

constexpr int EMD_LEVELS = 10;
constexpr int EMD_MAX_POINTS = 8192;                    // apn_emd_max_points()
constexpr int EMD_ONE_MAX = 128;                        // apn_emd_one_launch_max(): max(n, m) up to here takes one launch
constexpr int EMD_WAVES = 8;                            // waves of a workgroup at most: emd_threads()
constexpr int EMD_THREADS = EMD_WAVES * APN_WAVE;
constexpr int EMD_WIDE = 256;                           // max(n, m) from here on: 8 waves per workgroup, below: 4
constexpr int EMD_ROWS = APN_WAVE;                      // rows per workgroup (one per lane)
constexpr int EMD_CHUNK = 1024;                         // columns staged per chunk
constexpr float EMD_LOG2E = 1.44269504088896340736f;
constexpr float EMD_EPS = 1e-9f;

// level_q = -4^(7 - q), and 0 at q = 9 (the reference's j = 7 .. -2)
__host__ __device__ constexpr float emd_level(int q) {
    return q >= EMD_LEVELS - 1 ? 0.0f : (q == EMD_LEVELS - 2 ? -0.25f : -(float)(1 << (14 - 2 * q)));
}

// exp(level d) as the hardware's exp2; `c` is the pair's d * log2(e), rounded once and shared by the levels.  A level is
// a power of two or 0, so level * c is exact (= the rounded (level * d) * log2(e)); it is <= 0, the result lies in [0, 1]
__device__ __forceinline__ float emd_exp(float level, float c) { return __builtin_amdgcn_exp2f(level * c); }

// |column - row|^2 in the project's form; the squares do not see which way round the difference is taken
__device__ __forceinline__ float emd_dist(float rx, float ry, float rz, float cx, float cy, float cz) {
    return dist2(cy - ry, cx - rx, cz - rz);
}

// the sum of a row's per-wave runs, in wave order
__device__ __forceinline__ float emd_fold(const float (*part)[APN_WAVE], int waves, int lane) {
    float sum = part[0][lane];
    for (int w = 1; w < waves; ++w) sum += part[w][lane];
    return sum;
}

// a wave's run of a chunk of `padded` columns (a multiple of 4): the chunk is cut into `waves` runs of whole float4s
__device__ __forceinline__ int emd_run(int padded, int waves) { return ((padded / 4 + waves - 1) / waves) * 4; }

// match[l,k] from the tables: (e_q ratioL_q[k]) ratioR_q[l] summed over q ascending; `rev`: the row is l
__device__ __forceinline__ float emd_match_at(float c, const float (&rt)[EMD_LEVELS], const float (&ct)[EMD_LEVELS], bool rev) {
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < EMD_LEVELS; ++q) {
        const float e = emd_exp(emd_level(q), c);
        acc += rev ? (e * ct[q]) * rt[q] : (e * rt[q]) * ct[q];
    }
    return acc;
}

// The split kernels' LDS is sized at launch: rows of `stride` = min(EMD_CHUNK, max(n, m) rounded up to 4) floats -- three
// of coordinates, then the kernel's per-column values -- and behind them the waves' partial sums [..][EMD_WAVES][64].
extern __shared__ __align__(16) float emd_lds[];

// columns j0 .. j0 + cnt - 1 of a cloud into structure-of-arrays LDS, the pad up to `padded` zeroed
__device__ __forceinline__ void emd_stage_xyz(float *cs, int stride, const float *g, int cnt, int padded, int tid) {
    for (int e = tid; e < padded * 3; e += blockDim.x) {
        const int j = e / 3, c = e - j * 3;
        cs[c * stride + j] = j < cnt ? g[e] : 0.0f;
    }
}

__device__ __forceinline__ void emd_stage_row(float *dst, const float *g, int cnt, int padded, int tid) {
    for (int j = tid; j < padded; j += blockDim.x) dst[j] = j < cnt ? g[j] : 0.0f;
}

__device__ __forceinline__ float emd_f4(const float4 &v, int u) { return u == 0 ? v.x : (u == 1 ? v.y : (u == 2 ? v.z : v.w)); }

// ---------------------------------------------------------------------------------------------------------------------
// The iteration, one launch: thread = row of both clouds.
template <int T>
__global__ __launch_bounds__(T) void emd_one_kernel(int n, int m, float multi_l, float multi_r,
                                                    const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                    float *__restrict__ ratio_l, float *__restrict__ ratio_r) {
    __shared__ __align__(16) float s1[3][EMD_ONE_MAX];
    __shared__ __align__(16) float s2[3][EMD_ONE_MAX];
    __shared__ __align__(16) float s_ratl[EMD_ONE_MAX];
    __shared__ __align__(16) float s_ratr[EMD_ONE_MAX];
    __shared__ __align__(16) float s_remr[EMD_ONE_MAX];
    const int tid = threadIdx.x;
    const size_t cloud = blockIdx.x;
    const float *g1 = xyz1 + cloud * n * 3, *g2 = xyz2 + cloud * m * 3;
    for (int e = tid; e < EMD_ONE_MAX * 3; e += T) {
        const int j = e / 3, c = e - j * 3;
        s1[c][j] = j < n ? g1[e] : 0.0f;
        s2[c][j] = j < m ? g2[e] : 0.0f;
    }
    for (int j = tid; j < EMD_ONE_MAX; j += T) {         // the pads stay zero: a padded column adds +0
        s_ratl[j] = 0.0f;
        s_ratr[j] = 0.0f;
        s_remr[j] = j < m ? multi_r : 0.0f;
    }
    __syncthreads();
    const int n4 = (n + 3) & ~3, m4 = (m + 3) & ~3;
    const bool isk = tid < n, isl = tid < m;
    const float x1 = s1[0][tid], y1 = s1[1][tid], z1 = s1[2][tid];
    const float x2 = s2[0][tid], y2 = s2[1][tid], z2 = s2[2][tid];
    float rem_l = multi_l, rem_r = multi_r, rat_l = 0.0f;
    if (isk) {                                           // first pass of level 0
        const float lv = emd_level(0);
        float sum = 0.0f;
        for (int j = 0; j < m4; j += 4) {
            const float4 cx = *reinterpret_cast<const float4 *>(&s2[0][j]);
            const float4 cy = *reinterpret_cast<const float4 *>(&s2[1][j]);
            const float4 cz = *reinterpret_cast<const float4 *>(&s2[2][j]);
            const float4 rr = *reinterpret_cast<const float4 *>(&s_remr[j]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                sum += emd_exp(lv, emd_dist(x1, y1, z1, emd_f4(cx, u), emd_f4(cy, u), emd_f4(cz, u)) * EMD_LOG2E) * emd_f4(rr, u);
        }
        rat_l = rem_l / (EMD_EPS + sum);
    }
    for (int q = 0; q < EMD_LEVELS; ++q) {
        const float lv = emd_level(q), lv_next = emd_level(q + 1);
        if (isk) {
            s_ratl[tid] = rat_l;
            ratio_l[(cloud * EMD_LEVELS + q) * n + tid] = rat_l;
        }
        __syncthreads();
        if (isl) {                                       // second pass: per l over k
            float sum = 0.0f;
            for (int j = 0; j < n4; j += 4) {
                const float4 cx = *reinterpret_cast<const float4 *>(&s1[0][j]);
                const float4 cy = *reinterpret_cast<const float4 *>(&s1[1][j]);
                const float4 cz = *reinterpret_cast<const float4 *>(&s1[2][j]);
                const float4 rl = *reinterpret_cast<const float4 *>(&s_ratl[j]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    sum += emd_exp(lv, emd_dist(x2, y2, z2, emd_f4(cx, u), emd_f4(cy, u), emd_f4(cz, u)) * EMD_LOG2E) * emd_f4(rl, u);
            }
            const float sumr = sum * rem_r;
            const float rat_r = fminf(rem_r / (sumr + EMD_EPS), 1.0f) * rem_r;
            rem_r = fmaxf(0.0f, rem_r - sumr);
            s_ratr[tid] = rat_r;
            s_remr[tid] = rem_r;
            ratio_r[(cloud * EMD_LEVELS + q) * m + tid] = rat_r;
        }
        __syncthreads();
        if (q == EMD_LEVELS - 1) break;                  // the last level's remainL is never read
        if (isk) {                                       // third pass of level q and first of level q + 1: per k over l
            float sum_c = 0.0f, sum_a = 0.0f;
            for (int j = 0; j < m4; j += 4) {
                const float4 cx = *reinterpret_cast<const float4 *>(&s2[0][j]);
                const float4 cy = *reinterpret_cast<const float4 *>(&s2[1][j]);
                const float4 cz = *reinterpret_cast<const float4 *>(&s2[2][j]);
                const float4 rr = *reinterpret_cast<const float4 *>(&s_ratr[j]);
                const float4 mr = *reinterpret_cast<const float4 *>(&s_remr[j]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float c = emd_dist(x1, y1, z1, emd_f4(cx, u), emd_f4(cy, u), emd_f4(cz, u)) * EMD_LOG2E;
                    sum_c += (emd_exp(lv, c) * rat_l) * emd_f4(rr, u);
                    sum_a += emd_exp(lv_next, c) * emd_f4(mr, u);
                }
            }
            rem_l = fmaxf(0.0f, rem_l - sum_c);
            rat_l = rem_l / (EMD_EPS + sum_a);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The iteration, split: PASS 0 = first pass of level 0 (rows k); PASS 1 = second pass of level q (rows l); PASS 2 = third
// pass of level q with the first pass of level q + 1 (rows k).  At q == 0 the remainders are the multipliers: `state`
// is not read before it is written.
template <int PASS>
__global__ __launch_bounds__(EMD_THREADS) void emd_pass_kernel(int n, int m, int tiles, int stride, int q, float lv,
                                                               float lv_next, float multi_l, float multi_r,
                                                               const float *__restrict__ xyz1,
                                                               const float *__restrict__ xyz2, float *ratio_l,
                                                               float *ratio_r, float *state) {
    constexpr int NX = PASS == 2 ? 2 : 1;
    float *cs = emd_lds, *ex0 = emd_lds + 3 * stride, *ex1 = emd_lds + (2 + NX) * stride;
    float (*part)[APN_WAVE] = reinterpret_cast<float (*)[APN_WAVE]>(emd_lds + (3 + NX) * stride);
    const int tid = threadIdx.x;
    const int lane = tid & (APN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / APN_WAVE);
    const int waves = blockDim.x / APN_WAVE;
    const size_t cloud = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)cloud * tiles;
    const int nr = PASS == 1 ? m : n, nc = PASS == 1 ? n : m;
    const float *rowp = (PASS == 1 ? xyz2 : xyz1) + cloud * nr * 3;
    const float *colp = (PASS == 1 ? xyz1 : xyz2) + cloud * nc * 3;
    float *rem_l = state + cloud * (n + m), *rem_r = rem_l + n;
    float *rl_q = ratio_l + (cloud * EMD_LEVELS + q) * n;
    float *rr_q = ratio_r + (cloud * EMD_LEVELS + q) * m;
    const int i = tile * EMD_ROWS + lane;
    const int ic = i < nr ? i : nr - 1;                  // rows past the cloud repeat the last row (never written)
    const float rx = rowp[ic * 3], ry = rowp[ic * 3 + 1], rz = rowp[ic * 3 + 2];
    const float rat_l = PASS == 2 ? rl_q[ic] : 0.0f;
    float acc0 = 0.0f, acc1 = 0.0f;
    for (int j0 = 0; j0 < nc; j0 += EMD_CHUNK) {
        const int cnt = nc - j0 < EMD_CHUNK ? nc - j0 : EMD_CHUNK;
        const int padded = (cnt + 3) & ~3;
        __syncthreads();                                 // the previous chunk has been read
        emd_stage_xyz(cs, stride, colp + (size_t)j0 * 3, cnt, padded, tid);
        if (PASS == 0) {
            for (int j = tid; j < padded; j += blockDim.x) ex0[j] = j < cnt ? multi_r : 0.0f;
        } else if (PASS == 1) {
            emd_stage_row(ex0, rl_q + j0, cnt, padded, tid);
        } else {
            emd_stage_row(ex0, rr_q + j0, cnt, padded, tid);
            emd_stage_row(ex1, rem_r + j0, cnt, padded, tid);
        }
        __syncthreads();
        const int run = emd_run(padded, waves);
        const int lo = wave * run, hi = lo + run < padded ? lo + run : padded;
        for (int j = lo; j < hi; j += 4) {
            const float4 cx = *reinterpret_cast<const float4 *>(cs + j);
            const float4 cy = *reinterpret_cast<const float4 *>(cs + stride + j);
            const float4 cz = *reinterpret_cast<const float4 *>(cs + 2 * stride + j);
            const float4 x0 = *reinterpret_cast<const float4 *>(ex0 + j);
            const float4 x1 = *reinterpret_cast<const float4 *>(ex1 + j);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float c = emd_dist(rx, ry, rz, emd_f4(cx, u), emd_f4(cy, u), emd_f4(cz, u)) * EMD_LOG2E;
                if (PASS == 2) {
                    acc0 += (emd_exp(lv, c) * rat_l) * emd_f4(x0, u);
                    acc1 += emd_exp(lv_next, c) * emd_f4(x1, u);
                } else {
                    acc0 += emd_exp(lv, c) * emd_f4(x0, u);
                }
            }
        }
    }
    part[wave][lane] = acc0;
    if (PASS == 2) part[(NX - 1) * EMD_WAVES + wave][lane] = acc1;
    __syncthreads();
    if (wave != 0 || i >= nr) return;
    const float sum0 = emd_fold(part, waves, lane);
    if (PASS == 0) {
        rl_q[i] = multi_l / (EMD_EPS + sum0);
    } else if (PASS == 1) {
        const float r = q == 0 ? multi_r : rem_r[i];
        const float sumr = sum0 * r;
        rr_q[i] = fminf(r / (sumr + EMD_EPS), 1.0f) * r;
        rem_r[i] = fmaxf(0.0f, r - sumr);
    } else {
        const float sum1 = emd_fold(part + (NX - 1) * EMD_WAVES, waves, lane);
        const float r = fmaxf(0.0f, (q == 0 ? multi_l : rem_l[i]) - sum0);
        rem_l[i] = r;
        rl_q[n + i] = r / (EMD_EPS + sum1);                  // rl_q + n: level q + 1 of the same cloud
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The pair kernels: every (l,k) of a cloud once per direction, match[l,k] from the tables (TAB) or from memory.
//   EMD_MATCH  rows k, writes match                     EMD_COST  rows k, writes a tile's sum of d * match to `out1`
//   EMD_GRAD   rows k (grad1) and rows l (grad2)
enum { EMD_MATCH = 0, EMD_COST = 1, EMD_GRAD = 2 };

template <int MODE, bool TAB>
__global__ __launch_bounds__(EMD_THREADS) void emd_pair_kernel(int n, int m, int tiles1, int tiles2, int stride,
                                                               const float *__restrict__ xyz1,
                                                               const float *__restrict__ xyz2,
                                                               const float *__restrict__ match,
                                                               const float *__restrict__ ratio_l,
                                                               const float *__restrict__ ratio_r,
                                                               const float *__restrict__ grad_cost, float *out1, float *out2) {
    constexpr int NT = TAB ? EMD_LEVELS : 1;
    constexpr int NP = MODE == EMD_GRAD ? 3 : 1;
    float *cs = emd_lds, *ct = emd_lds + 3 * stride;
    float (*part)[APN_WAVE] = reinterpret_cast<float (*)[APN_WAVE]>(emd_lds + (3 + NT) * stride);
    const int tid = threadIdx.x;
    const int lane = tid & (APN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / APN_WAVE);
    const int waves = blockDim.x / APN_WAVE;
    const int per = tiles1 + tiles2;
    const size_t cloud = blockIdx.x / per;
    int tile = blockIdx.x - (int)cloud * per;
    const bool rev = tile >= tiles1;                     // rows l
    if (rev) tile -= tiles1;
    const int nr = rev ? m : n, nc = rev ? n : m;
    const float *rowp = (rev ? xyz2 : xyz1) + cloud * nr * 3;
    const float *colp = (rev ? xyz1 : xyz2) + cloud * nc * 3;
    const float *rtab = (rev ? ratio_r : ratio_l), *ctab = (rev ? ratio_l : ratio_r);
    const int i = tile * EMD_ROWS + lane;
    const int ic = i < nr ? i : nr - 1;                  // rows past the cloud repeat the last row (never written)
    const float rx = rowp[ic * 3], ry = rowp[ic * 3 + 1], rz = rowp[ic * 3 + 2];
    float rt[EMD_LEVELS];
#pragma unroll
    for (int q = 0; q < EMD_LEVELS; ++q) rt[q] = TAB ? rtab[(cloud * EMD_LEVELS + q) * nr + ic] : 0.0f;
    const float *mbase = TAB ? nullptr : match + cloud * m * n;     // 64-bit element offsets
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int j0 = 0; j0 < nc; j0 += EMD_CHUNK) {
        const int cnt = nc - j0 < EMD_CHUNK ? nc - j0 : EMD_CHUNK;
        const int padded = (cnt + 3) & ~3;
        __syncthreads();                                 // the previous chunk has been read
        emd_stage_xyz(cs, stride, colp + (size_t)j0 * 3, cnt, padded, tid);
        if constexpr (TAB) {
#pragma unroll
            for (int q = 0; q < NT; ++q) emd_stage_row(ct + q * stride, ctab + (cloud * EMD_LEVELS + q) * nc + j0, cnt, padded, tid);
        }
        __syncthreads();
        const int run = emd_run(padded, waves);
        const int lo = wave * run, hi = lo + run < padded ? lo + run : padded;
        for (int j = lo; j < hi; j += 4) {
            const float4 cx = *reinterpret_cast<const float4 *>(cs + j);
            const float4 cy = *reinterpret_cast<const float4 *>(cs + stride + j);
            const float4 cz = *reinterpret_cast<const float4 *>(cs + 2 * stride + j);
            float4 t4[NT];
            if constexpr (TAB) {
#pragma unroll
                for (int q = 0; q < NT; ++q) t4[q] = *reinterpret_cast<const float4 *>(ct + q * stride + j);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float px = emd_f4(cx, u), py = emd_f4(cy, u), pz = emd_f4(cz, u);
                const float d = emd_dist(rx, ry, rz, px, py, pz);
                const int col = j0 + j + u;
                const bool live = j + u < cnt;
                float mt;
                if constexpr (TAB) {
                    float cv[EMD_LEVELS];
#pragma unroll
                    for (int q = 0; q < EMD_LEVELS; ++q) cv[q] = emd_f4(t4[q], u);
                    mt = emd_match_at(d * EMD_LOG2E, rt, cv, rev);
                } else {
                    const size_t at = rev ? (size_t)ic * n + col : (size_t)col * n + ic;      // match[l][k]
                    mt = live ? mbase[at] : 0.0f;
                }
                if constexpr (MODE == EMD_MATCH) {
                    if (live && i < nr) out1[(cloud * m + col) * n + i] = mt;
                } else if constexpr (MODE == EMD_COST) {
                    a0 += d * mt;
                } else {
                    const float w = mt * 2.0f;
                    a0 += (rx - px) * w;
                    a1 += (ry - py) * w;
                    a2 += (rz - pz) * w;
                }
            }
        }
    }
    if constexpr (MODE == EMD_MATCH) return;
    part[wave][lane] = a0;
    if constexpr (MODE == EMD_GRAD) {
        part[EMD_WAVES + wave][lane] = a1;
        part[2 * EMD_WAVES + wave][lane] = a2;
    }
    __syncthreads();
    if (wave != 0) return;
    float s[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) s[c] = emd_fold(part + c * EMD_WAVES, waves, lane);
    if constexpr (MODE == EMD_COST) {
        // the tile's rows in ascending order: lane 0 walks them (rows past the cloud are left out)
        const int rows = nr - tile * EMD_ROWS < EMD_ROWS ? nr - tile * EMD_ROWS : EMD_ROWS;
        float total = 0.0f;
        for (int r = 0; r < rows; ++r) total += readlane_f(s[0], r);
        if (lane == 0) out1[cloud * tiles1 + tile] = total;
    } else if constexpr (MODE == EMD_GRAD) {
        if (i >= nr) return;
        const float g = grad_cost[cloud];
        float *out = (rev ? out2 : out1) + (cloud * nr + i) * 3;
        out[0] = s[0] * g;
        out[1] = s[1] * g;
        out[2] = s[2] * g;
    }
}

// cost[c] = the ascending sum of the cloud's tile sums
__global__ __launch_bounds__(256) void emd_cost_fold_kernel(int b, int tiles, const float *__restrict__ part,
                                                                    float *__restrict__ cost) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= b) return;
    float total = 0.0f;
    for (int t = 0; t < tiles; ++t) total += part[(size_t)c * tiles + t];
    cost[c] = total;
}

// 0: refuse, 1: nothing to do, 2: launch
static int emd_check(int b, int n, int m) {
    if (b < 0 || n < 1 || m < 1 || n > EMD_MAX_POINTS || m > EMD_MAX_POINTS) return 0;
    if ((long long)b * (n > m ? n : m) >= (1ll << 24)) return 0;
    return b == 0 ? 1 : 2;
}

static int emd_tiles(int rows) { return (rows + EMD_ROWS - 1) / EMD_ROWS; }

// threads of a workgroup: the columns of a chunk are cut over 4 waves for small clouds, over 8 from EMD_WIDE on
// the LDS row length of the split kernels, and their LDS bytes with `rows` per-column rows and `sums` partial sums
static int emd_stride(int n, int m) {
    const int big = ((n > m ? n : m) + 3) & ~3;
    return big < EMD_CHUNK ? big : EMD_CHUNK;
}
static size_t emd_lds_bytes(int stride, int rows, int sums) {
    return sizeof(float) * ((size_t)(3 + rows) * stride + (size_t)sums * EMD_WAVES * APN_WAVE);
}

static unsigned emd_threads(int n, int m) { return ((n > m ? n : m) >= EMD_WIDE ? EMD_WAVES : EMD_WAVES / 2) * APN_WAVE; }

}  // namespace apn

extern "C" int apn_emd_max_points(void) { return apn::EMD_MAX_POINTS; }
extern "C" int apn_emd_one_launch_max(void) { return apn::EMD_ONE_MAX; }
extern "C" int apn_emd_cost_parts(int n) { return n < 1 || n > apn::EMD_MAX_POINTS ? 0 : apn::emd_tiles(n); }

extern "C" int apn_emd_ratios(int b, int n, int m, const float *xyz1, const float *xyz2, float *ratio_l, float *ratio_r,
                              float *state, void *stream) {
    using namespace apn;
    const int what = emd_check(b, n, m);
    if (what == 0) return APN_EINVAL;
    if (what == 1) return APN_OK;
    if (!xyz1 || !xyz2 || !ratio_l || !ratio_r || !state) return APN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const float multi_l = n >= m ? 1.0f : (float)(m / n), multi_r = n >= m ? (float)(n / m) : 1.0f;   // integer division
    const int big = n > m ? n : m;
    if (big <= EMD_ONE_MAX) {
        if (big <= 64)
            hipLaunchKernelGGL(emd_one_kernel<64>, dim3((unsigned)b), dim3(64), 0, s, n, m, multi_l, multi_r, xyz1, xyz2,
                               ratio_l, ratio_r);
        else
            hipLaunchKernelGGL(emd_one_kernel<EMD_ONE_MAX>, dim3((unsigned)b), dim3(EMD_ONE_MAX), 0, s, n, m, multi_l,
                               multi_r, xyz1, xyz2, ratio_l, ratio_r);
        APN_LAUNCH_CHECK();
        return APN_OK;
    }
    const int tl = emd_tiles(n), tr = emd_tiles(m);
    const dim3 gl((unsigned)((long long)b * tl)), gr((unsigned)((long long)b * tr)), blk(emd_threads(n, m));
    const int stride = emd_stride(n, m);
    hipLaunchKernelGGL(emd_pass_kernel<0>, gl, blk, emd_lds_bytes(stride, 1, 1), s, n, m, tl, stride, 0, emd_level(0), 0.0f,
                       multi_l, multi_r, xyz1, xyz2, ratio_l, ratio_r, state);
    APN_LAUNCH_CHECK();
    for (int q = 0; q < EMD_LEVELS; ++q) {
        hipLaunchKernelGGL(emd_pass_kernel<1>, gr, blk, emd_lds_bytes(stride, 1, 1), s, n, m, tr, stride, q, emd_level(q),
                           0.0f, multi_l, multi_r, xyz1, xyz2, ratio_l, ratio_r, state);
        APN_LAUNCH_CHECK();
        if (q == EMD_LEVELS - 1) break;                  // the last level's remainL is never read
        hipLaunchKernelGGL(emd_pass_kernel<2>, gl, blk, emd_lds_bytes(stride, 2, 2), s, n, m, tl, stride, q, emd_level(q),
                           emd_level(q + 1), multi_l, multi_r, xyz1, xyz2, ratio_l, ratio_r, state);
        APN_LAUNCH_CHECK();
    }
    return APN_OK;
}

extern "C" int apn_emd_match(int b, int n, int m, const float *xyz1, const float *xyz2, const float *ratio_l,
                             const float *ratio_r, float *match, void *stream) {
    using namespace apn;
    const int what = emd_check(b, n, m);
    if (what == 0) return APN_EINVAL;
    if (what == 1) return APN_OK;
    if (!xyz1 || !xyz2 || !ratio_l || !ratio_r || !match) return APN_EINVAL;
    const int tl = emd_tiles(n);
    const int stride = emd_stride(n, m);
    hipLaunchKernelGGL((emd_pair_kernel<EMD_MATCH, true>), dim3((unsigned)((long long)b * tl)), dim3(emd_threads(n, m)),
                       emd_lds_bytes(stride, EMD_LEVELS, 0), (hipStream_t)stream, n, m, tl, 0, stride, xyz1, xyz2,
                       (const float *)nullptr, ratio_l, ratio_r, (const float *)nullptr, match, (float *)nullptr);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_emd_cost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                            const float *ratio_l, const float *ratio_r, float *part, float *cost, void *stream) {
    using namespace apn;
    const int what = emd_check(b, n, m);
    if (what == 0) return APN_EINVAL;
    if (what == 1) return APN_OK;
    if (!xyz1 || !xyz2 || !part || !cost || (!match && (!ratio_l || !ratio_r))) return APN_EINVAL;
    const int tl = emd_tiles(n);
    const dim3 grid((unsigned)((long long)b * tl)), blk(emd_threads(n, m));
    const int stride = emd_stride(n, m);
    if (match)
        hipLaunchKernelGGL((emd_pair_kernel<EMD_COST, false>), grid, blk, emd_lds_bytes(stride, 1, 1), (hipStream_t)stream, n,
                           m, tl, 0, stride, xyz1, xyz2, match, ratio_l, ratio_r, (const float *)nullptr, part, (float *)nullptr);
    else
        hipLaunchKernelGGL((emd_pair_kernel<EMD_COST, true>), grid, blk, emd_lds_bytes(stride, EMD_LEVELS, 1),
                           (hipStream_t)stream, n, m, tl, 0, stride, xyz1, xyz2, match, ratio_l, ratio_r,
                           (const float *)nullptr, part, (float *)nullptr);
    APN_LAUNCH_CHECK();
    hipLaunchKernelGGL(emd_cost_fold_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, b, tl, part, cost);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_emd_cost_grad(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2,
                                 const float *match, const float *ratio_l, const float *ratio_r, float *grad1,
                                 float *grad2, void *stream) {
    using namespace apn;
    const int what = emd_check(b, n, m);
    if (what == 0) return APN_EINVAL;
    if (what == 1) return APN_OK;
    if (!grad_cost || !xyz1 || !xyz2 || !grad1 || !grad2 || (!match && (!ratio_l || !ratio_r))) return APN_EINVAL;
    const int tl = emd_tiles(n), tr = emd_tiles(m);
    const dim3 grid((unsigned)((long long)b * (tl + tr))), blk(emd_threads(n, m));
    const int stride = emd_stride(n, m);
    if (match)
        hipLaunchKernelGGL((emd_pair_kernel<EMD_GRAD, false>), grid, blk, emd_lds_bytes(stride, 1, 3), (hipStream_t)stream, n,
                           m, tl, tr, stride, xyz1, xyz2, match, ratio_l, ratio_r, grad_cost, grad1, grad2);
    else
        hipLaunchKernelGGL((emd_pair_kernel<EMD_GRAD, true>), grid, blk, emd_lds_bytes(stride, EMD_LEVELS, 3),
                           (hipStream_t)stream, n, m, tl, tr, stride, xyz1, xyz2, match, ratio_l, ratio_r, grad_cost, grad1,
                           grad2);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
