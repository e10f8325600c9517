// pointops.hip -- the operators on STACKED clouds (the reference's `pointops_cuda` module): points (n,3), features
// (n,c), and an int32 offset (b) of cumulative end rows, so that every cloud has its own size; queries (m,...) come
// with their own new_offset (b).  Contract: include/adaptpoint_amd.h; design notes: DESIGN.md section 7m.
//
//   po_knn_kernel      a workgroup owns PO_TILE consecutive query rows of the FLAT list of m queries: no host knowledge
//                      of the offsets.  Each query finds its cloud [start, end) on the device (a search bounded by b);
//                      the tile scans the union of its queries' ranges through LDS, and a candidate outside a query's
//                      own range enters that query's list as +inf, i.e. never.  The running list is csrc/knn_list.h's.
//   po_ball_kernel     one wave per query: 64 rows per step in ascending index, hits compacted by a ballot, early exit.
//   po_fps_kernel      one workgroup per cloud; the cloud's coordinates and running minima live in registers (PER rows per
//                      thread, 24 * 1024 at the most) or, beyond that, stream from memory (PER = 0).  The reference's
//                      positional tie rule is a 64-bit integer key, see po_fps_kernel.
//   gather / list      elementwise forward kernels, and ONE backward kernel template that walks the reverse list of a
//                      support row (apn_po_csr, csrc/edge_conv.hip) in list order: no float atomics anywhere.
//
// Every sum starts from its first term and adds the others one by one in the stated order, each product rounded before
// it is added (the unit is built with -ffp-contract=off; po_d2 holds the file's only fma).
#include "apn_common.h"
#include "knn_list.h"

namespace apn {

constexpr int PO_WAVES = 4;
constexpr int PO_QPW = 4;                               // queries per wave
constexpr int PO_TILE = PO_WAVES * PO_QPW;              // queries per workgroup
constexpr int PO_THREADS = PO_WAVES * APN_WAVE;
constexpr int PO_CHUNK = 1024;                          // support rows staged per chunk (12 KiB)
constexpr int PO_K_MAX = 100;                           // the reference's array bound
constexpr int PO_ROWS_MAX = 1 << 24;
constexpr int PO_FPS_PER_MAX = 24;                      // rows per thread held in registers
constexpr float PO_FAR = 1e10f;                         // the reference's initial heap / tmp value

// apn_knn_query's squared distance at c = 3
__device__ __forceinline__ float po_d2(float tx, float ty, float tz) {
    return __builtin_fmaf(tz, tz, __builtin_fmaf(ty, ty, tx * tx));
}

// the cloud of query row q: the first i with q < new_offset[i]; a row at or past new_offset[b-1] belongs to the last
__device__ __forceinline__ int po_cloud(int q, int b, const int *__restrict__ new_offset) {
    int i = 0;
    while (i < b - 1 && q >= new_offset[i]) ++i;
    return i;
}

// the support rows [st, en) of cloud ci, clamped into [0, n]
__device__ __forceinline__ void po_range(int ci, int n, const int *__restrict__ offset, int &st, int &en) {
    st = ci > 0 ? offset[ci - 1] : 0;
    en = offset[ci];
    st = st < 0 ? 0 : (st > n ? n : st);
    en = en < st ? st : (en > n ? n : en);
}

__device__ __forceinline__ int po_clamp(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }

// ------------------------------------------------------------------------------------------------------- kNN
template <int R>
__global__ __launch_bounds__(PO_THREADS) void po_knn_kernel(int b, int n, int m, int k, const float *xyz,
                                                            const float *new_xyz,       // may alias
                                                            const int *__restrict__ offset,
                                                            const int *__restrict__ new_offset, int *__restrict__ idx,
                                                            float *__restrict__ dist2) {
    __shared__ __align__(16) float qs[3][PO_TILE];
    __shared__ int qlo[PO_TILE], qhi[PO_TILE];
    __shared__ float ss[3][PO_CHUNK + 1];
    const int tid = threadIdx.x;
    const int lane = tid & (APN_WAVE - 1);
    const int wave = tid / APN_WAVE;
    const int q0 = blockIdx.x * PO_TILE;
    const int tl = (k - 1) & (APN_WAVE - 1);

    if (tid < PO_TILE) {                                 // rows past m repeat the last query (computed, never written)
        const int q = q0 + tid < m ? q0 + tid : m - 1;
        int st, en;
        po_range(po_cloud(q, b, new_offset), n, offset, st, en);
        qlo[tid] = st;
        qhi[tid] = en;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) qs[ci][tid] = new_xyz[(size_t)q * 3 + ci];
    }
    __syncthreads();
    int lo = n, hi = 0;                                  // the union of the tile's ranges
#pragma unroll
    for (int t = 0; t < PO_TILE; ++t) {
        lo = qlo[t] < lo ? qlo[t] : lo;
        hi = qhi[t] > hi ? qhi[t] : hi;
    }
    int mylo[PO_QPW], myhi[PO_QPW], wlo = n, whi = 0;    // wave-uniform: this wave's four queries
    float ld[PO_QPW][R];
    int li[PO_QPW][R];
#pragma unroll
    for (int t = 0; t < PO_QPW; ++t) {
        mylo[t] = qlo[wave * PO_QPW + t];
        myhi[t] = qhi[wave * PO_QPW + t];
        wlo = mylo[t] < wlo ? mylo[t] : wlo;
        whi = myhi[t] > whi ? myhi[t] : whi;
#pragma unroll
        for (int j = 0; j < R; ++j) {                    // the reference's initial heap: (1e10, start of the cloud)
            ld[t][j] = PO_FAR;
            li[t][j] = mylo[t] < n ? mylo[t] : n - 1;
        }
    }
    const float4 qx = *reinterpret_cast<const float4 *>(&qs[0][wave * PO_QPW]);
    const float4 qy = *reinterpret_cast<const float4 *>(&qs[1][wave * PO_QPW]);
    const float4 qz = *reinterpret_cast<const float4 *>(&qs[2][wave * PO_QPW]);
    const float qxs[PO_QPW] = {qx.x, qx.y, qx.z, qx.w};
    const float qys[PO_QPW] = {qy.x, qy.y, qy.z, qy.w};
    const float qzs[PO_QPW] = {qz.x, qz.y, qz.z, qz.w};

    for (int s0 = lo; s0 < hi; s0 += PO_CHUNK) {
        const int cnt = hi - s0 < PO_CHUNK ? hi - s0 : PO_CHUNK;
        __syncthreads();                                 // the previous chunk has been read
        const float *g = xyz + (size_t)s0 * 3;
        for (int e = tid; e < cnt * 3; e += PO_THREADS) {
            const int si = e / 3, ci = e - si * 3;
            ss[ci][si] = g[e];
        }
        __syncthreads();
        for (int sb = 0; sb < cnt; sb += APN_WAVE) {
            if (s0 + sb >= whi || s0 + sb + APN_WAVE <= wlo) continue;      // (wave-uniform) none of these rows is ours
            const int sl = sb + lane;
            const bool live = sl < cnt;
            const int sr = live ? sl : 0;
            const float sx = ss[0][sr], sy = ss[1][sr], sz = ss[2][sr];
            const int s = s0 + sl;
#pragma unroll
            for (int t = 0; t < PO_QPW; ++t) {
                const float d = po_d2(qxs[t] - sx, qys[t] - sy, qzs[t] - sz);
                const bool own = live && s >= mylo[t] && s < myhi[t];
                knn_insert<R>(ld[t], li[t], own ? d : __builtin_inff(), s, tl, lane);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < PO_QPW; ++t) {
        const int q = q0 + wave * PO_QPW + t;
        if (q >= m) continue;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int r = j * APN_WAVE + lane;
            if (r < k) {
                const size_t o = (size_t)q * k + r;
                idx[o] = li[t][j];
                dist2[o] = ld[t][j];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ ball query
__global__ __launch_bounds__(PO_THREADS) void po_ball_kernel(int b, int n, int m, float r2, int nsample, const float *xyz,
                                                             const float *new_xyz, const int *__restrict__ offset,
                                                             const int *__restrict__ new_offset, int *__restrict__ idx) {
    const int lane = threadIdx.x & (APN_WAVE - 1);
    const int q = blockIdx.x * PO_WAVES + threadIdx.x / APN_WAVE;
    if (q >= m) return;                                  // (wave-uniform)
    int st, en;
    po_range(po_cloud(q, b, new_offset), n, offset, st, en);
    const float qx = new_xyz[(size_t)q * 3], qy = new_xyz[(size_t)q * 3 + 1], qz = new_xyz[(size_t)q * 3 + 2];
    int *__restrict__ out = idx + (size_t)q * nsample;
    int cnt = 0, first = 0;
    for (int s0 = st; s0 < en && cnt < nsample; s0 += APN_WAVE) {
        const int s = s0 + lane;
        bool hit = false;
        if (s < en) {
            const float *p = xyz + (size_t)s * 3;
            hit = po_d2(qx - p[0], qy - p[1], qz - p[2]) < r2;
        }
        const unsigned long long mask = __ballot(hit);
        if (!mask) continue;
        if (cnt == 0) first = s0 + __builtin_ctzll(mask);
        const int rank = cnt + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (hit && rank < nsample) out[rank] = s;
        cnt += __builtin_popcountll(mask);
    }
    cnt = cnt < nsample ? cnt : nsample;
    for (int j = cnt + lane; j < nsample; j += APN_WAVE) out[j] = first;   // no hit: first == 0, the reference's zeros
}

// ------------------------------------------------------------------------------------------ furthest sampling
// The reference runs T = blockDim threads, row k on thread (k - start) mod T; a thread keeps its first maximum and the
// block tree keeps the lower slot unless the upper one is strictly greater: the winner is the maximum with the smallest
// bit-reversed (over L = log2 T bits) thread id, then the smallest k.  Here thread t < T owns the same rows, i-th row
// k = start + t + i T, and the rule is an integer maximum of
//      key = ordered(d) << 32 | ~(bitrev_L(t) << 14 | i)          (i < 2^14 as n < 2^24; T < 1024 only when n_max < 2 T)
// taken over the wave by DPP and over the waves through LDS; threads beyond T (a workgroup is at least one full wave)
// and threads without rows carry key 0, below every real row's.  The winner hands its coordinates over through LDS.
template <int PER>
__global__ __launch_bounds__(1024) void po_fps_kernel(int T, int L, const float *__restrict__ xyz,
                                                      const int *__restrict__ offset,
                                                      const int *__restrict__ new_offset, float *__restrict__ tmp,
                                                      int *__restrict__ idx) {
    __shared__ unsigned long long wkey[16];
    __shared__ float pick[3];
    const int cloud = blockIdx.x, tid = threadIdx.x;
    const int start = cloud > 0 ? offset[cloud - 1] : 0, end = offset[cloud];
    const int start_m = cloud > 0 ? new_offset[cloud - 1] : 0, end_m = new_offset[cloud];
    if (end_m <= start_m) return;                        // an empty output range writes nothing
    if (tid == 0) idx[start_m] = start;
    if (end <= start) {                                  // an empty cloud: the reference's besti never leaves start
        for (int j = start_m + 1 + tid; j < end_m; j += blockDim.x) idx[j] = start;
        return;
    }
    const int nw = blockDim.x / APN_WAVE;
    const unsigned brev = L > 0 ? __brev((unsigned)tid) >> (32 - L) : 0u;
    const bool mine = tid < T;

    // this thread's rows: start + tid + i T for i < rows
    const int rows = mine && start + tid < end ? (end - start - tid + T - 1) / T : 0;
    const size_t first = (size_t)start + (rows ? tid : 0);
    const float *__restrict__ xr = xyz + first * 3;
    float *__restrict__ tr = tmp + first;
    constexpr int NR = PER > 0 ? PER : 1;
    float x[NR], y[NR], z[NR], dm[NR];
    if (PER > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const bool have = i < rows;                  // (loads without a branch: a missing row reads the first one)
            const size_t o = have ? (size_t)i * T : 0;
            const float vx = xr[o * 3], vy = xr[o * 3 + 1], vz = xr[o * 3 + 2], vd = tr[o];
            x[i] = have ? vx : 0.0f;
            y[i] = have ? vy : 0.0f;
            z[i] = have ? vz : 0.0f;
            dm[i] = have ? vd : -2.0f;                   // below the initial best of -1: never a maximum
        }
    }
    float cx = xyz[(size_t)start * 3], cy = xyz[(size_t)start * 3 + 1], cz = xyz[(size_t)start * 3 + 2];

    for (int j = start_m + 1; j < end_m; ++j) {
        float best = -1.0f;
        int bi = 0;
        if (PER > 0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const float d = fminf(po_d2(x[i] - cx, y[i] - cy, z[i] - cz), dm[i]);
                dm[i] = d;
                const bool g = d > best;                 // strict: a thread keeps its first maximum
                best = g ? d : best;
                bi = g ? i : bi;
            }
        } else if (mine) {
            int i = 0;
            for (long long k = (long long)start + tid; k < end; k += T, ++i) {
                const float d = fminf(po_d2(xyz[k * 3] - cx, xyz[k * 3 + 1] - cy, xyz[k * 3 + 2] - cz), tmp[k]);
                tmp[k] = d;
                const bool g = d > best;
                best = g ? d : best;
                bi = g ? i : bi;
            }
        }
        unsigned du = 0u, low = 0u;
        if (best >= 0.0f) {                              // (a thread with rows: squared distances are >= 0)
            du = __float_as_uint(best) | 0x80000000u;
            low = ~((brev << 14) | (unsigned)bi);
        }
        const unsigned wmax = wave_max_u32(du);
        const unsigned wlow = wave_max_u32(du == wmax ? low : 0u);
        if ((tid & (APN_WAVE - 1)) == 0) wkey[tid / APN_WAVE] = ((unsigned long long)wmax << 32) | wlow;
        __syncthreads();
        unsigned long long win = 0ull;
        for (int w = 0; w < nw; ++w) win = wkey[w] > win ? wkey[w] : win;
        const unsigned wl = win ? ~(unsigned)win : 0u;    // (no thread had a row with d >= 0: the cloud's first row)
        const unsigned wb = wl >> 14;
        const int wi = (int)(wl & 0x3fffu);
        const int wt = L > 0 ? (int)(__brev(wb) >> (32 - L)) : 0;
        const long long k = (long long)start + wt + (long long)wi * T;
        if (tid == wt) {
            float px = 0.0f, py = 0.0f, pz = 0.0f;
            if (PER > 0) {
#pragma unroll
                for (int i = 0; i < NR; ++i)
                    if (i == wi) { px = x[i]; py = y[i]; pz = z[i]; }
            } else {
                px = xyz[k * 3]; py = xyz[k * 3 + 1]; pz = xyz[k * 3 + 2];
            }
            pick[0] = px; pick[1] = py; pick[2] = pz;
            idx[j] = (int)k;
        }
        __syncthreads();
        cx = pick[0]; cy = pick[1]; cz = pick[2];
    }
    if (PER > 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i)
            if (i < rows) tr[(size_t)i * T] = dm[i];
    }
}

// --------------------------------------------------------------------------------------------- forward kernels
// the grid-stride loops stay scalar: interleaved by two, their arithmetic becomes packed FP32 (build.py: NO_SLP's note)
#define APN_PO_SCALAR_LOOP _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")

enum { PO_GROUP = 0, PO_INTERP = 1, PO_SUB = 2, PO_AGG = 3 };

// grouping: out[pos, ch] = input[idx[pos], ch];  subtraction: out[pos, ch] = in1[pos / k, ch] - in2[idx[pos], ch]
template <int MODE>
__global__ __launch_bounds__(256) void po_gather_kernel(long long total, int n, int k, int c, const float *__restrict__ in1,
                                                        const float *__restrict__ in2, const int *__restrict__ idx,
                                                        float *__restrict__ out) {
    APN_PO_SCALAR_LOOP
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long pos = e / c;
        const int ch = (int)(e - pos * c);
        const float v = in2[(long long)po_clamp(idx[pos], n) * c + ch];
        out[e] = MODE == PO_SUB ? in1[(pos / k) * c + ch] - v : v;
    }
}

// one thread per (i, ch): the sum over the slots ascending, starting from the first term
//   interpolation: input[idx[i,s], ch] * weight[i,s]
//   aggregation:   (input[idx[i,s], ch] + position[i,s,ch]) * weight[i,s, ch % w_c]
//   subtraction's grad1 (MODE PO_SUB): grad_out[i,s,ch]
template <int MODE>
__global__ __launch_bounds__(256) void po_slot_sum_kernel(long long total, int n, int k, int c, int w_c,
                                                          const float *__restrict__ input,
                                                          const float *__restrict__ position,
                                                          const float *__restrict__ weight,
                                                          const int *__restrict__ idx, float *__restrict__ out) {
    APN_PO_SCALAR_LOOP
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long i = e / c;
        const int ch = (int)(e - i * c);
        float acc = 0.0f;
        for (int s = 0; s < k; ++s) {
            const long long pos = i * k + s;
            float term;
            if (MODE == PO_SUB) {
                term = input[pos * c + ch];
            } else {
                const float v = input[(long long)po_clamp(idx[pos], n) * c + ch];
                term = MODE == PO_INTERP ? v * weight[pos] : (v + position[pos * c + ch]) * weight[pos * w_c + ch % w_c];
            }
            acc = s == 0 ? term : acc + term;
        }
        out[e] = acc;
    }
}

// aggregation: grad_position[i,s,ch] = g[i,ch] * weight[i,s, ch % w_c]
__global__ __launch_bounds__(256) void po_agg_gpos_kernel(long long total, int k, int c, int w_c,
                                                          const float *__restrict__ g, const float *__restrict__ weight,
                                                          float *__restrict__ gpos) {
    APN_PO_SCALAR_LOOP
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long pos = e / c;
        const int ch = (int)(e - pos * c);
        gpos[e] = g[(pos / k) * c + ch] * weight[pos * w_c + ch % w_c];
    }
}

// aggregation: grad_weight[i,s,w] = sum over ch = w, w + w_c, ... ascending of g[i,ch] * (input[idx[i,s],ch] + position[i,s,ch])
__global__ __launch_bounds__(256) void po_agg_gw_kernel(long long total, int n, int k, int c, int w_c,
                                                        const float *__restrict__ input,
                                                        const float *__restrict__ position, const int *__restrict__ idx,
                                                        const float *__restrict__ g, float *__restrict__ gw) {
    APN_PO_SCALAR_LOOP
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long pos = e / w_c;
        const int w = (int)(e - pos * w_c);
        const float *__restrict__ in = input + (long long)po_clamp(idx[pos], n) * c;
        const float *__restrict__ pp = position + pos * c;
        const float *__restrict__ gg = g + (pos / k) * c;
        float acc = 0.0f;
        for (int ch = w; ch < c; ch += w_c) {
            const float term = gg[ch] * (in[ch] + pp[ch]);
            acc = ch == w ? term : acc + term;
        }
        gw[e] = acc;
    }
}

// ------------------------------------------------------------------------------- backward: walk the reverse list
// one thread per (j, ch): the sum over row j's list (positions pos = i k + s, ascending) in list order, from the first term
//   grouping:      g[pos, ch]                          subtraction (grad2):  -g[pos, ch]
//   interpolation: g[i, ch] * weight[pos]              aggregation:          g[i, ch] * weight[pos, ch % w_c]
template <int MODE>
__global__ __launch_bounds__(256) void po_list_sum_kernel(long long total, int k, int c, int w_c,
                                                          const float *__restrict__ g, const float *__restrict__ weight,
                                                          const int *__restrict__ pcnt, const int *__restrict__ poff,
                                                          const int *__restrict__ plist, float *__restrict__ out) {
    APN_PO_SCALAR_LOOP
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long j = e / c;
        const int ch = (int)(e - j * c);
        const int cnt = pcnt[j];
        const int *__restrict__ list = plist + poff[j];
        float acc = 0.0f;
        for (int t = 0; t < cnt; ++t) {
            const long long pos = list[t];
            float term;
            if (MODE == PO_GROUP) term = g[pos * c + ch];
            else if (MODE == PO_SUB) term = -g[pos * c + ch];
            else if (MODE == PO_INTERP) term = g[(pos / k) * c + ch] * weight[pos];
            else term = g[(pos / k) * c + ch] * weight[pos * w_c + ch % w_c];
            acc = t == 0 ? term : acc + term;
        }
        out[e] = acc;
    }
}

}  // namespace apn

using namespace apn;

static inline unsigned po_blocks(long long total) {
    const long long nb = (total + 255) / 256;
    return (unsigned)(nb < (1ll << 20) ? nb : (1ll << 20));          // the kernels stride over what is left
}

static inline bool po_rows(int n, int m) { return n >= 0 && m >= 0 && n < PO_ROWS_MAX && m < PO_ROWS_MAX; }

// sizes of the feature entries: (n, c) rows gathered by an (m, k) index, positions i k + s kept in an int
static inline bool po_feat(int n, int m, int k, int c) {
    return po_rows(n, m) && k >= 1 && c >= 1 && c <= 65536 && (long long)m * k < (1ll << 31);
}

extern "C" int apn_po_knn_query(int b, int n, int m, int k, const float *xyz, const float *new_xyz, const int *offset,
                                const int *new_offset, int *idx, float *dist2, void *stream) {
    if (b < 1 || !po_rows(n, m) || k < 1 || k > PO_K_MAX) return APN_EINVAL;
    if (n == 0 || m == 0) return APN_OK;
    if (!xyz || !new_xyz || !offset || !new_offset || !idx || !dist2) return APN_EINVAL;
    const dim3 grid((m + PO_TILE - 1) / PO_TILE), block(PO_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (k <= APN_WAVE)
        hipLaunchKernelGGL(po_knn_kernel<1>, grid, block, 0, st, b, n, m, k, xyz, new_xyz, offset, new_offset, idx, dist2);
    else
        hipLaunchKernelGGL(po_knn_kernel<2>, grid, block, 0, st, b, n, m, k, xyz, new_xyz, offset, new_offset, idx, dist2);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_ball_query(int b, int n, int m, float radius, int nsample, const float *xyz, const float *new_xyz,
                                 const int *offset, const int *new_offset, int *idx, void *stream) {
    if (b < 1 || !po_rows(n, m) || nsample < 1 || !(radius >= 0.0f)) return APN_EINVAL;
    if (n == 0 || m == 0) return APN_OK;
    if (!xyz || !new_xyz || !offset || !new_offset || !idx) return APN_EINVAL;
    hipLaunchKernelGGL(po_ball_kernel, dim3((m + PO_WAVES - 1) / PO_WAVES), dim3(PO_THREADS), 0, (hipStream_t)stream, b, n,
                       m, radius * radius, nsample, xyz, new_xyz, offset, new_offset, idx);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_furthest_sampling(int b, int n_max, const float *xyz, const int *offset, const int *new_offset,
                                        float *tmp, int *idx, void *stream) {
    if (b < 0 || n_max < 0 || n_max >= PO_ROWS_MAX) return APN_EINVAL;
    if (b == 0 || n_max == 0) return APN_OK;
    if (!xyz || !offset || !new_offset || !tmp || !idx) return APN_EINVAL;
    int L = 0;
    while (L < 10 && (2 << L) <= n_max) ++L;             // T = min(1024, 2^floor(log2 n_max))
    const int T = 1 << L;
    const int per = (n_max + T - 1) / T;
    const dim3 grid(b), block(T < APN_WAVE ? APN_WAVE : T);
    hipStream_t st = (hipStream_t)stream;
#define APN_PO_FPS(PER) hipLaunchKernelGGL(po_fps_kernel<PER>, grid, block, 0, st, T, L, xyz, offset, new_offset, tmp, idx)
    if (per <= 1) APN_PO_FPS(1);
    else if (per <= 2) APN_PO_FPS(2);
    else if (per <= 4) APN_PO_FPS(4);
    else if (per <= 8) APN_PO_FPS(8);
    else if (per <= 16) APN_PO_FPS(16);
    else if (per <= PO_FPS_PER_MAX) APN_PO_FPS(PO_FPS_PER_MAX);
    else APN_PO_FPS(0);
#undef APN_PO_FPS
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_grouping_fwd(int n, int m, int k, int c, const float *input, const int *idx, float *out,
                                   void *stream) {
    if (!po_feat(n, m, k, c)) return APN_EINVAL;
    if (n == 0 || m == 0) return APN_OK;
    if (!input || !idx || !out) return APN_EINVAL;
    const long long total = (long long)m * k * c;
    hipLaunchKernelGGL(po_gather_kernel<PO_GROUP>, dim3(po_blocks(total)), dim3(256), 0, (hipStream_t)stream, total, n, k, c,
                       (const float *)nullptr, input, idx, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_grouping_bwd(int n, int m, int k, int c, const float *grad_out, const int *pcnt_poff,
                                   const int *plist, float *grad_input, void *stream) {
    if (!po_feat(n, m, k, c)) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!grad_out || !pcnt_poff || !plist || !grad_input) return APN_EINVAL;
    const long long total = (long long)n * c;
    hipLaunchKernelGGL(po_list_sum_kernel<PO_GROUP>, dim3(po_blocks(total)), dim3(256), 0, (hipStream_t)stream, total, k, c,
                       1, grad_out, (const float *)nullptr, pcnt_poff, pcnt_poff + n, plist, grad_input);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_interpolation_fwd(int n, int m, int k, int c, const float *input, const int *idx,
                                        const float *weight, float *out, void *stream) {
    if (!po_feat(n, m, k, c)) return APN_EINVAL;
    if (n == 0 || m == 0) return APN_OK;
    if (!input || !idx || !weight || !out) return APN_EINVAL;
    const long long total = (long long)m * c;
    hipLaunchKernelGGL(po_slot_sum_kernel<PO_INTERP>, dim3(po_blocks(total)), dim3(256), 0, (hipStream_t)stream, total, n, k,
                       c, 1, input, (const float *)nullptr, weight, idx, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_interpolation_bwd(int n, int m, int k, int c, const float *grad_out, const float *weight,
                                        const int *pcnt_poff, const int *plist, float *grad_input, void *stream) {
    if (!po_feat(n, m, k, c)) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!grad_out || !weight || !pcnt_poff || !plist || !grad_input) return APN_EINVAL;
    const long long total = (long long)n * c;
    hipLaunchKernelGGL(po_list_sum_kernel<PO_INTERP>, dim3(po_blocks(total)), dim3(256), 0, (hipStream_t)stream, total, k, c,
                       1, grad_out, weight, pcnt_poff, pcnt_poff + n, plist, grad_input);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_subtraction_fwd(int n, int m, int k, int c, const float *input1, const float *input2,
                                      const int *idx, float *out, void *stream) {
    if (!po_feat(n, m, k, c)) return APN_EINVAL;
    if (n == 0 || m == 0) return APN_OK;
    if (!input1 || !input2 || !idx || !out) return APN_EINVAL;
    const long long total = (long long)m * k * c;
    hipLaunchKernelGGL(po_gather_kernel<PO_SUB>, dim3(po_blocks(total)), dim3(256), 0, (hipStream_t)stream, total, n, k, c,
                       input1, input2, idx, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_subtraction_bwd(int n, int m, int k, int c, const float *grad_out, const int *pcnt_poff,
                                      const int *plist, float *grad_input1, float *grad_input2, void *stream) {
    if (!po_feat(n, m, k, c)) return APN_EINVAL;
    if (n == 0 && m == 0) return APN_OK;
    if (!grad_out || !pcnt_poff || !plist || !grad_input1 || !grad_input2) return APN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (m > 0) {
        const long long total = (long long)m * c;
        hipLaunchKernelGGL(po_slot_sum_kernel<PO_SUB>, dim3(po_blocks(total)), dim3(256), 0, st, total, n, k, c, 1, grad_out,
                           (const float *)nullptr, (const float *)nullptr, (const int *)nullptr, grad_input1);
    }
    if (n > 0) {
        const long long total = (long long)n * c;
        hipLaunchKernelGGL(po_list_sum_kernel<PO_SUB>, dim3(po_blocks(total)), dim3(256), 0, st, total, k, c, 1, grad_out,
                           (const float *)nullptr, pcnt_poff, pcnt_poff + n, plist, grad_input2);
    }
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_aggregation_fwd(int n, int m, int k, int c, int w_c, const float *input, const float *position,
                                      const float *weight, const int *idx, float *out, void *stream) {
    if (!po_feat(n, m, k, c) || w_c < 1 || c % w_c) return APN_EINVAL;
    if (n == 0 || m == 0) return APN_OK;
    if (!input || !position || !weight || !idx || !out) return APN_EINVAL;
    const long long total = (long long)m * c;
    hipLaunchKernelGGL(po_slot_sum_kernel<PO_AGG>, dim3(po_blocks(total)), dim3(256), 0, (hipStream_t)stream, total, n, k, c,
                       w_c, input, position, weight, idx, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_po_aggregation_bwd(int n, int m, int k, int c, int w_c, const float *input, const float *position,
                                      const float *weight, const int *idx, const float *grad_out, const int *pcnt_poff,
                                      const int *plist, float *grad_input, float *grad_position, float *grad_weight,
                                      void *stream) {
    if (!po_feat(n, m, k, c) || w_c < 1 || c % w_c) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!input || !position || !weight || !idx || !grad_out || !pcnt_poff || !plist || !grad_input || !grad_position ||
        !grad_weight)
        return APN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)n * c;
    hipLaunchKernelGGL(po_list_sum_kernel<PO_AGG>, dim3(po_blocks(rows)), dim3(256), 0, st, rows, k, c, w_c, grad_out, weight,
                       pcnt_poff, pcnt_poff + n, plist, grad_input);
    if (m > 0) {
        const long long tp = (long long)m * k * c, tw = (long long)m * k * w_c;
        hipLaunchKernelGGL(po_agg_gpos_kernel, dim3(po_blocks(tp)), dim3(256), 0, st, tp, k, c, w_c, grad_out, weight,
                           grad_position);
        hipLaunchKernelGGL(po_agg_gw_kernel, dim3(po_blocks(tw)), dim3(256), 0, st, tw, n, k, c, w_c, input, position, idx,
                           grad_out, grad_weight);
    }
    APN_LAUNCH_CHECK();
    return APN_OK;
}
