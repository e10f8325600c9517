// scene_seg.hip -- the per-point work of scene segmentation outside the network (examples/segmentation/main.py of the
// reference: train_one_epoch :334-385, validate :389-430, test :507-668; openpoints/dataset/data_util.py: crop_pc :146-174).
//
// Shared rules.  Every index read from a caller's tensor is range-checked before it addresses anything.  No float
// atomics; integer atomics only where their order cannot change the result (counters, LDS histograms, the stamp
// exchange below).  No workgroup waits for another.  Two runs give the same bits.  No host read: every entry is legal
// inside a captured graph.
//
// The confusion counters are c*c + 1 unsigned 64-bit cells, cell target * c + pred, the last one counting points whose
// target lies outside [0, c) and is not the ignored label (evaluate.ConfusionMatrix's layout).  A workgroup counts into
// a c*c + 1 integer histogram in LDS (c <= 64: 16 KiB) and flushes its non-zero cells with 64-bit integer atomics.  The
// argmax is argmax_better (apn_common.h): torch's rule, the first maximum wins and a NaN wins.
//
// ss_confusion_kernel     logits (b,c,n) channel-major: a thread owns points, so the c reads of a wave are 64 consecutive
//                         floats each.  Clouds at or beyond clamp(*valid, 0, b) get their pred and no count.
// ss_votes_add_kernel     acc[idx[j], :] += logits[:, j], cnt[idx[j]] += 1 with plain loads and stores.  That is only
//                         correct when a call's rows are distinct, so the kernel proves it: atomicExch(stamp[row], call)
//                         returns the previous stamp, and a thread that gets its own call number back bumps
//                         flags[0] (duplicates) and leaves the row alone -- exactly one thread per (call, row) owns
//                         the row, and each of its channels is added by one thread (the logits pass through an LDS tile).
//                         Rows outside [0, n) bump flags[1] (rejected).  A point's sum is therefore the sequence of fp32
//                         adds in call order, starting from +0.
// ss_votes_finish_kernel  mean = acc / max(cnt, 1), one correctly rounded division (torch_scatter's clamp_(1) and
//                         true_divide_), the argmax over the means, the counters against labels.
// ss_project_*            nearest-neighbour mode: argmax per voxel of column slot[v] of the per-voxel logits (c,m), then
//                         pred[i] = pred_voxel[voxel_of[i]] and the counters.  A slot or voxel outside [0, m) bumps
//                         flags[1]; its points get pred -1 and are not counted.
// ss_crop_kernel          the voxel_max nearest rows of a centre, one workgroup per cloud.  d = (dx*dx + dy*dy) + dz*dz in
//                         float32 with explicit roundings (numpy's result for np.sum(np.square(.), 1) over a length-3
//                         axis).  The bit pattern of a non-negative float orders as an unsigned integer: a 4-pass 8-bit
//                         radix select (per-wave LDS histograms) finds the k-th smallest key, rows with a smaller key are
//                         in, rows with the key itself are in by ascending row until k is reached -- the set
//                         np.argsort(d, kind='stable')[:k].  The survivors are written in ascending row by a ballot and
//                         scan compaction.  stats[0] counts rows with a non-finite coordinate; stats[1] counts clouds
//                         that were refused (bad offsets, a centre outside the cloud, fewer than k rows): nothing is
//                         written for those.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../../include/adaptpoint_amd.h"
#include "apn_common.h"

namespace apn {

constexpr int SS_THREADS = 256;
constexpr int SS_MAXC = 64;
constexpr int SS_MAX_BLOCKS_X = 64;        // confusion: tiles of a cloud are shared among at most this many workgroups
constexpr int SS_MAX_POINTS = INT_MAX - 1024 * SS_THREADS;   // grid-stride loops: i + stride stays an int
constexpr int SS_ADD_CH = 16;              // votes_add: channels per LDS tile
constexpr int SS_CROP_THREADS = 1024;
constexpr int SS_CROP_WAVES = SS_CROP_THREADS / APN_WAVE;

__device__ __forceinline__ void hist_clear(int *hist, int c) {
    for (int i = threadIdx.x; i <= c * c; i += blockDim.x) hist[i] = 0;
    __syncthreads();
}

// one point: target y, prediction p in [0, c)
__device__ __forceinline__ void hist_count(int *hist, int c, int y, int p, int ignore_index, int has_ignore) {
    if (has_ignore && y == ignore_index) return;
    atomicAdd(&hist[(y >= 0 && y < c) ? y * c + p : c * c], 1);
}

__device__ __forceinline__ void hist_flush(const int *hist, int c, unsigned long long *cm) {
    __syncthreads();
    for (int i = threadIdx.x; i <= c * c; i += blockDim.x) {
        const int v = hist[i];
        if (v) atomicAdd(cm + i, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(SS_THREADS) void ss_confusion_kernel(int b, int c, int n, const float *__restrict__ logits,
                                                                  const int *__restrict__ target, int ignore_index,
                                                                  int has_ignore, const int *__restrict__ valid,
                                                                  unsigned long long *__restrict__ cm,
                                                                  int *__restrict__ pred) {
    __shared__ int hist[SS_MAXC * SS_MAXC + 1];
    const int cloud = blockIdx.y;
    int nvalid = b;
    if (valid) nvalid = min(max(*valid, 0), b);
    const bool counted = cloud < nvalid;               // workgroup-uniform
    if (!counted && !pred) return;
    hist_clear(hist, c);
    const float *lg = logits + (size_t)cloud * c * n;
    const int *tg = target + (size_t)cloud * n;
    for (int i = blockIdx.x * SS_THREADS + threadIdx.x; i < n; i += gridDim.x * SS_THREADS) {
        float best = -__builtin_inff();
        int bi = INT_MAX;
        for (int ch = 0; ch < c; ++ch) {
            const float v = lg[(size_t)ch * n + i];
            if (argmax_better(v, ch, best, bi)) {
                best = v;
                bi = ch;
            }
        }
        // channel 0 beats the start pair (-inf, INT_MAX) whatever it holds, so bi lies in [0, c)
        if (pred) pred[(size_t)cloud * n + i] = bi;
        if (counted) hist_count(hist, c, tg[i], bi, ignore_index, has_ignore);
    }
    if (counted) hist_flush(hist, c, cm);
}

__global__ __launch_bounds__(SS_THREADS) void ss_votes_add_kernel(int n, int c, int n_part,
                                                                  const float *__restrict__ logits,
                                                                  const int *__restrict__ idx, int call,
                                                                  float *__restrict__ acc, int *__restrict__ cnt,
                                                                  int *__restrict__ stamp, int *__restrict__ flags) {
    // A workgroup owns SS_THREADS consecutive columns.  Thread t settles column j's row (range check, stamp exchange);
    // the logits go through an LDS tile of SS_ADD_CH channels so that they are read along n_part and added along a
    // row's channels: consecutive lanes touch consecutive addresses on both sides.
    __shared__ float tile[SS_ADD_CH][SS_THREADS + 1];
    __shared__ int rows[SS_THREADS];
    const int t = threadIdx.x;
    const long long j0 = (long long)blockIdx.x * SS_THREADS, j = j0 + t;
    int row = -1;
    if (j < n_part) {
        const int r = idx[j];
        if (r < 0 || r >= n) {
            atomicAdd(&flags[1], 1);
        } else if (atomicExch(&stamp[r], call) == call) {      // another thread of this call owns the row
            atomicAdd(&flags[0], 1);
        } else {
            row = r;
            cnt[r] = cnt[r] + 1;
        }
    }
    rows[t] = row;
    const int np = (int)min((long long)SS_THREADS, n_part - j0);    // workgroup-uniform, >= 1
    for (int c0 = 0; c0 < c; c0 += SS_ADD_CH) {
        const int cc = min(SS_ADD_CH, c - c0);
        __syncthreads();                               // rows[] written; the previous tile has been consumed
        if (j < n_part)
            for (int ch = 0; ch < cc; ++ch) tile[ch][t] = logits[(size_t)(c0 + ch) * n_part + j];
        __syncthreads();
        for (int e = t; e < np * cc; e += SS_THREADS) {
            const int p = e / cc, ch = e - p * cc, r = rows[p];
            if (r >= 0) {
                float *dst = acc + (size_t)r * c + c0 + ch;
                *dst = __fadd_rn(*dst, tile[ch][p]);
            }
        }
    }
}

__global__ __launch_bounds__(SS_THREADS) void ss_votes_finish_kernel(int n, int c, const float *__restrict__ acc,
                                                                     const int *__restrict__ cnt,
                                                                     const int *__restrict__ labels, int ignore_index,
                                                                     int has_ignore, unsigned long long *__restrict__ cm,
                                                                     float *__restrict__ mean, int *__restrict__ pred) {
    __shared__ int hist[SS_MAXC * SS_MAXC + 1];
    if (labels) hist_clear(hist, c);
    for (int i = blockIdx.x * SS_THREADS + threadIdx.x; i < n; i += gridDim.x * SS_THREADS) {
        const float den = (float)max(cnt[i], 1);
        const float *src = acc + (size_t)i * c;
        float best = -__builtin_inff();
        int bi = INT_MAX;
        for (int ch = 0; ch < c; ++ch) {
            const float v = __fdiv_rn(src[ch], den);
            if (mean) mean[(size_t)i * c + ch] = v;
            if (argmax_better(v, ch, best, bi)) {
                best = v;
                bi = ch;
            }
        }
        if (pred) pred[i] = bi;
        if (labels) hist_count(hist, c, labels[i], bi, ignore_index, has_ignore);
    }
    if (labels) hist_flush(hist, c, cm);
}

__global__ __launch_bounds__(SS_THREADS) void ss_project_voxel_kernel(int c, int m, const float *__restrict__ logits,
                                                                      const int *__restrict__ slot,
                                                                      int *__restrict__ pred_voxel,
                                                                      int *__restrict__ flags) {
    const int v = blockIdx.x * SS_THREADS + threadIdx.x;
    if (v >= m) return;
    const int s = slot[v];
    if (s < 0 || s >= m) {
        atomicAdd(&flags[1], 1);
        pred_voxel[v] = -1;
        return;
    }
    float best = -__builtin_inff();
    int bi = INT_MAX;
    for (int ch = 0; ch < c; ++ch) {
        const float x = logits[(size_t)ch * m + s];
        if (argmax_better(x, ch, best, bi)) {
            best = x;
            bi = ch;
        }
    }
    pred_voxel[v] = bi;
}

__global__ __launch_bounds__(SS_THREADS) void ss_project_point_kernel(int c, int m, int n,
                                                                      const int *__restrict__ pred_voxel,
                                                                      const int *__restrict__ voxel_of,
                                                                      const int *__restrict__ labels, int ignore_index,
                                                                      int has_ignore, unsigned long long *__restrict__ cm,
                                                                      int *__restrict__ pred, int *__restrict__ flags) {
    __shared__ int hist[SS_MAXC * SS_MAXC + 1];
    if (labels) hist_clear(hist, c);
    for (int i = blockIdx.x * SS_THREADS + threadIdx.x; i < n; i += gridDim.x * SS_THREADS) {
        const int v = voxel_of[i];
        int p = -1;
        if (v < 0 || v >= m)
            atomicAdd(&flags[1], 1);
        else
            p = pred_voxel[v];                         // -1: the voxel's slot was rejected (counted there)
        if (pred) pred[i] = p;
        if (labels && p >= 0) hist_count(hist, c, labels[i], p, ignore_index, has_ignore);
    }
    if (labels) hist_flush(hist, c, cm);
}

// ------------------------------------------------------------------------------------------------------ the crop
__device__ __forceinline__ unsigned crop_key(const float *__restrict__ row, float cx, float cy, float cz) {
    const float dx = __fsub_rn(row[0], cx), dy = __fsub_rn(row[1], cy), dz = __fsub_rn(row[2], cz);
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return __float_as_uint(d);
}

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__global__ __launch_bounds__(SS_CROP_THREADS) void ss_crop_kernel(int n, int k, const float *__restrict__ coord,
                                                                  const int *__restrict__ offset,
                                                                  const int *__restrict__ centre, int *__restrict__ idx,
                                                                  int *__restrict__ stats) {
    __shared__ int hist[SS_CROP_WAVES][256];
    __shared__ int wave_sum[SS_CROP_WAVES][2];
    __shared__ unsigned sel_prefix;
    __shared__ int sel_remaining;
    const int cloud = blockIdx.x, t = threadIdx.x, wave = t / APN_WAVE, lane = t % APN_WAVE;
    const int lo = cloud == 0 ? 0 : offset[cloud - 1], hi = offset[cloud];
    const int ctr = centre[cloud];
    // workgroup-uniform: every value below was read by every thread
    if (lo < 0 || hi < lo || hi > n || hi - lo < k || ctr < 0 || ctr >= hi - lo) {
        if (t == 0) atomicAdd(&stats[1], 1);
        return;
    }
    const int rows = hi - lo;
    const float *base = coord + (size_t)lo * 3;
    const float cx = base[(size_t)ctr * 3], cy = base[(size_t)ctr * 3 + 1], cz = base[(size_t)ctr * 3 + 2];

    int bad = 0;
    for (int i = t; i < rows; i += SS_CROP_THREADS) {
        const float *r = base + (size_t)i * 3;
        bad += !(finite_bits(r[0]) && finite_bits(r[1]) && finite_bits(r[2]));
    }
    if (bad) atomicAdd(&stats[0], bad);

    // the k-th smallest key: most significant byte first; `prefix` holds the bytes decided so far
    unsigned prefix = 0;
    int remaining = k;
    for (int pass = 3; pass >= 0; --pass) {
        const int shift = pass * 8;
        for (int i = t; i < SS_CROP_WAVES * 256; i += SS_CROP_THREADS) (&hist[0][0])[i] = 0;
        __syncthreads();
        for (int i = t; i < rows; i += SS_CROP_THREADS) {
            const unsigned key = crop_key(base + (size_t)i * 3, cx, cy, cz);
            if (pass == 3 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[wave][(key >> shift) & 255u], 1);
        }
        __syncthreads();
        // threads 0..255 (waves 0..3): bin t's total, then an inclusive scan over the 256 bins
        int total = 0, incl = 0;
        if (t < 256) {
            for (int w = 0; w < SS_CROP_WAVES; ++w) total += hist[w][t];
            incl = total;
            for (int d = 1; d < APN_WAVE; d <<= 1) {
                const int o = __shfl_up(incl, d, APN_WAVE);
                if (lane >= d) incl += o;
            }
            if (lane == APN_WAVE - 1) wave_sum[wave][0] = incl;
        }
        __syncthreads();
        if (t < 256) {
            for (int w = 0; w < wave; ++w) incl += wave_sum[w][0];
            const int excl = incl - total;
            if (excl < remaining && remaining <= incl) {               // exactly one bin: the counts sum to >= remaining
                sel_prefix = prefix | ((unsigned)t << shift);
                sel_remaining = remaining - excl;
            }
        }
        __syncthreads();
        prefix = sel_prefix;
        remaining = sel_remaining;
    }
    // rows with key < prefix: k - remaining of them; rows with key == prefix: the first `remaining` by ascending row
    int lt_base = 0, eq_base = 0;
    int *out = idx + (size_t)cloud * k;
    for (int start = 0; start < rows; start += SS_CROP_THREADS) {
        const int i = start + t;
        bool lt = false, eq = false;
        if (i < rows) {
            const unsigned key = crop_key(base + (size_t)i * 3, cx, cy, cz);
            lt = key < prefix;
            eq = key == prefix;
        }
        const unsigned long long lt_mask = __ballot(lt), eq_mask = __ballot(eq);
        __syncthreads();                                               // the previous chunk's wave_sum has been read
        if (lane == 0) {
            wave_sum[wave][0] = __popcll(lt_mask);
            wave_sum[wave][1] = __popcll(eq_mask);
        }
        __syncthreads();
        int lt_before = lt_base + lanes_below(lt_mask), eq_before = eq_base + lanes_below(eq_mask);
        int lt_all = 0, eq_all = 0;
        for (int w = 0; w < SS_CROP_WAVES; ++w) {
            const int a = wave_sum[w][0], b = wave_sum[w][1];
            if (w < wave) {
                lt_before += a;
                eq_before += b;
            }
            lt_all += a;
            eq_all += b;
        }
        if (lt || (eq && eq_before < remaining)) {
            const int pos = lt_before + min(eq_before, remaining);
            if (pos < k) out[pos] = lo + i;
        }
        lt_base += lt_all;
        eq_base += eq_all;
    }
}

static inline int ss_blocks(long long work) {
    const long long blocks = (work + SS_THREADS - 1) / SS_THREADS;
    return (int)(blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks));
}

}  // namespace apn

extern "C" int apn_ss_max_classes(void) { return apn::SS_MAXC; }

extern "C" int apn_ss_confusion(int b, int c, int n, const float *logits, const int *target, int ignore_index,
                                int has_ignore, const int *valid, unsigned long long *cm, int *pred, void *stream) {
    using namespace apn;
    if (b < 0 || b > 65535 || c < 1 || c > SS_MAXC || n < 0 || n > SS_MAX_POINTS) return APN_EINVAL;
    if (b == 0 || n == 0) return APN_OK;
    if (!logits || !target || !cm) return APN_EINVAL;
    const int tiles = (int)(((long long)n + SS_THREADS - 1) / SS_THREADS);
    hipLaunchKernelGGL(ss_confusion_kernel, dim3(tiles < SS_MAX_BLOCKS_X ? tiles : SS_MAX_BLOCKS_X, b), dim3(SS_THREADS), 0,
                       (hipStream_t)stream, b, c, n, logits, target, ignore_index, has_ignore, valid, cm, pred);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ss_votes_add(int n, int c, int n_part, const float *logits, const int *idx, int call, float *acc,
                                int *cnt, int *stamp, int *flags, void *stream) {
    using namespace apn;
    if (n < 0 || c < 1 || n_part < 0 || call < 1) return APN_EINVAL;      // stamps start at 0: calls count from 1
    if (n_part == 0) return APN_OK;
    if (!logits || !idx || !acc || !cnt || !stamp || !flags) return APN_EINVAL;
    const int blocks = (int)(((long long)n_part + SS_THREADS - 1) / SS_THREADS);
    hipLaunchKernelGGL(ss_votes_add_kernel, dim3(blocks), dim3(SS_THREADS), 0, (hipStream_t)stream, n, c, n_part, logits,
                       idx, call, acc, cnt, stamp, flags);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ss_votes_finish(int n, int c, const float *acc, const int *cnt, const int *labels, int ignore_index,
                                   int has_ignore, unsigned long long *cm, float *mean, int *pred, void *stream) {
    using namespace apn;
    if (n < 0 || n > SS_MAX_POINTS || c < 1 || c > SS_MAXC) return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!acc || !cnt || (labels && !cm)) return APN_EINVAL;
    hipLaunchKernelGGL(ss_votes_finish_kernel, dim3(ss_blocks(n)), dim3(SS_THREADS), 0, (hipStream_t)stream, n, c, acc,
                       cnt, labels, ignore_index, has_ignore, cm, mean, pred);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_ss_project(int c, int m, int n, const float *logits, const int *slot, const int *voxel_of,
                              const int *labels, int ignore_index, int has_ignore, int *pred_voxel,
                              unsigned long long *cm, int *pred, int *flags, void *stream) {
    using namespace apn;
    if (c < 1 || c > SS_MAXC || m < 0 || n < 0 || n > SS_MAX_POINTS) return APN_EINVAL;
    if (m == 0 && n == 0) return APN_OK;
    if (!flags || (m > 0 && (!logits || !slot || !pred_voxel)) || (n > 0 && !voxel_of) || (labels && !cm)) return APN_EINVAL;
    if (m > 0) {
        const int blocks = (int)(((long long)m + SS_THREADS - 1) / SS_THREADS);
        hipLaunchKernelGGL(ss_project_voxel_kernel, dim3(blocks), dim3(SS_THREADS), 0, (hipStream_t)stream, c, m, logits,
                           slot, pred_voxel, flags);
        APN_LAUNCH_CHECK();
    }
    if (n > 0) {
        hipLaunchKernelGGL(ss_project_point_kernel, dim3(ss_blocks(n)), dim3(SS_THREADS), 0, (hipStream_t)stream, c, m, n,
                           pred_voxel, voxel_of, labels, ignore_index, has_ignore, cm, pred, flags);
        APN_LAUNCH_CHECK();
    }
    return APN_OK;
}

extern "C" int apn_ss_crop_nearest(int b, int n, int k, const float *coord, const int *offset, const int *centre,
                                   int *idx, int *stats, void *stream) {
    using namespace apn;
    if (b < 0 || n < 0 || k < 1 || k > n) return APN_EINVAL;              // (a cloud shorter than k is refused in the kernel)
    if ((long long)b * k > INT_MAX) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!coord || !offset || !centre || !idx || !stats) return APN_EINVAL;
    hipLaunchKernelGGL(ss_crop_kernel, dim3(b), dim3(SS_CROP_THREADS), 0, (hipStream_t)stream, n, k, coord, offset, centre,
                       idx, stats);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
