// part_metrics.hip -- the part-segmentation metric of an evaluation batch on the device: per-point argmax over the part
// logits, intersection and union per part of each shape's category, the shape's mean IoU, and the running instance /
// category totals (examples/shapenetpart/train_adapt.py: get_ins_mious :77-107 behind `logits.max(dim=1)[1]`, and the
// accumulation of validate :576-582).  The reference walks (shape, part) in Python with three host reads per pair; here
// a batch is two launches and no host read.
//
// part_ious_kernel, one workgroup per shape.  A thread takes the argmax over the c channels for its points in
// ascending channel order under torch's order on (value, index) pairs (argmax_better, apn_common.h: a NaN beats every
// number and the first NaN wins, then the larger value, then the lower channel -- what `logits.max(dim=1)[1]` returns;
// an all -inf column gives channel 0), then counts by LDS integer atomics, per CHANNEL and not per part,
//     P[pred] += 1,   T[target] += 1 (target in [0, c)),   I[pred] += 1 (pred == target)
// -- integer adds commute, so the counts are exact and the same on every run.  A part p of the category then has
// intersection I[p] and union P[p] + T[p] - I[p]; a predicted (or target) label outside the category's part list is in
// no part's counts, as in the reference where it equals no `part` of the loop; a target outside [0, c) likewise.
// Thread 0 restates the reference's arithmetic: iou = float32(100 I) / float32(U) (correctly rounded), 100 where U == 0,
// added in the category's list order, divided by the number of parts.
// The category's parts come from a CSR table (part_offset [s + 1], part_ids [nparts]): nothing is assumed contiguous.
// A shape is REJECTED -- ious = -2, counted in *rejected, in no total -- when its class lies outside [0, s), its CSR
// range is empty, longer than 64, not inside [0, nparts], or names a part outside [0, c): no LDS index is formed from
// an unchecked value.  A shape with valid[b] == 0 (the padding of a last batch) gets ious = -1 and is in no total.
//
// part_totals_kernel, one workgroup.  Thread k < s owns category k, thread s the instance totals: each walks the batch's
// shapes in ascending order and adds the counted IoUs to what the accumulator already holds -- so the totals are one
// left-to-right sum over all shapes ever fed, whatever the split into batches, bit for bit.  cls_sum is float32 as the
// reference's `cls_mious[c] += miou`; ins_sum is float64 (the reference's torch.sum over the list has no order to restate).
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../../include/adaptpoint_amd.h"
#include "apn_common.h"

namespace apn {

constexpr int PM_THREADS = 256;
constexpr int PM_MAXC = 64;

__global__ __launch_bounds__(PM_THREADS) void part_ious_kernel(int c, int n, int s, int nparts,
                                                               const float *__restrict__ logits,
                                                               const int *__restrict__ target,
                                                               const int *__restrict__ cls,
                                                               const int *__restrict__ part_offset,
                                                               const int *__restrict__ part_ids,
                                                               const int *__restrict__ valid, float *__restrict__ ious) {
    __shared__ int cnt_i[PM_MAXC], cnt_p[PM_MAXC], cnt_t[PM_MAXC];
    const int b = blockIdx.x, t = threadIdx.x;
    if (valid && valid[b] == 0) {                      // workgroup-uniform
        if (t == 0) ious[b] = -1.0f;
        return;
    }
    const int k = cls[b];
    int lo = 0, hi = 0;
    bool ok = k >= 0 && k < s;
    if (ok) {
        lo = part_offset[k];
        hi = part_offset[k + 1];
        ok = lo >= 0 && hi > lo && hi - lo <= PM_MAXC && hi <= nparts;
    }
    if (!ok) {                                         // workgroup-uniform
        if (t == 0) ious[b] = -2.0f;
        return;
    }
    if (t < PM_MAXC) cnt_i[t] = cnt_p[t] = cnt_t[t] = 0;
    __syncthreads();
    const float *lg = logits + (size_t)b * c * n;
    const int *tg = target + (size_t)b * n;
    for (int i = t; i < n; i += PM_THREADS) {
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
        const int y = tg[i];
        atomicAdd(&cnt_p[bi], 1);
        if (y >= 0 && y < c) atomicAdd(&cnt_t[y], 1);
        if (y == bi) atomicAdd(&cnt_i[bi], 1);
    }
    __syncthreads();
    if (t != 0) return;
    float sum = 0.0f;
    for (int j = lo; j < hi; ++j) {
        const int p = part_ids[j];
        if (p < 0 || p >= c) {
            ious[b] = -2.0f;
            return;
        }
        const int in = cnt_i[p], un = cnt_p[p] + cnt_t[p] - in;
        const float iou = un == 0 ? 100.0f : __fdiv_rn((float)(100ll * in), (float)un);
        sum = sum + iou;
    }
    ious[b] = __fdiv_rn(sum, (float)(hi - lo));
}

__global__ __launch_bounds__(PM_THREADS) void part_totals_kernel(int b, int s, const float *__restrict__ ious,
                                                                 const int *__restrict__ cls, float *__restrict__ cls_sum,
                                                                 int *__restrict__ cls_num, double *__restrict__ ins_sum,
                                                                 int *__restrict__ ins_num, int *__restrict__ rejected) {
    for (int k = threadIdx.x; k <= s; k += PM_THREADS) {
        if (k < s) {
            float sum = cls_sum[k];
            int num = cls_num[k];
            for (int sh = 0; sh < b; ++sh) {
                const float v = ious[sh];
                if (v >= 0.0f && cls[sh] == k) {
                    sum = sum + v;
                    ++num;
                }
            }
            cls_sum[k] = sum;
            cls_num[k] = num;
        } else {
            double sum = ins_sum[0];
            int num = ins_num[0], bad = 0;
            for (int sh = 0; sh < b; ++sh) {
                const float v = ious[sh];
                if (v >= 0.0f) {
                    sum = sum + (double)v;
                    ++num;
                } else if (v < -1.5f) {
                    ++bad;
                }
            }
            ins_sum[0] = sum;
            ins_num[0] = num;
            if (rejected) rejected[0] += bad;
        }
    }
}

}  // namespace apn

extern "C" int apn_part_ious(int b, int c, int n, int s, int nparts, const float *logits, const int *target, const int *cls,
                             const int *part_offset, const int *part_ids, const int *valid, float *ious, float *cls_sum,
                             int *cls_num, double *ins_sum, int *ins_num, int *rejected, void *stream) {
    using namespace apn;
    if (b < 0 || c < 1 || c > PM_MAXC || n < 0 || s < 1 || nparts < 1) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!cls || !part_offset || !part_ids || !ious || !cls_sum || !cls_num || !ins_sum || !ins_num) return APN_EINVAL;
    if (n > 0 && (!logits || !target)) return APN_EINVAL;
    hipLaunchKernelGGL(part_ious_kernel, dim3(b), dim3(PM_THREADS), 0, (hipStream_t)stream, c, n, s, nparts, logits, target,
                       cls, part_offset, part_ids, valid, ious);
    APN_LAUNCH_CHECK();
    hipLaunchKernelGGL(part_totals_kernel, dim3(1), dim3(PM_THREADS), 0, (hipStream_t)stream, b, s, ious, cls, cls_sum,
                       cls_num, ins_sum, ins_num, rejected);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
