// cls_metrics.hip -- the classification metric of an evaluation batch on the device: argmax over the logits and a
// masked confusion-matrix update, one launch, no host read (openpoints/utils/metrics.py:62-73 behind
// `logits.argmax(dim=1)`, examples/classification/train_autoaug.py:540-541).
//
// One wave per row, lanes striding over the classes.  Each lane keeps the best (value, index) pair of its classes, and a
// butterfly of xor shuffles combines the lanes' pairs.  The order on pairs is torch.argmax's: a NaN beats every number
// (the lower index among NaNs), then the larger value, then the lower index.  It is a total order, so the butterfly's
// result does not depend on how the pairs meet.  A lane without a class holds (-inf, INT_MAX), which every real entry
// beats or ties with a lower index: an all -inf row gives 0.
// The counted rows (r < clamp(*valid, 0, b)) then add one to cell target * k + pred of the 64-bit counters by an
// integer atomic; a target outside [0, k) adds to cell k * k instead.  Integer adds commute, so the counts are exact and
// the same on every run.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../../include/adaptpoint_amd.h"
#include "apn_common.h"

namespace apn {

constexpr int CM_THREADS = 256;
constexpr int CM_ROWS = CM_THREADS / APN_WAVE;

__global__ __launch_bounds__(CM_THREADS) void cls_confusion_kernel(int b, int k, const float *__restrict__ logits,
                                                                   int ld, const int *__restrict__ target,
                                                                   const int *__restrict__ valid,
                                                                   unsigned long long *__restrict__ cm,
                                                                   int *__restrict__ pred) {
    const int lane = threadIdx.x % APN_WAVE;
    const int row = blockIdx.x * CM_ROWS + threadIdx.x / APN_WAVE;
    if (row >= b) return;                              // wave-uniform
    const float *src = logits + (size_t)row * ld;
    float best = -__builtin_inff();
    int bi = INT_MAX;
    for (int j = lane; j < k; j += APN_WAVE) {
        const float v = src[j];
        if (argmax_better(v, j, best, bi)) {
            best = v;
            bi = j;
        }
    }
#pragma unroll
    for (int m = APN_WAVE / 2; m > 0; m >>= 1) {
        const float ov = __shfl_xor(best, m, APN_WAVE);
        const int oi = __shfl_xor(bi, m, APN_WAVE);
        if (argmax_better(ov, oi, best, bi)) {
            best = ov;
            bi = oi;
        }
    }
    if (lane != 0) return;
    if (pred) pred[row] = bi;
    int nvalid = b;
    if (valid) nvalid = min(max(*valid, 0), b);
    if (row >= nvalid) return;
    const int t = target[row];
    const size_t cell = (t >= 0 && t < k) ? (size_t)t * k + bi : (size_t)k * k;
    atomicAdd(cm + cell, 1ull);
}

}  // namespace apn

extern "C" int apn_cls_confusion(int b, int k, const float *logits, int ld, const int *target, const int *valid,
                                 unsigned long long *cm, int *pred, void *stream) {
    using namespace apn;
    if (b < 0 || k < 1 || ld < k) return APN_EINVAL;
    if (b == 0) return APN_OK;
    if (!logits || !target || !cm) return APN_EINVAL;
    const int blocks = (int)(((long long)b + CM_ROWS - 1) / CM_ROWS);
    hipLaunchKernelGGL(cls_confusion_kernel, dim3(blocks), dim3(CM_THREADS), 0, (hipStream_t)stream, b, k, logits, ld,
                       target, valid, cm, pred);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
