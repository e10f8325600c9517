// col_sums.hip -- the library's one single-level fold: out[col] = the column sums of part[rows][ncol], the partial rows
// that the workgroups of a reduction leave, added in the shared order of include/adaptpoint_amd.h ("Partial-row folds"):
//
//   a workgroup of 256 threads is 256 / LANES columns x LANES row lanes (column = the fast index: a wave reads whole
//   row segments).  Lane l adds the rows l, l + LANES, l + 2 LANES, ... in ascending order into ONE float64 accumulator
//   that starts at +0 (the loads of four rows are issued together, the adds stay sequential); the LANES sums of a column
//   go through LDS and are combined by an adjacent-pair tree: (0+1), (2+3), ..., then pairs of those, and so on.  A
//   float32 output is the float64 total rounded once, at the store.
//
// An order fixed by (rows, LANES) alone: no atomic, two runs give the same bits.  rows == 0 writes zeros.  Indexing is
// 64-bit.  tail_count >= 0: one thread also writes out[ncol] = tail_count and out[ncol + 1] = 1 (the {count, 1} tail
// apn_sa_bn_fold and the SyncBatchNorm exchange take: no fill launch); a negative value writes no tail.
//
// Callers: apn_la_stats_fold, the split-K folds of csrc/pointwise.hip and apn_ag_fold at 4 lanes, apn_rl_moments and
// apn_rl_finalize at 8, apn_pt_fold at 16 -- more lanes for more rows per column.
#include "apn_common.h"

namespace apn {

template <typename TIn, typename TOut, int LANES>
__global__ __launch_bounds__(256) void col_sums_kernel(const TIn *__restrict__ part, int rows, size_t ncol,
                                                       TOut *__restrict__ out, double tail_count) {
    constexpr int COLS = 256 / LANES;
    __shared__ double red[LANES][COLS];
    const int cl = threadIdx.x % COLS, lane = threadIdx.x / COLS;
    const size_t col = (size_t)blockIdx.x * COLS + cl;
    double s = 0.0;
    if (col < ncol) {
#pragma unroll 4
        for (int r = lane; r < rows; r += LANES) s += (double)part[(size_t)r * ncol + col];
    }
    red[lane][cl] = s;
    __syncthreads();
    if (lane == 0 && col < ncol) {
        double v[LANES];
#pragma unroll
        for (int l = 0; l < LANES; ++l) v[l] = red[l][cl];
#pragma unroll
        for (int w = 1; w < LANES; w *= 2) {
#pragma unroll
            for (int l = 0; l < LANES; l += 2 * w) v[l] += v[l + w];
        }
        out[col] = (TOut)v[0];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && tail_count >= 0.0) {
        out[ncol] = (TOut)tail_count;
        out[ncol + 1] = (TOut)1.0;
    }
}

template <typename TIn, typename TOut>
int col_sums(const TIn *part, int rows, size_t ncol, int lanes, TOut *out, double tail_count, hipStream_t s) {
    if (rows < 0 || !out || (rows > 0 && !part) || (lanes != 4 && lanes != 8 && lanes != 16)) return APN_EINVAL;
    if (ncol == 0) return APN_OK;
    const size_t blocks = (ncol + 256 / lanes - 1) / (256 / lanes);
    if (blocks > 0x7fffffffull) return APN_EINVAL;
#define APN_COL_SUMS(LANES)                                                                                          \
    hipLaunchKernelGGL((col_sums_kernel<TIn, TOut, LANES>), dim3((unsigned)blocks), dim3(256), 0, s, part, rows, ncol, \
                       out, tail_count)
    switch (lanes) {
        case 4: APN_COL_SUMS(4); break;
        case 8: APN_COL_SUMS(8); break;
        default: APN_COL_SUMS(16); break;
    }
#undef APN_COL_SUMS
    APN_LAUNCH_CHECK();
    return APN_OK;
}

template int col_sums<double, double>(const double *, int, size_t, int, double *, double, hipStream_t);
template int col_sums<float, double>(const float *, int, size_t, int, double *, double, hipStream_t);
template int col_sums<float, float>(const float *, int, size_t, int, float *, double, hipStream_t);

}  // namespace apn
