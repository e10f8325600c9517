/*
 * adaptpoint_amd.h -- C ABI of libadaptpoint_amd.so (MI355X / gfx950).
 *
 * The drop-in boundary for the set-abstraction hot path of AdaptPoint /
 * OpenPoints.  Each entry point replaces one function that the reference binds
 * with pybind11 in openpoints/cpp/pointnet2_batch/src/pointnet2_api.cpp:10-24
 * (module `pointnet2_batch_cuda`), and takes what that function's C++ wrapper
 * hands to its kernel launcher: plain device pointers and sizes, plus the HIP
 * stream to launch on.  No torch types, no allocation, no global state.
 *
 * Contract shared by every entry point (reference: SURVEY.md section 8b):
 *   - all pointers are DEVICE pointers on the current HIP device, float32 /
 *     int32, dense row-major ("contiguous") in the layout given below;
 *   - outputs and scratch are allocated, and where stated pre-initialised, by
 *     the caller; kernels never allocate or free;
 *   - `stream` is a hipStream_t (NULL = the default stream); the call only
 *     enqueues work, it never synchronises the device;
 *   - return value: 0 on success; a positive value is the hipError_t of the
 *     failed launch; APN_EINVAL for an argument the kernels cannot handle.
 *     Nothing ever calls exit() (the reference launchers do, e.g.
 *     sampling_gpu.cu:46-50).
 *   - sizes of zero are no-ops that return 0.
 */
#ifndef ADAPTPOINT_AMD_H
#define ADAPTPOINT_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APN_OK 0
#define APN_EINVAL (-1)

#if defined(__GNUC__)
#define APN_API __attribute__((visibility("default")))
#else
#define APN_API
#endif

/* Library / ABI version: major*10000 + minor*100 + patch. */
APN_API int apn_version(void);

/* Text for a return code of any function below (static storage). */
APN_API const char *apn_error_string(int code);

/* The compiler flag line the library was built with (static storage).  No reference counterpart: the
 * reference's setup.py (openpoints/cpp/pointnet2_batch/setup.py) fixes its nvcc flags; here two flags are
 * part of correctness (-ffp-contract=off pins the float rounding of every distance, -fno-slp-vectorize
 * keeps compiler-made packed-FP32 out), and the loader checks for them. */
APN_API const char *apn_build_flags(void);

/* Partial-row folds.  A reduction that crosses workgroups leaves one partial row per workgroup, part[rows][ncol], and a
 * second launch adds the rows column by column (apn_la_stats_fold, apn_ag_fold, apn_pt_fold, the split-K shares of
 * apn_pw_contract / apn_pw_contract2 / apn_pw_conv_grad_weight, apn_rl_moments, apn_rl_finalize).  They all add in ONE
 * order (csrc/col_sums.hip), fixed by rows and a lane count L in {4, 8, 16} that each entry states:
 *   partial rows are added by L lanes per column: lane l adds the rows l, l + L, l + 2L, ... in ascending order into one
 *   float64 accumulator that starts at +0; the L sums are then combined by an adjacent-pair tree, (0+1), (2+3), ...,
 *   then pairs of those, and so on.  A float32 result is the float64 total rounded once.
 * No atomics: two runs give the same bits, and so does a replay from a captured graph.  rows == 0 gives zeros. */

/* Replaces furthest_point_sampling_wrapper (pointnet2_api.cpp:18,
 * sampling.cpp:39-48 -> sampling_gpu.cu:101-260).
 *   xyz  (B,N,3) in; temp (B,N) in/out, pre-filled by the caller (1e10,
 *   subsample.py:94), holds the final min squared distances on return;
 *   idxs (B,M) out.  idxs[:,0] = 0; ties follow the reference's block-tree
 *   order (smallest bit-reversed thread id, then lowest index). */
APN_API int apn_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp,
                                int *idxs, void *stream);

/* Replaces ball_query_wrapper (pointnet2_api.cpp:11, ball_query.cpp:29-39 ->
 * ball_query_gpu.cu:15-73).
 *   new_xyz (B,M,3) queries; xyz (B,N,3) support; idx (B,M,nsample) out,
 *   pre-zeroed by the caller (group.py:194): rows of empty balls are not
 *   written.  Strict d2 < radius*radius in float32. */
APN_API int apn_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                   const float *xyz, int *idx, void *stream);

/* Replaces group_points_wrapper (pointnet2_api.cpp:12, group_points.cpp:25-35 ->
 * group_points_gpu.cu:53-92).  points (B,C,N), idx (B,npoints,nsample) ->
 * out (B,C,npoints,nsample). */
APN_API int apn_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                     const int *idx, float *out, void *stream);

/* Replaces group_points_grad_wrapper (pointnet2_api.cpp:13, group_points.cpp:13-23
 * -> group_points_gpu.cu:14-50).  grad_out (B,C,npoints,nsample), idx ->
 * grad_points (B,C,N) += scatter; the caller zeroes grad_points (group.py:111). */
APN_API int apn_group_points_grad(int b, int c, int n, int npoints, int nsample,
                          const float *grad_out, const int *idx, float *grad_points,
                          void *stream);

/* Replaces gather_points_wrapper (pointnet2_api.cpp:15, sampling.cpp:16-24 ->
 * sampling_gpu.cu:15-51).  points (B,C,N), idx (B,npoints) -> out (B,C,npoints). */
APN_API int apn_gather_points(int b, int c, int n, int npoints, const float *points,
                      const int *idx, float *out, void *stream);

/* Replaces gather_points_grad_wrapper (pointnet2_api.cpp:16, sampling.cpp:27-36 ->
 * sampling_gpu.cu:53-90).  grad_points (B,C,N) += scatter of grad_out (B,C,npoints);
 * caller-zeroed (subsample.py:136). */
APN_API int apn_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out,
                           const int *idx, float *grad_points, void *stream);

/* The training loop's resampler (examples/classification/train_autoaug.py:493-498): points
 * (B,N,C) rows (3 <= C <= 8), fidx (B,p_all) FPS picks, choice (s_cnt) a subset of 0..p_all-1
 * shared by the batch -> pos (B,s_cnt,3) = points[b, fidx[b, choice[s]], :3] and
 * x (B,cx,s_cnt) = the first cx channels, channel-major (what `data['pos']`, `data['x']`
 * become at :500-501), one launch.  choice values must lie in [0, p_all). */
APN_API int apn_resample_points(int b, int n, int c, int p_all, int s_cnt, int cx,
                                const float *points, const int *fidx, const int *choice,
                                float *pos, float *x, void *stream);

/* Replaces three_nn_wrapper (pointnet2_api.cpp:20, interpolate.cpp:20-28 ->
 * interpolate_gpu.cu:16-81).  unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3)
 * SQUARED distances ascending, idx (B,n,3).  m < 3 leaves +inf / index 0 in
 * the unused slots, as the reference does. */
APN_API int apn_three_nn(int b, int n, int m, const float *unknown, const float *known,
                 float *dist2, int *idx, void *stream);

/* Replaces three_interpolate_wrapper (pointnet2_api.cpp:21, interpolate.cpp:31-43 ->
 * interpolate_gpu.cu:84-124).  points (B,C,M), idx/weight (B,N,3) -> out (B,C,N).
 * NOTE the reference's argument order: (b, c, m, n). */
APN_API int apn_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                          const float *weight, float *out, void *stream);

/* Replaces three_interpolate_grad_wrapper (pointnet2_api.cpp:22,
 * interpolate.cpp:45-57 -> interpolate_gpu.cu:127-168).  grad_out (B,C,N) ->
 * grad_points (B,C,M) += scatter; caller-zeroed (upsampling.py:82).
 * NOTE the reference's argument order: (b, c, n, m). */
APN_API int apn_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out,
                               const int *idx, const float *weight, float *grad_points,
                               void *stream);

/* ------------------------------------------------------------------------
 * Fused set-abstraction block (no single reference entry point: the reference runs
 * this chain as PyTorch ops over materialised (B,C,M,K) tensors --
 * openpoints/models/layers/group.py:235-255,323-335 and
 * openpoints/models/backbone/pointnext.py:146-168).  Shapes supported by this
 * build: c_in = 32 features (+3 relative xyz), c_mid = 32, c_out = 64,
 * nsample = 32; anything else returns APN_EINVAL and callers use the unfused ops.
 *   xyz (B,N,3) f32, new_xyz (B,M,3) f32, ft (B,N,32) bf16 point-major copy of the
 *   features, idx (B,M,32) i32, w1 (32,35) f32 with columns [dp(3), f(32)],
 *   w2 (64,32) f32.  Per-channel sums cross workgroups WITHOUT fold launches: BatchNorm-1's statistics
 *   leave apn_sa_prep_stats as a few dozen partial rows that every workgroup of the next launch sums itself;
 *   every other per-channel sum goes through an ACCUMULATOR SET -- apn_sa_acc_words(ncol) unsigned 64-bit
 *   words, zeroed by an earlier launch, added to with integer atomics on a two-limb fixed-point value
 *   (csrc/apn_common.h: order-independent, the same bits every run) -- which the consumer kernel reads in
 *   its prologue; with reduced (e.g. all-reduced) float64 sums `sums*` the consumers take those instead.
 *   Weight gradients leave their producers as partial rows summed in float64 by apn_sa_bwd_finalize; G and
 *   gip are float atomic adds into zeroed buffers.
 *   "pack" = {scale, shift, mean, invstd}[C] of a BatchNorm folded to y*scale+shift.
 * Everything below only enqueues kernels (graph-capturable).
 * ------------------------------------------------------------------------ */

/* FPS that also writes new_xyz (B,M,3) = xyz[idx] (pointnext.py:146-147); n <= 16384.
 * temp == NULL: start from 1e10 everywhere (what callers fill temp with, subsample.py:94)
 * and leave no min-distances behind. */
APN_API int apn_furthest_point_sampling_xyz(int b, int n, int m, const float *xyz, float *temp,
                                            int *idxs, float *new_xyz, void *stream);

/* apn_ball_query that writes zeros into the rows of empty balls (no pre-zeroed idx needed). */
APN_API int apn_ball_query_zero(int b, int n, int m, float radius, int nsample,
                                const float *new_xyz, const float *xyz, int *idx, void *stream);

/* Workgroups the fused passes launch for B clouds x M queries (without / with a tile map). */
APN_API int apn_sa_grid_blocks(int b, int m);
APN_API int apn_sa_grid_rows(int b, int m, int with_tile_map);
/* workgroups (= partial rows partW2) of the backward pass */
APN_API int apn_sa_bwd_main_rows(int b, int m);
/* unsigned 64-bit words of an accumulator set of ncol columns */
APN_API int apn_sa_acc_words(int ncol);
/* 16-byte granular zero fill by a kernel (graph-capturable) */
APN_API int apn_zero_fill(void *base, long long bytes, void *stream);
/* Diagnostic: stamps[slot] = the device's 100 MHz wall clock when the launch runs (one thread; graph-capturable:
 * phase boundaries of a replayed step on every branch of the graph).  stamps: unsigned 64-bit words. */
APN_API int apn_debug_stamp(void *stamps, int slot, void *stream);
/* Diagnostic: `blocks` workgroups of 256 lanes hold 24 register values each for `turns` barrier-and-LDS-atomic turns and
 * check them: bad[i] (i < 24) = lanes whose i-th value changed, bad[24 .. 31] samples (index << 32 | value found).
 * bad: 32 unsigned 64-bit words, zeroed by the caller.  (Does register state survive beside other kernels?) */
APN_API int apn_debug_vgpr_hold(int blocks, int turns, unsigned long long *bad, void *stream);
/* Diagnostic: a packed-FP32 instruction with operand selection, checked result by result beside whatever else runs.
 * form 0: v_pk_add_f32 ... op_sel_hi:[1,0] (a pair's LOW register feeds both lanes); form 1: ... op_sel:[0,1] (its HIGH
 * register feeds both lanes: the form blamed in profiles/r04_packed_fp32_op_sel.md); form 2: form 1 behind `s_nop 7`.
 * bad[0] results of the lane that crosses halves wrong, bad[1] of those computed with the pair's OTHER register, bad[2]
 * other results wrong, bad[3] results checked, bad[7] samples taken, bad[8 + 3k ..] sample k (k < 8): {turn << 32 | block
 * << 8 | lane}, {found << 32 | wanted}, {operand << 32 | the other lane's result}.  bad: 32 unsigned 64-bit words,
 * zeroed by the caller. */
APN_API int apn_debug_vpk_probe(int blocks, int turns, int form, unsigned long long *bad, void *stream);

/* `precision` (every function that takes ft): 1 = operands rounded to bf16; 2 = operands split
 * into hi + lo bf16 parts, each product three MFMAs (hi*hi + hi*lo + lo*hi, "bf16x3"): fp32-grade
 * results (~1e-5) at 3x the (small) MFMA cost.  ft then holds `precision` tables of (B,N,32)
 * bf16 back to back: [hi] or [hi][lo]. */

/* Index stage, last piece (csrc/sa_geo.hip): occurrence statistics of the neighbourhoods.  For every support
 * point n: geo[b][n] = {occ, Dx, Dy, Dz} as four int64 -- the number of positions (query, slot) with
 * idx == n and the sum over them of d = (xyz[n] - new_xyz[query]) / radius (group.py:250-253) in units of
 * 2^-36 (integer sums: reproducible); dd[b][apn_sa_geo_dd_doubles(n)] (float64) = the cloud's shares of
 * sum d d^T over its positions, six values {xx, xy, xz, yy, yz, zz} per slab of 2048 points.  One launch, LDS
 * accumulation, nothing to clear; nsample must be 32. */
APN_API int apn_sa_geo_dd_doubles(int n);
APN_API int apn_sa_point_geo(int b, int n, int m, int nsample, float radius, const float *xyz,
                             const float *new_xyz, const int *idx, void *geo, void *dd, void *stream);

/* Forward launch 1 of 3: f (B,32,N) f32 -> ft, and (stats != 0) BatchNorm-1's batch statistics WITHOUT a pass
 * over the positions: part1[apn_sa_prep_rows(b, n)][64] = {sum, sumsq}[32] of y1 = conv1(cat(dp, f[idx])) from geo / dd
 * (y1 is affine in per-point and per-position terms; operands as the MFMA sees them).  Also clears `zero_words`
 * 64-bit words at `zero` (the accumulator set of the next launch). */
APN_API int apn_sa_prep_rows(int b, int n);
APN_API int apn_sa_prep_stats(int b, int n, const float *f, const void *geo, const void *dd, const float *w1,
                              int precision, int stats, void *ft, float *part1, void *zero, long long zero_words,
                              void *stream);

/* out[0..ncol) = float64 column sums of part[rows][ncol] (ncol <= 128, a power of two) /
 * the totals of an accumulator set; out[ncol] = count (this rank's positions), out[ncol + 1] = 1.
 * The SyncBatchNorm path reduces, all-reduces the ncol + 2 values over ranks (sums, GLOBAL count, world size),
 * then calls the consumer with `sums`: it takes the count from the reduced vector (its `count` argument is
 * ignored) and dL/dgamma, dL/dbeta are reported as global sum / world (what SyncBatchNorm +
 * DistributedDataParallel leave in .grad). */
APN_API int apn_sa_reduce_rows(const float *part, int rows, int ncol, double count, double *out,
                               void *stream);
APN_API int apn_sa_reduce_acc(const void *acc, int ncol, double count, double *out, void *stream);

/* BatchNorm fold as a launch of its own (the width-generic family, csrc/sa_wide*.hip): {sum, sumsq}[C] over
 * `count` positions (part[rows][2C], or sums[2C] when part == NULL) -> pack[4][C]; updates the running
 * buffers / num_batches_tracked when training (torch.nn.BatchNorm semantics); uses the running buffers when
 * not training.  Rider: sgn_out[i] = sign(sgn_gamma[i]), i < sgn_c.  C a multiple of 4, <= 1024. */
APN_API int apn_sa_bn_fold(const float *part, int rows, const double *sums, int c, double count,
                           const float *gamma, const float *beta, float eps, float momentum,
                           float *running_mean, float *running_var, void *num_batches_tracked,
                           int training, float *pack, const float *sgn_gamma, int sgn_c,
                           float *sgn_out, void *stream);

/* Forward launch 2 of 3.  Prologue: BatchNorm-1 (g1, b1, running buffers, eps, momentum, training flag; `count`
 * positions) folded from part1[rows1][64] -- or from sums1 -- by every workgroup (workgroup 0 writes pack1
 * [4][32] and updates the running buffers).  Then a1 = relu(bn1(y1)); y2 = conv2(a1);
 * ysel/ksel (B,M,64): per (query, channel) the extreme of y2 over the K neighbours (max where gamma2 >= 0,
 * min otherwise) and the neighbour slot holding it; acc2 (accumulator set, 128 columns, zeroed by
 * apn_sa_prep_stats) += {sum[64], sumsq[64]} of y2. */
APN_API int apn_sa_fwd_main(int b, int n, int m, int precision, float radius, const float *xyz,
                            const float *new_xyz, const void *ft, const int *idx, const int *tmap, const float *w1,
                            const float *w2, const float *g1, const float *b1, float *rm1, float *rv1, void *nbt1,
                            float eps1, float mom1, int train1, double count, const float *part1, int rows1,
                            const double *sums1, float *pack1, const float *gamma2, float *ysel, void *ksel,
                            void *acc2, void *stream);

/* Forward launch 3 of 3.  Prologue: BatchNorm-2 folded from acc2 (or sums2) by every workgroup (the first
 * writes pack2 [4][64] and updates the running buffers).
 * out (B,64,M) = act(ysel*scale2 + shift2 + Ws f[:, fidx] + bs); ws/bs/ft/fidx may be null
 * (no skip branch), relu = 0/1.  f is read from the point-major table(s) ft; fidx (B,M), ws (64,32), bs (64).
 * (zero_base, zero_floats: optional region -- the backward's atomically accumulated gip | accS | accT --
 * cleared by this launch, the forward's last, so that apn_sa_backward_seq(zero_bytes = 0) needs no fill launch) */
APN_API int apn_sa_fwd_out(int b, int n, int m, const float *ysel, const void *acc2, const double *sums2,
                           const float *g2, const float *b2, float *rm2, float *rv2, void *nbt2, float eps2,
                           float mom2, int train2, double count, float *pack2, const void *ft, int precision,
                           const int *fidx, const float *ws, const float *bs, int relu, float *out,
                           float *zero_base, long long zero_floats, void *stream);

/* Backward launch 1 of 4: g = g_out * [out > 0] (relu) ; goa (B,M,64) = g * scale2;
 * g_out (B,64,M) is read with element strides (gs_b, gs_c, gs_m) -- a broadcast upstream
 * gradient (stride 0, e.g. from loss = out.sum()) needs no materialised copy;
 * accS (accumulator set, 128 columns, zeroed) += {S1 = sum g, S2 = sum g*yhat_sel}[64]; with the skip branch
 * partWs[apn_sa_bwd_prep_rows(b, m)][64*32] = dL/dWs per block of 64 queries and gip (B,N,32) += Ws^T g at the
 * sampled points (zeroed): float atomic adds, or -- dup (int32[b], may be NULL; the tail of the row map's blob,
 * apn_sa_rowmap_many) says 0 for a cloud, i.e. its picks are m different points -- plain stores. */
APN_API int apn_sa_bwd_prep_rows(int b, int m);
APN_API int apn_sa_bwd_prep(int b, int n, int m, const float *g_out, long long gs_b,
                            long long gs_c, long long gs_m, const float *out, int relu,
                            const float *ysel, const float *pack2, const void *ft, int precision,
                            const int *fidx, const float *ws, float *goa, void *accS,
                            float *partWs, float *gip, const int *dup, void *stream);

/* Backward launch 2 of 4: the pass over the positions.  Prologue (every workgroup): the constants of
 * dL/dy2 = goa*[pos==ksel] + y2*D2 + E2 from accS (or sumsS) and pack2, Qm = W2^T diag(D2) W2, evec = E2 W2.
 * accT (accumulator set, 64 columns, zeroed) += {sum g_u, sum g_u*yhat1}[32] (g_u = dL/da1 * [a1 > 0]);
 * partW2[apn_sa_bwd_main_rows(b, m)][64*32] = the workgroup's share of dL/dW2 (sparse arg-max part +
 * D2 (W2 Gram) + E2 (x) sum a1);  GU[place][32] = g_u of every live tile-map row, stored at the row's place in the
 * point-sorted order (rowdst: apn_sa_rowmap_many; 32 b m rows of 32 floats, nothing to clear) -- round 5: NO float
 * atomics; a point's rows are consecutive and apn_sa_bwd_point_grads sums them in ascending row order, so every
 * gradient of the chain is bit-reproducible (rounds 1-4: A (B,N,32) += g_u by memory-side float atomics, or 64-bit
 * fixed-point integer atomics in a separate "deterministic" mode).  tmap and rowdst are required: the pass runs over the
 * tile map.  HA, HB (B,M,32) = g_u and yhat1 summed per query.  pack1 = BN1's [4][32] of the forward. */
APN_API int apn_sa_bwd_main(int b, int n, int m, int precision, float radius, const float *xyz,
                            const float *new_xyz, const void *ft, const int *idx, const int *tmap, const float *w1,
                            const float *w2, const float *pack1, const float *pack2, const void *accS,
                            const double *sumsS, double count, int train2, const float *goa, const void *ksel,
                            void *accT, float *partW2, const int *rowdst, float *GU, float *HA, float *HB,
                            void *stream);

/* Backward launch 3 of 4.  Prologue: the batch constants of dL/dy1 = g_u*ca + yhat1*cb + cc from accT (or sumsT).
 * dL/dy1 summed per source point (G) and per query (H), formed from the point's rows of GU (pcnt_poff: int32[2 b n],
 * how many rows gather a point and the place of the first -- apn_sa_rowmap_many), geo (apn_sa_point_geo), HA, HB, and
 * everything linear in them, one workgroup per 64-point tile: g_f (B,32,N) = G W1[:,3:] (+ gip); optional
 * g_p (B,N,3) += G W1[:,:3]/r and g_newp (B,M,3) = -H W1[:,:3]/r; partW[apn_sa_bwd_weight_rows(b, n)][32*38] =
 * per-block products for dL/dW1 (sa_glue.hip). */
APN_API int apn_sa_bwd_weight_rows(int b, int n);
APN_API int apn_sa_bwd_point_grads(int b, int n, int m, const float *GU, const int *pcnt_poff, const void *geo,
                                   const float *HA, const float *HB, const void *accT, const double *sumsT,
                                   double count, int train1, const float *pack1, const void *ft, int precision,
                                   const float *xyz, const float *new_xyz, const float *w1,
                                   const float *gip, float radius, float *partW, float *g_f,
                                   float *g_p, float *g_newp, void *stream);

/* Backward launch 4 of 4: column sums in float64 -> g_w1 (32,35) from partW, g_w2 (64,32) from partW2, optional
 * g_ws (64,32) from partWs; g_bs [64] = S1 of this rank (accS); g_b2 / g_g2 = S1 / S2 and g_b1 / g_g1 = T1 / T2
 * from the accumulator sets or, with reduced sums, global / world.  Any gradient pointer may be null. */
APN_API int apn_sa_bwd_finalize(const float *partW, int rows_w, float radius, float *g_w1,
                                const float *partWs, int rows_s, float *g_ws, const float *partW2, int rows_2,
                                float *g_w2, const void *accS, const double *sumsS,
                                const void *accT, const double *sumsT, float *g_bs, float *g_g2, float *g_b2,
                                float *g_g1, float *g_b1, void *stream);

/* Diagnostics: attach (NULL: detach) a buffer of 8 x 4 x workgroups 64-bit wall-clock stamps that the next
 * launches of the two tile passes fill per wave (scripts/stamp_passes.py).  Not for concurrent use. */
APN_API int apn_sa_debug_stamps(void *buf);

/* Whole-direction launch sequences (csrc/sa_seq.hip): the same kernels as above, enqueued
 * back-to-back by ONE call so that an eager step stays GPU-bound.  `phases` (bit mask
 * 1|2|4) selects the part to enqueue, so a caller can all-reduce the BatchNorm sums between
 * phases (SyncBatchNorm): forward 1 = prep + BatchNorm-1 sums, 2 = main pass, 4 = output; backward
 * 1 = (zero +) entry, 2 = main pass, 4 = point gradients + finalize.
 * sums* (float64, reduced over ranks) replace the partial rows / accumulator sets when non-NULL. */
APN_API int apn_sa_forward_seq(
    int phases, int precision, int b, int n, int m, float radius, const float *xyz, const float *new_xyz,
    const float *f, const int *idx, const int *tmap, const int *fidx, const void *geo, const void *dd,
    const float *w1, const float *w2, const float *ws, const float *bs,
    const float *g1, const float *b1, float *rm1, float *rv1, void *nbt1, float eps1, float mom1,
    int train1,
    const float *g2, const float *b2, float *rm2, float *rv2, void *nbt2, float eps2, float mom2,
    int train2,
    double count, int relu, void *ft, float *part1, const double *sums1, const double *sums2,
    float *pack1, float *pack2, void *acc2, float *ysel, void *ksel,
    float *out, float *zero_base, long long zero_floats, void *stream);
APN_API int apn_sa_backward_seq(
    int phases, int precision, int b, int n, int m, float radius, const float *xyz, const float *new_xyz,
    const int *idx, const int *tmap, const int *fidx, const void *geo, const float *w1, const float *w2,
    const float *ws, const void *ft, const float *pack1, const float *pack2, const float *ysel,
    const void *ksel, const float *out, int relu, int train1, int train2, double count,
    const float *g_out, long long gs_b, long long gs_c, long long gs_m,
    void *zero_base, long long zero_bytes, float *gip, void *accS, void *accT,
    const int *pcnt_poff, const int *rowdst, float *GU,   /* the row map (apn_sa_rowmap_many) and the rows' scratch */
    float *goa, float *partWs, float *partW2, float *partW, const double *sumsS, const double *sumsT,
    float *HA, float *HB,
    float *g_f, float *g_p, float *g_newp, float *g_w1, float *g_w2, float *g_g1, float *g_b1, float *g_g2,
    float *g_b2, float *g_ws, float *g_bs, void *stream);
/* Index stages of consecutive batches, overlapped: FPS (+ sampled coordinates) of batch A and,
 * in the SAME launch, the zero-filling ball query of batch B, whose new_xyz_b an earlier call
 * produced (csrc/fps.hip: fps_ball_kernel; 512 < n <= 4096, else the two launches back to
 * back).  Either half may be absent: xyz_a == NULL or xyz_b == NULL. */
APN_API int apn_sa_sample_overlap(int b, int n, int m, float radius, int nsample,
                                  const float *xyz_a, int *fidx_a, float *new_xyz_a,
                                  const float *xyz_b, const float *new_xyz_b, int *idx_b,
                                  void *stream);
/* FPS of one level of an index PYRAMID (no reference counterpart: the reference runs the full sampler at every level --
 * pointnext.py:146 per block, models_adaptpoint/generator_component4_15.py:406 per stage -- with the same result).
 * FPS is progressive: run on a sample's picks in pick order it returns picks 0, 1, 2, ... again whenever every arg-max
 * was unique.  xyz (B,n,3): the cloud (level 1) or the previous level's sampled coordinates in pick order; tie_prev (B)
 * or null: the previous level's record; tie_out (B): the first step whose arg-max was not unique (INT_MAX: none; 0: not
 * recorded).  A cloud with tie_prev[cloud] >= m gets idxs = 0 .. m-1 and a copy of its first m rows; any other cloud
 * the full sampler.  idxs (B,m) int32, new_xyz (B,m,3). */
APN_API int apn_furthest_point_sampling_nested(int b, int n, int m, const float *xyz, const int *tie_prev, int *idxs,
                                               float *new_xyz, int *tie_out, void *stream);
/* apn_sa_sample_seq (below) with the nested sampler: one level of an index pyramid. */
APN_API int apn_sa_sample_seq_nested(int b, int n, int m, float radius, int nsample, const float *xyz,
                                     const int *tie_prev, int *tie_out, int *fidx, float *new_xyz, int *idx, void *geo,
                                     void *dd, void *stream);
/* Index stage: temp := 1e10, FPS (+ sampled coordinates), ball query (zero-filling) and, with geo != NULL,
 * apn_sa_point_geo.  temp may be NULL (no min-distances kept).  n <= 16384 (the register-resident sampler; larger
 * clouds: apn_furthest_point_sampling + apn_ball_query). */
APN_API int apn_sa_sample_seq(int b, int n, int m, float radius, int nsample, const float *xyz,
                              float *temp, int *fidx, float *new_xyz, int *idx, void *geo, void *dd,
                              void *stream);

/* ------------------------------------------------------------------------
 * the grouping stage of the imitator's PointsetGrouper
 * (openpoints/models_adaptpoint/generator_component4_15.py:394-431, normalize = "anchor"):
 *   out[b][ch][q] = max_k ( alpha[ch] * (points[b][idx[b][q][k]][ch] - points[b][fidx[b][q]][ch]) + beta[ch] )
 * without the (B, np, K, C) intermediates.  points (B,N,C) f32 point-major as in the reference,
 * idx (B,M,K) from apn_ball_query, fidx (B,M) from apn_furthest_point_sampling, alpha/beta [C];
 * out (B,C,M); ksel (B,M,C) uint8 = position of the (first) maximum, kept for the backward.
 * C a power of two in 4..1024, K <= 255.
 * Backward: g_points (B,N,C) = alpha*g at the selected neighbour - alpha*g at the anchor, summed over the
 * queries: caller-zeroed; where a cloud's slice [N][8..32 channels] fits in LDS (N <= 4096) it is accumulated
 * there (LDS atomics) and stored whole, otherwise added with global float atomics;
 * part[apn_pointset_group_rows(b, m, c)][2C] = partial rows of {sum g*(x_sel - anchor), sum g} = dL/dalpha,
 * dL/dbeta (summed by the caller).
 * ------------------------------------------------------------------------ */
APN_API int apn_pointset_group_rows(int b, int m, int c);
APN_API int apn_pointset_group_max(int b, int n, int m, int c, int k, const float *points,
                                   const int *idx, const int *fidx, const float *alpha,
                                   const float *beta, float *out, void *ksel, void *stream);
APN_API int apn_pointset_group_max_grad(int b, int n, int m, int c, int k, const float *points,
                                        const int *idx, const int *fidx, const float *alpha,
                                        const void *ksel, const float *g_out, float *g_points,
                                        float *part, void *stream);

/* ------------------------------------------------------------------------
 * multi-head self-attention over the M points of a cloud with
 * head_dim 16 (the imitator's Anchor_selfattention,
 * openpoints/models_adaptpoint/generator_component4_15.py:467-474) without the (B,H,M,M)
 * score tensor:  out = softmax(q k^T / 4) v  per head.  q, k, v, out: (B, M, heads*16) f32 (the
 * layout the reference holds them in before its reshape/permute); M % 32 == 0.
 * apn_attention_prep writes the bf16 hi|lo operand images into `images`: 3 (forward only) or 6
 * (for_backward != 0) blocks of b*heads*m*32 bf16 = 64 bytes per point and head each.
 * apn_attention_fwd also returns lse (B,heads,M), the log2-domain log-sum-exp of every query.
 * apn_attention_bwd: g_out = dL/d out -> dq, dk, dv (B,M,heads*16); scratch = 2 * b*heads*m*32
 * bf16 + b*heads*m floats.
 * b, heads <= 65535 (grid dimensions).  `images`, `scratch`, `out`, dq, dk, dv are reached by 16-byte vector accesses
 * and must be 16-byte aligned (the row pitch heads*64 bytes keeps every row so): APN_EINVAL otherwise, before any launch.
 * ------------------------------------------------------------------------ */
/* The same attention for few points (0 < m <= apn_attention_small_max() = 32; the imitator's 4-anchor head): one wave
 * per (cloud, head) in float32; the backward recomputes the probabilities from q, k, v. */
APN_API int apn_attention_small_max(void);
APN_API int apn_attention_small_fwd(int b, int m, int heads, const float *q, const float *k, const float *v,
                                    float *out, void *stream);
APN_API int apn_attention_small_bwd(int b, int m, int heads, const float *q, const float *k, const float *v,
                                    const float *g_out, float *dq, float *dk, float *dv, void *stream);
APN_API int apn_attention_prep(int b, int m, int heads, const float *q, const float *k,
                               const float *v, void *images, int for_backward, void *stream);
APN_API int apn_attention_fwd(int b, int m, int heads, const void *images, float *out, float *lse,
                              void *stream);
APN_API int apn_attention_bwd(int b, int m, int heads, const void *images, const float *out,
                              const float *lse, const float *g_out, void *scratch, float *dq,
                              float *dk, float *dv, void *stream);

/* ------------------------------------------------------------------------
 * Token attention at head_dim 64 (csrc/token_attention.hip): PointViT's `Attention`
 * (openpoints/models/backbone/pointvit.py), out = softmax(q k^T / 8) v per (cloud, head), for ANY t >= 1, without
 * the (B,H,T,T) score tensor in either direction.
 *   qkv   (B, t, [3][heads][64]) f32, as nn.Linear(dim, 3 dim) leaves it
 *   out   (B, t, heads*64) f32;  lse (B, heads, t) f32, the log2-domain log-sum-exp of every query
 *   bwd:  g_out (B, t, heads*64) = dL/d out -> dqkv (B, t, [3][heads][64]), every element written;
 *         delta: scratch of b*heads*t floats (rowsum(g_out * out), written first)
 * No atomics: two calls give the same bits, and a (cloud, head)'s results do not depend on b, heads or its neighbours.
 * 0 < b, heads <= 65535 (grid dimensions), 0 < t <= apn_token_attention_max_tokens() = 2^24 and
 * b*t*heads < 16 * (2^31 - 1).  qkv, out, g_out and dqkv are reached by 16-byte vector accesses and must be 16-byte
 * aligned: APN_EINVAL otherwise, before any launch.
 * ------------------------------------------------------------------------ */
APN_API int apn_token_attention_max_tokens(void);
APN_API int apn_token_attention_fwd(int b, int t, int heads, const float *qkv, float *out, float *lse, void *stream);
APN_API int apn_token_attention_bwd(int b, int t, int heads, const float *qkv, const float *out, const float *lse,
                                    const float *g_out, float *delta, float *dqkv, void *stream);

/* ------------------------------------------------------------------------
 * SimpleView's six-view depth rasteriser (csrc/depth_views.hip): `PCViews.get_img` -> `points2depth` -> `distribute`
 * (openpoints/models/backbone/simpleview_util.py) in one forward and one backward launch.
 *   points (b,n,3) f32; rot (views,3,3), trans (views,3): q = p R_v - t_v (fp32, summed left to right, no fma);
 *   rot == NULL: the points are camera-frame already and views must be 1.
 *   img, sw (b*views, h, w): image b*views + v is cloud b under view v.  Per pixel, in ascending (point, i, j) order of
 *   the sx*sy splats of every point: sw = sum w, sv = sum z w with w = 1 / (z + 1e-12f); img = sv / (sw + (sw == 0)).
 *   Every element of img and sw is written (nothing has to arrive zeroed); no float atomic, no memset, no scratch: two
 *   calls give the same bits.  Non-finite coordinates contribute nothing.
 *   bwd: g_img (b*views,h,w) = dL/d img, img and sw as the forward left them -> dpoints (b,n,3), every element
 *   written; the gradient flows through the depth only (the pixel coordinates pass through ceil).
 * sx, sy in {1,2,4}; n*sx*sy <= apn_depth_views_max_splats() = 16384, h*w <= apn_depth_views_max_pixels() = 65536,
 * views <= apn_depth_views_max_views() = 64, b*views <= apn_depth_views_max_images() = 2^22 - 1 (workgroups of 1024
 * threads: the grid stays below 2^32 threads), b*n < 2^31: APN_EINVAL otherwise, before any launch.
 * ------------------------------------------------------------------------ */
APN_API int apn_depth_views_max_splats(void);
APN_API int apn_depth_views_max_pixels(void);
APN_API int apn_depth_views_max_views(void);
APN_API int apn_depth_views_max_images(void);
APN_API int apn_depth_views_fwd(int b, int n, int views, int h, int w, int sx, int sy, const float *points,
                                const float *rot, const float *trans, float *img, float *sw, void *stream);
APN_API int apn_depth_views_bwd(int b, int n, int views, int h, int w, int sx, int sy, const float *points,
                                const float *rot, const float *trans, const float *g_img, const float *img,
                                const float *sw, float *dpoints, void *stream);

/* ---- width-generic fused grouped MLP (csrc/sa_wide.hip): C_mid = H in {32,64,128,256}, C_out = 2H,
 * K = 32.  conv1 is hoisted to the points by the caller: U (B,N,H) = W1f f + W1p p / r per point,
 * V (B,M,H) = W1p new_p / r per query, so that y1[q,k] = U[idx[q,k]] - V[q]
 * (openpoints/models/backbone/pointnext.py:157-166 with group.py:248-254).  pack1 = BatchNorm-1's
 * {scale, shift, mean, invstd}[H].  Weight operands are "B images" (bf16 hi/lo parts in MFMA
 * fragment order, adaptpoint_amd/fused_wide.py::mfma_b_image). ---- */
APN_API int apn_sa_wide_grid(int b, int m);          /* workgroups = partial rows of the three passes */
/* Tile map (distinct-hit packing; part of the index stage: it depends on idx only).  A ball query lists a
 * query's cnt distinct hits and fills the other 32 - cnt slots with copies of slot 0
 * (ball_query_gpu.cu:41-48), and every copy computes the same y1, a1, y2: the passes below run over ROWS
 * = (query, distinct slot, multiplicity), whole queries packed in order into 32-row MFMA tiles.
 * tmap: int32[apn_sa_wide_tilemap_ints(b, m)], device memory:
 *   [0] tiles in use; [4, 4 + b m) first query of each tile; [4 + roundup4(b m), ... + 32 b m) the rows,
 *   qlocal | slot << 8 | mult << 16 | (row 0: queries in the tile) << 24, mult = 0 for padding; then
 *   32 b m ints: every row's neighbour idx[query][slot]; scratch.
 * mode 1: fold the copies of slot 0 of every index row that has the ball-query structure (checked row
 * by row; any other row is kept whole); mode 0: one tile per query, 32 rows of multiplicity 1.
 * Every index must lie in [0, n), n the support points per cloud: the map stores idx as it comes, and
 * apn_sa_wide_csr adds it to the cloud's first point without a clamp. */
APN_API int apn_sa_wide_tilemap_ints(int b, int m);
APN_API int apn_sa_wide_tilemap(int b, int m, int mode, const int *idx, int *tmap, void *stream);
/* count tile maps in one pair of launches (the batches of a stacked index stage): map z reads idx + z * b * m * 32
 * and fills tmap + z * apn_sa_wide_tilemap_ints(b, m). */
APN_API int apn_sa_wide_tilemap_many(int count, int b, int m, int mode, const int *idx, int *tmap, void *stream);
/* The ROW MAP of `count` stacked tile maps (round 5; index-stage data, a pure function of the neighbour indices): per batch z
 *   pcnt_poff + z * apn_sa_rowmap_ints(b, n)  int32[2 b n + b]: per support point, the number of tile-map rows that gather it
 *                          and the place of the first of them in the point-sorted order (a cloud's places lie in its own
 *                          range of row ids); then per cloud dup = 0 iff its m picks fidx (z-th block of b m ints; may be
 *                          NULL: dup = 1) are m different points -- apn_sa_bwd_prep then STORES the skip branch's gradient
 *                          rows instead of adding them with float atomics;
 *   rowdst + z * 32 b m    int32[32 b m]: the place of every live row of map z = tmap + z * apn_sa_wide_tilemap_ints(b, m).
 * A point's rows occupy consecutive places in ascending row order; GU needs apn_sa_rowmap_places(b, n, m) rows of 32 floats.
 * Replaces the scatter-add of the reference's grouping backward (group_points_grad_kernel_fast,
 * openpoints/cpp/pointnet2_batch/src/group_points_gpu.cu:14-46, atomicAdd per element) inside the fused chain by a store +
 * an ordered sum.  scratch: int32[32 b m] (multi-launch path only). */
APN_API int apn_sa_rowmap_places(int b, int n, int m);
APN_API int apn_sa_rowmap_ints(int b, int n);
APN_API int apn_sa_rowmap_many(int count, int b, int n, int m, const int *tmap, const int *fidx, int *pcnt_poff, int *rowdst, int *scratch,
                               void *stream);
/* out[ncol] (float64) = column sums of part[rows][ncol] (float32) in a fixed order; two passes
 * through scratch[apn_sa_wide_colsum_chunks(rows, ncol)][ncol] (float64) when there is more than one chunk */
APN_API int apn_sa_wide_colsum_chunks(int rows, int ncol);
APN_API int apn_sa_wide_colsum(const float *part, int rows, int ncol, double *scratch, double *out,
                               void *stream);
/* part[grid][2H] = {sum, sumsq} of y1 */
APN_API int apn_sa_wide_stats1(int b, int n, int m, int c_mid, const float *U, const float *V,
                               const int *idx, const int *tmap, float *part, void *stream);
/* a1 = relu(scale1 y1 + shift1), y2 = a1 W2^T (w2_image: B image of W2^T, H x O, min(4, O/32) column
 * tiles per block) -> ysel/ksel (B,M,O): per (query, channel) the extreme of y2 over the K slots
 * (max where sgn2 = +1, min where -1; first slot among equals) and that slot;
 * part[grid][2*O] = {sum, sumsq} of y2 */
APN_API int apn_sa_wide_fwd_main(int b, int n, int m, int c_mid, int c_out, const float *U, const float *V,
                                 const int *idx, const int *tmap, const void *w2_image, const float *pack1,
                                 const float *sgn2, float *ysel, void *ksel, float *part, void *stream);
/* dL/da1 = S W2 + a1 Qm + evec (z_image: B image of [W2 ; Qm], (O+H) x H, min(4, H/32) column tiles
 * per block; S[pos,c] = goa[q,c] [ksel[q,c] == pos]), g_u = dL/da1 [a1 > 0]:
 * GU (32 b m, H): row tile * 32 + r = g_u summed over the positions the tile map's row stands for (rows in
 * use only; no atomics -- apn_sa_wide_point_grads sums them per point through the inverse map),
 * HA (B,M,H) = sum_k g_u, HB (B,M,H) = sum_k yhat1, part[grid][2H] = {sum g_u, sum g_u yhat1}.
 * evec == NULL: BatchNorm-2 on running statistics (D2 = E2 = 0): the a1 Qm part of the chain is skipped. */
APN_API int apn_sa_wide_bwd_main(int b, int n, int m, int c_mid, int c_out, const float *U, const float *V,
                                 const int *idx, const int *tmap, const void *z_image, const float *pack1,
                                 const float *evec, const float *goa, const void *ksel, float *GU,
                                 float *HA, float *HB, float *part, float *r_part, void *stream);
/* 1 when apn_sa_wide_bwd_main also leaves the weight-gradient products, as r_part[apn_sa_wide_grid(b, m)]
 * [(O+H) H + H] = the workgroups' shares of {[S^T ; a1^T] a1, sum a1} (c_mid = 32); 0: r_part is ignored and
 * apn_sa_wide_wgrad computes them */
APN_API int apn_sa_wide_wgrad_fused(int c_mid);
/* The small kernels around those passes (csrc/sa_wide_glue.hip).
 * image: B image of Bm (kd x nc): rows < k0 from src0 (row-major kd x nc, or nc x k0 read transposed when
 *   trans0), the rest from src1 ((kd - k0) x nc); ct column tiles per block.
 * bwd_prep: g (B,O,M; element strides gs_*), zeroed where out_act (B,O,M; NULL: no mask) is not positive
 *   -> goa (B,M,O) = g scale2, gpre (B,M,O; NULL: not wanted) = g, and
 *   part_s[apn_sa_wide_bwd_prep_rows(b, m)][2*O] = {sum g, sum g yhat_sel}.
 * consts2 / consts1: the BatchNorm backward constants from those rows (or from `sums`: float64
 *   {S[2C], global count, world} all-reduced over ranks): d2e2 = {D2, E2}[O]; cabc = {ca, cb, cc}[H];
 *   dgamma, dbeta (global / world with `sums`).
 * point_terms: G (B,N,H) = dL/dU = ca (GU rows of the point, summed through the inverse map of apn_sa_wide_csr)
 *   + cb inv1 (occ (U - mean1) - SP . W1p / r) + cc occ, with geo = {occ, SP} of apn_sa_wide_csr;
 *   HA <- -dL/dV = ca HA + cb HB + 32 cc (B,M,H); w1 (H x ldw) with W1p in its first three columns. */
APN_API int apn_sa_wide_image(const float *src0, int k0, int trans0, const float *src1, int kd, int nc, int ct,
                              void *image, void *stream);
APN_API int apn_sa_wide_bwd_prep_rows(int b, int m);
APN_API int apn_sa_wide_bwd_prep(int b, int m, int c_out, const float *g, long long gs_b, long long gs_c,
                                 long long gs_m, const float *ysel, const float *pack2, const float *out_act,
                                 float *gpre, float *goa, float *part_s, void *stream);
APN_API int apn_sa_wide_consts2(const float *part_s, int rows, const double *sums, int c_out,
                                const float *pack2, double count, int training, float *d2e2,
                                float *g_gamma2, float *g_beta2, void *stream);
APN_API int apn_sa_wide_consts1(const float *part_t, int rows, const double *sums, int c_mid,
                                const float *pack1, double count, int training, float *cabc,
                                float *g_gamma1, float *g_beta1, void *stream);
APN_API int apn_sa_wide_point_terms(int b, int n, int m, int c_mid, const float *cabc, const float *pack1,
                                    const float *U, const float *geo, const float *w1, int ldw, float radius,
                                    const float *GU, const int *pcnt_poff, const int *plist, float *G, float *HA,
                                    const float *HB, void *stream);
/* r_part[splits][(O+H) H + H] = partial {[S^T ; a1^T] a1 (rows < O: the sparse part of dL/dW2; the rest:
 * the Gram matrix of a1), sum of a1}; the caller sums the splits (apn_sa_wide_colsum) */
APN_API int apn_sa_wide_wgrad_splits(int b, int m, int c_mid);
APN_API int apn_sa_wide_wgrad(int b, int n, int m, int c_mid, int c_out, const float *U, const float *V,
                              const int *idx, const int *tmap, const float *pack1, const float *goa,
                              const void *ksel, int splits, float *r_part, void *stream);

/* Inverse map of the tile map (index stage): pcnt_poff int32[2 b n] = for every support point the number of
 * rows that gather it and where its list starts in plist int32[32 b m] (row ids tile * 32 + r, ascending);
 * geo float[4 b n] (may be NULL) = {occurrences, sum of the gathering queries' coordinates} per point; with fidx (b,m) = the
 * point every query is (FPS picks) also fq int32[b n] = the query a point is, or -1 (both may be NULL).
 * Every index of the map's idx must lie in [0, n): a row's neighbour is added to the cloud's first point as it
 * is (no clamp), and pcnt / plist / geo are written at that address. */
APN_API int apn_sa_wide_csr(int b, int n, int m, const int *idx, const float *new_xyz, const int *tmap,
                            int *pcnt_poff, int *plist, float *geo, const int *fidx, int *fq, void *stream);
/* The dense kernels of the path (csrc/sa_wide_dense.hip), one launch each:
 * fwd_prep: U (B,N,H) = W1f f + W1p p / r, V (B,M,H) = W1p new_p / r (w1: H x (C+3), coordinates first, as the
 *   reference's cat([dp, fj])), and the B image of W2^T (w2: O x H); with fq (B,N; apn_sa_wide_csr) also
 *   fs (B,M,C) = the sampled points' own features f[:, :, fidx] as query-major rows (fs NULL: not wanted);
 *   with geo (B,N,4; apn_sa_wide_csr) also part1[apn_sa_wide_fwd_prep_rows(b, n, m)][2H] = partial {sum, sumsq}
 *   of y1 over ALL positions -- BatchNorm-1's batch statistics from per-point and per-query terms alone
 *   (sum y1 = sum_n occ U - 32 sum_q V, ...), in place of apn_sa_wide_stats1's pass (part1 NULL: not wanted).
 * out: out (B,O,M) = act(ysel (B,M,O) scale2 + shift2 + skip) (pack2 = {scale, shift, mean, invstd}[O]);
 *   skip = ws (O x C) fs + bs, the residual branch on the sampled points' features fs (B,M,C) of fwd_prep
 *   (ws NULL: none; bs may be NULL); act = ReLU when relu.
 * bwd_mid: from part_s (or `sums`, as consts2): d2e2, dgamma2, dbeta2, evec[H] = E2 W2 and the B image of
 *   [W2 ; Qm], Qm = W2^T diag(D2) W2.
 * bwd_fin: from part_t (or `sums`, as consts1): cabc, dgamma1, dbeta1; and g_w2 (O,H) = R_S + D2 (W2 Gram)
 *   + E2 (x) suma, with R float64[(O+H) H + H] = {R_S ; Gram ; suma} (apn_sa_wide_wgrad's splits summed).
 * point_grads (C, H <= 64): G = dL/dU per point (GU rows summed through the inverse map, plus BatchNorm-1's
 *   mean/variance terms), g_f (B,C,N) = G W1f, g_p (B,N,3) = G W1p / r, g_q (B,M,3) = -Hq W1p / r (either may
 *   be NULL); with a residual branch (c_skip = O > 0: gpre (B,M,O) from bwd_prep, fq (B,N) = the query a point
 *   is or -1, fs (B,M,C) of fwd_prep, ws (O x C)) g_f also receives ws^T gpre at the sampled points;
 *   w_part[apn_sa_wide_point_grads_rows(b, n)][apn_sa_wide_point_grads_cols(C, H, O)] = the workgroups' shares
 *   of {dL/dW1 (H x (C+3)), dL/dws (O x C), dL/dbs (O)}; w_part NULL: no weight takes a gradient, the shares are
 *   not formed (the frozen classifier of the GAN's feedback pass).
 * colsum_f32: out[ncol] (float32) = column sums (in float64, fixed order) of part[rows][ncol]. */
APN_API int apn_sa_wide_fwd_prep(int b, int c_in, int n, int m, int c_mid, int c_out, float radius, const float *f,
                                 const float *p, const float *new_p, const float *w1, const float *w2, float *U,
                                 float *V, void *w2_image, const int *fq, float *fs, const float *geo, float *part1,
                                 void *stream);
APN_API int apn_sa_wide_fwd_prep_rows(int b, int n, int m);
APN_API int apn_sa_wide_out(int b, int m, int c_out, const float *ysel, const float *pack2, int c_in,
                            const float *fs, const float *ws, const float *bs, int relu, float *out, void *stream);
APN_API int apn_sa_wide_bwd_mid(const float *part_s, int rows, const double *sums, int c_mid, int c_out,
                                const float *pack2, double count, int training, const float *w2, float *d2e2,
                                float *g_gamma2, float *g_beta2, float *evec, void *z_image, void *stream);
APN_API int apn_sa_wide_bwd_fin(const float *part_t, int rows, const double *sums, int c_mid, int c_out,
                                const float *pack1, double count, int training, float *cabc, float *g_gamma1,
                                float *g_beta1, const double *R, const float *d2e2, const float *w2, float *g_w2,
                                void *stream);
APN_API int apn_sa_wide_point_grads_rows(int b, int n);
APN_API int apn_sa_wide_point_grads(int b, int c_in, int n, int m, int c_mid, float radius, const float *GU,
                                    const int *pcnt_poff, const int *plist, const float *geo, const float *U,
                                    const float *f, const float *p, const float *new_p, const float *HA,
                                    const float *HB, const float *cabc, const float *pack1, const float *w1,
                                    int c_skip, const float *gpre, const int *fq, const float *fs, const float *ws,
                                    float *g_f, float *g_p, float *g_q, float *w_part, void *stream);
APN_API int apn_sa_wide_point_grads_cols(int c_in, int c_mid, int c_skip);
APN_API int apn_sa_wide_colsum_f32(const float *part, int rows, int ncol, float *out, void *stream);

/* ------------------------------------------------------------------------
 * the imitator's per-point MLP layer `ConvBNReLU1D` =
 * Conv1d(kernel 1, no bias) + BatchNorm1d (+ ReLU)
 * (openpoints/models_adaptpoint/generator_component4_15.py:92-104; instantiated as the embedding, the four
 * extract_feat_list layers :588-657 and the `fuse` layer of PointNetFeaturePropagation :330-366), which the
 * reference runs as cuDNN convolution / batch-norm calls.  Tensors are channels-first contiguous float32 as
 * torch.nn.Conv1d takes them: x (B,c_in,N), w (c_out,c_in), y / out / g / gy (B,c_out,N).  Any sizes.
 * precision = 2: operands split into two bf16 planes (three MFMAs per product, ~4e-6 of an fp32 contraction);
 *   3: three planes, six MFMAs, fp32-class (~2e-7).  f32 accumulation either way.
 * conv_forward: y = w x per cloud; part (may be NULL)
 *   [apn_pw_conv_tiles(b, n)][2][c_out] = each 128-position tile's {sum, M2 = sum of squared deviations from the
 *   tile's own mean} of y per channel (combined over tiles in float64 by bn_act: no E[y^2] - mean^2 cancellation).
 * bn_act: out = [relu](gamma (y - mean) invstd + beta); training: batch statistics folded (float64) from `part`
 *   (tiles rows), running_mean / running_var updated with `momentum` (unbiased variance) and batches[0] += 1
 *   (each may be NULL); otherwise the running statistics are used.  stat [4][c] = {mean, invstd, scale, shift}.
 * bn_act_grad: gy = dL/dy from g = dL/dout (BatchNorm's batch-statistics gradient when training), g_gamma,
 *   g_beta [c] (may be NULL); part_b = scratch [apn_pw_bn_act_grad_splits(b, c)][2][c].  One launch when a channel's b * n
 *   values fit one workgroup's registers (b * n <= 32768, n % 4 == 0), else two.
 * conv_grad_input: gx (B,c_in,N) = w^T gy.   conv_grad_weight: gw (c_out,c_in) = sum_b gy_b x_b^T, split over
 *   apn_pw_conv_grad_weight_splits(...) ranges of (cloud, position) whose shares (scratch [splits][c_out][c_in])
 *   are added in the shared order at 4 lanes ("Partial-row folds", above): bit-reproducible. */
APN_API int apn_pw_conv_tiles(int b, int n);
APN_API int apn_pw_conv_forward(int b, int c_in, int c_out, int n, int precision, const float *x, const float *w,
                                float *y, float *part, void *stream);
APN_API int apn_pw_bn_act(int b, int c, int n, const float *y, const float *part, int tiles, const float *gamma,
                          const float *beta, float eps, float momentum, int training, int relu, float *run_mean,
                          float *run_var, long long *batches, float *stat, float *out, void *stream);
APN_API int apn_pw_bn_act_grad_splits(int b, int c);
APN_API int apn_pw_bn_act_grad(int b, int c, int n, const float *g, const float *y, const float *stat, int training,
                               int relu, float *part_b, float *gy, float *g_gamma, float *g_beta, void *stream);
APN_API int apn_pw_conv_grad_input(int b, int c_in, int c_out, int n, int precision, const float *gy, const float *w,
                                   float *gx, void *stream);
APN_API int apn_pw_conv_grad_weight_splits(int b, int c_in, int c_out, int n);
APN_API int apn_pw_conv_grad_weight(int b, int c_in, int c_out, int n, int precision, const float *gy, const float *x,
                                    float *scratch, float *gw, void *stream);

/* The contraction kernel of the per-point layers as such (csrc/pointwise.hip), for the small dense products around
 * the fused set-abstraction blocks (conv1 at the points, dL/df, dL/dW1 of the wide blocks):
 *   splits == 0: d[z] (r x q, ldd >= q) = a[z] (r x k) b[z] (k x q), z < nbatch (a batch stride of 0 shares the operand);
 *   splits  > 0: d (r x q, ldd == q) = sum_z a[z] b[z] in `splits` shares (apn_pw_contract_splits; scratch
 *                [splits][r][q]) added in the shared order at 4 lanes ("Partial-row folds", above).
 * a_kcont / b_kcont: the operand's element (i, k) lies at i * ld + k (1) or at k * ld + i (0). */
APN_API int apn_pw_contract_splits(int nbatch, int r, int q, int k);
APN_API int apn_pw_contract(int nbatch, int r, int q, int k, const float *a, long long a_batch, int lda, int a_kcont,
                            const float *b, long long b_batch, int ldb, int b_kcont, float *d, long long d_batch, int ldd,
                            int splits, float *scratch, int precision, void *stream);
/* TWO such products of the same operand form (a_kcont, b_kcont shared) as ONE launch: a grid that is the concatenation
 * of both problems' 128 x 128 tile grids, the problem picked from the workgroup index.  Every array argument has two
 * entries, problem p described as for apn_pw_contract.  splits[p] == 0 for both: d[p][z] = a[p][z] b[p][z] with leading
 * dimension ldd[p].  splits[p] > 0 for both (apn_pw_contract2_splits(p, ...)): d[p] = sum_z a[p][z] b[p][z] in
 * splits[p] shares (scratch[p]: [splits[p]][r][q]) added in that order by one fold launch that writes the r x q result
 * with leading dimension ldd[p] >= q[p] -- the two results may be column blocks of one matrix.  The fast loaders need
 * 16-byte aligned operand origins, rows and batch strides; anything else takes the value-by-value loads (correct, slower).
 * For pairs that each fill less than the chip (the hoisted feature-propagation block, csrc/feature_prop.hip). */
APN_API int apn_pw_contract2_splits(int which, int nbatch0, int r0, int q0, int k0, int nbatch1, int r1, int q1, int k1);
APN_API int apn_pw_contract2(int a_kcont, int b_kcont, int precision, const int *nbatch, const int *r, const int *q,
                             const int *k, const float *const *a, const long long *a_batch, const int *lda,
                             const float *const *b, const long long *b_batch, const int *ldb, float *const *d,
                             const long long *d_batch, const int *ldd, const int *splits, float *const *scratch,
                             void *stream);

/* Feature propagation with its convolution hoisted to the coarse points (csrc/feature_prop.hip): what follows the two
 * products a = W[:, :C1] f1 (B,O,n) and u = W[:, C1:] f2 (B,O,m):
 *     y[b][o][i] = a[b][o][i] + sum_{j<3} weight[b][i][j] * u[b][o][idx[b][i][j]]
 * a may be null (no skip features); idx / weight (B,n,3) as apn_three_nn + apn_three_nn_weights leave them; y may alias a.
 * training != 0: y and part are written -- part [apn_pw_conv_tiles(b, n)][2][o], BatchNorm's partial statistics in the
 *   layout apn_pw_bn_act folds ({sum, M2 around the tile's mean} per 128 columns of a cloud); apn_pw_bn_act follows.
 * training == 0: out = [relu](scale y + shift) from the running statistics (gamma / beta may be null) in the same launch;
 *   y (the pre-activation, what apn_pw_bn_act_grad reads) and stat [4][o] are written when not null.
 * Fixed-order sums only: results are bit-identical from run to run.
 * idx is TRUSTED to lie in [0, m), as apn_three_interpolate trusts it: it is not validated (an index outside is clamped
 * into the row, so it reads a wrong element, never memory outside u).
 * Negative sizes, b > 65535 or a missing pointer -> APN_EINVAL; b, o or n == 0 -> APN_OK without a launch. */
APN_API int apn_fp_blend_stats(int b, int o, int m, int n, const float *a, const float *u, const int *idx,
                               const float *weight, float *y, float *part, int training, const float *gamma,
                               const float *beta, const float *run_mean, const float *run_var, float eps, int relu,
                               float *stat, float *out, void *stream);

/* The same block with a per-cloud conditioning vector in front of the concatenation, W [cond 1^T ; f1 ; blend(f2)]
 * (PointNextPartDecoder's class conditioning, openpoints/models/backbone/pointnext.py:626-663): the vector's share of the
 * product is c (B,O), c[b] = W[:, :Cc] cond_b, one number per (cloud, channel), and
 *     y[b][o][i] = (a[b][o][i] + blend(u)[b][o][i]) + c[b][o]         -- this association order; a null: blend(u) + c
 * through the SAME kernel as apn_fp_blend_stats (one more pointer); every other argument as there.  c null -> APN_EINVAL.
 * _cond_grad: gc (B,O) = sum_i gy[b][o][i], the gradient with respect to c: one wave per row, lane l adds elements
 *   l, l + 64, ... in ascending order, then a fixed butterfly over the lanes; no atomic, bit-identical from run to run. */
APN_API int apn_fp_blend_stats_cond(int b, int o, int m, int n, const float *a, const float *u, const int *idx,
                                    const float *weight, const float *c, float *y, float *part, int training,
                                    const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                    float eps, int relu, float *stat, float *out, void *stream);
APN_API int apn_fp_cond_grad(int b, int o, int n, const float *gy, float *gc, void *stream);

/* out[z][j][i] = in[z][i][j] for in (nbatch, r, c) float32, contiguous: the layout change between the per-point layers'
 * (B, C, N) and the grouper's / attention's (B, N, C) (generator_component4_15.py:650-657 permutes and lets PyTorch copy). */
APN_API int apn_pw_transpose(int nbatch, int r, int c, const float *in, float *out, void *stream);
/* three_nn's squared distances (n, 3) -> the inverse-distance weights of openpoints/models/layers/upsampling.py:97-100,
 * w_j = (1 / (sqrt(d2_j) + 1e-8)) / sum_j (...): one launch for the five elementwise ones of the PyTorch form. */
APN_API int apn_three_nn_weights(long long n, const float *dist2, float *weight, void *stream);

/* the per-anchor transforms of AdaptPoint_Augmentor.local_transformaton
 * (openpoints/models_adaptpoint/generator_component4_15.py:236-297): prob (n,9) the imitator's numbers per anchor,
 * keep (n,3) / axes (n,3) the call's random switches as floats -> lin (n,3,3) = R diag(s), off (n,3); formulas in
 * csrc/augment.hip.  _grad: g_prob (n,9) from g_lin (n,3,3) and g_off (n,3) (either may be NULL = zero). */
APN_API int apn_anchor_transforms(int n, const float *prob, const float *keep, const float *axes, float r_range,
                                  float s_range, float t_range, float *lin, float *off, void *stream);
APN_API int apn_anchor_transforms_grad(int n, const float *prob, const float *keep, const float *axes, float r_range,
                                       float s_range, float t_range, const float *g_lin, const float *g_off,
                                       float *g_prob, void *stream);

/* The deformation that consumes them (generator_component4_15.py:156-232, 313-327 and the mask at :180): kernel
 * regression weights towards the m <= 8 anchors, blend of the anchors' affine maps, unit-sphere normalisation, mask:
 *   xyz (B,n,3), anchors (B,m,3), lin (B,m,3,3), off (B,m,3), axes (B,3) floats, mask (B,n) or NULL ->
 *   out (B,n,3); z (B,n,3) and stat (B,8) are kept for the backward.  n <= 4096.  One workgroup per cloud.
 * _backward: g_lin (B,m,3,3), g_off (B,m,3), g_mask (B,n) (may be NULL) from g_out (B,n,3). */
APN_API int apn_deform_forward(int b, int n, int m, const float *xyz, const float *anchors, const float *lin,
                               const float *off, const float *axes, const float *mask, float sigma, float *z, float *stat,
                               float *out, void *stream);
APN_API int apn_deform_backward(int b, int n, int m, const float *xyz, const float *anchors, const float *axes,
                                const float *mask, float sigma, const float *z, const float *stat, const float *g_out,
                                float *g_lin, float *g_off, float *g_mask, void *stream);

/* PointWOLF's per-anchor transforms (openpoints/online_aug/pointwolf.py:110-148) from the call's random draws, for
 * apn_deform_forward: draws = keep (b*m*3) | axis code 1..7 (b*m) | degree (b*m*3) | scale (b*m*3) | translation
 * (b*m*3) | kernel-axis code 1..7 (b), all float; uniform = 0: the reference's values, uniform = 1: U[0,1) numbers that
 * the kernel maps onto the same distributions.  -> lin (b,m,3,3) = R diag(s), off (b,m,3), kaxes (b,3) in {0,1}.
 * One thread per anchor; formulas in csrc/online_aug.hip. */
APN_API int apn_pointwolf_params(int b, int m, const float *draws, int uniform, float r_range, float s_range,
                                 float t_range, float *lin, float *off, float *kaxes, void *stream);

/* RSMix (openpoints/online_aug/rsmix_provider.py:161-222), points (b,n,c) float32 with xyz first, c >= 3,
 * n <= 8192, 0 < nsample < n; draws (3b) int32 = perm | i1 | i2.
 * _select: 2b selections (s < b: cloud s around point i1[s]; s >= b: cloud perm[s-b] around point i2[s-b]) of the points
 *   with numpy's float64 expanded squared distance <= r2 (knn_k < 0) or <= its knn_k-th smallest value (knn_k >= 0):
 *   the first nsample of them in ascending index order -> members (2b, nsample) int32 (-1 past the count), counts (2b).
 * _mix: per cloud, with |E| = counts[cl] and |A| = counts[b+cl]: the cloud without its erase set, in order, followed by
 *   |E| rows taken through pick (b, nsample) int32 -- positions in the add list, moved by q1 - q2 in float64 (|A| > 0),
 *   or rows in [0, n-|E|) of the cloud itself (|A| = 0); out (b,n,c), lam (b) = |E|/n (0 if either set is empty). */
APN_API int apn_rsmix_select(int b, int n, int c, const float *points, const int *draws, double r2, int knn_k,
                             int nsample, int *members, int *counts, void *stream);
APN_API int apn_rsmix_mix(int b, int n, int c, int nsample, const float *points, const int *draws, const int *members,
                          const int *counts, const int *pick, float *out, float *lam, void *stream);

/* The ScanObjectNN dataset transforms of a batch (openpoints/dataset/scanobjectnn/scanobjectnn.py:79-97 with the cfg
 * chain PointCloudScaling -> PointCloudCenterAndNormalize -> PointCloudRotation), one workgroup per cloud:
 *   source raw[rows[c], :n] ((s, n_raw, 3) float32, never written; rows NULL: raw[c, :n]), n <= 8192 and n <= n_raw;
 *   a row outside [0, s) gives a NaN cloud.  Stages by `flags` (APN_CT_*): permute src[perm[i]], scale, heights on
 *   axis gravity_dim (of the scaled points with APN_CT_HEIGHTS_SCALED, else the unscaled ones), centre, normalise by
 *   the largest norm, rotate p @ R^T.  -> out (b, n, 4) = [pos, heights].
 * Host draws: perm (b, n) int32, params (b, 12) float32 = scale (3) | R row-major (9).
 * Device draws (APN_CT_UNIFORM): uniforms = b*10 per-cloud U[0,1) numbers (scale 3 | mirror 3 | angle 3 | axis order 1)
 *   followed by b*n per-point ones, whose sorted order is the permutation; cfg (double, 11) = scale_lo, scale_hi,
 *   mirror (3), scale_xyz (3, 0 = off), angle bounds in radians (3, NaN = None).  perm / params are then unused.
 * perm_out (b, n) int32 and params_out (b, 12), either may be NULL: the permutation and parameters used. */
#define APN_CT_PERMUTE 1
#define APN_CT_SCALE 2
#define APN_CT_HEIGHTS_SCALED 4
#define APN_CT_CENTER 8
#define APN_CT_NORMALIZE 16
#define APN_CT_ROTATE 32
#define APN_CT_UNIFORM 64
#define APN_CT_ANISOTROPIC 128
#define APN_CT_MIRROR 256
APN_API int apn_cloud_transform(int b, int n, int n_raw, int s, const float *raw, const int *rows, int flags,
                                int gravity_dim, const double *cfg, const int *perm, const float *params,
                                const float *uniforms, int *perm_out, float *params_out, float *out, void *stream);

/* The classification metric of an evaluation batch (openpoints/utils/metrics.py:62-73 fed `logits.argmax(dim=1)`), one
 * launch, no host read:
 *   logits (b, k) float32 with row stride ld >= k; target (b,) int32; valid: a device int32 scalar -- only rows
 *   r < clamp(*valid, 0, b) are counted (NULL: all b), so one captured graph also serves a padded last batch.
 *   pred (b,) int32, may be NULL: the argmax of EVERY row, padding rows included, by torch.argmax's rule (the first
 *   index of the maximum; a NaN beats every number and the first NaN wins; an all -inf row gives 0).
 *   cm: k*k + 1 counters, added to and never cleared: cell t*k + p for target t and prediction p (torch.bincount's
 *   layout); the last cell counts counted rows whose target lies outside [0, k).
 * The one exception to this header's int32 / float32 contract: cm holds unsigned 64-bit counts, as bincount's are.
 * Integer atomics: exact and the same on every run. */
APN_API int apn_cls_confusion(int b, int k, const float *logits, int ld, const int *target, const int *valid,
                              unsigned long long *cm, int *pred, void *stream);

/* The part-segmentation metric of an evaluation batch (examples/shapenetpart/train_adapt.py: get_ins_mious :77-107 fed
 * `logits.max(dim=1)[1]`, and validate's accumulation :576-582), two launches, no host read (csrc/part_metrics.hip):
 *   logits (b, c, n) float32, c <= 64 part labels; target (b, n) int32; cls (b,) int32 in [0, s);
 *   part_offset (s + 1) / part_ids (nparts) int32: category k's parts are part_ids[part_offset[k] .. part_offset[k+1]),
 *   in the order the mean runs over them; valid (b,) int32 or NULL: shapes with valid[i] == 0 are padding.
 *   Prediction: the first channel of the maximum; a NaN beats every number and the first NaN wins (torch's max).
 *   ious (b,) float32, written: the shape's mean over its category's parts of float32(100 I) / float32(U), 100 where
 *   U == 0; a predicted or target label outside the category's list is in no part; -1 for padding; -2 for a REJECTED
 *   shape (class outside [0, s), CSR range empty, longer than 64 or outside [0, nparts], part id outside [0, c)).
 *   cls_sum (s) float32, cls_num (s) int32, ins_sum (1) float64, ins_num (1) int32, rejected (1) int32 (may be NULL):
 *   added to in ascending shape order and never cleared, so the totals do not depend on the split into batches.
 * Integer LDS atomics and fixed-order sums only: the same bits on every run.
 * c outside [1, 64], s < 1, nparts < 1, a negative size or a missing pointer -> APN_EINVAL; b == 0 -> APN_OK. */
APN_API int apn_part_ious(int b, int c, int n, int s, int nparts, const float *logits, const int *target, const int *cls,
                          const int *part_offset, const int *part_ids, const int *valid, float *ious, float *cls_sum,
                          int *cls_num, double *ins_sum, int *ins_num, int *rejected, void *stream);

/* Scene segmentation's per-point work outside the network (csrc/scene_seg.hip; the reference's
 * examples/segmentation/main.py and crop_pc of openpoints/dataset/data_util.py).  No host read in any entry, no float
 * atomics, integer atomics only where their order cannot matter: the same bits on every run.  Every index read from a
 * tensor is range-checked before it addresses anything.  c <= apn_ss_max_classes() = 64 wherever counters are kept.
 *
 * Counters `cm`: c*c + 1 unsigned 64-bit cells, added to and never cleared: cell t*c + p for target t and prediction p;
 *   a target equal to ignore_index (when has_ignore != 0) is skipped; any other target outside [0, c) adds to the last
 *   cell.  Predictions follow torch.argmax: the first channel of the maximum, a NaN beats every number.
 *
 * apn_ss_confusion: logits (b, c, n) float32 contiguous, target (b, n) int32, valid a device int32 scalar or NULL
 *   (clouds at or beyond clamp(*valid, 0, b) are not counted), pred (b, n) int32 or NULL (written for every cloud).
 * apn_ss_votes_add: one sub-cloud's logits (c, n_part) and rows idx (n_part): acc[idx[j], :] += logits[:, j] (acc (n, c)
 *   float32), cnt[idx[j]] += 1, by plain loads and stores; `call` >= 1 numbers the calls of one scene, stamp (n) int32
 *   starts at 0.  A row that occurs twice in one call is added once and counted in flags[0]; a row outside [0, n) is
 *   skipped and counted in flags[1].  A point's sum is the sequence of fp32 adds in call order.
 * apn_ss_votes_finish: mean (n, c) = acc / max(cnt, 1) (one correctly rounded division), pred (n) its argmax, both may
 *   be NULL; with labels (n) int32 the counters are added to.
 * apn_ss_project: logits (c, m) per voxel column, slot (m): voxel v's column, voxel_of (n): pred_voxel (m, scratch,
 *   written) = argmax of column slot[v], pred (n, may be NULL) = pred_voxel[voxel_of[i]], counters against labels (n, may
 *   be NULL).  A slot or voxel outside [0, m) is counted in flags[1]; its points get pred -1 and no count.
 * apn_ss_crop_nearest: coord (n, 3) float32, offset (b) int32 cumulative ends, centre (b) int32 a row inside each cloud:
 *   idx (b, k) int32 = the global rows of the k nearest rows of the centre in ascending row, the set
 *   argsort(d, stable)[:k] for d = (dx*dx + dy*dy) + dz*dz rounded after every operation.  stats[0] counts rows with a
 *   non-finite coordinate, stats[1] clouds that were refused and left unwritten (bad offsets, centre outside the cloud,
 *   fewer than k rows).  One workgroup per cloud.
 * A size outside its range or a missing pointer -> APN_EINVAL before any launch; empty work -> APN_OK. */
APN_API int apn_ss_max_classes(void);
APN_API int apn_ss_confusion(int b, int c, int n, const float *logits, const int *target, int ignore_index,
                             int has_ignore, const int *valid, unsigned long long *cm, int *pred, void *stream);
APN_API int apn_ss_votes_add(int n, int c, int n_part, const float *logits, const int *idx, int call, float *acc,
                             int *cnt, int *stamp, int *flags, void *stream);
APN_API int apn_ss_votes_finish(int n, int c, const float *acc, const int *cnt, const int *labels, int ignore_index,
                                int has_ignore, unsigned long long *cm, float *mean, int *pred, void *stream);
APN_API int apn_ss_project(int c, int m, int n, const float *logits, const int *slot, const int *voxel_of,
                           const int *labels, int ignore_index, int has_ignore, int *pred_voxel,
                           unsigned long long *cm, int *pred, int *flags, void *stream);
APN_API int apn_ss_crop_nearest(int b, int n, int k, const float *coord, const int *offset, const int *centre,
                                int *idx, int *stats, void *stream);

/* The last layer of the discriminator's group-all stage with its pooling
 * (openpoints/models_adaptpoint/point_discriminator.py:183-189: conv -> ReLU -> max over the cloud's points), fused:
 *   out (B,c_out) = [relu](max_n (w x_b)[o][n] + bias[o]),  idx (B,c_out) int32 = the position of that maximum (the
 *   lowest one among equals); the (B,c_out,N) activation is never written.  bias may be NULL.  Scratch: tile_val /
 *   tile_idx [b][apn_pw_conv_max_tiles(n)][c_out].
 * Backward (c_in <= 128): every (b, o) passes its gradient to position idx[b][o] alone -- g_x (B,c_in,N) (fully
 *   written; may be NULL), g_w (c_out,c_in), g_bias [c_out] (may be NULL); xsel = scratch (B,c_out,c_in).  No
 *   atomics: fixed orders, bit-reproducible. */
APN_API int apn_pw_conv_max_tiles(int n);
APN_API int apn_pw_conv_max_forward(int b, int c_in, int c_out, int n, int precision, const float *x, const float *w,
                                    const float *bias, int relu, float *tile_val, int *tile_idx, float *out, int *idx,
                                    void *stream);
APN_API int apn_pw_conv_max_backward(int b, int c_in, int c_out, int n, const float *g_out, const float *out,
                                     const int *idx, const float *x, const float *w, int relu, float *xsel, float *g_x,
                                     float *g_w, float *g_bias, void *stream);

/* ------------------------------------------------------------------------
 * spectral normalisation, the parametrisation of every layer of PointDiscriminator1
 * (openpoints/models_adaptpoint/point_discriminator.py:17-73, 149-191: torch.nn.utils.spectral_norm, which the
 * reference evaluates as ~13 small PyTorch launches per training-mode forward and ~7 per backward).
 *   w (rows x cols) the weight as a matrix; u [rows], v [cols] the module's power-iteration buffers.
 * spectral_norm (3 launches; 2 when !training): training: one power iteration u = normalize(w v),
 *   v = normalize(w^T u) written INTO u, v; sigma[0] = u^T w v; w_normalized = w / sigma; u_used / v_used = the
 *   vectors sigma was formed with (kept for the backward, as PyTorch clones them); scratch [rows + cols] floats.
 * spectral_norm_grad (2 launches): g_w = g / sigma - (sum(g o w_normalized) / sigma) u_used v_used^T;
 *   part = scratch of apn_spectral_norm_blocks(rows, cols) doubles.  Fixed summation orders: reproducible. */
APN_API int apn_spectral_norm_blocks(int rows, int cols);
APN_API int apn_spectral_norm(int rows, int cols, const float *w, int training, float eps, float *u, float *v,
                              float *scratch, float *u_used, float *v_used, float *sigma, float *w_normalized,
                              void *stream);
APN_API int apn_spectral_norm_grad(int rows, int cols, const float *g, const float *w_normalized, const float *sigma,
                                   const float *u_used, const float *v_used, double *part, float *g_w, void *stream);

/* The same for ALL layers of a network in one set of launches (3 forward, 2 backward; the layer rides on blockIdx.y): arrays
 * of n_layers (<= 8) entries with the meaning of the arguments above; scratch[i]: rows[i] + cols[i] floats; part[i]:
 * apn_spectral_norm_blocks(rows[i], cols[i]) doubles.  (PointDiscriminator1 holds seven spectral-normalised layers and is
 * evaluated three times per train_gan iteration, point_discriminator.py:17-73, train_autoaug.py:150-196.) */
APN_API int apn_spectral_norm_many(int n_layers, const int *rows, const int *cols, const float *const *w, int training,
                                   float eps, float *const *u, float *const *v, float *const *scratch,
                                   float *const *u_used, float *const *v_used, float *const *sigma,
                                   float *const *w_normalized, void *stream);
APN_API int apn_spectral_norm_grad_many(int n_layers, const int *rows, const int *cols, const float *const *g,
                                        const float *const *w_normalized, const float *const *sigma,
                                        const float *const *u_used, const float *const *v_used, double *const *part,
                                        float *const *g_w, void *stream);

/* LocalAggregation with one grouped convolution (InvResMLP's aggregation, pointnext.py:27-78, 246), the feature part of
 * the convolution hoisted to the points: U (b,n,c) = Wf f, y[q,k] = U[idx[q,k]] + Wp (xyz[idx[q,k]] - xyz[q]) / radius
 * (csrc/local_aggr.hip).  c in {64, 128, 256, 512}, nsample = 32, idx (b,n,32) a ball query of xyz (b,n,3) around itself,
 * wp: the convolution's coordinate columns (c rows of stride ldw).
 *   pool_fwd: ext (b,n,c) = ext_k y[q,k] (max where gamma >= 0, min elsewhere; gamma NULL: max), sel (b,n,c) uint8 = the
 *     slot that holds it; training (ysum and part both given): ysum (b,n,c) = sum_k y[q,k] and
 *     part[apn_la_pool_rows(b, n)][2c] (float64) = the workgroups' shares of {sum y, sum y^2} over the b*n*32 positions.
 *   stats_fold: sums[2c + 2] (float64) = {the shares added in the shared order at 4 lanes ("Partial-row folds", above),
 *     count, 1}: apn_sa_bn_fold's `sums`.  rows == 0 returns before it writes.
 *   pool_bwd: gsel (b,n,c) = the gradient at the selected positions (apn_sa_wide_bwd_prep's goa), de = {D[c], E[c]}
 *     (apn_sa_wide_consts2: BatchNorm's dense term dL/dy = D y + E), tmap / pcnt_poff / plist / geo: the NeighbourIndex
 *     of idx (apn_sa_wide_tilemap, apn_sa_wide_csr) -> dU (b,n,c) = dL/dU summed per point in a fixed order (no float
 *     atomics), dT (b,n,c) = dU - sum_k dL/dy[n,k] (dL/dWp = dT^T xyz / radius) and (dp given) dp (b,n,3) =
 *     dT wp / radius.  ysum NULL: eval mode (D = E = 0).
 * Indices outside [0, n): pool_fwd brings every idx into its cloud before it follows it (below 0 -> 0, n and above ->
 * n - 1); the index stage does NOT (apn_sa_wide_tilemap, apn_sa_wide_csr), so pool_bwd's maps must come from an idx
 * that lies in [0, n) throughout. */
APN_API int apn_la_pool_rows(int b, int n);
APN_API int apn_la_pool_fwd(int b, int n, int c, int nsample, float radius, const float *U, const float *xyz,
                            const float *wp, int ldw, const int *idx, const float *gamma, float *ext, void *sel,
                            float *ysum, double *part, void *stream);
APN_API int apn_la_stats_fold(const double *part, int rows, int c, double count, double *sums, void *stream);
APN_API int apn_la_pool_bwd(int b, int n, int c, int nsample, float radius, const float *gsel, const void *sel,
                            const int *tmap, const int *pcnt_poff, const int *plist, const float *geo, const float *U,
                            const float *xyz, const float *ysum, const float *de, const float *wp, int ldw, float *dU,
                            float *dT, float *dp, void *stream);

/* Exact brute-force k nearest neighbours of c-dimensional rows (csrc/knn.hip): for every query (b,m,c) the k supports
 * (b,n,c) with the smallest key (d2, support index), ascending -- ties go to the smaller index --, where
 * d2 = sum_c (q_c - s_c)^2 in fp32 by direct differences, a_0 = t_0 t_0, a_c = fma(t_c, t_c, a_{c-1}) over ascending c.
 * idx (b,m,k) int32, dist2 (b,m,k) or NULL; query may alias support.  1 <= k <= 64, k <= n, 1 <= c <= 128, b <= 65535,
 * b * max(n, m) < 2^24, non-null pointers: APN_EINVAL otherwise, before any HIP call; b == 0 or m == 0 is a no-op.
 * One launch: no synchronisation, memset or allocation.  Inputs are assumed finite. */
APN_API int apn_knn_query(int b, int n, int m, int c, int k, const float *support, const float *query, int *idx,
                          float *dist2, void *stream);

/* apn_knn_query to rank 256 with only the wanted ranks written (the same kernel of csrc/knn.hip, ceil(kd / 64) list
 * registers per lane; apn_knn_query is kd = k, dilation 1): the graph of a DeepGCN block.  With L the query's kd
 * smallest keys (d2, support index) in ascending order, idx[b,q,j] = L[slots[j]].index for a device table slots int32[k] (an entry outside [0, kd) is
 * clamped into it: nothing is read out of bounds whatever the table holds), or L[j * dilation].index with slots NULL;
 * dist2 (b,m,k) or NULL carries the matching distances.  1 <= kd <= 256, kd <= n, 1 <= k <= 64, k <= kd, with slots NULL
 * dilation >= 1 and (k - 1) dilation < kd, 1 <= c <= 128, b <= 65535, b * max(n, m) < 2^24, non-null pointers:
 * APN_EINVAL otherwise, before any HIP call; b == 0 or m == 0 is a no-op.  One launch: no synchronisation, memset,
 * allocation, global scratch or atomics; the result is a function of the inputs alone. */
APN_API int apn_knn_dilated(int b, int n, int m, int c, int kd, int k, int dilation, const int *slots,
                            const float *support, const float *query, int *idx, float *dist2, void *stream);

/* DGCNN's EdgeConv block, out = act(bn(max_k W [x_i ; x_j - x_i])) with W = [Wa | Wb] and act = LeakyReLU(slope), the
 * convolution hoisted to the points (csrc/edge_conv.hip): uv (b,n) rows [u (c) | v (c)] of pitch ld >= 2c (ld % 4 == 0),
 * u = (Wa - Wb) x, v = Wb x, y[i,k] = u_i + v_idx[i,k].  c in {64, 128, 256, 512}, idx (b,n,k) with 1 <= k <= 64 (indices
 * outside the cloud are clamped into it), b <= 65535, b * n < 2^24; APN_EINVAL otherwise, before any launch; b == 0 or
 * n == 0 is a no-op.  No entry synchronises, allocates or issues a memset.
 *   pool_fwd: ext (b,n,c) = ext_k y[i,k] (max where gamma >= 0, min elsewhere; gamma NULL: max), sel (b,n,c) uint8 = the
 *     first slot that holds it; training (ysum and part both given): ysum (b,n,c) = sum_k y[i,k] and
 *     part[apn_ec_pool_rows(b, n)][2c] (float64) = the workgroups' shares of {sum y, sum y^2} over the b*n*k positions
 *     (repeated neighbours count once per occurrence); apn_la_stats_fold adds them for apn_sa_bn_fold.
 *   out: out (b,c,n) = act(scale ext + shift), pack = apn_sa_bn_fold's; slope > 0.
 *   bwd_prep: g (b,c,n; element strides gs_*) -> gsel (b,n,c) = g act' scale and part_s[apn_ec_bwd_prep_rows(b, n)][2c] =
 *     {sum g act', sum g act' yhat_sel}: apn_sa_wide_consts2's rows.
 *   csr: the reverse neighbours of idx: pcnt_poff = {pcnt[b n], poff[b n]}, plist[b n k] = the positions (b n + i) k + slot
 *     that gather each point, ascending -- a pure function of idx; scratch: b n (k + 1) ints.
 *   pool_bwd: de = {D[c], E[c]} (apn_sa_wide_consts2: BatchNorm's dense term dL/dy = D y + E) -> duv (b,n) rows
 *     [du | dv] of pitch 2c, du_i = gsel_i + D ysum_i + k E, dv_j = sum over j's list {gsel_i [slot == sel_i]} +
 *     D (sum over j's list u_i + pcnt_j v_j) + pcnt_j E, summed in list order (no float atomics).  ysum NULL: eval mode. */
APN_API int apn_ec_pool_rows(int b, int n);
APN_API int apn_ec_pool_fwd(int b, int n, int c, int k, const float *uv, int ld, const int *idx, const float *gamma,
                            float *ext, void *sel, float *ysum, double *part, void *stream);
APN_API int apn_ec_out(int b, int n, int c, const float *ext, const float *pack, float slope, float *out, void *stream);
APN_API int apn_ec_bwd_prep_rows(int b, int n);
APN_API int apn_ec_bwd_prep(int b, int n, int c, const float *g, long long gs_b, long long gs_c, long long gs_n,
                            const float *ext, const float *pack, float slope, float *gsel, float *part_s, void *stream);
/* The two entries above with slope >= 0 (0 is ReLU; negative and NaN: APN_EINVAL): the same two launches, which
 * adaptpoint_amd.edge_conv takes for every block (apn_ec_out and apn_ec_bwd_prep only add the refusal of slope == 0).
 *   out_res: out = act(scale ext + shift) + res, res (b,c,n) with element strides rs_*, or NULL for no residual.
 *   bwd_prep_act: apn_ec_bwd_prep; act' is recomputed from ext and pack, so the residual (gradient: g) needs nothing. */
APN_API int apn_ec_out_res(int b, int n, int c, const float *ext, const float *pack, float slope, const float *res,
                           long long rs_b, long long rs_c, long long rs_n, float *out, void *stream);
APN_API int apn_ec_bwd_prep_act(int b, int n, int c, const float *g, long long gs_b, long long gs_c, long long gs_n,
                                const float *ext, const float *pack, float slope, float *gsel, float *part_s,
                                void *stream);
APN_API int apn_ec_csr(int b, int n, int k, const int *idx, int *pcnt_poff, int *plist, int *scratch, void *stream);
APN_API int apn_ec_pool_bwd(int b, int n, int c, int k, const float *gsel, const void *sel, const int *pcnt_poff,
                            const int *plist, const float *uv, int ld, const float *ysum, const float *de, float *duv,
                            void *stream);

/* Chamfer distance between the clouds xyz1 (b,n,3) and xyz2 (b,m,3), the reference's `chamfer` module
 * (csrc/chamfer.hip); dist1 / idx1 / grad_dist1 are (b,n), dist2 / idx2 / grad_dist2 (b,m), everything contiguous.
 *   forward: dist1[b,i] = min_j d(xyz1[b,i], xyz2[b,j]) and idx1[b,i] = the SMALLEST j that attains it (strict `<` over
 *     ascending j, as the reference's kernel decides), with d = fma(tz, tz, fma(ty, ty, tx * tx)), t = xyz2_j - xyz1_i, in
 *     fp32: apn_knn_query's form at c = 3 (the library is built with -ffp-contract=off: this is the only fma).  dist2 /
 *     idx2: the same with the clouds' roles swapped.  Inputs are assumed finite.
 *   backward: for every i, per component, in fp32 with separately rounded operations in exactly this order:
 *         acc = (grad_dist1[i] * 2) * (xyz1[i] - xyz2[idx1[i]])
 *         for j ascending with idx2[j] == i:   acc = acc - (grad_dist2[j] * 2) * (xyz2[j] - xyz1[i])
 *         grad_xyz1[i] = acc
 *     and grad_xyz2 symmetrically.  Every output element is written (nothing has to arrive zeroed); there is no float
 *     atomic, the result is a pure function of the inputs; indices outside the other cloud are clamped into it.
 * 1 <= n, m <= apn_chamfer_max_points() = 65536, b * max(n, m) < 2^24 (no limit on b beyond that: the grids are flat),
 * non-null pointers: APN_EINVAL otherwise, before any HIP call; b == 0 is a no-op.  One launch per entry for both
 * directions: no synchronisation, allocation, memset or global scratch. */
APN_API int apn_chamfer_max_points(void);
APN_API int apn_chamfer_forward(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1, float *dist2,
                                int *idx1, int *idx2, void *stream);
APN_API int apn_chamfer_backward(int b, int n, int m, const float *xyz1, const float *xyz2, const int *idx1,
                                 const int *idx2, const float *grad_dist1, const float *grad_dist2, float *grad_xyz1,
                                 float *grad_xyz2, void *stream);

/* Earth mover's distance (approximate, by annealed soft matching) between the clouds xyz1 (b,n,3) and xyz2 (b,m,3), the
 * reference's `emd_cuda` module (csrc/emd.hip); everything fp32 and contiguous.  The reference's `match` (b,m,n) is a sum
 * over ten levels q = 0..9 (its j = 7 .. -2) of rank-structured weights, so two small tables determine it:
 *         match[l,k] = sum over q ascending, from 0, of (e_q(d[l,k]) * ratio_l[q,k]) * ratio_r[q,l]
 *   d[l,k] = fma(tz, tz, fma(ty, ty, tx * tx)), t = xyz2_l - xyz1_k (apn_knn_query's form at c = 3: the only fma),
 *   level_q = -4^(7-q) for q < 9 and 0 for q = 9,    e_q(d) = exp2(level_q * (d * log2(e)f)), every operation rounded to
 *   fp32 (a level is a power of two or 0, so its product is exact: d * log2(e) is rounded once per pair) and exp2 the
 *   hardware's v_exp_f32 (1 ulp; results below 2^-126 are 0).  ONE device function is e_q for every kernel.
 *   ratios: writes ratio_l (b,10,n) and ratio_r (b,10,m).  With multiL, multiR = (1, n / m) if n >= m else (m / n, 1) by
 *     C INTEGER division ((7,3): multiR = 2), remainL_k = multiL and remainR_l = multiR at the start, per level q:
 *         ratio_l[q,k] = remainL_k / (1e-9f + sum_l e_q * remainR_l)
 *         sumr_l = (sum_k e_q * ratio_l[q,k]) * remainR_l
 *         ratio_r[q,l] = min(remainR_l / (sumr_l + 1e-9f), 1) * remainR_l;       remainR_l = max(0, remainR_l - sumr_l)
 *         remainL_k = max(0, remainL_k - sum_l (e_q * ratio_l[q,k]) * ratio_r[q,l])
 *     The sums run in an order fixed by (n, m) alone -- max(n, m) <= apn_emd_one_launch_max(): one workgroup per cloud,
 *     one launch, every sum in ascending index; beyond it 20 launches whose workgroups own 64 rows each, the sum of a
 *     row being p_0 + p_1 + .. + p_(W-1) added in this order, W = 8 if max(n, m) >= 256 else 4, with p_w the ascending
 *     sum over wave w's columns: the columns go by in chunks of 1024 (the last chunk has c of them), and of every chunk
 *     wave w takes columns r w .. r (w + 1) - 1, r = 4 ceil(ceil(c / 4) / W) -- without float atomics: two runs give the
 *     same bits.  `state` is scratch of b (n + m) floats (the remainders between the launches of the second form); it
 *     and the outputs may arrive uninitialised.
 *   match: writes every element of match (b,m,n) once, by the formula above (64-bit element offsets).
 *   cost:  cost[b] = sum_{k,l} d[l,k] * match[l,k].  grad: with g = grad_cost[b],
 *         grad1[k] = g * sum_l (xyz1_k - xyz2_l) * (2 * match[l,k]),  grad2[l] = g * sum_k (xyz2_l - xyz1_k) * (2 * match[l,k])
 *     (match is a constant).  Both take EITHER `match` OR, with match == NULL, the two tables, from which every match[l,k]
 *     is recomputed by the device function apn_emd_match runs: the two sources go through one template and give the
 *     same bits.  Row sums are ordered as in the second form above; a cloud's cost is the ascending sum over k inside a
 *     64-row tile, then the ascending sum over the tiles (`part`: scratch of b * apn_emd_cost_parts(n) floats).  Every
 *     output element is written; no float atomics.
 * 1 <= n, m <= apn_emd_max_points() = 8192, b * max(n, m) < 2^24, non-null pointers (match and the tables as stated):
 * APN_EINVAL otherwise, before any HIP call; b == 0 is a no-op.  No entry allocates, memsets or synchronises. */
APN_API int apn_emd_max_points(void);
APN_API int apn_emd_one_launch_max(void);
APN_API int apn_emd_cost_parts(int n);
APN_API int apn_emd_ratios(int b, int n, int m, const float *xyz1, const float *xyz2, float *ratio_l, float *ratio_r,
                           float *state, void *stream);
APN_API int apn_emd_match(int b, int n, int m, const float *xyz1, const float *xyz2, const float *ratio_l,
                          const float *ratio_r, float *match, void *stream);
APN_API int apn_emd_cost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                         const float *ratio_l, const float *ratio_r, float *part, float *cost, void *stream);
APN_API int apn_emd_cost_grad(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2,
                              const float *match, const float *ratio_l, const float *ratio_r, float *grad1, float *grad2,
                              void *stream);

/* Operators on STACKED clouds, the reference's `pointops_cuda` module (csrc/pointops.hip; the reverse lists: csrc/
 * edge_conv.hip): points xyz (n,3), features (n,c), int32 offset (b) of cumulative END rows (ascending, offset[b-1] == n),
 * so that every cloud has its own size; queries new_xyz (m,3) with their own new_offset (b), new_offset[b-1] == m.
 * Everything is fp32 / int32 and contiguous; element offsets are 64-bit inside the kernels (the reference's int products
 * overflow at n * nsample * c >= 2^31).  Query row q belongs to the first cloud i with q < new_offset[i]; a row at or past
 * new_offset[b-1] is treated as belonging to the last cloud (the reference's search runs off the array there).  A cloud's
 * rows [start, end) are clamped into [0, n].  Any index read from `idx` is clamped into [0, n).  Squared distances are
 *         d2 = fma(tz, tz, fma(ty, ty, tx * tx)),  t = q - s      (apn_knn_query's form at c = 3: the only fma)
 * No entry synchronises, allocates, issues a memset or reads offsets on the host; no float atomics: every result is a
 * pure function of the inputs, two runs give the same bits.  Every output element is written except where stated.
 *   knn_query: idx, dist2 (m,k): for every query the k rows OF ITS OWN CLOUD with the smallest key (d2, global row index)
 *     in ascending key order, 1 <= k <= 100 (the reference's array bound); new_xyz may alias xyz.  A cloud with fewer
 *     than k rows (or rows at d2 >= 1e10) leaves the remaining slots at idx = start of the cloud (clamped into [0, n)),
 *     dist2 = 1e10: the reference's initial heap, which its sqrt turns into 1e5 -- a kept quirk.  The reference's heap
 *     orders EQUAL distances by its sift history, this entry by index: the two agree wherever the k + 1 nearest distances
 *     of a query are distinct.  One launch, no scratch.
 *   ball_query: idx (m,nsample): the first nsample rows of the query's cloud in ascending index with d2 < radius * radius
 *     (strict, the product rounded to fp32); the remaining slots repeat the first hit; a query without a hit writes zeros
 *     (what the reference's pre-zeroed, unwritten row holds).  radius >= 0, nsample >= 1.
 *   furthest_sampling: per cloud with output rows [start_m, end_m) of idx: idx[start_m] = start; every later pick is the
 *     arg-max of the running minimum distance min(d2 to the last pick, tmp[k]); tmp (n) is in/out and arrives filled with
 *     1e10, as in the reference.  Ties, exactly the reference's: with T = min(1024, 2^floor(log2 n_max)), row k belongs to
 *     thread (k - start) mod T, a thread keeps its first maximum and the block tree the lower slot unless the upper one is
 *     strictly greater -- the winner is the maximum with the smallest bit-reversed (over log2 T bits) thread id, then
 *     the smallest k.  n_max is the largest cloud size (rows of a cloud beyond 24 * 1024 make the kernel stream from
 *     memory; a cloud larger than n_max claims is sampled from its first max(n_max, 24 T) rows only).  A cloud with an
 *     empty output range writes NOTHING: the reference writes idx[start_m] regardless, into the next cloud's slot -- a
 *     dropped quirk.  The offsets are trusted (the entry is given neither n nor m).  n_max < 2^24; b == 0 or n_max == 0
 *     is a no-op.
 *   csr: the reverse lists of idx (m,k) into n rows: pcnt_poff = {pcnt (n), poff (n)}, plist (m k) with row j's list
 *     plist[poff[j] .. poff[j] + pcnt[j]) = the positions i * k + slot whose (clamped) index is j, ASCENDING.  A pure
 *     function of idx (integer atomics count; the lists are sorted afterwards).  scratch: n + m k ints.  m k < 2^31.
 *     m == 0 gives n empty lists.
 *   grouping: fwd out (m,k,c) = input[idx[i,s]] (n,c).  bwd grad_input[j] = the sum over j's list, in list order, of
 *     grad_out[pos]: sequential fp32 adds STARTING FROM THE FIRST TERM (as every sum below; an empty list gives 0).
 *   interpolation: fwd out[i,ch] = sum over slots ascending of input[idx[i,s],ch] * weight[i,s], each product rounded,
 *     then added.  bwd grad_input[j,ch] = sum over j's list of grad_out[pos / k, ch] * weight[pos].
 *   subtraction: fwd out[i,s,ch] = input1[i,ch] - input2[idx[i,s],ch], input1 (m,c), input2 (n,c).  bwd grad_input1[i,ch]
 *     = sum over slots ascending of g[i,s,ch]; grad_input2[j,ch] = sum over j's list of -g[pos,ch].
 *   aggregation: c % w_c == 0, w = ch % w_c; input (n,c), position (m,k,c), weight (m,k,w_c).  fwd out[i,ch] = sum over
 *     slots ascending of (input[idx[i,s],ch] + position[i,s,ch]) * weight[i,s,w]: three separately rounded operations per
 *     term.  bwd grad_position[i,s,ch] = g[i,ch] * weight[i,s,w]; grad_weight[i,s,w] = sum over the c / w_c channels with
 *     ch % w_c == w, ascending ch, of g[i,ch] * (input[idx[i,s],ch] + position[i,s,ch]); grad_input[j,ch] = sum over j's
 *     list of g[pos / k, ch] * weight[pos, w].
 * 0 <= n, m < 2^24, b >= 1 (knn, ball), k >= 1, 1 <= c <= 65536, m k < 2^31, non-null pointers: APN_EINVAL otherwise,
 * before any HIP call.  n == 0 or m == 0 is a no-op, except that the backward entries and csr with n > 0 and m == 0
 * write the zeros / empty lists that no query leaves behind. */
APN_API int apn_po_knn_query(int b, int n, int m, int k, const float *xyz, const float *new_xyz, const int *offset,
                             const int *new_offset, int *idx, float *dist2, void *stream);
APN_API int apn_po_ball_query(int b, int n, int m, float radius, int nsample, const float *xyz, const float *new_xyz,
                              const int *offset, const int *new_offset, int *idx, void *stream);
APN_API int apn_po_furthest_sampling(int b, int n_max, const float *xyz, const int *offset, const int *new_offset,
                                     float *tmp, int *idx, void *stream);
APN_API int apn_po_csr(int n, int m, int k, const int *idx, int *pcnt_poff, int *plist, int *scratch, void *stream);
APN_API int apn_po_grouping_fwd(int n, int m, int k, int c, const float *input, const int *idx, float *out, void *stream);
APN_API int apn_po_grouping_bwd(int n, int m, int k, int c, const float *grad_out, const int *pcnt_poff, const int *plist,
                                float *grad_input, void *stream);
APN_API int apn_po_interpolation_fwd(int n, int m, int k, int c, const float *input, const int *idx, const float *weight,
                                     float *out, void *stream);
APN_API int apn_po_interpolation_bwd(int n, int m, int k, int c, const float *grad_out, const float *weight,
                                     const int *pcnt_poff, const int *plist, float *grad_input, void *stream);
APN_API int apn_po_subtraction_fwd(int n, int m, int k, int c, const float *input1, const float *input2, const int *idx,
                                   float *out, void *stream);
APN_API int apn_po_subtraction_bwd(int n, int m, int k, int c, const float *grad_out, const int *pcnt_poff,
                                   const int *plist, float *grad_input1, float *grad_input2, void *stream);
APN_API int apn_po_aggregation_fwd(int n, int m, int k, int c, int w_c, const float *input, const float *position,
                                   const float *weight, const int *idx, float *out, void *stream);
APN_API int apn_po_aggregation_bwd(int n, int m, int k, int c, int w_c, const float *input, const float *position,
                                   const float *weight, const int *idx, const float *grad_out, const int *pcnt_poff,
                                   const int *plist, float *grad_input, float *grad_position, float *grad_weight,
                                   void *stream);

/* Point Transformer's vector-attention layer behind its q/k/v projection (openpoints/models/backbone/
 * pointtransformer.py: PointTransformerLayer; csrc/point_transformer.hip).  n stacked rows, k = nsample slots, c channels,
 * c' = c / 8 attention weights; j = idx[i,s] (n,k) int32, an index outside [0, n) is clamped into it.
 *   qkv (n rows of pitch ld >= 3c) = [q (c) | k (c) | v (c)], h (n,k,3) = the positional hidden layer,
 *   wts = W2 (c,3) | b2 (c) | W3^T (c,c') | b3 (c') | W4 (c',c') | b4 (c'),
 *   bn  = sc1 (c) | sh1 (c) | sc2 (c') | sh2 (c'): the two BatchNorms folded to scale / shift,
 *   de  = D1 (c) | E1 (c) | D2 (c') | E2 (c'): BatchNorm's dense backward term dL/dx = sc g + D x + E (zeros in eval).
 *      pr = W2 h + b2 = fma(W2[c,2], h2, fma(W2[c,1], h1, fma(W2[c,0], h0, b2[c])))        r = (k_j - q_i) + pr
 *      y  = relu(fma(sc1, r, sh1))      t = b3 + sum_c W3[c',c] y[c] (fma, ascending c)     z = relu(fma(sc2, t, sh2))
 *      l  = b4 + sum_e W4[c',e] z[e]    a = exp(l - max_s l) / sum_s exp(l - max_s l)
 *      out[i,c] = sum over slots ascending of (v_j[c] + pr[c]) * a[i,s,c mod c']
 * Forward:
 *   rows: how many partial rows (workgroups) the strided kernels write: apn_pt_rows(n, k, c) = ceil(n k / 64), at most
 *     2048 (c <= 64), 1024 (c = 128), 256 (c = 256) or 128 (c = 512); 0 for n == 0 or refused arguments.
 *   rel_stats: part[rows][2c] (float64) = the workgroups' shares of {sum r, sum r^2} over the n k positions.
 *   fold: sums[width] (float64) = the rows of part[rows][width] added in the shared order at 16 lanes ("Partial-row
 *     folds", above); rows <= 2048, width <= 2^20.
 *   mid: t (n,k,c'); part given: part[apn_pt_mid_rows(n, k, c)][2c'] (float64) = the shares of {sum t, sum t^2}, one row per
 *     workgroup: a workgroup per tile of 8192 / c positions, at most apn_pt_rows(n, k, c).
 *   attend: a (n,k,c') and out (n,c).
 *   colsum: part[apn_pt_colsum_rows(n)][width] (float64) = the workgroups' shares of the column sums of src (n rows of
 *     pitch ld >= width, 1 <= width <= 1536), each the rows r, r + rows, ... in ascending order; apn_pt_fold adds them: the
 *     bias gradient of the q/k/v projection.  apn_pt_colsum_rows(n) = ceil(n / 32), at most 1024; 0 outside 0 < n < 2^24.
 * Backward, go (n,c) = dL/dout; every part is float64 shares of apn_pt_rows(n, k, c) rows, folded by apn_pt_fold:
 *   attend_bwd: da[i,s,w] = sum over the 8 channels c = w + m c' (m ascending) of go[i,c] (v_j[c] + pr[c]), dl = a (da - sum_s a da),
 *     g1 (n,k,c') = (W4^T dl) [z > 0]; part[rows][c'c' + 3c'] = {dW4[c',e] = sum dl[c'] z[e], db4 = sum dl, sum g1, sum g1 t}.
 *   mid_bwd: dt = fma(sc2, g1, fma(D2, t, E2)), g0 = (W3^T dt) [y > 0] (not written);
 *     part[rows][c'c + c' + 2c] = {dW3[c',c] = sum dt[c'] y[c], db3 = sum dt, sum g0, sum g0 r}.
 *   rel_bwd: dr (n,k,c) = fma(sc1, g0, fma(D1, r, E1)) -- the one grouped tensor --, dqkv[i, 0:c] = -sum_s dr[i,s] (rows
 *     of pitch ldg >= 3c), dpr = dr + go[i,c] a[i,s,c mod c'], dh (n,k,3) = W2^T dpr;
 *     part[rows][4c] = {dW2[c,d] = sum dpr[c] h[d], db2 = sum dpr}.
 *   scatter_bwd: pcnt_poff / plist = apn_po_csr of idx; dqkv[j, c:2c] = the sum over j's list, in list order, of dr[pos],
 *     dqkv[j, 2c:3c] = that of go[pos / k, c] a[pos, c mod c']: sequential fp32 adds starting from the first term (an
 *     empty list gives 0).
 * c in {32, 64, 128, 256, 512}, 1 <= k <= 32, 0 <= n < 2^24, ld >= 3c, ldg >= 3c, non-null pointers (mid's part may be
 * NULL): APN_EINVAL otherwise, before any HIP call; n == 0 is a no-op.  One launch per entry: no synchronisation,
 * allocation, memset or atomic; every output element is written; every sum has a fixed order (a thread's own terms,
 * then the groups of a workgroup ascending, then apn_pt_fold): two runs give the same bits. */
APN_API int apn_pt_rows(int n, int k, int c);
APN_API int apn_pt_mid_rows(int n, int k, int c);
APN_API int apn_pt_rel_stats(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                             const float *wts, double *part, void *stream);
APN_API int apn_pt_fold(const double *part, int rows, int width, double *sums, void *stream);
APN_API int apn_pt_colsum_rows(int n);
APN_API int apn_pt_colsum(int n, int width, const float *src, int ld, double *part, void *stream);
APN_API int apn_pt_mid(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx, const float *wts,
                       const float *bn, float *t, double *part, void *stream);
APN_API int apn_pt_attend(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                          const float *wts, const float *bn, const float *t, float *a, float *out, void *stream);
APN_API int apn_pt_attend_bwd(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                              const float *wts, const float *bn, const float *t, const float *a, const float *go,
                              float *g1, double *part, void *stream);
APN_API int apn_pt_mid_bwd(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                           const float *wts, const float *bn, const float *de, const float *t, const float *g1,
                           double *part, void *stream);
APN_API int apn_pt_rel_bwd(int n, int k, int c, const float *qkv, int ld, const float *h, const int *idx,
                           const float *wts, const float *bn, const float *de, const float *t, const float *g1,
                           const float *a, const float *go, float *dr, float *dh, float *dqkv, int ldg, double *part,
                           void *stream);
APN_API int apn_pt_scatter_bwd(int n, int k, int c, const float *dr, const float *go, const float *a,
                               const int *pcnt_poff, const int *plist, float *dqkv, int ldg, void *stream);

/* Voxel-grid subsampling of STACKED clouds (csrc/voxel_grid.hip; the reference does it on the host: openpoints/dataset/
 * data_util.py: voxelize, openpoints/cpp/subsampling): coord (n,3) float32 (is_double = 0) or float64 (is_double = 1),
 * int32 offset (b) of cumulative END rows as above; row i belongs to the first cloud c with i < offset[c], a row at or
 * past offset[b-1] to the last one.  Per axis
 *         cell(i) = floor((double)coord[i] / (double)voxel_size)          (IEEE double division)
 * A row whose cell does not fit an int32 on some axis, or whose coordinate is not finite, is BAD.  A VOXEL is a set of
 * rows with equal (cloud, cell); coordinates may be negative.  Every output is a pure function of the inputs: integer
 * atomics only (compare-and-swap, min, max, add), each where the final value does not depend on the order; two runs give
 * the same bits.
 *   voxelize: voxel_of (n): voxels are numbered 0..m-1 in ascending order of their smallest member row (so a cloud's
 *     voxels are contiguous); idx_sort (n): the rows grouped by voxel number, ascending row inside a voxel (the stable
 *     argsort of voxel_of); start, count (n each, the first m written): voxel v's rows are idx_sort[start[v] .. start[v] +
 *     count[v]); new_offset (b): cumulative voxel ends per cloud (an empty cloud repeats the previous end, new_offset[b-1]
 *     == m); stats (3) = {m, count_max, bad}.  With bad > 0 the bad rows form one voxel of their own and the caller
 *     rejects the result.  scratch: apn_vg_scratch_ints(n) ints, 16-byte aligned, contents irrelevant (0 for an n the
 *     entries refuse).  A fixed chain of 9 + 5 ceil(bits(n - 1) / 8) launches, kernel boundaries the only seams: no
 *     workgroup waits for another, the probe loop of the row table is bounded by the table's size (>= 2n slots: it never
 *     fills), and the work does not depend on how the rows spread over the voxels.
 *   mean_fwd: out (m,c): out[v,ch] = (float)((double)s / (double)count[v]), the correctly rounded fp32 quotient, where s
 *     = the sequential fp32 sum of values[idx_sort[j], ch] (values (n,c)) over j = start[v] .. start[v] + count[v],
 *     STARTING FROM THE FIRST TERM: ascending row.  One thread per (voxel, channel).
 *   mean_bwd: grad_values[i,ch] = (float)((double)grad_out[voxel_of[i], ch] / (double)count[voxel_of[i]]): a gather.
 * b >= 1, 0 <= n < 2^27, 0 <= m <= n, 1 <= c <= 65536, voxel sizes finite and > 0, non-null pointers: APN_EINVAL
 * otherwise, before any HIP call.  n == 0 (voxelize: m = 0, nothing is written) or m == 0 is a no-op.  No entry
 * synchronises, allocates or issues a memset; element offsets are 64-bit inside the kernels; indices read from memory
 * are clamped into range before they address anything. */
APN_API int apn_vg_scratch_ints(int n);
APN_API int apn_vg_voxelize(int b, int n, int is_double, const void *coord, double vx, double vy, double vz,
                            const int *offset, int *scratch, int *voxel_of, int *count, int *start, int *idx_sort,
                            int *new_offset, int *stats, void *stream);
APN_API int apn_vg_mean_fwd(int n, int m, int c, const float *values, const int *idx_sort, const int *start,
                            const int *count, float *out, void *stream);
APN_API int apn_vg_mean_bwd(int n, int m, int c, const float *grad_out, const int *voxel_of, const int *count,
                            float *grad_values, void *stream);

/* RandLA-Net's LocalSpatialEncoding + AttentivePooling as one layer (csrc/randla.hip).
 * coords (b,n,3) float32; idx (b,n,k) int32 and dist (b,n,k) float32 as apn_knn_query returns them for support = query
 * = coords (idx is clamped into [0, n)); sqrt_dist != 0: the kernels take the root of dist.  Per (point, neighbour) pair
 * e = [p_n, p_j, p_n - p_j, dist] (10 wide).  Shapes: b >= 0 (0: nothing is launched), n >= 1, 1 <= k <= 32,
 * b n < 2^24, c in {8, 16, 32, 64, 128}; anything else is APN_EINVAL before a launch.
 *   moments: mom[65] (float64) = {sum e_i (10), sum e_i e_j for i <= j (55, row-major upper triangle)} over the b n k
 *     pairs; part[apn_rl_moment_rows(b, n, k)][65] (float64) is the workgroups' shares, added in the shared order at 8
 *     lanes ("Partial-row folds", above).
 *   fold: w (c,10), bias (c or NULL): the convolution; gamma, beta (c or NULL), eps, momentum: its BatchNorm; count =
 *     b n k.  training != 0: batch mean = w.mu + bias and biased variance = w^T Sigma w from mom; running_mean /
 *     running_var (both or neither) take (1 - momentum) old + momentum new, the variance unbiased, and
 *     *num_batches_tracked (int64, or NULL) grows by one.  training == 0: the running buffers are the statistics (mom may
 *     be NULL).  wf[11 c + 10] (float32) = W' (c,10), b' (c), mu (10: the encoding's batch mean, zeros when training == 0):
 *     relu(W' (e - mu) + b') is the layer's hidden value;
 *     stat[3 c] (float64) = mean | variance | 1 / sqrt(variance + eps) as used.
 *   forward: at (c,c): at[c2 c + c1] = A_hh[c1][c2], the transposed top-left block of the 2c x 2c score weight.
 *     pooled (b,c,n): pooled[c1,n] = sum_k softmax_k((A_hh h_k)[c1]) h_k[c1].
 *   backward: a (c,c) = A_hh, at its transpose, dpooled (b,c,n); part[apn_rl_bwd_rows(b, n, k, c)][c c + 11 c]
 *     (float32): per workgroup the shares of dA_hh and, per channel, of {sum dy (e - mu)_0..9, sum dy}.
 *   finalize: rows = apn_rl_bwd_rows(...); sums[c c + 11 c] (float64): scratch, the rows added in the shared order at 8 lanes;
 *     grads[c c + 13 c] (float32) = dA_hh | dgamma | dbeta | dW (c,10) | dbias (dbias is an exact zero when training != 0).  No gradient flows to coords, dist or idx.
 * Every sum has an order fixed by the shapes: two runs give the same bits.  No atomics, no memset. */
APN_API int apn_rl_moment_rows(int b, int n, int k);
APN_API int apn_rl_bwd_rows(int b, int n, int k, int c);
APN_API int apn_rl_moments(int b, int n, int k, const float *coords, const int *idx, const float *dist, int sqrt_dist,
                           double *part, double *mom, void *stream);
APN_API int apn_rl_fold(int c, const double *mom, double count, const float *w, const float *bias, const float *gamma,
                        const float *beta, float eps, float momentum, int training, float *running_mean,
                        float *running_var, long long *num_batches_tracked, float *wf, double *stat, void *stream);
APN_API int apn_rl_forward(int b, int n, int k, int c, const float *coords, const int *idx, const float *dist,
                           int sqrt_dist, const float *wf, const float *at, float *pooled, void *stream);
APN_API int apn_rl_backward(int b, int n, int k, int c, const float *coords, const int *idx, const float *dist,
                            int sqrt_dist, const float *wf, const float *a, const float *at, const float *dpooled,
                            float *part, void *stream);
APN_API int apn_rl_finalize(int c, int rows, const float *part, const double *mom, double count, const float *w,
                            const float *bias, const float *gamma, const double *stat, int training, double *sums,
                            float *grads, void *stream);

/* PointMLP's geometric-affine grouping stage with its first convolution hoisted to the points (csrc/affine_group.hip):
 * LocalGrouper(normalize="anchor", use_xyz=False) + PreExtraction.transfer's bias-free convolution
 * (openpoints/models/backbone/pointmlp.py).  Per cloud, with j = idx[s,k] and a = fps_idx[s]:
 *         d[s,k,:] = x[j,:] - x[a,:],   sigma = unbiased std of the s k c entries of d,   r = 1 / (sigma + 1e-5)
 *         y[s,k,:] = r (P[j,:] - P[a,:]) + Q[a,:] + c0,    [P | Q] = x [W1 alpha | W2]^T,  c0 = W1 beta
 * b clouds of n points, s queries of k neighbours; x (b,n,c) ROWS, pq (b,n,2o) rows [P | Q], idx (b,s,k) and
 * fps_idx (b,s) int32 indices INTO THE CLOUD (every index read is clamped into [0, n)), y (b,o,s k) channels first with
 * position s k + slot.  Everything fp32 / int32 and contiguous; element offsets are 64-bit inside the kernels.
 *   moments: part [apn_ag_moment_rows(s)][b][2] = float64 {sum d, sum d^2} of each workgroup's queries (d rounded to
 *     fp32 as the subtraction gives it, squared and added in float64); apn_ag_fold(rows, 2 b) gives the (b,2) moments.
 *   fold: out[col] = the sum of part[rows][ncol] (float64) over the rows, in the shared order at 4 lanes ("Partial-row
 *     folds", above).
 *   combine_fwd: r (b) and c0 (o) are INPUT arrays.  v = ((r * (P[j] - P[a])) + Q[a]) + c0, each operation rounded.
 *     training != 0: y and part are written -- part [apn_pw_conv_tiles(b, s k)][2][o], BatchNorm's partial statistics in
 *       the layout apn_pw_bn_act folds ({sum, M2 around the tile's own mean} per 128 positions of a cloud).
 *     training == 0: out = [relu](scale v + shift) from the running statistics (gamma / beta may be null) in the same
 *       launch; y and stat [4][o] are written when not null (apn_fp_blend_stats's form).
 *   combine_bwd: gyt = dL/dy as ROWS (b, s k, o) (apn_pw_transpose of the channels-first gradient); the reverse lists of
 *     idx and of fps_idx are apn_po_csr's on FLAT rows (index + cloud * n; n = b n rows, m = b s queries, k and 1): the
 *     anchors of a cloud need not be distinct.  With A_i = the sum over i's neighbour list of gyt[pos] and G_i = the sum
 *     over the queries anchored at i of (sum_k gyt[s,k], ascending k), both in list order in fp32:
 *         dpq[i] = [ r (A_i - G_i) | G_i ]                                  every element written
 *         part_dr [apn_ag_point_rows(n)][b]  = float64 shares of  dr[b]  = sum_i <P_i, A_i - G_i>  (= sum <gy, P[j] - P[a]>)
 *         part_c0 [b apn_ag_point_rows(n)][o] = float64 shares of  dc0[o] = sum_i G_i
 *     both folded by apn_ag_fold.
 *   sigma_bwd: kappa (b), mu (b) input arrays;
 *         dx[i] = kappa (sum over i's neighbour list of ((x_i - x_a) - mu) - sum over the queries anchored at i of
 *                 sum_k ((x_j - x_i) - mu)),  every element of dx (b,n,c) written.
 *   res_relu_max: z, h (b,o,s k) -> out (b,o,s) = max_k relu(z + h), sel (b,o,s) uint8 = the slot of the FIRST maximum,
 *     0 where no sum is positive (out = 0 there).  grad: gz (and gh unless null) (b,o,s k) = g at the kept slot where
 *     out > 0, zero elsewhere; every element written.
 * No float atomics: every sum runs in an order fixed by the shapes.  One launch per entry; no synchronisation,
 * allocation or memset.  1 <= k <= 64, k <= n, b <= 65535, b n < 2^24, b s < 2^24 (res_relu_max: o <= 65535,
 * b o s < 2^31), non-negative sizes, non-null pointers: APN_EINVAL otherwise, before any HIP call; a zero-sized problem is
 * a no-op. */
APN_API int apn_ag_moment_rows(int s);
APN_API int apn_ag_point_rows(int n);
APN_API int apn_ag_moments(int b, int n, int s, int k, int c, const float *x, const int *idx, const int *fps_idx,
                           double *part, void *stream);
APN_API int apn_ag_fold(int rows, int ncol, const double *part, double *out, void *stream);
APN_API int apn_ag_combine_fwd(int b, int n, int s, int k, int o, const float *pq, const int *idx, const int *fps_idx,
                               const float *r, const float *c0, float *y, float *part, int training, const float *gamma,
                               const float *beta, const float *run_mean, const float *run_var, float eps, int relu,
                               float *stat, float *out, void *stream);
APN_API int apn_ag_combine_bwd(int b, int n, int s, int k, int o, const float *gyt, const float *r, const float *pq,
                               const int *pcnt_poff_i, const int *plist_i, const int *pcnt_poff_a, const int *plist_a,
                               float *dpq, double *part_dr, double *part_c0, void *stream);
APN_API int apn_ag_sigma_bwd(int b, int n, int s, int k, int c, const float *x, const int *idx, const int *fps_idx,
                             const float *kappa, const float *mu, const int *pcnt_poff_i, const int *plist_i,
                             const int *pcnt_poff_a, const int *plist_a, float *dx, void *stream);
APN_API int apn_ag_res_relu_max(int b, int o, int s, int k, const float *z, const float *h, float *out, void *sel,
                                void *stream);
APN_API int apn_ag_res_relu_max_grad(int b, int o, int s, int k, const float *g, const float *out, const void *sel,
                                     float *gz, float *gh, void *stream);

/* Tuning / diagnostic entry, NOT part of the reference boundary: apn_furthest_point_sampling
 * with the number of wavefronts that cooperate on one cloud (1, 2, 4, 8 or 16; 0 = the built-in
 * heuristic) and the step algorithm (0 = one LDS 64-bit atomic max per step for n <= 4096: what the operator
 * entries run; 1 = per-wave records + second reduction) chosen PER CALL.  No process-wide state: every entry
 * point of this library is re-entrant.  Results do not depend on either argument. */
APN_API int apn_furthest_point_sampling_tuned(int b, int n, int m, const float *xyz, float *temp,
                                              int *idx, int waves, int algo, void *stream);

/* Diagnostic only: the FPS step of the n = 1024 geometry with s_memtime stamps; dbg[0..5]
 * = cycles summed over the m-1 steps for {update, wave max, pick+LDS write, barrier,
 * LDS read, group max + broadcast}.  Not part of the product path. */
APN_API int apn_fps_debug_stamps(int b, int n, int m, const float *xyz, float *temp, int *idxs,
                                 unsigned long long *dbg, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ADAPTPOINT_AMD_H */
