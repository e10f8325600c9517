// token_attention.hip -- multi-head self-attention over the T tokens of a cloud at head_dim 64 (PointViT's
// `Attention`, openpoints/models/backbone/pointvit.py: softmax(q k^T * 64^-1/2) v), ANY T >= 1, without the (B,H,T,T)
// score tensor in either direction.
//
// Input is the packed qkv (B, T, [3][H][64]) f32 exactly as nn.Linear(dim, 3 dim) leaves it; the output is
// (B, T, H*64) in the layout `proj` consumes and the backward writes the packed dqkv (B, T, [3][H][64]): no permute,
// chunk or cat on the torch side.  There are no operand images in memory either: every workgroup splits what it stages
// into bf16 hi + lo planes on the way into LDS, and a wave splits its own 32 rows into registers.
//
// The arithmetic is attention.hip's (apn_mfma.h: v_mfma_f32_32x32x16_bf16 on split operands, three MFMAs per product),
// with four k-steps per score (64 dims) and two accumulators per second product (64 output rows):
//
//     S^T tile (32 keys x 32 queries) = K_tile (32 x 64) . Q^T (64 x 32)              4 k-steps
//     s2 = S^T * (0.125 * log2 e)                                                     0.125 = 64^-1/2, a power of two
//     O^T (64 x 32 queries)          += V_tile^T (64 x 32 keys) . P^T (32 x 32)       2 k-steps x 2 row blocks
//
// S is produced transposed so that a query is a lane and the keys run over the lane's registers: the soft-max
// statistics are in-register, and the accumulator of S^T is already the B operand of the second product.
//
// The ragged tail.  T is in general no multiple of 32 (65, 129, 257: cls token + groups).  A staged point past T is
// ZERO in LDS (never read from memory), and
//   * a padded KEY's score is replaced by -inf before the running maximum, so its probability is exp2(-inf) = 0
//     exactly -- whatever the real scores are (all negative, say: an unmasked zero pad would then hold the maximum);
//     in the backward its P and dS are selected to 0;
//   * a padded QUERY is computed on a copy of row T-1 where a wave owns it (nothing is stored), and is selected to
//     P = dS = 0 where the key-owning waves stream over it, so it adds nothing to dK / dV.
// Every tile that is visited holds at least one real key, so the running maximum is finite from the first tile on.
//
// Backward (P recomputed from the saved log-sum-exp, delta_i = dO_i . O_i from a small kernel of its own):
//   tok_bwd_kv: a wave owns 32 KEYS and streams over the queries   -> dK, dV   (sums over queries in tile order)
//   tok_bwd_q : a wave owns 32 QUERIES and streams over the keys   -> dQ       (sums over keys in tile order)
// No atomics anywhere: every output element has one owner and a fixed summation order, so results are bit-reproducible
// and do not depend on B, H or the other clouds / heads of the batch.
#include "apn_common.h"
#include "apn_mfma.h"

namespace apn {

constexpr int TK_D = 64;                 // head dim
constexpr int TK_WAVES = 4;              // waves per workgroup, each owning 32 rows
constexpr int TK_THREADS = TK_WAVES * 64;
constexpr int TK_FWD_CHUNK = 64;         // keys staged per LDS pass of the forward
constexpr int TK_BWD_CHUNK = 32;         // points staged per LDS pass of the two backward kernels (one tile)
constexpr int TK_RS = 2 * TK_D + 8;      // bf16 per staged row: [hi 64 | lo 64] + 16 bytes of padding
constexpr int TK_MAX_T = 1 << 24;
constexpr float TK_SCALE = 0.125f * 1.4426950408889634f;    // 64^-1/2 * log2(e): the float32 log2(e), scaled exactly

// position of point `key` (0..31) of a 32-tile in accumulator-row order: position 16 s + 8 h + j holds point
// acc_row(8 s + j, h) = (j & 3) | h << 2 | (j >> 2) << 3 | s << 4
__device__ __forceinline__ int tk_pos(int key) {
    return (key & 16) | (((key >> 2) & 1) << 3) | (((key >> 3) & 1) << 2) | (key & 3);
}

// CH points t0 .. t0+CH-1 of one (cloud, head) operand (`src`: its row 0, `pitch` floats between points) -> LDS, split
// into hi + lo bf16; points at or past T are staged as zeros and not read.
//   ROWS : sR[point][hi 64 | lo 64]            -- the point is an operand row / column
//   TRANS: sT[plane * 64 + d][CH + 8]          -- the point is a contraction index; every 32-tile in accumulator-row order
template <int CH, bool ROWS, bool TRANS>
__device__ __forceinline__ void tk_stage(const float *__restrict__ src, size_t pitch, int t0, int T, __bf16 *sR, __bf16 *sT) {
    constexpr int TS = CH + 8;
    for (int e = threadIdx.x; e < CH * 8; e += TK_THREADS) {
        const int pt = e >> 3, piece = e & 7;
        float x[8];
        if (t0 + pt < T) {
            const float4 *p = reinterpret_cast<const float4 *>(src + (size_t)(t0 + pt) * pitch + piece * 8);
            const float4 a = p[0], b = p[1];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = 0.0f;
        }
        const Frag<2> f = make_frag<2>(x);
        if (ROWS) {
            *reinterpret_cast<bf16x8 *>(sR + pt * TK_RS + piece * 8) = f.p[0];
            *reinterpret_cast<bf16x8 *>(sR + pt * TK_RS + TK_D + piece * 8) = f.p[1];
        }
        if (TRANS) {
            const int pos = (pt & ~31) | tk_pos(pt & 31);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sT[(piece * 8 + j) * TS + pos] = f.p[0][j];
                sT[(TK_D + piece * 8 + j) * TS + pos] = f.p[1][j];
            }
        }
    }
}

// operand whose row / column is a staged point: k-step ks holds d = 16 ks + 8 h .. + 7
__device__ __forceinline__ Frag<2> tk_row_frag(const __bf16 *row, int ks, int h) {
    Frag<2> f;
    f.p[0] = *reinterpret_cast<const bf16x8 *>(row + 16 * ks + 8 * h);
    f.p[1] = *reinterpret_cast<const bf16x8 *>(row + TK_D + 16 * ks + 8 * h);
    return f;
}

// A operand whose contraction index runs over staged points: row d, 8 positions from `pos`
template <int CH>
__device__ __forceinline__ Frag<2> tk_trans_frag(const __bf16 *img, int d, int pos) {
    Frag<2> f;
    f.p[0] = *reinterpret_cast<const bf16x8 *>(img + d * (CH + 8) + pos);
    f.p[1] = *reinterpret_cast<const bf16x8 *>(img + (TK_D + d) * (CH + 8) + pos);
    return f;
}

// the wave's own point as a B operand (lane = column): the four k-steps of its 64 numbers, split in registers
__device__ __forceinline__ void tk_own_frags(const float *__restrict__ row, int h, Frag<2> (&f)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const float4 *p = reinterpret_cast<const float4 *>(row + 16 * ks + 8 * h);
        const float4 a = p[0], b = p[1];
        const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        f[ks] = make_frag<2>(x);
    }
}

// acc[a][i] <-> d = 32 a + acc_row(i, h): four consecutive d per group of four registers
__device__ __forceinline__ void tk_store_row(float *__restrict__ dst, int h, const f32x16 (&acc)[2], float scale) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
            *reinterpret_cast<float4 *>(dst + 32 * a + 8 * g4 + 4 * h) =
                make_float4(acc[a][4 * g4] * scale, acc[a][4 * g4 + 1] * scale, acc[a][4 * g4 + 2] * scale,
                            acc[a][4 * g4 + 3] * scale);
}

// out (B,T,H*64) f32; lse (B,H,T) f32 = running max + log2(running sum), in log2 units.
__global__ __launch_bounds__(TK_THREADS) void tok_fwd_kernel(int T, int heads, const float *__restrict__ qkv,
                                                             float *__restrict__ out, float *__restrict__ lse) {
    constexpr int CH = TK_FWD_CHUNK;
    __shared__ __attribute__((aligned(16))) __bf16 sK[CH * TK_RS];
    __shared__ __attribute__((aligned(16))) __bf16 sVt[2 * TK_D * (CH + 8)];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = blockIdx.y, cloud = blockIdx.z, c = heads * TK_D;
    const size_t pitch = (size_t)3 * c;
    const float *qb = qkv + (size_t)cloud * T * pitch + head * TK_D;          // q of token 0; k at + c, v at + 2 c
    const int q0 = (blockIdx.x * TK_WAVES + wave) * 32;                       // this wave's query tile
    const int qr = q0 + r < T ? q0 + r : T - 1;                               // padded queries: a copy of the last row
    Frag<2> qf[4];
    tk_own_frags(qb + (size_t)qr * pitch, h, qf);
    f32x16 o[2] = {{0}, {0}};
    float mx = -INFINITY, lsum = 0.0f;
    for (int k0 = 0; k0 < T; k0 += CH) {
        __syncthreads();
        tk_stage<CH, true, false>(qb + c, pitch, k0, T, sK, nullptr);
        tk_stage<CH, false, true>(qb + 2 * c, pitch, k0, T, nullptr, sVt);
        __syncthreads();
        const int keys = T - k0 < CH ? T - k0 : CH, tiles = (keys + 31) >> 5;
        for (int t = 0; t < tiles; ++t) {
            f32x16 s = {0};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s = mfma<2>(tk_row_frag(sK + (t * 32 + r) * TK_RS, ks, h), qf[ks], s);
            // s[i]: key k0 + 32 t + acc_row(i, h), query r.  To log2 units; padded keys to -inf
            const int kb = k0 + t * 32 + 4 * h;
            float tmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = kb + (i & 3) + 8 * (i >> 2) < T ? s[i] * TK_SCALE : -INFINITY;
                tmax = __builtin_fmaxf(tmax, s[i]);
            }
            tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 32));
            const float mnew = __builtin_fmaxf(mx, tmax);                     // finite: the tile holds a real key
            const float alpha = __builtin_amdgcn_exp2f(mx - mnew);            // exp2(-inf) = 0 on the first tile
            float psum = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = __builtin_amdgcn_exp2f(s[i] - mnew);
                psum += s[i];
            }
            lsum = lsum * alpha + psum;
            mx = mnew;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[a][i] *= alpha;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const Frag<2> pf = pack8<2>(s, 8 * st);
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    o[a] = mfma<2>(tk_trans_frag<CH>(sVt, 32 * a + r, t * 32 + 16 * st + 8 * h), pf, o[a]);
            }
        }
    }
    if (q0 + r >= T) return;
    lsum += __shfl_xor(lsum, 32);        // (both halves of a live query are live)
    tk_store_row(out + ((size_t)cloud * T + q0 + r) * c + head * TK_D, h, o, 1.0f / lsum);
    if (h == 0) lse[((size_t)cloud * heads + head) * T + q0 + r] = mx + __builtin_amdgcn_logf(lsum);   // v_log_f32 = log2
}

// delta (B,H,T) = sum_d g_out[b,t,h,d] * out[b,t,h,d]: 16 lanes per (b, t, h) row of 64, a fixed butterfly.
__global__ __launch_bounds__(256) void tok_delta_kernel(long long rows, int T, int heads, const float *__restrict__ g,
                                                        const float *__restrict__ out, float *__restrict__ delta) {
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    float s = 0.0f;
    if (row < rows) {
        const float4 a = *reinterpret_cast<const float4 *>(g + row * TK_D + sub * 4);
        const float4 b = *reinterpret_cast<const float4 *>(out + row * TK_D + sub * 4);
        s = ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
    if (row < rows && sub == 0) {
        const long long bt = row / heads;
        const int head = (int)(row - bt * heads);
        const long long cloud = bt / T;
        delta[(cloud * heads + head) * T + (bt - cloud * T)] = s;
    }
}

// With P recomputed from lse and delta_i = dO_i . O_i:
//     dV_j = sum_i P_ij dO_i          dP_ij = dO_i . V_j          dS_ij = P_ij (dP_ij - delta_i)
//     dQ_i = sum_j dS_ij K_j / 8      dK_j = sum_i dS_ij Q_i / 8
// dk, dv of dqkv (B,T,[3][H][64]).
__global__ __launch_bounds__(TK_THREADS) void tok_bwd_kv_kernel(int T, int heads, const float *__restrict__ qkv,
                                                                const float *__restrict__ g_out,
                                                                const float *__restrict__ lse,
                                                                const float *__restrict__ delta,
                                                                float *__restrict__ dqkv) {
    constexpr int CH = TK_BWD_CHUNK;
    __shared__ __attribute__((aligned(16))) __bf16 sQ[CH * TK_RS], sG[CH * TK_RS];
    __shared__ __attribute__((aligned(16))) __bf16 sQt[2 * TK_D * (CH + 8)], sGt[2 * TK_D * (CH + 8)];
    __shared__ float sL[CH], sD[CH];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = blockIdx.y, cloud = blockIdx.z, c = heads * TK_D;
    const size_t pitch = (size_t)3 * c, bh = (size_t)cloud * heads + head;
    const float *qb = qkv + (size_t)cloud * T * pitch + head * TK_D;
    const float *gb = g_out + (size_t)cloud * T * c + head * TK_D;
    const int j0 = (blockIdx.x * TK_WAVES + wave) * 32;                       // this wave's key tile
    const int jr = j0 + r < T ? j0 + r : T - 1;
    // B operands (lane = key column): K^T for S, V^T for dP
    Frag<2> kf[4], vf[4];
    tk_own_frags(qb + c + (size_t)jr * pitch, h, kf);
    tk_own_frags(qb + 2 * c + (size_t)jr * pitch, h, vf);
    f32x16 dvt[2] = {{0}, {0}}, dkt[2] = {{0}, {0}};                          // dV^T, dK^T: rows d, columns keys
    for (int i0 = 0; i0 < T; i0 += CH) {
        __syncthreads();
        tk_stage<CH, true, true>(qb, pitch, i0, T, sQ, sQt);
        tk_stage<CH, true, true>(gb, (size_t)c, i0, T, sG, sGt);
        if (threadIdx.x < CH) {
            const bool real = i0 + (int)threadIdx.x < T;
            sL[threadIdx.x] = real ? lse[bh * T + i0 + threadIdx.x] : 0.0f;
            sD[threadIdx.x] = real ? delta[bh * T + i0 + threadIdx.x] : 0.0f;
        }
        __syncthreads();
        // S = Q K^T, dP = dO V^T: rows = queries i0 + acc_row(i, h), columns = keys (lane)
        f32x16 s = {0}, dp = {0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = mfma<2>(tk_row_frag(sQ + r * TK_RS, ks, h), kf[ks], s);
            dp = mfma<2>(tk_row_frag(sG + r * TK_RS, ks, h), vf[ks], dp);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int qi = acc_row(i, h);
            const float pij = i0 + qi < T ? __builtin_amdgcn_exp2f(s[i] * TK_SCALE - sL[qi]) : 0.0f;   // padded queries: 0
            s[i] = pij;                                        // P
            dp[i] = pij * (dp[i] - sD[qi]);                    // dS
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const Frag<2> pf = pack8<2>(s, 8 * st), sf = pack8<2>(dp, 8 * st);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                dvt[a] = mfma<2>(tk_trans_frag<CH>(sGt, 32 * a + r, 16 * st + 8 * h), pf, dvt[a]);
                dkt[a] = mfma<2>(tk_trans_frag<CH>(sQt, 32 * a + r, 16 * st + 8 * h), sf, dkt[a]);
            }
        }
    }
    if (j0 + r >= T) return;
    float *row = dqkv + ((size_t)cloud * T + j0 + r) * pitch + head * TK_D;
    tk_store_row(row + c, h, dkt, 0.125f);
    tk_store_row(row + 2 * c, h, dvt, 1.0f);
}

// dq of dqkv (B,T,[3][H][64]).
__global__ __launch_bounds__(TK_THREADS) void tok_bwd_q_kernel(int T, int heads, const float *__restrict__ qkv,
                                                               const float *__restrict__ g_out,
                                                               const float *__restrict__ lse,
                                                               const float *__restrict__ delta,
                                                               float *__restrict__ dqkv) {
    constexpr int CH = TK_BWD_CHUNK;
    __shared__ __attribute__((aligned(16))) __bf16 sK[CH * TK_RS], sV[CH * TK_RS];
    __shared__ __attribute__((aligned(16))) __bf16 sKt[2 * TK_D * (CH + 8)];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = blockIdx.y, cloud = blockIdx.z, c = heads * TK_D;
    const size_t pitch = (size_t)3 * c, bh = (size_t)cloud * heads + head;
    const float *qb = qkv + (size_t)cloud * T * pitch + head * TK_D;
    const float *gb = g_out + (size_t)cloud * T * c + head * TK_D;
    const int q0 = (blockIdx.x * TK_WAVES + wave) * 32;
    const int qr = q0 + r < T ? q0 + r : T - 1;
    // B operands (lane = query column): Q^T for S^T, dO^T for dP^T
    Frag<2> qf[4], gf[4];
    tk_own_frags(qb + (size_t)qr * pitch, h, qf);
    tk_own_frags(gb + (size_t)qr * c, h, gf);
    const float lq = lse[bh * T + qr], dl = delta[bh * T + qr];
    f32x16 dqt[2] = {{0}, {0}};
    for (int k0 = 0; k0 < T; k0 += CH) {
        __syncthreads();
        tk_stage<CH, true, true>(qb + c, pitch, k0, T, sK, sKt);
        tk_stage<CH, true, false>(qb + 2 * c, pitch, k0, T, sV, nullptr);
        __syncthreads();
        // S^T = K Q^T, dP^T = V dO^T: rows = keys k0 + acc_row(i, h), columns = queries (lane)
        f32x16 s = {0}, dp = {0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = mfma<2>(tk_row_frag(sK + r * TK_RS, ks, h), qf[ks], s);
            dp = mfma<2>(tk_row_frag(sV + r * TK_RS, ks, h), gf[ks], dp);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)                            // dS^T; padded keys: 0
            dp[i] = k0 + acc_row(i, h) < T ? __builtin_amdgcn_exp2f(s[i] * TK_SCALE - lq) * (dp[i] - dl) : 0.0f;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const Frag<2> sf = pack8<2>(dp, 8 * st);
#pragma unroll
            for (int a = 0; a < 2; ++a)
                dqt[a] = mfma<2>(tk_trans_frag<CH>(sKt, 32 * a + r, 16 * st + 8 * h), sf, dqt[a]);
        }
    }
    if (q0 + r >= T) return;
    tk_store_row(dqkv + ((size_t)cloud * T + q0 + r) * pitch + head * TK_D, h, dqt, 0.125f);
}

// b, heads: grid dimensions z, y.  t: the row tiles are grid dimension x and b * t * heads / 16 the delta kernel's.
static int tok_check(int b, int t, int heads) {
    if (b <= 0 || t <= 0 || heads <= 0 || b > 65535 || heads > 65535 || t > TK_MAX_T) return APN_EINVAL;
    if ((long long)b * t * heads / 16 >= 0x7fffffffLL) return APN_EINVAL;
    return APN_OK;
}

static bool tok_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace apn

extern "C" int apn_token_attention_max_tokens(void) { return apn::TK_MAX_T; }

extern "C" int apn_token_attention_fwd(int b, int t, int heads, const float *qkv, float *out, float *lse, void *stream) {
    using namespace apn;
    if (int e = tok_check(b, t, heads)) return e;
    if (!qkv || !out || !lse || !tok_aligned16(qkv) || !tok_aligned16(out)) return APN_EINVAL;
    const int per_wg = TK_WAVES * 32;
    hipLaunchKernelGGL(tok_fwd_kernel, dim3((t + per_wg - 1) / per_wg, heads, b), dim3(TK_THREADS), 0, (hipStream_t)stream,
                       t, heads, qkv, out, lse);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_token_attention_bwd(int b, int t, int heads, const float *qkv, const float *out, const float *lse,
                                       const float *g_out, float *delta, float *dqkv, void *stream) {
    using namespace apn;
    if (int e = tok_check(b, t, heads)) return e;
    if (!qkv || !out || !lse || !g_out || !delta || !dqkv) return APN_EINVAL;
    if (!tok_aligned16(qkv) || !tok_aligned16(out) || !tok_aligned16(g_out) || !tok_aligned16(dqkv)) return APN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)b * t * heads;
    hipLaunchKernelGGL(tok_delta_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, rows, t, heads, g_out, out,
                       delta);
    const int per_wg = TK_WAVES * 32;
    const dim3 grid((t + per_wg - 1) / per_wg, heads, b);
    hipLaunchKernelGGL(tok_bwd_kv_kernel, grid, dim3(TK_THREADS), 0, st, t, heads, qkv, g_out, lse, delta, dqkv);
    hipLaunchKernelGGL(tok_bwd_q_kernel, grid, dim3(TK_THREADS), 0, st, t, heads, qkv, g_out, lse, delta, dqkv);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
