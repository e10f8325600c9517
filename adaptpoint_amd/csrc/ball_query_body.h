// ball_query_body.h -- the radius search of ball_query.hip as a device function, so that it can
// also run as one ROLE of the fused index-stage launch (fps.hip: fps_ball_kernel).
#pragma once
#include "apn_common.h"

namespace apn {

constexpr int BQ_CHUNK = 4096;             // support points staged per LDS pass (48 KiB)
constexpr int BQ_QPW = 4;                  // consecutive queries a wave owns (8 for full tiles: ball_query.hip)
constexpr int BQ_SLOTS = 16;               // register slots of a wave's chunk: lane l, slot s holds point 64 s + l
constexpr int BQ_REG = 64 * BQ_SLOTS;      // support points a wave holds in registers (48 VGPRs)
constexpr int BQ_GROUP = 4;                // slots compared before their hits are emitted (the early exit's granularity)

// The value as the compiler cannot see through it: what is derived from it inside a rarely taken block is computed
// there, and not hoisted out of the query loop as sixteen loop-invariant registers (one per slot).
__device__ __forceinline__ int opaque_v(int v) { asm volatile("" : "+v"(v)); return v; }

// One workgroup of WAVES waves: tile `bx` of cloud `cloud`; each wave owns queries
// q0 + QPW * wave .. + QPW - 1, then those WAVES * QPW further on, of the tile.  s_dyn: three coordinate
// planes of min(n, BQ_CHUNK) floats, then 2 * q_per_block ints.
//
// A wave copies BQ_REG staged points into registers once and scans them for each of its queries without
// reading LDS again.  The scan of a query is straight-line: for a group of BQ_GROUP slots the BQ_GROUP
// hit masks (7 float instructions per slot, the compare writes the mask), THEN, for the non-empty masks in
// slot order, the slots of the hits (count + mbcnt) and their stores.  Lanes past the end of the cloud
// hold NaN coordinates: their d2 is NaN and `d2 < radius2` is false for every radius2, so the loop
// carries no per-lane bounds test.  A group of slots is copied from LDS when the first query reaches it:
// queries whose balls saturate early never pay for the rest of the chunk.
template <int WAVES, int QPW = BQ_QPW>
__device__ __forceinline__ void ball_query_body(
    int n, int m, float radius2, int nsample, int q_per_block, int zero_empty,
    const float *__restrict__ new_xyz, const float *__restrict__ xyz, int *__restrict__ idx,
    int cloud, int bx, float *s_dyn) {
    const int chunk = min(n, BQ_CHUNK);
    float *sx = s_dyn, *sy = s_dyn + chunk, *sz = s_dyn + 2 * chunk;
    int *s_cnt = reinterpret_cast<int *>(s_dyn + 3 * chunk);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q_begin = bx * q_per_block;
    const int q_end = min(q_begin + q_per_block, m);

    xyz += (size_t)cloud * n * 3;
    new_xyz += (size_t)cloud * m * 3;
    idx += (size_t)cloud * m * nsample;

    // Clouds above BQ_REG points: a query's hit count and first hit pass from one register chunk to the
    // next through LDS.  The same wave owns the query in every chunk, so no barrier orders these.
    const bool carried = n > BQ_REG;
    int *cnt_of = s_cnt;
    int *first_of = s_cnt + q_per_block;
    if (carried)
        for (int i = tid; i < q_per_block; i += WAVES * 64) { cnt_of[i] = 0; first_of[i] = 0; }

    // The end of a query's row, by the wave that scanned it: slots the scan never reached repeat the
    // first hit (ball_query_gpu.cu:41-45).  Rows of empty balls stay untouched, or become zeros.
    auto finish = [&](int q, int cnt, int first) {
        if ((cnt == 0 && !zero_empty) || cnt >= nsample) return;
        int *row = idx + (size_t)q * nsample;
#pragma nounroll
        for (int l = cnt + lane; l < nsample; l += 64) row[l] = first;   // first == 0 for an empty ball
    };

    for (int base = 0; base < n; base += BQ_CHUNK) {
        const int len = min(BQ_CHUNK, n - base);
        __syncthreads();  // previous pass done with the planes (and cnt init visible)
        // Coalesced staging: the chunk is 3*len consecutive floats.
        for (int i = tid; i < 3 * len; i += WAVES * 64) {
            const float v = xyz[(size_t)base * 3 + i];
            const int p = i / 3, c = i - p * 3;
            (c == 0 ? sx : c == 1 ? sy : sz)[p] = v;
        }
        __syncthreads();

        for (int rc = 0; rc < len; rc += BQ_REG) {
            const int rlen = min(BQ_REG, len - rc);                 // >= 1
            const bool last = base + rc + BQ_REG >= n;              // the cloud ends in this register chunk
            const int point0 = base + rc + lane;                    // the point of slot 0
            float px[BQ_SLOTS], py[BQ_SLOTS], pz[BQ_SLOTS];
#pragma unroll
            for (int s = 0; s < BQ_SLOTS; ++s) px[s] = py[s] = pz[s] = __builtin_nanf("");
            int loaded = 0;                                         // groups of slots already in registers (wave-uniform)

#pragma nounroll
            for (int qb = q_begin + wave * QPW; qb < q_end; qb += WAVES * QPW) {
                const int qe = min(qb + QPW, q_end);
                float nx = new_xyz[qb * 3 + 0], ny = new_xyz[qb * 3 + 1], nz = new_xyz[qb * 3 + 2];   // wave-uniform (scalar loads)
#pragma nounroll
                for (int q = qb; q < qe; ++q) {
                    const float qx = nx, qy = ny, qz = nz;
                    const int qn = min(q + 1, qe - 1);              // the next query's coordinates arrive during this one's scan
                    nx = new_xyz[qn * 3 + 0]; ny = new_xyz[qn * 3 + 1]; nz = new_xyz[qn * 3 + 2];
                    int cnt = 0, first = 0;
                    if (carried) {
                        cnt = __builtin_amdgcn_readfirstlane(cnt_of[q - q_begin]);
                        first = __builtin_amdgcn_readfirstlane(first_of[q - q_begin]);
                    }
                    if (cnt < nsample) {
                        int *row = idx + (size_t)q * nsample;
                        const bool empty = cnt == 0;
                        int rel = 0;                                // the first hit, counted from the register chunk's start
#pragma unroll
                        for (int g = 0; g < BQ_SLOTS / BQ_GROUP; ++g) {
                            if (g * BQ_GROUP * 64 >= rlen) break;
                            if (loaded == g) {                      // the first query to get here fills the group's registers
#pragma unroll
                                for (int t = 0; t < BQ_GROUP; ++t) {
                                    const int s = g * BQ_GROUP + t;
                                    const int k = 64 * s + opaque_v(lane);
                                    const int kc = rc + min(k, rlen - 1);
                                    const float vx = sx[kc], vy = sy[kc], vz = sz[kc];
                                    if (k < rlen) { px[s] = vx; py[s] = vy; pz[s] = vz; }
                                }
                                loaded = g + 1;
                            }
                            bool hit[BQ_GROUP];
                            unsigned long long mask[BQ_GROUP];
#pragma unroll
                            for (int t = 0; t < BQ_GROUP; ++t) {
                                const int s = g * BQ_GROUP + t;
                                hit[t] = dist2(qx - px[s], qy - py[s], qz - pz[s]) < radius2;
                                mask[t] = __ballot(hit[t]);
                            }
#pragma unroll
                            for (int t = 0; t < BQ_GROUP; ++t) {
                                if (mask[t] == 0ull) continue;      // wave-uniform
                                const int s = g * BQ_GROUP + t;
                                if (cnt == 0) rel = 64 * s + (int)__builtin_ctzll(mask[t]);   // a select, no branch
                                const int slot = cnt + (int)__builtin_amdgcn_mbcnt_hi(
                                                           (unsigned)(mask[t] >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((unsigned)mask[t], 0u));
                                if (hit[t] && slot < nsample)       // base pointer + 32-bit byte offset: one store, no 64-bit lane address
                                    *reinterpret_cast<int *>(reinterpret_cast<char *>(row) + (unsigned)slot * 4u) = opaque_v(point0) + 64 * s;
                                cnt += (int)__builtin_popcountll(mask[t]);
                            }
                            if (cnt >= nsample) break;              // once per group of slots
                        }
                        if (empty && cnt > 0) first = base + rc + rel;
                    }
                    if (last) {
                        finish(q, cnt, first);
                    } else if (lane == 0) {
                        cnt_of[q - q_begin] = cnt;
                        first_of[q - q_begin] = first;
                    }
                }
            }
        }
    }

    // a cloud without points under the zero-writing contract: every row of the tile is an empty ball
    if (n == 0)
        for (int q = q_begin + wave; q < q_end; q += WAVES) finish(q, 0, 0);
}


}  // namespace apn
