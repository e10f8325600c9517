// voxel_grid.hip -- voxel-grid subsampling of STACKED clouds: partition the rows of coord (n,3) by (cloud, grid cell),
// number the voxels, group the rows by voxel, average per voxel.  The reference does this on the host (openpoints/
// dataset/data_util.py: voxelize; openpoints/cpp/subsampling).  Contract: include/adaptpoint_amd.h; design notes:
// DESIGN.md section 7o.
//
// apn_vg_voxelize is a fixed chain of launches; kernel boundaries are its only seams: no workgroup ever waits for
// another one (no look-back scan, no flags, no grid barrier), and every loop has a bound that is known at its entry.
//
//   vg_cell_kernel     cell = floor((double)coord / (double)voxel_size) and the row's cloud -> cell (n) int4; clears the
//                      table and the stats.
//   vg_insert_kernel   an open-addressing table of `slots` >= 2n ints that holds ROW INDICES: a row claims an empty slot
//                      by a 32-bit compare-and-swap, otherwise compares its (cloud, cell) with the occupant's and probes
//                      on -- at most `slots` probes, and a table of 2n slots never fills.  A later member lowers the slot
//                      to its own row by an integer atomicMin, so that the slot ends as the voxel's SMALLEST row, whatever
//                      the order of arrival.  Which slot a voxel gets depends on that order; nothing downstream does.
//                      A lane with the key of its wave's first active lane takes that lane's slot without touching memory.
//   vg_rep_kernel      rep[i] = the smallest row of i's voxel; flag[i] = (rep[i] == i).
//   vg_scan_*          exclusive scan of an int array in three launches: tile sums, ONE workgroup over the sums (at most
//                      65536 of them, never over the rows), add.  In place.
//   vg_number_kernel   voxel_of[i] = scan(flag)[rep[i]]: voxels numbered by their first row; new_offset.
//   vg_sort_kernel     stable LSD radix placement of the rows on voxel_of, 8 bits per pass, ceil(bits(n - 1) / 8) passes:
//                      a tile of 1024 rows ranks its keys by digit with wave ballots (8 ballots give a lane the mask of
//                      its peers), the (digit, tile) counts are scanned, the rows are placed.  O(n) per pass whatever the
//                      voxels' populations: a scene that falls into ONE voxel costs what any other scene costs.
//   vg_start_kernel / vg_count_kernel   start and count from the boundaries of the sorted keys (no atomics); count_max by
//                      an integer atomicMax.
//   vg_mean_kernel     one thread per (voxel, channel): sequential fp32 adds over the members in ascending row.
//
// Atomics: integer compare-and-swap / min / max / add only, each with an order-independent final value.  No float
// atomics.  Every store whose position was computed from data is bounds-checked.
#include "apn_common.h"

namespace apn {

constexpr int VG_THREADS = 256;
constexpr int VG_WAVES = VG_THREADS / APN_WAVE;
constexpr int VG_ROWS_MAX = 1 << 27;
constexpr int VG_EMPTY = 0x7fffffff;
constexpr int VG_GRID_MAX = 4096;                       // grid-stride kernels: blocks at the most
constexpr int VG_SCAN_PER = 8;                          // consecutive elements per thread
constexpr int VG_SCAN_TILE = VG_THREADS * VG_SCAN_PER;
constexpr int VG_TOP_THREADS = 1024;
constexpr int VG_TOP_MAX = 1 << 16;                     // tile sums the one-workgroup scan takes
constexpr int VG_SORT_ROUNDS = 4;
constexpr int VG_SORT_TILE = VG_THREADS * VG_SORT_ROUNDS;
constexpr int VG_SUBTILES = VG_WAVES * VG_SORT_ROUNDS;  // runs of 64 consecutive rows in a tile
constexpr int VG_DIGIT_BITS = 8;
constexpr int VG_DIGITS = 1 << VG_DIGIT_BITS;
constexpr int VG_MEAN_BATCH = 16;                       // members of a voxel loaded ahead of their adds
static_assert(VG_DIGITS == VG_THREADS, "vg_sort_kernel scans one digit per thread");

__device__ __forceinline__ unsigned vg_hash(int4 c) {
    unsigned h = (unsigned)c.x * 73856093u ^ (unsigned)c.y * 19349663u ^ (unsigned)c.z * 83492791u ^
                 (unsigned)c.w * 0x9E3779B1u;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// the first cloud c with i < offset[c]; a row at or past offset[b - 1] belongs to the last one.  At most 32 steps.
__device__ __forceinline__ int vg_cloud(int i, int b, const int *__restrict__ offset) {
    int lo = 0, hi = b - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (i < offset[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ bool vg_cell_axis(double x, double v, int &c) {
    const double q = __builtin_floor(x / v);
    const bool ok = q >= -2147483648.0 && q <= 2147483647.0;            // false for NaN and the infinities
    c = ok ? (int)q : 0;
    return ok;
}

template <typename T>
__global__ __launch_bounds__(VG_THREADS) void vg_cell_kernel(int b, int n, int slots, const T *__restrict__ coord, double vx,
                                                             double vy, double vz, const int *__restrict__ offset,
                                                             int4 *__restrict__ cell, int *__restrict__ table,
                                                             int *__restrict__ stats) {
    const long long gtid = (long long)blockIdx.x * VG_THREADS + threadIdx.x;
    const long long stride = (long long)gridDim.x * VG_THREADS;
    if (gtid < 3) stats[gtid] = 0;
    for (long long j = gtid; j < slots; j += stride) table[j] = VG_EMPTY;
    for (long long i = gtid; i < n; i += stride) {
        int4 c;
        bool ok = vg_cell_axis((double)coord[i * 3 + 0], vx, c.x);
        ok = vg_cell_axis((double)coord[i * 3 + 1], vy, c.y) && ok;
        ok = vg_cell_axis((double)coord[i * 3 + 2], vz, c.z) && ok;
        c.w = vg_cloud((int)i, b, offset);
        if (!ok) c = make_int4(0, 0, 0, -1);                            // a bad row: counted by vg_insert_kernel
        cell[i] = c;
    }
}

// the slot of row i's voxel, -1 if the table is full (impossible at slots >= 2n); the slot ends as the voxel's smallest row
__device__ __forceinline__ int vg_probe(int i, int n, int slots, int4 me, const int4 *__restrict__ cell, int *table) {
    const unsigned mask = (unsigned)slots - 1u;
    unsigned s = vg_hash(me) & mask;
    for (int probe = 0; probe < slots; ++probe) {                       // bounded by the table size: it cannot spin
        // look before claiming: whatever a slot has ever held besides VG_EMPTY is a member row of its voxel, so an
        // occupant seen by a plain (even stale) read decides as well as the one a compare-and-swap returns
        int cur = __hip_atomic_load(&table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == VG_EMPTY) cur = atomicCAS(&table[s], VG_EMPTY, i);
        if (cur == VG_EMPTY) return (int)s;                             // claimed
        const int4 o = cell[cur < n ? cur : n - 1];                     // cur is a row index: only rows are stored
        if (o.x == me.x && o.y == me.y && o.z == me.z && o.w == me.w) {
            if (i < cur) atomicMin(&table[s], i);                       // the slot only ever decreases
            return (int)s;
        }
        s = (s + 1u) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(VG_THREADS) void vg_insert_kernel(int n, int slots, const int4 *__restrict__ cell, int *table,
                                                               int *__restrict__ slot, int *__restrict__ stats) {
    const long long gtid = (long long)blockIdx.x * VG_THREADS + threadIdx.x;
    const long long stride = (long long)gridDim.x * VG_THREADS;
    int bad = 0;
    for (long long i = gtid; i < n; i += stride) {
        const int4 me = cell[i];
        bad += me.w < 0;
        // The rows of a wave's lanes ascend with the lane.  A lane with the (cloud, cell) of the wave's FIRST active lane
        // is in that lane's voxel with a higher row: it takes that lane's slot and touches no memory, so a crowded
        // voxel (a whole scene in one cell) costs one probe per wave, not one same-address atomic per row.
        // (the five reads come first, with every lane of the iteration active: inside a short-circuit && the "first
        // active lane" would be another one)
        const int i0 = __builtin_amdgcn_readfirstlane((int)i);
        const int x0 = __builtin_amdgcn_readfirstlane(me.x), y0 = __builtin_amdgcn_readfirstlane(me.y);
        const int z0 = __builtin_amdgcn_readfirstlane(me.z), w0 = __builtin_amdgcn_readfirstlane(me.w);
        const bool follow = ((int)i != i0) & (me.x == x0) & (me.y == y0) & (me.z == z0) & (me.w == w0);
        int found = -1;
        if (!follow) found = vg_probe((int)i, n, slots, me, cell, table);
        const int lead = __builtin_amdgcn_readfirstlane(found);        // the lanes are together again: the first one's slot
        found = follow ? lead : found;
        bad += found < 0;
        slot[i] = found;
    }
    if (bad) atomicAdd(&stats[2], bad);
}

__global__ __launch_bounds__(VG_THREADS) void vg_rep_kernel(int n, const int *__restrict__ table, int *__restrict__ slot_rep,
                                                            int *__restrict__ flag) {
    const long long stride = (long long)gridDim.x * VG_THREADS;
    for (long long i = (long long)blockIdx.x * VG_THREADS + threadIdx.x; i < n; i += stride) {
        const int s = slot_rep[i];
        int r = s >= 0 ? table[s] : (int)i;
        r = r < 0 || r > (int)i ? (int)i : r;
        slot_rep[i] = r;
        flag[i] = r == (int)i;
    }
}

// exclusive scan of one value per thread in thread order over the NW waves of a workgroup; total = their sum
template <int NW>
__device__ __forceinline__ int vg_block_exscan(int v, int *wsum, int &total) {
    const int lane = threadIdx.x & (APN_WAVE - 1), wave = threadIdx.x / APN_WAVE;
    int x = v;
#pragma unroll
    for (int d = 1; d < APN_WAVE; d <<= 1) {
        const int y = __shfl_up(x, d, APN_WAVE);
        if (lane >= d) x += y;
    }
    if (lane == APN_WAVE - 1) wsum[wave] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int t = wsum[w];
        base += w < wave ? t : 0;
        tot += t;
    }
    __syncthreads();                                                    // wsum may be written again
    total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(VG_THREADS) void vg_scan_sums_kernel(int count, const int *__restrict__ in,
                                                                  int *__restrict__ sums) {
    __shared__ int wsum[VG_WAVES];
    const long long e0 = (long long)blockIdx.x * VG_SCAN_TILE + threadIdx.x * VG_SCAN_PER;
    int s = 0;
#pragma unroll
    for (int e = 0; e < VG_SCAN_PER; ++e) s += e0 + e < count ? in[e0 + e] : 0;
    int total;
    vg_block_exscan<VG_WAVES>(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ONE workgroup over the tile sums (nsums <= 65536: 64 per thread at the most), in place; *total_out = their sum
__global__ __launch_bounds__(VG_TOP_THREADS) void vg_scan_top_kernel(int nsums, int *__restrict__ sums,
                                                                     int *__restrict__ total_out) {
    __shared__ int wsum[VG_TOP_THREADS / APN_WAVE];
    const int per = (nsums + VG_TOP_THREADS - 1) / VG_TOP_THREADS;
    const int lo = threadIdx.x * per;
    const int hi = lo + per < nsums ? lo + per : nsums;
    int s = 0;
    for (int j = lo; j < hi; ++j) s += sums[j];
    int total;
    int run = vg_block_exscan<VG_TOP_THREADS / APN_WAVE>(s, wsum, total);
    for (int j = lo; j < hi; ++j) {
        const int t = sums[j];
        sums[j] = run;
        run += t;
    }
    if (threadIdx.x == 0 && total_out) *total_out = total;
}

__global__ __launch_bounds__(VG_THREADS) void vg_scan_apply_kernel(int count, const int *in, const int *__restrict__ sums,
                                                                   int *out) {     // in may alias out
    __shared__ int wsum[VG_WAVES];
    const long long e0 = (long long)blockIdx.x * VG_SCAN_TILE + threadIdx.x * VG_SCAN_PER;
    int v[VG_SCAN_PER], s = 0;
#pragma unroll
    for (int e = 0; e < VG_SCAN_PER; ++e) {
        v[e] = e0 + e < count ? in[e0 + e] : 0;
        s += v[e];
    }
    int total;
    int run = sums[blockIdx.x] + vg_block_exscan<VG_WAVES>(s, wsum, total);
#pragma unroll
    for (int e = 0; e < VG_SCAN_PER; ++e) {
        if (e0 + e < count) out[e0 + e] = run;
        run += v[e];
    }
}

__global__ __launch_bounds__(VG_THREADS) void vg_number_kernel(int b, int n, const int *__restrict__ rep,
                                                               const int *__restrict__ dense,
                                                               const int *__restrict__ offset,
                                                               const int *__restrict__ stats, int *__restrict__ voxel_of,
                                                               int *__restrict__ new_offset) {
    const long long gtid = (long long)blockIdx.x * VG_THREADS + threadIdx.x;
    const long long stride = (long long)gridDim.x * VG_THREADS;
    const int m = stats[0];
    for (long long c = gtid; c < b; c += stride) {                      // voxels whose first row lies before the cloud's end
        const int end = offset[c];
        new_offset[c] = c == b - 1 || end >= n ? m : (end <= 0 ? 0 : dense[end]);
    }
    for (long long i = gtid; i < n; i += stride) voxel_of[i] = dense[rep[i]];
}

// One pass of the stable placement on bits [shift, shift + 8) of the keys.  A tile is 1024 consecutive rows = 16 runs of
// 64 (run = round * 4 + wave); a lane's rank among the lanes of its run with the same digit comes from 8 ballots.
// SCATTER = false: hist[digit * ntiles + tile] = the tile's count of the digit.  SCATTER = true: hist holds the exclusive
// scan of those counts, and row j goes to hist[..] + (its digit's count in the earlier runs of the tile) + rank.
template <bool SCATTER>
__global__ __launch_bounds__(VG_THREADS) void vg_sort_kernel(int n, int shift, int ntiles, const int *__restrict__ keys_in,
                                                             const int *__restrict__ vals_in, int *__restrict__ hist,
                                                             int *__restrict__ keys_out, int *__restrict__ vals_out) {
    __shared__ int cnt[VG_SUBTILES][VG_DIGITS];
    const int tid = threadIdx.x, lane = tid & (APN_WAVE - 1), wave = tid / APN_WAVE;
    const int tile = blockIdx.x;
    for (int e = tid; e < VG_SUBTILES * VG_DIGITS; e += VG_THREADS) (&cnt[0][0])[e] = 0;
    __syncthreads();
    int key[VG_SORT_ROUNDS], rank[VG_SORT_ROUNDS];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < VG_SORT_ROUNDS; ++r) {
        const long long j = (long long)tile * VG_SORT_TILE + r * VG_THREADS + tid;
        const bool live = j < n;
        key[r] = live ? keys_in[j] : 0;
        const unsigned d = ((unsigned)key[r] >> shift) & (VG_DIGITS - 1);
        unsigned long long peers = __builtin_amdgcn_ballot_w64(live);
#pragma unroll
        for (int bit = 0; bit < VG_DIGIT_BITS; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long set = __builtin_amdgcn_ballot_w64(one);
            peers &= one ? set : ~set;
        }
        rank[r] = __builtin_popcountll(peers & below);
        if (live && rank[r] == 0) cnt[r * VG_WAVES + wave][d] = __builtin_popcountll(peers);
    }
    __syncthreads();
    {                                                                   // thread = digit: exclusive scan over the runs
        int run = 0;
#pragma unroll
        for (int s = 0; s < VG_SUBTILES; ++s) {
            const int c = cnt[s][tid];
            cnt[s][tid] = run;
            run += c;
        }
        if (!SCATTER) hist[(size_t)tid * ntiles + tile] = run;
    }
    if (SCATTER) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < VG_SORT_ROUNDS; ++r) {
            const long long j = (long long)tile * VG_SORT_TILE + r * VG_THREADS + tid;
            if (j >= n) continue;
            const unsigned d = ((unsigned)key[r] >> shift) & (VG_DIGITS - 1);
            const int pos = hist[(size_t)d * ntiles + tile] + cnt[r * VG_WAVES + wave][d] + rank[r];
            if ((unsigned)pos < (unsigned)n) {
                keys_out[pos] = key[r];
                vals_out[pos] = vals_in ? vals_in[j] : (int)j;
            }
        }
    }
}

// keys = voxel_of in idx_sort order (non-decreasing): a voxel starts where the key changes
__global__ __launch_bounds__(VG_THREADS) void vg_start_kernel(int n, const int *__restrict__ keys, int *__restrict__ start) {
    const long long stride = (long long)gridDim.x * VG_THREADS;
    for (long long j = (long long)blockIdx.x * VG_THREADS + threadIdx.x; j < n; j += stride) {
        const int k = keys[j];
        if ((j == 0 || keys[j - 1] != k) && (unsigned)k < (unsigned)n) start[k] = (int)j;
    }
}

__global__ __launch_bounds__(VG_THREADS) void vg_count_kernel(int n, const int *__restrict__ start, int *__restrict__ count,
                                                              int *__restrict__ stats) {
    const long long stride = (long long)gridDim.x * VG_THREADS;
    int m = stats[0];
    m = m < 0 ? 0 : (m > n ? n : m);
    unsigned most = 0;
    for (long long v = (long long)blockIdx.x * VG_THREADS + threadIdx.x; v < m; v += stride) {
        const int c = (v + 1 < m ? start[v + 1] : n) - start[v];
        count[v] = c;
        most = c > 0 && (unsigned)c > most ? (unsigned)c : most;
    }
    most = wave_max_u32(most);                                          // every lane is here
    if ((threadIdx.x & (APN_WAVE - 1)) == 0 && most) atomicMax(&stats[1], (int)most);
}

__device__ __forceinline__ int vg_clamp(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }

// the correctly rounded fp32 quotient of an fp32 by a count below 2^27
__device__ __forceinline__ float vg_div(float s, int count) { return (float)((double)s / (double)count); }

__global__ __launch_bounds__(VG_THREADS) void vg_mean_kernel(long long total, int n, int c, const float *__restrict__ values,
                                                             const int *__restrict__ idx_sort,
                                                             const int *__restrict__ start, const int *__restrict__ count,
                                                             float *__restrict__ out) {
    const long long stride = (long long)gridDim.x * VG_THREADS;
    for (long long e = (long long)blockIdx.x * VG_THREADS + threadIdx.x; e < total; e += stride) {
        const long long v = e / c;
        const int ch = (int)(e - v * c);
        long long st = start[v];
        st = st < 0 ? 0 : (st > n ? n : st);
        long long p = count[v];
        p = p < 0 ? 0 : (st + p > n ? n - st : p);
        if (p == 0) {
            out[e] = 0.0f;
            continue;
        }
        const int *members = idx_sort + st;
        float s = values[(size_t)vg_clamp(members[0], n) * c + ch];
        long long j = 1;
        for (; j + VG_MEAN_BATCH <= p; j += VG_MEAN_BATCH) {            // a batch's loads fly together; the adds stay in order
            float t[VG_MEAN_BATCH];
#pragma unroll
            for (int u = 0; u < VG_MEAN_BATCH; ++u) t[u] = values[(size_t)vg_clamp(members[j + u], n) * c + ch];
#pragma unroll
            for (int u = 0; u < VG_MEAN_BATCH; ++u) s += t[u];
        }
        for (; j < p; ++j) s += values[(size_t)vg_clamp(members[j], n) * c + ch];
        out[e] = vg_div(s, (int)p);
    }
}

__global__ __launch_bounds__(VG_THREADS) void vg_mean_grad_kernel(long long total, int m, int c,
                                                                  const float *__restrict__ grad_out,
                                                                  const int *__restrict__ voxel_of,
                                                                  const int *__restrict__ count,
                                                                  float *__restrict__ grad_values) {
    const long long stride = (long long)gridDim.x * VG_THREADS;
    for (long long e = (long long)blockIdx.x * VG_THREADS + threadIdx.x; e < total; e += stride) {
        const long long i = e / c;
        const int ch = (int)(e - i * c);
        const int v = vg_clamp(voxel_of[i], m);
        const int p = count[v];
        grad_values[e] = vg_div(grad_out[(size_t)v * c + ch], p > 0 ? p : 1);
    }
}

}  // namespace apn

using namespace apn;

static inline unsigned vg_blocks(long long total) {
    const long long nb = (total + VG_THREADS - 1) / VG_THREADS;
    return (unsigned)(nb < 1 ? 1 : (nb < VG_GRID_MAX ? nb : VG_GRID_MAX));     // the kernels stride over what is left
}

static inline int vg_slots(int n) {
    int s = 256;
    while (s < 2 * n) s <<= 1;                                          // n < 2^27: at most 2^28
    return s;
}

static inline int vg_sort_tiles(int n) { return (n + VG_SORT_TILE - 1) / VG_SORT_TILE; }
static inline int vg_scan_tiles(int count) { return (count + VG_SCAN_TILE - 1) / VG_SCAN_TILE; }

static inline int vg_passes(int n) {
    int bits = 1;
    while (bits < 27 && (1 << bits) < n) ++bits;                        // voxel numbers are below n
    return (bits + VG_DIGIT_BITS - 1) / VG_DIGIT_BITS;
}

// the scratch of apn_vg_voxelize, in ints: {cell 4n | table | rep n | dense n | hist | sums}; the sort's three
// buffers of n reuse the cell region, which is dead once the rows have their slots
struct VgLayout {
    long long cell, table, rep, dense, hist, sums, total;
    int slots, hist_ints, sums_ints;
};

static inline VgLayout vg_layout(int n) {
    VgLayout L;
    const auto up = [](long long x) { return (x + 63) / 64 * 64; };     // 256-byte pieces
    L.slots = vg_slots(n);
    L.hist_ints = VG_DIGITS * vg_sort_tiles(n);
    const int longest = L.hist_ints > n ? L.hist_ints : n;
    L.sums_ints = vg_scan_tiles(longest);
    L.cell = 0;
    L.table = up(4ll * n);
    L.rep = L.table + L.slots;
    L.dense = L.rep + up(n);
    L.hist = L.dense + up(n);
    L.sums = L.hist + up(L.hist_ints);
    L.total = L.sums + up(L.sums_ints);
    return L;
}

static inline bool vg_rows(int n) { return n >= 0 && n < VG_ROWS_MAX; }

extern "C" int apn_vg_scratch_ints(int n) {
    if (!vg_rows(n)) return 0;
    return (int)vg_layout(n).total;                                     // below 11 n + 2^17 < 2^31
}

// exclusive scan of data[0 .. count) in place: three launches
static void vg_scan(int count, int *data, int *sums, int *total_out, hipStream_t st) {
    const int tiles = vg_scan_tiles(count);
    hipLaunchKernelGGL(vg_scan_sums_kernel, dim3(tiles), dim3(VG_THREADS), 0, st, count, data, sums);
    hipLaunchKernelGGL(vg_scan_top_kernel, dim3(1), dim3(VG_TOP_THREADS), 0, st, tiles, sums, total_out);
    hipLaunchKernelGGL(vg_scan_apply_kernel, dim3(tiles), dim3(VG_THREADS), 0, st, count, data, sums, data);
}

extern "C" int apn_vg_voxelize(int b, int n, int is_double, const void *coord, double vx, double vy, double vz,
                               const int *offset, int *scratch, int *voxel_of, int *count, int *start, int *idx_sort,
                               int *new_offset, int *stats, void *stream) {
    const auto size_ok = [](double v) { return v > 0.0 && v <= 1.79769313486231570e308; };
    if (b < 1 || !vg_rows(n) || (is_double != 0 && is_double != 1) || !size_ok(vx) || !size_ok(vy) || !size_ok(vz))
        return APN_EINVAL;
    if (n == 0) return APN_OK;
    if (!coord || !offset || !scratch || !voxel_of || !count || !start || !idx_sort || !new_offset || !stats)
        return APN_EINVAL;
    if (((uintptr_t)scratch & 15u) != 0) return APN_EINVAL;              // the cells are int4
    const VgLayout L = vg_layout(n);
    if (L.sums_ints > VG_TOP_MAX) return APN_EINVAL;                     // cannot happen below 2^27 rows
    hipStream_t st = (hipStream_t)stream;
    int4 *cell = reinterpret_cast<int4 *>(scratch + L.cell);
    int *table = scratch + L.table, *rep = scratch + L.rep, *dense = scratch + L.dense, *hist = scratch + L.hist;
    int *sums = scratch + L.sums;
    const dim3 rows(vg_blocks(n)), block(VG_THREADS);
    if (is_double)
        hipLaunchKernelGGL(vg_cell_kernel<double>, dim3(vg_blocks(L.slots)), block, 0, st, b, n, L.slots,
                           (const double *)coord, vx, vy, vz, offset, cell, table, stats);
    else
        hipLaunchKernelGGL(vg_cell_kernel<float>, dim3(vg_blocks(L.slots)), block, 0, st, b, n, L.slots,
                           (const float *)coord, vx, vy, vz, offset, cell, table, stats);
    hipLaunchKernelGGL(vg_insert_kernel, rows, block, 0, st, n, L.slots, cell, table, rep, stats);
    hipLaunchKernelGGL(vg_rep_kernel, rows, block, 0, st, n, table, rep, dense);
    vg_scan(n, dense, sums, stats, st);                                  // stats[0] = m
    hipLaunchKernelGGL(vg_number_kernel, rows, block, 0, st, b, n, rep, dense, offset, stats, voxel_of, new_offset);
    // the placement: keys and rows ping-pong through the dead cell region; the last pass writes idx_sort
    int *kbuf[2] = {scratch + L.cell, scratch + L.cell + n};
    int *vbuf = scratch + L.cell + 2ll * n;
    const int passes = vg_passes(n), ntiles = vg_sort_tiles(n);
    const int *keys_in = voxel_of, *vals_in = nullptr;
    for (int p = 0; p < passes; ++p) {
        int *keys_out = kbuf[p & 1];
        int *vals_out = ((passes - 1 - p) & 1) ? vbuf : idx_sort;
        hipLaunchKernelGGL(vg_sort_kernel<false>, dim3(ntiles), block, 0, st, n, p * VG_DIGIT_BITS, ntiles, keys_in, vals_in,
                           hist, (int *)nullptr, (int *)nullptr);
        vg_scan(L.hist_ints, hist, sums, nullptr, st);
        hipLaunchKernelGGL(vg_sort_kernel<true>, dim3(ntiles), block, 0, st, n, p * VG_DIGIT_BITS, ntiles, keys_in, vals_in,
                           hist, keys_out, vals_out);
        keys_in = keys_out;
        vals_in = vals_out;
    }
    hipLaunchKernelGGL(vg_start_kernel, rows, block, 0, st, n, keys_in, start);
    hipLaunchKernelGGL(vg_count_kernel, rows, block, 0, st, n, start, count, stats);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

static inline bool vg_feat(int n, int m, int c) { return vg_rows(n) && m >= 0 && m <= n && c >= 1 && c <= 65536; }

extern "C" int apn_vg_mean_fwd(int n, int m, int c, const float *values, const int *idx_sort, const int *start,
                               const int *count, float *out, void *stream) {
    if (!vg_feat(n, m, c)) return APN_EINVAL;
    if (m == 0) return APN_OK;
    if (!values || !idx_sort || !start || !count || !out) return APN_EINVAL;
    const long long total = (long long)m * c;
    hipLaunchKernelGGL(vg_mean_kernel, dim3(vg_blocks(total)), dim3(VG_THREADS), 0, (hipStream_t)stream, total, n, c, values,
                       idx_sort, start, count, out);
    APN_LAUNCH_CHECK();
    return APN_OK;
}

extern "C" int apn_vg_mean_bwd(int n, int m, int c, const float *grad_out, const int *voxel_of, const int *count,
                               float *grad_values, void *stream) {
    if (!vg_feat(n, m, c)) return APN_EINVAL;
    if (n == 0 || m == 0) return APN_OK;
    if (!grad_out || !voxel_of || !count || !grad_values) return APN_EINVAL;
    const long long total = (long long)n * c;
    hipLaunchKernelGGL(vg_mean_grad_kernel, dim3(vg_blocks(total)), dim3(VG_THREADS), 0, (hipStream_t)stream, total, m, c,
                       grad_out, voxel_of, count, grad_values);
    APN_LAUNCH_CHECK();
    return APN_OK;
}
