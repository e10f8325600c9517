// tile_map.h -- the layout of the tile map, ONE int32 blob per batch (nq = b * m queries, nq4 = nq rounded up to 4):
//   [0]                      tiles in use
//   [4, 4 + nq)              tq0      each tile's first query
//   [4 + nq4, + 32 nq)       rowinfo  a record per row (room for nq tiles of 32 rows; the tiles beyond [0] stay unwritten)
//   [.., + 32 nq)            rownn    each row's neighbour (idx[query][slot], so that the passes need no second dependent load)
//   [.., + b) [.., + b)      tcount, toff  per cloud: its tiles and its first tile
//   then the builder's scratch: qmeta (a packing record per query), tnq_local (uint16 per tile of a cloud), cnt8 (a byte
//   per query).  tile_map_ints = the blob's size.  Written by csrc/sa_wide_glue.hip; every reader takes its offsets here.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace apn {

__host__ __device__ inline int tile_map_rowinfo_off(int nq) { return 4 + ((nq + 3) & ~3); }
__host__ __device__ inline size_t tile_map_rownn_off(int nq) { return tile_map_rowinfo_off(nq) + (size_t)32 * nq; }
__host__ __device__ inline size_t tile_map_tcount_off(int nq) { return tile_map_rownn_off(nq) + (size_t)32 * nq; }
__host__ __device__ inline size_t tile_map_toff_off(int nq, int b) { return tile_map_tcount_off(nq) + b; }
__host__ __device__ inline size_t tile_map_qmeta_off(int nq, int b) { return tile_map_toff_off(nq, b) + b; }
__host__ __device__ inline size_t tile_map_tnq_local_off(int nq, int b) { return tile_map_qmeta_off(nq, b) + nq; }
__host__ __device__ inline size_t tile_map_cnt8_off(int nq, int b) {
    return tile_map_tnq_local_off(nq, b) + ((size_t)nq + 1) / 2;
}
// (a multiple of four ints: maps stacked back to back stay 16-byte aligned)
__host__ __device__ inline size_t tile_map_ints(int nq, int b) {
    return (tile_map_cnt8_off(nq, b) + ((size_t)nq + 3) / 4 + 8 + 3) & ~(size_t)3;
}

__host__ __device__ inline const unsigned *tile_map_rowinfo(const int *tmap, int nq) {
    return reinterpret_cast<const unsigned *>(tmap + tile_map_rowinfo_off(nq));
}
__host__ __device__ inline const int *tile_map_rownn(const int *tmap, int nq) {
    return tmap + tile_map_rowinfo_off(nq) + (size_t)32 * nq;
}

// what a reader of a finished map needs
struct TileMapView {
    const int *tq0;
    const unsigned *rowinfo;
    const int *rownn, *tcount, *toff;
    __host__ __device__ TileMapView(const int *tmap, int nq, int b)
        : tq0(tmap + 4), rowinfo(tile_map_rowinfo(tmap, nq)), rownn(tile_map_rownn(tmap, nq)),
          tcount(rownn + (size_t)32 * nq), toff(tcount + b) {}
};

}  // namespace apn
