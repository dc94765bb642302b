// The tile helpers behind the compaction of a uint32 counter array (mst_pairs.hip: mst_pairs_compact; mst_pairs_trans.hip:
// mst_pairs_trans_compact): a workgroup of kThreads threads owns a tile of kTile consecutive counters, kPerThread per thread.
// The count per tile and the scan of the counts are the same for both; each file has its own write pass, which knows what a
// counter's index means.  No atomics anywhere.
#ifndef MST_PAIRS_TILES_H
#define MST_PAIRS_TILES_H

#include "mst_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;                       // counters per thread of a compact tile
constexpr int kTile = kThreads * kPerThread;        // 2048 counters per workgroup

// inclusive scan of one value per thread over the workgroup, thread order; *total = the workgroup's sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wave_sum, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const uint32_t s = wave_sum[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return v + before;
}

__device__ __forceinline__ void load_tile(const uint32_t *__restrict__ dense, int64_t total, int64_t first, uint32_t c[kPerThread]) {
    if (first + kPerThread <= total && ((reinterpret_cast<uintptr_t>(dense + first) & 15) == 0)) {
        const uint4 a = *reinterpret_cast<const uint4 *>(dense + first);
        const uint4 b = *reinterpret_cast<const uint4 *>(dense + first + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w;
        c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) c[k] = first + k < total ? dense[first + k] : 0u;
    }
}

// pass 1: non-zero counters per tile
__global__ __launch_bounds__(kThreads) void
compact_count_kernel(const uint32_t *__restrict__ dense, int64_t total, int64_t *__restrict__ tile_count) {
    __shared__ uint32_t wave_sum[kThreads / 64];
    uint32_t c[kPerThread];
    load_tile(dense, total, (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread, c);
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) mine += c[k] != 0u;
    uint32_t all;
    block_scan(mine, wave_sum, &all);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = all;
}

// the scan: tile_off[t] = records before tile t, tile_off[tiles] = all of them.  One workgroup; each thread adds a contiguous
// share of the tiles, the shares are scanned, then each thread writes its share's running sums.  In place over tile_count.
__global__ __launch_bounds__(kThreads) void compact_scan_kernel(int64_t *__restrict__ tile_off, int64_t tiles, int64_t *__restrict__ n_out) {
    __shared__ int64_t share_sum[kThreads];
    const int64_t per = (tiles + kThreads - 1) / kThreads;
    const int64_t t0 = (int64_t)threadIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    int64_t s = 0;
    for (int64_t t = t0; t < t1; ++t) s += tile_off[t];
    share_sum[threadIdx.x] = s;
    __syncthreads();
    int64_t before = 0;
    for (int k = 0; k < (int)threadIdx.x; ++k) before += share_sum[k];
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t c = tile_off[t];
        tile_off[t] = before;
        before += c;
    }
    if (threadIdx.x == kThreads - 1) {
        int64_t all = 0;
        for (int k = 0; k < kThreads; ++k) all += share_sum[k];
        tile_off[tiles] = all;
        *n_out = all;
    }
}

inline int grid_for(int64_t items, int64_t per_block, int64_t most) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > most ? most : g));
}

}  // namespace

#endif
