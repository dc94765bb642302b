// What mst_coarsen.hip (one chromosome's records) and mst_coarsen_pairs.hip (the trans records of many pairs) share: the rule
// for a count, the combining of adjacent lanes with equal keys -- a segmented suffix sum over the wave -- and the first pass of
// the compaction of 64-bit counters.
#ifndef MST_COARSEN_TILES_H
#define MST_COARSEN_TILES_H

#include "mst_pairs_tiles.h"                        // block_scan, compact_scan_kernel, compact_workspace_bytes, grid_for

namespace {

constexpr int64_t kMaxCount = 0xFFFFFFFFll;
constexpr uint32_t kLinear = 8;                     // runs up to this long are summed lane by lane

// a count as the kernel takes it: the integer, or -1 for what is no integer in [0, 2^32 - 1] (mst_thin.hip's rule)
__device__ __forceinline__ int64_t count_of(int64_t v) { return v < 0 || v > kMaxCount ? -1 : v; }
__device__ __forceinline__ int64_t count_of(double v) {
    return v >= 0.0 && v <= 4294967295.0 && v == floor(v) ? (int64_t)v : -1;          // NaN fails the first compare
}
__device__ __forceinline__ int64_t count_of(float v) { return count_of((double)v); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lane l receives lane l + 1's value, lane 63 receives 0: a DPP wave shift per 32-bit half, no LDS traffic
__device__ __forceinline__ unsigned long long from_next_lane(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x130, 0xf, 0xf, true);          // wave_shl:1
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x130, 0xf, 0xf, true);
    return ((unsigned long long)hi << 32) | lo;
}

// The sum of c over the lanes [lane, lane + rest) -- `rest` = the lanes left of this lane's run, itself included (>= 1, and
// lane + rest <= 64).  Every lane of the wave calls.
__device__ __forceinline__ unsigned long long run_suffix_sum(unsigned long long c, uint32_t rest) {
    uint32_t longest = rest;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)longest, o, 64);
        longest = other > longest ? other : longest;
    }
    unsigned long long sum = c;
    if (longest <= kLinear) {                       // wave-uniform
        unsigned long long moving = c;
        for (uint32_t j = 1; j < longest; ++j) {
            moving = from_next_lane(moving);        // the count of lane + j
            if (j < rest) sum += moving;
        }
    } else {
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {     // sum covers [lane, min(lane + 2 o, lane + rest))
            const unsigned long long other = __shfl_down(sum, o, 64);
            if (o < rest) sum += other;
        }
    }
    return sum;
}

// ---- compaction of 64-bit counters ----------------------------------------------------------------------------------------
// the thread's kPerThread counters from `first` on and how many of them are not zero
__device__ __forceinline__ uint32_t load_tile64(const unsigned long long *__restrict__ dense, int64_t total, int64_t first,
                                                unsigned long long c[kPerThread]) {
    if (first + kPerThread <= total && ((reinterpret_cast<uintptr_t>(dense + first) & 15) == 0)) {
#pragma unroll
        for (int k = 0; k < kPerThread; k += 2) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(dense + first + k);
            c[k] = a.x;
            c[k + 1] = a.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) c[k] = first + k < total ? dense[first + k] : 0ull;
    }
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) mine += c[k] != 0ull;
    return mine;
}

__global__ __launch_bounds__(kThreads) void
compact64_count_kernel(const unsigned long long *__restrict__ dense, int64_t total, int64_t *__restrict__ tile_count) {
    __shared__ uint32_t wave_sums[kWaves];
    unsigned long long c[kPerThread];
    uint32_t all;
    block_scan(load_tile64(dense, total, (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread, c), wave_sums, &all);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = all;
}

}  // namespace

#endif
