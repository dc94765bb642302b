// What mst_pairs.hip (cis) and mst_pairs_trans.hip (trans) share: a workgroup of kThreads threads on a tile.
//
//   Binning: one workgroup trip of "rows with keys -> counters and far list".  A workgroup takes kRowsPerBlock consecutive rows
//   per trip, each wave kUnroll groups of 64.  The kernel says per lane and group whether the row is kept, its pixel's key and
//   the counter to add to (or "far"): bin_group merges runs of adjacent lanes with equal keys and lets the head lane add the run
//   length into `dense`; bin_far reserves the far-list slots with a returning atomic -- ONE for the whole workgroup (trans), or
//   one per wave (cis: LABBOOK has the measurement) -- and writes the (key, multiplicity) entries.  Returning atomics on one
//   address are served one after the other.
//
//   Compaction of a uint32 counter array: a tile of kTile consecutive counters per workgroup, kPerThread per thread; a count per
//   tile, a scan of the counts, a write pass whose emitter knows what a counter's index means.  No atomics anywhere.
#ifndef MST_PAIRS_TILES_H
#define MST_PAIRS_TILES_H

#include "mst_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 8;                          // groups of 64 consecutive rows per wave and trip
constexpr int kRowsPerBlock = kThreads * kUnroll;   // 2048 rows per workgroup and trip
constexpr int kPerThread = 8;                       // counters per thread of a compact tile
constexpr int kTile = kThreads * kPerThread;        // 2048 counters per workgroup

// ---- binning --------------------------------------------------------------------------------------------------------------
struct BinTrip {                                    // a lane's share of its wave's kUnroll groups
    long long key[kUnroll];
    uint32_t run[kUnroll];
    unsigned long long fars[kUnroll];               // wave-uniform: the head lanes of the group that go to the far list
    uint32_t n_far = 0;                             // wave-uniform
};

struct BinSlots {                                   // LDS, by trip parity: a fast wave's next trip leaves this trip's words alone
    uint32_t wave_far[2][kWaves];
    unsigned long long base[2];
};

// Group u of the wave's trip.  active: the lane has a row; ok: the row is kept; key: its pixel (>= 0); near: the pixel has a
// counter, dense[dense_at] -- any other goes to the far list.  Every lane of the wave calls, whatever its row.
__device__ __forceinline__ void bin_group(BinTrip &t, int u, bool active, bool ok, long long key, bool near, int64_t dense_at,
                                          uint32_t *__restrict__ dense) {
    const int lane = threadIdx.x & 63;
    const long long k = ok ? key : (active ? -1 : -2);
    const long long prev = __shfl_up(k, 1, 64);
    const bool start = lane == 0 || prev != k;      // the first lane of a run of equal keys
    const unsigned long long starts = __ballot(start);
    const bool head = start && ok;
    const unsigned long long above = lane == 63 ? 0ull : (starts >> (lane + 1));
    t.key[u] = k;
    t.run[u] = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
    const bool far = head && !near;
    if (head && near) atomicAdd(&dense[dense_at], t.run[u]);
    t.fars[u] = __ballot(far);
    t.n_far += (uint32_t)__popcll(t.fars[u]);
}

// The end of a trip: the far-list slots of the trip's head lanes, reserved with a returning atomic on *n_far, and the entries.
// kPerWorkgroup: ONE reservation for the workgroup -- the waves' counts go through LDS, thread 0 issues the atomic, the base comes
// back through LDS; EVERY wave of the workgroup then calls on EVERY trip (two barriers), rows or none.  Otherwise one reservation
// per wave that has a far entry: no LDS, no barrier, four times the returning atomics.  Nothing is written at or past far_cap;
// the count goes on, so the caller sees an overflow in *n_far > far_cap.
template <bool kPerWorkgroup>
__device__ __forceinline__ void bin_far(const BinTrip &t, BinSlots &s, int parity, int64_t *__restrict__ far_key,
                                        uint32_t *__restrict__ far_mult, int64_t far_cap, unsigned long long *__restrict__ n_far) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t slot;
    if (kPerWorkgroup) {
        if (lane == 0) s.wave_far[parity][wave] = t.n_far;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) all += s.wave_far[parity][w];
            s.base[parity] = all ? atomicAdd(n_far, (unsigned long long)all) : 0ull;
        }
        __syncthreads();
        if (!t.n_far) return;                       // wave-uniform, and behind both barriers
        slot = (int64_t)s.base[parity];
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
            if (w < wave) slot += s.wave_far[parity][w];
    } else {
        if (!t.n_far) return;                       // wave-uniform
        unsigned long long slot0 = 0;
        if (lane == 0) slot0 = atomicAdd(n_far, (unsigned long long)t.n_far);
        slot = (int64_t)__shfl(slot0, 0, 64);
    }
    const unsigned long long below = (1ull << lane) - 1ull;      // the lanes before this one
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        if ((t.fars[u] >> lane) & 1ull) {
            const int64_t mine = slot + __popcll(t.fars[u] & below);
            if (mine < far_cap) {
                far_key[mine] = t.key[u];
                far_mult[mine] = t.run[u];
            }
        }
        slot += __popcll(t.fars[u]);
    }
}

inline int grid_for(int64_t items, int64_t per_block, int64_t most) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > most ? most : g));
}

// ---- compaction -----------------------------------------------------------------------------------------------------------
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
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t s = wave_sum[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return v + before;
}

// the thread's kPerThread counters from `first` on and how many of them are not zero
__device__ __forceinline__ uint32_t load_tile(const uint32_t *__restrict__ dense, int64_t total, int64_t first, uint32_t c[kPerThread]) {
    if (first + kPerThread <= total && ((reinterpret_cast<uintptr_t>(dense + first) & 15) == 0)) {
        const uint4 a = *reinterpret_cast<const uint4 *>(dense + first);
        const uint4 b = *reinterpret_cast<const uint4 *>(dense + first + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w;
        c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) c[k] = first + k < total ? dense[first + k] : 0u;
    }
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) mine += c[k] != 0u;
    return mine;
}

// pass 1: non-zero counters per tile
__global__ __launch_bounds__(kThreads) void
compact_count_kernel(const uint32_t *__restrict__ dense, int64_t total, int64_t *__restrict__ tile_count) {
    __shared__ uint32_t wave_sum[kWaves];
    uint32_t c[kPerThread], all;
    block_scan(load_tile(dense, total, (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread, c), wave_sum, &all);
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

// pass 2: the records of each tile, behind those of the tiles before it.  Emit knows what a counter's index means: a thread
// with a record calls emit.seek(index of its first counter) once, then emit(output slot, index, count) per non-zero counter,
// indices ascending.
template <class Emit>
__global__ __launch_bounds__(kThreads) void
compact_write_kernel(const uint32_t *__restrict__ dense, int64_t total, const int64_t *__restrict__ tile_off, int64_t cap, Emit emit) {
    __shared__ uint32_t wave_sum[kWaves];
    uint32_t c[kPerThread], all;
    const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
    const uint32_t mine = load_tile(dense, total, first, c);
    const uint32_t incl = block_scan(mine, wave_sum, &all);
    if (!mine) return;
    int64_t o = tile_off[blockIdx.x] + (int64_t)(incl - mine);
    emit.seek(first);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k)
        if (c[k] != 0u && o < cap) emit(o++, first + k, c[k]);
}

inline uint64_t compact_workspace_bytes(int64_t total) { return (uint64_t)((total + kTile - 1) / kTile + 1) * sizeof(int64_t); }

// the non-zero counters of dense[total] -> records through `emit`, *n_out = how many there are (cap or not).  have_out: every
// output array of the emitter is there (needed when cap > 0).
template <class Emit>
int compact_counters(const char *who, const uint32_t *dense, int64_t total, Emit emit, bool have_out, int64_t cap, int64_t *n_out,
                     void *workspace, uint64_t workspace_bytes, void *stream) {
    if (total < 0 || cap < 0 || !n_out || (cap > 0 && !have_out)) return mst::fail(MST_E_ARG, "%s: bad argument", who);
    hipStream_t s = mst::as_stream(stream);
    if (total == 0) {
        MST_HIP(hipMemsetAsync(n_out, 0, sizeof(int64_t), s));
        return MST_OK;
    }
    const int64_t tiles = (total + kTile - 1) / kTile;
    if (!dense || !workspace || workspace_bytes < compact_workspace_bytes(total) || tiles > 0x7fffffff)
        return mst::fail(MST_E_ARG, "%s: bad argument", who);
    int64_t *tile_off = static_cast<int64_t *>(workspace);
    compact_count_kernel<<<(int)tiles, kThreads, 0, s>>>(dense, total, tile_off);
    MST_LAUNCH_CHECK();
    compact_scan_kernel<<<1, kThreads, 0, s>>>(tile_off, tiles, n_out);
    MST_LAUNCH_CHECK();
    compact_write_kernel<<<(int)tiles, kThreads, 0, s>>>(dense, total, tile_off, cap, emit);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

}  // namespace

#endif
