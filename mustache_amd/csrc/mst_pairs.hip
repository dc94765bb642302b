// Read pairs -> pixels on the device (mustache_amd/pairs.py states the rule; include/mustache_hip.h the entry points).
//
//   mst_pairs_bin      one grid-stride pass over (pos1, pos2): each lane bins its row or marks it dropped; runs of adjacent
//                      lanes of a wave that hold the same pixel are merged (sorted files: most rows), and only a run's head lane
//                      writes -- one no-return integer atomic add of the run length into the diagonal-major counter array
//                      [K][n] for a pixel with y - x < K, one (key, multiplicity) entry of the far list otherwise, whose slots
//                      come from one returning atomic per wave and trip
//   mst_pairs_compact  the non-zero counters -> (x, dist, count) records in position order: a count per workgroup, a scan of
//                      the counts, a write.  No atomics.
//
// Every sum is an integer sum: the counters, the far list as a multiset and both totals are the same from run to run and under
// any order of the rows.  (The far list's ORDER is not: its slots are handed out in arrival order; the caller sorts it.)
#include "mst_pairs_tiles.h"                        // kThreads, kTile, the tile count and its scan (shared with mst_pairs_trans.hip)

namespace {

// A wave takes kUnroll groups of 64 consecutive rows per trip and asks for the far-list slots of all of them with ONE returning
// atomic: every wave of the grid adds to the same address, and such adds are served one after the other (with one per group of
// 64 rows, 50 M rows spent 9.5 ms on 781 000 of them, whatever their order and the resolution: scripts/pairs_time.py).
constexpr int kUnroll = 8;
constexpr int kRowsPerBlock = kThreads * kUnroll;

__global__ __launch_bounds__(kThreads) void
pairs_bin_kernel(const int32_t *__restrict__ pos1, const int32_t *__restrict__ pos2, int64_t N, int32_t res, int32_t zero_based,
                 int64_t limit, int64_t n, int32_t K, uint32_t *__restrict__ dense, int64_t *__restrict__ far_key,
                 uint32_t *__restrict__ far_mult, int64_t far_cap, unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
    const int32_t lo = zero_based ? 0 : 1;
    const unsigned long long below = (1ull << lane) - 1ull;      // the lanes before this one
    unsigned long long dropped = 0;                 // wave-uniform
    // `base` is the first row of the wave's kUnroll groups: the trip count is the same for every lane of a wave, as the shuffles
    // and ballots need
    for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock + (int64_t)wave * (64 * kUnroll); base < N; base += stride) {
        long long key[kUnroll];
        uint32_t run[kUnroll];
        unsigned long long fars[kUnroll];
        uint32_t n_far = 0;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t e = base + u * 64 + lane;
            const bool active = e < N;
            int32_t x = 0, y = 0;
            bool ok = false;
            if (active) {
                const int32_t a = pos1[e], b = pos2[e];
                ok = a >= lo && b >= lo && (zero_based ? ((int64_t)a < limit && (int64_t)b < limit)
                                                       : ((int64_t)a <= limit && (int64_t)b <= limit));
                if (ok) {
                    const int32_t ba = (a - lo) / res, bb = (b - lo) / res;
                    x = ba < bb ? ba : bb;
                    y = ba < bb ? bb : ba;
                    ok = (int64_t)y < n;            // never written out of bounds, whatever limit the caller gave
                }
            }
            key[u] = ok ? (long long)x * n + y : (active ? -1 : -2);
            const long long prev = __shfl_up(key[u], 1, 64);
            const bool start = lane == 0 || prev != key[u];                 // the first lane of a run of equal keys
            const unsigned long long starts = __ballot(start);
            dropped += (unsigned long long)__popcll(__ballot(active && !ok));
            const bool head = start && ok;
            const unsigned long long above = lane == 63 ? 0ull : (starts >> (lane + 1));
            run[u] = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
            const int32_t dist = y - x;
            const bool far = head && dist >= K;
            if (head && !far) atomicAdd(&dense[(int64_t)dist * n + x], run[u]);
            fars[u] = __ballot(far);
            n_far += (uint32_t)__popcll(fars[u]);
        }
        if (n_far) {                                // wave-uniform
            unsigned long long slot0 = 0;
            if (lane == 0) slot0 = atomicAdd(&counters[0], (unsigned long long)n_far);
            int64_t slot = (int64_t)__shfl(slot0, 0, 64);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if ((fars[u] >> lane) & 1ull) {
                    const int64_t mine = slot + __popcll(fars[u] & below);
                    if (mine < far_cap) {           // the count goes on: the caller sees an overflow in counters[0] > far_cap
                        far_key[mine] = key[u];
                        far_mult[mine] = run[u];
                    }
                }
                slot += __popcll(fars[u]);
            }
        }
    }
    if (lane == 0 && dropped) atomicAdd(&counters[1], dropped);
}

// pass 2: the records of each tile, behind those of the tiles before it
__global__ __launch_bounds__(kThreads) void
compact_write_kernel(const uint32_t *__restrict__ dense, int64_t total, int64_t n, const int64_t *__restrict__ tile_off,
                     int32_t *__restrict__ out_x, int32_t *__restrict__ out_dist, uint32_t *__restrict__ out_count, int64_t cap) {
    __shared__ uint32_t wave_sum[kThreads / 64];
    uint32_t c[kPerThread];
    const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
    load_tile(dense, total, first, c);
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) mine += c[k] != 0u;
    uint32_t all;
    const uint32_t incl = block_scan(mine, wave_sum, &all);
    if (!mine) return;
    int64_t o = tile_off[blockIdx.x] + (int64_t)(incl - mine);
    int64_t dist = first / n, x = first - dist * n;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (c[k] != 0u && o < cap) {
            out_x[o] = (int32_t)x;
            out_dist[o] = (int32_t)dist;
            out_count[o] = c[k];
            ++o;
        }
        if (++x == n) {
            x = 0;
            ++dist;
        }
    }
}

}  // namespace

extern "C" int mst_pairs_bin(const int32_t *pos1, const int32_t *pos2, int64_t n_rows, int32_t res, int32_t zero_based, int64_t limit,
                             int64_t n, int32_t dense_diags, uint32_t *dense, int64_t *far_key, uint32_t *far_mult, int64_t far_cap,
                             uint64_t *counters, void *stream) {
    if (n_rows < 0 || res < 1 || n < 1 || dense_diags < 0 || far_cap < 0 || !counters || (n_rows > 0 && (!pos1 || !pos2)) ||
        (dense_diags > 0 && !dense) || (far_cap > 0 && (!far_key || !far_mult)) || (int64_t)dense_diags > n)
        return mst::fail(MST_E_ARG, "mst_pairs_bin: bad argument");
    if (n_rows == 0) return MST_OK;
    // at most 2048 workgroups: 32 waves for each of 256 compute units, each wave on trips of kUnroll * 64 rows
    pairs_bin_kernel<<<grid_for(n_rows, kRowsPerBlock, 2048), kThreads, 0, mst::as_stream(stream)>>>(
        pos1, pos2, n_rows, res, zero_based, limit, n, dense_diags, dense, far_key, far_mult, far_cap,
        reinterpret_cast<unsigned long long *>(counters));
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" uint64_t mst_pairs_compact_workspace_bytes(int32_t dense_diags, int64_t n) {
    if (dense_diags < 0 || n < 0) return 0;
    const int64_t total = (int64_t)dense_diags * n;
    return (uint64_t)((total + kTile - 1) / kTile + 1) * sizeof(int64_t);
}

extern "C" int mst_pairs_compact(const uint32_t *dense, int32_t dense_diags, int64_t n, int32_t *out_x, int32_t *out_dist,
                                 uint32_t *out_count, int64_t cap, int64_t *n_out, void *workspace, uint64_t workspace_bytes,
                                 void *stream) {
    if (dense_diags < 0 || n < 0 || cap < 0 || !n_out || (cap > 0 && (!out_x || !out_dist || !out_count)))
        return mst::fail(MST_E_ARG, "mst_pairs_compact: bad argument");
    hipStream_t s = mst::as_stream(stream);
    const int64_t total = (int64_t)dense_diags * n;
    if (total == 0) {
        MST_HIP(hipMemsetAsync(n_out, 0, sizeof(int64_t), s));
        return MST_OK;
    }
    const int64_t tiles = (total + kTile - 1) / kTile;
    if (!dense || !workspace || workspace_bytes < mst_pairs_compact_workspace_bytes(dense_diags, n) || tiles > 0x7fffffff)
        return mst::fail(MST_E_ARG, "mst_pairs_compact: bad argument");
    int64_t *tile_off = static_cast<int64_t *>(workspace);
    compact_count_kernel<<<(int)tiles, kThreads, 0, s>>>(dense, total, tile_off);
    MST_LAUNCH_CHECK();
    compact_scan_kernel<<<1, kThreads, 0, s>>>(tile_off, tiles, n_out);
    MST_LAUNCH_CHECK();
    compact_write_kernel<<<(int)tiles, kThreads, 0, s>>>(dense, total, n, tile_off, out_x, out_dist, out_count, cap);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
