// Trans read pairs -> per-pair pixels on the device, all chromosome pairs of the genome in one pass (mustache_amd/pairs.py states
// the rule; include/mustache_hip.h the entry points).
//
// The rows arrive pair-major: pair p = (a, b), a < b in table order, owns rows [seg_off[p], seg_off[p + 1]), the position on a in
// posA and the position on b in posB.  A pixel's key is cell_off[p] + x * n_b + y (x = bin on a, y = bin on b; cell_off = the
// running sum of n_a * n_b over the pairs before p): unique across pairs, and ascending keys are pair-major.
//
//   mst_pairs_bin_trans      one grid-stride pass over the rows: each lane finds its row's pair (wave-uniform when lanes 0 and 63
//                            lie in one segment, a per-lane binary search of seg_off otherwise), bins its row or marks it
//                            dropped; runs of adjacent lanes with equal keys are merged as in mst_pairs_bin and only a run's head
//                            lane writes -- one no-return integer atomic add of the run length into dense[key] for
//                            key < dense_cells, one (key, multiplicity) entry of the far list otherwise.  The far list's slots are
//                            reserved ONCE PER WORKGROUP AND TRIP: the waves' counts go through LDS, thread 0 issues one
//                            returning atomic, the base is broadcast (returning atomics on one address are served one after the
//                            other: DESIGN section 8b).
//   mst_pairs_trans_compact  the non-zero counters -> (key, count) in ascending key order: count per tile, scan, write
//                            (mst_pairs_tiles.h).  No atomics.
//   mst_pairs_trans_decode   ascending keys + int64 counts -> (x int32, y int32, v float64): a binary search of cell_off per key.
//
// Every sum is an integer sum: the counters, the far list as a multiset and the dropped counts are the same from run to run and
// under any order of the rows within their pairs.
#include "mst_pairs_tiles.h"

namespace {

constexpr int kUnroll = 8;                          // groups of 64 consecutive rows per wave and trip
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerBlock = kThreads * kUnroll;   // 2048 rows per workgroup and trip

// the largest p in [lo, P) with off[p] <= e; off[lo] <= e is the caller's word.  With empty segments (equal offsets) that is the
// one that holds e.
__device__ __forceinline__ int32_t find_segment(const int64_t *__restrict__ off, int32_t lo, int32_t P, int64_t e) {
    int32_t hi = P;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void
pairs_bin_trans_kernel(const int32_t *__restrict__ posA, const int32_t *__restrict__ posB, int64_t N,
                       const int64_t *__restrict__ seg_off, int32_t P, const int64_t *__restrict__ limA,
                       const int64_t *__restrict__ limB, const int64_t *__restrict__ nA, const int64_t *__restrict__ nB,
                       const int64_t *__restrict__ cell_off, int32_t res, int32_t zero_based, int64_t dense_cells,
                       uint32_t *__restrict__ dense, int64_t *__restrict__ far_key, uint32_t *__restrict__ far_mult,
                       int64_t far_cap, unsigned long long *__restrict__ n_far_out, unsigned long long *__restrict__ dropped) {
    __shared__ uint32_t wave_far[2][kWaves];        // by trip parity: a fast wave's next trip leaves this trip's counts alone
    __shared__ unsigned long long slot_base[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
    const int32_t lo = zero_based ? 0 : 1;
    const unsigned long long below = (1ull << lane) - 1ull;      // the lanes before this one
    int32_t p_wave = 0;                             // wave-uniform: the pair of the wave's first row; rows only go forward
    int parity = 0;
    // the trip count is the same for every wave of a workgroup (the barriers need that) and for every lane of a wave (the
    // shuffles and ballots do)
    for (int64_t block_base = (int64_t)blockIdx.x * kRowsPerBlock; block_base < N; block_base += stride, parity ^= 1) {
        const int64_t base = block_base + (int64_t)wave * (64 * kUnroll);
        long long key[kUnroll];
        uint32_t run[kUnroll];
        unsigned long long fars[kUnroll];
        uint32_t n_far = 0;
        if (base < N) p_wave = __builtin_amdgcn_readfirstlane(find_segment(seg_off, p_wave, P, base));
        int32_t p_group = p_wave;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t e0 = base + u * 64, e = e0 + lane;
            const bool active = e < N;
            bool ok = false;
            long long k = active ? -1 : -2;
            if (e0 < N) {                           // wave-uniform
                const int64_t last = e0 + 63 < N ? e0 + 63 : N - 1;
                p_group = __builtin_amdgcn_readfirstlane(find_segment(seg_off, p_group, P, e0));
                const bool one_pair = p_group + 1 >= P || last < seg_off[p_group + 1];       // lanes 0 and 63 in one segment
                const int32_t p = one_pair ? p_group : (active ? find_segment(seg_off, p_group, P, e) : p_group);
                if (active) {
                    const int32_t a = posA[e], b = posB[e];
                    const int64_t la = limA[p], lb = limB[p], na = nA[p], nb = nB[p];
                    ok = a >= lo && b >= lo && (zero_based ? ((int64_t)a < la && (int64_t)b < lb)
                                                           : ((int64_t)a <= la && (int64_t)b <= lb));
                    if (ok) {
                        const int64_t x = (a - lo) / res, y = (b - lo) / res;
                        ok = x < na && y < nb;      // never a key outside the pair's cells, whatever limits the caller gave
                        const long long cell = cell_off[p] + x * nb + y;
                        ok = ok && cell >= 0;       // (a table with a negative entry: dropped, not written)
                        if (ok) k = cell;
                    }
                }
                if (one_pair) {
                    const uint32_t lost = (uint32_t)__popcll(__ballot(active && !ok));
                    if (lost && lane == 0) atomicAdd(&dropped[p_group], (unsigned long long)lost);
                } else if (active && !ok) {
                    atomicAdd(&dropped[p], 1ull);
                }
            }
            key[u] = k;
            const long long prev = __shfl_up(k, 1, 64);
            const bool start = lane == 0 || prev != k;                      // the first lane of a run of equal keys
            const unsigned long long starts = __ballot(start);
            const bool head = start && ok;
            const unsigned long long above = lane == 63 ? 0ull : (starts >> (lane + 1));
            run[u] = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
            const bool far = head && k >= dense_cells;
            if (head && !far) atomicAdd(&dense[k], run[u]);
            fars[u] = __ballot(far);
            n_far += (uint32_t)__popcll(fars[u]);
        }
        // one returning atomic per workgroup and trip
        if (lane == 0) wave_far[parity][wave] = n_far;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) all += wave_far[parity][w];
            slot_base[parity] = all ? atomicAdd(n_far_out, (unsigned long long)all) : 0ull;
        }
        __syncthreads();
        if (n_far) {                                // wave-uniform
            int64_t slot = (int64_t)slot_base[parity];
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
                if (w < wave) slot += wave_far[parity][w];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if ((fars[u] >> lane) & 1ull) {
                    const int64_t mine = slot + __popcll(fars[u] & below);
                    if (mine < far_cap) {           // the count goes on: the caller sees an overflow in *n_far > far_cap
                        far_key[mine] = key[u];
                        far_mult[mine] = run[u];
                    }
                }
                slot += __popcll(fars[u]);
            }
        }
    }
}

// pass 2 of the compaction: the (key, count) of each tile's non-zero counters, behind those of the tiles before it
__global__ __launch_bounds__(kThreads) void
trans_compact_write_kernel(const uint32_t *__restrict__ dense, int64_t total, const int64_t *__restrict__ tile_off,
                           int64_t *__restrict__ out_key, uint32_t *__restrict__ out_count, int64_t cap) {
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
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (c[k] != 0u && o < cap) {
            out_key[o] = first + k;
            out_count[o] = c[k];
            ++o;
        }
    }
}

__global__ __launch_bounds__(kThreads) void
trans_decode_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ counts, int64_t N,
                    const int64_t *__restrict__ cell_off, const int64_t *__restrict__ nB, int32_t P, int32_t *__restrict__ out_x,
                    int32_t *__restrict__ out_y, double *__restrict__ out_v) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += stride) {
        const int64_t key = keys[i];
        const int32_t p = find_segment(cell_off, 0, P, key);
        const int64_t cell = key - cell_off[p], nb = nB[p], x = cell / nb;
        out_x[i] = (int32_t)x;
        out_y[i] = (int32_t)(cell - x * nb);
        out_v[i] = (double)counts[i];               // int64 -> float64 directly: exact below 2^53
    }
}

}  // namespace

extern "C" int mst_pairs_bin_trans(const int32_t *posA, const int32_t *posB, int64_t n_rows, const int64_t *seg_off, int32_t n_pairs,
                                   const int64_t *limA, const int64_t *limB, const int64_t *nA, const int64_t *nB,
                                   const int64_t *cell_off, int32_t res, int32_t zero_based, int64_t dense_cells, uint32_t *dense,
                                   int64_t *far_key, uint32_t *far_mult, int64_t far_cap, uint64_t *n_far, uint64_t *dropped,
                                   void *stream) {
    if (n_rows < 0 || n_pairs < 0 || res < 1 || dense_cells < 0 || far_cap < 0) return mst::fail(MST_E_ARG, "mst_pairs_bin_trans: bad argument");
    if (n_rows == 0 || n_pairs == 0) return MST_OK;
    if (!posA || !posB || !seg_off || !limA || !limB || !nA || !nB || !cell_off || !n_far || !dropped || (dense_cells > 0 && !dense) ||
        (far_cap > 0 && (!far_key || !far_mult)))
        return mst::fail(MST_E_ARG, "mst_pairs_bin_trans: bad argument");
    // at most 2048 workgroups: 32 waves for each of 256 compute units, each workgroup on trips of 2048 rows
    pairs_bin_trans_kernel<<<grid_for(n_rows, kRowsPerBlock, 2048), kThreads, 0, mst::as_stream(stream)>>>(
        posA, posB, n_rows, seg_off, n_pairs, limA, limB, nA, nB, cell_off, res, zero_based, dense_cells, dense, far_key, far_mult,
        far_cap, reinterpret_cast<unsigned long long *>(n_far), reinterpret_cast<unsigned long long *>(dropped));
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" uint64_t mst_pairs_trans_compact_workspace_bytes(int64_t dense_cells) {
    if (dense_cells < 0) return 0;
    return (uint64_t)((dense_cells + kTile - 1) / kTile + 1) * sizeof(int64_t);
}

extern "C" int mst_pairs_trans_compact(const uint32_t *dense, int64_t dense_cells, int64_t *out_key, uint32_t *out_count, int64_t cap,
                                       int64_t *n_out, void *workspace, uint64_t workspace_bytes, void *stream) {
    if (dense_cells < 0 || cap < 0 || !n_out || (cap > 0 && (!out_key || !out_count)))
        return mst::fail(MST_E_ARG, "mst_pairs_trans_compact: bad argument");
    hipStream_t s = mst::as_stream(stream);
    if (dense_cells == 0) {
        MST_HIP(hipMemsetAsync(n_out, 0, sizeof(int64_t), s));
        return MST_OK;
    }
    const int64_t tiles = (dense_cells + kTile - 1) / kTile;
    if (!dense || !workspace || workspace_bytes < mst_pairs_trans_compact_workspace_bytes(dense_cells) || tiles > 0x7fffffff)
        return mst::fail(MST_E_ARG, "mst_pairs_trans_compact: bad argument");
    int64_t *tile_off = static_cast<int64_t *>(workspace);
    compact_count_kernel<<<(int)tiles, kThreads, 0, s>>>(dense, dense_cells, tile_off);
    MST_LAUNCH_CHECK();
    compact_scan_kernel<<<1, kThreads, 0, s>>>(tile_off, tiles, n_out);
    MST_LAUNCH_CHECK();
    trans_compact_write_kernel<<<(int)tiles, kThreads, 0, s>>>(dense, dense_cells, tile_off, out_key, out_count, cap);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_pairs_trans_decode(const int64_t *keys, const int64_t *counts, int64_t n, const int64_t *cell_off, const int64_t *nB,
                                      int32_t n_pairs, int32_t *out_x, int32_t *out_y, double *out_v, void *stream) {
    if (n < 0 || n_pairs < 0) return mst::fail(MST_E_ARG, "mst_pairs_trans_decode: bad argument");
    if (n == 0) return MST_OK;
    if (n_pairs == 0 || !keys || !counts || !cell_off || !nB || !out_x || !out_y || !out_v)
        return mst::fail(MST_E_ARG, "mst_pairs_trans_decode: bad argument");
    trans_decode_kernel<<<grid_for(n, kThreads, 8192), kThreads, 0, mst::as_stream(stream)>>>(keys, counts, n, cell_off, nB, n_pairs,
                                                                                               out_x, out_y, out_v);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
