// The resident trans records of MANY chromosome pairs at one resolution -> the pixels of a coarser one in one launch
// (mustache_amd/multires.py states the rule; include/mustache_hip.h the entry points; tests/coarsen_genome_reference.py restates
// it in NumPy).
//
//   mst_coarsen_pairs          the records of P pairs lie concatenated, pair p in [seg_off[p], seg_off[p + 1]).  A record (x, y,
//                              c) of pair p goes to X = x / k, Y = y / k.  A record with a negative bin, X >= n_a[p] or
//                              Y >= n_b[p] is dropped and counted -- BEFORE a key is formed: Y == n_b[p] would otherwise read
//                              as (X + 1, 0) and X == n_a[p] as the first row of pair p + 1.  The key of any other record is
//                              cell_off[p] + X * n_b[p] + Y, pairs.trans_tables' key space at the coarse resolution.  A key below
//                              dense_cells adds to the 64-bit counter dense[key], any other is a far entry (key, count): the
//                              split of mst_pairs_bin_trans, so every far key is >= dense_cells.
//   mst_coarsen_pairs_compact  the non-zero 64-bit counters -> (key, count int64) in ascending key order.  The count / scan /
//                              write scheme of mst_pairs_tiles.h on 8-byte counters; no atomics.
//
// A lane finds its pair with mst::segment_of; the search is wave-uniform while lanes 0 and 63 lie in one segment (the idiom of
// mst_thin_pairs.hip), and a workgroup takes consecutive tiles of 256 records so that it mostly is.  Records arrive with
// neighbours that share a destination -- `.hic` rows come block-ordered, binned pairs and thinned records in cell order, so runs
// of up to k lanes hit one cell -- and adjacent lanes of a wave with equal keys combine their counts before the atomic or the
// far entry (mst_coarsen_tiles.h's segmented suffix sum, as in mst_coarsen.hip).  The cell ranges of the pairs are disjoint, so
// equal keys imply the same pair: a run may cross a segment boundary in lanes, never in destination.  Every sum is an integer
// sum: the combined and the plain form (-DMST_COARSEN_PAIRS_PLAIN, `make coarsen_pairs_plain`: every record its own atomic)
// give the same counters, as does any order of the records within a pair and any launch shape.
#include "mst_coarsen_tiles.h"

namespace {

constexpr int kDefaultBlocks = 4096;                // 16 workgroups a CU, mst_thin_pairs.hip's

template <typename C>
__global__ __launch_bounds__(kThreads) void
coarsen_pairs_kernel(const int32_t *__restrict__ xs, const int32_t *__restrict__ ys, const C *__restrict__ count_in, int64_t N,
                     const int64_t *__restrict__ seg_off, const int64_t *__restrict__ n_a, const int64_t *__restrict__ n_b,
                     const int64_t *__restrict__ cell_off, int32_t P, int32_t factor, int64_t dense_cells,
                     unsigned long long *__restrict__ dense, int64_t *__restrict__ far_key, int64_t *__restrict__ far_count,
                     int64_t far_cap, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long part[2][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a workgroup takes consecutive tiles of kThreads records: a wave's trips stay in one pair for as long as the pair lasts
    const int64_t tiles = (N + kThreads - 1) / kThreads, per = (tiles + gridDim.x - 1) / gridDim.x;
    const int64_t tile0 = (int64_t)blockIdx.x * per, tile1 = tile0 + per < tiles ? tile0 + per : tiles;
    int32_t p_wave = -1;
    unsigned long long sum_in = 0, outside = 0;
    bool bad = false;
    // every lane of a wave makes the same trips (the ballots and the shifts need that); `e < N` guards the loads
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t e0 = tile * kThreads + wave * 64, e = e0 + lane;
        if (e0 >= N) continue;                      // wave-uniform: nothing of this trip is this wave's
        const bool active = e < N;
        const int64_t last = e0 + 63 < N ? e0 + 63 : N - 1;
        // e0 ascends from trip to trip: the search starts at the pair of the trip before and is skipped while that pair lasts
        if (p_wave < 0 || (p_wave + 1 < P && e0 >= seg_off[p_wave + 1]))
            p_wave = __builtin_amdgcn_readfirstlane(mst::segment_of(seg_off, p_wave < 0 ? 0 : p_wave, P, e0));
        const bool one_pair = p_wave + 1 >= P || last < seg_off[p_wave + 1];          // lanes 0 and 63 in one segment
        const int32_t p = one_pair ? p_wave : (active ? mst::segment_of(seg_off, p_wave, P, e) : p_wave);
        long long key = -1;                         // no destination: a lane past N, or a record outside its pair's matrix
        unsigned long long c = 0;
        if (active) {
            const int64_t na = n_a[p], nb = n_b[p], off = cell_off[p];               // p lies in [0, P) whatever seg_off holds
            const int64_t v = count_of(count_in[e]);
            const int64_t x = xs[e], y = ys[e];
            bad |= v < 0;
            c = v < 0 ? 0ull : (unsigned long long)v;
            const int64_t X = x / factor, Y = y / factor;
            // the outside test comes before the key: Y == nb is not (X + 1, 0), X == na not the first row of pair p + 1
            if (x >= 0 && y >= 0 && X < na && Y < nb && off >= 0) {
                key = off + X * nb + Y;
                sum_in += c;
            } else {
                outside += 1;
                c = 0;
            }
        }
#ifdef MST_COARSEN_PAIRS_PLAIN
        const bool head = key >= 0 && c != 0;
        const unsigned long long sum = c;
#else
        const long long prev = __shfl_up(key, 1, 64);
        const bool start = lane == 0 || prev != key;                // the first lane of a run of equal keys
        const unsigned long long starts = __ballot(start);
        const unsigned long long above = lane == 63 ? 0ull : (starts >> (lane + 1));
        const uint32_t rest = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
        const unsigned long long sum = run_suffix_sum(c, rest);
        const bool head = start && key >= 0 && sum != 0;
#endif
        const bool near = key < dense_cells;
        if (head && near) atomicAdd(&dense[key], sum);              // no-return, 64-bit integer; 0 <= key < dense_cells
        const unsigned long long fars = __ballot(head && !near);
        if (fars) {                                 // wave-uniform: one returning atomic per wave and trip
            unsigned long long slot0 = 0;
            if (lane == 0) slot0 = atomicAdd(&words[0], (unsigned long long)__popcll(fars));
            const int64_t mine = (int64_t)__shfl(slot0, 0, 64) + __popcll(fars & ((1ull << lane) - 1ull));
            if (head && !near && mine < far_cap) {  // nothing is written at or past far_cap; the count goes on
                far_key[mine] = key;
                far_count[mine] = (int64_t)sum;
            }
        }
    }
    if (bad) words[2] = 1;                          // a flag, not a count: every writer writes the same value
    sum_in = wave_sum(sum_in);
    outside = wave_sum(outside);
    if (lane == 0) {
        part[0][wave] = sum_in;
        part[1][wave] = outside;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0, o = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            s += part[0][w];
            o += part[1][w];
        }
        if (s) atomicAdd(&words[1], s);
        if (o) atomicAdd(&words[3], o);
    }
}

// a counter's index is its key
__global__ __launch_bounds__(kThreads) void
compact64_keys_kernel(const unsigned long long *__restrict__ dense, int64_t total, const int64_t *__restrict__ tile_off, int64_t cap,
                      int64_t *__restrict__ out_key, int64_t *__restrict__ out_count) {
    __shared__ uint32_t wave_sums[kWaves];
    unsigned long long c[kPerThread];
    uint32_t all;
    const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
    const uint32_t mine = load_tile64(dense, total, first, c);
    const uint32_t incl = block_scan(mine, wave_sums, &all);
    if (!mine) return;
    int64_t o = tile_off[blockIdx.x] + (int64_t)(incl - mine);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (c[k] == 0ull || o >= cap) continue;
        out_key[o] = first + k;
        out_count[o] = (int64_t)c[k];
        ++o;
    }
}

}  // namespace

extern "C" int mst_coarsen_pairs(const int32_t *x, const int32_t *y, const void *count_in, int32_t count_kind, int64_t n_records,
                                 const int64_t *seg_off, const int64_t *n_a, const int64_t *n_b, const int64_t *cell_off,
                                 int32_t n_pairs, int32_t factor, int64_t dense_cells, uint64_t *dense, int64_t *far_key,
                                 int64_t *far_count, int64_t far_cap, int64_t *words, int32_t max_blocks, void *stream) {
    if (n_records < 0 || n_pairs < 0 || factor < 1 || dense_cells < 0 || far_cap < 0 || max_blocks < 0 || !words || count_kind < 0 ||
        count_kind > 2 || (n_records > 0 && (!x || !y || !count_in || !seg_off || !n_a || !n_b || !cell_off || n_pairs < 1)) ||
        (dense_cells > 0 && !dense) || (far_cap > 0 && (!far_key || !far_count)))
        return mst::fail(MST_E_ARG, "mst_coarsen_pairs: bad argument");
    if (n_records == 0) return MST_OK;
    const dim3 grid((unsigned)grid_for(n_records, kThreads, max_blocks ? max_blocks : kDefaultBlocks));
    auto *d = reinterpret_cast<unsigned long long *>(dense);
    auto *w = reinterpret_cast<unsigned long long *>(words);
    hipStream_t s = mst::as_stream(stream);
    if (count_kind == MST_THIN_COUNT_I64)
        coarsen_pairs_kernel<int64_t><<<grid, kThreads, 0, s>>>(x, y, static_cast<const int64_t *>(count_in), n_records, seg_off, n_a,
                                                               n_b, cell_off, n_pairs, factor, dense_cells, d, far_key, far_count,
                                                               far_cap, w);
    else if (count_kind == MST_THIN_COUNT_F32)
        coarsen_pairs_kernel<float><<<grid, kThreads, 0, s>>>(x, y, static_cast<const float *>(count_in), n_records, seg_off, n_a, n_b,
                                                             cell_off, n_pairs, factor, dense_cells, d, far_key, far_count, far_cap,
                                                             w);
    else
        coarsen_pairs_kernel<double><<<grid, kThreads, 0, s>>>(x, y, static_cast<const double *>(count_in), n_records, seg_off, n_a,
                                                              n_b, cell_off, n_pairs, factor, dense_cells, d, far_key, far_count,
                                                              far_cap, w);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" uint64_t mst_coarsen_pairs_compact_workspace_bytes(int64_t dense_cells) {
    return dense_cells < 0 ? 0 : compact_workspace_bytes(dense_cells);
}

extern "C" int mst_coarsen_pairs_compact(const uint64_t *dense, int64_t dense_cells, int64_t *out_key, int64_t *out_count, int64_t cap,
                                         int64_t *n_out, void *workspace, uint64_t workspace_bytes, void *stream) {
    if (dense_cells < 0 || cap < 0 || !n_out || (cap > 0 && !(out_key && out_count)))
        return mst::fail(MST_E_ARG, "mst_coarsen_pairs_compact: bad argument");
    hipStream_t s = mst::as_stream(stream);
    if (dense_cells == 0) {
        MST_HIP(hipMemsetAsync(n_out, 0, sizeof(int64_t), s));
        return MST_OK;
    }
    const int64_t tiles = (dense_cells + kTile - 1) / kTile;
    if (!dense || !workspace || workspace_bytes < compact_workspace_bytes(dense_cells) || tiles > 0x7fffffff)
        return mst::fail(MST_E_ARG, "mst_coarsen_pairs_compact: bad argument");
    int64_t *tile_off = static_cast<int64_t *>(workspace);
    auto *d = reinterpret_cast<const unsigned long long *>(dense);
    compact64_count_kernel<<<(int)tiles, kThreads, 0, s>>>(d, dense_cells, tile_off);
    MST_LAUNCH_CHECK();
    compact_scan_kernel<<<1, kThreads, 0, s>>>(tile_off, tiles, n_out);
    MST_LAUNCH_CHECK();
    compact64_keys_kernel<<<(int)tiles, kThreads, 0, s>>>(d, dense_cells, tile_off, cap, out_key, out_count);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
