// Raw records of one resolution -> the pixels of a coarser one on the device (mustache_amd/multires.py states the rule;
// include/mustache_hip.h the entry points; tests/multires_reference.py restates it in NumPy).
//
//   mst_coarsen_records   one grid-stride pass over (x, dist, count).  A record goes to X = x / k, Y = (x + dist) / k; its key is
//                         X * n + Y, its counter (Y - X) * n + X of the diagonal-major array [K][n] when Y - X < K, the far list
//                         (key, count) otherwise.  Counters are 64-bit integers: a cell that receives 3 * 2^31 reads 3 * 2^31.
//   mst_coarsen_compact   the non-zero 64-bit counters -> (x, dist, count int64) records in position order.  The count / scan /
//                         write scheme of mst_pairs_tiles.h on 8-byte counters; no atomics.
//
// Records arrive with neighbours that share a destination: the binning's compaction emits them diagonal by diagonal with x
// ascending, so runs of up to k adjacent lanes hit one coarse cell; `.hic` rows come block-ordered.  Before the atomic the
// adjacent lanes of a wave with equal keys combine their counts -- a segmented suffix sum over the wave -- and the head lane of
// each run issues one atomic or takes one far entry.  Short runs (the usual case: at most kLinear lanes) are summed by shifting
// the counts one lane at a time with DPP wave shifts; longer ones by log steps of shuffles.  Every record is addressed by its
// own (x, dist) and integer addition is order-free: the combined and the plain form (-DMST_COARSEN_PLAIN, `make coarsen_plain`:
// every record its own atomic) give the same sums by construction, as does any order of the records.
#include "mst_coarsen_tiles.h"                      // count_of, run_suffix_sum, compact64_count_kernel; mst_pairs_tiles.h

namespace {

template <typename C>
__global__ __launch_bounds__(kThreads) void
coarsen_kernel(const int32_t *__restrict__ xs, const int32_t *__restrict__ dists, const C *__restrict__ count_in, int64_t N, int32_t factor,
               int64_t n, int32_t K, unsigned long long *__restrict__ dense, int64_t *__restrict__ far_key,
               int64_t *__restrict__ far_count, int64_t far_cap, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long part[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    unsigned long long sum_in = 0;
    bool bad = false;
    // the trip count is the same for every lane of a workgroup (the ballots and the shifts need that of a wave); `e < N` guards
    // the loads only
    for (int64_t base = (int64_t)blockIdx.x * kThreads; base < N; base += stride) {
        const int64_t e = base + threadIdx.x;
        long long key = -1;                         // no destination: a lane past N, or a record outside [0, n) x [0, n)
        int64_t X = 0, D = 0;
        unsigned long long c = 0;
        if (e < N) {
            const int64_t v = count_of(count_in[e]);
            const int64_t x = xs[e], y = x + (int64_t)dists[e];
            bad |= v < 0;
            c = v < 0 ? 0ull : (unsigned long long)v;
            sum_in += c;
            X = x / factor;
            const int64_t Y = y / factor;
            D = Y - X;
            if (x >= 0 && y >= x && Y < n) key = X * n + Y;         // never written out of bounds, whatever n the caller gave
        }
#ifdef MST_COARSEN_PLAIN
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
        const bool near = D < K;
        if (head && near) atomicAdd(&dense[D * n + X], sum);        // no-return, 64-bit integer
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
    if (lane == 0) part[wave] = sum_in;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += part[w];
        if (s) atomicAdd(&words[1], s);
    }
}

// ---- compaction of 64-bit counters (the count pass is mst_coarsen_tiles.h's) -----------------------------------------------
// a counter's index is dist * n + x; the thread walks the diagonals upwards from its first counter's (one division)
__global__ __launch_bounds__(kThreads) void
compact64_write_kernel(const unsigned long long *__restrict__ dense, int64_t total, const int64_t *__restrict__ tile_off, int64_t cap,
                       int64_t n, int32_t *__restrict__ out_x, int32_t *__restrict__ out_dist, int64_t *__restrict__ out_count) {
    __shared__ uint32_t wave_sums[kWaves];
    unsigned long long c[kPerThread];
    uint32_t all;
    const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
    const uint32_t mine = load_tile64(dense, total, first, c);
    const uint32_t incl = block_scan(mine, wave_sums, &all);
    if (!mine) return;
    int64_t o = tile_off[blockIdx.x] + (int64_t)(incl - mine);
    int64_t d = first / n, row = d * n;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (c[k] == 0ull || o >= cap) continue;
        const int64_t index = first + k;
        while (index - row >= n) {                  // indices only go up
            ++d;
            row += n;
        }
        out_x[o] = (int32_t)(index - row);
        out_dist[o] = (int32_t)d;
        out_count[o] = (int64_t)c[k];
        ++o;
    }
}

}  // namespace

extern "C" int mst_coarsen_records(const int32_t *x, const int32_t *dist, const void *count_in, int32_t count_kind, int64_t n_records,
                                   int32_t factor, int64_t n, int32_t dense_diags, uint64_t *dense, int64_t *far_key,
                                   int64_t *far_count, int64_t far_cap, int64_t *words, void *stream) {
    if (n_records < 0 || factor < 1 || n < 1 || dense_diags < 0 || (int64_t)dense_diags > n || far_cap < 0 || !words ||
        count_kind < 0 || count_kind > 2 || (n_records > 0 && (!x || !dist || !count_in)) || (dense_diags > 0 && !dense) ||
        (far_cap > 0 && (!far_key || !far_count)))
        return mst::fail(MST_E_ARG, "mst_coarsen_records: bad argument");
    if (n_records == 0) return MST_OK;
    // one lane per record and trip; at most 8192 workgroups (32 waves for each of 256 compute units, four trips deep)
    const dim3 grid((unsigned)grid_for(n_records, kThreads, 8192));
    auto *d = reinterpret_cast<unsigned long long *>(dense);
    auto *w = reinterpret_cast<unsigned long long *>(words);
    hipStream_t s = mst::as_stream(stream);
    if (count_kind == MST_THIN_COUNT_I64)
        coarsen_kernel<int64_t><<<grid, kThreads, 0, s>>>(x, dist, static_cast<const int64_t *>(count_in), n_records, factor, n,
                                                         dense_diags, d, far_key, far_count, far_cap, w);
    else if (count_kind == MST_THIN_COUNT_F32)
        coarsen_kernel<float><<<grid, kThreads, 0, s>>>(x, dist, static_cast<const float *>(count_in), n_records, factor, n, dense_diags,
                                                       d, far_key, far_count, far_cap, w);
    else
        coarsen_kernel<double><<<grid, kThreads, 0, s>>>(x, dist, static_cast<const double *>(count_in), n_records, factor, n,
                                                        dense_diags, d, far_key, far_count, far_cap, w);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" uint64_t mst_coarsen_compact_workspace_bytes(int32_t dense_diags, int64_t n) {
    if (dense_diags < 0 || n < 0) return 0;
    return compact_workspace_bytes((int64_t)dense_diags * n);
}

extern "C" int mst_coarsen_compact(const uint64_t *dense, int32_t dense_diags, int64_t n, int32_t *out_x, int32_t *out_dist,
                                   int64_t *out_count, int64_t cap, int64_t *n_out, void *workspace, uint64_t workspace_bytes,
                                   void *stream) {
    if (dense_diags < 0 || n < 0 || cap < 0 || !n_out || (cap > 0 && !(out_x && out_dist && out_count)))
        return mst::fail(MST_E_ARG, "mst_coarsen_compact: bad argument");
    const int64_t total = (int64_t)dense_diags * n;
    hipStream_t s = mst::as_stream(stream);
    if (total == 0) {
        MST_HIP(hipMemsetAsync(n_out, 0, sizeof(int64_t), s));
        return MST_OK;
    }
    const int64_t tiles = (total + kTile - 1) / kTile;
    if (!dense || !workspace || workspace_bytes < compact_workspace_bytes(total) || tiles > 0x7fffffff)
        return mst::fail(MST_E_ARG, "mst_coarsen_compact: bad argument");
    int64_t *tile_off = static_cast<int64_t *>(workspace);
    auto *d = reinterpret_cast<const unsigned long long *>(dense);
    compact64_count_kernel<<<(int)tiles, kThreads, 0, s>>>(d, total, tile_off);
    MST_LAUNCH_CHECK();
    compact_scan_kernel<<<1, kThreads, 0, s>>>(tile_off, tiles, n_out);
    MST_LAUNCH_CHECK();
    compact64_write_kernel<<<(int)tiles, kThreads, 0, s>>>(d, total, tile_off, cap, n, out_x, out_dist, out_count);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
