// Read pairs -> pixels on the device (mustache_amd/pairs.py states the rule; include/mustache_hip.h the entry points).
//
//   mst_pairs_bin      one grid-stride pass over (pos1, pos2).  The kernel holds the cis rule alone: a lane bins its row or marks
//                      it dropped, the pixel is (min, max) of the two bins, its key x * n + y, its counter (y - x) * n + x of the
//                      diagonal-major array [K][n] when y - x < K, the far list otherwise; dropped rows are counted per wave and
//                      added once.  The rest is the shared trip body (mst_pairs_tiles.h): runs of adjacent lanes of a wave that
//                      hold the same pixel are merged (sorted files: most rows), a run's head lane adds the run length with one
//                      no-return integer atomic or takes one (key, multiplicity) entry of the far list, whose slots come from
//                      one returning atomic per wave and trip (kFarPerWorkgroup below).
//   mst_pairs_compact  the non-zero counters -> (x, dist, count) records in position order: the shared compaction with the
//                      emitter that turns an index into (x, dist).  No atomics.
//
// Every sum is an integer sum: the counters, the far list as a multiset and both totals are the same from run to run and under
// any order of the rows.  (The far list's ORDER is not: its slots are handed out in arrival order; the caller sorts it.)
#include "mst_pairs_tiles.h"                        // the trip's body and the compaction, shared with mst_pairs_trans.hip

namespace {

// The far-slot reservation is per wave here.  Per workgroup, measured (50 M rows, scripts/pairs_time.py, per wave -> per
// workgroup): 1.91 -> 1.55 ms at 5 kb shuffled, 1.73 -> 1.47 at 1 kb sorted and 1.94 -> 1.63 at 1 kb shuffled, but 2.16 - 2.27 ->
// 2.23 - 2.28 at 5 kb sorted: not the same speed on every input, so the switch is left for a change that is about speed
// (DESIGN section 10).  The trip loop below is right for either form.
constexpr bool kFarPerWorkgroup = false;

__global__ __launch_bounds__(kThreads) void
pairs_bin_kernel(const int32_t *__restrict__ pos1, const int32_t *__restrict__ pos2, int64_t N, int32_t res, int32_t zero_based,
                 int64_t limit, int64_t n, int32_t K, uint32_t *__restrict__ dense, int64_t *__restrict__ far_key,
                 uint32_t *__restrict__ far_mult, int64_t far_cap, unsigned long long *__restrict__ counters) {
    __shared__ BinSlots slots;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
    const int32_t lo = zero_based ? 0 : 1;
    // the largest position kept: 1-based limit, 0-based limit - 1 (one compare per side and no convention inside the loop: the
    // two-sided form cost this loop two to four spilled scalar registers)
    const int64_t top = zero_based && limit > INT64_MIN ? limit - 1 : limit;
    unsigned long long dropped = 0;                 // wave-uniform
    int parity = 0;
    // the trip count is the same for every wave of a workgroup (bin_far's barriers need that: a wave whose rows all lie past N
    // still takes the trip) and for every lane of a wave (the shuffles and ballots do); `e < N` guards the loads only
    for (int64_t block_base = (int64_t)blockIdx.x * kRowsPerBlock; block_base < N; block_base += stride, parity ^= 1) {
        const int64_t base = block_base + (int64_t)wave * (64 * kUnroll);
        BinTrip t;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t e = base + u * 64 + lane;
            const bool active = e < N;
            int32_t x = 0, y = 0;
            bool ok = false;
            if (active) {
                const int32_t a = pos1[e], b = pos2[e];
                ok = a >= lo && b >= lo && (int64_t)a <= top && (int64_t)b <= top;
                if (ok) {
                    const int32_t ba = (a - lo) / res, bb = (b - lo) / res;
                    x = ba < bb ? ba : bb;
                    y = ba < bb ? bb : ba;
                    ok = (int64_t)y < n;            // never written out of bounds, whatever limit the caller gave
                }
            }
            dropped += (unsigned long long)__popcll(__ballot(active && !ok));
            const int32_t dist = y - x;
            bin_group(t, u, active, ok, (long long)x * n + y, dist < K, (int64_t)dist * n + x, dense);
        }
        bin_far<kFarPerWorkgroup>(t, slots, parity, far_key, far_mult, far_cap, &counters[0]);
    }
    if (lane == 0 && dropped) atomicAdd(&counters[1], dropped);
}

struct EmitXDist {                                  // a counter's index is dist * n + x
    int32_t *x, *dist;
    uint32_t *count;
    int64_t n, d, row;                              // d: the diagonal the thread stands on; row: the index of its first counter
    __device__ void seek(int64_t first) {           // the thread's one division
        d = first / n;
        row = d * n;
    }
    __device__ void operator()(int64_t o, int64_t index, uint32_t c) {
        while (index - row >= n) {                  // indices only go up
            ++d;
            row += n;
        }
        x[o] = (int32_t)(index - row);
        dist[o] = (int32_t)d;
        count[o] = c;
    }
};

}  // namespace

extern "C" int mst_pairs_bin(const int32_t *pos1, const int32_t *pos2, int64_t n_rows, int32_t res, int32_t zero_based, int64_t limit,
                             int64_t n, int32_t dense_diags, uint32_t *dense, int64_t *far_key, uint32_t *far_mult, int64_t far_cap,
                             uint64_t *counters, void *stream) {
    if (n_rows < 0 || res < 1 || n < 1 || dense_diags < 0 || far_cap < 0 || !counters || (n_rows > 0 && (!pos1 || !pos2)) ||
        (dense_diags > 0 && !dense) || (far_cap > 0 && (!far_key || !far_mult)) || (int64_t)dense_diags > n)
        return mst::fail(MST_E_ARG, "mst_pairs_bin: bad argument");
    if (n_rows == 0) return MST_OK;
    // at most 2048 workgroups: 32 waves for each of 256 compute units, each workgroup on trips of 2048 rows
    pairs_bin_kernel<<<grid_for(n_rows, kRowsPerBlock, 2048), kThreads, 0, mst::as_stream(stream)>>>(
        pos1, pos2, n_rows, res, zero_based, limit, n, dense_diags, dense, far_key, far_mult, far_cap,
        reinterpret_cast<unsigned long long *>(counters));
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" uint64_t mst_pairs_compact_workspace_bytes(int32_t dense_diags, int64_t n) {
    if (dense_diags < 0 || n < 0) return 0;
    return compact_workspace_bytes((int64_t)dense_diags * n);
}

extern "C" int mst_pairs_compact(const uint32_t *dense, int32_t dense_diags, int64_t n, int32_t *out_x, int32_t *out_dist,
                                 uint32_t *out_count, int64_t cap, int64_t *n_out, void *workspace, uint64_t workspace_bytes,
                                 void *stream) {
    if (dense_diags < 0 || n < 0) return mst::fail(MST_E_ARG, "mst_pairs_compact: bad argument");
    return compact_counters("mst_pairs_compact", dense, (int64_t)dense_diags * n, EmitXDist{out_x, out_dist, out_count, n, 0, 0},
                            out_x && out_dist && out_count, cap, n_out, workspace, workspace_bytes, stream);
}
