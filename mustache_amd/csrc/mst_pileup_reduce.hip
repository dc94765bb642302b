// The reduce of every pile-up (mustache_amd/pileup.py states the rules; tests/pileup_reference.py, ordered_aggregate, restates
// it addition by addition): per cell of the (2w+1) x (2w+1) window the sums and counts over the loops of two stacks of windows,
// in a given (sorted) loop order.
//
//   mst_pileup_reduce            agg[0..3][cell] = sum a, count a, sum b, count b: each stack under its own NaN mask (obs and oe)
//   mst_pileup_reduce_segmented  the same for P segments of the loops (the pairs of a trans batch): agg[pair][0..3][cell]
//   mst_pileup_reduce_pair       agg[0..2][cell] = sum a, sum b, count under the joint mask (oe of one loop list on two maps): a
//                                loop adds to a cell where neither window is NaN there
//
// One order of additions for all three, which depends only on the position in `order`: a segment's positions go in chunks of
// kLoopChunk loops; workgroup (block of 64 cells, chunk), wave v adds the chunk's loops v * 128 .. v * 128 + 127 in order for its
// 64 cells; the four wave partials are added in wave order, and a second launch adds a segment's chunks in chunk order.  An
// order entry outside its segment is skipped.  No float atomics: the results are bit-identical from run to run and under any
// permutation of the loops the caller sorts, and a segment's values do not depend on the segments beside it.
//
// A wave fetches 64 order entries with one load (lane j holds entry j) and takes each from its lane by a shuffle, and it requests
// the windows of kAhead loops -- 2 * kAhead loads -- before the first addition, so the latency of a window load is paid once per
// kAhead loops instead of once per loop.
#include <cmath>
#include <vector>
#include "mst_common.h"
#include "mst_pileup_sums.h"

namespace {

using mst_pileup::align256;
using mst_pileup::cells_of;
using mst_pileup::grid_ok;
using mst_pileup::kLoopChunk;
using mst_pileup::kLoopsPerWave;
using mst_pileup::kThreads;
using mst_pileup::kWaves;
using mst_pileup::loop_chunks;
using mst_pileup::partials_bytes;

constexpr int kAhead = 8;                              // loops whose windows a wave requests before it adds the first
static_assert(64 % kAhead == 0, "a group of 64 order entries is walked in whole steps of kAhead");

// part[chunk][row][cell], the chunks of all segments numbered through.  loop_off (with chunk_off[p] = the chunks before segment p)
// is null for the one segment 0 .. L-1: the same for the whole workgroup.  Every lane of a wave runs every trip of both loops --
// the shuffles need them all -- and a lane past the last cell, or an order entry that is past the wave's range or outside the
// segment, carries NaN: not counted.
template <bool kJoint>
__global__ void __launch_bounds__(kThreads)
reduce_partial_kernel(const double *__restrict__ sa, const double *__restrict__ sb, const int32_t *__restrict__ order, int64_t L,
                      const int64_t *__restrict__ loop_off, const int64_t *__restrict__ chunk_off, int32_t P, int64_t cells,
                      int64_t cell_blocks, double *__restrict__ part) {
    constexpr int kRows = kJoint ? 3 : 4;
    __shared__ double red[kWaves][kRows][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cb = blockIdx.x % cell_blocks, k = blockIdx.x / cell_blocks;
    const int64_t cell = cb * 64 + lane;
    const bool mine = cell < cells;
    int64_t l0 = 0, l1 = L, first = k * kLoopChunk;
    if (loop_off) {
        const int32_t seg = mst::segment_of(chunk_off, 0, P, k);
        l0 = loop_off[seg];
        l1 = loop_off[seg + 1];
        first = l0 + (k - chunk_off[seg]) * kLoopChunk;
    }
    const int64_t p0 = first + (int64_t)wave * kLoopsPerWave;
    const int64_t p1 = (p0 + kLoopsPerWave < l1) ? p0 + kLoopsPerWave : l1;
    double acc[kRows];
#pragma unroll
    for (int m = 0; m < kRows; ++m) acc[m] = 0.0;
    for (int64_t g = p0; g < p1; g += 64) {                // wave-uniform bounds
        const int32_t entry = g + lane < p1 ? order[g + lane] : -1;
        const int here = p1 - g < 64 ? (int)(p1 - g) : 64;
        for (int j = 0; j < here; j += kAhead) {
            double u[kAhead], v[kAhead];
#pragma unroll
            for (int i = 0; i < kAhead; ++i) {             // j + i <= 63; an entry past `here` is -1
                const int64_t l = __shfl(entry, j + i, 64);
                const bool ok = mine && l >= l0 && l < l1;
                const int64_t at = ok ? l * cells + cell : 0;             // every load is issued, at a safe address (L > 0):
                const double a = sa[at], b = sb[at];                       // a branch around a load would wait for each one
                u[i] = ok ? a : NAN;
                v[i] = ok ? b : NAN;
            }
#pragma unroll
            for (int i = 0; i < kAhead; ++i) {
                if constexpr (kJoint) {
                    if (u[i] == u[i] && v[i] == v[i]) {
                        acc[0] = acc[0] + u[i];
                        acc[1] = acc[1] + v[i];
                        acc[2] = acc[2] + 1.0;
                    }
                } else {
                    if (u[i] == u[i]) {
                        acc[0] = acc[0] + u[i];
                        acc[1] = acc[1] + 1.0;
                    }
                    if (v[i] == v[i]) {
                        acc[2] = acc[2] + v[i];
                        acc[3] = acc[3] + 1.0;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < kRows; ++m) red[wave][m][lane] = acc[m];
    __syncthreads();
    if (wave == 0 && mine) {
#pragma unroll
        for (int m = 0; m < kRows; ++m) {
            double t = red[0][m][lane];
#pragma unroll
            for (int v = 1; v < kWaves; ++v) t = t + red[v][m][lane];
            part[(k * kRows + m) * cells + cell] = t;
        }
    }
}

// workgroup (segment, block of 256 cells): the segment's chunks in chunk order; zeros for a segment without a loop.  chunk_off
// null: the one segment owns the chunks 0 .. nchunks-1.
template <int kRows>
__global__ void __launch_bounds__(kThreads)
reduce_finish_kernel(int64_t cells, int64_t cell_blocks, const int64_t *__restrict__ chunk_off, int64_t nchunks,
                     const double *__restrict__ part, double *__restrict__ agg) {
    const int64_t seg = blockIdx.x / cell_blocks;
    const int64_t cell = (blockIdx.x % cell_blocks) * kThreads + threadIdx.x;
    if (cell >= cells) return;
    const int64_t k0 = chunk_off ? chunk_off[seg] : 0, k1 = chunk_off ? chunk_off[seg + 1] : nchunks;
#pragma unroll
    for (int m = 0; m < kRows; ++m) {
        double t = 0.0;
        for (int64_t k = k0; k < k1; ++k) t = t + part[(k * kRows + m) * cells + cell];
        agg[(seg * kRows + m) * cells + cell] = t;
    }
}

// the workspace: with a segment table its device copy (loop_off, then chunk_off: P + 1 entries each) first, then the partials
struct Layout {
    uint64_t part, end;
    int64_t nchunks;
};

Layout layout(int64_t L, const int64_t *loop_off, int32_t P, int rows, int32_t w) {
    Layout o;
    o.nchunks = loop_off ? 0 : loop_chunks(L);
    for (int32_t p = 0; loop_off && p < P; ++p) o.nchunks += loop_chunks(loop_off[p + 1] - loop_off[p]);
    o.part = loop_off ? align256((uint64_t)2 * (P + 1) * 8) : 0;
    o.end = o.part + partials_bytes(o.nchunks, rows, w);
    return o;
}

template <bool kJoint>
int launch(const double *sa, const double *sb, const int32_t *order, int64_t L, const int64_t *d_loop_off, int32_t P, int64_t cells,
           int64_t nchunks, double *part, double *agg, hipStream_t s) {
    const int64_t cell_blocks = (cells + 63) / 64, finish_blocks = (cells + kThreads - 1) / kThreads;
    const int64_t *d_chunk_off = d_loop_off ? d_loop_off + (P + 1) : nullptr;
    reduce_partial_kernel<kJoint><<<(unsigned)(cell_blocks * nchunks), kThreads, 0, s>>>(sa, sb, order, L, d_loop_off, d_chunk_off, P,
                                                                                         cells, cell_blocks, part);
    MST_LAUNCH_CHECK();
    reduce_finish_kernel<kJoint ? 3 : 4><<<(unsigned)(finish_blocks * P), kThreads, 0, s>>>(cells, finish_blocks, d_chunk_off, nchunks,
                                                                                           part, agg);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

// ---- the body behind the three entry points (`who` names the caller in a refusal): every check, the layout, the launches.
// loop_off: the HOST table of P segments; null for the one segment 0 .. L-1 (P = 1), which builds and uploads no table.
int run_reduce(const char *who, bool joint, bool segmented, const double *sa, const double *sb, const int32_t *order, int64_t L,
               const int64_t *loop_off, int32_t P, int32_t w, double *agg, void *workspace, uint64_t workspace_bytes, void *stream) {
    int rc = mst_pileup::check_w(who, w, 1);
    if (rc != MST_OK) return rc;
    if ((rc = mst_pileup::check_pairs(who, P)) != MST_OK) return rc;
    if (L < 0 || L > INT32_MAX || !agg || (L > 0 && (!sa || !sb || !order)))
        return mst::fail(MST_E_ARG, "%s: bad argument (L %lld, agg %s; with L > 0 both stacks of windows and order are needed)", who,
                         (long long)L, agg ? "given" : "null");
    if (segmented && !mst_pileup::offsets_ok(loop_off, P, L))
        return mst::fail(MST_E_ARG, "%s: bad argument (L %lld; loop_off: host, P + 1 entries rising from 0 to L)", who, (long long)L);
    const int rows = joint ? 3 : 4;
    const int64_t cells = cells_of(w);
    hipStream_t s = mst::as_stream(stream);
    if (L == 0) {
        MST_HIP(hipMemsetAsync(agg, 0, (size_t)P * rows * cells * 8, s));
        return MST_OK;
    }
    const Layout o = layout(L, loop_off, P, rows, w);
    if (!workspace || workspace_bytes < o.end)
        return mst::fail(MST_E_ARG, "%s: workspace of %llu bytes, %llu needed", who, (unsigned long long)workspace_bytes,
                         (unsigned long long)o.end);
    if ((rc = grid_ok(who, (cells + 63) / 64 * o.nchunks)) != MST_OK) return rc;
    if ((rc = grid_ok(who, (cells + kThreads - 1) / kThreads * P)) != MST_OK) return rc;
    char *base = static_cast<char *>(workspace);
    int64_t *d_loop_off = nullptr;
    if (loop_off) {
        static thread_local std::vector<int64_t> table;
        table.assign((size_t)2 * (P + 1), 0);
        int64_t *h_loop_off = table.data(), *h_chunk_off = table.data() + (P + 1);
        for (int32_t p = 0; p < P; ++p) {
            h_loop_off[p] = loop_off[p];
            h_chunk_off[p + 1] = h_chunk_off[p] + loop_chunks(loop_off[p + 1] - loop_off[p]);
        }
        h_loop_off[P] = loop_off[P];
        d_loop_off = reinterpret_cast<int64_t *>(base);
        MST_HIP(mst::upload_small(d_loop_off, table.data(), table.size() * 8, s));
    }
    double *part = reinterpret_cast<double *>(base + o.part);
    return joint ? launch<true>(sa, sb, order, L, d_loop_off, P, cells, o.nchunks, part, agg, s)
                 : launch<false>(sa, sb, order, L, d_loop_off, P, cells, o.nchunks, part, agg, s);
}

}  // namespace

// mst_pileup_workspace_bytes (mst_pileup.hip) and mst_pileup_trans_workspace_bytes (mst_pileup_trans_batch.hip) cover the
// one-segment calls; the joint reduce needs three quarters of what mst_pileup_reduce needs for the same (L, w).
extern "C" uint64_t mst_pileup_reduce_segmented_workspace_bytes(const int64_t *loop_off, int32_t P, int32_t w) {
    if (P < 1 || P > mst_pileup::kMaxPairs || w < 0 || w > mst_pileup::kMaxW || !loop_off ||
        !mst_pileup::offsets_ok(loop_off, P, loop_off[P]))
        return 0;
    return align256(layout(loop_off[P], loop_off, P, 4, w).end) + 256;
}

extern "C" int mst_pileup_reduce(const double *obs, const double *oe, const int32_t *order, int64_t L, int32_t w, double *agg,
                                 void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_reduce");
    return run_reduce("mst_pileup_reduce", false, false, obs, oe, order, L, nullptr, 1, w, agg, workspace, workspace_bytes, stream);
}

extern "C" int mst_pileup_reduce_segmented(const double *obs, const double *oe, const int32_t *order, int64_t L,
                                           const int64_t *loop_off, int32_t P, int32_t w, double *agg, void *workspace,
                                           uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_reduce_segmented");
    return run_reduce("mst_pileup_reduce_segmented", false, true, obs, oe, order, L, loop_off, P, w, agg, workspace, workspace_bytes, stream);
}

extern "C" int mst_pileup_reduce_pair(const double *oe1, const double *oe2, const int32_t *order, int64_t L, int32_t w,
                                      double *agg, void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_reduce_pair");
    return run_reduce("mst_pileup_reduce_pair", true, false, oe1, oe2, order, L, nullptr, 1, w, agg, workspace, workspace_bytes, stream);
}
