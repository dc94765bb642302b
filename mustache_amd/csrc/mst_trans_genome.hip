// Inter-chromosomal (trans) maps of MANY chromosome pairs in shared launches (gfx950): the stages in front of the fused
// launch for a batch of P pairs whose records are concatenated (x, y, v [N]; seg_off [P + 1] gives each pair's range).  The
// rules are those of mustache_amd/trans.py; mustache_amd/trans_genome.py drives these entry points.
//
//   mst_trans_zscore_segmented   rule 2 per pair: stats[p] = {mean, std, n, flags}, out = (v - mean_p) / std_p, and the pair's
//                                extent {max x, max y}.  Bit-identical per pair to mst_trans_zscore on that pair alone: the same
//                                exact sums (mst_exact_sum.h), the same single rounding.
//   mst_trans_count_tiles        counts[t] = records with v' != 0 inside the window of tile t, for every tile of the batch.
//   mst_trans_scatter_worklist   the records of a pair range -> the B tiles of one launch, chosen by slot[t].
//
// Work is distributed in chunks of kChunk records that belong to ONE pair each (a pair of a few hundred records and one of a
// hundred million share a launch), every workgroup takes a run of consecutive chunks and flushes its LDS sums to a pair's words
// only when the pair changes.
//
// A tile's windows are an arithmetic progression plus one last window (trans_axis_tiles): window i of an axis of length n
// starts at i (C - 256) for i < K - 1 and at max(0, n - C) for i = K - 1.  The windows that hold a coordinate follow from
// the coordinate (axis_windows), so no kernel here loops over the tiles of a launch.
#include <cmath>
#include "mst_common.h"
#include "mst_exact_sum.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;            // records per chunk: 16 per thread
constexpr int kOverlap = 256;           // trans.TRANS_OVERLAP
using mst_exact::add_exact;
using mst_exact::exact_to_double;
using mst_exact::kLimbs;
using mst_exact::kSumWords;

// workspace of the z-score: chunk_first int64 [P + 1], then per pair 2 x kSumWords words
__host__ __device__ inline size_t words_offset(int P) { return ((size_t)(P + 1) * 8 + 15) / 16 * 16; }

// chunk_first[p] = chunks of the pairs before p; one thread: P is a few hundred
__global__ void chunk_table_kernel(const int64_t *__restrict__ seg_off, int P, int64_t *__restrict__ chunk_first) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t run = 0;
    for (int p = 0; p < P; ++p) {
        chunk_first[p] = run;
        const int64_t len = seg_off[p + 1] - seg_off[p];
        run += len > 0 ? (len + kChunk - 1) / kChunk : 0;
    }
    chunk_first[P] = run;
}

__device__ __forceinline__ int wave_max(int a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int b = __shfl_xor(a, o, 64);
        a = b > a ? b : a;
    }
    return a;
}

// PASS 0: words[p] += v and extent[p] = max(x), max(y);  PASS 1: words[p] += (v - mean_p)^2
template <int PASS>
__global__ void __launch_bounds__(kThreads)
zseg_sum_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, const double *__restrict__ v,
                const int64_t *__restrict__ seg_off, int P, const int64_t *__restrict__ chunk_first,
                const double *__restrict__ stats, unsigned long long *__restrict__ words, int32_t *__restrict__ extent) {
    __shared__ unsigned long long acc[kLimbs];
    __shared__ unsigned long long bad;
    __shared__ int ext[2];
    const int64_t total = chunk_first[P];
    const int64_t per = (total + gridDim.x - 1) / gridDim.x;
    const int64_t k0 = (int64_t)blockIdx.x * per, k1 = k0 + per < total ? k0 + per : total;
    if (k0 >= k1) return;                                          // uniform per workgroup
    for (int i = threadIdx.x; i < kLimbs; i += kThreads) acc[i] = 0;
    if (threadIdx.x == 0) {
        bad = 0;
        ext[0] = ext[1] = -1;
    }
    __syncthreads();
    int cur = mst::segment_of(chunk_first, 0, P, k0);
    for (int64_t k = k0; k < k1; ++k) {
        int p = cur;
        while (k >= chunk_first[p + 1]) ++p;                       // pairs without a record hold no chunk
        if (p != cur) {                                            // the pair changes: flush, start again
            __syncthreads();
            unsigned long long *w = words + (size_t)cur * 2 * kSumWords + PASS * kSumWords;
            for (int i = threadIdx.x; i < kLimbs; i += kThreads) {
                if (acc[i]) atomicAdd(&w[i], acc[i]);
                acc[i] = 0;
            }
            if (threadIdx.x == 0) {
                if (bad) atomicAdd(&w[kLimbs + 1], bad);
                bad = 0;
                if (PASS == 0) {
                    if (ext[0] >= 0) atomicMax(&extent[2 * cur], ext[0]);
                    if (ext[1] >= 0) atomicMax(&extent[2 * cur + 1], ext[1]);
                    ext[0] = ext[1] = -1;
                }
            }
            __syncthreads();
            cur = p;
        }
        const int64_t r0 = seg_off[p] + (k - chunk_first[p]) * kChunk;
        const int64_t end = seg_off[p + 1];
        const int64_t r1 = r0 + kChunk < end ? r0 + kChunk : end;
        const double mean = PASS ? stats[4 * p] : 0.0;
        unsigned long long nbad = 0;
        int mx = -1, my = -1;
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads) {
            double t = v[i];
            if (PASS) {
                const double d = t - mean;
                t = d * d;
            } else {
                const int xi = x[i], yi = y[i];
                mx = xi > mx ? xi : mx;
                my = yi > my ? yi : my;
            }
            if (!add_exact(t, acc)) ++nbad;
        }
        if (nbad) atomicAdd(&bad, nbad);
        if (PASS == 0) {
            mx = wave_max(mx);
            my = wave_max(my);
            if ((threadIdx.x & 63) == 0) {
                if (mx >= 0) atomicMax(&ext[0], mx);
                if (my >= 0) atomicMax(&ext[1], my);
            }
        }
    }
    __syncthreads();
    unsigned long long *w = words + (size_t)cur * 2 * kSumWords + PASS * kSumWords;
    for (int i = threadIdx.x; i < kLimbs; i += kThreads)
        if (acc[i]) atomicAdd(&w[i], acc[i]);
    if (threadIdx.x == 0) {
        if (bad) atomicAdd(&w[kLimbs + 1], bad);
        if (PASS == 0) {
            if (ext[0] >= 0) atomicMax(&extent[2 * cur], ext[0]);
            if (ext[1] >= 0) atomicMax(&extent[2 * cur + 1], ext[1]);
        }
    }
}

// one workgroup per pair.  stats[p] = {mean, std, n, flags}: PASS 0 sets mean and n, PASS 1 std (population: sqrt(sum / n));
// flags = 1 when a value (PASS 0) or a square (PASS 1) was not finite.  A pair without a record keeps {0, 0, 0, 0}.
template <int PASS>
__global__ void zseg_finish_kernel(const unsigned long long *__restrict__ words, const int64_t *__restrict__ seg_off,
                                   double *__restrict__ stats) {
    __shared__ long long digits[kLimbs + 1];
    if (threadIdx.x != 0) return;
    const int p = blockIdx.x;
    const int64_t n = seg_off[p + 1] - seg_off[p];
    if (n <= 0) return;
    const unsigned long long *w = words + (size_t)p * 2 * kSumWords + PASS * kSumWords;
    const double s = exact_to_double(w, digits);
    const bool bad = w[kLimbs + 1] != 0;
    if (PASS == 0) {
        stats[4 * p] = bad ? NAN : s / (double)n;
        stats[4 * p + 2] = (double)n;
    } else {
        stats[4 * p + 1] = bad ? NAN : sqrt(s / (double)n);
    }
    if (bad) stats[4 * p + 3] = 1.0;
}

__global__ void __launch_bounds__(kThreads)
zseg_apply_kernel(const double *__restrict__ v, const int64_t *__restrict__ seg_off, int P, const int64_t *__restrict__ chunk_first,
                  const double *__restrict__ stats, double *__restrict__ out) {
    const int64_t total = chunk_first[P];
    for (int64_t k = blockIdx.x; k < total; k += gridDim.x) {
        const int q = mst::segment_of(chunk_first, 0, P, k);       // chunk_first[q] <= k < chunk_first[q + 1]: q holds records
        const int64_t r0 = seg_off[q] + (k - chunk_first[q]) * kChunk;
        const int64_t end = seg_off[q + 1];
        const int64_t r1 = r0 + kChunk < end ? r0 + kChunk : end;
        const double mean = stats[4 * q], sd = stats[4 * q + 1];
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads) {
            const double z = (v[i] - mean) / sd;
            out[i] = isfinite(z) ? z : 0.0;
        }
    }
}

// ---- windows --------------------------------------------------------------------------------------------------------------
// The windows of one axis (length n, K windows of C) that hold coordinate a: the regular ones [lo, hi] (empty when lo > hi)
// and whether the last one (index K - 1, start max(0, n - C)) does.  K > 1 needs C > kOverlap (the host checks it; a table
// that breaks it names no regular window here).
struct AxisWindows {
    int lo, hi, step, last_start;
    bool last;
};

__device__ __forceinline__ AxisWindows axis_windows(int a, int n, int C, int K) {
    AxisWindows w;
    w.step = C - kOverlap;
    w.last_start = n > C ? n - C : 0;
    w.last = K > 0 && a >= w.last_start && a < n;
    w.lo = 0;
    w.hi = -1;
    if (K > 1 && w.step > 0 && a >= 0 && a < n) {
        const int below = a - C + 1;                               // window i holds a: i step <= a <= i step + C - 1
        w.lo = below > 0 ? (below + w.step - 1) / w.step : 0;
        w.hi = a / w.step;
        if (w.hi > K - 2) w.hi = K - 2;
        if (w.lo > w.hi + 1) w.lo = w.hi + 1;                      // past the regular windows: the last one alone
    }
    return w;
}

__device__ __forceinline__ int window_start(const AxisWindows &w, int i, int K) { return i < K - 1 ? i * w.step : w.last_start; }

// counts[t] += 1 from every active lane, one atomic per distinct tile among the lanes that call together
__device__ __forceinline__ void wave_count(uint32_t *__restrict__ counts, int t) {
    const int lane = threadIdx.x & 63;
    bool done = false;
    while (!done) {
        const unsigned long long waiting = __ballot(1);            // the lanes still in the loop
        const int leader = __ffsll((long long)waiting) - 1;
        const int lt = __shfl(t, leader, 64);
        const unsigned long long same = __ballot(t == lt);
        if (t == lt) {
            if (lane == leader) atomicAdd(&counts[lt], (uint32_t)__popcll(same));
            done = true;
        }
    }
}

// the pair of record i for a thread whose workgroup's first record lies in pair p_block
__device__ __forceinline__ int pair_of(const int64_t *__restrict__ seg_off, int p, int p_end, int64_t i) {
    while (p + 1 < p_end && i >= seg_off[p + 1]) ++p;
    return p;
}

__global__ void __launch_bounds__(kThreads)
count_tiles_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, const double *__restrict__ v,
                   const int64_t *__restrict__ seg_off, const mst_trans_pair *__restrict__ pairs, int P, int64_t T,
                   uint32_t *__restrict__ counts) {
    const int64_t n = seg_off[P];
    for (int64_t b0 = (int64_t)blockIdx.x * kThreads; b0 < n; b0 += (int64_t)gridDim.x * kThreads) {
        const int64_t i = b0 + threadIdx.x;
        if (i >= n) continue;
        const int p = pair_of(seg_off, mst::segment_of(seg_off, 0, P, b0), P, i);
        if (!(v[i] != 0.0)) continue;
        const mst_trans_pair pr = pairs[p];
        const AxisWindows wr = axis_windows(x[i], pr.n1, pr.C, pr.K1), wc = axis_windows(y[i], pr.n2, pr.C, pr.K2);
        for (int a = wr.lo; a <= wr.hi + (wr.last ? 1 : 0); ++a) {
            const int ti = a <= wr.hi ? a : pr.K1 - 1;
            for (int b = wc.lo; b <= wc.hi + (wc.last ? 1 : 0); ++b) {
                const int tj = b <= wc.hi ? b : pr.K2 - 1;
                const int64_t t = pr.tile_base + (int64_t)ti * pr.K2 + tj;
                if (t >= 0 && t < T) wave_count(counts, (int)t);
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads)
scatter_worklist_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, const double *__restrict__ v,
                        const int64_t *__restrict__ seg_off, const mst_trans_pair *__restrict__ pairs, int p0, int p1, int64_t T,
                        const int32_t *__restrict__ slot, int B, int C, double *__restrict__ c) {
    const int64_t first = seg_off[p0], n = seg_off[p1];
    for (int64_t b0 = first + (int64_t)blockIdx.x * kThreads; b0 < n; b0 += (int64_t)gridDim.x * kThreads) {
        const int64_t i = b0 + threadIdx.x;
        if (i >= n) continue;
        const int p = pair_of(seg_off, mst::segment_of(seg_off, p0, p1, b0), p1, i);
        const mst_trans_pair pr = pairs[p];
        if (pr.C != C) continue;                                   // a pair of another tile size inside the range: no tile here
        const int xi = x[i], yi = y[i];
        const double vi = v[i];
        const AxisWindows wr = axis_windows(xi, pr.n1, C, pr.K1), wc = axis_windows(yi, pr.n2, C, pr.K2);
        for (int a = wr.lo; a <= wr.hi + (wr.last ? 1 : 0); ++a) {
            const int ti = a <= wr.hi ? a : pr.K1 - 1;
            const int r = xi - window_start(wr, ti, pr.K1);
            for (int b = wc.lo; b <= wc.hi + (wc.last ? 1 : 0); ++b) {
                const int tj = b <= wc.hi ? b : pr.K2 - 1;
                const int q = yi - window_start(wc, tj, pr.K2);
                const int64_t t = pr.tile_base + (int64_t)ti * pr.K2 + tj;
                if (t < 0 || t >= T) continue;
                const int s = slot[t];
                if (s >= 0 && s < B && r >= 0 && r < C && q >= 0 && q < C) c[((int64_t)s * C + r) * C + q] = vi;
            }
        }
    }
}

int grid_for(long long n, int per, int cap) {
    const long long want = (n + per - 1) / per;
    return (int)(want < cap ? (want > 0 ? want : 1) : cap);
}

}  // namespace

extern "C" uint64_t mst_trans_zscore_segmented_workspace_bytes(int32_t P) {
    if (P <= 0 || P > 65535) return 0;
    return words_offset(P) + (uint64_t)P * 2 * kSumWords * 8;
}

extern "C" int mst_trans_zscore_segmented(const int32_t *x, const int32_t *y, const double *v, int64_t n, const int64_t *seg_off,
                                          int32_t P, double *out, double *stats, int32_t *extent, void *workspace,
                                          uint64_t workspace_bytes, void *stream) {
    MST_RANGE("trans: mst_trans_zscore_segmented");
    if (!seg_off || !stats || !extent || !workspace || P <= 0 || P > 65535 || n < 0 || n >= ((int64_t)1 << 31) ||
        (n > 0 && (!x || !y || !v || !out)) || workspace_bytes < mst_trans_zscore_segmented_workspace_bytes(P))
        return mst::fail(MST_E_ARG, "mst_trans_zscore_segmented: bad argument (1 <= P <= 65535 pairs, n < 2^31 records, "
                                    "workspace of mst_trans_zscore_segmented_workspace_bytes(P))");
    hipStream_t s = mst::as_stream(stream);
    auto *chunk_first = static_cast<int64_t *>(workspace);
    auto *w = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + words_offset(P));
    MST_HIP(hipMemsetAsync(workspace, 0, mst_trans_zscore_segmented_workspace_bytes(P), s));
    MST_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(double) * (size_t)P, s));
    MST_HIP(hipMemsetAsync(extent, 0xFF, 2 * sizeof(int32_t) * (size_t)P, s));      // -1: no record
    if (n == 0) return MST_OK;
    chunk_table_kernel<<<1, 64, 0, s>>>(seg_off, P, chunk_first);
    const int g = grid_for(n, 4 * kChunk, 2048);                  // a workgroup's run of chunks: 4 or more where there are many
    zseg_sum_kernel<0><<<g, kThreads, 0, s>>>(x, y, v, seg_off, P, chunk_first, stats, w, extent);
    zseg_finish_kernel<0><<<P, 64, 0, s>>>(w, seg_off, stats);
    zseg_sum_kernel<1><<<g, kThreads, 0, s>>>(x, y, v, seg_off, P, chunk_first, stats, w, extent);
    zseg_finish_kernel<1><<<P, 64, 0, s>>>(w, seg_off, stats);
    zseg_apply_kernel<<<grid_for(n, kChunk, 4096), kThreads, 0, s>>>(v, seg_off, P, chunk_first, stats, out);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_trans_count_tiles(const int32_t *x, const int32_t *y, const double *v, int64_t n, const int64_t *seg_off,
                                     const mst_trans_pair *pairs, int32_t P, int64_t T, uint32_t *counts, void *stream) {
    MST_RANGE("trans: mst_trans_count_tiles");
    if (!seg_off || !pairs || P <= 0 || T < 0 || T >= ((int64_t)1 << 31) || (T > 0 && !counts) || n < 0 ||
        (n > 0 && (!x || !y || !v)))
        return mst::fail(MST_E_ARG, "mst_trans_count_tiles: bad argument (P >= 1 pairs, T < 2^31 tiles)");
    hipStream_t s = mst::as_stream(stream);
    if (T > 0) MST_HIP(hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)T, s));
    if (n == 0 || T == 0) return MST_OK;
    count_tiles_kernel<<<grid_for(n, kThreads, 8192), kThreads, 0, s>>>(x, y, v, seg_off, pairs, P, T, counts);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_trans_scatter_worklist(const int32_t *x, const int32_t *y, const double *v, const int64_t *seg_off,
                                          const mst_trans_pair *pairs, int32_t p0, int32_t p1, int64_t n_range, int64_t T,
                                          const int32_t *slot, int32_t B, int32_t CH, double *c, void *stream) {
    MST_RANGE("trans: mst_trans_scatter_worklist");
    if (!c || !seg_off || !pairs || !slot || p0 < 0 || p1 <= p0 || T <= 0 || T >= ((int64_t)1 << 31) || B <= 0 || CH <= 0 ||
        n_range < 0 || (n_range > 0 && (!x || !y || !v)))
        return mst::fail(MST_E_ARG, "mst_trans_scatter_worklist: bad argument (pairs [p0, p1) with p0 < p1, B >= 1, T < 2^31)");
    hipStream_t s = mst::as_stream(stream);
    MST_HIP(hipMemsetAsync(c, 0, sizeof(double) * (size_t)B * CH * CH, s));
    if (n_range == 0) return MST_OK;
    scatter_worklist_kernel<<<grid_for(n_range, kThreads, 8192), kThreads, 0, s>>>(x, y, v, seg_off, pairs, p0, p1, T, slot, B, CH, c);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
