// Aggregate peak analysis (APA) of a loop list on one chromosome's raw band (mustache_amd/pileup.py states the rules;
// tests/pileup_reference.py restates them in NumPy).
//
//   mst_pileup_expected  valid bins and the expected count per diagonal, E[d], d = 0 .. D
//   mst_pileup_windows   one (2w+1) x (2w+1) window of obs and oe per loop, its centre and its own P2LL
//   mst_pileup_reduce    per cell: sum and non-NaN count of obs and oe over the loops, in a given (sorted) loop order
//
// The band is diagonal-major (band[d * n + i] = pixel (i, i + d), csrc/mst_band.hip), raw counts, at least D + 1 rows.
// Every sum runs in a fixed order that depends only on absolute positions: E[d] adds fixed kColChunk-column chunks of an
// absolute column grid (each a fixed per-thread order plus a fixed tree), then the chunks in chunk order; the reduce adds
// kLoopChunk-loop chunks of the sorted order (four waves of 128 loops each, in order, then the waves in index order), then the
// chunks in chunk order.  No float atomics: the results are bit-identical from run to run and under any permutation of the
// loops the caller sorts.  The valid flags are plain racing stores of the value 1.
#include <cmath>
#include "mst_common.h"
#include "mst_pileup_sums.h"

namespace {

using mst_pileup::align256;
using mst_pileup::block_sum2;
using mst_pileup::check_w;
using mst_pileup::grid_ok;
using mst_pileup::kThreads;
using mst_pileup::kWaves;
constexpr int kValidRows = 32;             // band rows per workgroup of the valid pass
constexpr int kColChunk = 4096;            // columns per chunk of the expected pass (absolute grid)
constexpr int kLoopChunk = 512;            // loops per chunk of the reduce
constexpr int kLoopsPerWave = kLoopChunk / kWaves;
constexpr int kMaxW = mst_pileup::kMaxW;

inline int64_t col_chunks(int64_t n) { return (n + kColChunk - 1) / kColChunk; }
inline int64_t loop_chunks(int64_t L) { return (L + kLoopChunk - 1) / kLoopChunk; }
inline int64_t cells_of(int w) { return (int64_t)(2 * w + 1) * (2 * w + 1); }

// workspace, used in turn from its start: mst_pileup_expected's partial sums [(D+1) x chunks] f64 and counts (same) int64, then
// mst_pileup_reduce's partials [chunks][4][cells] f64
inline uint64_t ws_expected(int64_t n, int32_t D) { return 2 * align256((uint64_t)(D + 1) * col_chunks(n) * 8); }
inline uint64_t ws_reduce(int64_t L, int32_t w) { return align256((uint64_t)loop_chunks(L) * 4 * cells_of(w) * 8); }

// ---- valid bins: bin i is valid when a non-zero pixel (i, j), |i - j| <= D, touches it -----------------------------------
// Workgroup (column block cb, row block rb): thread t reads band[d][i] for i = cb * 256 + t and kValidRows rows d.  A hit
// marks i itself (the pixel's row) and i + d (its column) -- the columns through an LDS map of the 256 + kValidRows - 1 bins
// the tile can reach, written to global memory once per workgroup.
__global__ void __launch_bounds__(kThreads)
valid_kernel(const double *__restrict__ band, int64_t n, int32_t D, int64_t col_blocks, uint8_t *__restrict__ valid) {
    __shared__ uint8_t hit[kThreads + kValidRows];
    const int t = threadIdx.x;
    const int64_t cb = blockIdx.x % col_blocks, rb = blockIdx.x / col_blocks;
    const int64_t i0 = cb * kThreads, d0 = rb * kValidRows;
    for (int k = t; k < kThreads + kValidRows; k += kThreads) hit[k] = 0;
    __syncthreads();
    const int64_t i = i0 + t;
    bool row = false;
    if (i < n) {
#pragma unroll 8
        for (int r = 0; r < kValidRows; ++r) {
            const int64_t d = d0 + r;
            if (d > D || i + d >= n) break;
            if (band[d * n + i] != 0.0) {
                row = true;
                hit[t + r] = 1;
            }
        }
    }
    if (row) valid[i] = 1;
    __syncthreads();
    for (int k = t; k < kThreads + kValidRows; k += kThreads)
        if (hit[k]) valid[i0 + d0 + k] = 1;                // set only for i + d < n
}

// ---- expected: per (diagonal d, absolute column chunk c) the sum and the count over i in the chunk with i + d < n and both
// ends valid -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
expected_partial_kernel(const double *__restrict__ band, int64_t n, int64_t nck, const uint8_t *__restrict__ valid,
                        double *__restrict__ psum, long long *__restrict__ pcnt) {
    __shared__ double lds[kWaves];
    __shared__ long long ldc[kWaves];
    const int64_t c = blockIdx.x % nck, d = blockIdx.x / nck;
    const int64_t i0 = c * kColChunk;
    const int64_t i1 = (i0 + kColChunk < n - d) ? i0 + kColChunk : n - d;
    double s = 0.0;
    long long cnt = 0;
    const double *row = band + d * n;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
        if (valid[i] && valid[i + d]) {
            s = s + row[i];
            ++cnt;
        }
    }
    block_sum2(s, cnt, lds, ldc);
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = s;                              // index d * nck + c
        pcnt[blockIdx.x] = cnt;
    }
}

__global__ void __launch_bounds__(kThreads)
expected_finish_kernel(int32_t D, int64_t nck, const double *__restrict__ psum, const long long *__restrict__ pcnt,
                       double *__restrict__ expected) {
    const int64_t d = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (d > D) return;
    double s = 0.0;
    long long cnt = 0;
    for (int64_t c = 0; c < nck; ++c) {
        s = s + psum[d * nck + c];
        cnt += pcnt[d * nck + c];
    }
    expected[d] = cnt ? s / (double)cnt : 0.0;
}

// ---- windows: one workgroup per loop.  Wave v takes the window's diagonals k = b - a = -2w + v, -2w + v + 4, ...; along one
// diagonal the pixels (x + a, y + a + k) are consecutive in the band row |y - x + k|, so its lanes read consecutive addresses.
__global__ void __launch_bounds__(kThreads)
windows_kernel(const double *__restrict__ band, int64_t n, int32_t D, const double *__restrict__ expected,
               const int64_t *__restrict__ xs, const int64_t *__restrict__ ys, int32_t w, int32_t q,
               double *__restrict__ obs, double *__restrict__ oe, double *__restrict__ stats) {
    __shared__ double lds[kWaves];
    __shared__ long long ldc[kWaves];
    __shared__ double centre[2];
    const int64_t l = blockIdx.x;
    const int64_t X = xs[l], Y = ys[l];
    const int S = 2 * w + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *o_out = obs + l * (int64_t)S * S, *e_out = oe + l * (int64_t)S * S;
    double ll = 0.0;
    long long ll_n = 0;
    for (int k = -2 * w + wave; k <= 2 * w; k += kWaves) {
        const int a_lo = k < 0 ? -w - k : -w, a_hi = k < 0 ? w : w - k;
        for (int a = a_lo + lane; a <= a_hi; a += 64) {
            const int b = a + k;
            const int64_t i = X + a, j = Y + b;
            double o = NAN, e = NAN;
            if (i >= 0 && j >= 0 && i < n && j < n) {
                const int64_t lo = i < j ? i : j, dd = i < j ? j - i : i - j;
                if (dd <= D) {                             // the caller's D covers every window; farther pixels stay NaN
                    o = band[dd * n + lo];
                    const double ex = expected[dd];
                    e = ex != 0.0 ? o / ex : NAN;
                }
            }
            const int cell = (a + w) * S + (b + w);
            o_out[cell] = o;
            e_out[cell] = e;
            if (a == 0 && b == 0) {
                centre[0] = o;
                centre[1] = e;
            }
            if (a + w >= 2 * w - q + 1 && b + w <= q - 1 && o == o) {      // the loop's own LL corner, on-chromosome cells
                ll = ll + o;
                ++ll_n;
            }
        }
    }
    block_sum2(ll, ll_n, lds, ldc);                        // its barriers also publish centre[]
    if (threadIdx.x == 0) {
        const double mean = ll_n ? ll / (double)ll_n : 0.0;
        stats[l * 3 + 0] = centre[0];
        stats[l * 3 + 1] = centre[1];
        stats[l * 3 + 2] = (ll_n && mean != 0.0) ? centre[0] / mean : NAN;
    }
}

// ---- reduce: workgroup (cell block cb of 64 cells, loop chunk k).  Wave v adds the chunk's loops v * 128 .. v * 128 + 127 in
// sorted order for its 64 cells; the four wave partials are added in wave order.  part[k][0..3][cell].
__global__ void __launch_bounds__(kThreads)
reduce_partial_kernel(const double *__restrict__ obs, const double *__restrict__ oe, const int32_t *__restrict__ order,
                      int64_t L, int64_t cells, int64_t cell_blocks, double *__restrict__ part) {
    __shared__ double red[kWaves][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cb = blockIdx.x % cell_blocks, k = blockIdx.x / cell_blocks;
    const int64_t cell = cb * 64 + lane;
    const int64_t p0 = k * kLoopChunk + (int64_t)wave * kLoopsPerWave;
    const int64_t p1 = (p0 + kLoopsPerWave < L) ? p0 + kLoopsPerWave : L;
    double so = 0.0, co = 0.0, se = 0.0, ce = 0.0;
    if (cell < cells) {
        for (int64_t p = p0; p < p1; ++p) {
            const int64_t l = order[p];
            if (l < 0 || l >= L) continue;
            const double vo = obs[l * cells + cell], ve = oe[l * cells + cell];
            if (vo == vo) {
                so = so + vo;
                co = co + 1.0;
            }
            if (ve == ve) {
                se = se + ve;
                ce = ce + 1.0;
            }
        }
    }
    red[wave][0][lane] = so;
    red[wave][1][lane] = co;
    red[wave][2][lane] = se;
    red[wave][3][lane] = ce;
    __syncthreads();
    if (wave == 0 && cell < cells) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double t = red[0][m][lane];
#pragma unroll
            for (int v = 1; v < kWaves; ++v) t = t + red[v][m][lane];
            part[(k * 4 + m) * cells + cell] = t;
        }
    }
}

__global__ void __launch_bounds__(kThreads)
reduce_finish_kernel(int64_t cells, int64_t nchunks, const double *__restrict__ part, double *__restrict__ agg) {
    const int64_t cell = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (cell >= cells) return;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double t = 0.0;
        for (int64_t k = 0; k < nchunks; ++k) t = t + part[(k * 4 + m) * cells + cell];
        agg[m * cells + cell] = t;
    }
}

int check_band(const char *who, const double *band, int64_t n, int32_t band_rows, int32_t D) {
    if (!band || n <= 0 || D < 0 || band_rows < D + 1)
        return mst::fail(MST_E_ARG, "%s: bad band (n %lld, rows %d, D %d: the band needs at least D + 1 rows)", who, (long long)n,
                         (int)band_rows, (int)D);
    return MST_OK;
}

}  // namespace

extern "C" uint64_t mst_pileup_workspace_bytes(int64_t n, int32_t D, int64_t L, int32_t w) {
    if (n <= 0 || D < 0 || L < 0 || w < 0 || w > kMaxW) return 0;
    const uint64_t a = ws_expected(n, D), b = ws_reduce(L, w);      // the two passes use the workspace in turn
    return (a > b ? a : b) + 256;
}

extern "C" int mst_pileup_expected(const double *band, int64_t n, int32_t band_rows, int32_t D, uint8_t *valid, double *expected,
                                   void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_expected");
    int rc = check_band("mst_pileup_expected", band, n, band_rows, D);
    if (rc != MST_OK) return rc;
    if (!valid || !expected) return mst::fail(MST_E_ARG, "mst_pileup_expected: null valid or expected");
    if (!workspace || workspace_bytes < ws_expected(n, D))
        return mst::fail(MST_E_ARG, "mst_pileup_expected: workspace of %llu bytes, %llu needed",
                         (unsigned long long)workspace_bytes, (unsigned long long)ws_expected(n, D));
    const int64_t col_blocks = (n + kThreads - 1) / kThreads, row_blocks = (D + kValidRows) / kValidRows;
    const int64_t nck = col_chunks(n);
    if ((rc = grid_ok("mst_pileup_expected", col_blocks * row_blocks)) != MST_OK) return rc;
    if ((rc = grid_ok("mst_pileup_expected", nck * (D + 1))) != MST_OK) return rc;
    hipStream_t s = mst::as_stream(stream);
    char *p = static_cast<char *>(workspace);
    double *psum = reinterpret_cast<double *>(p);
    long long *pcnt = reinterpret_cast<long long *>(p + align256((uint64_t)(D + 1) * nck * 8));
    MST_HIP(hipMemsetAsync(valid, 0, (size_t)n, s));
    valid_kernel<<<(unsigned)(col_blocks * row_blocks), kThreads, 0, s>>>(band, n, D, col_blocks, valid);
    MST_LAUNCH_CHECK();
    expected_partial_kernel<<<(unsigned)(nck * (D + 1)), kThreads, 0, s>>>(band, n, nck, valid, psum, pcnt);
    MST_LAUNCH_CHECK();
    expected_finish_kernel<<<(unsigned)((D + kThreads) / kThreads), kThreads, 0, s>>>(D, nck, psum, pcnt, expected);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_pileup_windows(const double *band, int64_t n, int32_t band_rows, int32_t D, const double *expected,
                                  const int64_t *x, const int64_t *y, int64_t L, int32_t w, int32_t q, double *obs, double *oe,
                                  double *loop_stats, void *stream) {
    MST_RANGE("pileup: mst_pileup_windows");
    int rc = check_band("mst_pileup_windows", band, n, band_rows, D);
    if (rc != MST_OK) return rc;
    if ((rc = check_w("mst_pileup_windows", w, q)) != MST_OK) return rc;
    if (L < 0 || (L > 0 && (!expected || !x || !y || !obs || !oe || !loop_stats)))
        return mst::fail(MST_E_ARG, "mst_pileup_windows: bad argument (L %lld)", (long long)L);
    if (L == 0) return MST_OK;
    if ((rc = grid_ok("mst_pileup_windows", L)) != MST_OK) return rc;
    windows_kernel<<<(unsigned)L, kThreads, 0, mst::as_stream(stream)>>>(band, n, D, expected, x, y, w, q, obs, oe, loop_stats);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_pileup_reduce(const double *obs, const double *oe, const int32_t *order, int64_t L, int32_t w, double *agg,
                                 void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_reduce");
    int rc = check_w("mst_pileup_reduce", w, 1);
    if (rc != MST_OK) return rc;
    if (L < 0 || L > INT32_MAX || !agg || (L > 0 && (!obs || !oe || !order)))
        return mst::fail(MST_E_ARG, "mst_pileup_reduce: bad argument (L %lld)", (long long)L);
    const int64_t cells = cells_of(w);
    hipStream_t s = mst::as_stream(stream);
    if (L == 0) {
        MST_HIP(hipMemsetAsync(agg, 0, (size_t)(4 * cells * 8), s));
        return MST_OK;
    }
    if (!workspace || workspace_bytes < ws_reduce(L, w))
        return mst::fail(MST_E_ARG, "mst_pileup_reduce: workspace of %llu bytes, %llu needed",
                         (unsigned long long)workspace_bytes, (unsigned long long)ws_reduce(L, w));
    const int64_t cell_blocks = (cells + 63) / 64, nchunks = loop_chunks(L);
    if ((rc = grid_ok("mst_pileup_reduce", cell_blocks * nchunks)) != MST_OK) return rc;
    double *part = static_cast<double *>(workspace);
    reduce_partial_kernel<<<(unsigned)(cell_blocks * nchunks), kThreads, 0, s>>>(obs, oe, order, L, cells, cell_blocks, part);
    MST_LAUNCH_CHECK();
    reduce_finish_kernel<<<(unsigned)((cells + kThreads - 1) / kThreads), kThreads, 0, s>>>(cells, nchunks, part, agg);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
