// Aggregate peak analysis (APA) of a loop list on one chromosome's raw band (mustache_amd/pileup.py states the rules;
// tests/pileup_reference.py restates them in NumPy).
//
//   mst_pileup_expected  valid bins and the expected count per diagonal, E[d], d = 0 .. D
//   mst_pileup_windows   one (2w+1) x (2w+1) window of obs and oe per loop, its centre and its own P2LL
// The reduce over the windows is mst_pileup_reduce (mst_pileup_reduce.hip).
//
// The band is diagonal-major (band[d * n + i] = pixel (i, i + d), csrc/mst_band.hip), raw counts, at least D + 1 rows.
// Every sum runs in a fixed order that depends only on absolute positions: E[d] adds fixed kColChunk-column chunks of an
// absolute column grid (each a fixed per-thread order plus a fixed tree), then the chunks in chunk order.  No float atomics: the
// results are bit-identical from run to run.  The valid flags are plain racing stores of the value 1.
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
constexpr int kMaxW = mst_pileup::kMaxW;

inline int64_t col_chunks(int64_t n) { return (n + kColChunk - 1) / kColChunk; }

// workspace, used in turn from its start: mst_pileup_expected's partial sums [(D+1) x chunks] f64 and counts (same) int64, then
// mst_pileup_reduce's partials (mst_pileup_sums.h)
inline uint64_t ws_expected(int64_t n, int32_t D) { return 2 * align256((uint64_t)(D + 1) * col_chunks(n) * 8); }

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

int check_band(const char *who, const double *band, int64_t n, int32_t band_rows, int32_t D) {
    if (!band || n <= 0 || D < 0 || band_rows < D + 1)
        return mst::fail(MST_E_ARG, "%s: bad band (n %lld, rows %d, D %d: the band needs at least D + 1 rows)", who, (long long)n,
                         (int)band_rows, (int)D);
    return MST_OK;
}

}  // namespace

extern "C" uint64_t mst_pileup_workspace_bytes(int64_t n, int32_t D, int64_t L, int32_t w) {
    if (n <= 0 || D < 0 || L < 0 || w < 0 || w > kMaxW) return 0;
    const uint64_t a = ws_expected(n, D), b = align256(mst_pileup::partials_bytes(mst_pileup::loop_chunks(L), 4, w));      // used in turn
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
