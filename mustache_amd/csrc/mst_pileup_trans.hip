// Aggregate peak analysis (APA) of a loop list on an inter-chromosomal (trans) pair's records (mustache_amd/pileup.py states
// the rules; tests/pileup_trans_reference.py restates them in NumPy).  A trans pair has no band and no distance decay: the map
// is the pair's COO records (x = bin of A, y = bin of B, v > 0), the expected value one scalar.
//
//   mst_pileup_trans_windows   one pass over the records for the valid rows / columns, the exact total and the window cells;
//                              then E, oe, each loop's centres and its own P2LL.  mst_pileup_reduce adds the windows up.
//
// Launches behind the call, in stream order:
//   rank_kernel      the loops sorted by row (lx, ties by input position): sx, sy, sid.  One thread per loop counts the loops
//                    before it -- L * L comparisons, L is a loop list (thousands), not a map.
//   init_kernel      one workgroup per loop: its window cells = 0.0, NaN off the map; the bit "some window covers this row"
//                    for its rows lx - w .. lx + w (integer atomicOr into a bitmap of n1 bits).
//   records_kernel   grid-stride over the records, 16 B read each (x, y int32, v f64).  Every record marks valid_rows[x] and
//                    valid_cols[y] (plain racing stores of 1) and adds v to the exact sum (mst_exact_sum.h); a record whose row
//                    bit is set binary-searches sx for the first loop with lx >= x - w, walks the run up to lx <= x + w and
//                    writes the cell of every loop with |y - ly| <= w: a 64-bit integer max on the bit pattern of the positive
//                    double, so a repeated pixel keeps its largest value whatever the order.
//   expected_kernel  E = exact total / (#valid rows * #valid columns), one workgroup (integer counts, one division).
//   finish_kernel    one workgroup per loop: oe = obs / E, the two centres and P2LL in a fixed tree.
//
// The row bits live in LDS when the bitmap fits kLdsFlagWords 32-bit words (n1 <= 131 072 rows: every chromosome at 2 kb and
// coarser); a finer map reads the same bitmap from global memory (it stays in L2).  The exact sum keeps kSumCopies copies of
// its LDS limbs, chosen by lane: the values of a trans map share a few exponents, so the lanes of a wave hit the same limbs, and
// LDS atomics on one address are served one after another.  No float atomics: every output is bit-identical from run to run and
// under any permutation of the records and of the loops.
#include <cmath>
#include "mst_common.h"
#include "mst_exact_sum.h"
#include "mst_pileup_sums.h"

namespace {

using mst_exact::add_exact;
using mst_exact::exact_to_double;
using mst_exact::kLimbs;
using mst_exact::kSumWords;
using mst_pileup::align256;
using mst_pileup::block_sum2;
using mst_pileup::check_w;
using mst_pileup::grid_ok;
using mst_pileup::kThreads;
using mst_pileup::kWaves;

constexpr int kLdsFlagWords = 4096;        // 16 KiB of row bits in LDS = 131 072 rows; beyond, the bitmap is read from global
constexpr int kSumCopies = 16;             // copies of the exact sum's LDS limbs, one per lane & 15
constexpr int kSumStride = kLimbs + 1;     // 67 words: the 16 copies of a limb start in 16 different bank pairs
constexpr int kRecordBlocks = 2048;        // grid cap of the record pass: 8 workgroups for each of the 256 CUs

struct Layout {                            // the workspace, in this order
    uint64_t words, sx, sy, sid, bits, end;
    int64_t nwords;
};

Layout layout(int64_t n1, int64_t L) {
    Layout o;
    o.nwords = (n1 + 31) / 32;
    o.words = 0;
    o.sx = o.words + align256((uint64_t)kSumWords * 8);
    o.sy = o.sx + align256((uint64_t)L * 8);
    o.sid = o.sy + align256((uint64_t)L * 8);
    o.bits = o.sid + align256((uint64_t)L * 4);
    o.end = o.bits + align256((uint64_t)o.nwords * 4);
    return o;
}

// ---- the loops by row ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
rank_kernel(const int64_t *__restrict__ lx, const int64_t *__restrict__ ly, int64_t L, int64_t *__restrict__ sx,
            int64_t *__restrict__ sy, int32_t *__restrict__ sid) {
    __shared__ int64_t tile[kThreads];
    const int64_t l = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t key = l < L ? lx[l] : 0;
    int64_t rank = 0;
    for (int64_t m0 = 0; m0 < L; m0 += kThreads) {
        __syncthreads();
        if (m0 + threadIdx.x < L) tile[threadIdx.x] = lx[m0 + threadIdx.x];
        __syncthreads();
        const int nm = L - m0 < kThreads ? (int)(L - m0) : kThreads;
        for (int k = 0; k < nm; ++k) {
            const int64_t o = tile[k];
            rank += (o < key || (o == key && m0 + k < l)) ? 1 : 0;
        }
    }
    if (l < L) {
        sx[rank] = key;
        sy[rank] = ly[l];
        sid[rank] = (int32_t)l;
    }
}

// ---- windows before the records: 0.0 on the map, NaN off it; the row bits ------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
init_kernel(const int64_t *__restrict__ lx, const int64_t *__restrict__ ly, int64_t n1, int64_t n2, int32_t w,
            double *__restrict__ obs, uint32_t *__restrict__ bits) {
    const int64_t l = blockIdx.x;
    const int64_t X = lx[l], Y = ly[l];
    const int S = 2 * w + 1;
    double *o_out = obs + l * (int64_t)S * S;
    for (int cell = threadIdx.x; cell < S * S; cell += kThreads) {
        const int64_t i = X + cell / S - w, j = Y + cell % S - w;
        o_out[cell] = (i >= 0 && i < n1 && j >= 0 && j < n2) ? 0.0 : NAN;
    }
    if ((int)threadIdx.x < S) {
        const int64_t row = X - w + threadIdx.x;
        if (row >= 0 && row < n1) atomicOr(&bits[row >> 5], 1u << (row & 31));
    }
}

// ---- the one pass over the records -----------------------------------------------------------------------------------------
template <bool LDS_FLAGS>
__global__ void __launch_bounds__(kThreads)
records_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, const double *__restrict__ v, int64_t N, int64_t n1,
               int64_t n2, const int64_t *__restrict__ sx, const int64_t *__restrict__ sy, const int32_t *__restrict__ sid,
               int64_t L, int32_t w, const uint32_t *__restrict__ bits, int32_t nwords, uint8_t *__restrict__ valid_rows,
               uint8_t *__restrict__ valid_cols, double *__restrict__ obs, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long acc[kSumCopies * kSumStride];
    __shared__ unsigned long long bad;
    __shared__ uint32_t flags[LDS_FLAGS ? kLdsFlagWords : 1];
    for (int i = threadIdx.x; i < kSumCopies * kSumStride; i += kThreads) acc[i] = 0;
    if (threadIdx.x == 0) bad = 0;
    if (LDS_FLAGS)
        for (int i = threadIdx.x; i < nwords; i += kThreads) flags[i] = bits[i];
    __syncthreads();
    unsigned long long *mine = acc + (threadIdx.x & (kSumCopies - 1)) * kSumStride;
    const int64_t cells = (int64_t)(2 * w + 1) * (2 * w + 1);
    unsigned long long nbad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        const int64_t xi = x[i], yi = y[i];
        const double vi = v[i];
        if (xi < 0 || xi >= n1 || yi < 0 || yi >= n2) continue;      // not a pixel of this map: ignored altogether
        valid_rows[xi] = 1;
        valid_cols[yi] = 1;
        if (!add_exact(vi, mine)) {
            ++nbad;
            continue;
        }
        const uint32_t word = LDS_FLAGS ? flags[xi >> 5] : bits[xi >> 5];
        if (!((word >> (xi & 31)) & 1u) || !(vi > 0.0)) continue;
        int64_t lo = 0, hi = L;                                       // the first loop with lx >= x - w
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (sx[mid] < xi - w) lo = mid + 1;
            else hi = mid;
        }
        for (int64_t p = lo; p < L; ++p) {
            const int64_t da = xi - sx[p];
            if (da < -w) break;
            const int64_t db = yi - sy[p];
            if (db < -w || db > w) continue;
            long long *cell = reinterpret_cast<long long *>(obs + sid[p] * cells + (da + w) * (2 * w + 1) + (db + w));
            atomicMax(cell, __double_as_longlong(vi));                // positive doubles order like their bit patterns
        }
    }
    if (nbad) atomicAdd(&bad, nbad);
    __syncthreads();
    for (int i = threadIdx.x; i < kLimbs; i += kThreads) {
        unsigned long long t = 0;
#pragma unroll
        for (int c = 0; c < kSumCopies; ++c) t += acc[c * kSumStride + i];
        if (t) atomicAdd(&words[i], t);
    }
    if (threadIdx.x == 0 && bad) atomicAdd(&words[kLimbs + 1], bad);
}

// ---- E = exact total / (#valid rows * #valid columns); NaN when a record was not finite -----------------------------------------
__global__ void __launch_bounds__(kThreads)
expected_kernel(const unsigned long long *__restrict__ words, const uint8_t *__restrict__ valid_rows, int64_t n1,
                const uint8_t *__restrict__ valid_cols, int64_t n2, double *__restrict__ expected) {
    __shared__ double lds[kWaves];
    __shared__ long long ldc[kWaves];
    __shared__ long long digits[kLimbs + 1];
    __shared__ double total;
    if (threadIdx.x == 0) total = exact_to_double(words, digits);
    long long rows = 0, cols = 0;
    double unused = 0.0;
    for (int64_t i = threadIdx.x; i < n1; i += kThreads) rows += valid_rows[i] ? 1 : 0;
    for (int64_t i = threadIdx.x; i < n2; i += kThreads) cols += valid_cols[i] ? 1 : 0;
    block_sum2(unused, rows, lds, ldc);
    block_sum2(unused, cols, lds, ldc);
    if (threadIdx.x != 0) return;
    const long long cnt = rows * cols;
    expected[0] = words[kLimbs + 1] ? NAN : (cnt ? total / (double)cnt : 0.0);
}

// ---- finish: oe, the centres and the loop's own P2LL ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
finish_kernel(const double *__restrict__ obs, const double *__restrict__ expected, int32_t w, int32_t q, double *__restrict__ oe,
              double *__restrict__ stats) {
    __shared__ double lds[kWaves];
    __shared__ long long ldc[kWaves];
    const int64_t l = blockIdx.x;
    const int S = 2 * w + 1;
    const double ex = expected[0];
    const double *o_in = obs + l * (int64_t)S * S;
    double *e_out = oe + l * (int64_t)S * S;
    double ll = 0.0;
    long long ll_n = 0;
    for (int cell = threadIdx.x; cell < S * S; cell += kThreads) {
        const double o = o_in[cell];
        e_out[cell] = (ex != 0.0 && o == o) ? o / ex : NAN;
        const int a = cell / S, b = cell % S;
        if (a >= 2 * w - q + 1 && b <= q - 1 && o == o) {             // the LL index range, cells on the map
            ll = ll + o;
            ++ll_n;
        }
    }
    block_sum2(ll, ll_n, lds, ldc);
    if (threadIdx.x == 0) {
        const double c = o_in[w * S + w];
        const double mean = ll_n ? ll / (double)ll_n : 0.0;
        stats[l * 3 + 0] = c;
        stats[l * 3 + 1] = (ex != 0.0 && c == c) ? c / ex : NAN;
        stats[l * 3 + 2] = (ll_n && mean != 0.0) ? c / mean : NAN;
    }
}

}  // namespace

extern "C" uint64_t mst_pileup_trans_workspace_bytes(int64_t n1, int64_t n2, int64_t L, int32_t w) {
    if (n1 <= 0 || n2 <= 0 || L < 0 || w < 0 || w > mst_pileup::kMaxW) return 0;
    const uint64_t own = layout(n1, L).end, red = mst_pileup_workspace_bytes(1, 0, L, w);    // mst_pileup_reduce comes after
    return (own > red ? own : red) + 256;
}

extern "C" int mst_pileup_trans_windows(const int32_t *x, const int32_t *y, const double *v, int64_t N, int64_t n1, int64_t n2,
                                        const int64_t *lx, const int64_t *ly, int64_t L, int32_t w, int32_t q, uint8_t *valid_rows,
                                        uint8_t *valid_cols, double *expected, double *obs, double *oe, double *loop_stats,
                                        void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_trans_windows");
    int rc = check_w("mst_pileup_trans_windows", w, q);
    if (rc != MST_OK) return rc;
    if (n1 <= 0 || n2 <= 0 || n1 > INT32_MAX || n2 > INT32_MAX || N < 0 || N >= ((int64_t)1 << 31) || L < 0 || L > INT32_MAX ||
        !valid_rows || !valid_cols || !expected || (N > 0 && (!x || !y || !v)) ||
        (L > 0 && (!lx || !ly || !obs || !oe || !loop_stats)))
        return mst::fail(MST_E_ARG, "mst_pileup_trans_windows: bad argument (n1 %lld, n2 %lld, N %lld < 2^31 records, L %lld)",
                         (long long)n1, (long long)n2, (long long)N, (long long)L);
    const Layout o = layout(n1, L);
    if (!workspace || workspace_bytes < o.end)
        return mst::fail(MST_E_ARG, "mst_pileup_trans_windows: workspace of %llu bytes, %llu needed",
                         (unsigned long long)workspace_bytes, (unsigned long long)o.end);
    if (L > 0 && (rc = grid_ok("mst_pileup_trans_windows", L)) != MST_OK) return rc;
    hipStream_t s = mst::as_stream(stream);
    char *p = static_cast<char *>(workspace);
    auto *words = reinterpret_cast<unsigned long long *>(p + o.words);
    auto *sx = reinterpret_cast<int64_t *>(p + o.sx), *sy = reinterpret_cast<int64_t *>(p + o.sy);
    auto *sid = reinterpret_cast<int32_t *>(p + o.sid);
    auto *bits = reinterpret_cast<uint32_t *>(p + o.bits);
    MST_HIP(hipMemsetAsync(words, 0, (size_t)kSumWords * 8, s));
    MST_HIP(hipMemsetAsync(bits, 0, (size_t)o.nwords * 4, s));
    MST_HIP(hipMemsetAsync(valid_rows, 0, (size_t)n1, s));
    MST_HIP(hipMemsetAsync(valid_cols, 0, (size_t)n2, s));
    if (L > 0) {
        rank_kernel<<<(unsigned)((L + kThreads - 1) / kThreads), kThreads, 0, s>>>(lx, ly, L, sx, sy, sid);
        MST_LAUNCH_CHECK();
        init_kernel<<<(unsigned)L, kThreads, 0, s>>>(lx, ly, n1, n2, w, obs, bits);
        MST_LAUNCH_CHECK();
    }
    if (N > 0) {
        const int64_t want = (N + kThreads - 1) / kThreads;
        const unsigned g = (unsigned)(want < kRecordBlocks ? want : kRecordBlocks);
        if (o.nwords <= kLdsFlagWords)
            records_kernel<true><<<g, kThreads, 0, s>>>(x, y, v, N, n1, n2, sx, sy, sid, L, w, bits, (int32_t)o.nwords, valid_rows,
                                                        valid_cols, obs, words);
        else
            records_kernel<false><<<g, kThreads, 0, s>>>(x, y, v, N, n1, n2, sx, sy, sid, L, w, bits, 0, valid_rows, valid_cols, obs,
                                                         words);
        MST_LAUNCH_CHECK();
    }
    expected_kernel<<<1, kThreads, 0, s>>>(words, valid_rows, n1, valid_cols, n2, expected);
    MST_LAUNCH_CHECK();
    if (L > 0) {
        finish_kernel<<<(unsigned)L, kThreads, 0, s>>>(obs, expected, w, q, oe, loop_stats);
        MST_LAUNCH_CHECK();
    }
    return MST_OK;
}
