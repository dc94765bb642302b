// Local enrichment of every loop of a pile-up (mustache_amd/pileup.py states the rules, "Enrichment"; tests/pileup_enrich_reference.py
// restates them in NumPy): over each loop's (2w+1) x (2w+1) window of obs, which the pile-up already holds on the device, the
// sums S_o = sum obs, S_e = sum e and the count of the counted cells of HiCCUPS's four neighbourhoods, in the order DONUT, LL,
// H, V.  The ratios are the host's work (pileup.enrichment).
//
//   mst_pileup_enrich    sums[l][N][0..2] = S_o, S_e, cnt of neighbourhood N of loop l
//
// One wave per loop, kWaves loops per workgroup, over the loop's contiguous window: the walk, the four neighbourhoods and the
// order of every addition are neighbourhood_sums' (mst_pileup_sums.h), the kernel says what a cell is.  No LDS, no atomics, no
// workspace, no barrier.  The order of every sum depends only on the cell index, so a loop's twelve numbers have the same bits
// in every run, at any position in the list and for any L.
#include <cmath>
#include "mst_common.h"
#include "mst_pileup_sums.h"

namespace {

using mst_pileup::grid_ok;
using mst_pileup::kThreads;
using mst_pileup::kWaves;

// kCis: e of cell (a, b) is expected[|(y + b) - (x + a)|] (0 beyond D); otherwise the loop's own scalar e_loop[l].
template <bool kCis>
__global__ void __launch_bounds__(kThreads)
enrich_kernel(const double *__restrict__ obs, int64_t L, int32_t w, int32_t p, const double *__restrict__ expected, int32_t D,
              const int64_t *__restrict__ xs, const int64_t *__restrict__ ys, const double *__restrict__ e_loop,
              double *__restrict__ sums) {
    const int64_t l = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (l >= L) return;                                    // the whole wave leaves: there is no barrier below
    const double *win = obs + l * (int64_t)(2 * w + 1) * (2 * w + 1);
    const int64_t sep = kCis ? ys[l] - xs[l] : 0;          // (y + b) - (x + a) = sep + b - a
    const double e_own = kCis ? 0.0 : e_loop[l];
    mst_pileup::neighbourhood_sums(w, p, [&](int c, int a, int b, bool &counted, double &o, double &e) {
        o = win[c];
        e = e_own;
        if (kCis) {
            const int64_t k = sep + b - a, dd = k < 0 ? -k : k;
            e = dd <= D ? expected[dd] : 0.0;
        }
        counted = o == o && e != 0.0;
    }, sums + l * 12);
}

}  // namespace

extern "C" int mst_pileup_enrich(const double *obs, int64_t L, int32_t w, int32_t p, const double *expected, int32_t D,
                                 const int64_t *xs, const int64_t *ys, const double *e_loop, double *sums, void *stream) {
    MST_RANGE("pileup: mst_pileup_enrich");
    int rc = mst_pileup::check_peak("mst_pileup_enrich", w, p);
    if (rc != MST_OK) return rc;
    if (L < 0) return mst::fail(MST_E_ARG, "mst_pileup_enrich: bad argument (L %lld)", (long long)L);
    if (L == 0) return MST_OK;
    if ((expected != nullptr) == (e_loop != nullptr))
        return mst::fail(MST_E_ARG, "mst_pileup_enrich: exactly one of expected (cis) and e_loop (trans) is given");
    if (!obs || !sums || (expected && (!xs || !ys || D < 0)))
        return mst::fail(MST_E_ARG, "mst_pileup_enrich: bad argument (null obs, sums, xs or ys, or D %d < 0)", (int)D);
    const int64_t blocks = (L + kWaves - 1) / kWaves;
    if ((rc = grid_ok("mst_pileup_enrich", blocks)) != MST_OK) return rc;
    hipStream_t s = mst::as_stream(stream);
    if (expected)
        enrich_kernel<true><<<(unsigned)blocks, kThreads, 0, s>>>(obs, L, w, p, expected, D, xs, ys, nullptr, sums);
    else
        enrich_kernel<false><<<(unsigned)blocks, kThreads, 0, s>>>(obs, L, w, p, nullptr, 0, nullptr, nullptr, e_loop, sums);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
