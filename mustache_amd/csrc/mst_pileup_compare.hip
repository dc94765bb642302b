// One loop list piled up on two maps (mustache_amd/pileup.py states the rules, "Two maps"; tests/pileup_compare_reference.py
// restates them in NumPy): the arithmetic over the two stacks of oe windows the two pile-ups leave on the device, under the
// joint mask -- a cell of loop l is shared when neither oe1[l] nor oe2[l] is NaN there.
//
//   mst_pileup_compare      sums[l][N][0..2] = S_1, S_2, cnt over the shared cells of neighbourhood N (DONUT, LL, H, V) of loop l
// The paired aggregate is mst_pileup_reduce_pair (mst_pileup_reduce.hip).
//
// One wave per loop, kWaves loops per workgroup, over the loop's two contiguous windows: the walk, the four neighbourhoods and the
// order of every addition are neighbourhood_sums' (mst_pileup_sums.h), the kernel says what a cell is.  No LDS, no atomics, no
// workspace, no barrier; the order of every sum depends only on the cell index, so a loop's twelve numbers have the same bits in
// every run, at any position in the list and for any L.
#include <cmath>
#include "mst_common.h"
#include "mst_pileup_sums.h"

namespace {

using mst_pileup::grid_ok;
using mst_pileup::kThreads;
using mst_pileup::kWaves;

__global__ void __launch_bounds__(kThreads)
compare_kernel(const double *__restrict__ oe1, const double *__restrict__ oe2, int64_t L, int32_t w, int32_t p,
               double *__restrict__ sums) {
    const int64_t l = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (l >= L) return;                                    // the whole wave leaves: there is no barrier below
    const int64_t cells = (int64_t)(2 * w + 1) * (2 * w + 1);
    const double *win1 = oe1 + l * cells, *win2 = oe2 + l * cells;
    mst_pileup::neighbourhood_sums(w, p, [&](int c, int, int, bool &shared, double &u, double &v) {
        u = win1[c];
        v = win2[c];
        shared = u == u && v == v;
    }, sums + l * 12);
}

}  // namespace

extern "C" int mst_pileup_compare(const double *oe1, const double *oe2, int64_t L, int32_t w, int32_t p, double *sums,
                                  void *stream) {
    MST_RANGE("pileup: mst_pileup_compare");
    int rc = mst_pileup::check_peak("mst_pileup_compare", w, p);
    if (rc != MST_OK) return rc;
    if (L < 0) return mst::fail(MST_E_ARG, "mst_pileup_compare: bad argument (L %lld)", (long long)L);
    if (L == 0) return MST_OK;
    if (!oe1 || !oe2 || !sums)
        return mst::fail(MST_E_ARG, "mst_pileup_compare: null %s with L = %lld", !oe1 ? "oe1" : !oe2 ? "oe2" : "sums", (long long)L);
    const int64_t blocks = (L + kWaves - 1) / kWaves;
    if ((rc = grid_ok("mst_pileup_compare", blocks)) != MST_OK) return rc;
    compare_kernel<<<(unsigned)blocks, kThreads, 0, mst::as_stream(stream)>>>(oe1, oe2, L, w, p, sums);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
