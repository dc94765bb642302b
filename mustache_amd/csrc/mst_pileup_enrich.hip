// Local enrichment of every loop of a pile-up (mustache_amd/pileup.py states the rules, "Enrichment"; tests/pileup_enrich_reference.py
// restates them in NumPy): over each loop's (2w+1) x (2w+1) window of obs, which the pile-up already holds on the device, the
// sums S_o = sum obs, S_e = sum e and the count of the counted cells of HiCCUPS's four neighbourhoods, in the order DONUT, LL,
// H, V.  The ratios are the host's work (pileup.enrichment).
//
//   mst_pileup_enrich    sums[l][N][0..2] = S_o, S_e, cnt of neighbourhood N of loop l
//
// One wave per loop, kWaves loops per workgroup.  Lane t takes the cells t, t + 64, ... of the loop's contiguous window (one
// coalesced 512-byte load per trip) and keeps the twelve accumulators in registers; the wave total is mst_pileup_sums.h's
// butterfly.  No LDS, no atomics, no workspace, no barrier.  The order of every sum depends only on the cell index, so a loop's
// twelve numbers have the same bits in every run, at any position in the list and for any L.
#include <cmath>
#include "mst_common.h"
#include "mst_pileup_sums.h"

namespace {

using mst_pileup::grid_ok;
using mst_pileup::kMaxW;
using mst_pileup::kThreads;
using mst_pileup::kWaves;
using mst_pileup::wave_sum;
using mst_pileup::wave_sum_l;

// kCis: e of cell (a, b) is expected[|(y + b) - (x + a)|] (0 beyond D); otherwise the loop's own scalar e_loop[l].
template <bool kCis>
__global__ void __launch_bounds__(kThreads)
enrich_kernel(const double *__restrict__ obs, int64_t L, int32_t w, int32_t p, const double *__restrict__ expected, int32_t D,
              const int64_t *__restrict__ xs, const int64_t *__restrict__ ys, const double *__restrict__ e_loop,
              double *__restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t l = (int64_t)blockIdx.x * kWaves + wave;
    if (l >= L) return;                                    // the whole wave leaves: there is no barrier below
    const int S = 2 * w + 1, cells = S * S;
    const double *win = obs + l * (int64_t)cells;
    const int64_t sep = kCis ? ys[l] - xs[l] : 0;          // (y + b) - (x + a) = sep + b - a
    const double e_own = kCis ? 0.0 : e_loop[l];
    double so[4] = {0.0, 0.0, 0.0, 0.0}, se[4] = {0.0, 0.0, 0.0, 0.0};
    int cn[4] = {0, 0, 0, 0};
    // cell c = row * S + col walks on by 64 = dr * S + dc; dc < S when S <= 64 and col + 64 < 2S when S > 64: one carry at most
    const int dr = 64 / S, dc = 64 % S;
    int row = lane / S, col = lane % S;
    for (int c = lane; c < cells; c += 64) {
        const int a = row - w, b = col - w;
        const double o = win[c];
        double e = e_own;
        if (kCis) {
            const int64_t k = sep + b - a, dd = k < 0 ? -k : k;
            e = dd <= D ? expected[dd] : 0.0;
        }
        const bool counted = o == o && e != 0.0;
        const int aa = a < 0 ? -a : a, ab = b < 0 ? -b : b;
        const bool outside = aa > p || ab > p;             // of the peak box
        const bool in[4] = {outside && a != 0 && b != 0, outside && a >= 1 && b <= -1, aa <= 1 && ab > p, ab <= 1 && aa > p};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (counted && in[m]) {
                so[m] = so[m] + o;
                se[m] = se[m] + e;
                ++cn[m];
            }
        }
        row += dr;
        col += dc;
        if (col >= S) {
            col -= S;
            ++row;
        }
    }
    // a neighbourhood has at most (2 * 64)^2 = 16 384 cells: the four counts ride through one butterfly, 16 bits each
    long long packed = (long long)cn[0] | (long long)cn[1] << 16 | (long long)cn[2] << 32 | (long long)cn[3] << 48;
    packed = wave_sum_l(packed);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        so[m] = wave_sum(so[m]);
        se[m] = wave_sum(se[m]);
    }
    if (lane == 0) {
        double *out = sums + l * 12;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            out[m * 3 + 0] = so[m];
            out[m * 3 + 1] = se[m];
            out[m * 3 + 2] = (double)((packed >> (16 * m)) & 0xFFFF);
        }
    }
}

}  // namespace

extern "C" int mst_pileup_enrich(const double *obs, int64_t L, int32_t w, int32_t p, const double *expected, int32_t D,
                                 const int64_t *xs, const int64_t *ys, const double *e_loop, double *sums, void *stream) {
    MST_RANGE("pileup: mst_pileup_enrich");
    if (w < 0 || w > kMaxW)
        return mst::fail(MST_E_ARG, "mst_pileup_enrich: window half-width w = %d is outside 0 .. %d", (int)w, kMaxW);
    if (p < 0 || p >= w)
        return mst::fail(MST_E_ARG, "mst_pileup_enrich: peak half-width p = %d is outside 0 .. w - 1 = %d", (int)p, (int)w - 1);
    if (L < 0) return mst::fail(MST_E_ARG, "mst_pileup_enrich: bad argument (L %lld)", (long long)L);
    if (L == 0) return MST_OK;
    if ((expected != nullptr) == (e_loop != nullptr))
        return mst::fail(MST_E_ARG, "mst_pileup_enrich: exactly one of expected (cis) and e_loop (trans) is given");
    if (!obs || !sums || (expected && (!xs || !ys || D < 0)))
        return mst::fail(MST_E_ARG, "mst_pileup_enrich: bad argument (null obs, sums, xs or ys, or D %d < 0)", (int)D);
    const int64_t blocks = (L + kWaves - 1) / kWaves;
    int rc = grid_ok("mst_pileup_enrich", blocks);
    if (rc != MST_OK) return rc;
    hipStream_t s = mst::as_stream(stream);
    if (expected)
        enrich_kernel<true><<<(unsigned)blocks, kThreads, 0, s>>>(obs, L, w, p, expected, D, xs, ys, nullptr, sums);
    else
        enrich_kernel<false><<<(unsigned)blocks, kThreads, 0, s>>>(obs, L, w, p, nullptr, 0, nullptr, nullptr, e_loop, sums);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
