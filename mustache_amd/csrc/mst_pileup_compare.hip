// One loop list piled up on two maps (mustache_amd/pileup.py states the rules, "Two maps"; tests/pileup_compare_reference.py
// restates them in NumPy): the arithmetic over the two stacks of oe windows the two pile-ups leave on the device, under the
// joint mask -- a cell of loop l is shared when neither oe1[l] nor oe2[l] is NaN there.
//
//   mst_pileup_compare      sums[l][N][0..2] = S_1, S_2, cnt over the shared cells of neighbourhood N (DONUT, LL, H, V) of loop l
//   mst_pileup_reduce_pair  agg[0..2][cell] = T_1, T_2, C: per cell the two sums and the number of the loops that share it
//
// mst_pileup_compare is enrich_kernel (mst_pileup_enrich.hip) over two windows: one wave per loop, kWaves loops per workgroup,
// lane t on the cells t, t + 64, ... of both windows (two coalesced 512-byte loads per cell, the loads of two cells requested
// together), the eight sums and the four counts in registers, mst_pileup_sums.h's butterfly at the end.  No LDS, no atomics, no workspace, no barrier; the order of
// every sum depends only on the cell index, so a loop's twelve numbers have the same bits in every run, at any position in the
// list and for any L.
//
// mst_pileup_reduce_pair has the shape and the addition order of mst_pileup_reduce (mst_pileup.hip): workgroup (block of 64
// cells, chunk of 512 loops), wave v adds the chunk's loops v * 128 .. v * 128 + 127 in sorted order, the wave partials are
// added in wave order and the chunk partials in chunk order.  Where the NaN masks of oe1 and oe2 coincide its three rows have
// the bits of mst_pileup_reduce's sum of oe1, sum of oe2 and count.  What differs is how the loads are issued: a wave fetches
// 64 order entries with one load (lane j holds entry j) and takes each from its lane by a shuffle, and it requests the windows
// of kAhead loops -- 2 * kAhead loads -- before the first addition, so the latency of a window load is paid once per kAhead
// loops instead of once per loop.  The additions keep their order.
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

constexpr int kLoopChunk = 512;                        // loops per chunk: mst_pileup_reduce's
constexpr int kLoopsPerWave = kLoopChunk / kWaves;
constexpr int kAhead = 8;                              // loops whose windows a wave requests before it adds the first
static_assert(64 % kAhead == 0, "a group of 64 order entries is walked in whole steps of kAhead");

inline int64_t loop_chunks(int64_t L) { return (L + kLoopChunk - 1) / kLoopChunk; }
inline int64_t cells_of(int w) { return (int64_t)(2 * w + 1) * (2 * w + 1); }

__global__ void __launch_bounds__(kThreads)
compare_kernel(const double *__restrict__ oe1, const double *__restrict__ oe2, int64_t L, int32_t w, int32_t p,
               double *__restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t l = (int64_t)blockIdx.x * kWaves + wave;
    if (l >= L) return;                                    // the whole wave leaves: there is no barrier below
    const int S = 2 * w + 1, cells = S * S;
    const double *win1 = oe1 + l * (int64_t)cells, *win2 = oe2 + l * (int64_t)cells;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    int cn[4] = {0, 0, 0, 0};
    // cell c = row * S + col walks on by 64 = dr * S + dc; dc < S when S <= 64 and col + 64 < 2S when S > 64: one carry at most
    const int dr = 64 / S, dc = 64 % S;
    int row = lane / S, col = lane % S;
    // two trips' loads (cells c and c + 64 of both windows) are requested together; the additions stay in cell order
    for (int c = lane; c < cells; c += 128) {
        const bool second = c + 64 < cells;
        const int c2 = second ? c + 64 : c;                // no branch around a load: a lane without a second cell re-reads c
        const double u2[2] = {win1[c], win1[c2]}, v2[2] = {win2[c], win2[c2]};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int a = row - w, b = col - w;
            const double u = u2[t], v = v2[t];
            const bool shared = u == u && v == v && (t == 0 || second);
            const int aa = a < 0 ? -a : a, ab = b < 0 ? -b : b;
            const bool outside = aa > p || ab > p;         // of the peak box
            const bool in[4] = {outside && a != 0 && b != 0, outside && a >= 1 && b <= -1, aa <= 1 && ab > p, ab <= 1 && aa > p};
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (shared && in[m]) {
                    s1[m] = s1[m] + u;
                    s2[m] = s2[m] + v;
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
    }
    // a neighbourhood has at most (2 * 64)^2 = 16 384 cells: the four counts ride through one butterfly, 16 bits each
    long long packed = (long long)cn[0] | (long long)cn[1] << 16 | (long long)cn[2] << 32 | (long long)cn[3] << 48;
    packed = wave_sum_l(packed);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        s1[m] = wave_sum(s1[m]);
        s2[m] = wave_sum(s2[m]);
    }
    if (lane == 0) {
        double *out = sums + l * 12;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            out[m * 3 + 0] = s1[m];
            out[m * 3 + 1] = s2[m];
            out[m * 3 + 2] = (double)((packed >> (16 * m)) & 0xFFFF);
        }
    }
}

// part[k][0..2][cell].  Every lane of a wave runs every trip of both loops -- the shuffles need them all -- and a lane past the
// last cell, or an order entry that is past the wave's range or outside 0 .. L-1, carries NaN: not shared.
__global__ void __launch_bounds__(kThreads)
reduce_pair_partial_kernel(const double *__restrict__ oe1, const double *__restrict__ oe2, const int32_t *__restrict__ order,
                           int64_t L, int64_t cells, int64_t cell_blocks, double *__restrict__ part) {
    __shared__ double red[kWaves][3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cb = blockIdx.x % cell_blocks, k = blockIdx.x / cell_blocks;
    const int64_t cell = cb * 64 + lane;
    const bool mine = cell < cells;
    const int64_t p0 = k * kLoopChunk + (int64_t)wave * kLoopsPerWave;
    const int64_t p1 = (p0 + kLoopsPerWave < L) ? p0 + kLoopsPerWave : L;
    double t1 = 0.0, t2 = 0.0, cn = 0.0;
    for (int64_t g = p0; g < p1; g += 64) {                // wave-uniform bounds
        const int32_t entry = g + lane < p1 ? order[g + lane] : -1;
        const int here = p1 - g < 64 ? (int)(p1 - g) : 64;
        for (int j = 0; j < here; j += kAhead) {
            double u[kAhead], v[kAhead];
#pragma unroll
            for (int i = 0; i < kAhead; ++i) {             // j + i <= 63; an entry past `here` is -1
                const int64_t l = __shfl(entry, j + i, 64);
                const bool ok = mine && l >= 0 && l < L;
                const int64_t at = ok ? l * cells + cell : 0;             // every load is issued, at a safe address (L > 0):
                const double a = oe1[at], b = oe2[at];                     // a branch around a load would wait for each one
                u[i] = ok ? a : NAN;
                v[i] = ok ? b : NAN;
            }
#pragma unroll
            for (int i = 0; i < kAhead; ++i) {
                if (u[i] == u[i] && v[i] == v[i]) {
                    t1 = t1 + u[i];
                    t2 = t2 + v[i];
                    cn = cn + 1.0;
                }
            }
        }
    }
    red[wave][0][lane] = t1;
    red[wave][1][lane] = t2;
    red[wave][2][lane] = cn;
    __syncthreads();
    if (wave == 0 && mine) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            double t = red[0][m][lane];
#pragma unroll
            for (int v = 1; v < kWaves; ++v) t = t + red[v][m][lane];
            part[(k * 3 + m) * cells + cell] = t;
        }
    }
}

__global__ void __launch_bounds__(kThreads)
reduce_pair_finish_kernel(int64_t cells, int64_t nchunks, const double *__restrict__ part, double *__restrict__ agg) {
    const int64_t cell = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (cell >= cells) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        double t = 0.0;
        for (int64_t k = 0; k < nchunks; ++k) t = t + part[(k * 3 + m) * cells + cell];
        agg[m * cells + cell] = t;
    }
}

}  // namespace

extern "C" int mst_pileup_compare(const double *oe1, const double *oe2, int64_t L, int32_t w, int32_t p, double *sums,
                                  void *stream) {
    MST_RANGE("pileup: mst_pileup_compare");
    if (w < 0 || w > kMaxW)
        return mst::fail(MST_E_ARG, "mst_pileup_compare: window half-width w = %d is outside 0 .. %d", (int)w, kMaxW);
    if (p < 0 || p >= w)
        return mst::fail(MST_E_ARG, "mst_pileup_compare: peak half-width p = %d is outside 0 .. w - 1 = %d", (int)p, (int)w - 1);
    if (L < 0) return mst::fail(MST_E_ARG, "mst_pileup_compare: bad argument (L %lld)", (long long)L);
    if (L == 0) return MST_OK;
    if (!oe1 || !oe2 || !sums)
        return mst::fail(MST_E_ARG, "mst_pileup_compare: null %s with L = %lld", !oe1 ? "oe1" : !oe2 ? "oe2" : "sums", (long long)L);
    const int64_t blocks = (L + kWaves - 1) / kWaves;
    int rc = grid_ok("mst_pileup_compare", blocks);
    if (rc != MST_OK) return rc;
    compare_kernel<<<(unsigned)blocks, kThreads, 0, mst::as_stream(stream)>>>(oe1, oe2, L, w, p, sums);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_pileup_reduce_pair(const double *oe1, const double *oe2, const int32_t *order, int64_t L, int32_t w,
                                      double *agg, void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_reduce_pair");
    if (w < 0 || w > kMaxW)
        return mst::fail(MST_E_ARG, "mst_pileup_reduce_pair: window half-width w = %d is outside 0 .. %d", (int)w, kMaxW);
    if (L < 0 || L > INT32_MAX || !agg)
        return mst::fail(MST_E_ARG, "mst_pileup_reduce_pair: bad argument (L %lld, agg %s)", (long long)L, agg ? "given" : "null");
    const int64_t cells = cells_of(w);
    hipStream_t s = mst::as_stream(stream);
    if (L == 0) {
        MST_HIP(hipMemsetAsync(agg, 0, (size_t)(3 * cells * 8), s));
        return MST_OK;
    }
    if (!oe1 || !oe2 || !order)
        return mst::fail(MST_E_ARG, "mst_pileup_reduce_pair: null %s with L = %lld", !oe1 ? "oe1" : !oe2 ? "oe2" : "order",
                         (long long)L);
    const int64_t cell_blocks = (cells + 63) / 64, nchunks = loop_chunks(L);
    const uint64_t need = (uint64_t)nchunks * 3 * cells * 8;         // three quarters of what mst_pileup_reduce needs for (L, w)
    if (!workspace || workspace_bytes < need)
        return mst::fail(MST_E_ARG, "mst_pileup_reduce_pair: workspace of %llu bytes, %llu needed",
                         (unsigned long long)workspace_bytes, (unsigned long long)need);
    int rc = grid_ok("mst_pileup_reduce_pair", cell_blocks * nchunks);
    if (rc != MST_OK) return rc;
    double *part = static_cast<double *>(workspace);
    reduce_pair_partial_kernel<<<(unsigned)(cell_blocks * nchunks), kThreads, 0, s>>>(oe1, oe2, order, L, cells, cell_blocks, part);
    MST_LAUNCH_CHECK();
    reduce_pair_finish_kernel<<<(unsigned)((cells + kThreads - 1) / kThreads), kThreads, 0, s>>>(cells, nchunks, part, agg);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
