// What the pile-up kernels share (mst_pileup*.hip): fixed-order block sums, the window limits and argument checks, the sizes of
// the reduce (mst_pileup_reduce.hip) and the walk over a window's four neighbourhoods (mst_pileup_enrich.hip,
// mst_pileup_compare.hip).
#pragma once
#include "mst_common.h"

namespace mst_pileup {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxW = 64;
constexpr int kMaxPairs = 65535;
constexpr int kLoopChunk = 512;            // loops per chunk of the reduce
constexpr int kLoopsPerWave = kLoopChunk / kWaves;

__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);
    return a;
}

__device__ __forceinline__ long long wave_sum_l(long long a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    return a;
}

// block totals in a fixed order: butterfly inside each wave, then the waves in index order.  Every thread gets them.
__device__ __forceinline__ void block_sum2(double &a, long long &c, double *lds, long long *ldc) {
    a = wave_sum(a);
    c = wave_sum_l(c);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
        lds[wave] = a;
        ldc[wave] = c;
    }
    __syncthreads();
    double t = 0.0;
    long long tc = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        t = t + lds[w];
        tc += ldc[w];
    }
    a = t;
    c = tc;
}

// ---- the four neighbourhoods of one window, by one wave ---------------------------------------------------------------------------
// Lane t takes the cells t, t + 64, ... of the (2w+1) x (2w+1) window in that order; cell(c, a, b, counted, first, second) loads
// cell c = (a + w)(2w + 1) + (b + w) and says whether it counts and which two numbers it adds.  Two trips' cells are asked for
// before the first addition, so their loads are in flight together; the additions stay in cell order.  out[N][0..2] = sum first,
// sum second, count over the counted cells of N = DONUT, LL, H, V (pileup.py, "Enrichment"; p is the peak half-width): the lane
// sums go through the butterfly, lane 0 stores.  No LDS, no barrier; every lane of the wave must call.
template <typename Cell>
__device__ __forceinline__ void neighbourhood_sums(int32_t w, int32_t p, const Cell &cell, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int S = 2 * w + 1, cells = S * S;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    int cn[4] = {0, 0, 0, 0};
    // cell c = row * S + col walks on by 64 = dr * S + dc; dc < S when S <= 64 and col + 64 < 2S when S > 64: one carry at most
    const int dr = 64 / S, dc = 64 % S;
    int row = lane / S, col = lane % S;
    for (int c = lane; c < cells; c += 128) {
        int a[2], b[2];
        bool counted[2];
        double u[2], v[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = row - w;
            b[t] = col - w;
            row += dr;
            col += dc;
            if (col >= S) {
                col -= S;
                ++row;
            }
        }
        const bool second = c + 64 < cells;                // no branch around a load: a lane without a second cell re-reads c
        cell(c, a[0], b[0], counted[0], u[0], v[0]);
        cell(second ? c + 64 : c, second ? a[1] : a[0], second ? b[1] : b[0], counted[1], u[1], v[1]);
        counted[1] = counted[1] && second;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int aa = a[t] < 0 ? -a[t] : a[t], ab = b[t] < 0 ? -b[t] : b[t];
            const bool outside = aa > p || ab > p;         // of the peak box
            const bool in[4] = {outside && a[t] != 0 && b[t] != 0, outside && a[t] >= 1 && b[t] <= -1, aa <= 1 && ab > p,
                                ab <= 1 && aa > p};
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (counted[t] && in[m]) {
                    s1[m] = s1[m] + u[t];
                    s2[m] = s2[m] + v[t];
                    ++cn[m];
                }
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
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            out[m * 3 + 0] = s1[m];
            out[m * 3 + 1] = s2[m];
            out[m * 3 + 2] = (double)((packed >> (16 * m)) & 0xFFFF);
        }
    }
}

inline uint64_t align256(uint64_t b) { return (b + 255) & ~uint64_t(255); }

inline int64_t loop_chunks(int64_t L) { return (L + kLoopChunk - 1) / kLoopChunk; }
inline int64_t cells_of(int w) { return (int64_t)(2 * w + 1) * (2 * w + 1); }
// the reduce's partial sums: [chunks][rows][cells] f64 -- what a call needs; the size queries round it up to 256
inline uint64_t partials_bytes(int64_t nchunks, int rows, int w) { return (uint64_t)nchunks * rows * cells_of(w) * 8; }

inline int grid_ok(const char *who, int64_t blocks) {
    if (blocks < 1 || blocks * kThreads > (int64_t)UINT32_MAX)
        return mst::fail(MST_E_ARG, "%s: %lld workgroups exceed the launch limit", who, (long long)blocks);
    return MST_OK;
}

inline int check_w(const char *who, int32_t w, int32_t q) {
    if (w < 0 || w > kMaxW)
        return mst::fail(MST_E_ARG, "%s: window half-width w = %d is outside 0 .. %d (at most %d cells per window)", who, (int)w,
                         kMaxW, (2 * kMaxW + 1) * (2 * kMaxW + 1));
    if (q < 1 || q > 2 * w + 1)
        return mst::fail(MST_E_ARG, "%s: corner size q = %d is outside 1 .. 2w + 1 = %d", who, (int)q, (int)(2 * w + 1));
    return MST_OK;
}

// the window and the peak box of the per-loop neighbourhood sums
inline int check_peak(const char *who, int32_t w, int32_t p) {
    const int rc = check_w(who, w, 1);
    if (rc != MST_OK) return rc;
    if (p < 0 || p >= w)
        return mst::fail(MST_E_ARG, "%s: peak half-width p = %d is outside 0 .. w - 1 = %d", who, (int)p, (int)w - 1);
    return MST_OK;
}

inline int check_pairs(const char *who, int32_t P) {
    if (P < 1 || P > kMaxPairs) return mst::fail(MST_E_ARG, "%s: P = %d pairs is outside 1 .. %d", who, (int)P, kMaxPairs);
    return MST_OK;
}

// a host table of P + 1 offsets, non-decreasing from 0 to `total`
inline bool offsets_ok(const int64_t *off, int32_t P, int64_t total) {
    if (!off || off[0] != 0 || off[P] != total) return false;
    for (int32_t p = 0; p < P; ++p)
        if (off[p + 1] < off[p]) return false;
    return true;
}

}  // namespace mst_pileup
