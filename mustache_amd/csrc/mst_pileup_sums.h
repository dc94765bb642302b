// Fixed-order block sums and the window limits shared by the pile-up kernels (mst_pileup.hip, mst_pileup_trans_batch.hip).
#pragma once
#include "mst_common.h"

namespace mst_pileup {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxW = 64;

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

inline uint64_t align256(uint64_t b) { return (b + 255) & ~uint64_t(255); }

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

}  // namespace mst_pileup
