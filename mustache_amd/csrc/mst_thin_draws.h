// The draws of the binomial thinning (mustache_amd/downsample.py states the rule), shared by mst_thin.hip (one chromosome's cis
// pixels) and mst_thin_pairs.hip (the trans records of many pairs in one launch): Philox4x32-10, the kept reads of a sequence of
// calls, a count as the kernels take it, and the 64-lane integer sum.
#pragma once
#include "mst_common.h"

namespace mst {

constexpr int64_t kThinHeavy = (int64_t)MST_THIN_HEAVY;
constexpr int64_t kThinMaxCount = 0xFFFFFFFFll;

// Philox4x32-10 (Salmon et al., Random123): the number of the four words of call (c0, c1, c2, c3) under key (k0, k1) that lie
// below T, the first `words` of them only (4: all)
__device__ __forceinline__ uint32_t philox_below(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                 uint32_t T, uint32_t words) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (uint32_t)(c0 < T) + (uint32_t)(words > 1 && c1 < T) + (uint32_t)(words > 2 && c2 < T) + (uint32_t)(words > 3 && c3 < T);
}

// the kept reads among the calls q = first, first + step, ... of a pixel with n reads (n <= 2^32 - 1: at most 2^30 calls)
__device__ __forceinline__ uint32_t thin_calls(uint32_t x, uint32_t y, uint32_t n, uint32_t first, uint32_t step, uint32_t tag,
                                               uint32_t seed, uint32_t sample, uint32_t T) {
    const uint32_t full = n >> 2, rest = n & 3;
    uint32_t k = 0;
    for (uint32_t q = first; q < full; q += step) k += philox_below(x, y, q, tag, seed, sample, T, 4);
    // the call that holds the last n & 3 reads belongs to the lane whose sequence reaches it
    if (rest && full >= first && (full - first) % step == 0) k += philox_below(x, y, full, tag, seed, sample, T, rest);
    return k;
}

// a count as the kernels take it: the integer, or -1 for what is no integer in [0, 2^32 - 1]
__device__ __forceinline__ int64_t count_of(int64_t v) { return v < 0 || v > kThinMaxCount ? -1 : v; }
__device__ __forceinline__ int64_t count_of(double v) {
    return v >= 0.0 && v <= 4294967295.0 && v == floor(v) ? (int64_t)v : -1;          // NaN fails the first compare
}
__device__ __forceinline__ int64_t count_of(float v) { return count_of((double)v); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace mst
