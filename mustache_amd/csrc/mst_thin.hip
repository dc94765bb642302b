// Binomial thinning of raw pixel counts on the device (mustache_amd/downsample.py states the rule; include/mustache_hip.h the
// entry point; tests/downsample_reference.py restates it in NumPy).
//
//   mst_thin_counts    a pixel (x, y = x + dist) with count n keeps k = #{ j in [0, n) : u_j < T }, u_j = word j & 3 of
//                      Philox4x32-10(counter = (x, y, j >> 2, tag), key = (seed, sample)).  Every draw is addressed by (x, y, j):
//                      k depends on nothing but the pixel, so any split of the draws over lanes gives the same k.
//
// The work is one Philox call per four reads, and counts are skewed (thousands on the first diagonals, ones far out), so a
// wave works in two modes.  Light: a lane whose n < MST_THIN_HEAVY loops over its own ceil(n / 4) calls.  Heavy: the lanes whose
// n >= MST_THIN_HEAVY are found with a ballot and taken one at a time by the whole wave -- (x, y, n) broadcast, lane l takes the
// calls l, l + 64, ..., the last call is masked to n & 3 words, the 64 partial counts are added across the wave and the owning
// lane keeps the sum.  The totals (reads in, reads kept) are integer sums: per lane over its trips, per wave, per workgroup in
// LDS, then one 64-bit integer atomic per workgroup and total.  Integer addition is order-free: the totals and every k are the
// same from run to run, under any order of the records and for any launch shape.  The draws themselves (Philox, the calls of a
// pixel, a count as the kernel takes it, the wave sum) are mst_thin_draws.h's, shared with mst_thin_pairs.hip.
#include "mst_common.h"
#include "mst_thin_draws.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kHeavy = mst::kThinHeavy;
using mst::count_of;                               // the draws: mst_thin_draws.h
using mst::thin_calls;
using mst::wave_sum;

template <typename C>
__global__ __launch_bounds__(kThreads) void
thin_kernel(const int32_t *__restrict__ xs, const int32_t *__restrict__ dists, const C *__restrict__ count_in, int64_t N, uint32_t tag,
            uint32_t seed, uint32_t sample, uint32_t T, int64_t *__restrict__ count_out, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long part[2][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    unsigned long long sum_in = 0, sum_kept = 0;
    bool bad = false;
    // the trip count is the same for every lane of a workgroup (the ballot and the shuffles need that of a wave); `e < N`
    // guards the loads and the store only
    for (int64_t base = (int64_t)blockIdx.x * kThreads; base < N; base += stride) {
        const int64_t e = base + threadIdx.x;
        const bool active = e < N;
        uint32_t x = 0, y = 0, n = 0;
        if (active) {
            const int64_t c = count_of(count_in[e]);
            x = (uint32_t)xs[e];
            y = x + (uint32_t)dists[e];
            bad |= c < 0;
            n = c < 0 ? 0u : (uint32_t)c;
        }
        sum_in += n;
        if (!count_out) continue;                   // wave-uniform: a call that only sums and checks
        const bool heavy = (int64_t)n >= kHeavy;
        uint32_t k = heavy ? 0u : thin_calls(x, y, n, 0, 1, tag, seed, sample, T);
        for (unsigned long long todo = __ballot(heavy); todo; todo &= todo - 1) {
            const int owner = __ffsll((long long)todo) - 1;
            const uint32_t ox = __shfl(x, owner, 64), oy = __shfl(y, owner, 64), on = __shfl(n, owner, 64);
            const uint32_t mine = (uint32_t)wave_sum(thin_calls(ox, oy, on, (uint32_t)lane, 64, tag, seed, sample, T));
            if (lane == owner) k = mine;
        }
        if (active) count_out[e] = (int64_t)k;
        sum_kept += k;
    }
    if (bad) words[2] = 1;                          // a flag, not a count: every writer writes the same value
    sum_in = wave_sum(sum_in);
    sum_kept = wave_sum(sum_kept);
    if (lane == 0) {
        part[0][wave] = sum_in;
        part[1][wave] = sum_kept;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += part[threadIdx.x][w];
        if (s) atomicAdd(&words[threadIdx.x], s);
    }
}

}  // namespace

extern "C" int mst_thin_counts(const int32_t *x, const int32_t *dist, const void *count_in, int32_t count_kind, int64_t n_records,
                               uint32_t tag, uint32_t seed, uint32_t sample, uint64_t T, int64_t *count_out, int64_t *words,
                               void *stream) {
    if (n_records < 0 || !words || count_kind < 0 || count_kind > 2 || (n_records > 0 && (!x || !dist || !count_in)) ||
        (count_out && (T < 1 || T > 0xFFFFFFFFull)))
        return mst::fail(MST_E_ARG, "mst_thin_counts: bad argument");
    if (n_records == 0) return MST_OK;
    // one lane per record and trip; at most 16384 workgroups, so that a few long trips of heavy pixels spread over the chip
    const int64_t blocks = (n_records + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
    auto *w = reinterpret_cast<unsigned long long *>(words);
    const uint32_t t32 = (uint32_t)T;
    hipStream_t s = mst::as_stream(stream);
    if (count_kind == MST_THIN_COUNT_I64)
        thin_kernel<int64_t><<<grid, kThreads, 0, s>>>(x, dist, static_cast<const int64_t *>(count_in), n_records, tag, seed, sample,
                                                      t32, count_out, w);
    else if (count_kind == MST_THIN_COUNT_F32)
        thin_kernel<float><<<grid, kThreads, 0, s>>>(x, dist, static_cast<const float *>(count_in), n_records, tag, seed, sample, t32,
                                                    count_out, w);
    else
        thin_kernel<double><<<grid, kThreads, 0, s>>>(x, dist, static_cast<const double *>(count_in), n_records, tag, seed, sample,
                                                     t32, count_out, w);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
