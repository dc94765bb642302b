// Significance of every loop of a pile-up from raw counts (mustache_amd/pileup.py states the rules, "Significance";
// tests/pileup_poisson_reference.py restates them cell by cell).
//
//   mst_pileup_centre_counts   counts[k] = the sum of the raw counts of the records whose pixel is keys[k]
//   mst_pileup_poisson         EXP, FE, LAMBDA and P of every (loop, neighbourhood) from the sums mst_pileup_enrich wrote
//
// mst_pileup_centre_counts is the one pass over the chromosome's raw records: 8 bytes of (x, dist) per record, the count of a
// record only when its distance lies inside the list's range [min_sep, max_sep].  A workgroup stages a sample of the sorted keys
// in LDS -- every key when K <= kLdsKeys, every stride-th key otherwise -- and walks the records in a grid-stride loop, kUnroll
// coalesced loads per lane in flight.  A record inside the range finds the last sample <= its key in LDS and, when the sample is
// thinner than the list, finishes among the stride - 1 keys behind it in global memory (the list is a few hundred KiB: L2).  A hit
// is one 64-bit integer atomic add: integer sums are exact and order-free, so counts has the same bits under any record order.
// Tried and dropped: a one-hash filter of the keys in LDS in front of a search in L2 (7.87 ms against 3.16 ms at 3.1e8 records
// and 20 000 keys: 7 % of the records pass it, so some lane of nearly every wave still pays the whole search, now in L2).
//
// mst_pileup_poisson is one lane per (loop, neighbourhood): a dozen loads, the ratios in pileup.enrichment()'s operation order,
// and the regularised lower incomplete gamma function P(c, lambda) by the classical split -- the power series for x <= 1 or
// x <= a, 1 - Q by the continued fraction otherwise -- in float64, both stopped at a relative term of 2^-53.  Lanes of a wave
// run different trip counts; the launch is L x 4 lanes and nothing is built around that.
#include <cmath>
#include "mst_common.h"
#include "mst_pileup_sums.h"

namespace {

using mst_pileup::grid_ok;
using mst_pileup::kThreads;

constexpr int kLdsKeys = 4096;          // 32 KiB of samples: five workgroups of a CU's 160 KiB stay resident
constexpr int kUnroll = 4;              // records per lane and trip
constexpr int kMaxBlocks = 256 * 5;     // CUs x resident workgroups: every workgroup stages the samples once
// Trips either iteration may take.  c = lambda = 2^24 (the largest integer a float32 count holds exactly) needs 30 767 terms of
// the series, and the continued fraction one ulp above it 2 350 (tests/test_pileup_poisson_reference.py runs both on the CPU);
// a tail that has not converged under the cap is NaN and is counted.
constexpr int kTailMaxIter = 131072;
constexpr double kTailEps = 1.1102230246251565e-16;          // 2^-53
constexpr double kBig = 4503599627370496.0, kBigInv = 2.22044604925031308085e-16;          // 2^52, 2^-52

// the slot of `key` among keys[0 .. K), -1 when it is none of them.  smp[j] = keys[j * stride], j < S.
__device__ __forceinline__ int64_t find_key(const int64_t *smp, int32_t S, const int64_t *__restrict__ keys, int64_t K,
                                            int64_t stride, int64_t key) {
    int32_t lo = 0, hi = S;                                  // the first sample > key
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (smp[mid] <= key) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return -1;
    const int32_t j = lo - 1;
    if (smp[j] == key) return (int64_t)j * stride;
    if (stride == 1) return -1;
    int64_t a = (int64_t)j * stride + 1, b = (int64_t)(j + 1) * stride;        // the keys between this sample and the next
    if (b > K) b = K;
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        const int64_t k = keys[mid];
        if (k == key) return mid;
        if (k < key) a = mid + 1; else b = mid;
    }
    return -1;
}

// kFloat: count is float32 (a `.hic` file's), and a value that is no integer in [0, 2^63) raises the flag word; otherwise int64.
template <bool kFloat>
__global__ void __launch_bounds__(kThreads)
centre_counts_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ dist, const void *__restrict__ count, int64_t R,
                     const int64_t *__restrict__ keys, int64_t K, int64_t stride, int32_t S, int32_t min_sep, int32_t max_sep,
                     unsigned long long *__restrict__ counts, unsigned long long *__restrict__ flag) {
    extern __shared__ int64_t smp[];
    for (int32_t j = threadIdx.x; j < S; j += kThreads) smp[j] = keys[(int64_t)j * stride];
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * kThreads * kUnroll;
    for (int64_t base = (int64_t)blockIdx.x * kThreads * kUnroll; base < R; base += step) {
        int32_t xv[kUnroll], dv[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t i = base + u * kThreads + threadIdx.x;
            const bool in = i < R;
            xv[u] = in ? x[i] : 0;
            dv[u] = in ? dist[i] : -1;                       // min_sep >= 0: -1 is outside every range
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (dv[u] < min_sep || dv[u] > max_sep) continue;
            const int64_t i = base + u * kThreads + threadIdx.x;
            long long c = 0;
            if (kFloat) {
                const float v = static_cast<const float *>(count)[i];
                if (!(v >= 0.0f && v < 9.0e18f && v == rintf(v))) {          // a NaN fails the first comparison
                    atomicOr(flag, 1ull);
                    continue;
                }
                c = (long long)v;
            }
            const int64_t slot = find_key(smp, S, keys, K, stride, (int64_t)xv[u] << 32 | (int64_t)(uint32_t)dv[u]);
            if (slot < 0) continue;
            if (!kFloat) c = static_cast<const long long *>(count)[i];
            atomicAdd(counts + slot, (unsigned long long)c);
        }
    }
}

// P(a, x), a >= 1 an integer value, 0 < x < inf.  ok = false when an iteration ran into kTailMaxIter.
__device__ double lower_gamma(double a, double x, bool &ok) {
    const double pre = exp(a * log(x) - x - lgamma(a));
    ok = true;
    if (x <= 1.0 || x <= a) {                                // the power series
        double r = a, c = 1.0, ans = 1.0;
        int it = 0;
        do {
            r = r + 1.0;
            c = c * (x / r);
            ans = ans + c;
            if (++it >= kTailMaxIter) {
                ok = false;
                break;
            }
        } while (c / ans > kTailEps);
        return ans * pre / a;
    }
    double y = 1.0 - a, z = x + y + 1.0, c = 0.0;           // 1 - Q, Q by the continued fraction
    double pkm2 = 1.0, qkm2 = x, pkm1 = x + 1.0, qkm1 = z * x, ans = pkm1 / qkm1, t;
    int it = 0;
    do {
        c = c + 1.0;
        y = y + 1.0;
        z = z + 2.0;
        const double yc = y * c, pk = pkm1 * z - pkm2 * yc, qk = qkm1 * z - qkm2 * yc;
        if (qk != 0.0) {
            const double r = pk / qk;
            t = fabs((ans - r) / r);
            ans = r;
        } else {
            t = 1.0;
        }
        pkm2 = pkm1;
        pkm1 = pk;
        qkm2 = qkm1;
        qkm1 = qk;
        if (fabs(pk) > kBig) {
            pkm2 = pkm2 * kBigInv;
            pkm1 = pkm1 * kBigInv;
            qkm2 = qkm2 * kBigInv;
            qkm1 = qkm1 * kBigInv;
        }
        if (++it >= kTailMaxIter) {
            ok = false;
            break;
        }
    } while (t > kTailEps);
    return 1.0 - ans * pre;
}

__global__ void __launch_bounds__(kThreads)
poisson_kernel(const double *__restrict__ sums, const double *__restrict__ centre_obs, const double *__restrict__ centre_e,
               const int64_t *__restrict__ counts, const double *__restrict__ bias, int64_t n, const int64_t *__restrict__ xs,
               const int64_t *__restrict__ ys, int64_t L, double *__restrict__ exp_out, double *__restrict__ fe_out,
               double *__restrict__ lambda_out, double *__restrict__ p_out, unsigned long long *__restrict__ unconverged) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;          // = l * 4 + neighbourhood
    if (i >= L * 4) return;
    const int64_t l = i >> 2;
    const double nan = __builtin_nan("");
    const double so = sums[i * 3 + 0], se = sums[i * 3 + 1], cnt = sums[i * 3 + 2];
    const double c = centre_obs[l], e = centre_e[l];
    double ex = e * so / se;                                 // enrichment()'s order: (e * so) / se
    if (cnt == 0.0 || se == 0.0 || c != c) ex = nan;
    double fe = c / ex;
    if (ex != ex || ex == 0.0) fe = nan;
    const int64_t x = xs[l], y = ys[l];
    const double b1 = x >= 0 && x < n ? bias[x] : nan, b2 = y >= 0 && y < n ? bias[y] : nan;
    double lam = (ex * b1) * b2;
    if (!(b1 >= 0.2) || !(b2 >= 0.2) || ex != ex) lam = nan;          // a NaN bias fails the comparison
    const int64_t k = counts[l];
    double p;
    if (!(lam >= 0.0)) {
        p = nan;                                             // NaN, or a negative lambda no count data gives
    } else if (k <= 0) {
        p = 1.0;
    } else if (lam == 0.0) {
        p = 0.0;
    } else if (lam == INFINITY) {
        p = 1.0;
    } else {
        bool ok;
        p = lower_gamma((double)k, lam, ok);
        if (!ok) {
            p = nan;
            atomicAdd(unconverged, 1ull);
        }
    }
    exp_out[i] = ex;
    fe_out[i] = fe;
    lambda_out[i] = lam;
    p_out[i] = p;
}

}  // namespace

extern "C" int mst_pileup_centre_counts(const int32_t *x, const int32_t *dist, const void *count, int32_t count_kind, int64_t R,
                                        const int64_t *keys, int64_t K, int32_t min_sep, int32_t max_sep, int64_t *counts,
                                        int64_t *flag, void *stream) {
    MST_RANGE("pileup: mst_pileup_centre_counts");
    if (R < 0 || K < 0) return mst::fail(MST_E_ARG, "mst_pileup_centre_counts: bad argument (R %lld, K %lld)", (long long)R, (long long)K);
    if (K == 0) return MST_OK;
    if (count_kind != 0 && count_kind != 1)
        return mst::fail(MST_E_ARG, "mst_pileup_centre_counts: count_kind %d is neither 0 (float32) nor 1 (int64)", (int)count_kind);
    if (min_sep < 0 || max_sep < min_sep)
        return mst::fail(MST_E_ARG, "mst_pileup_centre_counts: the distance range [%d, %d] is empty or negative", (int)min_sep, (int)max_sep);
    if (!keys || !counts || !flag || (R > 0 && (!x || !dist || !count)))
        return mst::fail(MST_E_ARG, "mst_pileup_centre_counts: bad argument (null x, dist, count, keys, counts or flag)");
    hipStream_t s = mst::as_stream(stream);
    MST_HIP(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int64_t), s));
    if (R == 0) return MST_OK;
    const int64_t stride = (K + kLdsKeys - 1) / kLdsKeys;          // 1 while every key fits
    const int32_t S = (int32_t)((K + stride - 1) / stride);      // <= kLdsKeys, and (S - 1) * stride < K
    const int64_t per_block = (int64_t)kThreads * kUnroll;
    int64_t blocks = (R + per_block - 1) / per_block;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    int rc = grid_ok("mst_pileup_centre_counts", blocks);
    if (rc != MST_OK) return rc;
    const size_t lds = (size_t)S * sizeof(int64_t);
    auto *cnt = reinterpret_cast<unsigned long long *>(counts);
    auto *flg = reinterpret_cast<unsigned long long *>(flag);
    if (count_kind == 0)
        centre_counts_kernel<true><<<(unsigned)blocks, kThreads, lds, s>>>(x, dist, count, R, keys, K, stride, S, min_sep, max_sep, cnt, flg);
    else
        centre_counts_kernel<false><<<(unsigned)blocks, kThreads, lds, s>>>(x, dist, count, R, keys, K, stride, S, min_sep, max_sep, cnt, flg);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_pileup_poisson(const double *sums, const double *centre_obs, const double *centre_e, const int64_t *counts,
                                  const double *bias, int64_t n, const int64_t *xs, const int64_t *ys, int64_t L, double *exp_out,
                                  double *fe_out, double *lambda_out, double *p_out, int64_t *unconverged, void *stream) {
    MST_RANGE("pileup: mst_pileup_poisson");
    if (L < 0 || n < 0) return mst::fail(MST_E_ARG, "mst_pileup_poisson: bad argument (L %lld, n %lld)", (long long)L, (long long)n);
    if (L == 0) return MST_OK;
    if (!sums || !centre_obs || !centre_e || !counts || !bias || !xs || !ys || !exp_out || !fe_out || !lambda_out || !p_out || !unconverged)
        return mst::fail(MST_E_ARG, "mst_pileup_poisson: bad argument (a null pointer with L %lld)", (long long)L);
    const int64_t blocks = (L * 4 + kThreads - 1) / kThreads;
    int rc = grid_ok("mst_pileup_poisson", blocks);
    if (rc != MST_OK) return rc;
    poisson_kernel<<<(unsigned)blocks, kThreads, 0, mst::as_stream(stream)>>>(
        sums, centre_obs, centre_e, counts, bias, n, xs, ys, L, exp_out, fe_out, lambda_out, p_out,
        reinterpret_cast<unsigned long long *>(unconverged));
    MST_LAUNCH_CHECK();
    return MST_OK;
}
