// Inter-chromosomal (trans) maps on the device (gfx950): the stages of a chromosome pair's loop call that the cis path does
// not have.  The rules are stated in mustache_amd/trans.py and restated in NumPy in tests/trans_reference.py.
//
//   mst_trans_decode_hic_rows  `.hic` rows of a trans matrix (mst_hic_rawstream_open_trans) -> COO x, y, v: counts divided by
//                              norm_x[x] * norm_y[y] (straw's float32 value), NaN / non-positive dropped, the stored (B, A)
//                              order transposed.  The per-record half of the read, in the style of mst_band_scatter_hic_rows.
//   mst_trans_zscore           v' = (v - mean) / std over the records (population std), NaN / inf -> 0, in place.
//   mst_trans_scatter_tiles    records -> B square tiles of CH x CH with per-tile (row, col) origins, zero elsewhere.
//   mst_trans_prologue         nz = c != 0 over the whole tile (no triangle masks, no fills) and its count per tile.
//
// The z-score's two sums (sum v, sum (v - mean)^2) are EXACT (mst_exact_sum.h: fixed-point integer pieces, one rounding per
// sum), so mean, std and every v' are bit-identical under any permutation of the records and any launch geometry.
#include <cmath>
#include "mst_common.h"
#include "mst_exact_sum.h"
#include "../../include/mustache_hicrow.h"

namespace {

constexpr int kThreads = 256;
using mst_exact::add_exact;
using mst_exact::exact_to_double;
using mst_exact::kLimbs;
using mst_exact::kSumWords;

__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return *reinterpret_cast<const uint16_t *>(p); }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | (ld16(p + 2) << 16); }   // 2-byte aligned

// ---- .hic rows -> COO ---------------------------------------------------------------------------------------------------
constexpr int kRowsPerBlock = 8;

__global__ void __launch_bounds__(kThreads)
trans_rows_kernel(const uint8_t *__restrict__ payload, const mst_hic_row *__restrict__ rows, int n_rows,
                  const double *__restrict__ norm_x, long long n_norm_x, const double *__restrict__ norm_y, long long n_norm_y,
                  int transposed, int32_t *__restrict__ out_x, int32_t *__restrict__ out_y, double *__restrict__ out_v,
                  long long cap, unsigned long long *__restrict__ stats) {
    __shared__ mst_hic_row srow[kRowsPerBlock];
    __shared__ int sbeg[kRowsPerBlock + 1];
    const int tid = threadIdx.x;
    for (int r0 = blockIdx.x * kRowsPerBlock; r0 < n_rows; r0 += gridDim.x * kRowsPerBlock) {
        const int nr = n_rows - r0 < kRowsPerBlock ? n_rows - r0 : kRowsPerBlock;
        __syncthreads();
        if (tid < nr) srow[tid] = rows[r0 + tid];
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int i = 0; i < nr; ++i) {
                sbeg[i] = run;
                run += (int)(srow[i].count & MST_HIC_ROW_COUNT_MASK);
            }
            for (int i = nr; i <= kRowsPerBlock; ++i) sbeg[i] = run;
        }
        __syncthreads();
        const int total = sbeg[kRowsPerBlock];
        for (int i = tid; i < total; i += kThreads) {
            int q = 0;
#pragma unroll
            for (int t = 1; t < kRowsPerBlock; ++t) q += (i >= sbeg[t]) ? 1 : 0;
            const mst_hic_row e = srow[q];
            const int j = i - sbeg[q];
            const bool short_c = e.count & MST_HIC_ROW_SHORT_COUNTS, int_x = e.count & MST_HIC_ROW_INT_COLUMNS,
                       dense = e.count & MST_HIC_ROW_DENSE;
            const int rec = (dense ? 0 : (int_x ? 4 : 2)) + (short_c ? 2 : 4);
            const uint8_t *q8 = payload + e.off + (size_t)j * rec;
            int x = j;
            if (!dense) {
                x = int_x ? (int)ld32(q8) : (int)(int16_t)ld16(q8);
                q8 += int_x ? 4 : 2;
            }
            float val;
            if (short_c) {
                const int16_t sv = (int16_t)ld16(q8);
                if (dense && sv == -32768) continue;
                val = (float)sv;
            } else {
                val = __uint_as_float(ld32(q8));
                if (dense && val != val) continue;
            }
            // the file's binX belongs to its first chromosome, binY to its second; (a, b) = (row of A, column of B)
            const long long bx = (long long)e.x_off + x, by = e.y;
            const long long a = transposed ? by : bx, b = transposed ? bx : by;
            if (a < 0 || b < 0 || a > 0x7FFFFFFFLL || b > 0x7FFFFFFFLL) continue;
            float c = val;
            if (norm_x) {
                if (a >= n_norm_x || b >= n_norm_y) continue;
                c = (float)((double)val / (norm_x[a] * norm_y[b]));
            }
            if (c != c || !(c > 0.0f) || isinf(c)) continue;
            const unsigned long long k = atomicAdd(&stats[0], 1ull);
            if ((long long)k < cap) {
                out_x[k] = (int32_t)a;
                out_y[k] = (int32_t)b;
                out_v[k] = (double)c;
            }
        }
    }
}

// ---- exact sums (mst_exact_sum.h: add_exact, exact_to_double) --------------------------------------------------------------
// PASS 0: words += v;  PASS 1: words += (v - mean)^2 with mean = stats[0]
template <int PASS>
__global__ void __launch_bounds__(kThreads)
zsum_kernel(const double *__restrict__ v, long long n, const double *__restrict__ stats, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long acc[kLimbs];
    __shared__ unsigned long long bad;
    for (int i = threadIdx.x; i < kLimbs; i += kThreads) acc[i] = 0;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const double mean = PASS ? stats[0] : 0.0;
    unsigned long long nbad = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        double t = v[i];
        if (PASS) {
            const double d = t - mean;
            t = d * d;
        }
        if (!add_exact(t, acc)) ++nbad;
    }
    if (nbad) atomicAdd(&bad, nbad);
    __syncthreads();
    for (int i = threadIdx.x; i < kLimbs; i += kThreads)
        if (acc[i]) atomicAdd(&words[i], acc[i]);
    if (threadIdx.x == 0 && bad) atomicAdd(&words[kLimbs + 1], bad);
}

// stats = {mean, std, n, flags}: PASS 0 sets mean, PASS 1 std (population: sqrt(sum / n))
template <int PASS>
__global__ void zfinish_kernel(const unsigned long long *__restrict__ words, long long n, double *__restrict__ stats) {
    __shared__ long long digits[kLimbs + 1];
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double s = exact_to_double(words, digits);
    const bool bad = words[kLimbs + 1] != 0;
    if (PASS == 0) {
        stats[0] = bad ? NAN : s / (double)n;
        stats[2] = (double)n;
    } else {
        stats[1] = bad ? NAN : sqrt(s / (double)n);
    }
}

__global__ void __launch_bounds__(kThreads)
zapply_kernel(const double *__restrict__ v, long long n, const double *__restrict__ stats, double *__restrict__ out) {
    const double mean = stats[0], sd = stats[1];
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double z = (v[i] - mean) / sd;
        out[i] = isfinite(z) ? z : 0.0;
    }
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------
// One thread per record; the B tile origins are in LDS, every tile whose window holds (x, y) receives the value.
constexpr int kMaxTilesLds = 4096;

__global__ void __launch_bounds__(kThreads)
tiles_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, const double *__restrict__ v, long long n,
             const int64_t *__restrict__ row0, const int64_t *__restrict__ col0, int B, int CH, double *__restrict__ c) {
    __shared__ int64_t sr[kMaxTilesLds], sc[kMaxTilesLds];
    for (int b = threadIdx.x; b < B; b += kThreads) {
        sr[b] = row0[b];
        sc[b] = col0[b];
    }
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const int64_t xi = x[i], yi = y[i];
        const double vi = v[i];
        for (int b = 0; b < B; ++b) {
            const int64_t r = xi - sr[b], q = yi - sc[b];
            if (r >= 0 && r < CH && q >= 0 && q < CH) c[((int64_t)b * CH + r) * CH + q] = vi;
        }
    }
}

__global__ void __launch_bounds__(kThreads)
trans_prologue_kernel(const double *__restrict__ c, uint8_t *__restrict__ nz, uint32_t *__restrict__ nz_count, int CH) {
    const int b = blockIdx.y;
    const int64_t np = (int64_t)CH * CH;
    const double *cb = c + (int64_t)b * np;
    uint8_t *nb = nz + (int64_t)b * np;
    uint32_t local = 0;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < np; p += (int64_t)gridDim.x * kThreads) {
        const bool t = cb[p] != 0.0;
        nb[p] = t ? 1 : 0;
        local += t ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(nz_count + b, local);
}

int grid_for(long long n, int cap) {
    const long long want = (n + kThreads - 1) / kThreads;
    return (int)(want < cap ? (want > 0 ? want : 1) : cap);
}

}  // namespace

extern "C" int mst_trans_decode_hic_rows(const void *payload, const void *rows, int32_t n_rows, const double *norm_x,
                                         int64_t n_norm_x, const double *norm_y, int64_t n_norm_y, int32_t transposed,
                                         int32_t *x, int32_t *y, double *v, int64_t capacity, uint64_t *count, void *stream) {
    MST_RANGE("read: mst_trans_decode_hic_rows");
    if (!x || !y || !v || !count || capacity < 0 || n_rows < 0 || (n_rows > 0 && (!payload || !rows)) ||
        (!norm_x != !norm_y) || (norm_x && (n_norm_x < 0 || n_norm_y < 0)) ||
        (reinterpret_cast<uintptr_t>(payload) & 1) || (reinterpret_cast<uintptr_t>(rows) & 3))
        return mst::fail(MST_E_ARG, "mst_trans_decode_hic_rows: bad argument (both norm vectors or none; payload 2-byte, rows "
                                    "4-byte aligned)");
    if (n_rows == 0) return MST_OK;
    hipStream_t s = mst::as_stream(stream);
    const int64_t want = ((int64_t)n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
    const int g = (int)(want < 4096 ? want : 4096);
    trans_rows_kernel<<<g, kThreads, 0, s>>>(static_cast<const uint8_t *>(payload), static_cast<const mst_hic_row *>(rows), n_rows,
                                             norm_x, n_norm_x, norm_y, n_norm_y, transposed ? 1 : 0, x, y, v, capacity,
                                             reinterpret_cast<unsigned long long *>(count));
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" uint64_t mst_trans_zscore_workspace_bytes(void) { return 8ull * 2 * kSumWords; }

extern "C" int mst_trans_zscore(const double *v, int64_t n, double *out, double *stats, void *workspace, uint64_t workspace_bytes,
                                void *stream) {
    MST_RANGE("trans: mst_trans_zscore");
    if (!stats || !workspace || n < 0 || (n > 0 && (!v || !out)) || n >= ((int64_t)1 << 31) ||
        workspace_bytes < mst_trans_zscore_workspace_bytes())
        return mst::fail(MST_E_ARG, "mst_trans_zscore: bad argument (n < 2^31 records, workspace of "
                                    "mst_trans_zscore_workspace_bytes())");
    hipStream_t s = mst::as_stream(stream);
    auto *w = static_cast<unsigned long long *>(workspace);
    MST_HIP(hipMemsetAsync(w, 0, mst_trans_zscore_workspace_bytes(), s));
    MST_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(double), s));
    if (n == 0) return MST_OK;
    const int g = grid_for(n, 2048);
    zsum_kernel<0><<<g, kThreads, 0, s>>>(v, n, stats, w);
    zfinish_kernel<0><<<1, 64, 0, s>>>(w, n, stats);
    zsum_kernel<1><<<g, kThreads, 0, s>>>(v, n, stats, w + kSumWords);
    zfinish_kernel<1><<<1, 64, 0, s>>>(w + kSumWords, n, stats);
    zapply_kernel<<<g, kThreads, 0, s>>>(v, n, stats, out);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_trans_scatter_tiles(const int32_t *x, const int32_t *y, const double *v, int64_t n, const int64_t *row0,
                                       const int64_t *col0, int32_t B, int32_t CH, double *c, void *stream) {
    MST_RANGE("trans: mst_trans_scatter_tiles");
    if (!c || !row0 || !col0 || B <= 0 || B > kMaxTilesLds || CH <= 0 || n < 0 || (n > 0 && (!x || !y || !v)))
        return mst::fail(MST_E_ARG, "mst_trans_scatter_tiles: bad argument (1 <= B <= 4096)");
    hipStream_t s = mst::as_stream(stream);
    MST_HIP(hipMemsetAsync(c, 0, sizeof(double) * (size_t)B * CH * CH, s));
    if (n == 0) return MST_OK;
    tiles_kernel<<<grid_for(n, 8192), kThreads, 0, s>>>(x, y, v, n, row0, col0, B, CH, c);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_trans_prologue(const double *c, uint8_t *nz, uint32_t *nz_count, int32_t B, int32_t CH, void *stream) {
    if (!c || !nz || !nz_count || B <= 0 || CH <= 0 || B > 65535)
        return mst::fail(MST_E_ARG, "mst_trans_prologue: bad argument");
    hipStream_t s = mst::as_stream(stream);
    MST_HIP(hipMemsetAsync(nz_count, 0, sizeof(uint32_t) * B, s));
    trans_prologue_kernel<<<dim3(grid_for((long long)CH * CH, 4096), B), kThreads, 0, s>>>(c, nz, nz_count, CH);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
