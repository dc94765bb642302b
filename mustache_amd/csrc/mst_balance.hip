// ICE balancing of one chromosome's intra-chromosomal map (mustache_amd/balance.py; the algorithm is stated there and in
// tests/balance_reference.py).
//
//   mst_balance_marginals  m_i = w_i * sum_c A_ic w_c and the row's non-zero count (the filter stage)
//   mst_balance_iterate    `steps` ICE iterations; mean, variance and the convergence test stay on the device
//   mst_balance_bias       kappa = sqrt(sum_{i<=j} A_ij w_i w_j / sum_{i<=j} A_ij) and b = kappa / w (NaN where w = 0)
//   mst_balance_apply_packed  (v / b[x]) / b[x + dist] for `.hic` records already on the device
//
// The matrix is the full symmetric CSR of the kept pixels (int32 column, float64 value), sorted by (row, column).  Each row
// is cut into chunks of kChunk entries counted from the row's first entry; one wave reduces one chunk (lane l takes entries
// l, l + 64, ... in order, then a fixed xor butterfly), and one thread per row adds its chunks' partial sums in chunk order.
// Bin-wide sums (the mean of s, the variance, kappa) add fixed 256-row blocks in a fixed tree, then one workgroup adds the
// block partials in a fixed per-thread order (linear in n).  Every order depends only on absolute row and entry positions: the result is the same from run
// to run, under any permutation of the input records and for any n (an appended empty bin adds exact zeros).  No float
// atomics.
#include <cmath>
#include "mst_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 1024;               // entries per chunk: 16 per lane

__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);
    return a;
}

__device__ __forceinline__ int wave_sum_i(int a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    return a;
}

// block total in a fixed order: butterfly inside each wave, then the waves in index order.  Every thread gets the total.
__device__ __forceinline__ double block_sum(double a, double *lds) {
    a = wave_sum(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = a;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t = t + lds[w];
    return t;
}

__device__ __forceinline__ int block_sum_i(int a, int *lds) {
    a = wave_sum_i(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = a;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += lds[w];
    return t;
}

// partial sums of the block partials p[0, nb): thread t adds p[t], p[t + 256], ... in order, then block_sum
__device__ __forceinline__ double reduce_partials(const double *p, int64_t nb, double *lds) {
    double a = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += kThreads) a = a + p[b];
    return block_sum(a, lds);
}

__device__ __forceinline__ int reduce_partials_i(const int *p, int64_t nb, int *lds) {
    int a = 0;                                       // bin counts: n < 2^31
    for (int64_t b = threadIdx.x; b < nb; b += kThreads) a += p[b];
    return block_sum_i(a, lds);
}

struct Workspace {
    double *part;      // [n_chunks]  chunk partial sums (numerator)
    double *part2;     // [n_chunks]  second partial (kappa's denominator)
    int *pcount;       // [n_chunks]  chunk non-zero counts
    double *s;         // [n]         balanced marginals of the current iteration
    double *blk_a;     // [nblk]
    double *blk_b;     // [nblk]
    double *blk_e;     // [nblk]
    int *blk_c;        // [nblk]
    double *kappa;     // [1]
};

__host__ __device__ inline int64_t nblocks(int64_t n) { return (n + kThreads - 1) / kThreads; }
inline uint64_t align256(uint64_t b) { return (b + 255) & ~uint64_t(255); }

inline uint64_t ws_need(int64_t n, int64_t n_chunks) {
    const int64_t nb = nblocks(n);
    return align256(n_chunks * 8) * 2 + align256(n_chunks * 4) + align256(n * 8) + align256(nb * 8) * 3 + align256(nb * 4) + 256;
}

inline Workspace carve(void *ws, int64_t n, int64_t n_chunks) {
    char *p = static_cast<char *>(ws);
    const int64_t nb = nblocks(n);
    Workspace w;
    w.part = reinterpret_cast<double *>(p);   p += align256(n_chunks * 8);
    w.part2 = reinterpret_cast<double *>(p);  p += align256(n_chunks * 8);
    w.pcount = reinterpret_cast<int *>(p);    p += align256(n_chunks * 4);
    w.s = reinterpret_cast<double *>(p);      p += align256(n * 8);
    w.blk_a = reinterpret_cast<double *>(p);  p += align256(nb * 8);
    w.blk_b = reinterpret_cast<double *>(p);  p += align256(nb * 8);
    w.blk_e = reinterpret_cast<double *>(p);  p += align256(nb * 8);
    w.blk_c = reinterpret_cast<int *>(p);     p += align256(nb * 4);
    w.kappa = reinterpret_cast<double *>(p);
    return w;
}

enum { kMarginal = 0, kUpper = 1 };

// One wave per chunk.  kMarginal: part = sum A_e w[col_e], pcount = #{e: w[col_e] != 0}.
// kUpper: entries with col >= row only, part = sum (A_e w[row]) w[col_e], part2 = sum A_e.
template <int MODE>
__global__ void __launch_bounds__(kThreads)
chunk_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
             const int32_t *__restrict__ chunk_row, const int64_t *__restrict__ chunk_ptr, int64_t n_chunks,
             const double *__restrict__ w, const mst_balance_state *__restrict__ state, Workspace ws) {
    if (state && state->done) return;
    const int lane = threadIdx.x & 63;
    const int64_t wstride = (int64_t)gridDim.x * kWaves;
    for (int64_t c = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); c < n_chunks; c += wstride) {
        const int r = chunk_row[c];
        const int64_t beg = row_ptr[r] + (c - chunk_ptr[r]) * kChunk;
        const int64_t end = min(beg + kChunk, row_ptr[r + 1]);
        double a = 0.0, b = 0.0;
        int cnt = 0;
        if (MODE == kMarginal) {
            for (int64_t e = beg + lane; e < end; e += 64) {
                const double wc = w[col[e]];
                a = a + val[e] * wc;
                cnt += wc != 0.0 ? 1 : 0;
            }
        } else {
            const double wr = w[r];
            for (int64_t e = beg + lane; e < end; e += 64) {
                const int cc = col[e];
                if (cc >= r) {
                    const double v = val[e];
                    a = a + (v * wr) * w[cc];
                    b = b + v;
                }
            }
        }
        a = wave_sum(a);
        if (MODE == kMarginal) cnt = wave_sum_i(cnt);
        else b = wave_sum(b);
        if (lane == 0) {
            ws.part[c] = a;
            if (MODE == kMarginal) ws.pcount[c] = cnt;
            else ws.part2[c] = b;
        }
    }
}

// One thread per row, one 256-row block per workgroup (grid = nblocks(n), no stride: the block of a row is fixed).
// KIND 0: m = w_r * sum, nnz = sum of counts.  KIND 1: s = w_r * sum; block partials of sum(s) and #(s != 0) over s != 0.
// KIND 2: block partials of the two kUpper sums.
template <int KIND>
__global__ void __launch_bounds__(kThreads)
row_kernel(const int64_t *__restrict__ chunk_ptr, int64_t n, const double *__restrict__ w, double *__restrict__ m_out,
           int32_t *__restrict__ nnz_out, const mst_balance_state *__restrict__ state, Workspace ws) {
    if (state && state->done) return;
    __shared__ double lds[kWaves];
    __shared__ int ldsi[kWaves];
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double a = 0.0, b = 0.0;
    int cnt = 0;
    if (r < n) {
        const int64_t c0 = chunk_ptr[r], c1 = chunk_ptr[r + 1];
        for (int64_t c = c0; c < c1; ++c) {
            a = a + ws.part[c];
            if (KIND == 2) b = b + ws.part2[c];
            if (KIND == 0) cnt += ws.pcount[c];
        }
    }
    if (KIND == 0) {
        if (r < n) {
            m_out[r] = w[r] * a;
            if (nnz_out) nnz_out[r] = cnt;
        }
        return;
    }
    if (KIND == 1) {
        const double s = r < n ? w[r] * a : 0.0;
        if (r < n) ws.s[r] = s;
        const bool nz = s != 0.0;
        const double t = block_sum(nz ? s : 0.0, lds);
        const int tc = block_sum_i(nz ? 1 : 0, ldsi);
        if (threadIdx.x == 0) {
            ws.blk_a[blockIdx.x] = t;
            ws.blk_c[blockIdx.x] = tc;
        }
        return;
    }
    const double ta = block_sum(a, lds);
    const double tb = block_sum(b, lds);
    if (threadIdx.x == 0) {
        ws.blk_a[blockIdx.x] = ta;
        ws.blk_b[blockIdx.x] = tb;
    }
}

// one workgroup: mu = mean of s over s != 0 from the block partials blk_a / blk_c, kept in state->mean (1 when no s is
// non-zero: then r = 1 everywhere, w stays as it is and the variance is 0)
__global__ void __launch_bounds__(kThreads)
mean_kernel(int64_t n, mst_balance_state *__restrict__ state, Workspace ws) {
    if (state->done) return;
    __shared__ double lds[kWaves];
    __shared__ int ldsi[kWaves];
    const int64_t nb = nblocks(n);
    const double tot = reduce_partials(ws.blk_a, nb, lds);
    const int cnt = reduce_partials_i(ws.blk_c, nb, ldsi);
    if (threadIdx.x == 0) state->mean = cnt > 0 ? tot / (double)cnt : 1.0;
}

// r = s / mu where s != 0 and 1 elsewhere, w /= r; block partials of sum(r - 1) and sum((r - 1)^2) over s != 0
__global__ void __launch_bounds__(kThreads)
update_kernel(int64_t n, double *__restrict__ w, const mst_balance_state *__restrict__ state, Workspace ws) {
    if (state->done) return;
    __shared__ double lds[kWaves];
    const double mu = state->mean;
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double d = 0.0;
    bool nz = false;
    if (r < n) {
        const double s = ws.s[r];
        nz = s != 0.0;
        const double q = nz ? s / mu : 1.0;
        w[r] = w[r] / q;
        d = q - 1.0;
    }
    const double t1 = block_sum(nz ? d : 0.0, lds);
    const double t2 = block_sum(nz ? d * d : 0.0, lds);
    if (threadIdx.x == 0) {
        ws.blk_b[blockIdx.x] = t1;
        ws.blk_e[blockIdx.x] = t2;
    }
}

// one workgroup: variance of r over s != 0 (population), the iteration count, convergence and the stop flag
__global__ void __launch_bounds__(kThreads)
finish_kernel(int64_t n, int32_t max_iter, double tol, mst_balance_state *__restrict__ state, Workspace ws) {
    if (state->done) return;
    __shared__ double lds[kWaves];
    __shared__ int ldsi[kWaves];
    const int64_t nb = nblocks(n);
    const int cnt = reduce_partials_i(ws.blk_c, nb, ldsi);
    const double s1 = reduce_partials(ws.blk_b, nb, lds);
    const double s2 = reduce_partials(ws.blk_e, nb, lds);
    if (threadIdx.x == 0) {
        double var = 0.0;
        if (cnt > 0) {
            const double m1 = s1 / (double)cnt;
            var = s2 / (double)cnt - m1 * m1;
        }
        const int it = state->iterations + 1;
        state->iterations = it;
        state->variance = var;
        state->converged = var < tol ? 1 : 0;
        state->done = (var < tol || it >= max_iter) ? 1 : 0;
    }
}

// one workgroup: kappa from the kUpper block partials
__global__ void __launch_bounds__(kThreads)
kappa_kernel(int64_t n, double *__restrict__ kappa, Workspace ws) {
    __shared__ double lds[kWaves];
    const int64_t nb = nblocks(n);
    const double num = reduce_partials(ws.blk_a, nb, lds);
    const double den = reduce_partials(ws.blk_b, nb, lds);
    if (threadIdx.x == 0) {
        const double k = sqrt(num / den);
        *ws.kappa = k;
        if (kappa) *kappa = k;
    }
}

// b = kappa / w (NaN where w == 0)
__global__ void __launch_bounds__(kThreads)
bias_kernel(int64_t n, const double *__restrict__ w, double *__restrict__ bias, Workspace ws) {
    const double k = *ws.kappa;
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r < n) {
        const double wr = w[r];
        bias[r] = wr != 0.0 ? k / wr : NAN;
    }
}

__device__ __forceinline__ double bias_at(const double *b, int64_t n, int64_t i) {
    if (i < 0 || i >= n) return 1.0;                         // read_bias' default for a bin the vector does not name
    const double v = b[i];
    return (v >= 0.2) ? v : INFINITY;                        // NaN or < 0.2: the contact is dropped (v / inf = 0)
}

__global__ void __launch_bounds__(kThreads)
apply_packed_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ dist, const float *__restrict__ v, int64_t nnz,
                    const double *__restrict__ bias, int64_t nb, double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t a = x[e], b = a + dist[e];
        out[e] = ((double)v[e] / bias_at(bias, nb, a)) / bias_at(bias, nb, b);
    }
}

int grid_for(int64_t items, int64_t per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g < 1048576 ? g : 1048576));
}

int check_csr(const char *who, const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
              const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, void *workspace, uint64_t workspace_bytes) {
    if (!row_ptr || !chunk_ptr || n <= 0 || n > INT32_MAX || n_chunks < 0 || (n_chunks > 0 && (!col || !val || !chunk_row)))
        return mst::fail(MST_E_ARG, "%s: bad CSR argument (n %lld, chunks %lld)", who, (long long)n, (long long)n_chunks);
    if (!workspace || workspace_bytes < ws_need(n, n_chunks))
        return mst::fail(MST_E_ARG, "%s: workspace of %llu bytes, %llu needed", who, (unsigned long long)workspace_bytes,
                         (unsigned long long)ws_need(n, n_chunks));
    return MST_OK;
}

}  // namespace

extern "C" uint64_t mst_balance_workspace_bytes(int64_t n, int64_t n_chunks) {
    if (n <= 0 || n_chunks < 0) return 0;
    return ws_need(n, n_chunks);
}

extern "C" int mst_balance_marginals(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                                     const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, const double *w, double *m,
                                     int32_t *nnz, void *workspace, uint64_t workspace_bytes, void *stream) {
    int rc = check_csr("mst_balance_marginals", row_ptr, col, val, chunk_row, chunk_ptr, n, n_chunks, workspace, workspace_bytes);
    if (rc != MST_OK) return rc;
    if (!w || !m) return mst::fail(MST_E_ARG, "mst_balance_marginals: null w or m");
    hipStream_t s = mst::as_stream(stream);
    Workspace ws = carve(workspace, n, n_chunks);
    if (n_chunks > 0) {
        chunk_kernel<kMarginal><<<grid_for(n_chunks, kWaves), kThreads, 0, s>>>(row_ptr, col, val, chunk_row, chunk_ptr,
                                                                                n_chunks, w, nullptr, ws);
        MST_LAUNCH_CHECK();
    }
    row_kernel<0><<<(int)nblocks(n), kThreads, 0, s>>>(chunk_ptr, n, w, m, nnz, nullptr, ws);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_balance_iterate(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                                   const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, double *w, int32_t steps,
                                   int32_t max_iter, double tol, mst_balance_state *state, void *workspace,
                                   uint64_t workspace_bytes, void *stream) {
    int rc = check_csr("mst_balance_iterate", row_ptr, col, val, chunk_row, chunk_ptr, n, n_chunks, workspace, workspace_bytes);
    if (rc != MST_OK) return rc;
    if (!w || !state || steps < 0 || max_iter < 1) return mst::fail(MST_E_ARG, "mst_balance_iterate: bad argument");
    hipStream_t s = mst::as_stream(stream);
    Workspace ws = carve(workspace, n, n_chunks);
    const int nb = (int)nblocks(n);
    for (int k = 0; k < steps; ++k) {
        if (n_chunks > 0) {
            chunk_kernel<kMarginal><<<grid_for(n_chunks, kWaves), kThreads, 0, s>>>(row_ptr, col, val, chunk_row, chunk_ptr,
                                                                                    n_chunks, w, state, ws);
            MST_LAUNCH_CHECK();
        }
        row_kernel<1><<<nb, kThreads, 0, s>>>(chunk_ptr, n, w, nullptr, nullptr, state, ws);
        MST_LAUNCH_CHECK();
        mean_kernel<<<1, kThreads, 0, s>>>(n, state, ws);
        MST_LAUNCH_CHECK();
        update_kernel<<<nb, kThreads, 0, s>>>(n, w, state, ws);
        MST_LAUNCH_CHECK();
        finish_kernel<<<1, kThreads, 0, s>>>(n, max_iter, tol, state, ws);
        MST_LAUNCH_CHECK();
    }
    return MST_OK;
}

extern "C" int mst_balance_bias(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                                const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, const double *w, double *bias,
                                double *kappa, void *workspace, uint64_t workspace_bytes, void *stream) {
    int rc = check_csr("mst_balance_bias", row_ptr, col, val, chunk_row, chunk_ptr, n, n_chunks, workspace, workspace_bytes);
    if (rc != MST_OK) return rc;
    if (!w || !bias) return mst::fail(MST_E_ARG, "mst_balance_bias: null w or bias");
    hipStream_t s = mst::as_stream(stream);
    Workspace ws = carve(workspace, n, n_chunks);
    const int nb = (int)nblocks(n);
    if (n_chunks > 0) {
        chunk_kernel<kUpper><<<grid_for(n_chunks, kWaves), kThreads, 0, s>>>(row_ptr, col, val, chunk_row, chunk_ptr,
                                                                             n_chunks, w, nullptr, ws);
        MST_LAUNCH_CHECK();
    }
    row_kernel<2><<<nb, kThreads, 0, s>>>(chunk_ptr, n, w, nullptr, nullptr, nullptr, ws);
    MST_LAUNCH_CHECK();
    kappa_kernel<<<1, kThreads, 0, s>>>(n, kappa, ws);
    MST_LAUNCH_CHECK();
    bias_kernel<<<nb, kThreads, 0, s>>>(n, w, bias, ws);
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" int mst_balance_apply_packed(const int32_t *x, const int32_t *dist, const float *v, int64_t nnz, const double *bias,
                                        int64_t n_bias, double *out, void *stream) {
    if (nnz < 0 || n_bias < 0 || (nnz > 0 && (!x || !dist || !v || !out)) || (n_bias > 0 && !bias))
        return mst::fail(MST_E_ARG, "mst_balance_apply_packed: bad argument");
    if (nnz == 0) return MST_OK;
    apply_packed_kernel<<<grid_for(nnz, kThreads), kThreads, 0, mst::as_stream(stream)>>>(x, dist, v, nnz, bias, n_bias, out);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
