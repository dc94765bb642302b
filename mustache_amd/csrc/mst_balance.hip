// ICE balancing of one chromosome's intra-chromosomal map (mustache_amd/balance.py; the algorithm is stated there and in
// tests/balance_reference.py).
//
//   mst_balance_marginals  m_i = w_i * sum_c A_ic w_c and the row's non-zero count (the filter stage)
//   mst_balance_iterate    `steps` ICE iterations; mean, variance and the convergence test stay on the device
//   mst_balance_newton     `steps` steps of the Newton balancing (Knight & Ruiz); every decision stays on the device
//   mst_balance_bias       kappa = sqrt(sum_{i<=j} A_ij w_i w_j / sum_{i<=j} A_ij) and b = kappa / w (NaN where w = 0)
//   mst_balance_apply_packed  (v / b[x]) / b[x + dist] for `.hic` records already on the device
//   mst_balance_apply_pairs   (v / b[row_off[p] + x]) / b[col_off[p] + y] for the records of P chromosome pairs in one launch
//                             (mustache_amd/balance_genome.py: a genome-wide bias applied to inter-chromosomal records)
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

// One wave per chunk (done: the stop flag of the iteration's state record, or null).
// kMarginal: part = sum A_e w[col_e], pcount = #{e: w[col_e] != 0}.
// kUpper: entries with col >= row only, part = sum (A_e w[row]) w[col_e], part2 = sum A_e.
template <int MODE>
__global__ void __launch_bounds__(kThreads)
chunk_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
             const int32_t *__restrict__ chunk_row, const int64_t *__restrict__ chunk_ptr, int64_t n_chunks,
             const double *__restrict__ w, const int32_t *__restrict__ done, Workspace ws) {
    if (done && *done) return;
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

// ---- a genome-wide bias applied to the records of P chromosome pairs (mustache_amd/balance_genome.py) -----------------------
// b of the application rule: the vector's value where it is >= 0.2; +inf where it is NaN or below 0.2, and for a bin outside
// [0, n) -- such a record leaves as 0 (or NaN) and is dropped by the caller's v' > 0.  Nothing outside the vector is read.
__device__ __forceinline__ double genome_bias_at(const double *b, int64_t n, int64_t off, int32_t i) {
    const int64_t g = off + (int64_t)i;
    if (i < 0 || g < 0 || g >= n) return INFINITY;
    const double v = b[g];
    return (v >= 0.2) ? v : INFINITY;
}

// One pass, no atomics.  kVec: a thread takes the records 2 t and 2 t + 1 -- their coordinates as one 8-byte load each, their
// values as one 16-byte load and one 16-byte store (the host takes this path when the pointers are aligned for it); the second
// record looks its pair up again only when it lies past the first one's segment.
template <bool kVec>
__global__ void __launch_bounds__(kThreads)
apply_pairs_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, const double *v, int64_t N,
                   const int64_t *__restrict__ seg_off, const int64_t *__restrict__ row_off, const int64_t *__restrict__ col_off,
                   int32_t P, const double *__restrict__ bias, int64_t n, double *out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (kVec) {
        const int64_t pairs = N >> 1;
        for (int64_t t = t0; t < pairs; t += stride) {
            const int64_t e = 2 * t;
            const int2 xx = *reinterpret_cast<const int2 *>(x + e);
            const int2 yy = *reinterpret_cast<const int2 *>(y + e);
            const double2 vv = *reinterpret_cast<const double2 *>(v + e);
            int32_t p = mst::segment_of(seg_off, 0, P, e);
            double2 o;
            o.x = (vv.x / genome_bias_at(bias, n, row_off[p], xx.x)) / genome_bias_at(bias, n, col_off[p], yy.x);
            if (p + 1 < P && seg_off[p + 1] <= e + 1) p = mst::segment_of(seg_off, 0, P, e + 1);
            o.y = (vv.y / genome_bias_at(bias, n, row_off[p], xx.y)) / genome_bias_at(bias, n, col_off[p], yy.y);
            *reinterpret_cast<double2 *>(out + e) = o;
        }
        if ((N & 1) && t0 == 0) {                                // the odd record at the end
            const int64_t e = N - 1;
            const int32_t p = mst::segment_of(seg_off, 0, P, e);
            out[e] = (v[e] / genome_bias_at(bias, n, row_off[p], x[e])) / genome_bias_at(bias, n, col_off[p], y[e]);
        }
    } else {
        for (int64_t e = t0; e < N; e += stride) {
            const int32_t p = mst::segment_of(seg_off, 0, P, e);
            out[e] = (v[e] / genome_bias_at(bias, n, row_off[p], x[e])) / genome_bias_at(bias, n, col_off[p], y[e]);
        }
    }
}

// ---- Newton balancing (Knight & Ruiz): inexact Newton on x_i (A x)_i = 1, conjugate gradients preconditioned by v ----------
// One *step* is one mat-vec (chunk_kernel<kMarginal>, then the same in-order chunk sum per row as row_kernel) plus its vector
// stages.  state->phase says what the step is: kStart (v, r and the active set from x = 1), kCG (one CG step) or kOuter
// (x *= y, then v, r, rout and the next forcing term).  Every decision is taken on the device by a one-workgroup kernel; the
// row-wide kernels only read the record.  Sums: 256-row blocks, then reduce_partials.  Min/max: any order (exact).
enum { kStart = 0, kCG = 1, kOuter = 2 };
constexpr double kCapLo = 0.1, kCapHi = 3.0, kG = 0.9, kEtaMax = 0.1;

struct NewtonWs {
    double *y, *p, *r, *v, *q, *wv;     // [n] each: step, direction, residual, x*(A x), CG's w, the mat-vec's weight vector
    int *act;                           // [n] 1 on the active set
    double *mn, *mx, *clo, *chi;        // [nblk] block min / max of ynew and of the two candidate cap factors
    int *blk_k;                         // [nblk] block counts of unmasked bins (start step)
};

inline uint64_t newton_need(int64_t n, int64_t n_chunks) {
    const int64_t nb = nblocks(n);
    return ws_need(n, n_chunks) + align256(n * 8) * 6 + align256(n * 4) + align256(nb * 8) * 4 + align256(nb * 4);
}

inline NewtonWs carve_newton(void *ws, int64_t n, int64_t n_chunks) {
    char *p = static_cast<char *>(ws) + ws_need(n, n_chunks);
    const int64_t nb = nblocks(n);
    NewtonWs w;
    double **vec[6] = {&w.y, &w.p, &w.r, &w.v, &w.q, &w.wv};
    for (double **d : vec) { *d = reinterpret_cast<double *>(p); p += align256(n * 8); }
    w.act = reinterpret_cast<int *>(p);  p += align256(n * 4);
    double **blk[4] = {&w.mn, &w.mx, &w.clo, &w.chi};
    for (double **d : blk) { *d = reinterpret_cast<double *>(p); p += align256(nb * 8); }
    w.blk_k = reinterpret_cast<int *>(p);
    return w;
}

__device__ __forceinline__ double wave_min(double a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double b = __shfl_xor(a, o, 64);
        a = b < a ? b : a;
    }
    return a;
}

// block minimum; every thread gets it
__device__ __forceinline__ double block_min(double a, double *lds) {
    a = wave_min(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = a;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t = lds[w] < t ? lds[w] : t;
    return t;
}

__device__ __forceinline__ double reduce_min(const double *p, int64_t nb, double *lds) {
    double a = INFINITY;
    for (int64_t b = threadIdx.x; b < nb; b += kThreads) a = p[b] < a ? p[b] : a;
    return block_min(a, lds);
}

// the weight vector of the step's mat-vec: x * p with the new direction p (CG), or x (after x *= y in an outer update)
__global__ void __launch_bounds__(kThreads)
newton_prep_kernel(int64_t n, double *__restrict__ x, const mst_newton_state *__restrict__ state, NewtonWs nw) {
    if (state->done) return;
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    const int phase = state->phase;
    if (phase == kCG) {
        double wv = 0.0;
        if (nw.act[r]) {
            const double z = nw.r[r] / nw.v[r];
            const double p = state->k == 0 ? z : z + (state->rho / state->rho_prev) * nw.p[r];
            nw.p[r] = p;
            wv = x[r] * p;
        }
        nw.wv[r] = wv;
    } else {
        double xr = x[r];
        if (phase == kOuter && nw.act[r]) {
            xr = xr * nw.y[r];
            x[r] = xr;
        }
        nw.y[r] = 1.0;
        nw.wv[r] = xr;
    }
}

// One thread per row, one 256-row block per workgroup; the row's chunk partials are added in chunk order (as row_kernel does).
// kCG: q = x * (A (x p)) + v p; block partials of p.q (blk_a) and, on the first CG step, of r.z (blk_b).
// kStart / kOuter: v = x * (A x), r = 1 - v on the active set; block partials of r.r (blk_a), sum r (blk_b), |Act| (blk_c).
// kStart also fixes the active set (unmasked, (A 1_K) != 0) and counts the unmasked bins (blk_k).
__global__ void __launch_bounds__(kThreads)
newton_row_kernel(const int64_t *__restrict__ chunk_ptr, int64_t n, const double *__restrict__ x,
                  const mst_newton_state *__restrict__ state, Workspace ws, NewtonWs nw) {
    if (state->done) return;
    __shared__ double lds[kWaves];
    __shared__ int ldsi[kWaves];
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int phase = state->phase;
    double a = 0.0;
    if (r < n) {
        const int64_t c0 = chunk_ptr[r], c1 = chunk_ptr[r + 1];
        for (int64_t c = c0; c < c1; ++c) a = a + ws.part[c];
    }
    if (phase == kCG) {
        const bool first = state->k == 0;
        double pq = 0.0, rz = 0.0;
        if (r < n && nw.act[r]) {
            const double p = nw.p[r], v = nw.v[r];
            const double q = x[r] * a + v * p;
            nw.q[r] = q;
            pq = p * q;
            if (first) rz = nw.r[r] * p;                // z = p on the first step
        }
        const double t1 = block_sum(pq, lds);
        const double t2 = first ? block_sum(rz, lds) : 0.0;
        if (threadIdx.x == 0) {
            ws.blk_a[blockIdx.x] = t1;
            if (first) ws.blk_b[blockIdx.x] = t2;
        }
        return;
    }
    double res = 0.0;
    int act = 0, unmasked = 0;
    if (r < n) {
        const double xr = x[r];
        const double v = xr * a;
        if (phase == kStart) {
            unmasked = xr != 0.0 ? 1 : 0;
            act = (unmasked && v != 0.0) ? 1 : 0;
            nw.act[r] = act;
            nw.p[r] = 0.0;
            nw.q[r] = 0.0;
        } else {
            act = nw.act[r];
        }
        res = act ? 1.0 - v : 0.0;
        nw.v[r] = act ? v : 0.0;
        nw.r[r] = res;
    }
    const double t1 = block_sum(res * res, lds);
    const double t2 = block_sum(res, lds);
    const int tc = block_sum_i(act, ldsi);
    const int tk = phase == kStart ? block_sum_i(unmasked, ldsi) : 0;
    if (threadIdx.x == 0) {
        ws.blk_a[blockIdx.x] = t1;
        ws.blk_b[blockIdx.x] = t2;
        ws.blk_c[blockIdx.x] = tc;
        if (phase == kStart) nw.blk_k[blockIdx.x] = tk;
    }
}

// one workgroup: the step's scalars.  kCG: p.q, rho on the first step, alpha (or the stop when p.q is not positive and
// finite).  kStart / kOuter: rout, the variance of v, the counters, the trace, the forcing term eta, the stop test and the
// next inner tolerance.  state->cg_step tells the rest of this step's kernels whether they run.
__global__ void __launch_bounds__(kThreads)
newton_scalar_kernel(int64_t n, double tol, int32_t max_matvecs, mst_newton_state *state, Workspace ws,
                     NewtonWs nw, double *__restrict__ trace, int32_t trace_cap) {
    if (state->done) return;
    __shared__ double lds[kWaves];
    __shared__ int ldsi[kWaves];
    const int64_t nb = nblocks(n);
    const int phase = state->phase;
    if (phase == kCG) {
        const bool first = state->k == 0;
        const double pq = reduce_partials(ws.blk_a, nb, lds);
        const double rz = first ? reduce_partials(ws.blk_b, nb, lds) : 0.0;
        if (threadIdx.x == 0) {
            const double rho = first ? rz : state->rho;
            state->rho = rho;
            state->k = state->k + 1;
            state->matvecs = state->matvecs + 1;
            state->cg_step = 1;
            if (!(pq > 0.0) || !isfinite(pq)) {
                state->converged = 0;
                state->done = 1;
            } else {
                state->alpha = rho / pq;
            }
        }
        return;
    }
    const double rout = reduce_partials(ws.blk_a, nb, lds);
    const double s1 = reduce_partials(ws.blk_b, nb, lds);
    const int cnt = reduce_partials_i(ws.blk_c, nb, ldsi);
    const int nk = phase == kStart ? reduce_partials_i(nw.blk_k, nb, ldsi) : 0;
    if (threadIdx.x == 0) {
        double var = 0.0;
        if (cnt > 0) {                                   // v - 1 = -r: var(v) = mean(r^2) - mean(r)^2
            const double m1 = s1 / (double)cnt;
            var = rout / (double)cnt - m1 * m1;
        }
        state->variance = var > 0.0 ? var : 0.0;
        double eta;
        if (phase == kStart) {
            state->active = cnt;
            state->isolated = nk - cnt;
            eta = kEtaMax;
        } else {
            const int it = state->iterations;
            if (it < trace_cap) trace[it] = sqrt(rout);
            state->iterations = it + 1;
            state->matvecs = state->matvecs + 1;
            const double eta_o = state->eta;
            eta = kG * (rout / state->rold);
            if (kG * eta_o * eta_o > 0.1) eta = fmax(eta, kG * eta_o * eta_o);
            eta = fmax(fmin(eta, kEtaMax), 0.5 * tol / sqrt(rout));
        }
        state->eta = eta;
        state->rold = rout;
        state->rout = rout;
        state->rho = rout;
        state->cg_step = 0;
        const double tol2 = tol * tol;
        const bool conv = rout <= tol2;
        if (conv || state->matvecs >= max_matvecs) {
            state->converged = conv ? 1 : 0;
            state->done = 1;
        } else {
            state->phase = kCG;
            state->k = 0;
            state->innertol = fmax(eta * eta * rout, tol2);
        }
    }
}

// CG step: block min / max of ynew = y + alpha p over the active set and of the two candidate cap factors
__global__ void __launch_bounds__(kThreads)
newton_try_kernel(int64_t n, const mst_newton_state *__restrict__ state, NewtonWs nw) {
    if (state->done || !state->cg_step) return;
    __shared__ double lds[kWaves];
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double mn = INFINITY, mx = -INFINITY, clo = INFINITY, chi = INFINITY;
    if (r < n && nw.act[r]) {
        const double y = nw.y[r];
        const double ap = state->alpha * nw.p[r];
        const double yn = y + ap;
        mn = mx = yn;
        if (ap < 0.0) clo = (kCapLo - y) / ap;
        if (yn > kCapHi) chi = (kCapHi - y) / ap;
    }
    mn = block_min(mn, lds);
    mx = -block_min(-mx, lds);
    clo = block_min(clo, lds);
    chi = block_min(chi, lds);
    if (threadIdx.x == 0) {
        nw.mn[blockIdx.x] = mn;
        nw.mx[blockIdx.x] = mx;
        nw.clo[blockIdx.x] = clo;
        nw.chi[blockIdx.x] = chi;
    }
}

// one workgroup: is this CG step capped, and by which factor (state->capped: 0 no, 1 lower cap, 2 upper cap)
__global__ void __launch_bounds__(kThreads)
newton_decide_kernel(int64_t n, mst_newton_state *state, NewtonWs nw) {
    if (state->done || !state->cg_step) return;
    __shared__ double lds[kWaves];
    const int64_t nb = nblocks(n);
    const double mn = reduce_min(nw.mn, nb, lds);
    double a = -INFINITY;
    for (int64_t b = threadIdx.x; b < nb; b += kThreads) a = nw.mx[b] > a ? nw.mx[b] : a;
    const double mx = -block_min(-a, lds);
    const double clo = reduce_min(nw.clo, nb, lds);
    const double chi = reduce_min(nw.chi, nb, lds);
    if (threadIdx.x == 0) {
        int capped = 0;
        double gamma = 1.0;
        if (mn <= kCapLo) {
            capped = 1;
            gamma = clo;
        } else if (mx >= kCapHi) {
            capped = 2;
            gamma = isfinite(chi) ? chi : 1.0;           // no ynew above the cap: max(ynew) equals it, the whole step
        }
        state->capped = capped;
        state->gamma = gamma;
    }
}

// CG step: y and r; block partials of the new r.z (blk_a).  A capped step moves y by gamma * alpha p and leaves r (the outer
// update that follows recomputes it).
__global__ void __launch_bounds__(kThreads)
newton_update_kernel(int64_t n, const mst_newton_state *__restrict__ state, Workspace ws, NewtonWs nw) {
    if (state->done || !state->cg_step) return;
    __shared__ double lds[kWaves];
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool capped = state->capped != 0;
    double rz = 0.0;
    if (r < n && nw.act[r]) {
        const double alpha = state->alpha;
        const double ap = alpha * nw.p[r];
        if (capped) {
            nw.y[r] = nw.y[r] + state->gamma * ap;
        } else {
            nw.y[r] = nw.y[r] + ap;
            const double res = nw.r[r] - alpha * nw.q[r];
            nw.r[r] = res;
            rz = res * (res / nw.v[r]);
        }
    }
    if (capped) return;
    const double t = block_sum(rz, lds);
    if (threadIdx.x == 0) ws.blk_a[blockIdx.x] = t;
}

// one workgroup: the end of a CG step -- the new rho and whether the inner iteration goes on
__global__ void __launch_bounds__(kThreads)
newton_finish_kernel(int64_t n, int32_t max_matvecs, mst_newton_state *state, Workspace ws) {
    if (state->done || !state->cg_step) return;
    __shared__ double lds[kWaves];
    const int capped = state->capped;
    if (capped) {
        if (threadIdx.x == 0) {
            state->capped_steps = state->capped_steps + 1;
            if (capped == 2) state->capped_upper = state->capped_upper + 1;
            state->phase = kOuter;
        }
        return;
    }
    const double rho = reduce_partials(ws.blk_a, nblocks(n), lds);
    if (threadIdx.x == 0) {
        state->rho_prev = state->rho;
        state->rho = rho;
        if (!(rho > state->innertol) || state->matvecs >= max_matvecs) state->phase = kOuter;
    }
}

int grid_for(int64_t items, int64_t per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g < 1048576 ? g : 1048576));
}

int check_csr(const char *who, const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
              const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, void *workspace, uint64_t workspace_bytes,
              bool newton = false) {
    if (!row_ptr || !chunk_ptr || n <= 0 || n > INT32_MAX || n_chunks < 0 || (n_chunks > 0 && (!col || !val || !chunk_row)))
        return mst::fail(MST_E_ARG, "%s: bad CSR argument (n %lld, chunks %lld)", who, (long long)n, (long long)n_chunks);
    const uint64_t need = newton ? newton_need(n, n_chunks) : ws_need(n, n_chunks);
    if (!workspace || workspace_bytes < need)
        return mst::fail(MST_E_ARG, "%s: workspace of %llu bytes, %llu needed", who, (unsigned long long)workspace_bytes,
                         (unsigned long long)need);
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
                                                                                    n_chunks, w, &state->done, ws);
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

extern "C" uint64_t mst_balance_newton_workspace_bytes(int64_t n, int64_t n_chunks) {
    if (n <= 0 || n_chunks < 0) return 0;
    return newton_need(n, n_chunks);
}

extern "C" int mst_balance_newton(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                                  const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, double *w, int32_t steps,
                                  int32_t max_matvecs, double tol, mst_newton_state *state, double *trace, int32_t trace_cap,
                                  void *workspace, uint64_t workspace_bytes, void *stream) {
    int rc = check_csr("mst_balance_newton", row_ptr, col, val, chunk_row, chunk_ptr, n, n_chunks, workspace, workspace_bytes,
                       true);
    if (rc != MST_OK) return rc;
    if (!w || !state || steps < 0 || max_matvecs < 0 || !(tol > 0.0) || trace_cap < 0 || (trace_cap > 0 && !trace))
        return mst::fail(MST_E_ARG, "mst_balance_newton: bad argument");
    hipStream_t s = mst::as_stream(stream);
    Workspace ws = carve(workspace, n, n_chunks);
    NewtonWs nw = carve_newton(workspace, n, n_chunks);
    const int nb = (int)nblocks(n);
    for (int k = 0; k < steps; ++k) {
        newton_prep_kernel<<<nb, kThreads, 0, s>>>(n, w, state, nw);
        MST_LAUNCH_CHECK();
        if (n_chunks > 0) {
            chunk_kernel<kMarginal><<<grid_for(n_chunks, kWaves), kThreads, 0, s>>>(row_ptr, col, val, chunk_row, chunk_ptr,
                                                                                    n_chunks, nw.wv, &state->done, ws);
            MST_LAUNCH_CHECK();
        }
        newton_row_kernel<<<nb, kThreads, 0, s>>>(chunk_ptr, n, w, state, ws, nw);
        MST_LAUNCH_CHECK();
        newton_scalar_kernel<<<1, kThreads, 0, s>>>(n, tol, max_matvecs, state, ws, nw, trace, trace_cap);
        MST_LAUNCH_CHECK();
        newton_try_kernel<<<nb, kThreads, 0, s>>>(n, state, nw);
        MST_LAUNCH_CHECK();
        newton_decide_kernel<<<1, kThreads, 0, s>>>(n, state, nw);
        MST_LAUNCH_CHECK();
        newton_update_kernel<<<nb, kThreads, 0, s>>>(n, state, ws, nw);
        MST_LAUNCH_CHECK();
        newton_finish_kernel<<<1, kThreads, 0, s>>>(n, max_matvecs, state, ws);
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

extern "C" int mst_balance_apply_pairs(const int32_t *x, const int32_t *y, const double *v, int64_t n_records, const int64_t *seg_off,
                                       const int64_t *row_off, const int64_t *col_off, int32_t P, const double *bias, int64_t n_bias,
                                       double *out, void *stream) {
    if (n_records < 0 || P < 0 || n_bias < 0 || (n_bias > 0 && !bias) ||
        (n_records > 0 && (P < 1 || !x || !y || !v || !out || !seg_off || !row_off || !col_off)))
        return mst::fail(MST_E_ARG, "mst_balance_apply_pairs: bad argument");
    if (n_records == 0 || P == 0) return MST_OK;
    hipStream_t s = mst::as_stream(stream);
    const bool vec = ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 &&
                     ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 7) == 0;
    if (vec)
        apply_pairs_kernel<true><<<grid_for((n_records + 1) / 2, kThreads), kThreads, 0, s>>>(x, y, v, n_records, seg_off, row_off,
                                                                                              col_off, P, bias, n_bias, out);
    else
        apply_pairs_kernel<false><<<grid_for(n_records, kThreads), kThreads, 0, s>>>(x, y, v, n_records, seg_off, row_off, col_off,
                                                                                     P, bias, n_bias, out);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
