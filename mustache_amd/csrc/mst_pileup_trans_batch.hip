// Aggregate peak analysis (APA) of a loop list on inter-chromosomal (trans) pairs, P chromosome pairs at once (mustache_amd/pileup.py
// states the rules; tests/pileup_trans_reference.py restates them per pair).  A trans pair has no band and no distance decay: the
// map is the pair's COO records (x = bin of A, y = bin of B, v > 0), the expected value one scalar per pair.  The records of the
// pairs are concatenated (x, y, v with seg_off, as mst_balance_apply_pairs writes them), and so are the loops (lx, ly with loop_off).
//
//   mst_pileup_trans_batch        per pair: one pass over the records for the valid rows / columns, the exact total and the window
//                                 cells; then E, oe, each loop's centres and its own P2LL.  A pair's values do not depend on the
//                                 pairs beside it.
//   mst_pileup_trans_windows      a single pair: the same body with P = 1 (host tables seg_off = {0, N}, loop_off = {0, L})
// The reduce over the pairs' windows is mst_pileup_reduce_segmented (mst_pileup_reduce.hip).
//
// A record with !(v > 0) -- zero, negative, NaN -- is ignored altogether: no valid flag, nothing in the sum, no window.  So the
// output of mst_balance_apply_pairs goes in as it is, without a compaction per pair.
//
// The small tables are built on the host from the segment lengths (host metadata: no wait) and uploaded in ONE copy:
//   pair table    per pair: its records, its loops, where its valid flags and its row bits start, n1, n2
//   loop_off      the loops' segment table, for the kernels that find a loop's pair (segment_of)
//   chunk table   (first record, count, pair): kChunk records of ONE pair, so a workgroup's trip never crosses a segment
//   rank table    (first loop, pair): kThreads loops of ONE pair
//
// Launches behind mst_pileup_trans_batch, in stream order (five and a few memsets, whatever P is):
//   rank_kernel      one workgroup per rank-table entry: its loops sorted by row (lx, ties by input position) INSIDE their segment
//                    (sx, sy, sid at the segment's own positions) -- sum of L_p^2 comparisons, not (sum L_p)^2; L_p is a loop
//                    list (thousands), not a map.
//   init_kernel      one workgroup per loop: window cells 0.0 / NaN with ITS pair's n1, n2; the bit "some window covers this row"
//                    of (pair, row) for its rows lx - w .. lx + w (integer atomicOr).
//   records_kernel   workgroups stride over the chunk table, 16 B read per record (x, y int32, v f64).  Every record that counts
//                    marks its pair's valid_rows[x] and valid_cols[y] (plain racing stores of 1) and adds v to the exact sum
//                    (mst_exact_sum.h).  The exact sum's LDS limbs, the kept and the non-finite counts and the LDS copy of the row
//                    bits belong to the pair of the current chunk; when the next chunk is another pair's, the limbs are flushed
//                    (64-bit integer atomics into that pair's words) and the next pair's row bits are loaded: once per workgroup
//                    and pair.  A pair whose bitmap exceeds kLdsFlagWords reads it from global memory -- decided per pair, the
//                    same values either way.  A record whose row bit is set binary-searches sx inside [loop0, loop1) of the pair
//                    for the first loop with lx >= x - w, walks the run up to lx <= x + w and writes the cell of every loop with
//                    |y - ly| <= w: a 64-bit integer max on the bit pattern of the positive double, so a repeated pixel keeps
//                    its largest value whatever the order.
//   expected_kernel  one workgroup per pair: E = exact total / (#valid rows * #valid columns) (integer counts, one division), kept.
//   finish_kernel    one workgroup per loop, reading its pair's E: oe = obs / E, the two centres and P2LL in a fixed tree.
//
// The exact sum keeps kSumCopies copies of its LDS limbs, chosen by lane: the values of a trans map share a few exponents, so the
// lanes of a wave hit the same limbs, and LDS atomics on one address are served one after another.  The sums are integer sums
// (mst_exact_sum.h) or fixed-order trees.  No float atomics: every output is bit-identical from run to run and under any
// permutation of the records within a segment and of the loops within a segment.
#include <cmath>
#include <vector>
#include "mst_common.h"
#include "mst_exact_sum.h"
#include "mst_pileup_sums.h"

namespace {

using mst_exact::add_exact;
using mst_exact::exact_to_double;
using mst_exact::kLimbs;
using mst_exact::kSumWords;
using mst_pileup::align256;
using mst_pileup::block_sum2;
using mst_pileup::check_pairs;
using mst_pileup::check_w;
using mst_pileup::grid_ok;
using mst_pileup::kMaxPairs;
using mst_pileup::kThreads;
using mst_pileup::kWaves;
using mst_pileup::offsets_ok;

constexpr int kLdsFlagWords = 4096;        // 16 KiB of row bits in LDS = 131 072 rows of one pair; beyond, read from global
constexpr int kSumCopies = 16;             // copies of the exact sum's LDS limbs, one per lane & 15
constexpr int kSumStride = kLimbs + 1;
constexpr int kRecordBlocks = 2048;        // grid cap of the record pass
constexpr int kChunk = 4096;               // records of a chunk: 16 per thread, 64 KiB read
constexpr int64_t kMaxRecords = ((int64_t)1 << 31) - 1;      // of one call
constexpr uint64_t kKeptSlot = 256;        // mst_pileup_trans_windows: the batch's `kept` word, at the start of the workspace

struct PairRow {                           // one pair of the batch
    int64_t seg0, seg1;                    // its records
    int64_t loop0, loop1;                  // its loops
    int64_t row_off, col_off;              // its first valid_rows / valid_cols byte
    int64_t bit_off;                       // its first word of row bits
    int32_t n1, n2;
};

struct Chunk {
    int64_t first;
    int32_t count, pair;
};

struct RankBlock {
    int64_t first;                         // the first loop of the workgroup
    int32_t pair, unused;
};

struct Layout {                            // the workspace, in this order
    uint64_t words, sx, sy, sid, bits, tables, end;
    uint64_t t_pairs, t_loop_off, t_chunks, t_ranks, t_bytes;      // inside the table blob
    int64_t nwords, nchunks, nranks;
};

inline int64_t words_of(int64_t n1) { return (n1 + 31) / 32; }

// seg_off, n1, loop_off: host tables the caller has checked (or zeros); loop_off may be null (no loop)
Layout layout(const int64_t *seg_off, const int64_t *n1, const int64_t *loop_off, int32_t P, int64_t L) {
    Layout o;
    o.nwords = o.nchunks = o.nranks = 0;
    for (int32_t p = 0; p < P; ++p) {
        o.nwords += words_of(n1[p]);
        o.nchunks += (seg_off[p + 1] - seg_off[p] + kChunk - 1) / kChunk;
        if (loop_off) o.nranks += (loop_off[p + 1] - loop_off[p] + kThreads - 1) / kThreads;
    }
    o.t_pairs = 0;
    o.t_loop_off = o.t_pairs + align256((uint64_t)P * sizeof(PairRow));
    o.t_chunks = o.t_loop_off + align256((uint64_t)(P + 1) * 8);
    o.t_ranks = o.t_chunks + align256((uint64_t)o.nchunks * sizeof(Chunk));
    o.t_bytes = o.t_ranks + align256((uint64_t)o.nranks * sizeof(RankBlock));
    o.words = 0;
    o.sx = o.words + align256((uint64_t)P * kSumWords * 8);
    o.sy = o.sx + align256((uint64_t)L * 8);
    o.sid = o.sy + align256((uint64_t)L * 8);
    o.bits = o.sid + align256((uint64_t)L * 4);
    o.tables = o.bits + align256((uint64_t)o.nwords * 4);
    o.end = o.tables + o.t_bytes;
    return o;
}

// ---- the loops by row, inside their segment --------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
rank_kernel(const int64_t *__restrict__ lx, const int64_t *__restrict__ ly, const PairRow *__restrict__ pairs,
            const RankBlock *__restrict__ ranks, int64_t *__restrict__ sx, int64_t *__restrict__ sy, int32_t *__restrict__ sid) {
    __shared__ int64_t tile[kThreads];
    const RankBlock rb = ranks[blockIdx.x];
    const int64_t l0 = pairs[rb.pair].loop0, l1 = pairs[rb.pair].loop1;
    const int64_t l = rb.first + threadIdx.x;
    const int64_t key = l < l1 ? lx[l] : 0;
    int64_t rank = 0;
    for (int64_t m0 = l0; m0 < l1; m0 += kThreads) {
        __syncthreads();
        if (m0 + threadIdx.x < l1) tile[threadIdx.x] = lx[m0 + threadIdx.x];
        __syncthreads();
        const int nm = l1 - m0 < kThreads ? (int)(l1 - m0) : kThreads;
        for (int k = 0; k < nm; ++k) {
            const int64_t o = tile[k];
            rank += (o < key || (o == key && m0 + k < l)) ? 1 : 0;
        }
    }
    if (l < l1) {
        sx[l0 + rank] = key;
        sy[l0 + rank] = ly[l];
        sid[l0 + rank] = (int32_t)l;
    }
}

// ---- windows before the records: 0.0 on the pair's map, NaN off it; the row bits of (pair, row) --------------------------------
__global__ void __launch_bounds__(kThreads)
init_kernel(const int64_t *__restrict__ lx, const int64_t *__restrict__ ly, const PairRow *__restrict__ pairs,
            const int64_t *__restrict__ loop_off, int32_t P, int32_t w, double *__restrict__ obs, uint32_t *__restrict__ bits) {
    const int64_t l = blockIdx.x;
    const PairRow pr = pairs[mst::segment_of(loop_off, 0, P, l)];
    const int64_t n1 = pr.n1, n2 = pr.n2;
    const int64_t X = lx[l], Y = ly[l];
    const int S = 2 * w + 1;
    double *o_out = obs + l * (int64_t)S * S;
    for (int cell = threadIdx.x; cell < S * S; cell += kThreads) {
        const int64_t i = X + cell / S - w, j = Y + cell % S - w;
        o_out[cell] = (i >= 0 && i < n1 && j >= 0 && j < n2) ? 0.0 : NAN;
    }
    if ((int)threadIdx.x < S) {
        const int64_t row = X - w + threadIdx.x;
        if (row >= 0 && row < n1) atomicOr(&bits[pr.bit_off + (row >> 5)], 1u << (row & 31));
    }
}

// A pair is over for this workgroup: its LDS limbs and counts go to its words (64-bit integer atomics), the LDS copies back to
// zero.  Called by every thread of the workgroup; a barrier follows before the LDS is used again.
__device__ __forceinline__ void flush_pair(unsigned long long *acc, unsigned long long *bad, unsigned long long *kept,
                                           unsigned long long &nbad, unsigned long long &nkept, unsigned long long *out) {
    if (nbad) atomicAdd(bad, nbad);
    if (nkept) atomicAdd(kept, nkept);
    nbad = nkept = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < kLimbs; i += kThreads) {
        unsigned long long t = 0;
#pragma unroll
        for (int c = 0; c < kSumCopies; ++c) {
            t += acc[c * kSumStride + i];
            acc[c * kSumStride + i] = 0;
        }
        if (t) atomicAdd(&out[i], t);
    }
    if (threadIdx.x == 0) {
        if (*kept) atomicAdd(&out[kLimbs], *kept);
        if (*bad) atomicAdd(&out[kLimbs + 1], *bad);
        *bad = *kept = 0;
    }
}

// ---- the one pass over the records ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
records_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, const double *__restrict__ v,
               const PairRow *__restrict__ pairs, const Chunk *__restrict__ chunks, int64_t nchunks,
               const int64_t *__restrict__ sx, const int64_t *__restrict__ sy, const int32_t *__restrict__ sid, int32_t w,
               const uint32_t *__restrict__ bits, uint8_t *__restrict__ valid_rows, uint8_t *__restrict__ valid_cols,
               double *__restrict__ obs, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long acc[kSumCopies * kSumStride];
    __shared__ unsigned long long bad, kept;
    __shared__ uint32_t flags[kLdsFlagWords];
    for (int i = threadIdx.x; i < kSumCopies * kSumStride; i += kThreads) acc[i] = 0;
    if (threadIdx.x == 0) bad = kept = 0;
    unsigned long long *mine = acc + (threadIdx.x & (kSumCopies - 1)) * kSumStride;
    const int64_t cells = (int64_t)(2 * w + 1) * (2 * w + 1);
    unsigned long long nbad = 0, nkept = 0;
    int32_t cur = -1;
    PairRow pr = {};
    bool lds_flags = false;
    const uint32_t *pbits = bits;

    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ch = chunks[c];
        if (ch.pair != cur) {                                         // the same for every thread of the workgroup
            if (cur >= 0) flush_pair(acc, &bad, &kept, nbad, nkept, words + (int64_t)cur * kSumWords);
            cur = ch.pair;
            pr = pairs[cur];
            const int64_t nwords = ((int64_t)pr.n1 + 31) / 32;
            lds_flags = nwords <= kLdsFlagWords;
            pbits = bits + pr.bit_off;
            __syncthreads();                                          // nobody reads the old flags any more
            if (lds_flags)
                for (int i = threadIdx.x; i < (int)nwords; i += kThreads) flags[i] = pbits[i];
            __syncthreads();
        }
        const int64_t n1 = pr.n1, n2 = pr.n2, L0 = pr.loop0, L1 = pr.loop1;
        const int64_t end = ch.first + ch.count;
        for (int64_t i = ch.first + threadIdx.x; i < end; i += kThreads) {
            const int64_t xi = x[i], yi = y[i];
            const double vi = v[i];
            if (!(vi > 0.0)) continue;                                // zero, negative, NaN: not a record of the map
            if (xi < 0 || xi >= n1 || yi < 0 || yi >= n2) continue;   // not a pixel of this pair's map
            valid_rows[pr.row_off + xi] = 1;
            valid_cols[pr.col_off + yi] = 1;
            ++nkept;
            if (!add_exact(vi, mine)) {
                ++nbad;
                continue;
            }
            const uint32_t word = lds_flags ? flags[xi >> 5] : pbits[xi >> 5];
            if (!((word >> (xi & 31)) & 1u)) continue;
            int64_t lo = L0, hi = L1;                                 // the pair's first loop with lx >= x - w
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (sx[mid] < xi - w) lo = mid + 1;
                else hi = mid;
            }
            for (int64_t p = lo; p < L1; ++p) {
                const int64_t da = xi - sx[p];
                if (da < -w) break;
                const int64_t db = yi - sy[p];
                if (db < -w || db > w) continue;
                long long *cell = reinterpret_cast<long long *>(obs + sid[p] * cells + (da + w) * (2 * w + 1) + (db + w));
                atomicMax(cell, __double_as_longlong(vi));            // positive doubles order like their bit patterns
            }
        }
    }
    if (cur >= 0) flush_pair(acc, &bad, &kept, nbad, nkept, words + (int64_t)cur * kSumWords);
}

// ---- per pair: E = exact total / (#valid rows * #valid columns); NaN when a record was not finite; kept ------------------------
__global__ void __launch_bounds__(kThreads)
expected_kernel(const unsigned long long *__restrict__ words, const PairRow *__restrict__ pairs,
                const uint8_t *__restrict__ valid_rows, const uint8_t *__restrict__ valid_cols, double *__restrict__ expected,
                int64_t *__restrict__ kept) {
    __shared__ double lds[kWaves];
    __shared__ long long ldc[kWaves];
    __shared__ long long digits[kLimbs + 1];
    __shared__ double total;
    const unsigned long long *mine = words + (int64_t)blockIdx.x * kSumWords;
    if (threadIdx.x == 0) total = exact_to_double(mine, digits);
    const PairRow *pr = pairs + blockIdx.x;
    const uint8_t *vr = valid_rows + pr->row_off, *vc = valid_cols + pr->col_off;
    const int64_t n1 = pr->n1, n2 = pr->n2;
    long long rows = 0, cols = 0;
    double unused = 0.0;
    for (int64_t i = threadIdx.x; i < n1; i += kThreads) rows += vr[i] ? 1 : 0;
    for (int64_t i = threadIdx.x; i < n2; i += kThreads) cols += vc[i] ? 1 : 0;
    block_sum2(unused, rows, lds, ldc);
    block_sum2(unused, cols, lds, ldc);
    if (threadIdx.x != 0) return;
    const long long cnt = rows * cols;
    expected[blockIdx.x] = mine[kLimbs + 1] ? NAN : (cnt ? total / (double)cnt : 0.0);
    kept[blockIdx.x] = (int64_t)mine[kLimbs];
}

// ---- finish: oe, the centres and the loop's own P2LL, with its pair's E ---------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
finish_kernel(const double *__restrict__ obs, const double *__restrict__ expected, const int64_t *__restrict__ loop_off, int32_t P,
              int32_t w, int32_t q, double *__restrict__ oe, double *__restrict__ stats) {
    __shared__ double lds[kWaves];
    __shared__ long long ldc[kWaves];
    const int64_t l = blockIdx.x;
    const int S = 2 * w + 1;
    const double ex = expected[mst::segment_of(loop_off, 0, P, l)];
    const double *o_in = obs + l * (int64_t)S * S;
    double *e_out = oe + l * (int64_t)S * S;
    double ll = 0.0;
    long long ll_n = 0;
    for (int cell = threadIdx.x; cell < S * S; cell += kThreads) {
        const double o = o_in[cell];
        e_out[cell] = (ex != 0.0 && o == o) ? o / ex : NAN;
        const int a = cell / S, b = cell % S;
        if (a >= 2 * w - q + 1 && b <= q - 1 && o == o) {             // the LL index range, cells on the map
            ll = ll + o;
            ++ll_n;
        }
    }
    block_sum2(ll, ll_n, lds, ldc);
    if (threadIdx.x == 0) {
        const double c = o_in[w * S + w];
        const double mean = ll_n ? ll / (double)ll_n : 0.0;
        stats[l * 3 + 0] = c;
        stats[l * 3 + 1] = (ex != 0.0 && c == c) ? c / ex : NAN;
        stats[l * 3 + 2] = (ll_n && mean != 0.0) ? c / mean : NAN;
    }
}

// ---- the body behind both entry points (`who` names the caller in a refusal): every check, the tables, the launches ------------
int run_batch(const char *who, const int32_t *x, const int32_t *y, const double *v, int64_t N, const int64_t *seg_off,
              const int64_t *n1, const int64_t *n2, const int64_t *lx, const int64_t *ly, int64_t L, const int64_t *loop_off,
              int32_t P, int32_t w, int32_t q, uint8_t *valid_rows, uint8_t *valid_cols, double *expected, int64_t *kept,
              double *obs, double *oe, double *loop_stats, void *workspace, uint64_t workspace_bytes, void *stream) {
    int rc = check_w(who, w, q);
    if (rc != MST_OK) return rc;
    if ((rc = check_pairs(who, P)) != MST_OK) return rc;
    if (N < 0 || N > kMaxRecords || L < 0 || L > INT32_MAX || !n1 || !n2 || !valid_rows || !valid_cols || !expected ||
        !kept || (N > 0 && (!x || !y || !v)) || (L > 0 && (!lx || !ly || !obs || !oe || !loop_stats)))
        return mst::fail(MST_E_ARG, "%s: bad argument (N %lld < 2^31 records, L %lld)", who, (long long)N, (long long)L);
    if (!offsets_ok(seg_off, P, N) || !offsets_ok(loop_off, P, L))
        return mst::fail(MST_E_ARG, "%s: seg_off / loop_off (host, P + 1 entries) must rise from 0 to N = %lld / L = %lld", who,
                         (long long)N, (long long)L);
    int64_t rows = 0, cols = 0;
    for (int32_t p = 0; p < P; ++p) {
        if (n1[p] < 1 || n2[p] < 1 || n1[p] > INT32_MAX || n2[p] > INT32_MAX)
            return mst::fail(MST_E_ARG, "%s: pair %d is %lld x %lld bins", who, (int)p, (long long)n1[p], (long long)n2[p]);
        rows += n1[p];
        cols += n2[p];
    }
    const Layout o = layout(seg_off, n1, loop_off, P, L);
    if (!workspace || workspace_bytes < o.end)
        return mst::fail(MST_E_ARG, "%s: workspace of %llu bytes, %llu needed", who, (unsigned long long)workspace_bytes,
                         (unsigned long long)o.end);
    if (L > 0 && (rc = grid_ok(who, L)) != MST_OK) return rc;

    // the tables: one blob, one copy
    static thread_local std::vector<char> blob;
    blob.assign(o.t_bytes, 0);
    auto *h_pairs = reinterpret_cast<PairRow *>(blob.data() + o.t_pairs);
    auto *h_loop_off = reinterpret_cast<int64_t *>(blob.data() + o.t_loop_off);
    auto *h_chunks = reinterpret_cast<Chunk *>(blob.data() + o.t_chunks);
    auto *h_ranks = reinterpret_cast<RankBlock *>(blob.data() + o.t_ranks);
    int64_t row_off = 0, col_off = 0, bit_off = 0, nc = 0, nr = 0;
    for (int32_t p = 0; p < P; ++p) {
        PairRow &pr = h_pairs[p];
        pr.seg0 = seg_off[p];
        pr.seg1 = seg_off[p + 1];
        pr.loop0 = loop_off[p];
        pr.loop1 = loop_off[p + 1];
        pr.row_off = row_off;
        pr.col_off = col_off;
        pr.bit_off = bit_off;
        pr.n1 = (int32_t)n1[p];
        pr.n2 = (int32_t)n2[p];
        row_off += n1[p];
        col_off += n2[p];
        bit_off += words_of(n1[p]);
        h_loop_off[p] = loop_off[p];
        for (int64_t f = pr.seg0; f < pr.seg1; f += kChunk)
            h_chunks[nc++] = Chunk{f, (int32_t)(pr.seg1 - f < kChunk ? pr.seg1 - f : kChunk), p};
        for (int64_t f = pr.loop0; f < pr.loop1; f += kThreads) h_ranks[nr++] = RankBlock{f, p, 0};
    }
    h_loop_off[P] = loop_off[P];

    hipStream_t s = mst::as_stream(stream);
    char *base = static_cast<char *>(workspace);
    auto *words = reinterpret_cast<unsigned long long *>(base + o.words);
    auto *sx = reinterpret_cast<int64_t *>(base + o.sx), *sy = reinterpret_cast<int64_t *>(base + o.sy);
    auto *sid = reinterpret_cast<int32_t *>(base + o.sid);
    auto *bits = reinterpret_cast<uint32_t *>(base + o.bits);
    char *tables = base + o.tables;
    const auto *d_pairs = reinterpret_cast<const PairRow *>(tables + o.t_pairs);
    const auto *d_loop_off = reinterpret_cast<const int64_t *>(tables + o.t_loop_off);
    const auto *d_chunks = reinterpret_cast<const Chunk *>(tables + o.t_chunks);
    const auto *d_ranks = reinterpret_cast<const RankBlock *>(tables + o.t_ranks);
    MST_HIP(mst::upload_small(tables, blob.data(), o.t_bytes, s));
    MST_HIP(hipMemsetAsync(words, 0, (size_t)P * kSumWords * 8, s));
    MST_HIP(hipMemsetAsync(bits, 0, (size_t)o.nwords * 4, s));
    MST_HIP(hipMemsetAsync(valid_rows, 0, (size_t)rows, s));
    MST_HIP(hipMemsetAsync(valid_cols, 0, (size_t)cols, s));
    if (L > 0) {
        rank_kernel<<<(unsigned)o.nranks, kThreads, 0, s>>>(lx, ly, d_pairs, d_ranks, sx, sy, sid);
        MST_LAUNCH_CHECK();
        init_kernel<<<(unsigned)L, kThreads, 0, s>>>(lx, ly, d_pairs, d_loop_off, P, w, obs, bits);
        MST_LAUNCH_CHECK();
    }
    if (o.nchunks > 0) {
        const unsigned g = (unsigned)(o.nchunks < kRecordBlocks ? o.nchunks : kRecordBlocks);
        records_kernel<<<g, kThreads, 0, s>>>(x, y, v, d_pairs, d_chunks, o.nchunks, sx, sy, sid, w, bits, valid_rows, valid_cols,
                                              obs, words);
        MST_LAUNCH_CHECK();
    }
    expected_kernel<<<(unsigned)P, kThreads, 0, s>>>(words, d_pairs, valid_rows, valid_cols, expected, kept);
    MST_LAUNCH_CHECK();
    if (L > 0) {
        finish_kernel<<<(unsigned)L, kThreads, 0, s>>>(obs, expected, d_loop_off, P, w, q, oe, loop_stats);
        MST_LAUNCH_CHECK();
    }
    return MST_OK;
}

}  // namespace

extern "C" uint64_t mst_pileup_trans_batch_workspace_bytes(const int64_t *seg_off, const int64_t *n1, const int64_t *loop_off,
                                                           int32_t P, int32_t w) {
    if (P < 1 || P > kMaxPairs || w < 0 || w > mst_pileup::kMaxW || !seg_off || !n1 || !loop_off) return 0;
    if (!offsets_ok(seg_off, P, seg_off[P]) || !offsets_ok(loop_off, P, loop_off[P])) return 0;
    for (int32_t p = 0; p < P; ++p)
        if (n1[p] < 1 || n1[p] > INT32_MAX) return 0;
    return layout(seg_off, n1, loop_off, P, loop_off[P]).end + 256;
}

extern "C" int mst_pileup_trans_batch(const int32_t *x, const int32_t *y, const double *v, int64_t N, const int64_t *seg_off,
                                      const int64_t *n1, const int64_t *n2, const int64_t *lx, const int64_t *ly, int64_t L,
                                      const int64_t *loop_off, int32_t P, int32_t w, int32_t q, uint8_t *valid_rows,
                                      uint8_t *valid_cols, double *expected, int64_t *kept, double *obs, double *oe,
                                      double *loop_stats, void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_trans_batch");
    return run_batch("mst_pileup_trans_batch", x, y, v, N, seg_off, n1, n2, lx, ly, L, loop_off, P, w, q, valid_rows, valid_cols,
                     expected, kept, obs, oe, loop_stats, workspace, workspace_bytes, stream);
}

// ---- a single pair: a batch of one.  The caller's workspace starts with the slot of the batch's `kept` word, which this call does
// not hand out.  N is no argument of the size query, so it reports the chunk table of the most records a call takes (8 MiB).
extern "C" uint64_t mst_pileup_trans_workspace_bytes(int64_t n1, int64_t n2, int64_t L, int32_t w) {
    if (n1 <= 0 || n2 <= 0 || n1 > INT32_MAX || n2 > INT32_MAX || L < 0 || L > INT32_MAX || w < 0 || w > mst_pileup::kMaxW) return 0;
    const int64_t seg_off[2] = {0, kMaxRecords}, loop_off[2] = {0, L};
    const uint64_t own = kKeptSlot + layout(seg_off, &n1, loop_off, 1, L).end;
    const uint64_t red = mst_pileup_workspace_bytes(1, 0, L, w);                              // mst_pileup_reduce comes after
    return (own > red ? own : red) + 256;
}

extern "C" int mst_pileup_trans_windows(const int32_t *x, const int32_t *y, const double *v, int64_t N, int64_t n1, int64_t n2,
                                        const int64_t *lx, const int64_t *ly, int64_t L, int32_t w, int32_t q, uint8_t *valid_rows,
                                        uint8_t *valid_cols, double *expected, double *obs, double *oe, double *loop_stats,
                                        void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("pileup: mst_pileup_trans_windows");
    const uint64_t need = mst_pileup_trans_workspace_bytes(n1, n2, L, w);      // 0: a bad n1, n2, L or w, which run_batch names
    if (need && (!workspace || workspace_bytes < need))
        return mst::fail(MST_E_ARG, "mst_pileup_trans_windows: workspace of %llu bytes, %llu needed",
                         (unsigned long long)workspace_bytes, (unsigned long long)need);
    const int64_t seg_off[2] = {0, N}, loop_off[2] = {0, L};
    char *base = static_cast<char *>(workspace);
    return run_batch("mst_pileup_trans_windows", x, y, v, N, seg_off, &n1, &n2, lx, ly, L, loop_off, 1, w, q, valid_rows,
                     valid_cols, expected, reinterpret_cast<int64_t *>(base), obs, oe, loop_stats, base ? base + kKeptSlot : nullptr,
                     need ? need - kKeptSlot : 0, stream);
}
