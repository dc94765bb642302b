// Binomial thinning of the resident trans records of MANY chromosome pairs in one launch (mustache_amd/downsample.py states the
// rule; include/mustache_hip.h the entry point; tests/downsample_genome_reference.py restates it in NumPy).
//
//   mst_thin_pairs    the records of P pairs lie concatenated, pair p in [seg_off[p], seg_off[p + 1]).  A record (x, y) of pair p
//                     with count n keeps k = #{ j in [0, n) : u_j < T }, u_j = word j & 3 of Philox4x32-10(counter = (a, b,
//                     j >> 2, tag_p), key = (seed, key1)), (a, b) = (y, x) when swap_p is set and (x, y) otherwise: the bin on
//                     the pair's first chromosome leads, however the record is stored.  The draws are mst_thin_draws.h's, so a
//                     pair with swap = 0 gives what mst_thin_counts gives for (x, dist = y - x) under the same tag and key.
//
// A lane finds its pair with mst::segment_of.  The search is wave-uniform when lanes 0 and 63 lie in one segment (the idiom of
// mst_pairs_trans.hip): the pair's {tag, swap} is then one scalar load.  The light / heavy split of mst_thin.hip stays; in heavy
// mode the owner's tag is broadcast with its (already oriented) pixel, since neighbouring lanes may belong to different pairs.
// The per-pair totals (reads in, reads kept) are integer sums.  A wave that lies in one pair adds across its lanes and keeps the
// two sums in registers for as long as its trips stay in that pair -- a workgroup takes consecutive tiles of 256 records, so
// they do while the pair lasts: one pair of 64-bit atomics when the pair changes and at the end.  A wave that straddles a
// boundary credits each pair it touches exactly: the pairs of its lanes are taken one at a time (they ascend with the lane),
// each with a masked sum across the wave.  Integer addition is order-free: the totals and every k are the same under any order
// of the records within a pair and for any launch shape.
#include "mst_common.h"
#include "mst_thin_draws.h"

namespace {

constexpr int kThreads = 256;
constexpr int kDefaultBlocks = 4096;               // 16 workgroups a CU, the fastest of a sweep; trans counts are small
using mst::count_of;
using mst::thin_calls;
using mst::wave_sum;

__device__ __forceinline__ void credit(unsigned long long *__restrict__ words, int32_t p, unsigned long long in,
                                       unsigned long long kept) {
    if (in) atomicAdd(&words[2 * (int64_t)p], in);
    if (kept) atomicAdd(&words[2 * (int64_t)p + 1], kept);
}

template <typename C>
__global__ __launch_bounds__(kThreads) void
thin_pairs_kernel(const int32_t *__restrict__ xs, const int32_t *__restrict__ ys, const C *__restrict__ count_in, int64_t N,
                  const int64_t *__restrict__ seg_off, const mst_thin_pair *__restrict__ table, int32_t P, uint32_t seed,
                  uint32_t key1, uint32_t T, int64_t *__restrict__ count_out, unsigned long long *__restrict__ words) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a workgroup takes consecutive tiles of kThreads records, so that a wave's trips stay in one pair for as long as the pair
    // lasts: its sums stay in registers and its pair is found with one comparison
    const int64_t tiles = (N + kThreads - 1) / kThreads, per = (tiles + gridDim.x - 1) / gridDim.x;
    const int64_t tile0 = (int64_t)blockIdx.x * per, tile1 = tile0 + per < tiles ? tile0 + per : tiles;
    // the sums of the pair this wave is in (the same in every lane), not yet credited
    int32_t held = -1, p_wave = -1;
    unsigned long long held_in = 0, held_kept = 0;
    bool bad = false;
    // every lane of a wave makes the same trips (the ballot and the shuffles need that); `e < N` guards the loads and the store
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t e0 = tile * kThreads + wave * 64, e = e0 + lane;
        if (e0 >= N) continue;                      // wave-uniform: nothing of this trip is this wave's
        const bool active = e < N;
        const int64_t last = e0 + 63 < N ? e0 + 63 : N - 1;
        // e0 ascends from trip to trip: the search starts at the pair of the trip before and is skipped while that pair lasts
        if (p_wave < 0 || (p_wave + 1 < P && e0 >= seg_off[p_wave + 1]))
            p_wave = __builtin_amdgcn_readfirstlane(mst::segment_of(seg_off, p_wave < 0 ? 0 : p_wave, P, e0));
        const bool one_pair = p_wave + 1 >= P || last < seg_off[p_wave + 1];          // lanes 0 and 63 in one segment
        const int32_t p = one_pair ? p_wave : (active ? mst::segment_of(seg_off, p_wave, P, e) : p_wave);
        const mst_thin_pair mine = table[p];        // p lies in [0, P) whatever seg_off holds
        uint32_t a = 0, b = 0, n = 0;
        if (active) {
            const int64_t c = count_of(count_in[e]);
            const uint32_t x = (uint32_t)xs[e], y = (uint32_t)ys[e];
            a = mine.swap ? y : x;
            b = mine.swap ? x : y;
            bad |= c < 0;
            n = c < 0 ? 0u : (uint32_t)c;
        }
        uint32_t k = 0;
        if (count_out) {                            // wave-uniform: a null pointer sums and checks only
            const bool heavy = (int64_t)n >= mst::kThinHeavy;
            if (!heavy) k = thin_calls(a, b, n, 0, 1, mine.tag, seed, key1, T);
            for (unsigned long long todo = __ballot(heavy); todo; todo &= todo - 1) {
                const int owner = __ffsll((long long)todo) - 1;
                const uint32_t oa = __shfl(a, owner, 64), ob = __shfl(b, owner, 64), on = __shfl(n, owner, 64);
                const uint32_t otag = __shfl(mine.tag, owner, 64);
                const uint32_t got = (uint32_t)wave_sum(thin_calls(oa, ob, on, (uint32_t)lane, 64, otag, seed, key1, T));
                if (lane == owner) k = got;
            }
            if (active) count_out[e] = (int64_t)k;
        }
        if (one_pair) {
            if (p_wave != held) {                   // wave-uniform
                if (lane == 0 && held >= 0) credit(words, held, held_in, held_kept);
                held = p_wave;
                held_in = held_kept = 0;
            }
            held_in += wave_sum(n);
            held_kept += wave_sum(k);
        } else {
            // the pairs of the lanes ascend with the lane: each pair the wave touches gets the sum of exactly its lanes
            for (unsigned long long todo = __ballot(active); todo;) {
                const int32_t q = __shfl(p, __ffsll((long long)todo) - 1, 64);
                const bool in_q = active && p == q;
                const unsigned long long q_in = wave_sum(in_q ? n : 0u), q_kept = wave_sum(in_q ? k : 0u);
                if (lane == 0) credit(words, q, q_in, q_kept);
                todo &= ~__ballot(in_q);
            }
        }
    }
    if (lane == 0 && held >= 0) credit(words, held, held_in, held_kept);
    if (bad) words[2 * (int64_t)P] = 1;             // a flag, not a count: every writer writes the same value
}

}  // namespace

extern "C" int mst_thin_pairs(const int32_t *x, const int32_t *y, const void *count_in, int32_t count_kind, int64_t n_records,
                              const int64_t *seg_off, const mst_thin_pair *table, int32_t n_pairs, uint32_t seed, uint32_t key1,
                              uint64_t T, int64_t *count_out, int64_t *words, int32_t max_blocks, void *stream) {
    if (n_records < 0 || n_pairs < 0 || max_blocks < 0 || !words || count_kind < 0 || count_kind > 2 ||
        (n_records > 0 && (!x || !y || !count_in || !seg_off || !table || n_pairs < 1)) ||
        (count_out && (T < 1 || T > 0xFFFFFFFFull)))
        return mst::fail(MST_E_ARG, "mst_thin_pairs: bad argument");
    if (n_records == 0) return MST_OK;
    const int64_t cap = max_blocks ? max_blocks : kDefaultBlocks;
    const int64_t blocks = (n_records + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
    auto *w = reinterpret_cast<unsigned long long *>(words);
    const uint32_t t32 = (uint32_t)T;
    hipStream_t s = mst::as_stream(stream);
    if (count_kind == MST_THIN_COUNT_I64)
        thin_pairs_kernel<int64_t><<<grid, kThreads, 0, s>>>(x, y, static_cast<const int64_t *>(count_in), n_records, seg_off, table,
                                                            n_pairs, seed, key1, t32, count_out, w);
    else if (count_kind == MST_THIN_COUNT_F32)
        thin_pairs_kernel<float><<<grid, kThreads, 0, s>>>(x, y, static_cast<const float *>(count_in), n_records, seg_off, table,
                                                          n_pairs, seed, key1, t32, count_out, w);
    else
        thin_pairs_kernel<double><<<grid, kThreads, 0, s>>>(x, y, static_cast<const double *>(count_in), n_records, seg_off, table,
                                                           n_pairs, seed, key1, t32, count_out, w);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
