// Trans read pairs -> per-pair pixels on the device, all chromosome pairs of the genome in one pass (mustache_amd/pairs.py states
// the rule; include/mustache_hip.h the entry points).
//
// The rows arrive pair-major: pair p = (a, b), a < b in table order, owns rows [seg_off[p], seg_off[p + 1]), the position on a in
// posA and the position on b in posB.  A pixel's key is cell_off[p] + x * n_b + y (x = bin on a, y = bin on b; cell_off = the
// running sum of n_a * n_b over the pairs before p): unique across pairs, and ascending keys are pair-major.
//
//   mst_pairs_bin_trans      one grid-stride pass over the rows.  The kernel holds the trans rule alone: each lane finds its row's
//                            pair (wave-uniform when lanes 0 and 63 lie in one segment, a per-lane binary search of seg_off
//                            otherwise), bins its row or marks it dropped (counted per pair); the key is the cell, its counter
//                            dense[key] when key < dense_cells, the far list otherwise.  The run merge, the head lane's add and
//                            the far list with its one reservation per workgroup and trip are the shared trip body
//                            (mst_pairs_tiles.h), as in mst_pairs_bin.
//   mst_pairs_trans_compact  the non-zero counters -> (key, count) in ascending key order: the shared compaction with the
//                            emitter that writes the index as the key.  No atomics.
//   mst_pairs_trans_decode   ascending keys + int64 counts -> (x int32, y int32, v float64): a binary search of cell_off per key.
//
// Every sum is an integer sum: the counters, the far list as a multiset and the dropped counts are the same from run to run and
// under any order of the rows within their pairs.
#include "mst_pairs_tiles.h"

namespace {

__global__ __launch_bounds__(kThreads) void
pairs_bin_trans_kernel(const int32_t *__restrict__ posA, const int32_t *__restrict__ posB, int64_t N,
                       const int64_t *__restrict__ seg_off, int32_t P, const int64_t *__restrict__ limA,
                       const int64_t *__restrict__ limB, const int64_t *__restrict__ nA, const int64_t *__restrict__ nB,
                       const int64_t *__restrict__ cell_off, int32_t res, int32_t zero_based, int64_t dense_cells,
                       uint32_t *__restrict__ dense, int64_t *__restrict__ far_key, uint32_t *__restrict__ far_mult,
                       int64_t far_cap, unsigned long long *__restrict__ n_far_out, unsigned long long *__restrict__ dropped) {
    __shared__ BinSlots slots;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
    const int32_t lo = zero_based ? 0 : 1;
    int32_t p_wave = 0;                             // wave-uniform: the pair of the wave's first row; rows only go forward
    int parity = 0;
    // the trip count is the same for every wave of a workgroup (bin_far's barriers need that) and for every lane of a wave (the
    // shuffles and ballots do); `base < N` and `e0 < N` guard the loads only
    for (int64_t block_base = (int64_t)blockIdx.x * kRowsPerBlock; block_base < N; block_base += stride, parity ^= 1) {
        const int64_t base = block_base + (int64_t)wave * (64 * kUnroll);
        BinTrip t;
        if (base < N) p_wave = __builtin_amdgcn_readfirstlane(mst::segment_of(seg_off, p_wave, P, base));
        int32_t p_group = p_wave;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t e0 = base + u * 64, e = e0 + lane;
            const bool active = e < N;
            bool ok = false;
            long long cell = 0;
            if (e0 < N) {                           // wave-uniform
                const int64_t last = e0 + 63 < N ? e0 + 63 : N - 1;
                p_group = __builtin_amdgcn_readfirstlane(mst::segment_of(seg_off, p_group, P, e0));
                const bool one_pair = p_group + 1 >= P || last < seg_off[p_group + 1];       // lanes 0 and 63 in one segment
                const int32_t p = one_pair ? p_group : (active ? mst::segment_of(seg_off, p_group, P, e) : p_group);
                if (active) {
                    const int32_t a = posA[e], b = posB[e];
                    const int64_t la = limA[p], lb = limB[p], na = nA[p], nb = nB[p];
                    ok = a >= lo && b >= lo && (zero_based ? ((int64_t)a < la && (int64_t)b < lb)
                                                           : ((int64_t)a <= la && (int64_t)b <= lb));
                    if (ok) {
                        const int64_t x = (a - lo) / res, y = (b - lo) / res;
                        cell = cell_off[p] + x * nb + y;
                        // never a key outside the pair's cells, whatever limits the caller gave; a table with a negative
                        // entry: dropped, not written
                        ok = x < na && y < nb && cell >= 0;
                    }
                }
                if (one_pair) {
                    const uint32_t lost = (uint32_t)__popcll(__ballot(active && !ok));
                    if (lost && lane == 0) atomicAdd(&dropped[p_group], (unsigned long long)lost);
                } else if (active && !ok) {
                    atomicAdd(&dropped[p], 1ull);
                }
            }
            bin_group(t, u, active, ok, cell, cell < dense_cells, cell, dense);
        }
        bin_far<true>(t, slots, parity, far_key, far_mult, far_cap, n_far_out);
    }
}

struct EmitKey {                                    // a counter's index is its key
    int64_t *key;
    uint32_t *count;
    __device__ void seek(int64_t) {}
    __device__ void operator()(int64_t o, int64_t index, uint32_t c) {
        key[o] = index;
        count[o] = c;
    }
};

__global__ __launch_bounds__(kThreads) void
trans_decode_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ counts, int64_t N,
                    const int64_t *__restrict__ cell_off, const int64_t *__restrict__ nB, int32_t P, int32_t *__restrict__ out_x,
                    int32_t *__restrict__ out_y, double *__restrict__ out_v) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += stride) {
        const int64_t key = keys[i];
        const int32_t p = mst::segment_of(cell_off, 0, P, key);
        const int64_t cell = key - cell_off[p], nb = nB[p], x = cell / nb;
        out_x[i] = (int32_t)x;
        out_y[i] = (int32_t)(cell - x * nb);
        out_v[i] = (double)counts[i];               // int64 -> float64 directly: exact below 2^53
    }
}

}  // namespace

extern "C" int mst_pairs_bin_trans(const int32_t *posA, const int32_t *posB, int64_t n_rows, const int64_t *seg_off, int32_t n_pairs,
                                   const int64_t *limA, const int64_t *limB, const int64_t *nA, const int64_t *nB,
                                   const int64_t *cell_off, int32_t res, int32_t zero_based, int64_t dense_cells, uint32_t *dense,
                                   int64_t *far_key, uint32_t *far_mult, int64_t far_cap, uint64_t *n_far, uint64_t *dropped,
                                   void *stream) {
    if (n_rows < 0 || n_pairs < 0 || res < 1 || dense_cells < 0 || far_cap < 0) return mst::fail(MST_E_ARG, "mst_pairs_bin_trans: bad argument");
    if (n_rows == 0 || n_pairs == 0) return MST_OK;
    if (!posA || !posB || !seg_off || !limA || !limB || !nA || !nB || !cell_off || !n_far || !dropped || (dense_cells > 0 && !dense) ||
        (far_cap > 0 && (!far_key || !far_mult)))
        return mst::fail(MST_E_ARG, "mst_pairs_bin_trans: bad argument");
    // at most 2048 workgroups: 32 waves for each of 256 compute units, each workgroup on trips of 2048 rows
    pairs_bin_trans_kernel<<<grid_for(n_rows, kRowsPerBlock, 2048), kThreads, 0, mst::as_stream(stream)>>>(
        posA, posB, n_rows, seg_off, n_pairs, limA, limB, nA, nB, cell_off, res, zero_based, dense_cells, dense, far_key, far_mult,
        far_cap, reinterpret_cast<unsigned long long *>(n_far), reinterpret_cast<unsigned long long *>(dropped));
    MST_LAUNCH_CHECK();
    return MST_OK;
}

extern "C" uint64_t mst_pairs_trans_compact_workspace_bytes(int64_t dense_cells) {
    return dense_cells < 0 ? 0 : compact_workspace_bytes(dense_cells);
}

extern "C" int mst_pairs_trans_compact(const uint32_t *dense, int64_t dense_cells, int64_t *out_key, uint32_t *out_count, int64_t cap,
                                       int64_t *n_out, void *workspace, uint64_t workspace_bytes, void *stream) {
    return compact_counters("mst_pairs_trans_compact", dense, dense_cells, EmitKey{out_key, out_count}, out_key && out_count, cap,
                            n_out, workspace, workspace_bytes, stream);
}

extern "C" int mst_pairs_trans_decode(const int64_t *keys, const int64_t *counts, int64_t n, const int64_t *cell_off, const int64_t *nB,
                                      int32_t n_pairs, int32_t *out_x, int32_t *out_y, double *out_v, void *stream) {
    if (n < 0 || n_pairs < 0) return mst::fail(MST_E_ARG, "mst_pairs_trans_decode: bad argument");
    if (n == 0) return MST_OK;
    if (n_pairs == 0 || !keys || !counts || !cell_off || !nB || !out_x || !out_y || !out_v)
        return mst::fail(MST_E_ARG, "mst_pairs_trans_decode: bad argument");
    trans_decode_kernel<<<grid_for(n, kThreads, 8192), kThreads, 0, mst::as_stream(stream)>>>(keys, counts, n, cell_off, nB, n_pairs,
                                                                                               out_x, out_y, out_v);
    MST_LAUNCH_CHECK();
    return MST_OK;
}
