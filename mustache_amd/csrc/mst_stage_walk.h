// Staging of an INNER tile from a diagonal-major band (band[d * n + i] = pixel (i, i + d)): the one walk behind the fused
// kernel's band source (mst_scale_space.hip) and the difference kernel's (mst_diff.hip).  Inner: the CTR x CTC window at
// (Y0, X0) of the block, halo included, lies inside the block, so nothing is reflected.
//
// The window is walked by diagonals: pixels (Y0 + i, X0 + i + dd) of one diagonal are CONTIGUOUS in band row off = X0 - Y0 + dd,
// so a wave reads one run per diagonal and band; wave w takes the diagonals q = w, w + NW, w + 2 NW, ... (dd = q - (CTR - 1)).
// All loads of a round (U diagonals) are issued before the round's first LDS store: the staging is latency bound (every diagonal
// lives in another band row), so memory-level parallelism is what shortens it.
//
// A lane owns tile ROW i = lane + 64 e on every diagonal (not the e-th element of each diagonal), which leaves almost nothing
// to compute per diagonal and lane:
//   column         j = i + dd = jl + NW u: one add.  0 <= j < CTC and the chromosome's end start + X0 + j < n are ONE unsigned
//                  compare of j with a wave-uniform bound (the smaller of the two, 0 on a diagonal outside the band); a lane
//                  whose row lies below the tile (two rows per lane, CTR < 128) starts from a column no step brings into range.
//   band address   the diagonal's row is a wave-uniform 64-bit base that moves by NW n elements per diagonal on the scalar
//                  side; the lane adds its constant 8 i (< 1 KB).  No 32-bit offset holds a multiple of n: (CTR + CTC) * n * 8
//                  passes 2^32 from n = 3.5 million bins (chr1 at 70 bp) and the library sets no such limit on n.
//   LDS address    j * CTP + i = i (CTP + 1) + dd CTP: a lane constant plus a multiple of the step u that is an immediate.
//   tested flag    the region test of row i is lane-constant and folded into the start column jr like the row test above; the
//                  column test is one unsigned compare of jr + NW u; the flag's address is a lane constant plus NW u.
//   fills, band    off = off0 + NW u is wave-uniform: decided on the scalar side, nothing per diagonal is live across the loads.
//
// A wave's last steps can pass the tile's corner (q >= ND): every column of such a diagonal is CTC or beyond, so the column test
// covers it.
//
// put(raw[NB], off, in_tile, cp, in_region, zp) is what a kernel does with one staged element: raw[s] is band s's sample (0.0
// outside the band and past the chromosome's end), off its diagonal (wave-uniform), cp = &ct[j * CTP + i] its place in the
// transposed tile and zp = &nzb[(i - RMAX) * RGC + (j - RMAX)] its place among the region's flags; in_region implies in_tile.
#pragma once
#include <cstdint>

namespace {

// LDS and global pointers with their address space in the type: a value that passes through an empty asm statement (below)
// keeps it, where a generic pointer would come out as a flat one.
using lds_f64 = __attribute__((address_space(3))) double;
using lds_u8 = __attribute__((address_space(3))) uint8_t;
using global_f64 = const __attribute__((address_space(1))) double;

// band: wave-uniform pointers (a caller that selects the band by block makes the selection uniform first).
template <class T, int NB, class Put>
__device__ __forceinline__ void stage_inner_walk(const double *const (&band)[NB], int64_t n, int64_t start, int dpx, int Y0,
                                                 int X0, double *ct, uint8_t *nzb, int tid, Put &&put) {
    constexpr int CTR = T::CTR, CTC = T::CTC, CTP = T::CTP, NW = T::NW, RMAX = T::RMAX, RGR = T::RGR, RGC = T::RGC;
    constexpr int ND = CTR + CTC - 1;
    constexpr int PER = (CTR + 63) / 64;                 // rows per lane
    constexpr int NU = (ND + NW - 1) / NW;               // diagonals per wave
    // 20 samples in flight per lane at most, in two rounds where that is enough.  One round of all 38 diagonals fits the
    // default tile's registers too, and was timed: no faster (LABBOOK R11.1), so the smaller code stays.
    constexpr int CAP = 20 / (NB * PER) > 0 ? 20 / (NB * PER) : 1;
    constexpr int U = (NU + 1) / 2 <= CAP ? (NU + 1) / 2 : CAP;         // diagonals per round: loads first, then the stores
    constexpr int FAR = 1 << 30;                         // a start column that stays out of every range: FAR + NW u > CTC
    static_assert(CTR <= 64 * PER && NW * (NU + U) < FAR / 2, "a lane's rows cover the tile; FAR stays far");

    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    // wave-uniform: the wave's first diagonal, and the columns of the tile that lie before the chromosome's end.  The work
    // item's fields reach the kernel through vector loads; readfirstlane moves what is formed from them to the scalar side ONCE.
    const int dd0 = w - (CTR - 1);
    const int off0 = __builtin_amdgcn_readfirstlane(X0 - Y0) + dd0;
    const int64_t room = n - start - X0;
    const uint32_t cols = (uint32_t)__builtin_amdgcn_readfirstlane(room <= 0 ? 0 : room < CTC ? (int)room : CTC);
    // band element of (row 0, diagonal dd0): dereferenced inside the band only
    const int64_t at_lane = (int64_t)off0 * n + start + Y0;
    const int64_t at0 = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)at_lane >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)at_lane));
    global_f64 *row[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) row[s] = (global_f64 *)(band[s] + at0);
    const int64_t stride = (int64_t)NW * n;              // a wave's successive diagonals are NW band rows apart
    // lane constants: the column of diagonal dd0 for the tile test and for the region test, the two LDS addresses
    int jl[PER], jr[PER];
    lds_f64 *cp[PER];
    lds_u8 *zp[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int i = lane + 64 * e;
        const bool in_rows = i < CTR;
        jl[e] = in_rows ? i + dd0 : FAR;
        jr[e] = in_rows && (uint32_t)(i - RMAX) < (uint32_t)RGR ? i + dd0 - RMAX : FAR;
        cp[e] = (lds_f64 *)ct + ((i + dd0) * CTP + i);
        zp[e] = (lds_u8 *)nzb + ((i - RMAX) * RGC + (i + dd0 - RMAX));
        // opaque from here on: the compiler keeps the address in its register and the step in the store's offset field,
        // where it would otherwise form the address again from the lane number at every store
        asm("" : "+v"(cp[e]), "+v"(zp[e]));
    }
    int off = off0;      // the round's first diagonal
#pragma unroll 1
    for (int u0 = 0; u0 < NU; u0 += U) {
        double raw[NB][U][PER];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int step = NW * u;
            // one scalar select per diagonal; held in a scalar register, so it is not taken apart into lane masks
            uint32_t bound = (uint32_t)(off + step) <= (uint32_t)(dpx + 1) ? cols : 0u;      // inside the band
            asm("" : "+s"(bound));
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const bool on = (uint32_t)(jl[e] + step) < bound;
#pragma unroll
                for (int s = 0; s < NB; ++s) raw[s][u][e] = on ? row[s][lane + 64 * e] : 0.0;
            }
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                row[s] += stride;
                asm("" : "+s"(row[s]));      // one add per diagonal, not U multiples of the stride kept in scalar registers
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int step = NW * u;
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                double r[NB];
#pragma unroll
                for (int s = 0; s < NB; ++s) r[s] = raw[s][u][e];
                // a diagonal past the tile's corner (q >= ND) has every column at CTC or beyond: no test of its own
                put(r, off + step, (uint32_t)(jl[e] + step) < (uint32_t)CTC, (double *)(cp[e] + step * CTP),
                    (uint32_t)(jr[e] + step) < (uint32_t)RGC, (uint8_t *)(zp[e] + step));
            }
        }
        off += NW * U;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            jl[e] += NW * U;
            jr[e] += NW * U;
            cp[e] += NW * U * CTP;
            zp[e] += NW * U;
            asm("" : "+v"(cp[e]), "+v"(zp[e]));      // moved once per round, not re-formed from a round offset at every store
        }
    }
}

}  // namespace
