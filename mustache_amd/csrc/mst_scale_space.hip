// Fused sigma-stack kernel for gfx950 (MI355X):  reference mustache/mustache.py:714-772 in ONE launch.
//
// What the reference does per dense block (CH x CH float64), through SciPy:
//   for each octave o in {1.6, 3.2}:  G_k = gaussian_filter(c, sigma_k), k = 1..12   (:719, :725, :734, :751)
//                                     D_k = G_k - G_{k+1}, k = 1..11                 (:728, :738, :754)
//                                     M_k = maximum_filter(D_k, 3x3, zero padded)    (:740-743, :757-758)
//     for each tested level c = 2..10: on the nz pixels
//         loc/scale of |D_c| (expon.fit, :755), and the sieve (:760-768)
//         upd = D_c > best  &  D_c == M_c  &  (D_p == M_p | D_n == M_n)  &  D_c > M_p  &  D_c > M_n
// 24 full-image blurs, 22 DoG images, 22 max images, ~10 boolean gathers per level: ~600 B of HBM traffic per
// pixel if every level is materialised.
//
// What this kernel does instead: one 256-thread workgroup owns a 30 x 62 pixel tile (a 32 x 64 "region" with the
// 1-pixel ring the 3x3 max needs).  It loads the tile of c with a 14-pixel reflect halo into LDS ONCE (~15 B/pixel
// of HBM/L2 reads), then walks all 24 levels out of LDS:
//   V pass  (axis 0): a thread produces 8 vertically consecutive samples of one column from a register window of
//                     8+2r samples (c tile stored transposed -> the window is contiguous, read as ds_read_b128;
//                     lanes run along columns with a pitch of 30 mod 32 doubles -> the main items' loads are
//                     conflict-free; the 4-row pieces of the halo columns are not, see pitch_for in mst_fir.h).
//                     At odd RMAX - r the window starts on an odd row: fir_chunk then loads the aligned pairs
//                     around it and keeps the compiler from re-cutting them into ds_read2_b64 (mst_fir.h);
//                     result -> LDS vb
//   H pass  (axis 1): a thread produces 8 horizontally consecutive samples of one row (same access pattern on vb),
//                     result stays in registers
//   DoG in registers; zero-padded 3x3 max = horizontal 3-max in registers (2 edge samples through a 4 KB LDS strip)
//   then vertical 3-max across lanes with DPP wave shifts (lanes of a wave are consecutive rows); the 5-term sieve
//   and the running best/level per pixel live in registers across all levels and both octaves; per-level min / sum
//   of |D_c| are reduced per workgroup in a fixed order.
//   Per-pixel state carried from level to level: G, D, ONE set of maxima, best, level.  The level loop cannot be unrolled, so
//   G and D are renamed once per level (2 K register-pair copies); nothing else is copied: the maxima are overwritten in
//   place between the sieve's two comparisons, and the radius switch has no path without a case, so the axis-1 pass
//   accumulates straight into G (scripts/isa_census.py --state-copies, tests/test_level_state_copies.py).
// Only the found pixels (~1 % of the block) and 2 x 18 partial statistics per tile are written back.
// Outside the level loop (scripts/isa_census.py prints it by path; tests/test_outside_loop_census.py bounds it):
//   staging of an inner tile from the band: the diagonal walk of mst_stage_walk.h (shared with mst_diff.hip).  A lane owns a tile
//     row on every diagonal, so a diagonal costs a lane one add and one compare per load and the stores' addresses are lane
//     constants plus an immediate; the band row, the fills and the tested rule are wave-uniform and live on the scalar side.
//   statistics: the slots of st start at {inf, 0}; only a wave that owns a tested pixel writes its slots.
//   epilogue: a workgroup without a tested pixel (61 % of a dense launch) writes the identity statistics and leaves -- no
//     ballot, no barrier.  A tested one exchanges its waves' record totals ONCE (one barrier; ct is dead by then); every wave
//     forms its own prefix and the total from them, one lane reserves the slots in both blocks, and the statistics are folded
//     while that atomic is under way.  Nothing found: no second barrier, no record loop.  A wave without records leaves
//     behind the second barrier.
// 77 KB of LDS per workgroup -> two independent workgroups per CU, so one's LDS window loads overlap the other's
// FP64 work instead of every wave of the CU alternating between the two in barrier lock-step.
// The kernel is FP64-VALU bound (~1150 non-fusable flops per pixel for the blurs alone), not HBM bound.
// Tiles sit on a lattice anchored at the chromosome's origin, and a tile that lies inside two consecutive (overlapping) blocks of
// a launch with its whole blur halo is computed once for both (struct WorkItem, build_items): the reference's blocks overlap by
// up to half their edge (mustache.py:899-908) and recompute those pixels block by block.
//
// Bit-exactness: the tap order is SciPy's C correlate1d on a symmetric kernel,
//     t = x[c]*w0;  for j = r..1:  t += (x[c-j] + x[c+j]) * w[j]
// axis 0 first, float64 intermediate, mode='reflect'; compiled with -ffp-contract=off so no FMA is formed.
// The taps themselves come from the host (NumPy), see mustache_amd/levels.py.
// Build flags for this file add -fno-honor-nans -mno-amdgpu-ieee: inputs are finite (checked through the level
// statistics), and with IEEE mode off v_max_f64 needs no canonicalising pre-pass; no value-changing fast-math
// flag (reassociation, contraction, reciprocal) is enabled.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>
#include "mst_common.h"

#include "mst_fir.h"
#include "mst_stage_walk.h"

namespace {

__device__ __forceinline__ double dmax(double a, double b) { return __builtin_fmax(a, b); }

// One of the sieve's two per-level comparisons for four pixels, shifted into a bit word: GT ? d > p : d == p.
// v_addc_co_u32 w, w, w computes 2 w + carry, so each compare result enters its word with ONE instruction and
// never exists as a 0 / 1 << k select that an or then merges.  After K pixels pixel k sits at bit K - 1 - k.
// The compiler neither schedules nor pads the inside of an asm statement: a lane mask written by a VALU compare needs two
// wait states before a VALU instruction reads it (as carry-in here), and the order below leaves two instructions between
// every compare and the add that consumes it -- three mask registers in rotation, no s_nop.  FIRST starts the word from 0.
// One kind of comparison per statement, not both: the level loop takes d > M_prev BEFORE it forms the new maxima and
// d == M_new behind them, so the new maxima are written over the previous level's and the state holds ONE set of them.
template <bool GT, bool FIRST>
__device__ __forceinline__ void sieve_bits4(uint32_t &w, double d0, double p0, double d1, double p1, double d2, double p2,
                                            double d3, double p3) {
    unsigned long long y, z;      // lane-mask temporaries (SGPR pairs)
#define MST_SIEVE4(CMP_, ADD0_, W_)                        \
    asm("v_cmp_" CMP_ "_f64 vcc, %3, %4\n\t"               \
        "v_cmp_" CMP_ "_f64 %1, %5, %6\n\t"                \
        "v_cmp_" CMP_ "_f64 %2, %7, %8\n\t"                \
        "v_addc_co_u32 %0, vcc, " ADD0_ ", vcc\n\t"        \
        "v_cmp_" CMP_ "_f64 vcc, %9, %10\n\t"              \
        "v_addc_co_u32 %0, %1, %0, %0, %1\n\t"            \
        "v_addc_co_u32 %0, %2, %0, %0, %2\n\t"            \
        "v_addc_co_u32 %0, vcc, %0, %0, vcc"               \
        : W_(w), "=&s"(y), "=&s"(z)                        \
        : "v"(d0), "v"(p0), "v"(d1), "v"(p1), "v"(d2), "v"(p2), "v"(d3), "v"(p3) \
        : "vcc")
    if constexpr (GT && FIRST) MST_SIEVE4("gt", "0, 0", "=&v");
    else if constexpr (GT) MST_SIEVE4("gt", "%0, %0", "+v");
    else if constexpr (FIRST) MST_SIEVE4("eq", "0, 0", "=&v");
    else MST_SIEVE4("eq", "%0, %0", "+v");
#undef MST_SIEVE4
}

// d > t on the lanes whose top bit of `bits` is set; `bits` moves up by one, so the next call tests the next bit.
// v_add_co_u32 bits, bits, bits shifts the word and delivers the bit shifted out as the carry's lane mask: the gate of a
// pixel costs ONE vector instruction and a scalar and, where a bit test costs two and an or.  The mask the statement
// returns was last written by the scalar unit, so the selects that read it need no wait states.
__device__ __forceinline__ bool gated_greater(uint32_t &bits, double d, double t) {
    unsigned long long mask;
    asm("v_add_co_u32 %0, vcc, %0, %0\n\t"
        "v_cmp_gt_f64 %1, %2, %3\n\t"
        "s_and_b64 %1, %1, vcc"
        : "+v"(bits), "=&s"(mask)
        : "v"(d), "v"(t)
        : "vcc", "scc");      // s_and_b64 writes SCC: no scalar compare may be kept live across the statement
    return __builtin_amdgcn_inverse_ballot_w64(mask);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant expression
template <int... I, class F>
__device__ __forceinline__ void for_each_index(std::integer_sequence<int, I...>, F &&f) {
    (f(std::integral_constant<int, I>()), ...);
}

// value held by the previous / next lane: DPP wave shifts, no LDS traffic.  bound_ctrl is set, so the lane without a
// source (0 for prev, 63 for next) reads 0.0 and no `old` operand has to be copied in first; those lanes hold ring
// rows whose maxima are never used.
__device__ __forceinline__ double lane_prev(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x138, 0xf, 0xf, true);   // wave_shr:1
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_next(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x130, 0xf, 0xf, true);   // wave_shl:1
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// 64-lane reductions with DPP moves only (no LDS round trips): inclusive scans inside the four 16-lane rows
// (row_shr 1, 2, 4, 8), then row_bcast15 / row_bcast31 carry the row totals upward; lane 63 ends up with the total.
// The combination order is fixed, so the result is deterministic.  ONLY lane 63 is meaningful afterwards: the lanes a
// shift or a row mask leaves without a source are not given an identity value (that costs four extra moves per step) --
// they read 0 / keep an unspecified register, and none of them lies on the path into lane 63 (lane 15 of a row combines
// lanes 14, 13, 11, 7 after steps 1, 2, 4, 8, each of which only ever read lanes with a valid source; the broadcasts
// read lanes 15 / 47 and 31).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_fetch(double x) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, ROW_MASK, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void wave_reduce_min_sum(double &mn, double &sm) {
#define MST_STEP(CTRL, MASK)                                           \
    {                                                                  \
        const double a_ = dpp_fetch<CTRL, MASK>(mn);                   \
        const double b_ = dpp_fetch<CTRL, MASK>(sm);                   \
        mn = a_ < mn ? a_ : mn;                                        \
        sm = sm + b_;                                                  \
    }
    MST_STEP(0x111, 0xf)   // row_shr:1
    MST_STEP(0x112, 0xf)   // row_shr:2
    MST_STEP(0x114, 0xf)   // row_shr:4
    MST_STEP(0x118, 0xf)   // row_shr:8
    MST_STEP(0x142, 0xa)   // row_bcast:15 -> rows 1 and 3
    MST_STEP(0x143, 0xc)   // row_bcast:31 -> rows 2 and 3
#undef MST_STEP
}

// K output samples from a register window of K + 2R input samples, SciPy's order per sample:
//     t = x[c]*w0;  for j = R..1:  t += (x[c-j] + x[c+j]) * w[j]
// The K accumulation chains are independent; the loops are written tap-major so the K adds / muls / adds of one
// tap are adjacent in program order and the FP64 pipe always has K independent instructions to issue (a
// sample-major order leaves one serial add->mul->add chain per sample and stalls on every instruction).
template <class T, int R>
__device__ __forceinline__ void blur_level(const double *ct, double *vb, const double (&w)[T::RMAX + 1], int tid,
                                           const double *vsrc, double *vdst, const double *hsrc, double (&g)[T::K],
                                           int variant, unsigned long long *tr MST_INJECT_ARG) {
    vpass<T, R>(ct, vb, w, tid, vsrc, vdst, variant MST_INJECT_PASS);
    MST_STAMP(tr, 1)
    __syncthreads();
    MST_STAMP(tr, 2)
    if (MST_VARIANT(32)) {              // [ablation 32] axis-0 pass only (with 24 = the other half: the "roles" experiment)
#pragma unroll
        for (int k = 0; k < T::K; ++k) g[k] = 0.0;
        return;
    }
    hpass<T, R>(hsrc, w, g);
    MST_STAMP(tr, 3)
}

template <class T>
__device__ __forceinline__ void blur_dispatch(int r, const double *ct, double *vb, const double (&wg)[T::RMAX + 1],
                                              int tid, const double *vsrc, double *vdst, const double *hsrc,
                                              double (&g)[T::K], int variant, unsigned long long *tr MST_INJECT_ARG) {
    // Every path through the switch runs a case: radii above T::RMAX and outside [1, 28] are UNREACHABLE, not empty.  With an
    // empty path `g` may leave the switch unwritten, and the compiler then keeps the axis-1 accumulators in registers of their
    // own and copies them into g behind the join -- K v_mov_b64 per thread and level.  The host cannot get there: check_levels
    // refuses a table with a radius outside [1, 28]; with_tile and build_list choose the tile from the table's largest radius
    // (default tile up to 14, the wide one up to 28); MST_FLAG_FMA, whose tile stops at 14, is refused above that; and
    // enqueue_launch checks the chosen tile's RMAX against the table once more before anything is launched.
#define MST_CASE(R_)                                                  \
    case R_:                                                          \
        if constexpr (R_ <= T::RMAX) blur_level<T, R_>(ct, vb, wg, tid, vsrc, vdst, hsrc, g, variant, tr MST_INJECT_PASS); \
        else __builtin_unreachable();                                 \
        break;
    switch (r) {
        MST_CASE(1) MST_CASE(2) MST_CASE(3) MST_CASE(4) MST_CASE(5) MST_CASE(6) MST_CASE(7)
        MST_CASE(8) MST_CASE(9) MST_CASE(10) MST_CASE(11) MST_CASE(12) MST_CASE(13) MST_CASE(14)
        MST_CASE(15) MST_CASE(16) MST_CASE(17) MST_CASE(18) MST_CASE(19) MST_CASE(20) MST_CASE(21)
        MST_CASE(22) MST_CASE(23) MST_CASE(24) MST_CASE(25) MST_CASE(26) MST_CASE(27) MST_CASE(28)
        default: __builtin_unreachable();
    }
#undef MST_CASE
}

// Where the block pixels come from.  Dense: caller-built filled blocks + nz masks (the reference's `c`).  Band: straight from
// the chromosome's diagonal-major band -- the fills of mustache.py:703-706 and the nz rule of :699 are applied while the
// tile is staged, so dense blocks are never materialised (no 9 B/pixel write + re-read, no 18 GB for chr1 @ 1 kb).
struct BandSrc {
    const double *band;        // band[d * n + i] = pixel (i, i + d)
    int64_t n;
    int dpx;
    const int64_t *starts;     // dev [B]: block origins
    uint32_t *nz_count;        // dev [B]: out, number of tested pixels per block
    const double *band2;       // two-sample launches: blocks [split, B) are windows of this band (same n, dpx); else unused
    int split;                 // first block of band2 (INT_MAX: one band)
};

// One workgroup's job: the tile whose region (interior + ring) starts at (y0, x0) of block b.  Consecutive blocks of a
// chromosome overlap by half their edge (mustache.py:899-908), and a Gaussian level at a pixel depends on c within its blur
// radius only: a tile that lies inside BOTH blocks, halo included, sees the same c values, fills and tested pixels in either
// -- its DoG values, maxima, sieve decisions and statistics are the same bits.  Such a tile is computed ONCE (for block b) and
// its found records, tested-pixel count and level statistics are delivered to block b2 as well (pixel indices shifted by
// delta2 = start_b - start_b2 along both axes); b2 < 0: the tile belongs to one block only.  The host builds the list
// (build_items): tiles sit on a lattice anchored at chromosome coordinate 0, so that overlapping blocks cut the same tiles.
struct WorkItem {
    int32_t y0, x0, b, delta2;      // delta2 != 0: also delivered to block b + 1 (delta2 = start_b - start_{b+1} < 0)
};

// The kernel's argument block as the hardware lays it out (each argument at its natural alignment, in order): the wide-radius
// instantiation re-reads the arguments only its EPILOGUE needs from there, so that they do not occupy scalar registers through
// the level loop (29 taps of two registers each leave none to spare; the default tile is untouched).
struct KernArgs {
    const double *c;
    const uint8_t *nz;
    BandSrc src;
    int CH;
    const DevLevels *lv;
    mst_found *found;
    uint32_t found_cap;
    uint32_t *found_count;
    double *partial;
    const WorkItem *items;
    int n_items, n_tested, skip_empty, variant;
    unsigned long long *trace;
};

template <class T, bool BAND>
__global__ void __launch_bounds__(T::NT, T::MINW)
scale_space_kernel(const double *__restrict__ c, const uint8_t *__restrict__ nz, BandSrc src, int CH,
                   const DevLevels *__restrict__ lv, mst_found *__restrict__ found, uint32_t found_cap,
                   uint32_t *__restrict__ found_count, double *__restrict__ partial, const WorkItem *__restrict__ items,
                   int n_items, int n_tested, int skip_empty, int variant, unsigned long long *__restrict__ trace) {
    constexpr int K = T::K, RGR = T::RGR, RGC = T::RGC, RMAX = T::RMAX;
    extern __shared__ __align__(16) double lds[];
    double *ct = lds;
    double *vb = ct + T::CT_ELEMS;
    double *de = vb + T::VB_ELEMS;
    double *st = de + T::DE_ELEMS;

    const int tid = threadIdx.x;
    // XCD-aware order: hardware places workgroup i on XCD i % 8 (gridDim.x is a multiple of 8), so give each XCD a
    // contiguous run of the item list -- neighbouring tiles share their halo through that XCD's L2.  The host orders the list
    // so that every XCD's run holds the same mix of work (build_items).
    const int per_xcd = gridDim.x >> 3;
    const int slot = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (slot >= n_items) return;
    const WorkItem item = items[slot];
    const int b = item.b, b2 = item.delta2 != 0 ? item.b + 1 : -1;
    const int y0 = item.y0, x0 = item.x0;  // block coordinates of region (0, 0)

    const int rr = tid % RGR;  // region row owned in the H pass; consecutive lanes = consecutive rows
    const int cg = tid / RGR;  // column group
    const int gy = y0 + rr;
    const bool row_in = gy >= 0 && gy < CH;
    const bool row_own = row_in && rr >= 1 && rr <= T::ITR;
    double *part = partial + (size_t)slot * n_tested * 2;

    uint32_t in_mask = 0, nz_mask = 0;  // per-k bits: column inside the block / tested pixel owned by this thread
    int any_nz;                         // some thread of the workgroup owns a tested pixel (workgroup-uniform)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int gx = x0 + cg * K + k;
        if (row_in && gx >= 0 && gx < CH) in_mask |= 1u << k;
    }

    if constexpr (!BAND) {
        const double *cb = c + (size_t)b * CH * CH;
        const uint8_t *nb = nz + (size_t)b * CH * CH;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int rc = cg * K + k;
            const int gx = x0 + rc;
            if (row_own && gx >= 0 && gx < CH && rc >= 1 && rc <= T::ITC && nb[(size_t)gy * CH + gx]) nz_mask |= 1u << k;
        }
        any_nz = __syncthreads_or(nz_mask != 0);
        if (!any_nz && skip_empty) {
            for (int t = tid; t < n_tested; t += T::NT) {
                part[2 * t] = INFINITY;
                part[2 * t + 1] = 0.0;
            }
            return;
        }
        // ---- stage the c tile (reflect halo) in LDS, transposed: the only bulk HBM/L2 read of the kernel.
        // A wave takes whole rows (row reflection is wave-uniform); each lane's column reflections are computed once.
        constexpr int CPL = (T::CTC + 63) / 64;          // columns per lane
        int sx[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) sx[q] = reflect_idx(x0 - RMAX + (tid & 63) + 64 * q, CH);
        for (int i = tid >> 6; i < T::CTR; i += T::NW) {
            const double *srow = cb + (size_t)reflect_idx(y0 - RMAX + i, CH) * CH;
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int j = (tid & 63) + 64 * q;
                if (j < T::CTC) ct[j * T::CTP + i] = srow[sx[q]];
            }
        }
        __syncthreads();
    } else {
        // ---- band source.  Pixel (by, bx) of the block: off = bx - by;
        //   raw    = band[off][start + by]            for 0 <= off <= dpx+1 and start + bx < n, else 0
        //   tested = raw != 0 and off >= 4            (mustache.py:699, before the fills)
        //   value  = 2 where off <= 4 or off >= dpx+1 (mustache.py:703-706), else raw
        const int64_t start = src.starts[b];
        const int64_t n = src.n;
        const int dpx = src.dpx;
        const double *const bandp = b >= src.split ? src.band2 : src.band;       // (workgroup-uniform)
        uint8_t *nzb = reinterpret_cast<uint8_t *>(vb);      // [RGR][RGC] tested flags of the region; vb is free until the V pass
        const int Y0 = y0 - RMAX, X0 = x0 - RMAX;
        const bool inner = Y0 >= 0 && X0 >= 0 && Y0 + T::CTR <= CH && X0 + T::CTC <= CH;   // no reflection in this tile
        // the tile incl. its halo lies entirely in one of the constant regions, col - row <= 3 or >= dpx + 2 (diagonals 4 and
        // dpx + 1 are filled too, but their pixels can be TESTED, mustache.py:699 vs :703-706): every sample is the fill
        // value and no pixel is tested -- the same LDS contents as the general walk below, written with wide stores
        const bool constant = inner && (X0 + T::CTC - 1 - Y0 <= 3 || X0 - (Y0 + T::CTR - 1) >= dpx + 2);
        if (constant) {
            double2 *ct2 = reinterpret_cast<double2 *>(ct);
            for (int i = tid; i < T::CT_ELEMS / 2; i += T::NT) ct2[i] = make_double2(2.0, 2.0);
            uint4 *nz4 = reinterpret_cast<uint4 *>(nzb);
            static_assert((RGR * RGC) % 16 == 0, "nzb is cleared in 16-byte pieces");
            for (int i = tid; i < RGR * RGC / 16; i += T::NT) nz4[i] = make_uint4(0, 0, 0, 0);
        } else if (inner) {
            // one diagonal walk for every band source (mst_stage_walk.h): a lane owns a tile row, the fills and the tested rule
            // are wave-uniform per diagonal
            const double *const bands[1] = {__builtin_amdgcn_readfirstlane(b >= src.split) ? src.band2 : src.band};
            stage_inner_walk<T, 1>(bands, n, start, dpx, Y0, X0, ct, nzb, tid,
                                   [&](const double (&raw)[1], int off, bool in_tile, double *cp, bool in_region, uint8_t *zp)
                                       __attribute__((always_inline)) {
                                           if (in_tile) *cp = (off <= 4 || off >= dpx + 1) ? 2.0 : raw[0];
                                           if (in_region) *zp = (raw[0] != 0.0 && off >= 4) ? 1 : 0;
                                       });
        } else {
            // border tiles: element-wise with reflection (few tiles; loads are served by L2)
            for (int idx = tid; idx < T::CTR * T::CTC; idx += T::NT) {
                const int i = idx / T::CTC, j = idx - i * T::CTC;
                const int uy = Y0 + i, ux = X0 + j;                       // unreflected block coordinates
                const int by = reflect_idx(uy, CH), bx = reflect_idx(ux, CH);
                const int off = bx - by;
                double raw = 0.0;
                if (off >= 0 && off <= dpx + 1 && start + bx < n) raw = bandp[(int64_t)off * n + start + by];
                ct[j * T::CTP + i] = (off <= 4 || off >= dpx + 1) ? 2.0 : raw;
                const int ri = i - RMAX, rj = j - RMAX;
                if (ri >= 0 && ri < RGR && rj >= 0 && rj < RGC) {
                    const bool inside = uy >= 0 && uy < CH && ux >= 0 && ux < CH;
                    nzb[ri * RGC + rj] = (inside && raw != 0.0 && off >= 4) ? 1 : 0;
                }
            }
        }
        __syncthreads();
        uint32_t mine = 0;
        // The thread's K flags are K consecutive bytes at a multiple of K: read as words.  A flag byte is 0 or 1, and
        // w * 0x204081 puts bytes 0 .. 3 of w side by side at bits 21 .. 24 (every partial product lands on a bit of its own,
        // so nothing carries).  Owned columns are region columns 1 .. ITC: the first group drops its first, the last its last.
        static_assert(K % 4 == 0 && (RGC & 3) == 0 && T::ITC == RGC - 2, "flag bytes are gathered four at a time");
        uint32_t flag_bits = 0;
#pragma unroll
        for (int w = 0; w < K / 4; ++w) {
            const uint32_t four = reinterpret_cast<const uint32_t *>(nzb)[(rr * RGC + cg * K) / 4 + w];
            flag_bits |= (((four * 0x00204081u) >> 21) & 0xFu) << (4 * w);
        }
        constexpr uint32_t ALLK = (1u << K) - 1u;
        const uint32_t col_mask = cg == 0 ? ALLK & ~1u : cg == T::NCG - 1 ? ALLK >> 1 : ALLK;
        nz_mask = row_own ? flag_bits & in_mask & col_mask : 0u;
        // the wave's count from K ballots, in scalar registers (integer: exact in any order)
#pragma unroll
        for (int k = 0; k < K; ++k) mine += (uint32_t)__builtin_popcountll(__ballot((nz_mask >> k) & 1u));
        if ((tid & 63) == 0 && mine) {                                         // integer: exact in any order
            atomicAdd(src.nz_count + b, mine);
            if (b2 >= 0) atomicAdd(src.nz_count + b2, mine);
        }
        any_nz = __syncthreads_or(nz_mask != 0);                            // also fences nzb reads before vb is reused
        if (!any_nz && skip_empty) {
            for (int t = tid; t < n_tested; t += T::NT) {
                part[2 * t] = INFINITY;
                part[2 * t + 1] = 0.0;
            }
            return;
        }
    }

    // per-pixel rolling state across levels.  For the tested level c the sieve needs
    //   D_c == M_c (ec),  D_{c-1} == M_{c-1} (ep),  D_c > M_{c-1} (gp),  and against the incoming level D_c > M_{c+1};
    // the first three are decided when their level arrives and kept as one bit per pixel.
    double gprev[K], Dc[K], Mc[K], best[K];
    uint32_t lvl[K];
    uint32_t ep = 0, ec = 0, gp = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        gprev[k] = Dc[k] = Mc[k] = 0.0;
        best[k] = ((nz_mask >> k) & 1u) ? 0.0 : INFINITY;   // never tested: no D_c exceeds it, lvl stays 0 and best is never written out
        lvl[k] = 0;
    }
    const int wave = tid >> 6, lane = tid & 63;
    const bool wave_has_nz = __any(nz_mask != 0);
    // the statistics slots start at the identities {inf, 0}: only a wave that owns a tested pixel writes its slots in the level
    // loop, and a workgroup without any never reads them (the epilogue's short path).  The level loop's barriers lie between
    // these stores and the first slot a wave writes.
    // Not in the wide tile: there the store inside the branch costs a scalar spill in the level loop, so every wave writes its
    // slot at every tested level as before, and nothing has to be initialised.
    constexpr bool ST_ONCE = T::RMAX <= 14;
    if (ST_ONCE && any_nz)
        for (int i = tid; i < n_tested * T::NW; i += T::NT) {
            st[2 * i] = INFINITY;
            st[2 * i + 1] = 0.0;
        }
    const bool wave_all_in = __all(in_mask == (1u << K) - 1u);   // no pixel of this wave lies outside the block
    double *de_mine = de + (cg * 2) * RGR + rr;                                   // [cg][0 = left edge, 1 = right edge][rr]
    const double *de_left = de + ((cg > 0 ? cg - 1 : 0) * 2 + 1) * RGR + rr;      // left neighbour's right edge
    const double *de_right = de + ((cg < T::NCG - 1 ? cg + 1 : cg) * 2) * RGR + rr;  // right neighbour's left edge

    // thread-constant LDS addresses of the blur passes
    constexpr int V_MAINC = T::NT / (T::RGR / K);
    const int v_rgp = tid / V_MAINC, v_col = tid - v_rgp * V_MAINC;
    const double *vsrc = ct + v_col * T::CTP + v_rgp * K;
    double *vdst = vb + (v_rgp * K) * T::VP + v_col;
    const double *hsrc = vb + rr * T::VP + cg * K;

    const int n_oct = MST_VARIANT(4) ? 0 : lv->n_octaves, lpo = lv->levels_per_octave;   // [ablation 4: staging + epilogue only]
    const int prot = (int)(blockIdx.x >> 3) * 2 + (int)(blockIdx.x >> 11);
    int tested = 0;
#if defined(MST_INJECT)
    Inject inj;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        inj.q[k] = (double)(tid + k);
        inj.u[k] = (uint32_t)(tid * 7 + k);
    }
#endif
    unsigned long long *tr = nullptr;
#ifdef MST_PROFILE
    // timeline sample: MST_TRACE_WGS consecutive slots of block 0, starting at 3/8 of the grid (tiles inside the band)
    if (trace && slot >= 3 * (per_xcd >> 3) && slot < 3 * (per_xcd >> 3) + MST_TRACE_WGS) {
        tr = trace + ((size_t)(slot - 3 * (per_xcd >> 3)) * T::NW + (tid >> 6)) * (MST_MAX_LEVELS + 1) * MST_TRACE_STAMPS;
        MST_STAMP(tr, MST_MAX_LEVELS * MST_TRACE_STAMPS + 1)        // end of staging
        if ((tid & 63) == 0) tr[MST_MAX_LEVELS * MST_TRACE_STAMPS + 2] = (unsigned long long)slot | ((unsigned long long)(nz_mask != 0) << 40);
    }
#endif
    for (int o = 0; o < n_oct; ++o) {
        // With octaves a factor 2 apart and s = 10, sigma_11 and sigma_12 of one octave are bit-identical to sigma_1 and
        // sigma_2 of the next (checked on the host), so G_1, G_2 and D_1 of the new octave are exactly the G_11, G_12
        // and D_11 this thread already holds: the rolling state after the previous octave's last level IS the state
        // after this octave's second level, and the two blurs are skipped.
        for (int kl = lv->first_level[o]; kl <= lpo; ++kl) {
            const int l = o * lpo + kl - 1;
            const int r = lv->radius[l];
            MST_STAMP(tr, 0)
            // the level's taps, fetched ONCE (scalar loads, wave-uniform -> SGPRs) and shared by both passes
            double taps[RMAX + 1];
#pragma unroll
            for (int j = 0; j <= RMAX; ++j) taps[j] = lv->taps[l][j];
            double g[K];
            // the leftover V-pass pieces occupy the first ceil(R/4) waves of a rotated wave order, so that over the
            // levels (and between the workgroups sharing a CU) every SIMD carries the same share of them
            const int ptid = (tid + 64 * ((l + prot) & 3)) & (T::NT - 1);
            blur_dispatch<T>(r, ct, vb, taps, ptid, vsrc, vdst, hsrc, g, variant, tr MST_INJECT_PASS);
            double d[K];
            if (kl >= 2) {
#pragma unroll
                for (int k = 0; k < K; ++k) d[k] = gprev[k] - g[k];
                if (!wave_all_in) {                          // maximum_filter pads with zeros outside the block
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (!((in_mask >> k) & 1u)) d[k] = 0.0;
                }
                de_mine[0] = d[0];
                de_mine[RGR] = d[K - 1];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) gprev[k] = g[k];
            MST_STAMP(tr, 4)
            __syncthreads();   // edge strip visible; every H-pass read of vb is done before the next V pass writes it
            MST_STAMP(tr, 5)
#ifdef MST_PROFILE
            unsigned long long *tr_lvl = tr;
            if (tr) tr += MST_TRACE_STAMPS;
#endif
#if defined(MST_INJECT) && MST_INJECT == 2
            inject_work<>(inj);
#endif
            if (kl < 2) continue;
            if (MST_VARIANT(1) || MST_VARIANT(32)) continue;     // [ablation 1] blur + DoG only

            // zero-padded 3x3 max at the owned pixels: 3-max along the row in registers, then across rows via lane shifts.
            // A pixel's maximum is only ever compared with DoG values of the SAME pixel (mustache.py:760-765, on the tested
            // pixels), the row shifts stay inside the wave and the neighbouring column groups read this wave's edge samples
            // from the strip written above -- so a wave that owns no tested pixel has no observable use for its maxima and
            // skips them together with the sieve (its Gaussian levels, DoG values and edge samples are produced as before).
            // The maxima live in ONE set of registers, Mc: the comparisons against the previous level's maxima are taken first,
            // then the new maxima are written over them, then the comparisons against the new ones.  A wave without a tested
            // pixel touches neither: its Mc keeps the initial zeros, which nobody reads (every reader is under wave_has_nz).
            uint32_t en = 0, gn = 0;   // en: D_new == M_new;  gn: D_new > M_prev (M of the level before it); pixel k at bit K - 1 - k
            [[maybe_unused]] double lmin_all = INFINITY, lsum_all = 0.0;      // (wide tile: every wave writes its slot)
            if (wave_has_nz) {
                const double dl = de_left[0], dr = de_right[0];      // requested first: the comparisons below cover the LDS latency
                // the comparisons belong to the sieve, which the reference evaluates on the tested pixels only
                // (LocMaxC[nz] == Lc[nz] ..., mustache.py:760-765)
                static_assert(K % 4 == 0, "sieve_bits4 takes the pixels in fours");
                for_each_index(std::make_integer_sequence<int, K / 4>(), [&](auto jc) __attribute__((always_inline)) {
                    constexpr int j = 4 * decltype(jc)::value;
                    sieve_bits4<true, j == 0>(gn, d[j], Mc[j], d[j + 1], Mc[j + 1], d[j + 2], Mc[j + 2], d[j + 3], Mc[j + 3]);
                });
                double hm[K];
#pragma unroll
                for (int j = 0; j < K / 2; ++j) {      // max(d[2j], d[2j+1]) serves both of its pixels: 12 v_max_f64, not 16
                    const double pj = dmax(d[2 * j], d[2 * j + 1]);
                    hm[2 * j] = dmax(j == 0 ? dl : d[2 * j - 1], pj);
                    hm[2 * j + 1] = dmax(pj, 2 * j + 2 == K ? dr : d[2 * j + 2]);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) Mc[k] = dmax(dmax(lane_prev(hm[k]), hm[k]), lane_next(hm[k]));
                for_each_index(std::make_integer_sequence<int, K / 4>(), [&](auto jc) __attribute__((always_inline)) {
                    constexpr int j = 4 * decltype(jc)::value;
                    sieve_bits4<false, j == 0>(en, d[j], Mc[j], d[j + 1], Mc[j + 1], d[j + 2], Mc[j + 2], d[j + 3], Mc[j + 3]);
                });
                // the reference evaluates the sieve and expon.fit on the tested pixels only (Lc[nz], mustache.py:755-768);
                // a wave that owns none has nothing to do here.  (Under the maxima's own test of wave_has_nz: a second test
                // behind the join makes the compiler carry the condition there as a per-lane 0 / 1 value.)
                if (kl >= 4) {
                    // tested level = D_{kl-2}: previous = D_{kl-3} (ep), current (Dc, ec, gp), next = this one (Mc by now, en)
                    const uint32_t code = (uint32_t)tested + 1u;
                    double lmin = INFINITY, lsum = 0.0;      // the level's statistics over this thread's tested pixels
                    // branch-free form: the five terms fold into ONE floating-point comparison per pixel (D_c > best and
                    // D_c > M_n <=> D_c > max(best, M_n): no NaN reaches here) and one bit of a mask that is combined for all
                    // K pixels at once; updates and statistics are selects, so the K pixels are independent instruction streams
                    // instead of K nested exec-mask branches in a row
                    //
                    // The mask bit is never tested on its own (a bit test into a second lane mask, then an or of the two): the
                    // flag word is shifted up pixel by pixel and the bit that falls out IS the gate's lane mask (gated_greater).
                    // A pixel that is never tested holds best = +inf from the start, so the tested-pixel bits are no term of the
                    // gate.  What the phase costs is its instruction COUNT: 13 -> 11 vector instructions per pixel here.
                    uint32_t flags = (ec & (ep | en) & gp) << (32 - K);      // pixel 0 on top (sieve_bits4's bit order)
                    for_each_index(std::make_integer_sequence<int, K>(), [&](auto kc) __attribute__((always_inline)) {
                        constexpr int k = decltype(kc)::value;
                        const bool upd = gated_greater(flags, Dc[k], dmax(best[k], Mc[k]));
                        best[k] = upd ? Dc[k] : best[k];
                        lvl[k] = upd ? code : lvl[k];
                        // statistics of |D_c| over the tested pixels, on the words of D_c (fabs is a source modifier).  Not
                        // tested: the sum gets +0.0 (x + 0.0 == x for every x >= +0.0: its bits are unchanged), the minimum
                        // exactly +inf (0x7ff00000 over the zero low word).  The low word is selected once for both: one
                        // register pair serves the minimum and then, its high word selected again in place, the sum -- three
                        // selects where two separate pairs take four.
                        const bool tz = (nz_mask & (1u << k)) != 0;                  // loop-invariant: a lane mask in scalar registers
                        const uint32_t alo = tz ? (uint32_t)__double2loint(Dc[k]) : 0u;
                        uint32_t ahi = tz ? (uint32_t)__double2hiint(Dc[k]) : 0x7ff00000u;
                        // The empty statement hides that ahi is a select on tz: otherwise `tz ? ahi : 0` below folds to a
                        // select on D_c's high word, the sum's operand becomes a register pair of its own and needs a copy of
                        // alo.  It works while scripts/isa_census.py shows 3 v_cndmask_b32 per pixel for the statistics and
                        // no v_mov_b32 between them (48 selects in the sieve's block at K = 8, 24 of them the updates).
                        asm("" : "+v"(ahi));
                        lmin = __builtin_fmin(lmin, fabs(__hiloint2double((int)ahi, (int)alo)));      // both >= 0: operand order immaterial
                        lsum = lsum + fabs(__hiloint2double((int)(tz ? ahi : 0u), (int)alo));
                    });
                    // fixed-order DPP reduction inside the wave (total lands in lane 63), one slot per (level, wave)
                    if (!MST_VARIANT(2)) wave_reduce_min_sum(lmin, lsum);
                    // a wave without a tested pixel leaves its slot at the identities it was given before the loop
                    if constexpr (ST_ONCE) {
                        if (lane == 63) {
                            st[(tested * T::NW + wave) * 2] = lmin;
                            st[(tested * T::NW + wave) * 2 + 1] = lsum;
                        }
                    } else {
                        lmin_all = lmin;
                        lsum_all = lsum;
                    }
                }
            }
            if (kl >= 4) {
                if constexpr (!ST_ONCE) {
                    if (lane == 63) {
                        st[(tested * T::NW + wave) * 2] = lmin_all;
                        st[(tested * T::NW + wave) * 2 + 1] = lsum_all;
                    }
                }
                ++tested;
            }
            ep = ec;
            ec = en;
            gp = gn;
#pragma unroll
            for (int k = 0; k < K; ++k) Dc[k] = d[k];
#ifdef MST_PROFILE
            MST_STAMP(tr_lvl, 6)
#endif
        }
    }

    // ---- found pixels -> per-block record list.  One atomicAdd per WORKGROUP reserves its slots (a returning atomic
    // per pixel serialises ~150k same-address operations per block at the L2); inside the reservation the order is
    // wave, then k, then lane.  The list is sorted by pixel index before it reaches the host.
    int e_b = b, e_b2 = b2, e_x0 = x0, e_delta2 = item.delta2, e_CH = CH;      // what the epilogue needs of the work item
    if constexpr (T::RMAX > 14) {
        typedef const KernArgs __attribute__((address_space(4))) *KernArgsPtr;       // constant address space: scalar loads
        KernArgsPtr ka = (KernArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
        found = ka->found;
        found_cap = ka->found_cap;
        found_count = ka->found_count;
        n_tested = ka->n_tested;
        part = ka->partial + (size_t)slot * n_tested * 2;
        const WorkItem again = ka->items[slot];
        e_b = again.b;
        e_b2 = again.delta2 != 0 ? again.b + 1 : -1;
        e_x0 = again.x0;
        e_delta2 = again.delta2;
        e_CH = ka->CH;
    }
#if defined(MST_INJECT)
    {
        double qs = 0.0;
        uint32_t us = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            qs += inj.q[k];
            us ^= inj.u[k];
        }
        if (qs == -1.0 && us == 0x12345u) part[0] = qs;      // never true: keeps the injected chains alive
    }
#endif
    // [census: epilogue empty]  A workgroup without a tested pixel (workgroup-uniform, from __syncthreads_or) found nothing and
    // its statistics are the identities: what the skip_empty return writes, and the bits the fold below would form from slots
    // that all hold {inf, 0}.
    if (T::RMAX <= 14 && !any_nz) {     // (the wide tile does not carry any_nz through its level loop: it goes the long way)
        for (int t = tid; t < tested; t += T::NT) {
            part[2 * t] = INFINITY;
            part[2 * t + 1] = 0.0;
        }
        return;
    }
    // [census: epilogue reservation]  Wave totals: a wave without a tested pixel holds lvl == 0 everywhere and counts nothing.
    unsigned long long bal[K];          // lanes of this wave with a record for pixel k
    uint32_t my_total = 0;              // wave-uniform
#pragma unroll
    for (int k = 0; k < K; ++k) bal[k] = 0;
    if (wave_has_nz) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            bal[k] = __ballot(lvl[k] != 0);
            my_total += (uint32_t)__builtin_popcountll(bal[k]);
        }
    }
    // The totals are exchanged ONCE; every wave forms its own prefix and the workgroup's total from them.  ct is dead behind
    // the last level's barriers (the edge strip is not: the last level's maxima read it), so the exchange needs no barrier in
    // front of it, and the one behind it also makes every wave's statistics slots visible to the fold.
    uint32_t *cnt_lds = reinterpret_cast<uint32_t *>(ct);
    if (lane == 0) cnt_lds[wave] = my_total;
    __syncthreads();
    uint32_t tot = 0, wave_off = 0;
#pragma unroll
    for (int w = 0; w < T::NW; ++w) {
        const uint32_t n = cnt_lds[w];
        wave_off += w < wave ? n : 0u;
        tot += n;
    }
    tot = __builtin_amdgcn_readfirstlane(tot);
    if (tot && tid == 0) {              // one lane reserves the workgroup's slots in both blocks
        cnt_lds[T::NW] = atomicAdd(found_count + e_b, tot);
        cnt_lds[T::NW + 1] = e_b2 >= 0 ? atomicAdd(found_count + e_b2, tot) : 0u;
    }
    // [census: epilogue fold]
    for (int t = tid; t < tested; t += T::NT) {
        double mn = st[(t * T::NW) * 2], sm = st[(t * T::NW) * 2 + 1];
        for (int w = 1; w < T::NW; ++w) {
            const double a = st[(t * T::NW + w) * 2];
            mn = a < mn ? a : mn;
            sm = sm + st[(t * T::NW + w) * 2 + 1];
        }
        part[2 * t] = mn;
        part[2 * t + 1] = sm;
    }
    if (!tot) return;                   // tested, nothing found (workgroup-uniform): no record loop
    __syncthreads();
    // [census: epilogue records]
    if (!my_total) return;              // (wave-uniform; no barrier follows)
    const uint32_t wave_base = cnt_lds[T::NW] + wave_off;
    const uint32_t wave_base2 = cnt_lds[T::NW + 1] + wave_off;
    uint32_t kbase = 0;                 // records of this wave for smaller k
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (lvl[k]) {
            // kbase + the records of the lanes below mine
            const uint32_t off = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[k], kbase));
            mst_found rec;
            rec.pixel = (uint32_t)gy * (uint32_t)e_CH + (uint32_t)(e_x0 + cg * K + k);
            rec.level = lvl[k];
            rec.value = best[k];
            if (wave_base + off < found_cap) found[(size_t)e_b * found_cap + wave_base + off] = rec;
            if (e_b2 >= 0 && wave_base2 + off < found_cap) {        // the same pixel in the neighbouring block's coordinates
                rec.pixel = (uint32_t)(gy + e_delta2) * (uint32_t)e_CH + (uint32_t)(e_x0 + cg * K + k + e_delta2);
                found[(size_t)e_b2 * found_cap + wave_base2 + off] = rec;
            }
        }
        kbase += (uint32_t)__builtin_popcountll(bal[k]);
    }
}

// partial[item][t][2] -> level_stats[b][t][2].  A block's tiles are numbered by their position in ITS tile grid (row-major);
// slot_of_pos[b][pos] is the work item that computed that tile -- one of the block's own, or a shared one that the previous
// block's list carries -- or -1.  The summation order is fixed by the POSITION numbering (thread i takes positions i, i + 256,
// ... in ascending order, then a fixed tree), whichever items were launched: a tile that is not in the list would have
// contributed {inf, 0}, which changes neither the minimum nor the sum, so a block's statistics do not depend on
// MST_FLAG_SKIP_EMPTY down to the last bit.
__global__ void __launch_bounds__(256)
stats_reduce_kernel(const double *__restrict__ partial, int npos, const int32_t *__restrict__ slot_of_pos, int n_tested,
                    double *__restrict__ level_stats) {
    __shared__ double smin[256], ssum[256];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int32_t *sop = slot_of_pos + (size_t)b * npos;
    double mn = INFINITY, sm = 0.0;
    for (int i = tid; i < npos; i += 256) {
        const int slot = sop[i];
        if (slot < 0) continue;
        const double a = partial[((size_t)slot * n_tested + t) * 2];
        mn = a < mn ? a : mn;
        sm = sm + partial[((size_t)slot * n_tested + t) * 2 + 1];
    }
    smin[tid] = mn;
    ssum[tid] = sm;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            smin[tid] = smin[tid + s] < smin[tid] ? smin[tid + s] : smin[tid];
            ssum[tid] = ssum[tid] + ssum[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        level_stats[((size_t)b * MST_MAX_TESTED + t) * 2] = smin[0];
        level_stats[((size_t)b * MST_MAX_TESTED + t) * 2 + 1] = ssum[0];
    }
}

int check_levels(const mst_levels *lv, int *max_radius, int *n_tested) {
    if (!lv) return mst::fail(MST_E_ARG, "level table is null");
    if (lv->n_octaves < 1 || lv->levels_per_octave < 4 ||
        lv->n_octaves * lv->levels_per_octave > MST_MAX_LEVELS)
        return mst::fail(MST_E_ARG, "level table: need >= 1 octave, >= 4 levels per octave, <= %d levels",
                         MST_MAX_LEVELS);
    const int nt = lv->n_octaves * (lv->levels_per_octave - 3);
    if (nt > MST_MAX_TESTED) return mst::fail(MST_E_ARG, "level table: more than %d tested levels", MST_MAX_TESTED);
    int mr = 0;
    for (int l = 0; l < lv->n_octaves * lv->levels_per_octave; ++l) {
        if (lv->radius[l] < 1 || lv->radius[l] > 28)
            return mst::fail(MST_E_ARG, "level %d: blur radius %d outside the supported range [1, 28]", l,
                             lv->radius[l]);
        mr = lv->radius[l] > mr ? lv->radius[l] : mr;
    }
    *max_radius = mr;
    *n_tested = nt;
    return MST_OK;
}

#ifdef MST_EXP_DEFAULT_COLS
// Experiment (round 4, variant builds): the default radii on a K = 4 tile of MST_EXP_DEFAULT_COLS columns -- 96: 768 threads =
// 12 waves = THREE per SIMD in one workgroup per CU (<= 168 VGPRs, ~115 KB of LDS); 64: 512 threads, two per SIMD
#ifndef MST_EXP_DEFAULT_K
#define MST_EXP_DEFAULT_K 4
#endif
#ifndef MST_EXP_DEFAULT_ROWS
#define MST_EXP_DEFAULT_ROWS 32
#endif
#ifndef MST_EXP_DEFAULT_TIGHT
#define MST_EXP_DEFAULT_TIGHT true
#endif
using TileDefault = Tile<MST_EXP_DEFAULT_ROWS, MST_EXP_DEFAULT_COLS, 14, MST_EXP_DEFAULT_K, 1, false, MST_EXP_DEFAULT_TIGHT>;
#else
using TileDefault = Tile<32, 64, 14>;   // the reference's default octaves (radius <= 14)
#endif
// -sz / -oc variants up to radius 28: the default tile's 32 x 64 region with 512 threads x 4 pixels and tight LDS pitches
// (131 KB: ONE workgroup of 8 waves per CU, 155 VGPRs).  Round 4 measured it against the 32 x 32 / 256-thread tile of rounds 2-3
// (two workgroups per CU, 251 VGPRs, 1.26 x more executed blur flops): octaves (3.2, 6.4) 45.6 -> 25.4 ms per 12 blocks dense,
// 18.8 -> 10.2 ms with the tile list, identical found sets (LABBOOK.md R4.2)
using TileWide = Tile<32, 64, 28, 4, 1, false, true>;
using TileDefaultFma = Tile<32, 64, 14, 8, 1, true>;   // opt-in relaxed arithmetic (MST_FLAG_FMA), default radii only
#ifdef MST_EXP_TILE7
// Experiment (round 4, variant builds only: scripts/build_variant.sh ... -DMST_EXP_TILE7=<waves per SIMD>): a tile for level
// tables whose largest blur radius is 7 (octave 1.6 alone) -- 7-pixel halo, tight pitches: 53.3 KB of LDS, three workgroups
// per CU if the register allocation allows MST_EXP_TILE7 waves per SIMD.  Prices the "two launches by octave" design.
using TileOct1 = Tile<32, 64, 7, 8, MST_EXP_TILE7, false, true>;
#endif

// A block's tile grid has at most this many rows / columns of tiles, whatever the lattice phase of its origin
template <class T>
int grid_rows(int CH) { return (CH + T::ITR - 1) / T::ITR + 1; }
template <class T>
int grid_cols(int CH) { return (CH + T::ITC - 1) / T::ITC + 1; }
template <class T>
int grid_positions(int CH) { return grid_rows<T>(CH) * grid_cols<T>(CH); }

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
int positions_max(int CH) {
    const int a = grid_positions<TileDefault>(CH), b = grid_positions<TileWide>(CH);
    return a > b ? a : b;
}

int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The work list of one launch (see WorkItem).  Tiles sit on a lattice of ITR x ITC interiors; with `share` (band source: the
// blocks' origins in chromosome coordinates are known) the lattice is anchored at chromosome coordinate 0, so overlapping
// blocks cut the same tiles, and a tile that lies inside block b AND block b + 1 with its whole halo is listed once, for
// block b, with b2 = b + 1.  Without it (dense blocks from the caller, or MST_FLAG_NO_SHARE) every block has its own lattice
// anchored at its origin -- the grid of rounds 1 and 2.
//   band_only : list only the tiles whose owned pixels can reach the tested band 4 <= col - row <= dpx + 1 (skip_empty on the
//               band source: the others would return at once)
//   slot_of_pos[b * npos + pos] = index of the item that computes the tile at grid position pos of block b, or -1
// Order: a block's items row-major; without band_only the tile ROWS are dealt to eight buckets in turn (the kernel gives each
// XCD a contiguous eighth of the list): the upper rows of a block hold the wide part of the band, whose tiles cost more than
// the constant ones, and the dispatcher hands out workgroups in order, so an XCD that got only upper rows would set the pace.
//   cuts / stage_begin (staged launches, mst_scale_space_band_stage): stage i holds the items of blocks [cuts[i - 1], cuts[i]); the
//               list is ordered stage by stage (each stage dealt on its own) and stage_begin[i] is its first item.  The list
//               itself -- which tile is computed for which blocks -- is that of the whole launch: sharing crosses the cuts.
template <class T>
void build_items(const int64_t *starts, int B, int CH, int dpx, bool share, bool band_only, std::vector<WorkItem> &items,
                 std::vector<int32_t> &slot_of_pos, int *tiles_total_out, const int32_t *cuts = nullptr, int n_cuts = 0,
                 std::vector<int32_t> *stage_begin = nullptr) {
    const int npos = grid_positions<T>(CH), gcols = grid_cols<T>(CH);
    slot_of_pos.assign((size_t)B * npos, -1);
    std::vector<WorkItem> list;
    std::vector<int> row_of;                      // running tile-row counter of each item (for the dealing)
    std::vector<int32_t> pos_of, pos2_of;
    std::vector<char> given((size_t)npos, 0), given_next((size_t)npos, 0);   // tiles of block b that block b - 1 delivers
    int rows_seen = 0, tiles_total = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t s0 = share ? starts[b] : 0;
        const int64_t a_lo = floor_div(s0, T::ITR), c_lo = floor_div(s0, T::ITC);
        // lattice cell a owns chromosome rows [a ITR, a ITR + ITR); region row 0 is the ring row above it
        const int64_t a_hi = floor_div(s0 + CH - 1, T::ITR), c_hi = floor_div(s0 + CH - 1, T::ITC);
        const bool next_ok = share && b + 1 < B && starts[b + 1] > starts[b] && starts[b + 1] - starts[b] < CH;
        const int64_t s1 = next_ok ? starts[b + 1] : 0;
        std::fill(given_next.begin(), given_next.end(), 0);
        for (int64_t a = a_lo; a <= a_hi; ++a) {
            bool row_has = false;
            for (int64_t cc = c_lo; cc <= c_hi; ++cc) {
                const int y0 = (int)(a * T::ITR - s0) - 1, x0 = (int)(cc * T::ITC - s0) - 1;
                const int pos = (int)(a - a_lo) * gcols + (int)(cc - c_lo);
                ++tiles_total;
                // owned pixels inside the block
                const int r_lo = y0 + 1 > 0 ? y0 + 1 : 0, r_hi = y0 + T::ITR < CH - 1 ? y0 + T::ITR : CH - 1;
                const int q_lo = x0 + 1 > 0 ? x0 + 1 : 0, q_hi = x0 + T::ITC < CH - 1 ? x0 + T::ITC : CH - 1;
                if (r_lo > r_hi || q_lo > q_hi) continue;                       // the cell only grazes the block with its ring
                if (band_only && !((q_hi - r_lo >= 4) && (q_lo - r_hi <= dpx + 1))) continue;
                if (given[(size_t)pos]) continue;                               // block b - 1's list computes it for both
                WorkItem it;
                it.b = b;
                it.y0 = y0;
                it.x0 = x0;
                it.delta2 = 0;
                int pos2 = -1;
                if (next_ok) {
                    // staged window (region + blur halo) inside both blocks: no reflection, no zero padding, no pixel outside
                    const int Y0 = y0 - T::RMAX, X0 = x0 - T::RMAX;
                    const int d = (int)(s0 - s1);                               // block b + 1 coordinate = block b coordinate + d
                    const bool in_b = Y0 >= 0 && X0 >= 0 && Y0 + T::CTR <= CH && X0 + T::CTC <= CH;
                    const bool in_n = Y0 + d >= 0 && X0 + d >= 0 && Y0 + d + T::CTR <= CH && X0 + d + T::CTC <= CH;
                    if (in_b && in_n) {
                        const int64_t a1_lo = floor_div(s1, T::ITR), c1_lo = floor_div(s1, T::ITC);
                        pos2 = (int)(a - a1_lo) * gcols + (int)(cc - c1_lo);
                        it.delta2 = d;
                        given_next[(size_t)pos2] = 1;
                    }
                }
                list.push_back(it);
                row_of.push_back(rows_seen);
                pos_of.push_back(pos);
                pos2_of.push_back(pos2);
                row_has = true;
            }
            if (row_has) ++rows_seen;
        }
        given.swap(given_next);
    }
    // final order + the position maps
    const size_t n = list.size();
    items.clear();
    items.reserve(n);
    std::vector<size_t> order;
    order.reserve(n);
    if (stage_begin) stage_begin->clear();
    // `list` is in block order, so a stage is a contiguous run [lo, hi) of it
    size_t lo = 0;
    for (int sgi = 0; sgi <= n_cuts; ++sgi) {
        const int b_end = sgi < n_cuts ? cuts[sgi] : B;
        size_t hi = lo;
        while (hi < n && list[hi].b < b_end) ++hi;
        if (stage_begin) stage_begin->push_back((int32_t)order.size());
        if (band_only) {
            for (size_t i = lo; i < hi; ++i) order.push_back(i);
        } else {
            size_t at[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (size_t i = lo; i < hi; ++i) ++at[row_of[i] % 8 + 1];
            for (int x = 0; x < 8; ++x) at[x + 1] += at[x];
            const size_t base = order.size();
            order.resize(base + (hi - lo));
            for (size_t i = lo; i < hi; ++i) order[base + at[row_of[i] % 8]++] = i;
        }
        lo = hi;
    }
    if (stage_begin) stage_begin->push_back((int32_t)order.size());
    for (size_t k = 0; k < n; ++k) {
        const size_t i = order[k];
        items.push_back(list[i]);
        slot_of_pos[(size_t)list[i].b * npos + pos_of[i]] = (int32_t)k;
        if (list[i].delta2 != 0) slot_of_pos[(size_t)(list[i].b + 1) * npos + pos2_of[i]] = (int32_t)k;
    }
    if (tiles_total_out) *tiles_total_out = tiles_total;
}

// the launch's counters to zero.  A kernel, not hipMemsetAsync: the launch can be captured into a hipGraph, and a replayed memset
// node is not reliable on this ROCm (mst_tail.hip, fit_kernel; LABBOOK.md R4.6)
__global__ void zero_counts_kernel(uint32_t *found_count, uint32_t *nz_count, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        found_count[i] = 0;
        if (nz_count) nz_count[i] = 0;
    }
}

// level_stats of blocks without any tested tile: {min, sum} = {inf, 0}, what the reduction of zero tiles yields
__global__ void fill_stats_kernel(double *level_stats, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        level_stats[2 * i] = INFINITY;
        level_stats[2 * i + 1] = 0.0;
    }
}

}  // namespace

namespace {
// The ONE map from a level table's largest blur radius (and MST_FLAG_FMA) to the tile a launch runs: f(TileTag<T>())
template <class T>
struct TileTag {
    using type = T;
};
template <class F>
static auto with_tile(int max_radius, bool fma, F &&f) {
    if (fma) return f(TileTag<TileDefaultFma>());
#ifdef MST_EXP_TILE7
    if (max_radius <= 7 && getenv("MST_EXP_USE_TILE7")) return f(TileTag<TileOct1>());
#endif
    if (max_radius <= TileDefault::RMAX) return f(TileTag<TileDefault>());
    return f(TileTag<TileWide>());
}

// build_items on the lattice of the level table's tile -- the default tile's or the wide one's: the FMA tile and the experiment's
// TileOct1 are launched on lists of the default lattice; returns the tile's grid_positions
static int build_list(int max_radius, const int64_t *starts, int B, int CH, int dpx, bool share, bool band_only,
                      std::vector<WorkItem> &items, std::vector<int32_t> &sop, int *tiles_total, const int32_t *cuts = nullptr,
                      int n_cuts = 0, std::vector<int32_t> *stage_begin = nullptr) {
    if (max_radius > TileDefault::RMAX) {
        build_items<TileWide>(starts, B, CH, dpx, share, band_only, items, sop, tiles_total, cuts, n_cuts, stage_begin);
        return grid_positions<TileWide>(CH);
    }
    build_items<TileDefault>(starts, B, CH, dpx, share, band_only, items, sop, tiles_total, cuts, n_cuts, stage_begin);
    return grid_positions<TileDefault>(CH);
}

// Byte offsets of a launch's tables in its workspace: level table, block origins, work list, position map (slot_of_pos), and
// behind them the per-item partial statistics.  worst() is what mst_scale_space_workspace_bytes promises and every plain launch
// carves; a captured launch packs the same layout with its actual counts (enqueue_launch) but keeps the partials where they are.
struct Workspace {
    size_t levels = 0, starts, items, sop, partial;
    Workspace(int B, size_t n_items, size_t n_sop) {
        starts = align_up(sizeof(DevLevels), 256);
        items = starts + align_up(sizeof(int64_t) * (size_t)B, 256);
        sop = items + align_up(sizeof(WorkItem) * n_items, 256);
        partial = sop + align_up(sizeof(int32_t) * n_sop, 256);
    }
    static Workspace worst(int B, int CH) {
        const size_t n = (size_t)B * positions_max(CH);
        return Workspace(B, n, n);
    }
};
}  // namespace

extern "C" uint64_t mst_scale_space_workspace_bytes(int32_t B, int32_t CH, const mst_levels *lv) {
    int mr = 0, nt = 0;
    if (B <= 0 || CH <= 0 || check_levels(lv, &mr, &nt) != MST_OK) return 0;
    return Workspace::worst(B, CH).partial + sizeof(double) * 2 * (size_t)B * positions_max(CH) * nt;
}

template <class T, bool BAND>
static int launch_scale_space(const double *c, const uint8_t *nz, BandSrc src, int CH, const DevLevels *d_lv,
                              mst_found *found, uint32_t found_cap, uint32_t *found_count, double *partial,
                              int n_tested, int skip_empty, const WorkItem *d_items, int n_items, hipStream_t s) {
    static unsigned long long lds_allowed = 0;      // per device (mst_common.h)
    MST_HIP(mst::allow_dynamic_lds(reinterpret_cast<const void *>(&scale_space_kernel<T, BAND>), (int)T::LDS_BYTES,
                                   &lds_allowed));
    const int gx = (n_items + 7) / 8 * 8;
    int variant = 0;
    unsigned long long *trace = nullptr;
#ifdef MST_PROFILE
    const char *venv = getenv("MST_ABLATE");          // timing ablations (results invalid), PROFILE builds only
    variant = venv ? atoi(venv) : 0;
    const char *tpath = getenv("MST_TRACE");          // phase timeline of a sample of workgroups -> file
    const size_t tbytes = sizeof(unsigned long long) * MST_TRACE_WGS * T::NW * (MST_MAX_LEVELS + 1) * MST_TRACE_STAMPS;
    if (tpath) {
        MST_HIP(hipMalloc((void **)&trace, tbytes));
        MST_HIP(hipMemsetAsync(trace, 0, tbytes, s));
    }
#endif
    scale_space_kernel<T, BAND><<<gx, T::NT, T::LDS_BYTES, s>>>(c, nz, src, CH, d_lv, found, found_cap, found_count, partial,
                                                              d_items, n_items, n_tested, skip_empty, variant, trace);
    MST_LAUNCH_CHECK();
#ifdef MST_PROFILE
    if (trace) {
        std::vector<unsigned long long> host(tbytes / sizeof(unsigned long long));
        MST_HIP(hipStreamSynchronize(s));
        MST_HIP(hipMemcpy(host.data(), trace, tbytes, hipMemcpyDeviceToHost));
        MST_HIP(hipFree(trace));
        if (FILE *f = fopen(tpath, "wb")) {
            const unsigned long long hdr[4] = {MST_TRACE_WGS, (unsigned long long)T::NW, MST_MAX_LEVELS + 1, MST_TRACE_STAMPS};
            fwrite(hdr, sizeof(hdr), 1, f);
            fwrite(host.data(), 1, tbytes, f);
            fclose(f);
        }
    }
#endif
    return MST_OK;
}

extern "C" int mst_scale_space_band_tiles(int32_t CH, int32_t dpx, const mst_levels *lv, int32_t *tiles_total_out) {
    int mr = 0, nt = 0;
    if (CH <= 0 || dpx < 0 || check_levels(lv, &mr, &nt) != MST_OK) return -1;
    std::vector<WorkItem> items;
    std::vector<int32_t> sop;
    const int64_t start = 0;
    int total = 0;
    build_list(mr, &start, 1, CH, dpx, false, true, items, sop, &total);
    if (tiles_total_out) *tiles_total_out = total;
    return (int)items.size();
}

extern "C" int mst_scale_space_band_items(const int64_t *starts, int32_t B, int32_t CH, int32_t dpx, const mst_levels *lv,
                                          int32_t flags, int64_t *tiles_out, int64_t *shared_out) {
    int mr = 0, nt = 0;
    if (!starts || B <= 0 || CH <= 0 || dpx < 0 || check_levels(lv, &mr, &nt) != MST_OK) return -1;
    const bool share = !(flags & MST_FLAG_NO_SHARE), band_only = (flags & MST_FLAG_SKIP_EMPTY) != 0;
    std::vector<WorkItem> items;
    std::vector<int32_t> sop;
    int total = 0;
    build_list(mr, starts, B, CH, dpx, share, band_only, items, sop, &total);
    int64_t shared = 0;
    for (const WorkItem &it : items) shared += it.delta2 != 0;
    if (tiles_out) *tiles_out = (int64_t)items.size() + shared;      // tiles the blocks would run one by one
    if (shared_out) *shared_out = shared;
    return (int)items.size();
}

// level table -> the kernel's form.  first_level[o] = 3 where octave o's first two levels repeat the previous octave's last two
// (same radius, same taps): the kernel keeps those blurs instead of computing them again
static int make_dev_levels(const mst_levels *lv, const char *who, DevLevels *h) {
    if (lv->n_octaves > 16) return mst::fail(MST_E_ARG, "%s: more than 16 octaves", who);
    memset(h, 0, sizeof(*h));
    h->n_octaves = lv->n_octaves;
    h->levels_per_octave = lv->levels_per_octave;
    for (int l = 0; l < lv->n_octaves * lv->levels_per_octave; ++l) {
        h->radius[l] = lv->radius[l];
        for (int j = 0; j <= lv->radius[l]; ++j) h->taps[l][j] = lv->taps[l][j];
    }
    const int lpo = lv->levels_per_octave;
    for (int o = 0; o < lv->n_octaves; ++o) {
        h->first_level[o] = 1;
        if (o == 0) continue;
#ifdef MST_PROFILE
        if (getenv("MST_NO_LEVEL_REUSE")) continue;       // PROFILE builds only: time the 24-blur form
#endif
        bool same = true;
        for (int q = 0; q < 2 && same; ++q) {
            const int a = (o - 1) * lpo + lpo - 2 + q, b = o * lpo + q;      // (prev octave, k = lpo-1+q) vs (this, k = 1+q)
            same = lv->radius[a] == lv->radius[b] &&
                   memcmp(lv->taps[a], lv->taps[b], sizeof(double) * (lv->radius[a] + 1)) == 0;
        }
        if (same) h->first_level[o] = 3;
    }
    return MST_OK;
}

namespace {
// The work list of a launch as the launches use it: the list, page-locked copies the uploads read (no host memcpy per launch)
// and a DEVICE copy, uploaded once per list: a step that repeats its launch (a benchmark loop, the second sample, the same
// chromosome again) does not send the list -- 17 MB for the 124 blocks of chr1 at 1 kb, 0.4 ms in front of the kernel -- again.
// The device buffer belongs to the list and only grows.
struct WorkList {
    std::vector<int64_t> key;
    std::vector<WorkItem> items;
    std::vector<int32_t> sop;
    std::vector<int32_t> stage_begin;        // staged lists: first item of every stage, then the item count
    int npos = 0;
    mst::PinnedList pin_items, pin_sop;
    char *dbuf = nullptr;
    size_t dcap = 0;
    int ddev = -1;
    bool uploaded = false;
    hipEvent_t up = nullptr;                 // behind the upload: launches on other streams wait for it on the device
    mst::UseFence used;                      // behind every launch, on any stream, that read dbuf
    ~WorkList() {
        (void)used.wait();
        if (up) (void)hipEventDestroy(up);
        if (dbuf) (void)hipFree(dbuf);
    }
    // the device copy, for work enqueued on s: uploaded by the first launch that uses the list, read in place afterwards
    int on_device(hipStream_t s, const WorkItem **d_items, const int32_t **d_sop) {
        int dev = 0;
        MST_HIP(hipGetDevice(&dev));
        const size_t off_sop = align_up(pin_items.bytes, 256), need_dev = off_sop + pin_sop.bytes;
        if (uploaded && ddev != dev) uploaded = false;
        if (!uploaded) {
            MST_HIP(used.wait());            // launches on other streams may still read what is overwritten or freed here
            if (dcap < need_dev || ddev != dev) {
                if (dbuf) (void)hipFree(dbuf);
                dbuf = nullptr;
                dcap = 0;
                if (up) (void)hipEventDestroy(up);
                up = nullptr;
                const size_t want = need_dev + need_dev / 4;
                MST_HIP(hipMalloc((void **)&dbuf, want));
                dcap = want;
                ddev = dev;
                MST_HIP(hipEventCreateWithFlags(&up, hipEventDisableTiming));
            }
            MST_HIP(pin_items.upload(dbuf, s));
            MST_HIP(pin_sop.upload(dbuf + off_sop, s));
            MST_HIP(hipEventRecord(up, s));
            uploaded = true;
        } else {
            MST_HIP(hipStreamWaitEvent(s, up, 0));      // uploaded on another stream, perhaps
        }
        *d_items = reinterpret_cast<const WorkItem *>(dbuf);
        *d_sop = reinterpret_cast<const int32_t *>(dbuf + off_sop);
        return MST_OK;
    }
};

// A few recent lists per host thread: a caller that runs the same blocks again -- a benchmark loop, the second sample of a
// two-sample run -- does not pay the ~1 ms of host time per 100 k items again.
//   band source -> tiles on the chromosome's lattice, tiles inside two consecutive blocks computed once (share; without it every
//   block on its own lattice, every tile once per block: the cross-check form of MST_FLAG_NO_SHARE and the dense source)
//   dpx < 0: dense source;  staged: the list in the staged order of build_items (cuts, n_cuts)
struct WorkListCache {
    WorkList list[4];
    unsigned turn = 0;
    int find_or_build(int max_radius, const int64_t *starts, int B, int CH, int dpx, bool share, bool band_only, bool staged,
                      const int32_t *cuts, int n_cuts, WorkList **out) {
        std::vector<int64_t> key;
        key.reserve((size_t)B + 6 + (staged ? n_cuts : 0));
        key.push_back(B);
        key.push_back(CH);
        key.push_back(dpx);
        key.push_back((share ? 1 : 0) | (band_only ? 2 : 0) | (max_radius > TileDefault::RMAX ? 4 : 0));
        if (share) key.insert(key.end(), starts, starts + B);     // without sharing the list does not depend on the origins
        if (staged) {
            key.push_back(-7);
            key.insert(key.end(), cuts, cuts + n_cuts);
        }
        for (WorkList &wl : list)
            if (wl.key == key) *out = &wl;
        if (*out) return MST_OK;
        WorkList *wl = *out = &list[turn++ % 4];
        (void)wl->used.wait();              // (a launch four lists ago: long done) its device copy is about to be replaced
        wl->uploaded = false;
        wl->key = key;
        const std::vector<int64_t> zeros(share ? 0 : (size_t)B, 0);
        wl->npos = build_list(max_radius, share ? starts : zeros.data(), B, CH, dpx < 0 ? 0 : dpx, share, band_only, wl->items,
                              wl->sop, nullptr, staged ? cuts : nullptr, staged ? n_cuts : 0, &wl->stage_begin);
        hipError_t pe = wl->pin_items.assign(wl->items.data(), sizeof(WorkItem) * wl->items.size());
        if (pe == hipSuccess) pe = wl->pin_sop.assign(wl->sop.data(), sizeof(int32_t) * (size_t)B * wl->npos);
        if (pe != hipSuccess) wl->key.clear();
        MST_HIP(pe);
        return MST_OK;
    }
};

// Everything a fused launch enqueues, spelled out: enqueue_launch reads nothing else
struct Launch {
    const double *c;
    const uint8_t *nz;
    BandSrc src;                     // src.starts is set by enqueue_launch
    const int64_t *starts_host;
    int B, CH, max_radius, n_tested, skip_empty;
    bool fma;
    const DevLevels *levels;         // host copy
    mst_found *found;
    uint32_t found_cap;
    uint32_t *found_count;
    double *level_stats;
    char *workspace;
    WorkList *list;
    const int32_t *cuts;             // staged form (mst_scale_space_band_stage): stage >= 0 enqueues only the items of blocks
    int n_cuts, stage;               // [cuts[stage - 1], cuts[stage]) of the launch's ONE work list and the level statistics of
};                                   // those blocks; stage 0 also uploads the tables and zeroes the counters
}  // namespace

// image != nullptr: the call is being CAPTURED into a graph whose copy node reads image (mst::ReplayCache)
template <bool BAND>
static int enqueue_launch(const Launch &a, char *image, hipStream_t s) {
    const bool staged = a.stage >= 0, first = a.stage <= 0, captured = image != nullptr;
    const int B = a.B, nt = a.n_tested, npos = a.list->npos, n_items = (int)a.list->items.size();
    const size_t items_bytes = sizeof(WorkItem) * (size_t)n_items, sop_bytes = sizeof(int32_t) * (size_t)B * npos;
    // Captured launches (small, latency-bound): the four tables lie side by side in the workspace -- the tile positions packed
    // right behind the work list instead of at their worst-case offset -- in the order and alignment of the graph entry's
    // page-locked image, so ONE copy node uploads them all (four nodes of ~5 us each stood in front of a 0.5 ms kernel).
    const Workspace worst = Workspace::worst(B, a.CH), at = captured ? Workspace(B, n_items, (size_t)B * npos) : worst;
    DevLevels *d_lv = reinterpret_cast<DevLevels *>(a.workspace + at.levels);
    int64_t *d_starts = reinterpret_cast<int64_t *>(a.workspace + at.starts);
    const WorkItem *d_items = reinterpret_cast<const WorkItem *>(a.workspace + at.items);
    const int32_t *d_sop = reinterpret_cast<const int32_t *>(a.workspace + at.sop);
    double *partial = reinterpret_cast<double *>(a.workspace + worst.partial);
    if (captured) {
        memcpy(image + at.levels, a.levels, sizeof(DevLevels));
        if (BAND) memcpy(image + at.starts, a.starts_host, sizeof(int64_t) * (size_t)B);
        if (n_items) {
            memcpy(image + at.items, a.list->items.data(), items_bytes);
            memcpy(image + at.sop, a.list->sop.data(), sop_bytes);
        }
        MST_HIP(hipMemcpyAsync(a.workspace, image, n_items ? at.sop + sop_bytes : at.items, hipMemcpyHostToDevice, s));
    } else if (first) {              // through a pinned staging slot (mst::upload_small): the source may die as soon as this returns
        MST_HIP(mst::upload_small(d_lv, a.levels, sizeof(DevLevels), s));
    }
    if (first) {
        zero_counts_kernel<<<(B + 255) / 256, 256, 0, s>>>(a.found_count, BAND ? a.src.nz_count : nullptr, B);
        MST_LAUNCH_CHECK();
    }
    BandSrc src = a.src;
    if (BAND) {
        if (!captured && first) MST_HIP(mst::upload_small(d_starts, a.starts_host, sizeof(int64_t) * B, s));
        src.starts = d_starts;
    }
    if (n_items == 0) {          // no tile reaches the band: nothing is tested, nothing is found
        if (first) {
            fill_stats_kernel<<<(B * MST_MAX_TESTED + 255) / 256, 256, 0, s>>>(a.level_stats, B * MST_MAX_TESTED);
            MST_LAUNCH_CHECK();
        }
        return MST_OK;
    }
    if (!captured) {             // (never while capturing: the device copy's path waits on events and allocates)
        const int drc = a.list->on_device(s, &d_items, &d_sop);
        if (drc != MST_OK) return drc;
    }
    // this call's share of the list and of the blocks (everything, unless staged).  Staged: this stage's run of the list; its
    // items' slots in `partial` keep their positions in the WHOLE list, which is what the position map refers to -- both
    // pointers are simply advanced
    const int it0 = staged ? a.list->stage_begin[a.stage] : 0, it1 = staged ? a.list->stage_begin[a.stage + 1] : n_items;
    const int blk0 = staged && a.stage > 0 ? a.cuts[a.stage - 1] : 0, blk1 = staged && a.stage < a.n_cuts ? a.cuts[a.stage] : B;
    if (it1 > it0) {
        const int lrc = with_tile(a.max_radius, a.fma, [&](auto tag) {
            // the kernel's radius switch has no path for a radius above its tile's RMAX (blur_dispatch)
            if (a.max_radius > decltype(tag)::type::RMAX)
                return mst::fail(MST_E_ARG, "blur radius %d: the launch's tile is built for radii <= %d", a.max_radius,
                                 (int)decltype(tag)::type::RMAX);
            return launch_scale_space<typename decltype(tag)::type, BAND>(
                a.c, a.nz, src, a.CH, d_lv, a.found, a.found_cap, a.found_count, partial + (size_t)it0 * nt * 2, nt, a.skip_empty,
                d_items + it0, it1 - it0, s);
        });
        if (lrc != MST_OK) return lrc;
    }
    // a block's tiles are its own items and shared ones of the block before it: complete once its stage has run
    if (blk1 > blk0) {
        stats_reduce_kernel<<<dim3(nt, blk1 - blk0), 256, 0, s>>>(partial, npos, d_sop + (size_t)blk0 * npos, nt,
                                                                a.level_stats + (size_t)blk0 * MST_MAX_TESTED * 2);
        MST_LAUNCH_CHECK();
    }
    if (!captured) MST_HIP(a.list->used.record(s));
    return MST_OK;
}

// the signature of a fused launch for graph replay: every scalar / pointer argument, the block origins, the level table
static std::vector<int64_t> launch_signature(const BandSrc &src, const int64_t *starts, int B, int CH, const mst_levels *lv,
                                             const void *found, uint32_t found_cap, const void *found_count,
                                             const void *level_stats, int flags, const void *workspace, uint64_t workspace_bytes,
                                             int dev) {
    std::vector<int64_t> sig;
    const size_t lv_words = (sizeof(mst_levels) + 7) / 8;
    sig.reserve((size_t)B + 16 + lv_words);
    for (const void *p : {(const void *)src.band, (const void *)src.band2, found, found_count, level_stats,
                          (const void *)src.nz_count, workspace})
        sig.push_back((int64_t)(intptr_t)p);
    for (int64_t v : {(int64_t)src.n, (int64_t)src.dpx, (int64_t)src.split, (int64_t)B, (int64_t)CH, (int64_t)found_cap,
                      (int64_t)flags, (int64_t)workspace_bytes, (int64_t)dev})
        sig.push_back(v);
    sig.insert(sig.end(), starts, starts + B);
    sig.resize(sig.size() + lv_words, 0);
    memcpy(&sig[sig.size() - lv_words], lv, sizeof(mst_levels));
    return sig;
}

// MST_FLAG_GRAPH: a launch whose every argument repeats (same buffers, same blocks, same level table) is captured into a
// hipGraph the second time it is seen and REPLAYED from then on (mst::ReplayCache) -- one hipGraphLaunch instead of ~16 runtime
// calls (four uploads, two memsets, two kernels and their bookkeeping) in front of the fused kernel.  That matters for small
// launches: six blocks of 2000 x 2000 are 1.75 ms of kernel and the enqueue was 0.07 ms during which the GPU waited.  Band
// source only; staged launches are never captured.  This is the shared body of mst_scale_space (dense blocks) and of
// mst_scale_space_band and its kin (blocks cut out of the band on the fly).
template <bool BAND>
static int scale_space_impl(const double *c, const uint8_t *nz, BandSrc src, const int64_t *starts_host, int32_t B,
                            int32_t CH, const mst_levels *lv, mst_found *found, uint32_t found_cap,
                            uint32_t *found_count, double *level_stats, int32_t flags, void *workspace,
                            uint64_t workspace_bytes, void *stream, const char *who, const int32_t *cuts = nullptr,
                            int32_t n_cuts = 0, int32_t stage = -1) {
    const bool staged = stage >= 0;
    if (staged) flags &= ~MST_FLAG_GRAPH;
    const int skip_empty = (flags & MST_FLAG_SKIP_EMPTY) ? 1 : 0;
    const bool fma = (flags & MST_FLAG_FMA) != 0;
    int mr = 0, nt = 0;
    int rc = check_levels(lv, &mr, &nt);
    if (rc != MST_OK) return rc;
    if (!found || !found_count || !level_stats || !workspace || B <= 0 || B > 65535 || CH <= 0 ||
        (int64_t)CH * CH > 0xFFFFFFFFLL)
        return mst::fail(MST_E_ARG, "%s: bad argument", who);
    const uint64_t need = mst_scale_space_workspace_bytes(B, CH, lv);
    if (workspace_bytes < need)
        return mst::fail(MST_E_ARG, "%s: workspace too small (%llu < %llu bytes)", who,
                         (unsigned long long)workspace_bytes, (unsigned long long)need);
    hipStream_t s = mst::as_stream(stream);
    DevLevels h;
    if ((rc = make_dev_levels(lv, who, &h)) != MST_OK) return rc;
    if (fma && mr > TileDefault::RMAX)
        return mst::fail(MST_E_ARG, "%s: MST_FLAG_FMA is only built for blur radii <= %d", who, TileDefault::RMAX);

    static thread_local mst::ReplayCache graphs(4, "launch");
    mst::ReplayCache::Sight sight = mst::ReplayCache::kFirst;
    if (BAND && graphs.usable(flags, s)) {
        int dev = 0;
        MST_HIP(hipGetDevice(&dev));
        sight = graphs.look(launch_signature(src, starts_host, B, CH, lv, found, found_cap, found_count, level_stats, flags,
                                             workspace, workspace_bytes, dev));
        mst::note("scale_space graph B=%d CH=%d n=%lld dpx=%d cap=%u flags=%d band=%p found=%p count=%p stats=%p nz=%p ws=%p -> %s", B, CH,
                  (long long)src.n, (int)src.dpx, found_cap, flags, (const void *)src.band, (const void *)found, (const void *)found_count,
                  (const void *)level_stats, (const void *)src.nz_count, workspace, mst::ReplayCache::name(sight));
        if (sight == mst::ReplayCache::kReplay) return graphs.replay(s);
    }

    static thread_local WorkListCache lists;
    WorkList *wl = nullptr;
    rc = lists.find_or_build(mr, starts_host, B, CH, BAND ? src.dpx : -1, BAND && !(flags & MST_FLAG_NO_SHARE), BAND && skip_empty,
                             staged, cuts, n_cuts, &wl);
    if (rc != MST_OK) return rc;
    if (!(flags & MST_FLAG_GRAPH))
        mst::note("scale_space plain B=%d CH=%d cap=%u flags=%d found=%p count=%p stats=%p ws=%p items=%d", B, CH, found_cap, flags,
                  (const void *)found, (const void *)found_count, (const void *)level_stats, workspace, (int)wl->items.size());
    const Launch a = {c, nz, src, starts_host, B, CH, mr, nt, skip_empty, fma, &h, found, found_cap, found_count, level_stats,
                      static_cast<char *>(workspace), wl, cuts, n_cuts, stage};
    if (sight != mst::ReplayCache::kCapture) return enqueue_launch<BAND>(a, nullptr, s);
    // everything the graph's copy node will read goes into page-locked memory the entry owns: the tables, packed
    const size_t image_bytes = Workspace(B, wl->items.size(), (size_t)B * wl->npos).partial;
    return graphs.capture(who, s, image_bytes, [&](char *image) { return enqueue_launch<BAND>(a, image, s); });
}

extern "C" int mst_scale_space(const double *c, const uint8_t *nz, int32_t B, int32_t CH, const mst_levels *lv,
                               mst_found *found, uint32_t found_cap, uint32_t *found_count, double *level_stats,
                               int32_t flags, void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("launch: mst_scale_space");
    if (!c || !nz) return mst::fail(MST_E_ARG, "mst_scale_space: bad argument");
    BandSrc none = {nullptr, 0, 0, nullptr, nullptr, nullptr, INT_MAX};
    return scale_space_impl<false>(c, nz, none, nullptr, B, CH, lv, found, found_cap, found_count, level_stats, flags,
                                   workspace, workspace_bytes, stream, "mst_scale_space");
}

extern "C" int mst_scale_space_band(const double *band, int64_t n, int32_t dpx, const int64_t *starts, int32_t B,
                                    int32_t CH, const mst_levels *lv, mst_found *found, uint32_t found_cap,
                                    uint32_t *found_count, double *level_stats, uint32_t *nz_count, int32_t flags,
                                    void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("launch: mst_scale_space_band");
    if (!band || !starts || !nz_count || n <= 0 || dpx < 0)
        return mst::fail(MST_E_ARG, "mst_scale_space_band: bad argument");
    BandSrc src = {band, n, dpx, nullptr, nz_count, nullptr, INT_MAX};
    return scale_space_impl<true>(nullptr, nullptr, src, starts, B, CH, lv, found, found_cap, found_count, level_stats,
                                  flags, workspace, workspace_bytes, stream, "mst_scale_space_band");
}

extern "C" int mst_scale_space_band_stage(const double *band, int64_t n, int32_t dpx, const int64_t *starts, int32_t B,
                                          int32_t CH, const mst_levels *lv, mst_found *found, uint32_t found_cap,
                                          uint32_t *found_count, double *level_stats, uint32_t *nz_count, int32_t flags,
                                          void *workspace, uint64_t workspace_bytes, const int32_t *cuts, int32_t n_cuts,
                                          int32_t stage, void *stream) {
    MST_RANGE("launch: mst_scale_space_band_stage");
    if (!band || !starts || !nz_count || n <= 0 || dpx < 0 || n_cuts < 0 || (n_cuts > 0 && !cuts) || stage < 0 || stage > n_cuts)
        return mst::fail(MST_E_ARG, "mst_scale_space_band_stage: bad argument");
    for (int i = 0; i < n_cuts; ++i)
        if (cuts[i] <= (i ? cuts[i - 1] : 0) || cuts[i] >= B)
            return mst::fail(MST_E_ARG, "mst_scale_space_band_stage: cuts must be ascending block indices in (0, B)");
    BandSrc src = {band, n, dpx, nullptr, nz_count, nullptr, INT_MAX};
    return scale_space_impl<true>(nullptr, nullptr, src, starts, B, CH, lv, found, found_cap, found_count, level_stats,
                                  flags, workspace, workspace_bytes, stream, "mst_scale_space_band_stage", cuts, n_cuts, stage);
}

extern "C" int mst_scale_space_band_pair(const double *band1, const double *band2, int32_t split, int64_t n, int32_t dpx,
                                         const int64_t *starts, int32_t B, int32_t CH, const mst_levels *lv, mst_found *found,
                                         uint32_t found_cap, uint32_t *found_count, double *level_stats, uint32_t *nz_count,
                                         int32_t flags, void *workspace, uint64_t workspace_bytes, void *stream) {
    MST_RANGE("launch: mst_scale_space_band_pair");
    if (!band1 || !band2 || !starts || !nz_count || n <= 0 || dpx < 0 || split < 1 || split >= B)
        return mst::fail(MST_E_ARG, "mst_scale_space_band_pair: bad argument (0 < split < B)");
    if (starts[split] > starts[split - 1] && starts[split] - starts[split - 1] < CH)
        return mst::fail(MST_E_ARG, "mst_scale_space_band_pair: block %d (the second band's first) must not continue block %d "
                         "(tiles are shared between CONSECUTIVE overlapping blocks of one band only)", split, split - 1);
    BandSrc src = {band1, n, dpx, nullptr, nz_count, band2, split};
    return scale_space_impl<true>(nullptr, nullptr, src, starts, B, CH, lv, found, found_cap, found_count, level_stats,
                                  flags, workspace, workspace_bytes, stream, "mst_scale_space_band_pair");
}
