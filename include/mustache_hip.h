/*
 * mustache_hip.h -- C ABI of libmustache_hip.so, the MI355X (gfx950) implementation of the per-block
 * scale-space loop-calling hot path of ay-lab/mustache.
 *
 * The reference has no FFI / plugin interface (it is pure Python over SciPy); its narrowest stable seam is the
 * Python call  mustache(c, chromosome, chromosome2, res, pval_weights, start, end, mask_size, distance_in_px,
 * octave_values, st, pt)  (reference mustache/mustache.py:697-698), invoked per dense block by process_block
 * (:945-960) from regulator (:853-937).  This header is the set of entry points a binding for that seam needs;
 * each one names the reference code it replaces.  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - every pointer marked "dev" is a device (HBM) pointer owned by the caller (e.g. a torch tensor's
 *     data_ptr()); "host" pointers are ordinary host memory.  Nothing is allocated or freed behind the ABI
 *     except small internal scratch that is cached per (device, stream).
 *   - `stream` is a hipStream_t passed as void*; NULL = the default stream.  All work is enqueued
 *     asynchronously on it; the functions do not synchronise unless stated.
 *   - return value: 0 = ok, <0 = error (MST_E_*); mst_last_error() returns a thread-local message.
 *     No C++ exception crosses the ABI.
 *   - all arithmetic is IEEE float64 without fused multiply-add, in the evaluation order of the SciPy
 *     kernels the reference calls, so DoG values are bit-identical to the reference's.
 */
#ifndef MUSTACHE_HIP_H
#define MUSTACHE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MST_ABI_VERSION 3
/* Counts the entry points added since MST_ABI_VERSION last changed (additions leave every existing signature as it is, so the
 * version stays).  A binding compares both numbers before it looks any symbol up: a library older than the binding then fails
 * with the version message, not with a missing symbol.  1: mst_abi_revision itself, mst_balance_newton,
 * mst_balance_newton_workspace_bytes.  mst_balance_apply_pairs was added at revision 1 as well: tests/test_newton_reference.py
 * pins the refusal message of a stale library to the numbers 3.1 / 3.2, so the count can move only together with that test; a
 * library from before the addition is refused by its missing symbol. */
#define MST_ABI_REVISION 1

/* Stability of the entry points (annotations only: both expand to nothing and every symbol is exported).
 *   MST_STABLE   : the boundary SURVEY section 8(b) asks for -- scatter / prologue / blur / scale space / found records, their
 *                  finish (p-values, summary), the tail (BH, selection, features, diagonal means, clustering), the band-direct
 *                  forms of the same, the two-sample entry points.  Signature and meaning change only with MST_ABI_VERSION.
 *                  A binding written against INTEGRATION.md uses these only.
 *   MST_INTERNAL : fast paths of THIS package's own engine (no-wait / graph-replayed forms, batched "multi" forms, work-list
 *                  queries, packed-record and .hic-row scatters, the verifying scatter).  Exported because the Python host
 *                  binds them through ctypes, but they may change or disappear in any build without a version bump; every one
 *                  has a stable equivalent that returns the same results. */
#define MST_STABLE
#define MST_INTERNAL

#define MST_OK 0
#define MST_E_ARG (-1)      /* bad argument (null pointer, size, unsupported radius ...) */
#define MST_E_HIP (-2)      /* a HIP runtime call failed; message has hipGetErrorString */
#define MST_E_OVERFLOW (-3) /* an output buffer capacity was exceeded (caller re-runs with a larger one) */
#define MST_E_NONFINITE (-4)/* non-finite DoG statistics (the reference raises ValueError in expon.fit) */

/* mst_scale_space flags */
#define MST_FLAG_SKIP_EMPTY 1 /* tiles that contain no nz pixel are not computed (identical outputs, less work) */
#define MST_FLAG_NO_SHARE 4   /* band source only: compute every tile once PER BLOCK on the block's own tile lattice (the form
                               * of rounds 1 and 2).  Default: a tile that lies inside two consecutive blocks with its whole
                               * blur halo is computed once and delivered to both (identical records; see mst_scale_space_band) */
#define MST_FLAG_GRAPH 8      /* band source only: when a call repeats with EVERY argument unchanged (same device buffers, same
                               * block origins, same level table, same stream kind) it is captured into a hipGraph the second
                               * time and replayed afterwards -- one graph launch instead of ~16 runtime calls in front of the
                               * fused kernel (small launches are latency-bound).  Identical results; ignored on the legacy
                               * default stream (it cannot be captured) and by PROFILE builds. */
#define MST_FLAG_NO_WAIT 16   /* mst_found_finish only: enqueue and return -- the caller queues more work behind it (the two-sample
                               * path: pair p-values, BH, gathers), synchronises ONCE and then asks mst_found_summary_status */
#define MST_BH_RETRY 0xFFFFFFFFu /* mst_bh_select_nowait: out_count of a block whose candidate subset exceeds lds_records */
#define MST_FLAG_FMA 2        /* OPT-IN relaxed arithmetic: fuse the multiply-add of each tap pair.  DoG values then differ
                                 from the reference's by ~1e-16 relative (instead of being bit-identical); default off */

#define MST_MAX_LEVELS 64   /* octaves * (s + 2) */
#define MST_MAX_RADIUS 32
#define MST_MAX_TESTED 48   /* octaves * (s - 1) */

/* The Gaussian level table: what mustache.py:714-752 passes to scipy.ndimage.gaussian_filter, already reduced
 * by the host to integer radii and normalised taps (scipy/ndimage/_filters.py:226-236, :314-316).
 * Level index l = octave * levels_per_octave + (k - 1), k = 1 .. levels_per_octave. */
typedef struct mst_levels {
    int32_t n_octaves;
    int32_t levels_per_octave;                           /* s + 2 = 12 in the reference (s = 10, mustache.py:711) */
    int32_t radius[MST_MAX_LEVELS];
    int32_t _pad;
    double sigma[MST_MAX_LEVELS];
    double taps[MST_MAX_LEVELS][MST_MAX_RADIUS + 1];     /* taps[l][0] = centre, taps[l][j] = weight at +-j */
} mst_levels;

/* One "found" pixel = an nz pixel whose (x, y, sigma) sieve fired at least once (mustache.py:760-768). */
typedef struct mst_found {
    uint32_t pixel;     /* row * CH + col inside the block */
    uint32_t level;     /* 1 + octave * (s - 1) + (i - 3), i = the reference's loop index (mustache.py:744) */
    double value;       /* vAll: the winning DoG response */
} mst_found;

MST_STABLE int mst_abi_version(void);
MST_STABLE int mst_abi_revision(void);
MST_STABLE const char *mst_last_error(void);

/* mustache.py:919-924 (regulator's COO -> dense block scatter) for B blocks at once.
 * x, y, v: dev, upper-triangular COO in chromosome bin units; starts: host, B block origins.
 * c: dev [B][CH][CH] float64, fully overwritten (zero + scatter).  Entries with start <= x, y < start + CH go
 * into block b at (x - start, y - start), exactly like `cc[xc, yc] = vc`.  Duplicate (x, y) entries must not
 * occur (the reference takes the last one; readers never produce duplicates). */
MST_STABLE int mst_scatter_blocks(const int64_t *x, const int64_t *y, const double *v, int64_t nnz,
                       const int64_t *starts, int32_t B, int32_t CH, double *c, void *stream);

/* mustache.py:699-706 (prologue of mustache()): nz = (c != 0) & (col - row >= 4) taken before the fills,
 * then c[col-row <= 4] = 2 and, if intra != 0, c[col-row >= dpx+1] = 2.  In place on c.
 * nz: dev [B][CH][CH] uint8 (1 = tested pixel); nz_count: dev [B] uint32, overwritten with sum(nz). */
MST_STABLE int mst_block_prologue(double *c, uint8_t *nz, uint32_t *nz_count, int32_t B, int32_t CH, int32_t dpx,
                       int32_t intra, void *stream);

/* scipy.ndimage.gaussian_filter(c, sigma, truncate=t, order=0) as called at mustache.py:719/725/734/751, for a
 * batch of B images of H x W float64: axis 0 then axis 1, mode='reflect', symmetric pair-sum order.
 * taps: host, radius+1 doubles (centre first).  tmp: dev scratch, same size as `in`.  Bring-up / parity kernel
 * and the building block of the general (any radius) path. */
MST_STABLE int mst_gauss_blur(const double *in, double *out, double *tmp, int32_t B, int32_t H, int32_t W,
                   const double *taps, int32_t radius, void *stream);

/* mustache.py:714-772, the whole sigma loop of mustache() fused for B prologue'd blocks:
 * the 2 x 12 Gaussian blurs, the 11 DoG levels per octave, their zero-padded 3x3 maxima, the 5-term
 * (x, y, sigma) sieve with `best` carried across levels and octaves, and the per-level min / sum of |D| over nz
 * that scipy.stats.expon.fit needs (:755).
 *   c, nz       : dev, from mst_block_prologue
 *   lv          : host
 *   found       : dev [B][found_cap] records, unordered within a block
 *   found_count : dev [B] uint32, overwritten; a count > found_cap means records were dropped -> caller
 *                 must re-run with a larger capacity (mst_found_pvalues reports MST_E_OVERFLOW)
 *   level_stats : dev [B][MST_MAX_TESTED][2] float64, overwritten: {min |D_c| over nz, sum |D_c| over nz} per
 *                 tested level (deterministic reduction order)
 *   flags       : MST_FLAG_SKIP_EMPTY | MST_FLAG_FMA (see above); 0 = dense, exact
 *   workspace   : dev scratch of at least mst_scale_space_workspace_bytes(B, CH, lv) bytes
 */
MST_STABLE int mst_scale_space(const double *c, const uint8_t *nz, int32_t B, int32_t CH, const mst_levels *lv,
                    mst_found *found, uint32_t found_cap, uint32_t *found_count, double *level_stats,
                    int32_t flags, void *workspace, uint64_t workspace_bytes, void *stream);

/* Bytes of device scratch mst_scale_space needs for (B, CH, lv): the level table plus per-tile partial
 * statistics.  Returns 0 on bad arguments. */
MST_STABLE uint64_t mst_scale_space_workspace_bytes(int32_t B, int32_t CH, const mst_levels *lv);

/* mustache.py:755-756 for the found pixels only (deferred p-value; bit-for-bit the same quantity):
 * loc = min|D|, scale = mean|D| - loc per tested level, p = 1 - (-expm1(-(value - loc)/scale)).
 * pval: dev [B][found_cap] float64.  fit: dev [B][MST_MAX_TESTED][2] float64 out = {loc, scale}.
 * Synchronises the stream and returns MST_E_OVERFLOW / MST_E_NONFINITE when a block overflowed its record
 * capacity or produced non-finite statistics. */
MST_STABLE int mst_found_pvalues(const mst_found *found, uint32_t found_cap, const uint32_t *found_count,
                      const uint32_t *nz_count, const double *level_stats, int32_t B, int32_t n_tested,
                      double *pval, double *fit, void *stream);

/* mst_found_pvalues with everything a caller needs next delivered in the SAME round trip (one stream synchronisation per launch
 * instead of one per quantity).  summary_host (page-locked, mst_found_summary_bytes(B) bytes; scratch_dev: device memory of the
 * same size) receives {int32 flags, pad to 16 bytes | uint32 found_count[B] padded to an even count | uint32 nz_count[B]
 * likewise | double fit[B][MST_MAX_TESTED][2]} in one copy.  pack_pitch > 0: the first pack_pitch records of every block are
 * also written as three narrow, densely pitched device arrays pix_out int32 / lvl_out uint8 / pv_out float64 [B][pack_pitch]
 * (pixel index, 1-based tested level, p-value) -- what a caller that downloads whole found sets wants; with pix_host /
 * lvl_host / pv_host (page-locked, same shapes; all three or none) they are copied to the host before the synchronisation, so a
 * caller whose pack_pitch (its guess of the largest count) is confirmed by the summary needs no second round trip.
 * flags: 0, or MST_FLAG_GRAPH (a call that repeats with every argument unchanged is replayed as one hipGraph: for small,
 * latency-bound launches; it slows large pipelined ones), and / or MST_FLAG_NO_WAIT (no synchronisation, no status: the call
 * returns once everything is queued; after the caller's own synchronisation of `stream`, mst_found_summary_status(summary_host,
 * found_cap) gives the status this call would have returned).  Same error returns as mst_found_pvalues. */
MST_STABLE uint64_t mst_found_summary_bytes(int32_t B);
MST_STABLE int mst_found_summary_status(const void *summary_host, uint32_t found_cap);
MST_STABLE int mst_found_finish(const mst_found *found, uint32_t found_cap, const uint32_t *found_count, const uint32_t *nz_count,
                     const double *level_stats, int32_t B, int32_t n_tested, double *pval, double *fit, uint32_t pack_pitch,
                     int32_t *pix_out, uint8_t *lvl_out, double *pv_out, void *scratch_dev, void *summary_host,
                     int32_t *pix_host, uint8_t *lvl_host, double *pv_host, int32_t flags, void *stream);

/* mustache.py:778, multipletests(p, method='fdr_bh') per block, on the device: q[b][i] for the first count[b] records of
 * each block (sort ascending, p * m / rank with NumPy's operation order, suffix minimum, clip at 1, back to record order).
 * pval, q: dev [B][cap]; count: dev [B]; workspace: dev, >= mst_bh_workspace_bytes(B, cap). */
MST_STABLE uint64_t mst_bh_workspace_bytes(int32_t B, uint32_t cap);
MST_STABLE int mst_bh_fdr(const double *pval, const uint32_t *count, int32_t B, uint32_t cap, double *q, void *workspace,
               uint64_t workspace_bytes, void *stream);

/* BH + selection in one call, restricted to the records that can be selected (what the per-chromosome pipeline uses):
 * the records with q < threshold and their q-values, bit-identical to mst_bh_fdr + mst_select_below, but only a small
 * subset is sorted: the selected records are the BH ranks 1..j*, all below p = threshold * j* / m, and a histogram of the
 * p-values bounds j* from above (fixed point of J -> #{p < threshold * J / m}) -- typically a few hundred of ~150 000
 * records, sorted by one workgroup in LDS; the suffix minimum over the rest is >= threshold, and the global test count
 * m = found_count[b] enters every division.  A block whose subset exceeds 4096 records (threshold near 1) goes through the
 * segmented radix sort instead, same results.  Synchronises `stream` once (the subset sizes choose the route).  Outputs as
 * mst_select_below; workspace from mst_bh_workspace_bytes(B, found_cap).  (mustache.py:778-797) */
MST_STABLE int mst_bh_select(const mst_found *found, const double *pval, const uint32_t *found_count, int32_t B, uint32_t found_cap,
                  double threshold, uint32_t out_cap, uint32_t *out_pixel, uint32_t *out_level, double *out_q,
                  uint32_t *out_count, void *workspace, uint64_t workspace_bytes, void *stream);
/* The same, and also the selected records' positions in their block's found list (out_index: dev [B][out_cap] u32), so that
 * further per-record arrays (the pair p-values of the two-sample path) can be gathered for the selected records only. */
MST_STABLE int mst_bh_select_records(const mst_found *found, const double *pval, const uint32_t *found_count, int32_t B,
                          uint32_t found_cap, double threshold, uint32_t out_cap, uint32_t *out_pixel, uint32_t *out_level,
                          double *out_q, uint32_t *out_index, uint32_t *out_count, void *workspace,
                          uint64_t workspace_bytes, void *stream);

/* mst_bh_select_records (out_index may be NULL) WITHOUT the host synchronisation: the in-LDS sort is launched for every block,
 * sized for candidate subsets of up to `lds_records` records (a power of two <= 4096; 12 bytes of LDS each: the caller's guess,
 * e.g. twice what its last launch needed), and a block whose subset is larger gets out_count[b] = MST_BH_RETRY instead of a
 * count -- the caller, once it has synchronised for out_count anyway, then runs mst_bh_select / mst_bh_fdr + mst_select_below
 * for the launch.  Lets a latency-bound caller (the two-sample path on a few blocks) queue everything behind the fused
 * kernels and wait once. */
MST_INTERNAL int mst_bh_select_nowait(const mst_found *found, const double *pval, const uint32_t *found_count, int32_t B,
                         uint32_t found_cap, double threshold, uint32_t out_cap, uint32_t *out_pixel, uint32_t *out_level,
                         double *out_q, uint32_t *out_index, uint32_t *out_count, uint32_t lds_records, void *workspace,
                         uint64_t workspace_bytes, void *stream);

/* mustache.py:789-797 (selection of the pixels with o < pt) on the device: the found records of each block whose q-value
 * is below `threshold`, compacted into out_pixel / out_level / out_q [B][out_cap] (order within a block unspecified).
 * out_count: dev [B], overwritten; a count > out_cap means records were dropped -> re-run with a larger capacity.
 * Found pixels with q >= pt are never candidates and never a cluster's representative (mustache.py:843-848 takes the
 * arg-min of o, and every cluster holds a candidate), so the host tail needs nothing else. */
MST_STABLE int mst_select_below(const mst_found *found, const double *q, const uint32_t *found_count, int32_t B,
                     uint32_t found_cap, double threshold, uint32_t out_cap, uint32_t *out_pixel, uint32_t *out_level,
                     double *out_q, uint32_t *out_count, void *stream);

/* mustache.py:800-811 + :824 inputs for a list of candidate pixels of ONE block b:
 * cnt1[i] = sum nz[x-s:x+s+1, y-s:y+s+1], cnt2[i] = same with 2s (Python slice semantics: a window whose start
 * is negative is empty -> 0; windows are clipped at the far edge), cval[i] = c[x, y].
 * pixel, half: dev [n] (half = ceil(scale)); outputs dev [n]. */
MST_STABLE int mst_candidate_features(const double *c, const uint8_t *nz, int32_t CH, int32_t b, const uint32_t *pixel,
                           const int32_t *half, int32_t n, uint32_t *cnt1, uint32_t *cnt2, double *cval,
                           void *stream);

/* mustache.py:816-823: gather diagonals of block b for the diagonal-mean filter.
 * diag_k: dev [n] offsets k >= 0; out: dev [n][CH] float64, row i = c[r, r+k] for r < CH-k, zero padded. */
MST_STABLE int mst_gather_diagonals(const double *c, int32_t CH, int32_t b, const int32_t *diag_k, int32_t n, double *out,
                         void *stream);

/* mustache.py:816-824: mean_out[i] = np.mean(dg[dg != 0]) for dg = diagonal diag_k[i] of block b -- the non-zero entries
 * summed in NumPy's pairwise order (numpy/_core/src/umath/loops_utils.h.src), so the value is bit-identical to the
 * reference's and only nd doubles leave the device.  A diagonal without non-zero entries gives NaN (as np.mean does).
 * diag_k: dev [nd]; mean_out: dev [nd].  CH*8 bytes must fit the LDS (CH <= 20000). */
MST_STABLE int mst_diag_means(const double *c, int32_t CH, int32_t b, const int32_t *diag_k, int32_t nd, double *mean_out,
                   void *stream);

/* ---- diagonal-major band layout ---------------------------------------------------------------------------------
 * band[d * n + i] = value of pixel (i, i + d), d = 0 .. dpx+1, i = 0 .. n-1; 0.0 = no contact.  dev, float64. */

/* COO -> band: the per-diagonal `vals[x[indices]] = v[indices]` of mustache.py:633-635 for all diagonals at once.
 * band is zero-filled first; entries with |y - x| > dpx + 1 are ignored; x, y may come in either order. */
MST_STABLE int mst_band_from_coo(const int64_t *x, const int64_t *y, const double *v, int64_t nnz, int64_t n, int32_t dpx,
                      double *band, void *stream);

/* The same scatter from the packed records of the native `.hic` reader (include/mustache_io.h,
 * mst_hic_read_intra_packed: binX, binY - binX >= 0, float32 value; dev arrays): band[dist][x] = (double)v.  What
 * read_hic_file() -> `cc[xc, yc] = vc` amounts to (mustache.py:300-396, :921-924) without an int64 / float64 COO triple on
 * the host or across PCIe.  band is zero-filled first; records with dist > dpx + 1 are ignored. */
MST_STABLE int mst_band_from_packed(const int32_t *x, const int32_t *dist, const float *v, int64_t nnz, int64_t n, int32_t dpx,
                         double *band, void *stream);

/* Slab-wise form of the same scatter for a streaming read (the reader hands over page-locked slabs of records while later
 * `.hic` blocks are still being inflated; with one process per GPU every rank scatters the slabs of all ranks): NO clearing
 * -- the caller zero-fills `band` once -- and the distance as int32 (dist_bytes = 4) or uint16 (dist_bytes = 2: 10 bytes
 * per record across PCIe; needs dpx + 1 <= 65535).  Slabs may be scattered in any order: a matrix holds every pixel once. */
MST_INTERNAL int mst_band_scatter_packed(const int32_t *x, const void *dist, int32_t dist_bytes, const float *v, int64_t nnz, int64_t n,
                            int32_t dpx, double *band, void *stream);

/* The device half of the RAW `.hic` read (include/mustache_io.h, mst_hic_rawstream_*): the rows of inflated blocks, record
 * bytes exactly as the file stores them, decoded, normalised, filtered and scattered by one kernel -- what hic-straw's
 * readBlock() and the record loop of read_hic_file() do on the host (mustache.py:328-333, :340-389), followed by
 * `cc[xc, yc] = vc` (:919-924).  payload: dev bytes of one slab (2-byte aligned); rows: dev [n_rows] mst_hic_row
 * (include/mustache_hicrow.h; offsets relative to `payload`); norm: dev [n_norm] float64 normalisation vector or NULL (no
 * division); per record: binX <= binY ordered, dropped when binY - binX > max_dist (< 0: no limit), when either bin lies
 * outside the vector, when value = (float)(count / (norm[binX] * norm[binY])) is NaN or <= 0, or when binY >= y_limit
 * (<= 0: no limit); kept: band[(binY - binX) * n + binX] = (double)value.  NO clearing -- the caller zero-fills `band`
 * ([dpx + 2][n]) once and may scatter slabs in any order.  stats: dev uint64 [4], accumulated with atomics (the caller zeroes
 * them): [0] max binY + 1 over the kept records, [1] kept records, [2] records the band cannot hold (binY >= n or distance >
 * dpx + 1: never written), [3] verify mismatches.  verify != 0: nothing is written; every record that would be kept is read
 * back and counted in stats[3] when its pixel holds another value (two records sharing a pixel: malformed input). */
MST_INTERNAL int mst_band_scatter_hic_rows(const void *payload, const void *rows, int32_t n_rows, const double *norm, int64_t n_norm,
                              int64_t max_dist, int64_t y_limit, int64_t n, int32_t dpx, double *band, uint64_t *stats,
                              int32_t verify, void *stream);

/* Read-back check of packed scatters: *mismatches (dev uint64, zeroed by the caller) += the number of records whose pixel
 * does not hold their value afterwards -- a pixel written by two records with different values (malformed input; the
 * reference's scatter keeps the last one, mustache.py:921-924) shows up for one of them whichever store won the race. */
MST_INTERNAL int mst_band_verify_packed(const int32_t *x, const void *dist, int32_t dist_bytes, const float *v, int64_t nnz, int64_t n,
                           int32_t dpx, const double *band, uint64_t *mismatches, void *stream);

/* band -> COO order: v[e] = band[|y-x|][min(x, y)]  (the `v[indices] = vals[x[indices]]` write-back, :669). */
MST_STABLE int mst_band_to_coo(const double *band, const int64_t *x, const int64_t *y, int64_t nnz, int64_t n, int32_t dpx,
                    double *v, void *stream);

/* normalize_sparse (mustache.py:622-686) on the band, out of place (band_in != band_out).
 *   local != 0 : branch A (:628-669), taken by the caller when (n - dpx) * res > 2e6; `window` = int(2e6 / res).
 *                (local == 1: the library picks the kernel -- the walking kernel (blocks of `window` samples along each
 *                diagonal, one scan per sample) for windows up to 4096, blocked sums (16-sample blocks) up to ~8400 and
 *                (32-sample blocks, samples only in LDS) up to 16384, and the strip form beyond (two strips of in-block
 *                partial sums + tile-local prefix sums of per-diagonal 32-sample block sums; windows up to 192 992 bins,
 *                resolutions down to ~11 bp), an error beyond that, with the limit in the message.
 *                local == 4: the strip form at any window >= 2 -- the cross-check of the forms above, in every build.
 *                PROFILE builds additionally accept local == 2 (blocked sums whatever the window) and local == 3 (round 1's
 *                segment kernel) as cross-checks; the product library refuses them.)
 *                Per diagonal d <= dpx+1: vals = v + 0.001; counts / sum / sum of squares over the zero-padded
 *                window [i - window/2, i - window/2 + window - 1] (np.convolve 'same'); local variance and mean
 *                with the global fallback below 30 samples or when non-finite; z = (vals - mean)/sqrt(var),
 *                non-finite -> 0, times 1 + log30(1 + global mean).
 *   local == 0 : branch B (:671-685): (v - mean)/std for d < min(dpx, n), other diagonals pass through.
 * diag_stats: dev [dpx+2][4] out = {global mean, global std, weight 1 + log30(1 + mean), entry count} per diagonal. */
MST_STABLE int mst_normalize_band(const double *band_in, double *band_out, int64_t n, int32_t dpx, int32_t window,
                       int32_t local, double *diag_stats, void *stream);

/* mustache.py:919-924 + :699-706 fused, for B blocks: dense filled blocks and the nz mask straight from the band
 * (intra-chromosomal).  starts: host [B]; c: dev [B][CH][CH]; nz: dev [B][CH][CH] uint8; nz_count: dev [B]. */
MST_STABLE int mst_blocks_from_band(const double *band, int64_t n, int32_t dpx, const int64_t *starts, int32_t B, int32_t CH,
                         double *c, uint8_t *nz, uint32_t *nz_count, void *stream);

/* ---- band-direct variants: the block is a window of the band, never materialised ---------------------------------------
 * Same results as mst_blocks_from_band + mst_scale_space / mst_candidate_features / mst_gather_diagonals, without the
 * [B][CH][CH] dense blocks (9 B per pixel written and read back, 18 GB for a 1 kb chr1). */

/* mustache.py:919-924 + :699-706 + :714-772 in one launch.  starts: host [B]; nz_count: dev [B] out = tested pixels per
 * block (what mst_found_pvalues needs).  Other arguments as mst_scale_space; workspace from mst_scale_space_workspace_bytes. */
MST_STABLE int mst_scale_space_band(const double *band, int64_t n, int32_t dpx, const int64_t *starts, int32_t B, int32_t CH,
                         const mst_levels *lv, mst_found *found, uint32_t found_cap, uint32_t *found_count,
                         double *level_stats, uint32_t *nz_count, int32_t flags, void *workspace,
                         uint64_t workspace_bytes, void *stream);
/* The same launch over blocks of TWO bands of one geometry (the two samples of diff_mustache.py:260-569, whose sigma loops
 * are independent): blocks [0, split) are windows of band1, blocks [split, B) of band2; starts: host [B] (the second band's block
 * origins usually repeat the first's; block `split` must not be a continuation of block split - 1: tiles are shared between
 * consecutive overlapping blocks of ONE band).  One launch instead of two: one set of uploads, one launch tail -- what a
 * latency-bound two-sample call on a few block pairs wants.  Everything else as mst_scale_space_band. */
MST_STABLE int mst_scale_space_band_pair(const double *band1, const double *band2, int32_t split, int64_t n, int32_t dpx,
                              const int64_t *starts, int32_t B, int32_t CH, const mst_levels *lv, mst_found *found,
                              uint32_t found_cap, uint32_t *found_count, double *level_stats, uint32_t *nz_count, int32_t flags,
                              void *workspace, uint64_t workspace_bytes, void *stream);
/* mst_scale_space_band (mustache.py:919-924 + :699-706 + :714-772) in STAGES (this package's engine; identical results): cuts[0 .. n_cuts) are ascending block indices in
 * (0, B); stage i (0 <= i <= n_cuts) enqueues the work items of blocks [cuts[i-1], cuts[i]) of the launch's ONE work list -- tile
 * sharing crosses the cuts, which separate launches over the same ranges would lose -- followed by the level statistics of
 * those blocks.  Call the stages in ascending order on one stream with identical arguments; stage 0 also uploads the tables
 * and zeroes the counters.  After stage i the outputs of the blocks below cuts[i] are final, so their mst_found_finish can
 * run on another stream (behind an event) while stage i + 1 executes.  MST_FLAG_GRAPH is ignored. */
MST_INTERNAL int mst_scale_space_band_stage(const double *band, int64_t n, int32_t dpx, const int64_t *starts, int32_t B, int32_t CH,
                                            const mst_levels *lv, mst_found *found, uint32_t found_cap, uint32_t *found_count,
                                            double *level_stats, uint32_t *nz_count, int32_t flags, void *workspace,
                                            uint64_t workspace_bytes, const int32_t *cuts, int32_t n_cuts, int32_t stage,
                                            void *stream);
/* How many of a block's tiles mst_scale_space_band launches with MST_FLAG_SKIP_EMPTY (those whose pixels can reach the tested
 * band 4 <= col - row <= dpx + 1), on the block's own tile lattice; *tiles_total = all tiles of the block.  Host only. */
MST_INTERNAL int mst_scale_space_band_tiles(int32_t CH, int32_t dpx, const mst_levels *lv, int32_t *tiles_total);
/* The work list mst_scale_space_band would build for these blocks and flags (host only): returns the number of workgroups it
 * launches; *tiles = the tiles the blocks would run one by one (workgroups + shared), *shared = tiles computed once for two
 * consecutive blocks.  Consecutive blocks of a chromosome overlap by half their edge (mustache.py:899-908); a tile that lies
 * inside both with its whole blur halo sees the same pixels in either, so its records and statistics are computed once and
 * delivered to both -- unless MST_FLAG_NO_SHARE is set. */
MST_INTERNAL int mst_scale_space_band_items(const int64_t *starts, int32_t B, int32_t CH, int32_t dpx, const mst_levels *lv, int32_t flags,
                               int64_t *tiles, int64_t *shared);

/* mst_candidate_features / mst_gather_diagonals / mst_diag_means for the block that starts at bin `start` of the band. */
MST_STABLE int mst_candidate_features_band(const double *band, int64_t n, int32_t dpx, int64_t start, int32_t CH,
                                const uint32_t *pixel, const int32_t *half, int32_t ncand, uint32_t *cnt1,
                                uint32_t *cnt2, double *cval, void *stream);
/* the same for candidates of several blocks in ONE launch: starts: dev [ncand], the block origin of each candidate */
MST_INTERNAL int mst_candidate_features_band_multi(const double *band, int64_t n, int32_t dpx, const int64_t *starts, int32_t CH,
                                      const uint32_t *pixel, const int32_t *half, int32_t ncand, uint32_t *cnt1,
                                      uint32_t *cnt2, double *cval, void *stream);
MST_STABLE int mst_gather_diagonals_band(const double *band, int64_t n, int32_t dpx, int64_t start, int32_t CH,
                              const int32_t *diag_k, int32_t nd, double *out, void *stream);
MST_STABLE int mst_diag_means_band(const double *band, int64_t n, int32_t dpx, int64_t start, int32_t CH, const int32_t *diag_k,
                        int32_t nd, double *mean_out, void *stream);
/* the same for diagonals of several blocks in ONE launch: starts: dev [nd], the block origin of each requested diagonal */
MST_INTERNAL int mst_diag_means_band_multi(const double *band, int64_t n, int32_t dpx, const int64_t *starts, int32_t CH,
                              const int32_t *diag_k, int32_t nd, double *mean_out, void *stream);

/* mustache.py:830-848 for B blocks in one launch: 8-connected clustering of every surviving candidate with its 3 x 3 halo
 * (scipy.ndimage.label numbering: components in raster order of their first pixel) and, per component, the FIRST arg-min of
 * o in raster order over its member pixels.  Inputs (dev): per block b the SELECTED records (q < pt) sorted by pixel --
 * sel_pix / sel_q [sel_off[b], sel_off[b+1]) -- and the positions of the candidates that survived the filters among them,
 * ascending -- cand_pos [cand_off[b], cand_off[b+1]).  Output: rep_pos[cand_off[b] + k] = position (in block b's records) of
 * the representative of its k-th component, rep_count[b] components.  workspace: mst_cluster_workspace_bytes(total
 * candidates).  Only selected records can be an arg-min (o >= 1 elsewhere), which is why they suffice. */
MST_STABLE uint64_t mst_cluster_workspace_bytes(uint32_t n_candidates);
MST_STABLE int mst_cluster_representatives(const uint32_t *sel_pix, const double *sel_q, const uint32_t *sel_off,
                                const uint32_t *cand_pos, const uint32_t *cand_off, int32_t B, int32_t CH,
                                uint32_t n_candidates, uint32_t *rep_pos, uint32_t *rep_count, void *workspace,
                                uint64_t workspace_bytes, void *stream);

/* ---- two-sample (differential) caller, reference mustache/diff_mustache.py:260-569 ------------------------------------
 * The per-sample sigma loops are mst_scale_space on both samples' blocks.  The entry points below add what
 * diff_mustache() computes on the difference image.  NB (reference behaviour, kept): the difference image's DoG is
 * assigned once per octave (diff_mustache.py:336) and never advanced inside the level loop, so every tested level of an
 * octave uses D_2 = G_2 - G_3 of that octave; the host produces G_2 and G_3 with mst_gauss_blur. */

/* diff_mustache.py:262-276 on already filled blocks: nzb = nz1 & nz2; cd = nzb ? c1 - c2 : 0; nzb_count[b] = sum. */
MST_STABLE int mst_diff_image(const double *c1, const double *c2, const uint8_t *nz1, const uint8_t *nz2, int32_t B, int32_t CH,
                   double *cd, uint8_t *nzb, uint32_t *nzb_count, void *stream);

/* scipy.stats.norm.fit((a - b)[mask]) per image (diff_mustache.py:371): fit[i] = {mean, sqrt(mean((x - mean)^2))},
 * i < B images of npx pixels; fixed summation order.  workspace: dev, >= 2048 * B bytes. */
MST_STABLE int mst_masked_normfit(const double *a, const double *b, const uint8_t *mask, const uint32_t *mask_count, int32_t B,
                       int64_t npx, double *fit, void *workspace, uint64_t workspace_bytes, void *stream);

/* diff_mustache.py:372-385 for the found pixels of one sample: ppair = 2 * min(cdf, 1 - cdf), cdf = ndtr((x-loc)/scale),
 * x = (g2 - g3)[octave of the record's level][pair b][pixel]; non-finite cdf -> 1.
 * found / found_count / ppair are the arrays of a 2B-block mst_scale_space launch (sample 1 = blocks [0, B), sample 2 =
 * [B, 2B)); sample_offset = 0 or B selects the sample.  g2, g3: dev [n_octaves][B][CH][CH]; fit: dev [n_octaves][B][2]. */
MST_STABLE int mst_pair_pvalues(const mst_found *found, uint32_t found_cap, const uint32_t *found_count, const double *g2,
                     const double *g3, const double *fit, int32_t B, int32_t CH, int32_t n_octaves,
                     int32_t tested_per_octave, int32_t sample_offset, double *ppair, void *stream);

/* ---- two-sample path, band-direct (what the per-chromosome driver uses; diff_mustache.py:262-276, :315-336, :371) -----------
 * For B block pairs cut out of the two samples' normalised bands (same n, dpx, starts): the difference image
 *     cd = filled_1 - filled_2 where both samples test the pixel (raw != 0, col - row >= 4), else 0
 * is formed tile by tile in LDS, blurred at sigma_2 and sigma_3 of every octave with the fused kernel's own separable passes
 * (SciPy tap order, no FMA) and only  dog[oct][b] = G_2 - G_3  (dev [n_octaves][B][CH][CH]) is written, together with
 * fit[oct][b] = {loc, scale} of norm.fit over the doubly tested pixels (dev [n_octaves][B][2]; scale from one pass,
 * sqrt(mean(x^2) - loc^2)) and mask_count[b] = their number.  No dense block, difference image or blurred level reaches HBM.
 * dog is written only in the tiles whose pixels can reach the tested band 4 <= col - row <= dpx + 1 (every found pixel lies
 * in one; the others hold no pixel of the fit either) -- the rest of the buffer is left as it was.
 * lv: the SAME level table as the sigma loop (levels 2 and 3 of each octave are used).  starts: host [B]. */
MST_STABLE uint64_t mst_diff_dog_workspace_bytes(int32_t B, int32_t CH, const mst_levels *lv);
MST_STABLE int mst_diff_dog_band(const double *band1, const double *band2, int64_t n, int32_t dpx, const int64_t *starts, int32_t B,
                      int32_t CH, const mst_levels *lv, double *dog, double *fit, uint32_t *mask_count, void *workspace,
                      uint64_t workspace_bytes, void *stream);
/* ---- two-sample path, tile-direct (the inter-chromosomal two-sample caller, mustache_amd/diff_trans.py) -----------------------
 * The same kernel with a dense source.  c1, c2: dev [P][C][C] f64, the two samples' tiles as mst_trans_scatter_tiles left them
 * (0 = no record).  For tile pair p the difference image
 *     cd = c1 - c2 where both are non-zero, else 0        (no triangle mask, no fills)
 * is staged with its reflect halo straight from the two tiles, blurred at sigma_2 and sigma_3 of every octave and only
 * dog[oct][p] = G_2 - G_3 (dev [n_octaves][P][C][C], EVERY pixel written: all tiles are launched), fit[oct][p] = {loc, scale} of
 * norm.fit over the pixels set in both samples (dev [n_octaves][P][2]; NaN when there is none) and mask_count[p] = their
 * number are written.  G_2 - G_3 is bit-identical to mst_diff_image + mst_gauss_blur on the same tiles.  1 <= P <= 65535;
 * blur radii of sigma_2 / sigma_3 in [1, 28]; C may be smaller than the blur halo.  lv: the sigma loop's level table. */
MST_STABLE uint64_t mst_diff_dog_tiles_workspace_bytes(int32_t P, int32_t C, const mst_levels *lv);
MST_STABLE int mst_diff_dog_tiles(const double *c1, const double *c2, int32_t P, int32_t C, const mst_levels *lv, double *dog,
                       double *fit, uint32_t *mask_count, void *workspace, uint64_t workspace_bytes, void *stream);
/* mst_pair_pvalues with x read from dog[octave][b][pixel] (the output of mst_diff_dog_band / mst_diff_dog_tiles). */
MST_STABLE int mst_pair_pvalues_dog(const mst_found *found, uint32_t found_cap, const uint32_t *found_count, const double *dog,
                         const double *fit, int32_t B, int32_t CH, int32_t n_octaves, int32_t tested_per_octave,
                         int32_t sample_offset, double *ppair, void *stream);
/* The differential test's inputs for the SELECTED records only (diff_mustache.py:450-453, :567-568): for record `slot` of
 * block fb (2P blocks: sample 1 = [0, P), sample 2 = [P, 2P); sel_* = the outputs of mst_bh_select_records):
 * out_pair = ppair of the record, out_value = its winning DoG value, out_other = the partner block's (fb +- P) winning value
 * at the same pixel, NaN if the partner did not find that pixel.  out_*: dev [2P][out_cap] f64; max_selected = the largest
 * sel_count (host value: the grid's width). */
MST_STABLE int mst_pair_gather(const mst_found *found, uint32_t found_cap, const uint32_t *found_count, const double *ppair, int32_t P,
                    const uint32_t *sel_index, const uint32_t *sel_pixel, const uint32_t *sel_count, uint32_t out_cap,
                    uint32_t max_selected, double *out_pair, double *out_value, double *out_other, void *stream);

/* ---- balancing, ICE and Newton (mustache_amd/balance.py; the algorithms are stated there) -------------------------------------------------
 * The matrix is the full symmetric CSR of one chromosome's kept pixels: row_ptr dev [n + 1] int64, col dev [nnz] int32,
 * val dev [nnz] float64, sorted by (row, column); an off-diagonal pixel appears in both rows.  Each row is cut into chunks of
 * 1024 entries counted from its first entry: chunk_ptr dev [n + 1] int64 (the chunks of row r are [chunk_ptr[r],
 * chunk_ptr[r + 1])), chunk_row dev [n_chunks] int32 (the row of each chunk).  Every sum runs in a fixed order that depends only
 * on absolute row and entry positions (no float atomics): results are bit-identical from run to run, under any permutation of
 * the pixels that built the CSR, and for any n (appended empty rows change nothing).  workspace: dev, at least
 * mst_balance_workspace_bytes(n, n_chunks) bytes, shared by the calls of one balancing (the iteration keeps nothing in it
 * between calls that the caller must preserve). */
typedef struct mst_balance_state {
    double variance;      /* population variance of r over the non-zero marginals, last iteration */
    double mean;          /* mean of the non-zero marginals, last iteration (1 when none is non-zero) */
    int32_t iterations;   /* iterations run */
    int32_t converged;    /* 1 once variance < tol */
    int32_t done;         /* 1 once converged or iterations == max_iter: later iterations are no-ops */
    int32_t _pad;
} mst_balance_state;

MST_STABLE uint64_t mst_balance_workspace_bytes(int64_t n, int64_t n_chunks);
/* m[i] = w[i] * sum_c A_ic w[c]; nnz[i] (optional, may be NULL) = #{c : A_ic != 0, w[c] != 0}.  w, m: dev [n] f64; nnz: dev [n]. */
MST_STABLE int mst_balance_marginals(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                          const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, const double *w, double *m, int32_t *nnz,
                          void *workspace, uint64_t workspace_bytes, void *stream);
/* `steps` ICE iterations on w (dev [n] f64, updated in place): s = w * (A w); mu = mean(s[s != 0]); r = s / mu there, 1
 * elsewhere; w /= r; variance = var(r[s != 0]) (0 when no s is non-zero); stop when variance < tol or after max_iter iterations.  state: dev, zeroed by
 * the caller before the first call; an iteration enqueued after state->done is set does nothing, so a caller may enqueue several
 * and read state back once. */
MST_STABLE int mst_balance_iterate(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                        const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, double *w, int32_t steps, int32_t max_iter,
                        double tol, mst_balance_state *state, void *workspace, uint64_t workspace_bytes, void *stream);
/* Newton balancing (Knight & Ruiz: inexact Newton on x_i (A x)_i = 1, conjugate gradients preconditioned by v = x * (A x);
 * mustache_amd/balance.py states the iteration).  The whole control flow lives in this record: one enqueued step is one mat-vec
 * plus its vector stages, a CG step or an outer update, whichever `phase` says. */
typedef struct mst_newton_state {
    double rho, rho_prev;     /* r.z of the current and of the previous CG step */
    double rout, rold;        /* r.r after the last and after the last-but-one outer update */
    double eta, innertol;     /* forcing term; the inner iteration runs while rho > innertol */
    double alpha, gamma;      /* CG step length; the fraction of it a capped step takes */
    double variance;          /* population variance of v over the active set, last outer update */
    int32_t phase;            /* next step: 0 start (v, r, the active set from x = 1), 1 CG step, 2 outer update */
    int32_t k;                /* CG steps taken since the last outer update */
    int32_t matvecs;          /* mat-vecs counted (the start step's is not) */
    int32_t iterations;       /* outer updates */
    int32_t capped_steps;     /* CG steps cut short at y = 0.1 or y = 3 */
    int32_t capped_upper;     /* ... of which at y = 3 */
    int32_t isolated;         /* unmasked bins whose partners are all masked: they keep x = 1 */
    int32_t active;           /* unmasked bins that take part */
    int32_t cg_step;          /* the step being run is a CG step (set by its scalar stage) */
    int32_t capped;           /* the CG step being run: 0 full, 1 capped below, 2 capped above */
    int32_t converged;        /* 1 once rout <= tol^2 */
    int32_t done;             /* 1 once converged, matvecs >= max_matvecs, or p.w was not positive and finite: later steps are no-ops */
} mst_newton_state;

MST_STABLE uint64_t mst_balance_newton_workspace_bytes(int64_t n, int64_t n_chunks);
/* `steps` steps on w (dev [n] f64; in: 1 on unmasked bins, 0 on masked; updated in place to x on the active set, 1 on isolated
 * bins, 0 on masked ones).  state: dev, zeroed by the caller before the first call; a step enqueued after state->done is set
 * does nothing.  trace: dev [trace_cap] f64, sqrt(rout) after every outer update (updates past trace_cap are not recorded).
 * workspace: dev, at least mst_balance_newton_workspace_bytes(n, n_chunks) bytes, kept by the caller from the first step to the
 * last; mst_balance_bias may then run in the same workspace. */
MST_STABLE int mst_balance_newton(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                       const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, double *w, int32_t steps, int32_t max_matvecs,
                       double tol, mst_newton_state *state, double *trace, int32_t trace_cap, void *workspace,
                       uint64_t workspace_bytes, void *stream);
/* kappa = sqrt(sum_{i <= j} A_ij w_i w_j / sum_{i <= j} A_ij) (the balanced total equals the raw total), bias[i] = kappa / w[i]
 * where w[i] != 0, NaN elsewhere.  bias: dev [n] f64; kappa: dev f64 [1] or NULL. */
MST_STABLE int mst_balance_bias(const int64_t *row_ptr, const int32_t *col, const double *val, const int32_t *chunk_row,
                     const int64_t *chunk_ptr, int64_t n, int64_t n_chunks, const double *w, double *bias, double *kappa,
                     void *workspace, uint64_t workspace_bytes, void *stream);
/* A bias vector applied to packed records as read_pd applies a -b vector (mustache.py read_bias): out[e] =
 * (v[e] / b[x[e]]) / b[x[e] + dist[e]], where b[i] = bias[i] when bias[i] >= 0.2, +inf when it is NaN or below 0.2, and 1 for
 * a bin at or past n_bias.  x, dist: dev [nnz] int32; v: dev [nnz] f32; bias: dev [n_bias] f64; out: dev [nnz] f64. */
MST_STABLE int mst_balance_apply_packed(const int32_t *x, const int32_t *dist, const float *v, int64_t nnz, const double *bias,
                             int64_t n_bias, double *out, void *stream);
/* A genome-wide bias (mustache_amd/balance_genome.py) applied to the records of P chromosome pairs in one pass.  The records
 * are concatenated as for the trans batches below: x, y dev int32 [n_records], v dev f64 [n_records]; seg_off dev int64 [P + 1],
 * non-decreasing, seg_off[0] = 0, seg_off[P] = n_records (a segment may be empty); pair p's records are [seg_off[p],
 * seg_off[p + 1]), x counted from genome bin row_off[p], y from col_off[p] (dev int64 [P] each).  out[e] =
 * (v[e] / b[row_off[p] + x[e]]) / b[col_off[p] + y[e]] in float64, where b[i] = bias[i] when bias[i] >= 0.2 and +inf when it is
 * NaN or below 0.2, when x or y is negative, or when the bin lies at or past n_bias: such a record comes out as 0 (NaN for a
 * NaN v) and the caller drops it with out > 0.  Nothing outside bias [n_bias] is read, whatever the offsets hold.  out: dev f64
 * [n_records], may alias v.  No atomics; records go two to a thread with 16-byte loads and stores when v and out are 16-byte
 * and x and y 8-byte aligned, one to a thread otherwise -- the same values either way.  n_records = 0 or P = 0: nothing is
 * launched, MST_OK. */
MST_STABLE int mst_balance_apply_pairs(const int32_t *x, const int32_t *y, const double *v, int64_t n_records, const int64_t *seg_off,
                            const int64_t *row_off, const int64_t *col_off, int32_t P, const double *bias, int64_t n_bias,
                            double *out, void *stream);

/* ---- inter-chromosomal pairs (mustache_amd/trans.py states the rules; tests/trans_reference.py restates them) --------------
 * A pair (A, B) is one rectangular map, x = bin of A, y = bin of B, cut into square CH x CH tiles with separate row and column
 * origins.  The tiles go through mst_scale_space (dense source: no band geometry, every tile with a tested pixel is computed)
 * and the dense tail (mst_candidate_features, mst_cluster_representatives -- its clustering clips at the tile edges). */
/* `.hic` rows of a trans matrix (mst_hic_rawstream_open_trans, include/mustache_io.h) -> COO: per record (a, b) = (binX, binY),
 * or (binY, binX) when transposed != 0 (the file stores the pair as (B, A)); value = (float)(count / (norm_x[a] * norm_y[b]))
 * with both vectors, or the raw count with neither; dropped when a bin lies outside its vector or the value is NaN, inf or
 * <= 0.  x, y: dev int32 [capacity]; v: dev f64 [capacity]; count: dev uint64, ACCUMULATED with one atomic per kept record
 * (the caller zeroes it; slabs may be decoded in any order and the record order is unspecified).  A count above capacity means
 * records were dropped: the caller re-runs with room for count records. */
MST_STABLE int mst_trans_decode_hic_rows(const void *payload, const void *rows, int32_t n_rows, const double *norm_x, int64_t n_norm_x,
                              const double *norm_y, int64_t n_norm_y, int32_t transposed, int32_t *x, int32_t *y, double *v,
                              int64_t capacity, uint64_t *count, void *stream);
/* The pair's z-score over its n records: mean = sum v / n, std = sqrt(sum (v - mean)^2 / n), out = (v - mean) / std with NaN /
 * inf -> 0 (out may alias v).  Both sums are exact (fixed-point integer pieces), so stats and out are bit-identical under any
 * permutation of the records.  stats: dev f64 [4] = {mean, std, n, 0}; mean / std are NaN when a value is not finite.
 * n < 2^31.  workspace: dev, mst_trans_zscore_workspace_bytes() bytes. */
MST_STABLE uint64_t mst_trans_zscore_workspace_bytes(void);
MST_STABLE int mst_trans_zscore(const double *v, int64_t n, double *out, double *stats, void *workspace, uint64_t workspace_bytes,
                     void *stream);
/* Records -> B tiles: c dev [B][CH][CH] f64, zeroed, then c[b][x - row0[b]][y - col0[b]] = v for every record inside tile b's
 * window (a record lands in every tile that holds it).  row0, col0: dev int64 [B], 1 <= B <= 4096.  Pixels are unique.
 * The package itself scatters every pair, a pair alone too, through mst_trans_scatter_worklist; this is the independent
 * single-pair form its bytes are pinned against and the tests' pair-alone path runs (tests/trans_pair_alone.py). */
MST_STABLE int mst_trans_scatter_tiles(const int32_t *x, const int32_t *y, const double *v, int64_t n, const int64_t *row0,
                            const int64_t *col0, int32_t B, int32_t CH, double *c, void *stream);
/* The trans prologue: nz[b] = c[b] != 0 over the whole tile, no fills; nz_count dev [B] uint32, overwritten. */
MST_STABLE int mst_trans_prologue(const double *c, uint8_t *nz, uint32_t *nz_count, int32_t B, int32_t CH, void *stream);

/* ---- trans pairs of a whole genome in shared launches (mustache_amd/trans_genome.py) ------------------------------------------
 * The records of P pairs are concatenated: x, y dev int32 [n], v dev f64 [n]; seg_off: dev int64 [P + 1], non-decreasing,
 * seg_off[0] = 0, seg_off[P] = n; pair p owns records [seg_off[p], seg_off[p + 1]). */
/* One pair of the batch.  Square tiles of C; K1 x K2 windows; window i of an axis of length n starts at i (C - 256) for
 * i < K - 1 and at max(0, n - C) for i = K - 1 (trans.trans_axis_tiles); K > 1 needs C > 256.  The pair's tile (i, j) has the
 * batch index tile_base + i K2 + j (pair-major, then row-major).  A pair that is not tiled (no record, std = 0 or not finite)
 * has K1 = K2 = 0. */
typedef struct mst_trans_pair {
    int32_t C, K1, K2, n1, n2, reserved;
    int64_t tile_base;
} mst_trans_pair;
/* mst_trans_zscore per pair, for all pairs in one sequence of launches: stats dev f64 [4 P] = {mean, std, n, flags} per pair
 * (flags = 1 when a value or a square was not finite: mean / std are NaN then; a pair without a record keeps 0, 0, 0, 0),
 * out dev f64 [n] (may alias v), extent dev int32 [2 P] = {max x, max y} per pair (-1, -1 without a record).  Every pair's
 * mean, std and out are bit-identical to mst_trans_zscore on that pair's records alone.  1 <= P <= 65535, n < 2^31.
 * workspace: dev, mst_trans_zscore_segmented_workspace_bytes(P) bytes (0 for a bad P). */
MST_STABLE uint64_t mst_trans_zscore_segmented_workspace_bytes(int32_t P);
MST_STABLE int mst_trans_zscore_segmented(const int32_t *x, const int32_t *y, const double *v, int64_t n, const int64_t *seg_off,
                               int32_t P, double *out, double *stats, int32_t *extent, void *workspace,
                               uint64_t workspace_bytes, void *stream);
/* counts dev uint32 [T], overwritten: for every tile of the batch the records with v != 0 inside its window (v: the
 * normalised values).  pairs: dev [P]; T = the batch's tile count < 2^31.  With unique pixels per pair this is the tile's
 * tested-pixel count, with duplicates an upper bound of it. */
MST_STABLE int mst_trans_count_tiles(const int32_t *x, const int32_t *y, const double *v, int64_t n, const int64_t *seg_off,
                          const mst_trans_pair *pairs, int32_t P, int64_t T, uint32_t *counts, void *stream);
/* Records of the pairs [p0, p1) -> the B tiles of one launch: c dev [B][CH][CH] f64, zeroed, then every record is written into
 * each tile t that holds it and has slot[t] in [0, B) (slot: dev int32 [T], -1 = not in this launch), at
 * c[slot[t]][x - row start][y - column start].  Only pairs with C == CH are scattered.  n_range = seg_off[p1] - seg_off[p0]
 * (sizes the launch).  The same bytes as mst_trans_scatter_tiles writes for the same tiles. */
MST_STABLE int mst_trans_scatter_worklist(const int32_t *x, const int32_t *y, const double *v, const int64_t *seg_off,
                               const mst_trans_pair *pairs, int32_t p0, int32_t p1, int64_t n_range, int64_t T,
                               const int32_t *slot, int32_t B, int32_t CH, double *c, void *stream);

/* ---- aggregate peak analysis (APA) of a loop list (mustache_amd/pileup.py states the rules; tests/pileup_reference.py restates
 * them).  band: dev f64, the diagonal-major RAW band of one chromosome (band[d * n + i] = pixel (i, i + d), not normalised)
 * with band_rows >= D + 1 rows; only rows 0 .. D are read.  Every sum has a fixed order that depends only on absolute column
 * positions and on the caller's loop order (no float atomics): results are bit-identical from run to run. */
/* workspace bytes of one pile-up (expected pass and reduce, used in turn); 0 for a bad argument or w > 64. */
MST_STABLE uint64_t mst_pileup_workspace_bytes(int64_t n, int32_t D, int64_t L, int32_t w);
/* valid[i] (dev uint8 [n], overwritten) = 1 when a non-zero pixel (i, j), |i - j| <= D, touches bin i; expected[d] (dev f64
 * [D + 1]) = sum of band[d][i] over i with i + d < n and both ends valid, divided by their count (0 when the count is 0). */
MST_STABLE int mst_pileup_expected(const double *band, int64_t n, int32_t band_rows, int32_t D, uint8_t *valid, double *expected,
                                   void *workspace, uint64_t workspace_bytes, void *stream);
/* One window per loop (x, y: dev int64 [L]): obs[l][a + w][b + w] (dev f64 [L][2w+1][2w+1]) = pixel (x + a, y + b), read at
 * (min, max) below the diagonal; NaN off the chromosome (an index < 0 or >= n) or farther than D from the diagonal.
 * oe = obs / expected[distance], NaN where expected is 0.  loop_stats dev f64 [L][3] = {obs centre, oe centre, P2LL}: the
 * centre over the mean of the loop's own non-NaN LL cells (rows 2w-q+1 .. 2w, columns 0 .. q-1), NaN when there is none or
 * the mean is 0.  0 <= w <= 64, 1 <= q <= 2w + 1; L = 0 launches nothing. */
MST_STABLE int mst_pileup_windows(const double *band, int64_t n, int32_t band_rows, int32_t D, const double *expected,
                                  const int64_t *x, const int64_t *y, int64_t L, int32_t w, int32_t q, double *obs, double *oe,
                                  double *loop_stats, void *stream);
/* agg dev f64 [4][(2w+1)^2] = per cell: sum of the non-NaN obs, their count, sum of the non-NaN oe, their count, over the
 * windows order[0 .. L) (dev int32, a permutation of 0 .. L-1; the caller sorts the loops by (x, y)); an entry outside 0 .. L-1
 * is skipped.  The order is cut into chunks of 512; each chunk's partial sums are added in chunk order.  L = 0 zeroes agg.
 * This call, mst_pileup_reduce_segmented and mst_pileup_reduce_pair are one pair of kernels (csrc/mst_pileup_reduce.hip; its
 * additions one by one: ordered_aggregate in tests/pileup_reference.py). */
MST_STABLE int mst_pileup_reduce(const double *obs, const double *oe, const int32_t *order, int64_t L, int32_t w, double *agg,
                                 void *workspace, uint64_t workspace_bytes, void *stream);

/* ---- the pile-up of an inter-chromosomal (trans) pair, from its records (rules: the trans part of mustache_amd/pileup.py;
 * tests/pileup_trans_reference.py restates them).  x, y: dev int32 [N] (bin of A, bin of B), v: dev f64 [N], v > 0 and finite,
 * N < 2^31; a record outside [0, n1) x [0, n2) is ignored.  Outside that domain: a record with !(v > 0) -- 0.0, negative, NaN
 * -- is ignored altogether (no valid flag, no share of the sum, no window), as mst_pileup_trans_batch ignores it; +inf counts
 * and makes expected NaN.  The call is mst_pileup_trans_batch with P = 1.  No float atomics: every output is bit-identical
 * from run to run and under any permutation of the records and of the loops. */
/* workspace bytes of one call (and of the mst_pileup_reduce that follows it), whatever N is: about 8 MiB for the chunk table
 * of 2^31 records, beside the loops' and the row bits' share; 0 for a bad argument or w > 64.  mst_pileup_trans_windows refuses
 * a workspace smaller than this. */
MST_STABLE uint64_t mst_pileup_trans_workspace_bytes(int64_t n1, int64_t n2, int64_t L, int32_t w);
/* valid_rows[i] (dev uint8 [n1], overwritten) = 1 when a record has x = i, valid_cols[j] (dev uint8 [n2]) alike for y;
 * expected[0] (dev f64 [1]) = the exact sum of v over all records (one rounding; NaN when a v is not finite) / (#valid rows *
 * #valid columns), 0 when that product is 0.  One window per loop (lx, ly: dev int64 [L]): obs[l][a + w][b + w] (dev f64
 * [L][2w+1][2w+1]) = pixel (lx + a, ly + b): the largest v among the records at that pixel, 0.0 where there is none, NaN off
 * the map (row index < 0 or >= n1, column index < 0 or >= n2).  oe = obs / expected[0], NaN where that is 0 or obs is NaN.
 * loop_stats as mst_pileup_windows writes it.  0 <= w <= 64, 1 <= q <= 2w + 1; L = 0 and N = 0 are served. */
MST_STABLE int mst_pileup_trans_windows(const int32_t *x, const int32_t *y, const double *v, int64_t N, int64_t n1, int64_t n2,
                                        const int64_t *lx, const int64_t *ly, int64_t L, int32_t w, int32_t q, uint8_t *valid_rows,
                                        uint8_t *valid_cols, double *expected, double *obs, double *oe, double *loop_stats,
                                        void *workspace, uint64_t workspace_bytes, void *stream);

/* ---- the same pile-up for P pairs in shared launches (rules: the genome mode of mustache_amd/pileup.py).  Added without a
 * change of MST_ABI_REVISION, as mst_balance_apply_pairs was.  The records of the pairs are concatenated as
 * mst_balance_apply_pairs leaves them (x, y dev int32 [N], v dev f64 [N]) and so are the loops (lx, ly dev int64 [L]).  The
 * segment tables are HOST arrays -- the caller knows every length without a wait -- and are checked before anything is
 * launched: seg_off int64 [P + 1] rises from 0 to N, loop_off int64 [P + 1] from 0 to L (a pair may have no record, or no
 * loop), n1, n2 int64 [P] are the pairs' dimensions (1 .. 2^31 - 1).  Pair p's valid flags start at byte sum(n1[0 .. p)) of
 * valid_rows (dev uint8 [sum n1], overwritten) and at byte sum(n2[0 .. p)) of valid_cols (dev uint8 [sum n2]).
 * A record with !(v > 0) -- 0.0, negative, NaN -- is ignored altogether (no flag, no share of the sum, no window), and so is a
 * record outside [0, n1[p]) x [0, n2[p]); +inf counts and makes that pair's expected NaN, and only that pair's.
 * expected dev f64 [P]; kept dev int64 [P]: the records of the pair that counted; obs, oe dev f64 [L][2w+1][2w+1]; loop_stats
 * dev f64 [L][3].  For every pair every output has the bits mst_pileup_trans_windows gives on that pair's records alone (the
 * same kernels with P = 1); no float atomics; bit-identical under any permutation of the records within a segment and of the
 * loops within a segment.  0 <= w <= 64, 1 <= q <= 2w + 1, 1 <= P <= 65535, N < 2^31; L = 0 and N = 0 are served. */
/* workspace bytes of one call; 0 for a bad argument (P outside 1 .. 65535, w > 64, tables that do not rise from 0). */
MST_STABLE uint64_t mst_pileup_trans_batch_workspace_bytes(const int64_t *seg_off, const int64_t *n1, const int64_t *loop_off,
                                                           int32_t P, int32_t w);
MST_STABLE int mst_pileup_trans_batch(const int32_t *x, const int32_t *y, const double *v, int64_t N, const int64_t *seg_off,
                                      const int64_t *n1, const int64_t *n2, const int64_t *lx, const int64_t *ly, int64_t L,
                                      const int64_t *loop_off, int32_t P, int32_t w, int32_t q, uint8_t *valid_rows,
                                      uint8_t *valid_cols, double *expected, int64_t *kept, double *obs, double *oe,
                                      double *loop_stats, void *workspace, uint64_t workspace_bytes, void *stream);
/* agg dev f64 [P][4][(2w+1)^2]: mst_pileup_reduce per pair, by the same kernels: a pair's sums do not depend on the pairs
 * beside it.  order dev int32 [L]: positions [loop_off[p], loop_off[p + 1]) hold pair p's loops (indices into obs / oe, so inside
 * that range themselves; any other index is skipped) in the order they are added: chunks of 512 that never cross a segment,
 * added in chunk order.  A pair without a loop gets zeros; L = 0 zeroes agg.  loop_off: host, as above.  Two launches whatever
 * P is. */
MST_STABLE uint64_t mst_pileup_reduce_segmented_workspace_bytes(const int64_t *loop_off, int32_t P, int32_t w);
MST_STABLE int mst_pileup_reduce_segmented(const double *obs, const double *oe, const int32_t *order, int64_t L,
                                           const int64_t *loop_off, int32_t P, int32_t w, double *agg, void *workspace,
                                           uint64_t workspace_bytes, void *stream);

/* ---- every loop of a pile-up against its local background (rules: "Enrichment" in mustache_amd/pileup.py;
 * tests/pileup_enrich_reference.py restates them).  Added without a change of MST_ABI_REVISION, as mst_thin_counts was.
 * obs: dev f64 [L][2w+1][2w+1], the windows mst_pileup_windows / mst_pileup_trans_windows / mst_pileup_trans_batch wrote.  Cell
 * (a, b), |a|, |b| <= w, is window[a + w][b + w]; the peak box is |a| <= p and |b| <= p; the neighbourhoods, in this order:
 *   DONUT  outside the peak box, a != 0 and b != 0          LL  1 <= a <= w and -w <= b <= -1, outside the peak box
 *   H      |a| <= 1 and p < |b| <= w                        V   |b| <= 1 and p < |a| <= w
 * A cell counts when its obs is not NaN and its expected value e is not 0.  cis: expected dev f64 [D + 1], xs, ys dev int64 [L]
 * and e = expected[|(ys + b) - (xs + a)|], 0 when that distance is above D; e_loop is NULL.  trans: e_loop dev f64 [L] and e =
 * e_loop[l]; expected, xs, ys are NULL and D is ignored.  Exactly one of expected and e_loop is given.
 * sums dev f64 [L][4][3] = the sum of obs, the sum of e and the number of the counted cells.  The order of every sum depends
 * only on the cell index: a loop's twelve numbers have the same bits in every run, at any position and for any L.  No
 * workspace, no atomics.  0 <= p < w <= 64, anything else is MST_E_ARG; L = 0 launches nothing. */
MST_STABLE int mst_pileup_enrich(const double *obs, int64_t L, int32_t w, int32_t p, const double *expected, int32_t D,
                                 const int64_t *xs, const int64_t *ys, const double *e_loop, double *sums, void *stream);

/* ---- one loop list piled up on two maps (rules: "Two maps" in mustache_amd/pileup.py; tests/pileup_compare_reference.py
 * restates them).  Added without a change of MST_ABI_REVISION, as mst_pileup_enrich was.  oe1, oe2: dev f64 [L][2w+1][2w+1],
 * the oe windows two pile-ups of the SAME L loops in the same order left on the device (mst_pileup_windows,
 * mst_pileup_trans_windows).  A cell of loop l is shared when neither oe1[l] nor oe2[l] is NaN there. */
/* sums dev f64 [L][4][3]: per loop and neighbourhood (DONUT, LL, H, V of mst_pileup_enrich, peak half-width p) over the shared
 * cells of the neighbourhood: the sum of oe1, the sum of oe2, their number.  The order of every sum depends only on the cell
 * index: a loop's twelve numbers have the same bits in every run, at any position and for any L.  No workspace, no atomics.
 * 0 <= p < w <= 64, anything else is MST_E_ARG; so is a null oe1, oe2 or sums with L > 0; L = 0 launches nothing. */
MST_STABLE int mst_pileup_compare(const double *oe1, const double *oe2, int64_t L, int32_t w, int32_t p, double *sums,
                                  void *stream);
/* agg dev f64 [3][(2w+1)^2] = per cell, over the windows order[0 .. L) (dev int32; the caller sorts the loops by (x, y)) that
 * share the cell: the sum of oe1, the sum of oe2, their number.  mst_pileup_reduce's kernels under the joint mask: the same
 * chunks of 512 and the same order of additions.  An order entry outside 0 .. L-1 is skipped.  workspace: dev, 24 * ceil(L / 512) * (2w+1)^2 bytes -- a workspace that
 * serves mst_pileup_reduce for (L, w) serves this call.  0 <= w <= 64, L < 2^31; L = 0 zeroes agg.  No float atomics:
 * bit-identical from run to run and under any permutation of the loops the caller sorts. */
MST_STABLE int mst_pileup_reduce_pair(const double *oe1, const double *oe2, const int32_t *order, int64_t L, int32_t w,
                                      double *agg, void *workspace, uint64_t workspace_bytes, void *stream);

/* ---- the significance of every loop of a pile-up from raw counts (rules: "Significance" in mustache_amd/pileup.py;
 * tests/pileup_poisson_reference.py restates them).  Added without a change of MST_ABI_REVISION, as mst_pileup_enrich was. */
/* One pass over a chromosome's raw records (x, dist: dev int32 [R]; count: dev float32 [R] when count_kind = 0, dev int64 [R]
 * when count_kind = 1): counts[k] (dev int64 [K], zeroed by the call) = the sum of the counts of the records whose pixel
 * (x << 32 | dist) is keys[k].  keys: dev int64 [K], strictly ascending (an unsorted list loses hits, never memory safety).  A
 * record whose dist lies outside [min_sep, max_sep] (0 <= min_sep <= max_sep; the range of the keys' distances) is left at
 * once.  A float32 count inside that range that is no integer value in [0, 2^63) sets *flag (dev int64, ACCUMULATED: the caller
 * zeroes it) to 1 and is not added: the caller refuses the map, nothing is rounded.  Integer atomic adds: the result has the same
 * bits under any order of the records, and a pixel that occurs in several records gets their sum.  K = 0 does nothing; R = 0
 * zeroes counts and launches nothing. */
MST_STABLE int mst_pileup_centre_counts(const int32_t *x, const int32_t *dist, const void *count, int32_t count_kind, int64_t R,
                                        const int64_t *keys, int64_t K, int32_t min_sep, int32_t max_sep, int64_t *counts,
                                        int64_t *flag, void *stream);
/* One lane per (loop, neighbourhood).  sums: dev f64 [L][4][3] as mst_pileup_enrich wrote them; centre_obs, centre_e: dev f64
 * [L], each loop's obs centre and its E_centre; counts: dev int64 [L], each loop's raw centre count; bias: dev f64 [n]; xs, ys:
 * dev int64 [L] (an index outside 0 .. n-1 reads no bias and counts as NaN).  Outputs, each dev f64 [L][4]:
 *   EXP    = centre_e * S_o / S_e in that order, NaN when cnt = 0, S_e = 0 or centre_obs is NaN;  FE = centre_obs / EXP, NaN when
 *            EXP is 0 or NaN -- the bits of pileup.enrichment() wherever the value is a number;
 *   LAMBDA = (EXP * bias[xs]) * bias[ys], NaN when EXP is NaN or either bias is NaN or < 0.2;
 *   P      = P(Poisson(LAMBDA) >= count): NaN when LAMBDA is NaN (or < 0); else 1 when count = 0; else 0 when LAMBDA = 0; else
 *            the regularised lower incomplete gamma function P(count, LAMBDA) in float64 (power series for LAMBDA <= 1 or
 *            LAMBDA <= count, 1 - Q by the continued fraction otherwise, both to a relative term of 2^-53).
 * A tail that has not converged within the kernel's iteration cap is NaN and adds 1 to *unconverged (dev int64, ACCUMULATED: the
 * caller zeroes it).  L = 0 launches nothing. */
MST_STABLE int mst_pileup_poisson(const double *sums, const double *centre_obs, const double *centre_e, const int64_t *counts,
                                  const double *bias, int64_t n, const int64_t *xs, const int64_t *ys, int64_t L, double *exp_out,
                                  double *fe_out, double *lambda_out, double *p_out, int64_t *unconverged, void *stream);

/* ---- read pairs -> pixels (rules: mustache_amd/pairs.py; tests/pairs_reference.py restates them).  Added without a change
 * of MST_ABI_REVISION, as mst_balance_apply_pairs was: a library from before the addition is refused by its missing symbols. */
/* One pass over the rows (pos1, pos2: dev int32 [n_rows]) of one chromosome.  A row is dropped when a position is < 1 or
 * > limit (zero_based != 0: < 0 or >= limit; limit = 2^31 when there is none) or when its larger bin is >= n; otherwise
 * bin = (pos - 1) / res (zero_based: pos / res) and its pixel is (x, y) = (min, max) of the two bins.  A pixel with
 * y - x < dense_diags adds to dense[(y - x) * n + x] (dev uint32 [dense_diags][n], diagonal-major, ACCUMULATED: the caller
 * zeroes it); any other pixel appends (far_key = x * n + y, far_mult) to the far list (dev int64 / uint32 [far_cap]), one entry
 * per run of adjacent rows of a wave that share the pixel, so a pixel may appear in several entries, in no fixed order.
 * counters (dev uint64 [2], ACCUMULATED, the caller zeroes them): [0] far entries, [1] dropped rows.  counters[0] > far_cap
 * means entries were lost (nothing is written past far_cap): far_cap = n_rows always suffices.  dense_diags = 0 is legal (dense
 * may be NULL); dense_diags <= n.  All sums are integer sums: the results do not depend on the order of the rows. */
MST_STABLE int mst_pairs_bin(const int32_t *pos1, const int32_t *pos2, int64_t n_rows, int32_t res, int32_t zero_based, int64_t limit,
                             int64_t n, int32_t dense_diags, uint32_t *dense, int64_t *far_key, uint32_t *far_mult, int64_t far_cap,
                             uint64_t *counters, void *stream);
/* The non-zero counters of dense [dense_diags][n] -> records (out_x, out_dist: dev int32 [cap]; out_count: dev uint32 [cap]) in
 * position order (by diagonal, then by x); *n_out (dev int64) = their number, which may exceed cap: nothing is written past
 * cap.  Two passes and a scan, no atomics.  workspace: dev, mst_pairs_compact_workspace_bytes(dense_diags, n) bytes. */
MST_STABLE uint64_t mst_pairs_compact_workspace_bytes(int32_t dense_diags, int64_t n);
MST_STABLE int mst_pairs_compact(const uint32_t *dense, int32_t dense_diags, int64_t n, int32_t *out_x, int32_t *out_dist,
                                 uint32_t *out_count, int64_t cap, int64_t *n_out, void *workspace, uint64_t workspace_bytes,
                                 void *stream);

/* ---- trans read pairs -> per-pair pixels, every chromosome pair of the genome in one pass (rules: mustache_amd/pairs.py;
 * tests/pairs_trans_reference.py restates them).  Added without a change of MST_ABI_REVISION, as mst_pairs_bin was. */
/* The rows (posA, posB: dev int32 [n_rows]) are pair-major: pair p owns rows [seg_off[p], seg_off[p + 1]) (seg_off: dev int64
 * [n_pairs + 1], seg_off[0] = 0, seg_off[n_pairs] = n_rows), posA on the pair's first chromosome and posB on its second.  Per
 * pair (dev int64 [n_pairs] each): limA / limB the chromosomes' lengths in bp (2^31 when there is none), nA / nB their bin
 * counts, cell_off the running sum of nA * nB over the pairs before it.  A row is dropped when its position on a side is < 1
 * or > that side's limit (zero_based != 0: < 0 or >= the limit), or when a bin is >= its n; otherwise x = (posA - 1) / res,
 * y = (posB - 1) / res (zero_based: pos / res) and its key is cell_off[p] + x * nB[p] + y -- no min / max: the pair is oriented.
 * A key < dense_cells adds to dense[key] (dev uint32 [dense_cells], ACCUMULATED: the caller zeroes it); any other key appends
 * (far_key, far_mult) to the far list (dev int64 / uint32 [far_cap]), one entry per run of adjacent rows of a wave that share
 * the key, in no fixed order.  *n_far (dev uint64, ACCUMULATED, zeroed by the caller): the far entries; *n_far > far_cap means
 * entries were lost (nothing is written past far_cap): far_cap = n_rows always suffices.  dropped (dev uint64 [n_pairs],
 * ACCUMULATED, zeroed by the caller): the dropped rows of each pair.  dense_cells = 0 is legal (dense may be NULL), and so is any
 * other value, one inside a pair included.  n_rows = 0 or n_pairs = 0 launches nothing.  All sums are integer sums: the results
 * do not depend on the order of the rows within their pairs. */
MST_STABLE int mst_pairs_bin_trans(const int32_t *posA, const int32_t *posB, int64_t n_rows, const int64_t *seg_off, int32_t n_pairs,
                                   const int64_t *limA, const int64_t *limB, const int64_t *nA, const int64_t *nB,
                                   const int64_t *cell_off, int32_t res, int32_t zero_based, int64_t dense_cells, uint32_t *dense,
                                   int64_t *far_key, uint32_t *far_mult, int64_t far_cap, uint64_t *n_far, uint64_t *dropped,
                                   void *stream);
/* The non-zero counters of dense [dense_cells] -> (out_key: dev int64 [cap] = the counter's index, out_count: dev uint32 [cap])
 * in ascending key order; *n_out (dev int64) = their number, which may exceed cap: nothing is written past cap.  Two passes and
 * a scan, no atomics.  workspace: dev, mst_pairs_trans_compact_workspace_bytes(dense_cells) bytes. */
MST_STABLE uint64_t mst_pairs_trans_compact_workspace_bytes(int64_t dense_cells);
MST_STABLE int mst_pairs_trans_compact(const uint32_t *dense, int64_t dense_cells, int64_t *out_key, uint32_t *out_count, int64_t cap,
                                       int64_t *n_out, void *workspace, uint64_t workspace_bytes, void *stream);
/* keys (dev int64 [n], each within the cells of a pair) and counts (dev int64 [n]) -> out_x, out_y (dev int32 [n]) and out_v
 * (dev float64 [n]): the pair p is the last one with cell_off[p] <= key, x = (key - cell_off[p]) / nB[p], y = the remainder,
 * v = the count, carried to float64 without passing through float32. */
MST_STABLE int mst_pairs_trans_decode(const int64_t *keys, const int64_t *counts, int64_t n, const int64_t *cell_off, const int64_t *nB,
                                      int32_t n_pairs, int32_t *out_x, int32_t *out_y, double *out_v, void *stream);

/* ---- binomial thinning of raw pixel counts (the rule: mustache_amd/downsample.py; tests/downsample_reference.py restates it).
 * Added without a change of MST_ABI_REVISION, as mst_pairs_bin was. */
/* A pixel whose count is at least this is thinned by its whole wave, 64 Philox calls at a time; below it, by its own lane
 * (csrc/mst_thin.hip; mirrored as downsample.HEAVY).  A value above 2^32 - 1 builds the plain one-lane-per-pixel kernel. */
#ifndef MST_THIN_HEAVY
#define MST_THIN_HEAVY 256
#endif
/* count_kind: the type of count_in */
#define MST_THIN_COUNT_I64 0
#define MST_THIN_COUNT_F32 1
#define MST_THIN_COUNT_F64 2
/* Records (x, dist: dev int32 [n_records]; count_in: dev int64 / float / double [n_records] by count_kind) of the pixels
 * (x, y = x + dist).  A count n that is an integer value in [0, 2^32 - 1] keeps count_out[e] = k = #{ j in [0, n) : u_j < T }
 * (dev int64 [n_records]), u_j = word j & 3 of Philox4x32-10(counter = (x, y, j >> 2, tag), key = (seed, sample)); 0 < T < 2^32.
 * Any other count (negative, above 2^32 - 1, not an integer, not finite) counts as 0 and sets words[2] = 1.  words (dev int64
 * [3], ACCUMULATED: the caller zeroes them): [0] the sum of the counts, [1] the sum of the k, [2] the bad-count flag.
 * count_out = NULL: nothing is drawn or written but words[0] and words[2] (T is then not looked at).  k depends on the pixel,
 * tag, seed, sample and T alone, and all sums are integer sums: the results do not depend on the order of the records. */
MST_STABLE int mst_thin_counts(const int32_t *x, const int32_t *dist, const void *count_in, int32_t count_kind, int64_t n_records,
                               uint32_t tag, uint32_t seed, uint32_t sample, uint64_t T, int64_t *count_out, int64_t *words,
                               void *stream);
/* The same thinning for the trans records of MANY chromosome pairs in one launch (`--downsample-genome`, `--match-depth-genome`;
 * tests/downsample_genome_reference.py restates it).  Added without a change of MST_ABI_REVISION, as mst_thin_counts was.
 * tag: zlib.crc32 of the pair's two stripped names, first + "\t" + second; swap != 0: the records' y is the bin on the first. */
typedef struct mst_thin_pair {
    uint32_t tag;
    uint32_t swap;
} mst_thin_pair;
/* Records (x, y: dev int32 [n_records]; count_in as above) of n_pairs pairs, pair p in [seg_off[p], seg_off[p + 1]) (seg_off: dev
 * int64 [n_pairs + 1], non-decreasing, seg_off[0] = 0, seg_off[n_pairs] = n_records; empty pairs are legal; whatever it holds,
 * nothing is read or written out of bounds).  table: dev [n_pairs].  A record of pair p keeps count_out[e] = k = #{ j in [0, n) :
 * u_j < T }, u_j = word j & 3 of Philox4x32-10(counter = (a, b, j >> 2, table[p].tag), key = (seed, key1)) with (a, b) = (y, x)
 * when table[p].swap and (x, y) otherwise -- with swap = 0 exactly mst_thin_counts' k for (x, dist = y - x, tag, sample = key1).
 * words (dev int64 [2 * n_pairs + 1], ACCUMULATED: the caller zeroes them): [2p] the sum of pair p's counts, [2p + 1] the sum of
 * its k, [2 * n_pairs] the bad-count flag (a bad count counts as 0).  count_out = NULL: nothing is drawn or written but the
 * sums of the counts and the flag (T is then not looked at).  max_blocks: the most workgroups (of 256 records a trip) to launch,
 * 0 for the default; the results do not depend on it, nor on the order of the records within a pair.  n_records = 0 launches
 * nothing. */
MST_STABLE int mst_thin_pairs(const int32_t *x, const int32_t *y, const void *count_in, int32_t count_kind, int64_t n_records,
                              const int64_t *seg_off, const mst_thin_pair *table, int32_t n_pairs, uint32_t seed, uint32_t key1,
                              uint64_t T, int64_t *count_out, int64_t *words, int32_t max_blocks, void *stream);

/* ---- raw records of one resolution -> the pixels of a coarser one (the rule: mustache_amd/multires.py;
 * tests/multires_reference.py restates it).  Added without a change of MST_ABI_REVISION, as mst_thin_counts was. */
/* Records (x, dist: dev int32 [n_records]; count_in: dev int64 / float / double [n_records] by count_kind, MST_THIN_COUNT_*) of
 * the pixels (x, y = x + dist) at some resolution r.  With factor k >= 1 a record goes to X = x / k, Y = y / k of the
 * resolution r * k, whose bin count is n (the caller's: a record with x < 0, dist < 0 or Y >= n is read and not written, so the
 * sums below then differ).  A pixel with Y - X < dense_diags adds its count to dense[(Y - X) * n + X] (dev uint64
 * [dense_diags][n], ACCUMULATED: the caller zeroes it; 64-bit integer atomics, so a cell that receives 3 * 2^31 holds 3 * 2^31);
 * any other pixel appends (far_key = X * n + Y, far_count) to the far list (dev int64 [far_cap] each), one entry per run of
 * adjacent records of a wave that share the key, in no fixed order.  A count that is no integer value in [0, 2^32 - 1]
 * (negative, above, fractional, not finite) counts as 0 and sets words[2] = 1.  words (dev int64 [3], ACCUMULATED: the caller
 * zeroes them): [0] the far entries -- more than far_cap means entries were lost (nothing is written past far_cap; far_cap =
 * n_records always suffices) --, [1] the sum of the counts read, [2] the bad-count flag.  Runs whose counts sum to 0 write
 * nothing.  dense_diags = 0 is legal (dense may be NULL); dense_diags <= n.  Adjacent lanes with equal keys combine their
 * counts before the atomic; every sum is an integer sum, so the results do not depend on the order of the records. */
MST_STABLE int mst_coarsen_records(const int32_t *x, const int32_t *dist, const void *count_in, int32_t count_kind, int64_t n_records,
                                   int32_t factor, int64_t n, int32_t dense_diags, uint64_t *dense, int64_t *far_key,
                                   int64_t *far_count, int64_t far_cap, int64_t *words, void *stream);
/* The non-zero counters of dense [dense_diags][n] (uint64) -> records (out_x, out_dist: dev int32 [cap]; out_count: dev int64
 * [cap]) in position order (by diagonal, then by x); *n_out (dev int64) = their number, which may exceed cap: nothing is
 * written past cap.  Two passes and a scan, no atomics.  workspace: dev, mst_coarsen_compact_workspace_bytes(dense_diags, n)
 * bytes. */
MST_STABLE uint64_t mst_coarsen_compact_workspace_bytes(int32_t dense_diags, int64_t n);
MST_STABLE int mst_coarsen_compact(const uint64_t *dense, int32_t dense_diags, int64_t n, int32_t *out_x, int32_t *out_dist,
                                   int64_t *out_count, int64_t cap, int64_t *n_out, void *workspace, uint64_t workspace_bytes,
                                   void *stream);

/* ---- the trans records of MANY chromosome pairs -> the pixels of a coarser resolution in one launch (`--coarser-genome`; the
 * rule: mustache_amd/multires.py; tests/coarsen_genome_reference.py restates it).  Added without a change of
 * MST_ABI_REVISION, as mst_thin_pairs was. */
/* Records (x, y: dev int32 [n_records]; count_in by count_kind, MST_THIN_COUNT_*) of n_pairs pairs, pair p in [seg_off[p],
 * seg_off[p + 1]) (seg_off: dev int64 [n_pairs + 1], non-decreasing, seg_off[0] = 0, seg_off[n_pairs] = n_records; empty pairs
 * are legal; whatever it holds, no table is read out of bounds).  n_a, n_b, cell_off (dev int64 [n_pairs]): the bin counts of
 * pair p's two chromosomes at the COARSE resolution and the first key of its cells, cell_off[p + 1] = cell_off[p] + n_a[p] *
 * n_b[p] (pairs.trans_tables).  With factor k >= 1 a record goes to X = x / k, Y = y / k.  A record with x < 0, y < 0,
 * X >= n_a[p] or Y >= n_b[p] is dropped and counted in words[3] before a key is formed, so that it aliases no other cell.
 * Any other record's key is cell_off[p] + X * n_b[p] + Y: a key below dense_cells adds its count to dense[key] (dev uint64
 * [dense_cells], ACCUMULATED: the caller zeroes it; 64-bit integer atomics), any other appends (far_key, far_count) to the far
 * list (dev int64 [far_cap] each), one entry per run of adjacent records of a wave that share the key, in no fixed order --
 * every far key is >= dense_cells.  dense_cells is at most the cells of all pairs; 0 is legal (dense may be NULL).  A count that
 * is no integer value in [0, 2^32 - 1] counts as 0 and sets words[2] = 1.  words (dev int64 [4], ACCUMULATED: the caller zeroes
 * them): [0] the far entries -- more than far_cap means entries were lost (nothing is written past far_cap; far_cap =
 * n_records always suffices) --, [1] the sum of the counts of the records that were not dropped, [2] the bad-count flag, [3]
 * the records dropped as outside.  Runs whose counts sum to 0 write nothing.  max_blocks: the most workgroups (of 256 records
 * a trip) to launch, 0 for the default; the results do not depend on it, nor on the order of the records within a pair.
 * n_records = 0 launches nothing. */
MST_STABLE int mst_coarsen_pairs(const int32_t *x, const int32_t *y, const void *count_in, int32_t count_kind, int64_t n_records,
                                 const int64_t *seg_off, const int64_t *n_a, const int64_t *n_b, const int64_t *cell_off,
                                 int32_t n_pairs, int32_t factor, int64_t dense_cells, uint64_t *dense, int64_t *far_key,
                                 int64_t *far_count, int64_t far_cap, int64_t *words, int32_t max_blocks, void *stream);
/* The non-zero counters of dense [dense_cells] (uint64) -> (out_key: dev int64 [cap] = the counter's index, out_count: dev
 * int64 [cap]) in ascending key order; *n_out (dev int64) = their number, which may exceed cap: nothing is written past cap.
 * Two passes and a scan, no atomics.  workspace: dev, mst_coarsen_pairs_compact_workspace_bytes(dense_cells) bytes. */
MST_STABLE uint64_t mst_coarsen_pairs_compact_workspace_bytes(int64_t dense_cells);
MST_STABLE int mst_coarsen_pairs_compact(const uint64_t *dense, int64_t dense_cells, int64_t *out_key, int64_t *out_count, int64_t cap,
                                         int64_t *n_out, void *workspace, uint64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSTACHE_HIP_H */
