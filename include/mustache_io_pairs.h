/*
 * mustache_io_pairs.h -- the read-pair reader of libmustache_io.so (mustache_amd/pairs.py states the rule): a 4DN `.pairs`
 * or `.pairs.gz` file -> per-chromosome arrays of the cis rows' two positions.  The host only parses; mst_pairs_bin
 * (include/mustache_hip.h) turns the positions into pixels on the device.
 *
 * Only symbols are added to the library: MST_IO_ABI_VERSION stays.  A binding looks the symbols up and refuses a library
 * that lacks them by naming them.
 */
#ifndef MUSTACHE_IO_PAIRS_H
#define MUSTACHE_IO_PAIRS_H

#include "mustache_io.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mst_pairs mst_pairs;

/* One pass over the whole file.  Lines starting with '#' are header lines: `#chromsize: NAME LENGTH` lines give the
 * chromosomes in that order, `#columns:` names the columns (chr1 pos1 chr2 pos2 are taken by name; without the line they are
 * columns 2 to 5); both are honoured in the leading header block, a '#' line further down is skipped, and so is a blank line.
 * Without a `#chromsize` line the chromosomes are the names in order of first appearance (chr1 before chr2 of a row) and have
 * length -1: no upper position limit.  Fields are separated by runs of tabs or blanks.
 *
 * Every data line is parsed.  A line with too few fields, or whose pos1 / pos2 is not a decimal integer ([+-]?[0-9]+), fails
 * the open with MST_IO_E_FORMAT and a message that names the line number (1-based; the first such line of the file whatever
 * n_threads is).  A row with chr1 != chr2 (exact byte compare) is a trans row; a cis row whose chromosome is not in the header
 * is an unknown row; both are counted and dropped.  Every other row is stored: (pos1, pos2) as int32 in file order within its
 * chromosome -- 8 bytes of host memory per cis pair.  A position that does not fit int32 is stored as INT32_MIN, which is out
 * of range under either convention.  A stored row is out of range when a position is < 1 or > length (zero_based: < 0 or
 * >= length); such rows are counted here and stay in the arrays: mst_pairs_bin drops and counts them again on the device.
 *
 * Plain files are mapped, cut at line ends into chunks and parsed by n_threads threads (<= 0: the hardware's count); `.gz`
 * files (bgzf included: concatenated members) are inflated by one producer thread through zlib, which cuts the chunks at line
 * ends for the same workers.  chunk_bytes (mst_pairs_open_chunked; <= 0: 4 MiB) is the chunk size aimed at -- the result does
 * not depend on it or on n_threads. */
int mst_pairs_open(const char *path, int32_t zero_based, int32_t n_threads, mst_pairs **out);
int mst_pairs_open_chunked(const char *path, int32_t zero_based, int32_t n_threads, int64_t chunk_bytes, mst_pairs **out);
void mst_pairs_close(mst_pairs *h);

/* The chromosome table.  *name is valid until close; *length_bp is -1 when the file has no `#chromsize` line. */
int32_t mst_pairs_n_chromosomes(const mst_pairs *h);
int mst_pairs_chromosome(const mst_pairs *h, int32_t index, const char **name, int64_t *length_bp);

/* The stored rows of chromosome `index`: the return value is their count (>= 0) or an MST_IO_E_* code; *pos1 / *pos2 are
 * borrowed, valid until close (NULL when the count is 0); *out_of_range: how many of them are out of range. */
int64_t mst_pairs_rows(const mst_pairs *h, int32_t index, const int32_t **pos1, const int32_t **pos2, int64_t *out_of_range);

/* counters[0 .. 4]: data rows read; rows kept (stored and in range); trans rows; out-of-range rows; rows of an unknown
 * chromosome.  rows read = the sum of the other four. */
int mst_pairs_counters(const mst_pairs *h, int64_t counters[5]);

/* ---- trans rows, on request (inter-chromosomal calls from a pairs file: --pairs-trans) -------------------------------------
 * mst_pairs_open_ex is mst_pairs_open_chunked with keep_trans.  keep_trans == 0: exactly mst_pairs_open_chunked -- no trans
 * row is stored.  keep_trans != 0: a trans row whose two chromosomes are both in the `#chromsize` table is stored as well,
 * 8 bytes of host memory per such row.  For the pair (a, b) of table indices a < b the position on a goes into the first array
 * and the position on b into the second, whichever way round the row named them; rows keep file order within their pair for
 * any n_threads and chunk_bytes; a position that does not fit int32 is stored as INT32_MIN.  Every counter, array and entry
 * point above keeps its meaning.  A file without `#chromsize` lines fails the open with MST_IO_E_FORMAT and a message that
 * names `#chromsize`: the pairs are those of the table, and the genome layout needs the lengths. */
int mst_pairs_open_ex(const char *path, int32_t zero_based, int32_t n_threads, int64_t chunk_bytes, int32_t keep_trans,
                      mst_pairs **out);

/* The stored trans rows of the whole file, in one pair of int32 arrays in pair-major order: (0,1), (0,2), ..., (1,2), ... --
 * every pair of the table, empty ones included.  *n_pairs = P = C (C - 1) / 2; *seg_off: int64 [P + 1], pair p's rows are
 * [seg_off[p], seg_off[p + 1]); *posA / *posB: int32 [seg_off[P]] (NULL when there is no row); *out_of_range: int64 [P], how
 * many of the pair's rows are out of range -- the position on a outside a's range or the position on b outside b's, by the
 * rule of the cis rows.  All borrowed, valid until close.  MST_IO_E_ARG on a handle opened without keep_trans. */
int mst_pairs_trans_rows(const mst_pairs *h, int64_t *n_pairs, const int64_t **seg_off, const int32_t **posA, const int32_t **posB,
                         const int64_t **out_of_range);

/* counters[0 .. 2]: trans rows stored; how many of those are out of range; trans rows naming a chromosome the table lacks (not
 * stored).  [0] + [2] = counters[2] of mst_pairs_counters.  MST_IO_E_ARG on a handle opened without keep_trans. */
int mst_pairs_trans_counters(const mst_pairs *h, int64_t counters[3]);

#ifdef __cplusplus
}
#endif
#endif
