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

#ifdef __cplusplus
}
#endif
#endif
