/*
 * mustache_io_trans.h -- the inter-chromosomal read of libmustache_io.so (mustache_amd/trans.py): the raw-row stream of
 * include/mustache_io.h (mst_hic_rawstream_*) over every block of the matrix of a chromosome PAIR.  The host only inflates;
 * mst_trans_decode_hic_rows (include/mustache_hip.h) decodes the rows on the device, divides by both normalisation vectors and
 * transposes a pair the file stores the other way round.
 */
#ifndef MUSTACHE_IO_TRANS_H
#define MUSTACHE_IO_TRANS_H

#include "mustache_io.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same stream over EVERY block of the inter-chromosomal matrix of chrom_a and chrom_b (versions 7-9; no distance limit).
 * The file keys a pair by its lower chromosome index first; *transposed = 1 when that is chrom_b, i.e. the rows' binX belong to
 * chrom_b and their binY to chrom_a (mst_trans_decode_hic_rows, include/mustache_hip.h, swaps them).  next / release / close
 * as for mst_hic_rawstream_open.  mst_hic_rawstream_info_trans: the normalisation vectors of chrom_a and chrom_b (NULL and -1 for "NONE"; valid
 * until close) and the two lengths in base pairs. */
int mst_hic_rawstream_open_trans(mst_hic *h, const char *chrom_a, const char *chrom_b, int32_t resolution, const char *norm,
                                 int32_t n_threads, void *slab_memory, int32_t n_slabs, int64_t slab_bytes, int32_t *transposed,
                                 mst_hic_rawstream **out);
int mst_hic_rawstream_info_trans(mst_hic_rawstream *s, const double **norm_a, int64_t *count_a, const double **norm_b,
                                 int64_t *count_b, int64_t *length_a_bp, int64_t *length_b_bp);

#ifdef __cplusplus
}
#endif
#endif
