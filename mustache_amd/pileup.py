"""Aggregate peak analysis (APA) of a loop list on the GPU: the map piled up around every loop of a Mustache TSV, with
Juicer APA's names and defaults (w = 10, q = 6, n = 30).  `python -m mustache_amd.pileup`, `pileup()` / `pileup_band()` in
Python.  tests/pileup_reference.py restates the arithmetic in NumPy.

Rules:
  * Loop list: any TSV Mustache writes (`.tsv`, `.loop1`, `.diffloop1`, ...); columns 1-6 are read, later ones are kept as
    they are.  An anchor's bin is ((start + end) // 2) // res, so a list from another resolution piles up on this map; the
    two anchors are taken as (x, y) = (min, max).  Chromosome names match with or without a `chr` prefix.
  * Status of every row: `trans` (two chromosomes), `no_chrom` (not selected, or not in the map), `short` (y - x < n_min),
    `long` (-x given and y - x > x_max), `off_map` (an anchor >= n), `used` otherwise.
  * Per chromosome: D = max(y - x) + 2w over its kept loops; the map is read with the distance limit D * res (not the
    caller's -d clamp ladder) into the RAW band (not normalised) with D + 1 used rows; n is the band width as the caller has it.
  * Valid bins: touched by a non-zero pixel (i, j), |i - j| <= D.  E[d] = sum band[d, i] / #{i : i and i + d valid,
    i + d < n} over i with both ends valid; 0 when the count is 0.
  * Windows: cell [a + w, b + w] = pixel (x + a, y + b), a, b in [-w, w], read at (min, max) below the diagonal; NaN off the
    chromosome (index < 0 or >= n), excluded from every sum and count.  obs = band value, oe = obs / E[distance] (NaN where
    E is 0).
  * Aggregate: the loops sorted by (x, y), per cell the sum and the non-NaN count of obs and oe (chunks of 512 loops added in
    chunk order); the genome-wide aggregate adds the chromosome partials in the order the chromosomes ran.  Bit-identical
    under any permutation of the input rows and from run to run.
  * Metrics on M = sum / count: corners q x q, rows = a index, columns = b index; LL = rows 2w-q+1 .. 2w, columns 0 .. q-1
    (nearest the diagonal), UL, UR, LR alike; c = M[w, w]; P2X = c / mean(X); ZscoreLL = (c - mean LL) / std LL (population);
    P2M = c / mean(M without the centre).  Per loop: P2LL = centre / mean of its own non-NaN LL cells (NaN when there is none
    or the mean is 0).
Not claimed: agreement with Juicer's own output.

Device work (mustache_amd/csrc/mst_pileup.hip): valid flags and E (two reads of the band), the windows with each loop's
centre and P2LL; the reduce of every mode is csrc/mst_pileup_reduce.hip (tests/pileup_reference.py, ordered_aggregate, restates
its additions one by one).  One host wait per chromosome, when the aggregates come back.

Inter-chromosomal lists (`--trans`, `pileup(..., trans=True)`, `pileup_trans_records()`; tests/pileup_trans_reference.py
restates the rules).  Without the switch nothing changes: rows with two chromosomes keep the status `trans`.
  * Rows: a row with one chromosome gets the status `cis`.  A row with two belongs to the unordered pair {chr1, chr2}; the
    pair's orientation (A, B) is that of its first row in the file, and a row written (B, A) has its anchors swapped.  Bins:
    a = ((start + end) // 2) // res on A, b likewise on B -- no min / max across chromosomes.  -ch keeps the pairs whose two
    chromosomes are both in the list; the other rows get `no_pair`.  Pairs run in order of first appearance.  -n / -x are
    refused: there is no distance.
  * Map: trans.read_trans_contacts(f, norm, A, B, res) -- what the trans caller has before its z-score (trans.py rule 1: v > 0
    and finite, divided by the file's vectors); n1 = max x + 1, n2 = max y + 1; no z-score.  A pair without a record, or not in
    the file, gives its rows `no_pair`; a row with a >= n1 or b >= n2 is `off_map`; every other row is `used`.  Text input,
    --balance, -b and `.hic` files of version 6 are refused as the trans caller refuses them.
  * A pixel that occurs more than once among the records takes the largest of its values (an order-free rule).
  * Row i of A is valid when some record has x = i, column j of B when some record has y = j.  E = (sum of v over ALL records,
    a repeated pixel's every record counted) / (#valid rows * #valid columns): one scalar per pair, 0 when the product is 0.
    The sum is exact (csrc/mst_exact_sum.h: one rounding, equal to math.fsum of the records in any order).
  * Windows: cell [da + w][db + w] = pixel (a + da, b + db); NaN when an index is < 0, or >= n1 on the A axis or >= n2 on the B
    axis; 0.0 where the map has no record.  oe = obs / E, NaN where E is 0 or obs is NaN.  Per loop: the obs centre, the oe
    centre and P2LL with the cis definition (the same row and column index ranges).  In a trans window no corner is nearer a
    diagonal than another: the four corners are equivalent by symmetry, and "LL" names an index range only.
  * Aggregate: the loops sorted by (a, b), the same reduce with the same chunks of 512; genome-wide = the pair partials added
    in run order; the same metrics().  Bit-identical under any permutation of the records and of the rows.
  * Records outside the rule: pileup_trans_records() ignores a record whose v is not > 0 (zero, negative, NaN) altogether -- no
    valid flag, no share of E, no window -- as it ignores one off the map; +inf counts and makes E NaN.  read_trans_contacts
    hands over v > 0 and finite only, so no run meets either.
Device work (mustache_amd/csrc/mst_pileup_trans_batch.hip): one pass over the pair's records finds the valid rows and columns,
the exact total and the window cells together; one host wait per pair.  A pair alone is a batch of one pair of the genome
mode's kernels below.

Genome mode (`--trans --balance-genome ICE|NEWTON [--balance-pixels all|inter] [--pairs-trans]`, `pileup(..., trans=True,
balance_genome=...)`, `pileup_trans_batch()`): the lists the callers write from a raw `.hic` file or a pairs file, piled up on
the map they were called from.  The rows, the windows, E, the aggregate and the files are the trans rules above; what differs:
  * Map of a pair (A, B): the genome-balanced records the trans caller has before its z-score -- GenomeBias.records(A, B)
    through mst_balance_apply_pairs, the records with v' > 0.  The genome is read and balanced ONCE for the run
    (balance_genome.read_genome, solve_genome: one `... balancing of the genome (... pixels)` line), on every chromosome of the
    file whichever pairs the list names; its memory refusal is balance_genome's.
  * Dimensions: n1 = n_A, n2 = n_B of the genome layout (length // res + 1, GenomeBias.bins), known on the host before anything
    runs -- NOT max x + 1 as above: under --balance-genome the chromosome's extent is known, so NaN means "off the
    chromosome".  E does not depend on the choice.
  * Statuses: `off_map` when a >= n_A or b >= n_B, decided on the host before the launch; `no_pair` when a chromosome of the
    pair is not in the file, when the pair has no raw record, or when none of its records counts after the balancing (its
    `kept` comes back 0: the pair's device result is discarded and its partial is the empty one).
  * Pairs run in order of first appearance; the genome-wide aggregate adds the pair partials in that order on the host.
  * Batches: consecutive pairs until their raw records reach balance_genome.APPLY_BATCH_RECORDS (balanced_segments), cut
    earlier where the windows of their loops (16 (2w+1)^2 bytes per loop) would exceed WINDOW_SHARE of the device's free
    memory; a single pair whose windows do not fit is refused with both numbers.  One host wait per batch: one concatenated
    copy carries every pair's aggregate, loop statistics, E and kept.
  * Refused: --balance-genome without --trans, with --balance, -b or -norm other than NONE, on `.cool` / `.mcool` / text input;
    --balance-pixels without --balance-genome; a pairs file without --pairs-trans; --pairs-trans without --balance-genome or
    on another input; --pairs-zero-based without --pairs-trans (no other pile-up bins a pairs file with it).  Each is one `Error:` line before anything is read.
Device work (mustache_amd/csrc/mst_pileup_trans_batch.hip): mst_pileup_trans_batch serves P pairs in five launches -- a record
whose v' is not > 0 is skipped in the pass, so the balanced records go in without a compaction -- and
mst_pileup_reduce_segmented (csrc/mst_pileup_reduce.hip) is the reduce for P pairs in two; every pair's values have the bits a
batch of that pair alone gives.

Enrichment (`--enrich [--peak P] [--min-enrichment T]`, `peak=P` on pileup() / pileup_band() / pileup_trans_records() /
pileup_trans_batch(); tests/pileup_enrich_reference.py restates the rules).  Every used loop against its own local background,
HiCCUPS's four neighbourhoods, in all three modes above.  Without the switch (`peak=None`) nothing is launched and nothing changes.
  * Parameters: w, the window half-width above, and the peak half-width p, 0 <= p < w (default 2).
  * Cell (a, b), |a|, |b| <= w, is the pixel (x + a, y + b) as above.  The peak box is |a| <= p and |b| <= p.  The
    neighbourhoods, in the fixed order DONUT, LL, H, V:
      DONUT  outside the peak box, a != 0 and b != 0;
      LL     1 <= a <= w and -w <= b <= -1, outside the peak box (the side nearer the diagonal, as the LL corner);
      H      |a| <= 1 and p < |b| <= w;
      V      |b| <= 1 and p < |a| <= w.
  * A cell counts when its obs is not NaN and its expected value e is not 0.  cis: e = E[|(y + b) - (x + a)|], and that distance
    must be <= D.  trans: e is the pair's scalar E.
  * Per loop and neighbourhood N, over the counted cells: S_o = sum obs, S_e = sum e, cnt = their number.
    EXP_N = E_centre * S_o / S_e (E_centre = E[y - x], or the pair's E), NaN when cnt = 0, S_e = 0 or the obs centre is NaN.
    FE_N = obs centre / EXP_N, NaN when EXP_N is 0 or NaN.  FE_MIN = the smallest of the four, NaN when any of them is NaN.
  * The aggregate, on the host, per neighbourhood: apa_oe[w, w] / mean of apa_oe over the neighbourhood's non-NaN cells (NaN when
    there is none or the mean is 0), for every chromosome or pair and for the genome-wide pile-up.
  * Files: PREFIX.enrich.tsv (each row as read, then STATUS OBS_CENTER E_CENTER EXP_* FE_* FE_MIN; NaN for a row that is not
    `used`), PREFIX.enrich.stats.tsv (one line per chromosome or pair and `all`: the aggregate's four ratios), and with
    --min-enrichment T PREFIX.enriched.tsv: the input's header and the unchanged lines of the `used` rows with FE_MIN >= T (NaN
    fails), a loop list the tools read.  The four files above stay byte for byte what they are without --enrich.
  * Refused, one `Error:` line before anything is read: --peak or --min-enrichment without --enrich; P >= w (or P < 0).
  * Not done: widening w where a neighbourhood is sparse.  A Poisson p-value needs the raw counts beside the balanced band:
    "Significance" below, in the one mode that has them.
Device work (mustache_amd/csrc/mst_pileup_enrich.hip): mst_pileup_enrich, one wave per loop over the window of obs that is already
resident, the twelve sums per loop by the walk of csrc/mst_pileup_sums.h (neighbourhood_sums; ordered_neighbourhood_sums in
tests/pileup_enrich_reference.py restates its additions one by one); they come back in the one concatenated copy each mode waits for.  The ratios are NumPy's.

Significance (`--enrich --poisson [--max-fdr T]` under `--balance ICE|NEWTON` on a `.hic` or pairs file, `poisson=True` on pileup(),
`poisson=PoissonInput(...)` on pileup_band(); tests/pileup_poisson_reference.py restates the rules cell by cell).  A fold
enrichment cannot tell a centre count of 3 from one of 300; under --balance the chromosome's raw integer pixel set and the bias
are on the device anyway, so every used loop gets a Poisson p-value against each of its four backgrounds and the list a BH FDR.
Without the switch nothing is launched, no result gains a key and no file changes.
  * For a used loop at bins (x, y), with the window half-width w and the peak half-width p of the enrichment:
      c        the raw count of pixel (x, y) in the chromosome's raw pixel set (balance.read_hic_raw / pairs.read_pairs_raw): an
               integer, 0 when the set has no such pixel; a pixel that occurs in several records counts their sum;
      b1, b2   bias[x], bias[y] of the vector balance.solve returned;
      EXP_N    for N in DONUT, LL, H, V exactly the enrichment's: the same sums, the same NaN rules, the same bits;
      LAMBDA_N = (EXP_N * b1) * b2 -- HiCCUPS's step, the expected value of the balanced map taken back to count space by the
               centre pixel's two bias values; NaN when EXP_N is NaN, or when either bias is NaN or < 0.2 (the bins
               balance_records_device treats as +inf);
      P_N      = P(Poisson(LAMBDA_N) >= c): NaN when LAMBDA_N is NaN (whatever c is; so is a negative LAMBDA_N, which no count
               data gives); else 1.0 when c = 0; else 0.0 when LAMBDA_N = 0; else the regularised lower incomplete gamma function
               P(c, LAMBDA_N) (1.0 at LAMBDA_N = +inf);
      P_MAX    the largest of the four, NaN when one of them is: a loop must beat all four backgrounds, as in HiCCUPS.
  * The tail, in float64: for x <= 1 or x <= a the power series sum_k x^k / ((a + 1) .. (a + k)) with the prefactor
    exp(a log x - x - lgamma(a)) / a, otherwise 1 - Q by the continued fraction (the classical cephes / Numerical Recipes
    split); both stop at a relative term of 2^-53.  At most 131 072 iterations (c = lambda = 2^24, the largest integer a `.hic`
    float32 count holds exactly, takes 30 767); a tail that has not converged by then is NaN and is counted
    ("poisson_unconverged"), never a wrong number.  The error grows like c * 2^-53 through the prefactor: 1e-9 relative to SciPy
    holds for c < 5 000 with a margin of 50.
  * Q_N: Benjamini-Hochberg over the used loops OF THE WHOLE RUN, all chromosomes together, once per neighbourhood, over the
    loops whose P_N is not NaN: ascending sort, p * m / rank, suffix minimum, clip at 1 -- mst_bh_fdr, the rule the callers' own
    q-values follow.  Q_MAX is the largest of the four, NaN when one is.  This is BH over the list, NOT HiCCUPS's lambda-chunked
    FDR over every pixel of the map.
  * Files: PREFIX.poisson.tsv (each row as read, then STATUS RAW_CENTER BIAS1 BIAS2 LAMBDA_* P_* P_MAX Q_* Q_MAX; NaN for a row
    that is not `used`) and, with --max-fdr T, PREFIX.significant.tsv: the input's header and the unchanged lines of the `used`
    rows with Q_MAX <= T (NaN fails), a loop list the tools read.  The six files above stay byte for byte what the same run
    writes without --poisson.  One line reports the used loops, those with a defined P_MAX and those that pass --max-fdr.
  * Refused, one `Error:` line before anything is read (poisson_request): --poisson without --enrich; without --balance
    ICE|NEWTON (stored vectors and -b leave no raw counts in hand); with --trans, --balance-genome or -f2; on text or `.cool`
    input (text counts may be fractional and may repeat a pixel); in a multi-rank run; --max-fdr without --poisson or outside
    (0, 1].  A `.hic` file whose counts are fractional ends the run with one `Error:` line that names the chromosome: a flag
    word written by the kernel, nothing is rounded.
  * Not claimed: agreement with Juicer's own output.
Device work (mustache_amd/csrc/mst_pileup_poisson.hip): mst_pileup_centre_counts, the one new pass over the map -- every raw record
against the sorted centre pixels of the list, a 64-bit integer atomic add per hit, so the counts have the same bits under any
record order; mst_pileup_poisson, one lane per (loop, neighbourhood): EXP and FE in enrichment()'s operation order (the host
ratios are not run in this mode), LAMBDA and the tail.  Everything rides in the one concatenated copy the chromosome already waits
for; the genome-wide BH adds one wait at the end of the run.

Two maps (`-f2 FILE [-b2 BIAS] [--peak P] [--min-lfc T]`, `pileup_pair()`, `pileup_band_pair()`, `pileup_trans_records_pair()`;
tests/pileup_compare_reference.py restates the rules).  One loop list piled up on two maps f (sample 1) and f2 (sample 2) at one
resolution with the same w, q and a peak half-width p (0 <= p < w, default 2), and what differs between them scored.  --balance,
-norm, -n, -x, -ch and --trans apply to both maps alike; -b is the bias file of -f, -b2 that of -f2.  Without -f2 nothing
changes and nothing is launched.
  * Rows: classify() runs once.  Per chromosome D = max(y - x) + 2w over the kept rows as above, one D for both maps, and both
    bands are read before either is piled up.  A row is `no_chrom` when either map lacks the chromosome, `off_map` when
    y >= min(n_1, n_2), `used` otherwise: one status column, and a `used` row is used on both maps.  Trans, pair by pair:
    `no_pair` when either file lacks the pair or has no record of it, `off_map` when a >= min(n1_1, n1_2) or b >= min(n2_1, n2_2).
  * Per sample: each sample's pile-up dict is what pileup_band() (trans: pileup_trans_records()) gives on that map with the
    jointly used loops, to the bit; the four files above are written per sample as PREFIX.1.* and PREFIX.2.*.
  * Shared cell: a cell of loop l is shared when neither oe1[l] nor oe2[l] is NaN there.
  * Per loop and neighbourhood N (DONUT, LL, H, V of enrichment_masks(w, p)), over the shared cells of N: S_1 = sum oe1, S_2 =
    sum oe2, cnt.  R_sN = c_s / (S_s / cnt), c_s the loop's oe centre on sample s; NaN when cnt = 0, when c_s is NaN or when
    S_s / cnt is 0.  LFC_N = log2(R_1N / R_2N), NaN unless both R are finite and > 0.  LFC: NaN when any LFC_N is NaN; the
    smallest when all four are > 0, the largest when all four are < 0, 0.0 otherwise -- as FE_MIN, a loop counts as stronger on
    one map only when every neighbourhood agrees.  Positive means stronger on -f.
  * Paired aggregate: the used loops sorted by (x, y) (trans: (a, b)); per cell, over the loops where the cell is shared, T_1 =
    sum oe1, T_2 = sum oe2, C = their number, chunks of 512 loops added in chunk order; genome-wide the
    chromosome (or pair) partials are added in run order on the host.  M_s = T_s / C (NaN where C = 0); the differential map is
    log2(M_1 / M_2), NaN unless both are > 0.  Per chromosome (or pair) and `all`: P2LL_s = metrics(M_s, w, q)["P2LL"], LFC_P2LL
    = log2(P2LL_1 / P2LL_2) and AGG_LFC_N = log2(aggregate_enrichment(M_1, w, p)[N] / aggregate_enrichment(M_2, w, p)[N]), each
    NaN unless both operands are finite and > 0.
  * Files beside the eight per-sample ones: PREFIX.compare.tsv (each row as read, then STATUS OE_CENTER_1 OE_CENTER_2 R1_* R2_*
    LFC_* LFC; NaN for a row that is not `used`), PREFIX.diff.tsv (the differential map, as write_matrix writes),
    PREFIX.compare.stats.tsv (CHR LOOPS_USED P2LL_1 P2LL_2 LFC_P2LL AGG_LFC_*: one line per chromosome or pair, and `all`); with
    --min-lfc T (finite, > 0) PREFIX.up1.tsv, the header and the unchanged lines of the used rows with LFC >= T, and
    PREFIX.up2.tsv, those with LFC <= -T: loop lists the tools read.  NaN fails both.
  * Refused, one `Error:` line before anything is read (compare_request): -b2 or --min-lfc without -f2; an -f2 or -b2 that does
    not exist; --min-lfc not finite or <= 0; P outside 0 .. w - 1; -f2 with --enrich or --min-enrichment (per-loop enrichment of
    each sample alone is what a single-map run is for); -f2 with --balance-genome, --balance-pixels or --pairs-trans (the
    genome-balanced two-map pile-up is not built).
  * Not claimed: a significance -- there are no counts; a minimum cnt; depth matching -- O/E and the ratio to the local
    background remove the scale, not the noise.
Device work (mustache_amd/csrc/mst_pileup_compare.hip) over the two stacks of oe windows the two pile-ups leave resident:
mst_pileup_compare, one wave per loop, the twelve sums per loop under the joint mask (the same walk, neighbourhood_sums);
mst_pileup_reduce_pair (csrc/mst_pileup_reduce.hip), the one reduce under the joint mask.  One host wait per chromosome or pair beyond the two per-sample pile-ups' own: one concatenated copy.
"""
import argparse
import math
import os
import sys

import numpy as np

MAX_W = 64
CORNERS = ("LL", "UL", "UR", "LR")
METRICS = ("P2LL", "P2UL", "P2UR", "P2LR", "ZscoreLL", "P2M")
STATS_HEADER = "CHR\tROWS_IN\tLOOPS_USED\t" + "\t".join(METRICS) + "\tOE_P2LL\n"
LOOP_COLUMNS = ("STATUS", "OBS_CENTER", "OE_CENTER", "P2LL")
DEFAULT_HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"
NEIGHBOURHOODS = ("DONUT", "LL", "H", "V")
DEFAULT_PEAK = 2
ENRICH_COLUMNS = ("STATUS", "OBS_CENTER", "E_CENTER") + tuple("EXP_" + n for n in NEIGHBOURHOODS) \
    + tuple("FE_" + n for n in NEIGHBOURHOODS) + ("FE_MIN",)
ENRICH_STATS_HEADER = "CHR\tLOOPS_USED\t" + "\t".join("OE_P2" + n for n in NEIGHBOURHOODS) + "\n"
POISSON_COLUMNS = ("STATUS", "RAW_CENTER", "BIAS1", "BIAS2") + tuple("LAMBDA_" + n for n in NEIGHBOURHOODS) \
    + tuple("P_" + n for n in NEIGHBOURHOODS) + ("P_MAX",) + tuple("Q_" + n for n in NEIGHBOURHOODS) + ("Q_MAX",)
COMPARE_COLUMNS = ("STATUS", "OE_CENTER_1", "OE_CENTER_2") + tuple("R1_" + n for n in NEIGHBOURHOODS) \
    + tuple("R2_" + n for n in NEIGHBOURHOODS) + tuple("LFC_" + n for n in NEIGHBOURHOODS) + ("LFC",)
COMPARE_STATS_HEADER = "CHR\tLOOPS_USED\tP2LL_1\tP2LL_2\tLFC_P2LL\t" + "\t".join("AGG_LFC_" + n for n in NEIGHBOURHOODS) + "\n"


class PileupError(ValueError):
    """A pile-up request that cannot be honoured."""


def check_window(w, q):
    if not 0 <= int(w) <= MAX_W:
        raise PileupError("window half-width w = %d is outside 0 .. %d (a window holds at most %d cells)"
                          % (w, MAX_W, (2 * MAX_W + 1) ** 2))
    if not 1 <= int(q) <= 2 * int(w) + 1:
        raise PileupError("corner size q = %d is outside 1 .. 2w + 1 = %d" % (q, 2 * int(w) + 1))


def check_peak(w, p):
    if not 0 <= int(p) < int(w):
        raise PileupError("peak half-width p = %d is outside 0 .. w - 1 = %d: the neighbourhoods lie between the peak box and "
                          "the window's edge" % (p, int(w) - 1))


# ----------------------------------------------------------------------------------------------------------------------
# metrics (host, on the (2w+1)^2 mean map)
# ----------------------------------------------------------------------------------------------------------------------
def corner_slices(w, q):
    near, far = slice(0, q), slice(2 * w - q + 1, 2 * w + 1)
    return {"LL": (far, near), "UL": (near, near), "UR": (near, far), "LR": (far, far)}


def mean_map(s, c):
    """sum / count per cell, NaN where the count is 0."""
    s, c = np.asarray(s, np.float64), np.asarray(c, np.float64)
    out = np.full(s.shape, np.nan)
    np.divide(s, c, out=out, where=c > 0)
    return out


def metrics(M, w, q):
    M = np.asarray(M, np.float64)
    c = M[w, w]
    sl = corner_slices(w, q)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name in CORNERS:
            out["P2" + name] = float(c / M[sl[name]].mean())
        ll = M[sl["LL"]]
        out["ZscoreLL"] = float((c - ll.mean()) / ll.std())
        rest = np.delete(M.reshape(-1), w * (2 * w + 1) + w)
        out["P2M"] = float(c / rest.mean()) if rest.size else math.nan
    return out


# ----------------------------------------------------------------------------------------------------------------------
# enrichment of every loop over its local background (host; the sums are the device's, mst_pileup_enrich)
# ----------------------------------------------------------------------------------------------------------------------
def enrichment_masks(w, p):
    """bool [4, 2w+1, 2w+1]: the cells of DONUT, LL, H, V (rows = a index, columns = b index)."""
    w, p = int(w), int(p)
    check_peak(w, p)
    off = np.arange(-w, w + 1)
    a, b = off[:, None], off[None, :]
    outside = (np.abs(a) > p) | (np.abs(b) > p)
    return np.stack([outside & (a != 0) & (b != 0), outside & (a >= 1) & (b <= -1),
                     (np.abs(a) <= 1) & (np.abs(b) > p), (np.abs(b) <= 1) & (np.abs(a) > p)])


def enrich_windows(obs, w, p, E=None, xs=None, ys=None, e_loop=None):
    """sums, a device float64 [L, 4, 3] tensor (S_o, S_e, cnt per neighbourhood), of the windows `obs` (device float64
    [L, 2w+1, 2w+1]).  cis: E (device float64 [D + 1]) with xs, ys (device int64 [L]); trans: e_loop (device float64 [L]).
    L = 0 launches nothing."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    L = int(obs.shape[0])
    cis = E is not None
    with torch.cuda.device(obs.device):
        sums = torch.empty((L, 4, 3), dtype=torch.float64, device=obs.device)
        _lib.check(lib.mst_pileup_enrich(_ptr(obs) if L else None, L, int(w), int(p), _ptr(E) if cis else None,
                                         int(E.numel()) - 1 if cis else 0, _ptr(xs) if cis and L else None,
                                         _ptr(ys) if cis and L else None, None if cis else (_ptr(e_loop) if L else None),
                                         _ptr(sums) if L else None, _stream()))
    return sums


def enrichment(sums, centre_obs, centre_e):
    """(EXP [L, 4], FE [L, 4], FE_MIN [L]) of the sums [L, 4, 3] mst_pileup_enrich wrote, each loop's obs centre and its E_centre."""
    sums = np.asarray(sums, np.float64).reshape(-1, 4, 3)
    so, se, cnt = np.ascontiguousarray(sums.transpose(2, 1, 0))          # each [4, L] with unit stride: a third of the time
    c = np.asarray(centre_obs, np.float64).reshape(1, -1)
    e = np.asarray(centre_e, np.float64).reshape(1, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = e * so / se
        exp[(cnt == 0) | (se == 0) | np.isnan(c)] = np.nan
        fe = c / exp                                     # a NaN EXP hands itself on
        fe[exp == 0] = np.nan
    fe_min = np.minimum(np.minimum(fe[0], fe[1]), np.minimum(fe[2], fe[3]))          # np.minimum hands a NaN on
    return exp.T, fe.T, fe_min


def aggregate_enrichment(apa_oe, w, p):
    """float64 [4]: apa_oe[w, w] / mean of apa_oe over each neighbourhood's non-NaN cells; NaN when there is none or the mean is 0."""
    M = np.asarray(apa_oe, np.float64)
    out = np.full(4, np.nan)
    for k, mask in enumerate(enrichment_masks(w, p)):
        cells = M[mask]
        cells = cells[~np.isnan(cells)]
        if cells.size and cells.mean() != 0:
            out[k] = M[int(w), int(w)] / cells.mean()
    return out


def _peak_kw(peak):
    """the keyword a driver hands on: a run without a peak makes the call it has always made"""
    return {} if peak is None else {"peak": peak}


def _enrich_result(sums, centre_obs, centre_e, apa_oe, w, p, ratios=None):
    """the keys a pile-up dict gains under `peak`; ratios = (EXP, FE) [L, 4] when the device has made them (poisson_windows)"""
    if ratios is None:
        exp, fe, fe_min = enrichment(sums, centre_obs, centre_e)
    else:
        exp, fe = ratios
        fe_min = _nan_extreme(np.minimum, fe)
    return {"center_e": np.asarray(centre_e, np.float64), "enrich_sums": np.asarray(sums, np.float64).reshape(-1, 4, 3),
            "enrich_exp": exp, "enrich_fe": fe, "fe_min": fe_min, "enrich_agg": aggregate_enrichment(apa_oe, w, p)}


# ----------------------------------------------------------------------------------------------------------------------
# significance of every loop from raw counts ("Significance" in the module docstring; csrc/mst_pileup_poisson.hip)
# ----------------------------------------------------------------------------------------------------------------------
class PoissonInput:
    """What `poisson=` takes: one chromosome's raw pixel set on the device as balance.read_hic_raw / pairs.read_pairs_raw leave
    it -- x, dist: int32 [R]; count: float32 (a `.hic` file's) or int64 (read pairs) [R] -- and the bias vector balance.solve
    returned for it (float64 [n], host array or device tensor; NaN on masked bins)."""

    def __init__(self, x, dist, count, bias):
        self.x, self.dist, self.count, self.bias = x, dist, count, bias


def _nan_extreme(op, a):
    """op (np.minimum / np.maximum, which hand a NaN on) over the four columns of a [L, 4] array -> [L]"""
    a = np.asarray(a, np.float64).reshape(-1, 4)
    return op(op(a[:, 0], a[:, 1]), op(a[:, 2], a[:, 3]))


def centre_counts(x, dist, count, keys, min_sep, max_sep, flag=None):
    """(counts, flag): counts, a device int64 [K] tensor, = per key the sum of the raw counts of the records (device x, dist
    int32 [R]; count float32 or int64 [R]) whose pixel x << 32 | dist is that key.  keys: device int64 [K], strictly ascending;
    [min_sep, max_sep]: the range of the keys' distances.  flag: a zeroed device int64 [1] tensor (made here when None) that
    holds 1 afterwards when a float32 count inside the range is no integer value.  K = 0 or R = 0 launches nothing."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    R, K = int(count.numel()), int(keys.numel())
    if count.dtype not in (torch.float32, torch.int64):
        raise PileupError("raw counts are float32 (a .hic file's) or int64 (read pairs), not %s" % count.dtype)
    if x.dtype != torch.int32 or dist.dtype != torch.int32 or keys.dtype != torch.int64 or not (x.numel() == dist.numel() == R):
        raise PileupError("raw records are x int32, dist int32 and count of one length, keys are int64 (got %s, %s, %d, %d, %d, %s)"
                          % (x.dtype, dist.dtype, x.numel(), dist.numel(), R, keys.dtype))
    with torch.cuda.device(keys.device):
        x, dist, count, keys = x.contiguous(), dist.contiguous(), count.contiguous(), keys.contiguous()
        counts = torch.empty(K, dtype=torch.int64, device=keys.device)
        if flag is None:
            flag = torch.zeros(1, dtype=torch.int64, device=keys.device)
        _lib.check(lib.mst_pileup_centre_counts(_ptr(x) if R else None, _ptr(dist) if R else None, _ptr(count) if R else None,
                                                0 if count.dtype == torch.float32 else 1, R, _ptr(keys) if K else None, K,
                                                int(min_sep), int(max_sep), _ptr(counts) if K else None, _ptr(flag), _stream()))
    return counts, flag


def poisson_windows(sums, centre_obs, centre_e, counts, bias, xs, ys, unconverged=None):
    """(out, unconverged): out, a device float64 [4, L, 4] tensor = EXP, FE, LAMBDA, P of every loop and neighbourhood, from the
    sums [L, 4, 3] enrich_windows() wrote, each loop's obs centre, E_centre (device float64 [L]) and raw centre count (device int64
    [L]), the bias (device float64 [n]) and xs, ys (device int64 [L]).  unconverged: a zeroed device int64 [1] tensor (made here
    when None) to which every tail that did not converge adds 1 (its P is NaN).  L = 0 launches nothing."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    L = int(xs.numel())
    with torch.cuda.device(sums.device):
        out = torch.empty((4, L, 4), dtype=torch.float64, device=sums.device)
        if unconverged is None:
            unconverged = torch.zeros(1, dtype=torch.int64, device=sums.device)
        if L:
            centre_obs, centre_e, counts, bias = centre_obs.contiguous(), centre_e.contiguous(), counts.contiguous(), bias.contiguous()
            _lib.check(lib.mst_pileup_poisson(_ptr(sums), _ptr(centre_obs), _ptr(centre_e), _ptr(counts), _ptr(bias),
                                              int(bias.numel()), _ptr(xs), _ptr(ys), L, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                              _ptr(out[3]), _ptr(unconverged), _stream()))
    return out, unconverged


def bh_rows(p):
    """Q [rows, 4]: Benjamini-Hochberg per column of P [rows, 4] (host) over its non-NaN entries, NaN where P is NaN -- the
    device's mst_bh_fdr with B = 4 and cap = rows, the rule the callers' own q-values follow.  One host wait; rows = 0 or no
    number at all launches nothing."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    p = np.asarray(p, np.float64).reshape(-1, 4)
    m = len(p)
    q = np.full((m, 4), np.nan)
    have = [np.flatnonzero(~np.isnan(p[:, k])) for k in range(4)]
    if m == 0 or not any(len(h) for h in have):
        return q
    lib = require_gpu()
    packed = np.zeros((4, m))
    for k, h in enumerate(have):
        packed[k, :len(h)] = p[h, k]
    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        pv = torch.from_numpy(packed).to(dev)
        count = torch.tensor([len(h) for h in have], dtype=torch.int32, device=dev)
        qd = torch.empty_like(pv)
        ws_bytes = int(lib.mst_bh_workspace_bytes(4, m))
        if ws_bytes == 0:
            raise PileupError("%d loops are too many for one BH launch (4 * loops must fit in int32)" % m)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.mst_bh_fdr(_ptr(pv), _ptr(count), 4, m, _ptr(qd), _ptr(ws), ws_bytes, _stream()))
        qh = qd.cpu().numpy()                                             # the one wait
    for k, h in enumerate(have):
        q[h, k] = qh[k, :len(h)]
    return q


def _poisson_result(out, counts, bias1, bias2):
    """the keys a pile-up dict gains under `poisson`"""
    out = np.asarray(out, np.float64).reshape(4, -1, 4)
    return {"raw_center": np.asarray(counts, np.int64).reshape(-1), "bias1": np.asarray(bias1, np.float64),
            "bias2": np.asarray(bias2, np.float64), "poisson_lambda": out[2], "poisson_p": out[3],
            "p_max": _nan_extreme(np.maximum, out[3])}


# ----------------------------------------------------------------------------------------------------------------------
# the device pile-up of one chromosome
# ----------------------------------------------------------------------------------------------------------------------
def _workspace(lib, n, D, L, w, device):
    import torch
    return torch.empty(max(int(lib.mst_pileup_workspace_bytes(int(n), int(D), int(L), int(w))), 256), dtype=torch.uint8,
                       device=device)


def expected(band, n, D, ws=None):
    """(valid uint8 [n], E float64 [D + 1]) device tensors of a raw band (device, [rows >= D + 1, n])."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    n, D = int(n), int(D)
    if band.dim() != 2 or band.shape[1] != n or band.shape[0] < D + 1 or band.dtype != torch.float64 or not band.is_contiguous():
        raise PileupError("band must be a contiguous float64 [rows >= D + 1, n] tensor (got %s, n %d, D %d)"
                          % (tuple(band.shape), n, D))
    with torch.cuda.device(band.device):
        if ws is None:
            ws = _workspace(lib, n, D, 0, 0, band.device)
        valid = torch.empty(n, dtype=torch.uint8, device=band.device)
        E = torch.empty(D + 1, dtype=torch.float64, device=band.device)
        _lib.check(lib.mst_pileup_expected(_ptr(band), n, int(band.shape[0]), D, _ptr(valid), _ptr(E), _ptr(ws), ws.numel(),
                                           _stream()))
    return valid, E


def windows(band, n, D, E, xd, yd, w, q):
    """(obs, oe [L, 2w+1, 2w+1], loop stats [L, 3] = obs centre, oe centre, P2LL) device tensors; xd, yd int64 device [L]."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    L, S = int(xd.numel()), 2 * int(w) + 1
    with torch.cuda.device(band.device):
        obs = torch.empty((L, S, S), dtype=torch.float64, device=band.device)
        oe = torch.empty_like(obs)
        st = torch.empty((L, 3), dtype=torch.float64, device=band.device)
        _lib.check(lib.mst_pileup_windows(_ptr(band), int(n), int(band.shape[0]), int(D), _ptr(E), _ptr(xd), _ptr(yd), L, int(w),
                                          int(q), _ptr(obs), _ptr(oe), _ptr(st), _stream()))
    return obs, oe, st


def _reduce(a, b, order, w, ws, joint=False, loop_off=None):
    """The one launcher of csrc/mst_pileup_reduce.hip: the sums over the two stacks of windows a, b in `order` (int32 device) into a
    new device tensor -- [4, (2w+1)^2] from mst_pileup_reduce, [3, (2w+1)^2] from mst_pileup_reduce_pair (joint), [P, 4, (2w+1)^2]
    from mst_pileup_reduce_segmented (loop_off: the host table of P + 1 offsets).  With no loop the C calls get null pointers and
    zero the sums."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    S, L = 2 * int(w) + 1, int(order.numel())
    stacks = [_ptr(t) if L else None for t in (a, b, order)]
    with torch.cuda.device(ws.device):
        if loop_off is not None:
            P = len(loop_off) - 1
            agg = torch.empty((max(P, 1), 4, S * S), dtype=torch.float64, device=ws.device)
            rc = lib.mst_pileup_reduce_segmented(*stacks, L, _host_ptr(loop_off), P, int(w), _ptr(agg), _ptr(ws), ws.numel(), _stream())
        else:
            agg = torch.empty((3 if joint else 4, S * S), dtype=torch.float64, device=ws.device)
            entry = lib.mst_pileup_reduce_pair if joint else lib.mst_pileup_reduce
            rc = entry(*stacks, L, int(w), _ptr(agg), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc)
    return agg


def reduce(obs, oe, order, w, ws):
    """agg [4, (2w+1)^2] device tensor: sum obs, count obs, sum oe, count oe over the windows in `order` (int32 device)."""
    return _reduce(obs, oe, order, w, ws)


def _loop_bins(xs, ys):
    import torch
    xs = np.asarray(xs.cpu() if isinstance(xs, torch.Tensor) else xs, np.int64).reshape(-1)
    ys = np.asarray(ys.cpu() if isinstance(ys, torch.Tensor) else ys, np.int64).reshape(-1)
    if len(xs) != len(ys):
        raise PileupError("xs and ys differ in length (%d, %d)" % (len(xs), len(ys)))
    return xs, ys


def _one_copy(parts):
    """The one concatenated copy, and the one host wait, of a chromosome, pair or batch.  parts: [(name, device tensor)] in the
    order they travel, float64 or int64 (carried as float64 bits).  Returns {name: flat host array}, an int64 part viewed back."""
    import torch
    host = torch.cat([(t.view(torch.float64) if t.dtype == torch.int64 else t).view(-1) for _, t in parts]).cpu().numpy()
    out, at = {}, 0
    for name, t in parts:
        piece = host[at:at + t.numel()]
        out[name] = piece.view(np.int64) if t.dtype == torch.int64 else piece
        at += t.numel()
    return out


def _result(agg, st, w, q, valid, expected, obs, oe):
    """The 15 keys every pile-up dict has, from the host aggregate [4, S, S], the host loop statistics [L, 3] and the device
    handles (or whatever stands for them)."""
    apa, apa_oe = mean_map(agg[0], agg[1]), mean_map(agg[2], agg[3])
    return {"valid": valid, "expected": expected, "obs": obs, "oe": oe, "sum_obs": agg[0], "count_obs": agg[1], "sum_oe": agg[2],
            "count_oe": agg[3], "apa": apa, "apa_oe": apa_oe, "center_obs": st[:, 0].copy(), "center_oe": st[:, 1].copy(),
            "p2ll": st[:, 2].copy(), "metrics": metrics(apa, w, q), "metrics_oe": metrics(apa_oe, w, q)}


def _empty_result(w, q, peak=None, poisson=False):
    S = 2 * w + 1
    if poisson:
        return dict(_empty_result(w, q, peak), poisson_unconverged=0,
                    **_poisson_result(np.zeros((4, 0, 4)), np.zeros(0, np.int64), np.zeros(0), np.zeros(0)))
    if peak is not None:
        return dict(_empty_result(w, q), **_enrich_result(np.zeros((0, 4, 3)), np.zeros(0), np.zeros(0), np.full((S, S), np.nan),
                                                          w, peak))
    return _result(np.zeros((4, S, S)), np.zeros((0, 3)), w, q, None, None, None, None)


def pileup_band(band, n, D, xs, ys, w=10, q=6, peak=None, poisson=None):
    """The pile-up of one chromosome's raw band (device float64 [rows >= D + 1, n]) around the loops (xs, ys) (bins, host
    arrays or tensors, y - x + 2w <= D).  Returns a dict: "valid", "expected", "obs", "oe" (device tensors), "sum_obs",
    "count_obs", "sum_oe", "count_oe", "apa" (mean obs), "apa_oe" (host [2w+1, 2w+1]), "center_obs", "center_oe", "p2ll"
    (host [L], input order), "metrics" and "metrics_oe" (dicts of METRICS).  L = 0 returns empty aggregates without a launch.
    peak=p adds the enrichment of every loop (the module docstring has the rules): "center_e" (E[y - x], host [L]),
    "enrich_sums" [L, 4, 3], "enrich_exp", "enrich_fe" [L, 4], "fe_min" [L] and "enrich_agg" [4], from one more launch inside the
    same host wait.
    poisson=PoissonInput(...) (with `peak`; "Significance" in the module docstring) adds "raw_center" (int64 [L]), "bias1", "bias2"
    [L], "poisson_lambda", "poisson_p" [L, 4] and "p_max" [L] from two more launches inside the same wait; EXP and FE are then the
    device's, with the bits enrichment() gives.  A float32 count that is no integer value is a PileupError."""
    import torch
    w, q = int(w), int(q)
    check_window(w, q)
    if peak is not None:
        check_peak(w, peak)
    elif poisson is not None:
        raise PileupError("poisson= without peak=: the significance is taken against the four neighbourhoods of the enrichment")
    xs, ys = _loop_bins(xs, ys)
    L, S = len(xs), 2 * w + 1
    if L == 0:
        return _empty_result(w, q, peak, poisson is not None)
    from ._lib import require_gpu
    lib = require_gpu()
    dev = band.device
    with torch.cuda.device(dev):
        ws = _workspace(lib, n, D, L, w, dev)
        valid, E = expected(band, n, D, ws)
        xd = torch.from_numpy(xs).to(dev, non_blocking=True)
        yd = torch.from_numpy(ys).to(dev, non_blocking=True)
        obs, oe, st = windows(band, n, D, E, xd, yd, w, q)
        order = torch.from_numpy(np.lexsort((ys, xs)).astype(np.int32)).to(dev, non_blocking=True)
        agg = reduce(obs, oe, order, w, ws)
        parts = [("agg", agg), ("st", st)]
        if peak is not None:
            sums, e_centre = enrich_windows(obs, w, peak, E=E, xs=xd, ys=yd), E[yd - xd]
            parts += [("sums", sums), ("e_centre", e_centre)]
        if poisson is not None:
            if bool(((xs < 0) | (ys < xs)).any()):
                raise PileupError("poisson=: a loop's bins must satisfy 0 <= x <= y")
            sep = ys - xs
            keys, inverse = np.unique((xs << 32) | sep, return_inverse=True)          # the centre pixels, each once
            words = torch.zeros(2, dtype=torch.int64, device=dev)                     # fractional-count flag, tails not converged
            per_key, _ = centre_counts(poisson.x, poisson.dist, poisson.count, torch.from_numpy(keys).to(dev, non_blocking=True),
                                       int(sep.min()), int(sep.max()), flag=words[:1])
            counts = per_key[torch.from_numpy(inverse.reshape(-1).astype(np.int64)).to(dev, non_blocking=True)]
            bias = torch.as_tensor(poisson.bias).to(dev, dtype=torch.float64)
            if int(bias.numel()) <= int(ys.max()):
                raise PileupError("poisson=: the bias vector has %d bins, the loops reach bin %d" % (bias.numel(), int(ys.max())))
            out4, _ = poisson_windows(sums, st[:, 0], e_centre, counts, bias, xd, yd, unconverged=words[1:])
            parts += [("out4", out4), ("counts", counts), ("bias1", bias[xd]), ("bias2", bias[yd]), ("words", words)]
        host = _one_copy(parts)
    out = _result(host["agg"].reshape(4, S, S), host["st"].reshape(L, 3), w, q, valid, E, obs, oe)
    if poisson is not None:
        bad, unconverged = (int(v) for v in host["words"])
        if bad:
            raise PileupError("a raw count is not an integer value: the significance needs raw integer counts")
        out4 = host["out4"].reshape(4, L, 4)
        out.update(_enrich_result(host["sums"], out["center_obs"], host["e_centre"], out["apa_oe"], w, peak,
                                  ratios=(out4[0], out4[1])))
        out.update(_poisson_result(out4, host["counts"], host["bias1"], host["bias2"]))
        out["poisson_unconverged"] = unconverged
    elif peak is not None:
        out.update(_enrich_result(host["sums"], out["center_obs"], host["e_centre"], out["apa_oe"], w, peak))
    return out


def pileup_trans_records(x, y, v, n1, n2, xs, ys, w=10, q=6, peak=None):
    """The pile-up of one inter-chromosomal pair's records (x = bins of A, y = bins of B, v > 0; host arrays or device tensors)
    on the n1 x n2 map around the loops (xs, ys) (bins of A, bins of B): pileup_trans_batch's dict of a batch of this one pair.
    That is pileup_band's dict with "expected" the scalar E (a float), "valid" the pair (rows uint8 [n1], columns uint8 [n2]) of
    device tensors and "kept", the records that counted (those with v > 0 on the map).  L = 0 still finds the valid flags and E;
    N = 0 gives E = 0.  One host wait.  peak=p adds pileup_band's enrichment keys, every cell's e and E_centre being the scalar E."""
    w, q, n1, n2 = int(w), int(q), int(n1), int(n2)
    check_window(w, q)
    if peak is not None:
        check_peak(w, peak)
    xs, ys = _loop_bins(xs, ys)
    if not (len(x) == len(y) == len(v)):
        raise PileupError("x, y and v differ in length (%d, %d, %d)" % (len(x), len(y), len(v)))
    if n1 < 1 or n2 < 1:
        raise PileupError("a trans map needs n1 >= 1 and n2 >= 1 (got %d x %d)" % (n1, n2))
    return pileup_trans_batch(x, y, v, [0, len(v)], [(n1, n2)], [(xs, ys)], w, q, peak)[0]


def _host_ptr(a):
    """a contiguous host array as the C ABI takes a host table"""
    import ctypes
    return ctypes.c_void_p(a.ctypes.data)


def pileup_trans_batch(x, y, v, seg_off, dims, loops, w=10, q=6, peak=None):
    """The pile-up of P inter-chromosomal pairs in shared launches (csrc/mst_pileup_trans_batch.hip).  x, y, v: the pairs' records
    concatenated (device int32 / int32 / float64, or host arrays; None when there is none), pair p owning [seg_off[p],
    seg_off[p + 1]) -- seg_off a HOST table of P + 1 entries; a record whose v is not > 0 is ignored, so the output of
    mst_balance_apply_pairs goes in unfiltered.  dims: [(n1, n2)] per pair; loops: [(xs, ys)] per pair (host arrays, bins of A
    and of B; either may be empty).  Returns one dict per pair: pileup_band's keys with "expected" the pair's scalar E (a float)
    and "valid" the pair (rows uint8 [n1], columns uint8 [n2]) -- "obs", "oe" and "valid" are views into the batch's device
    tensors -- and "kept", the records of the pair that counted.  A pair's values do not depend on the pairs beside it: they have
    the bits of a batch of that pair alone (pileup_trans_records).  One host wait for the whole batch.  peak=p adds the
    enrichment keys to every pair's dict: one launch over all the windows, each loop's e its own pair's E, gathered on the device."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    w, q, P = int(w), int(q), len(dims)
    check_window(w, q)
    if peak is not None:
        check_peak(w, peak)
    if len(loops) != P:
        raise PileupError("dims and loops differ in length (%d, %d)" % (P, len(loops)))
    seg = np.ascontiguousarray(seg_off, np.int64).reshape(-1)
    if len(seg) != P + 1:
        raise PileupError("seg_off has %d entries, %d pairs need %d" % (len(seg), P, P + 1))
    n1 = np.ascontiguousarray([d[0] for d in dims], np.int64)
    n2 = np.ascontiguousarray([d[1] for d in dims], np.int64)
    xs = [np.asarray(a, np.int64).reshape(-1) for a, _ in loops]
    ys = [np.asarray(b, np.int64).reshape(-1) for _, b in loops]
    for p in range(P):
        if len(xs[p]) != len(ys[p]):
            raise PileupError("xs and ys of pair %d differ in length (%d, %d)" % (p, len(xs[p]), len(ys[p])))
    loop_off = np.zeros(P + 1, np.int64)
    np.cumsum([len(a) for a in xs], out=loop_off[1:])
    N, L, S = int(seg[-1]) if P else 0, int(loop_off[-1]), 2 * w + 1
    if v is None:
        x = y = np.zeros(0, np.int32)
        v = np.zeros(0, np.float64)
    if not (len(x) == len(y) == len(v) == N):
        raise PileupError("x, y and v hold %d, %d and %d records, seg_off ends at %d" % (len(x), len(y), len(v), N))
    lib = require_gpu()
    dev = v.device if isinstance(v, torch.Tensor) and v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        x = torch.as_tensor(x).to(dev, dtype=torch.int32).contiguous()
        y = torch.as_tensor(y).to(dev, dtype=torch.int32).contiguous()
        v = torch.as_tensor(v).to(dev, dtype=torch.float64).contiguous()
        lxy = np.concatenate(xs + ys) if L else np.zeros(0, np.int64)
        order = np.concatenate([np.lexsort((ys[p], xs[p])) + loop_off[p] for p in range(P)]).astype(np.int32) if L \
            else np.zeros(0, np.int32)
        lxy_d = torch.from_numpy(lxy).to(dev, non_blocking=True)
        order_d = torch.from_numpy(order).to(dev, non_blocking=True)
        need = max(int(lib.mst_pileup_trans_batch_workspace_bytes(_host_ptr(seg), _host_ptr(n1), _host_ptr(loop_off), P, w)),
                   int(lib.mst_pileup_reduce_segmented_workspace_bytes(_host_ptr(loop_off), P, w)), 256)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rows = torch.empty(max(int(n1.sum()), 1), dtype=torch.uint8, device=dev)
        cols = torch.empty(max(int(n2.sum()), 1), dtype=torch.uint8, device=dev)
        E = torch.empty(max(P, 1), dtype=torch.float64, device=dev)
        kept = torch.empty(max(P, 1), dtype=torch.int64, device=dev)
        obs = torch.empty((L, S, S), dtype=torch.float64, device=dev)
        oe = torch.empty_like(obs)
        st = torch.empty((L, 3), dtype=torch.float64, device=dev)
        _lib.check(lib.mst_pileup_trans_batch(
            _ptr(x) if N else None, _ptr(y) if N else None, _ptr(v) if N else None, N, _host_ptr(seg), _host_ptr(n1), _host_ptr(n2),
            _ptr(lxy_d) if L else None, _lib.off(lxy_d, L) if L else None, L, _host_ptr(loop_off), P, w, q, _ptr(rows), _ptr(cols),
            _ptr(E), _ptr(kept), _ptr(obs) if L else None, _ptr(oe) if L else None, _ptr(st) if L else None, _ptr(ws), ws.numel(),
            _stream()))
        agg = _reduce(obs, oe, order_d, w, ws, loop_off=loop_off)
        parts = [("agg", agg), ("st", st), ("E", E), ("kept", kept)]
        if peak is not None:                           # e_loop: the E of the pair each loop belongs to
            pair_of = torch.from_numpy(np.repeat(np.arange(P, dtype=np.int64), np.diff(loop_off))).to(dev, non_blocking=True)
            parts.insert(2, ("sums", enrich_windows(obs, w, peak, e_loop=E[pair_of])))
        host = _one_copy(parts)
    agg_h, st_h = host["agg"].reshape(P, 4, S, S), host["st"].reshape(L, 3)
    row_off = np.concatenate([[0], np.cumsum(n1)])
    col_off = np.concatenate([[0], np.cumsum(n2)])
    out = []
    for p in range(P):
        l0, l1 = int(loop_off[p]), int(loop_off[p + 1])
        valid = (rows[int(row_off[p]):int(row_off[p + 1])], cols[int(col_off[p]):int(col_off[p + 1])])
        out.append(_result(agg_h[p], st_h[l0:l1], w, q, valid, float(host["E"][p]), obs[l0:l1], oe[l0:l1]))
        out[-1]["kept"] = int(host["kept"][p])
        if peak is not None:
            out[-1].update(_enrich_result(host["sums"].reshape(L, 4, 3)[l0:l1], out[-1]["center_obs"],
                                          np.full(l1 - l0, host["E"][p]), out[-1]["apa_oe"], w, peak))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# one loop list on two maps ("Two maps" in the module docstring; the sums are the device's, csrc/mst_pileup_compare.hip)
# ----------------------------------------------------------------------------------------------------------------------
def compare_windows(oe1, oe2, w, p):
    """sums, a device float64 [L, 4, 3] tensor (S_1, S_2, cnt per neighbourhood over the shared cells), of the two stacks of oe
    windows (device float64 [L, 2w+1, 2w+1] each, the same loops in the same order).  L = 0 launches nothing."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    L = int(oe1.shape[0])
    if oe2 is not None and tuple(oe2.shape) != tuple(oe1.shape):
        raise PileupError("the two window stacks differ in shape (%s, %s)" % (tuple(oe1.shape), tuple(oe2.shape)))
    with torch.cuda.device(oe1.device):
        sums = torch.empty((L, 4, 3), dtype=torch.float64, device=oe1.device)
        _lib.check(lib.mst_pileup_compare(_ptr(oe1) if L else None, _ptr(oe2) if L and oe2 is not None else None, L, int(w),
                                          int(p), _ptr(sums) if L else None, _stream()))
    return sums


def reduce_pair(oe1, oe2, order, w, ws):
    """agg [3, (2w+1)^2] device tensor: T_1 = sum oe1, T_2 = sum oe2, C = the number, per cell over the windows in `order` (int32
    device) that share the cell.  `ws`: a workspace that serves reduce() for these loops."""
    return _reduce(oe1, oe2, order, w, ws, joint=True)


def _log2_ratio(a, b):
    """log2(a / b), NaN unless both are finite and > 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        ok = (a > 0) & (b > 0) & (a < np.inf) & (b < np.inf)          # a NaN fails every comparison
        return np.where(ok, np.log2(a / b), np.nan)


def compare_ratios(sums, c1, c2):
    """(R1 [L, 4], R2 [L, 4], LFC_N [L, 4]) of the sums [L, 4, 3] mst_pileup_compare wrote and each loop's oe centre on the two
    samples."""
    sums = np.asarray(sums, np.float64).reshape(-1, 4, 3)
    s1, s2, cnt = np.ascontiguousarray(sums.transpose(2, 1, 0))         # each [4, L] with unit stride, as in enrichment()
    out = []
    for s, c in ((s1, c1), (s2, c2)):
        c = np.asarray(c, np.float64).reshape(1, -1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            bg = s / cnt
            r = c / bg                                   # a NaN centre hands itself on
        r[(cnt == 0) | (bg == 0)] = np.nan
        out.append(r)
    return out[0].T, out[1].T, _log2_ratio(out[0], out[1]).T


def lfc_summary(lfc_n):
    """[L]: NaN when any of the four LFC_N is NaN; the smallest when all four are > 0, the largest when all are < 0, else 0.0."""
    a = np.ascontiguousarray(np.asarray(lfc_n, np.float64).reshape(-1, 4).T)          # [4, L] with unit stride
    with np.errstate(invalid="ignore"):
        lo, hi = np.minimum(np.minimum(a[0], a[1]), np.minimum(a[2], a[3])), np.maximum(np.maximum(a[0], a[1]), np.maximum(a[2], a[3]))
        out = np.where(lo > 0, lo, np.where(hi < 0, hi, 0.0))            # all four > 0: the smallest; all four < 0: the largest
    out[np.isnan(lo)] = np.nan                                           # np.minimum hands a NaN on
    return out


def diff_map(T1, T2, C):
    """log2(M_1 / M_2) with M_s = T_s / C (NaN where C = 0): NaN unless both means are > 0."""
    return _log2_ratio(mean_map(T1, C), mean_map(T2, C))


def compare_aggregate(T1, T2, C, w, q, p):
    """The paired aggregate's dict: "t1", "t2", "count" (the sums as given), "m1", "m2" (T_s / C), "diff" (diff_map), "p2ll_1",
    "p2ll_2", "lfc_p2ll" (floats) and "agg_lfc" [4] (DONUT, LL, H, V)."""
    S = 2 * int(w) + 1
    T1, T2, C = (np.asarray(t, np.float64).reshape(S, S) for t in (T1, T2, C))
    m1, m2 = mean_map(T1, C), mean_map(T2, C)
    p1, p2 = metrics(m1, w, q)["P2LL"], metrics(m2, w, q)["P2LL"]
    return {"t1": T1, "t2": T2, "count": C, "m1": m1, "m2": m2, "diff": _log2_ratio(m1, m2), "p2ll_1": p1, "p2ll_2": p2,
            "lfc_p2ll": float(_log2_ratio(p1, p2)),
            "agg_lfc": _log2_ratio(aggregate_enrichment(m1, w, p), aggregate_enrichment(m2, w, p))}


def _compare_result(sums, c1, c2, agg, w, q, p):
    """the compare dict of one chromosome or pair: the per-loop arrays and the paired aggregate"""
    S = 2 * w + 1
    sums = np.asarray(sums, np.float64).reshape(-1, 4, 3)
    r1, r2, lfc_n = compare_ratios(sums, c1, c2)
    agg = np.asarray(agg, np.float64).reshape(3, S, S)
    return dict(compare_aggregate(agg[0], agg[1], agg[2], w, q, p), sums=sums, r1=r1, r2=r2, lfc_n=lfc_n, lfc=lfc_summary(lfc_n))


def _empty_compare(w, q, p):
    """the compare dict of no loop at all: empty arrays, zero sums, NaN ratios"""
    S = 2 * w + 1
    return _compare_result(np.zeros((0, 4, 3)), np.zeros(0), np.zeros(0), np.zeros((3, S, S)), w, q, p)


def _compare_resident(r1, r2, xs, ys, w, q, p):
    """the compare dict of two pile-up dicts of the same loops (xs, ys) whose "oe" windows are still on the device: two launches
    and a finish, one host wait"""
    import torch
    L = len(xs)
    if L == 0:
        return _empty_compare(w, q, p)
    from ._lib import require_gpu
    lib = require_gpu()
    oe1, oe2 = r1["oe"], r2["oe"]
    with torch.cuda.device(oe1.device):
        ws = _workspace(lib, 1, 0, L, w, oe1.device)
        order = torch.from_numpy(np.lexsort((ys, xs)).astype(np.int32)).to(oe1.device, non_blocking=True)
        host = _one_copy([("agg", reduce_pair(oe1, oe2, order, w, ws)), ("sums", compare_windows(oe1, oe2, w, p))])
    return _compare_result(host["sums"], r1["center_oe"], r2["center_oe"], host["agg"], w, q, p)


def pileup_band_pair(band1, n1, band2, n2, D, xs, ys, w=10, q=6, peak=DEFAULT_PEAK):
    """One chromosome on two maps: (dict 1, dict 2, compare dict).  band1, band2: the two raw bands (device float64 [rows >= D + 1,
    n_s]); the loops (xs, ys) must lie on both maps (y < min(n1, n2), y - x + 2w <= D).  Dict s is pileup_band(band_s, n_s, D, xs,
    ys, w, q) to the bit, its "obs" dropped (None) as soon as its "oe" is in hand; the compare dict holds "sums" [L, 4, 3], "r1",
    "r2", "lfc_n" [L, 4], "lfc" [L] (input order) and compare_aggregate()'s keys.  One host wait beyond the two pile-ups' own.
    L = 0 returns empty arrays without a launch."""
    w, q, peak = int(w), int(q), int(peak)
    check_window(w, q)
    check_peak(w, peak)
    xs, ys = _loop_bins(xs, ys)
    r1 = pileup_band(band1, n1, D, xs, ys, w, q)
    del band1                                            # a caller that holds no reference of its own has it freed here
    r1["obs"] = None
    r2 = pileup_band(band2, n2, D, xs, ys, w, q)
    del band2
    r2["obs"] = None
    return r1, r2, _compare_resident(r1, r2, xs, ys, w, q, peak)


def pileup_trans_records_pair(rec1, dims1, rec2, dims2, xs, ys, w=10, q=6, peak=DEFAULT_PEAK):
    """One inter-chromosomal pair on two maps: (dict 1, dict 2, compare dict).  rec_s = (x, y, v), the pair's records on sample s
    (host arrays or device tensors), dims_s = (n1, n2) of that map; the loops (xs, ys) = (bins of A, bins of B) must lie on both
    maps.  Dict s is pileup_trans_records(*rec_s, *dims_s, xs, ys, w, q) to the bit with "obs" dropped; the compare dict is
    pileup_band_pair's.  A sample without a record has E = 0, so every ratio is NaN.  One host wait beyond the two pile-ups'."""
    w, q, peak = int(w), int(q), int(peak)
    check_window(w, q)
    check_peak(w, peak)
    xs, ys = _loop_bins(xs, ys)
    r1 = pileup_trans_records(rec1[0], rec1[1], rec1[2], dims1[0], dims1[1], xs, ys, w, q)
    r1["obs"] = None
    r2 = pileup_trans_records(rec2[0], rec2[1], rec2[2], dims2[0], dims2[1], xs, ys, w, q)
    r2["obs"] = None
    return r1, r2, _compare_resident(r1, r2, xs, ys, w, q, peak)


def joint_status(ys, n1, n2):
    """The status of every eligible cis row of one chromosome on two maps of n1 and n2 bins (None: the map lacks the chromosome):
    `no_chrom` when either is missing, `off_map` when y >= min(n1, n2), `used` otherwise."""
    if n1 is None or n2 is None:
        return ["no_chrom"] * len(ys)
    n = min(int(n1), int(n2))
    return ["off_map" if int(y) >= n else "used" for y in ys]


def joint_status_trans(a, b, dims1, dims2):
    """joint_status for the rows of one pair: dims_s = (n1, n2) of sample s, None when the file lacks the pair or has no record
    of it (`no_pair`); `off_map` when a >= min(n1_1, n1_2) or b >= min(n2_1, n2_2)."""
    if dims1 is None or dims2 is None:
        return ["no_pair"] * len(a)
    na, nb = min(int(dims1[0]), int(dims2[0])), min(int(dims1[1]), int(dims2[1]))
    return ["off_map" if int(i) >= na or int(j) >= nb else "used" for i, j in zip(a, b)]


# ----------------------------------------------------------------------------------------------------------------------
# loop lists
# ----------------------------------------------------------------------------------------------------------------------
def _key(c):
    return str(c).replace("chr", "")


class LoopTable:
    """The rows of a Mustache loop TSV: `header` (without newline), `lines` (each row as read), the six anchor columns."""

    def __init__(self, header, lines, chr1, s1, e1, chr2, s2, e2):
        self.header, self.lines = header, lines
        self.chr1, self.chr2 = chr1, chr2
        self.s1, self.e1 = np.asarray(s1, np.int64), np.asarray(e1, np.int64)
        self.s2, self.e2 = np.asarray(s2, np.int64), np.asarray(e2, np.int64)

    def __len__(self):
        return len(self.lines)

    def bins(self, res):
        """(x, y) = (min, max) of the two anchors' bins, ((start + end) // 2) // res."""
        a = ((self.s1 + self.e1) // 2) // int(res)
        b = ((self.s2 + self.e2) // 2) // int(res)
        return np.minimum(a, b), np.maximum(a, b)


def read_loops(path):
    header, lines, cols = DEFAULT_HEADER, [], [[] for _ in range(6)]
    with open(path) as fh:
        for k, raw in enumerate(fh):
            line = raw.rstrip("\r\n")
            if not line.strip():
                continue
            f = line.split("\t")
            if k == 0 and f[0] == "BIN1_CHR":
                header = line
                continue
            if len(f) < 6:
                raise PileupError("%s: row %d has %d columns, a loop row has at least 6" % (path, k + 1, len(f)))
            lines.append(line)
            for c in range(6):
                cols[c].append(f[c])
    try:
        return LoopTable(header, lines, cols[0], [int(float(v)) for v in cols[1]], [int(float(v)) for v in cols[2]], cols[3],
                         [int(float(v)) for v in cols[4]], [int(float(v)) for v in cols[5]])
    except ValueError as e:
        raise PileupError("%s: an anchor position is not a number (%s)" % (path, e))


def _classify_trans(table, res, chromosomes):
    """classify() in trans mode: (status list, a, b, [(A, B)]) with a = bins on A, b = bins on B in the pair's orientation."""
    a = ((table.s1 + table.e1) // 2) // int(res)
    b = ((table.s2 + table.e2) // 2) // int(res)
    keys = None if not chromosomes else {_key(c) for c in chromosomes}
    pairs, first, status = [], {}, []
    for k in range(len(table)):
        k1, k2 = _key(table.chr1[k]), _key(table.chr2[k])
        if k1 == k2:
            status.append("cis")
        elif keys is not None and not (k1 in keys and k2 in keys):
            status.append("no_pair")
        else:
            if frozenset((k1, k2)) not in first:         # the pair's orientation: that of its first row
                first[frozenset((k1, k2))] = k1
                pairs.append((table.chr1[k], table.chr2[k]))
            if first[frozenset((k1, k2))] != k1:
                a[k], b[k] = b[k], a[k]
            status.append(None)
    return status, a, b, pairs


def classify(table, res, chromosomes=None, n_min=None, x_max=None, trans=False):
    """Statuses before the map is read: (status list, x, y, selected chromosome names).  Rows still eligible have status
    None; `x_max` is in bins; `n_min` = None is the default of 30 bins.  trans=True: (status list, a, b, [(A, B)]), the bins in
    each pair's orientation and the pairs in order of first appearance; `n_min` and `x_max` are refused."""
    if trans:
        if n_min is not None or x_max is not None:
            raise PileupError("-n / -x do not apply to inter-chromosomal loops: there is no distance")
        return _classify_trans(table, res, chromosomes)
    n_min = 30 if n_min is None else int(n_min)
    x, y = table.bins(res)
    cis = [_key(a) == _key(b) for a, b in zip(table.chr1, table.chr2)]
    selected, seen = [], set()
    for c, ok in (((c, True) for c in chromosomes) if chromosomes else zip(table.chr1, cis)):
        if ok and _key(c) not in seen:                   # each chromosome once, in order of first appearance
            seen.add(_key(c))
            selected.append(c)
    keys = {_key(c) for c in selected}
    status = []
    for k in range(len(table)):
        sep = int(y[k] - x[k])
        if not cis[k]:
            status.append("trans")
        elif _key(table.chr1[k]) not in keys:
            status.append("no_chrom")
        elif sep < n_min:
            status.append("short")
        elif x_max is not None and sep > x_max:
            status.append("long")
        else:
            status.append(None)
    return status, x, y, selected


# ----------------------------------------------------------------------------------------------------------------------
# the whole run
# ----------------------------------------------------------------------------------------------------------------------
def _read_band(f, chromosome, res, D, norm=False, bias=False, balance=None, device=None, verbose=False):
    """The chromosome's RAW band with distance limit D (device [D + 2, n]) and n, or (None, 0) when the map has no record of
    it (or no such chromosome)."""
    import torch
    from .hicfile import PackedContacts
    from .mustache import read_contacts
    from .normalize import band_from_host_coo, band_from_packed
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    try:
        r = read_contacts(f, norm, False, res, D * res, bias, chromosome, chromosome, verbose=verbose, packed=True, device=dev,
                          balance=balance)
    except NameError:                                  # a `.hic` file without this chromosome
        return None, 0
    if r is None:
        return None, 0
    if isinstance(r, PackedContacts):
        band = band_from_packed(r, D, dev)
        return band, int(band.shape[1])
    x, y, v, _res = r
    x = np.ascontiguousarray(x, dtype=np.int64)
    y = np.ascontiguousarray(y, dtype=np.int64)
    n = int(max(x.max(), y.max())) + 1
    return band_from_host_coo(x, y, np.ascontiguousarray(v, dtype=np.float64), n, D, dev), n


def _read_band_raw(f, chromosome, res, D, balance, device=None, verbose=False):
    """_read_band under `poisson`: (band, n, PoissonInput), or (None, 0, None).  The chromosome's raw pixel set is read as
    read_contacts reads it under `balance` (balance.read_hic_raw / pairs.read_pairs_raw), balanced by the same call
    (balance.balance_records_with_bias) and scattered by the same band_from_host_coo, so the band has the values _read_band
    gives; the raw records and the bias stay on the device."""
    import torch
    from .balance import balance_records_with_bias, check_request, method_of
    from .mustache import read_raw_sample
    from .normalize import band_from_host_coo
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    check_request(balance, f, False, False)
    if verbose:
        print("Reading contact map...")
    try:
        raw = read_raw_sample(f, False, res, D * res, chromosome, device=dev, balance=balance, verbose=verbose)
    except NameError:                                  # a file without this chromosome
        return None, 0, None
    if raw is None:
        return None, 0, None
    xd, dd, counts, dev, _depth = raw
    vd = counts if counts.dtype == torch.float32 else counts.to(torch.float64)
    r, bias = balance_records_with_bias(xd, dd, vd, D * res, chromosome, res, dev, method=method_of(balance))
    if r is None:
        return None, 0, None
    x = np.ascontiguousarray(r[0], dtype=np.int64)
    y = np.ascontiguousarray(r[1], dtype=np.int64)
    n = int(max(x.max(), y.max())) + 1
    return band_from_host_coo(x, y, np.ascontiguousarray(r[2], dtype=np.float64), n, D, dev), n, PoissonInput(xd, dd, counts, bias)


class PileupResult:
    """What pileup() returns: the table, per row `status`, `obs_center`, `oe_center`, `p2ll`; `chromosomes` = [(name, rows in,
    loops used, pile-up dict)] in run order; `all` = the genome-wide pile-up dict (sums, counts, means, metrics).  Under `peak`
    also per row `e_center`, `enrich_exp`, `enrich_fe` ([rows, 4]: DONUT, LL, H, V) and `fe_min`, NaN for a row that was not
    used, and "enrich_agg" in every pile-up dict; without it they are None.  Under `poisson` also per row `raw_center`, `bias1`,
    `bias2`, `p_max`, `poisson_lambda`, `poisson_p` ([rows, 4]) and, once total() has run the genome-wide BH over the used rows,
    `poisson_q` ([rows, 4]) and `q_max`; NaN for a row that was not used, None without `poisson`."""

    def __init__(self, table, status, w, q, peak=None, poisson=False):
        self.table, self.status, self.w, self.q, self.peak, self.poisson = table, status, w, q, peak, bool(poisson)
        L = len(table)
        self.obs_center, self.oe_center, self.p2ll = np.full(L, np.nan), np.full(L, np.nan), np.full(L, np.nan)
        self.e_center = self.enrich_exp = self.enrich_fe = self.fe_min = None
        if peak is not None:
            self.e_center, self.fe_min = np.full(L, np.nan), np.full(L, np.nan)
            self.enrich_exp, self.enrich_fe = np.full((L, 4), np.nan), np.full((L, 4), np.nan)
        self.raw_center = self.bias1 = self.bias2 = self.p_max = self.poisson_lambda = self.poisson_p = None
        self.poisson_q = self.q_max = None
        self.poisson_unconverged = 0
        if self.poisson:
            self.raw_center, self.bias1, self.bias2, self.p_max = (np.full(L, np.nan) for _ in range(4))
            self.poisson_lambda, self.poisson_p = np.full((L, 4), np.nan), np.full((L, 4), np.nan)
            self._scored = []                            # the used rows, in the order they were taken
        self.chromosomes = []
        self.all = None

    def take(self, rows, part):
        """the per-loop values of pile-up dict `part` to the table rows `rows` (one per loop of `part`, in its order)"""
        rows = np.asarray(rows, np.int64)
        self.obs_center[rows], self.oe_center[rows], self.p2ll[rows] = part["center_obs"], part["center_oe"], part["p2ll"]
        if self.peak is not None:
            self.e_center[rows], self.fe_min[rows] = part["center_e"], part["fe_min"]
            self.enrich_exp[rows], self.enrich_fe[rows] = part["enrich_exp"], part["enrich_fe"]
        if self.poisson:
            self.raw_center[rows], self.bias1[rows], self.bias2[rows] = part["raw_center"], part["bias1"], part["bias2"]
            self.poisson_lambda[rows], self.poisson_p[rows], self.p_max[rows] = part["poisson_lambda"], part["poisson_p"], part["p_max"]
            self.poisson_unconverged += part["poisson_unconverged"]
            self._scored.append(rows)

    def total(self, tot):
        """`all` from the four genome-wide sums and counts"""
        apa, apa_oe = mean_map(tot[0], tot[1]), mean_map(tot[2], tot[3])
        self.all = {"sum_obs": tot[0], "count_obs": tot[1], "sum_oe": tot[2], "count_oe": tot[3], "apa": apa, "apa_oe": apa_oe,
                    "metrics": metrics(apa, self.w, self.q), "metrics_oe": metrics(apa_oe, self.w, self.q)}
        if self.peak is not None:
            self.all["enrich_agg"] = aggregate_enrichment(apa_oe, self.w, self.peak)
        if self.poisson:                                 # BH over the used loops of the whole run, all chromosomes together
            rows = np.concatenate(self._scored) if self._scored else np.zeros(0, np.int64)
            self.poisson_q, self.q_max = np.full((len(self.table), 4), np.nan), np.full(len(self.table), np.nan)
            self.poisson_q[rows] = bh_rows(self.poisson_p[rows])
            self.q_max[rows] = _nan_extreme(np.maximum, self.poisson_q[rows])


def _read_pair(f, norm, A, B, res, device):
    """read_trans_contacts, or None when the file has no such chromosome or no matrix for the pair."""
    from .hicfile import HicError
    from .trans import read_trans_contacts
    try:
        return read_trans_contacts(f, norm, A, B, res, device=device)
    except NameError:
        return None
    except HicError as e:
        if e.code == -4 and ("is not in the file" in str(e) and "chromosome" in str(e) or "no matrix for the pair" in str(e)):
            return None
        raise


def _pileup_trans(f, table, res, chromosomes, norm, bias, balance, w, q, n_min, x_max, device, verbose, peak=None):
    """pileup() in trans mode: one pile-up per chromosome pair."""
    import torch
    from .request import balance_on_trans, trans_input
    why = trans_input((f,)) or balance_on_trans(balance or None)
    if why is None and bias:
        why = "-b does not apply to inter-chromosomal pairs"
    if why:
        raise PileupError(why)
    status, a, b, pairs = classify(table, res, chromosomes, n_min, x_max, trans=True)
    out = PileupResult(table, status, w, q, peak)
    S = 2 * w + 1
    tot = [np.zeros((S, S)) for _ in range(4)]
    for A, B in pairs:
        pair = frozenset((_key(A), _key(B)))
        rows = [k for k in range(len(table)) if status[k] is None
                and frozenset((_key(table.chr1[k]), _key(table.chr2[k]))) == pair]
        part, used = _empty_result(w, q, peak), []
        got = _read_pair(f, norm, A, B, res, device)
        if got is None:
            for k in rows:
                status[k] = "no_pair"
        else:
            x, y, v, _res = got
            n1 = int(torch.as_tensor(x).max().item()) + 1
            n2 = int(torch.as_tensor(y).max().item()) + 1
            for k in rows:
                status[k] = "off_map" if a[k] >= n1 or b[k] >= n2 else "used"
            used = [k for k in rows if status[k] == "used"]
            part = pileup_trans_records(x, y, v, n1, n2, a[used], b[used], w, q, **_peak_kw(peak))
            del x, y, v, got
            out.take(used, part)
        part = {k_: v_ for k_, v_ in part.items() if k_ not in ("valid", "expected", "obs", "oe")}   # device arrays freed
        out.chromosomes.append(("%s,%s" % (A, B), len(rows), len(used), part))
        for t, name in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
            t += part[name]                              # genome-wide: in the order the pairs ran
        if verbose:
            print("pile-up of the pair %s,%s: %d of %d rows used, P2M %r" % (A, B, len(used), len(rows), part["metrics"]["P2M"]))
    out.total(tot)
    return out


WINDOW_SHARE = 0.25               # genome mode: the windows of a batch's loops may take this share of the device's free memory


def window_bytes(loops, w):
    """device bytes of the obs and oe windows of `loops` loops"""
    return 16 * (2 * int(w) + 1) ** 2 * int(loops)


def window_budget():
    """the bytes the windows of one batch may take: WINDOW_SHARE of the device memory that is free now"""
    import torch
    return int(WINDOW_SHARE * int(torch.cuda.mem_get_info()[0]))


def _window_batches(loops_of, w, budget, names):
    """Consecutive pairs (indices into loops_of, the pairs' used-loop counts) whose windows fit `budget` bytes together.  A
    single pair that does not fit is a PileupError with both numbers, before anything is launched."""
    for p, n in enumerate(loops_of):
        if window_bytes(n, w) > budget:
            raise PileupError("the windows of the pair %s (%d loops, w = %d) need %d bytes of device memory; %d bytes (%d%% of "
                              "what is free) are allowed" % (names[p], n, w, window_bytes(n, w), budget, round(100 * WINDOW_SHARE)))
    batch, held = [], 0
    for p, n in enumerate(loops_of):
        if batch and held + window_bytes(n, w) > budget:
            yield batch
            batch, held = [], 0
        batch.append(p)
        held += window_bytes(n, w)
    if batch:
        yield batch


def _pileup_trans_genome(f, table, res, chromosomes, norm, bias, balance, method, pixels, pairs_zero_based, w, q, n_min, x_max,
                         device, verbose, peak=None):
    """pileup() in trans mode on the genome-balanced map (the module docstring has the rules): the genome read and balanced
    once, every pair's records balanced and piled up in shared launches, one host wait per batch."""
    from . import pairs as pairs_mod
    from .balance import BalanceError, report
    from .balance_genome import APPLY_BATCH_RECORDS, balanced_segments, check_genome_request, read_genome, solve_genome
    from .request import keep_trans_rows
    from_pairs = pairs_mod.is_pairs(f)
    try:
        method, pixels = check_genome_request(method, pixels, [f], bias or None, norm, balance or None, 1, "all",
                                              pairs_trans=from_pairs)
    except BalanceError as e:
        raise PileupError(str(e))
    why = keep_trans_rows([f], pairs_zero_based) if from_pairs else None      # the one parse of a pairs file, host only
    if why:
        raise PileupError(why)
    status, a, b, pairs = classify(table, res, chromosomes, n_min, x_max, trans=True)
    out = PileupResult(table, status, w, q, peak)
    import torch
    try:
        gb = solve_genome(read_genome(f, res, pixels, device, pairs_zero_based, verbose), method)
    except BalanceError as e:
        raise PileupError(str(e))
    if verbose:
        report(gb.info, gb.label)
    at = {frozenset((_key(A), _key(B))): p for p, (A, B) in enumerate(pairs)}
    rows_of, used_of, live = [[] for _ in pairs], [[] for _ in pairs], []
    for k in range(len(table)):                         # one pass: every eligible row to its pair
        if status[k] is None:
            rows_of[at[frozenset((_key(table.chr1[k]), _key(table.chr2[k])))]].append(k)
    for p, (A, B) in enumerate(pairs):
        rows = rows_of[p]
        try:
            have = gb.records(A, B) is not None
        except NameError:                               # a chromosome of the pair is not in the file
            have = False
        if not have:
            for k in rows:
                status[k] = "no_pair"
            continue
        n1, n2 = gb.bins[gb.index(A)], gb.bins[gb.index(B)]
        for k in rows:
            status[k] = "off_map" if a[k] >= n1 or b[k] >= n2 else "used"
        used_of[p] = [k for k in rows if status[k] == "used"]
        live.append(p)
    parts = [_empty_result(w, q, peak) for _ in pairs]
    drop = ("valid", "expected", "obs", "oe", "kept")
    with torch.cuda.device(gb.device):
        budget = window_budget()
        names = ["%s,%s" % pairs[p] for p in live]
        for group in list(_window_batches([len(used_of[p]) for p in live], w, budget, names)):
            mine = [live[i] for i in group]
            for k0, k1, x, y, v, seg in balanced_segments(gb, [pairs[p] for p in mine], release=True,
                                                          max_records=APPLY_BATCH_RECORDS):
                batch = mine[k0:k1]
                dims = [(gb.bins[gb.index(pairs[p][0])], gb.bins[gb.index(pairs[p][1])]) for p in batch]
                got = pileup_trans_batch(x, y, v, seg, dims, [(a[used_of[p]], b[used_of[p]]) for p in batch], w, q,
                                         **_peak_kw(peak))
                del x, y, v
                for p, part in zip(batch, got):
                    if part["kept"] == 0:               # nothing of the pair survives the balancing: its result is discarded
                        for k in rows_of[p]:
                            status[k] = "no_pair"
                        used_of[p] = []
                        continue
                    out.take(used_of[p], part)
                    parts[p] = {k_: v_ for k_, v_ in part.items() if k_ not in drop}
                del got
    S = 2 * w + 1
    tot = [np.zeros((S, S)) for _ in range(4)]
    for p, (A, B) in enumerate(pairs):
        part = {k_: v_ for k_, v_ in parts[p].items() if k_ not in drop}
        out.chromosomes.append(("%s,%s" % (A, B), len(rows_of[p]), len(used_of[p]), part))
        for t, name in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
            t += part[name]                              # genome-wide: in the order of first appearance
        if verbose:
            print("pile-up of the pair %s,%s: %d of %d rows used, P2M %r" % (A, B, len(used_of[p]), len(rows_of[p]),
                                                                            part["metrics"]["P2M"]))
    out.total(tot)
    return out


def pileup(f, loops, res, chromosomes=None, norm=False, bias=False, balance=None, w=10, q=6, n_min=None, x_max=None,
           device=None, verbose=False, trans=False, balance_genome=None, balance_pixels="all", pairs_zero_based=False, peak=None,
           poisson=False):
    """Pile up map `f` around the loops of `loops` (a TSV path or a LoopTable) at resolution `res` (bp).  The reader
    arguments (`norm`, `bias`, `balance`) mean what they mean for the caller; `n_min` is in bins (None: 30), `x_max` in bp.
    trans=True piles up the inter-chromosomal rows instead, pair by pair (the module docstring has the rules); in that mode
    `chromosomes` of the result holds ("A,B", rows in, loops used, pile-up dict).  balance_genome="NEWTON" | "ICE" (with
    trans=True; balance_pixels "all" | "inter"; pairs_zero_based for a pairs file) piles the rows up on the genome-balanced map
    of a raw `.hic` file or a `.pairs` / `.pairs.gz` file, every pair in shared launches.  peak=p (0 <= p < w) scores every
    used loop against its local background in any of the three modes ("Enrichment" in the module docstring).  poisson=True (with `peak` and balance="ICE" |
    "NEWTON" on a `.hic` or pairs file, intra-chromosomal only) adds each used loop's Poisson p-values from the raw counts and
    the run's BH q-values ("Significance").  Returns a PileupResult."""
    w, q, res = int(w), int(q), int(res)
    check_window(w, q)
    if peak is not None:
        peak = int(peak)
        check_peak(w, peak)
    if poisson:
        why = poisson_conflict(f, peak is not None, balance, bias, trans, balance_genome is not None)
        if why:
            raise PileupError(why)
    table = read_loops(loops) if isinstance(loops, (str, os.PathLike)) else loops
    if balance_genome is not None:
        if not trans:
            raise PileupError("--balance-genome is for inter-chromosomal pile-ups: give --trans (--balance balances one "
                              "chromosome's own map)")
        return _pileup_trans_genome(f, table, res, chromosomes, norm, bias, balance, balance_genome, balance_pixels,
                                    pairs_zero_based, w, q, n_min, x_max, device, verbose, peak)
    if trans:
        return _pileup_trans(f, table, res, chromosomes, norm, bias, balance, w, q, n_min, x_max, device, verbose, peak)
    status, x, y, selected = classify(table, res, chromosomes, n_min, None if x_max is None else int(x_max) // res)
    out = PileupResult(table, status, w, q, peak, poisson)
    S = 2 * w + 1
    tot = [np.zeros((S, S)) for _ in range(4)]
    for chrom in selected:
        rows = [k for k in range(len(table)) if _key(table.chr1[k]) == _key(chrom) and status[k] != "trans"]
        cand = [k for k in rows if status[k] is None]
        part = _empty_result(w, q, peak, poisson)
        used = []
        if cand:
            D = int(max(y[k] - x[k] for k in cand)) + 2 * w
            raw = None
            if poisson:
                band, n, raw = _read_band_raw(f, chrom, res, D, balance, device, verbose)
            else:
                band, n = _read_band(f, chrom, res, D, norm, bias, balance, device, verbose)
            if band is None:
                for k in cand:
                    status[k] = "no_chrom"
            else:
                for k in cand:
                    status[k] = "off_map" if y[k] >= n else "used"
                used = [k for k in cand if status[k] == "used"]
                try:
                    part = pileup_band(band, n, D, x[used], y[used], w, q, **_peak_kw(peak), **({"poisson": raw} if poisson else {}))
                except PileupError as e:
                    if "not an integer value" not in str(e):
                        raise
                    raise PileupError("chromosome %s holds a count that is not an integer value: --poisson needs raw integer "
                                      "counts" % chrom)
                del band, raw
            out.take(used, part)
        part = {k_: v for k_, v in part.items() if k_ not in ("valid", "expected", "obs", "oe")}   # device arrays freed
        out.chromosomes.append((chrom, len(rows), len(used), part))
        for t, name in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
            t += part[name]                              # genome-wide: in the order the chromosomes ran
        if verbose:
            print("pile-up of chromosome %s: %d of %d rows used, P2LL %r" % (chrom, len(used), len(rows),
                                                                           part["metrics"]["P2LL"]))
    out.total(tot)
    return out


class PileupPairResult:
    """What pileup_pair() returns: `first`, `second` (the PileupResult of each sample; they share `table` and ONE `status`
    list), per row `r1`, `r2`, `lfc_n` ([rows, 4]: DONUT, LL, H, V) and `lfc`, NaN for a row that was not used; `chromosomes`
    = [(name, loops used, compare dict)] in run order (trans: "A,B"); `all` = the genome-wide compare dict
    (compare_aggregate's keys)."""

    def __init__(self, table, status, w, q, peak):
        self.table, self.status, self.w, self.q, self.peak = table, status, w, q, peak
        self.first, self.second = PileupResult(table, status, w, q), PileupResult(table, status, w, q)
        L, S = len(table), 2 * w + 1
        self.r1, self.r2, self.lfc_n = np.full((L, 4), np.nan), np.full((L, 4), np.nan), np.full((L, 4), np.nan)
        self.lfc = np.full(L, np.nan)
        self.chromosomes = []
        self.all = None
        self._tot = [[np.zeros((S, S)) for _ in range(4)], [np.zeros((S, S)) for _ in range(4)], [np.zeros((S, S)) for _ in range(3)]]

    def add(self, name, rows_in, used, part1, part2, cmp):
        """one chromosome's or pair's three dicts (the loops of `used`, table rows, in their order): the per-row values, the
        per-sample entries and the genome-wide partial sums, in the order of the calls"""
        rows = np.asarray(used, np.int64)
        self.r1[rows], self.r2[rows], self.lfc_n[rows], self.lfc[rows] = cmp["r1"], cmp["r2"], cmp["lfc_n"], cmp["lfc"]
        for res, part, tot in ((self.first, part1, self._tot[0]), (self.second, part2, self._tot[1])):
            res.take(used, part)
            part = {k: v for k, v in part.items() if k not in ("valid", "expected", "obs", "oe")}       # device arrays freed
            res.chromosomes.append((name, rows_in, len(used), part))
            for t, key in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
                t += part[key]
        for t, key in zip(self._tot[2], ("t1", "t2", "count")):
            t += cmp[key]
        self.chromosomes.append((name, len(used), {k: v for k, v in cmp.items() if k not in ("sums", "r1", "r2", "lfc_n", "lfc")}))

    def total(self):
        self.first.total(self._tot[0])
        self.second.total(self._tot[1])
        self.all = compare_aggregate(self._tot[2][0], self._tot[2][1], self._tot[2][2], self.w, self.q, self.peak)


def _pileup_pair_trans(f1, f2, table, res, chromosomes, norm, bias, bias2, balance, w, q, n_min, x_max, device, verbose, peak):
    """pileup_pair() in trans mode: one pair of pile-ups per chromosome pair, from the files' stored vectors."""
    import torch
    from .request import balance_on_trans, trans_input
    why = trans_input((f1,)) or trans_input((f2,)) or balance_on_trans(balance or None)
    if why is None and (bias or bias2):
        why = "-b / -b2 do not apply to inter-chromosomal pairs"
    if why:
        raise PileupError(why)
    status, a, b, pairs = classify(table, res, chromosomes, n_min, x_max, trans=True)
    out = PileupPairResult(table, status, w, q, peak)
    for A, B in pairs:
        pair = frozenset((_key(A), _key(B)))
        rows = [k for k in range(len(table)) if status[k] is None
                and frozenset((_key(table.chr1[k]), _key(table.chr2[k]))) == pair]
        got = [_read_pair(f, norm, A, B, res, device) for f in (f1, f2)]          # both maps before either is piled up
        dims = [None if g is None else (int(torch.as_tensor(g[0]).max().item()) + 1, int(torch.as_tensor(g[1]).max().item()) + 1)
                for g in got]
        for k, s in zip(rows, joint_status_trans(a[rows], b[rows], dims[0], dims[1])):
            status[k] = s
        used = [k for k in rows if status[k] == "used"]
        if dims[0] is None or dims[1] is None:
            p1, p2, cmp = _empty_result(w, q), _empty_result(w, q), _empty_compare(w, q, peak)
        else:
            p1, p2, cmp = pileup_trans_records_pair(got[0][:3], dims[0], got[1][:3], dims[1], a[used], b[used], w, q, peak)
        del got
        out.add("%s,%s" % (A, B), len(rows), used, p1, p2, cmp)
        if verbose:
            print("pile-up of the pair %s,%s on both maps: %d of %d rows used, LFC_P2LL %r" % (A, B, len(used), len(rows),
                                                                                          cmp["lfc_p2ll"]))
    out.total()
    return out


def pileup_pair(f1, f2, loops, res, chromosomes=None, norm=False, bias=False, balance=None, w=10, q=6, n_min=None, x_max=None,
                device=None, verbose=False, trans=False, peak=DEFAULT_PEAK, bias2=False):
    """Pile up the maps `f1` and `f2` around the loops of `loops` and score what differs ("Two maps" in the module docstring).
    The arguments are pileup()'s and apply to both maps alike; `bias` is the bias file of f1, `bias2` that of f2; `peak` is the
    peak half-width of the four neighbourhoods.  Returns a PileupPairResult."""
    w, q, res, peak = int(w), int(q), int(res), int(peak)
    check_window(w, q)
    check_peak(w, peak)
    table = read_loops(loops) if isinstance(loops, (str, os.PathLike)) else loops
    if trans:
        return _pileup_pair_trans(f1, f2, table, res, chromosomes, norm, bias, bias2, balance, w, q, n_min, x_max, device, verbose,
                                  peak)
    status, x, y, selected = classify(table, res, chromosomes, n_min, None if x_max is None else int(x_max) // res)
    out = PileupPairResult(table, status, w, q, peak)
    for chrom in selected:
        rows = [k for k in range(len(table)) if _key(table.chr1[k]) == _key(chrom) and status[k] != "trans"]
        cand = [k for k in rows if status[k] is None]
        p1, p2, cmp, used = _empty_result(w, q), _empty_result(w, q), _empty_compare(w, q, peak), []
        if cand:
            D = int(max(y[k] - x[k] for k in cand)) + 2 * w
            bands, ns = [], []
            for f, b in ((f1, bias), (f2, bias2)):       # both bands before either is piled up: the smaller n decides off_map
                band, n = _read_band(f, chrom, res, D, norm, b, balance, device, verbose)
                bands.append(band)
                ns.append(None if band is None else n)
            for k, s in zip(cand, joint_status(y[cand], ns[0], ns[1])):
                status[k] = s
            used = [k for k in cand if status[k] == "used"]
            if ns[0] is not None and ns[1] is not None:
                # the bands leave the list in the call: each is freed inside it as soon as its sample's oe is in hand
                p1, p2, cmp = pileup_band_pair(bands.pop(0), ns[0], bands.pop(0), ns[1], D, x[used], y[used], w, q, peak)
            del bands
        out.add(chrom, len(rows), used, p1, p2, cmp)
        if verbose:
            print("pile-up of chromosome %s on both maps: %d of %d rows used, LFC_P2LL %r" % (chrom, len(used), len(rows),
                                                                                         cmp["lfc_p2ll"]))
    out.total()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# output files
# ----------------------------------------------------------------------------------------------------------------------
def _r(v):
    return repr(float(v))


def write_matrix(path, M):
    with open(path, "w") as fh:
        fh.write("".join("\t".join(_r(v) for v in row) + "\n" for row in np.asarray(M)))


def write_outputs(prefix, res):
    """PREFIX.apa.tsv, PREFIX.oe.tsv, PREFIX.stats.tsv, PREFIX.loops.tsv of a PileupResult."""
    write_matrix(prefix + ".apa.tsv", res.all["apa"])
    write_matrix(prefix + ".oe.tsv", res.all["apa_oe"])

    def stats_row(name, rows_in, used, p):
        return "%s\t%d\t%d\t%s\t%s\n" % (name, rows_in, used, "\t".join(_r(p["metrics"][m]) for m in METRICS),
                                        _r(p["metrics_oe"]["P2LL"]))
    with open(prefix + ".stats.tsv", "w") as fh:
        fh.write(STATS_HEADER)
        for name, rows_in, used, p in res.chromosomes:
            fh.write(stats_row(name, rows_in, used, p))
        fh.write(stats_row("all", len(res.table), sum(u for _, _, u, _ in res.chromosomes), res.all))
    with open(prefix + ".loops.tsv", "w") as fh:
        fh.write(res.table.header + "\t" + "\t".join(LOOP_COLUMNS) + "\n")
        fh.write("".join("%s\t%s\t%s\t%s\t%s\n" % (line, s, _r(a), _r(b), _r(c)) for line, s, a, b, c in
                         zip(res.table.lines, res.status, res.obs_center, res.oe_center, res.p2ll)))


def write_enrichment(prefix, res, min_enrichment=None):
    """PREFIX.enrich.tsv and PREFIX.enrich.stats.tsv of a PileupResult made with `peak`; with min_enrichment = T also
    PREFIX.enriched.tsv, the `used` rows with FE_MIN >= T as a loop list (NaN fails).  Returns how many rows that list holds
    (None without T)."""
    if res.peak is None:
        raise PileupError("this pile-up ran without a peak half-width: there is no enrichment to write")
    with open(prefix + ".enrich.tsv", "w") as fh:
        fh.write(res.table.header + "\t" + "\t".join(ENRICH_COLUMNS) + "\n")
        for k, line in enumerate(res.table.lines):
            vals = [res.obs_center[k], res.e_center[k]] + list(res.enrich_exp[k]) + list(res.enrich_fe[k]) + [res.fe_min[k]]
            fh.write("%s\t%s\t%s\n" % (line, res.status[k], "\t".join(_r(v) for v in vals)))
    with open(prefix + ".enrich.stats.tsv", "w") as fh:
        fh.write(ENRICH_STATS_HEADER)
        for name, _rows_in, used, part in res.chromosomes:
            fh.write("%s\t%d\t%s\n" % (name, used, "\t".join(_r(v) for v in part["enrich_agg"])))
        fh.write("all\t%d\t%s\n" % (sum(u for _, _, u, _ in res.chromosomes), "\t".join(_r(v) for v in res.all["enrich_agg"])))
    if min_enrichment is None:
        return None
    with np.errstate(invalid="ignore"):
        keep = [k for k in range(len(res.table)) if res.status[k] == "used" and res.fe_min[k] >= min_enrichment]
    with open(prefix + ".enriched.tsv", "w") as fh:
        fh.write(res.table.header + "\n")
        fh.write("".join(res.table.lines[k] + "\n" for k in keep))
    return len(keep)


def write_poisson(prefix, res, max_fdr=None):
    """PREFIX.poisson.tsv of a PileupResult made with `poisson` (each row as read, then POISSON_COLUMNS; NaN for a row that is not
    `used`); with max_fdr = T also PREFIX.significant.tsv, the `used` rows with Q_MAX <= T as a loop list (NaN fails).  Returns
    (used loops, those with a defined P_MAX, the rows of that list or None without T)."""
    if not res.poisson or res.poisson_q is None:
        raise PileupError("this pile-up ran without `poisson`: there is no significance to write")
    with open(prefix + ".poisson.tsv", "w") as fh:
        fh.write(res.table.header + "\t" + "\t".join(POISSON_COLUMNS) + "\n")
        for k, line in enumerate(res.table.lines):
            vals = [res.raw_center[k], res.bias1[k], res.bias2[k]] + list(res.poisson_lambda[k]) + list(res.poisson_p[k]) \
                + [res.p_max[k]] + list(res.poisson_q[k]) + [res.q_max[k]]
            fh.write("%s\t%s\t%s\n" % (line, res.status[k], "\t".join(_r(v) for v in vals)))
    used = [k for k in range(len(res.table)) if res.status[k] == "used"]
    defined = sum(1 for k in used if not np.isnan(res.p_max[k]))
    if max_fdr is None:
        return len(used), defined, None
    with np.errstate(invalid="ignore"):
        keep = [k for k in used if res.q_max[k] <= max_fdr]
    with open(prefix + ".significant.tsv", "w") as fh:
        fh.write(res.table.header + "\n")
        fh.write("".join(res.table.lines[k] + "\n" for k in keep))
    return len(used), defined, len(keep)


def write_compare(prefix, res, min_lfc=None):
    """PREFIX.compare.tsv, PREFIX.diff.tsv and PREFIX.compare.stats.tsv of a PileupPairResult; with min_lfc = T also
    PREFIX.up1.tsv, the `used` rows with LFC >= T, and PREFIX.up2.tsv, those with LFC <= -T, as loop lists (NaN fails both).
    Returns the two lists' lengths (None without T).  The per-sample files are write_outputs(prefix + ".1", res.first) and
    write_outputs(prefix + ".2", res.second)."""
    with open(prefix + ".compare.tsv", "w") as fh:
        fh.write(res.table.header + "\t" + "\t".join(COMPARE_COLUMNS) + "\n")
        for k, line in enumerate(res.table.lines):
            vals = [res.first.oe_center[k], res.second.oe_center[k]] + list(res.r1[k]) + list(res.r2[k]) + list(res.lfc_n[k]) \
                + [res.lfc[k]]
            fh.write("%s\t%s\t%s\n" % (line, res.status[k], "\t".join(_r(v) for v in vals)))
    write_matrix(prefix + ".diff.tsv", res.all["diff"])

    def stats_row(name, used, c):
        return "%s\t%d\t%s\n" % (name, used, "\t".join(_r(v) for v in [c["p2ll_1"], c["p2ll_2"], c["lfc_p2ll"]] + list(c["agg_lfc"])))
    with open(prefix + ".compare.stats.tsv", "w") as fh:
        fh.write(COMPARE_STATS_HEADER)
        for name, used, c in res.chromosomes:
            fh.write(stats_row(name, used, c))
        fh.write(stats_row("all", sum(u for _, u, _ in res.chromosomes), res.all))
    if min_lfc is None:
        return None
    kept = []
    with np.errstate(invalid="ignore"):
        # by the LFC as written: repr() round-trips a float64, so this is the value a reader of compare.tsv sees
        for ext, ok in ((".up1.tsv", res.lfc >= min_lfc), (".up2.tsv", res.lfc <= -min_lfc)):
            keep = [k for k in range(len(res.table)) if res.status[k] == "used" and ok[k]]
            with open(prefix + ext, "w") as fh:
                fh.write(res.table.header + "\n")
                fh.write("".join(res.table.lines[k] + "\n" for k in keep))
            kept.append(len(keep))
    return tuple(kept)


# ----------------------------------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------------------------------
def parse_args(args):
    p = argparse.ArgumentParser(description="Aggregate peak analysis (APA) of a Mustache loop list on the GPU")
    p.add_argument("-f", "--file", dest="f_path", required=True, help="contact map (text + -b, .hic, .cool, .mcool)")
    p.add_argument("-l", "--loops", dest="loops", required=True, help="loop list: a TSV written by Mustache")
    p.add_argument("-r", "--resolution", dest="resolution", required=True, help="resolution of the map")
    p.add_argument("-o", "--outfile", dest="prefix", required=True, help="output prefix")
    p.add_argument("-ch", "--chromosome", dest="chromosome", nargs="+", default=None,
                   help="chromosomes to use (default: those of the cis rows, in order of first appearance)")
    p.add_argument("-b", "--biases", dest="biasfile", default=None, help="bias vector of a text map")
    p.add_argument("-norm", "--normalization", dest="norm_method", default=False, help=".hic normalisation (KR, VC, NONE)")
    p.add_argument("--balance", dest="balance", default=None, metavar="ICE|NEWTON",
                   help="balance the raw map on the GPU (ICE or NEWTON)")
    p.add_argument("-w", "--window", dest="w", type=int, default=10, help="window half-width in bins (default 10, at most 64)")
    p.add_argument("-q", "--corner", dest="q", type=int, default=6, help="corner size in bins (default 6)")
    p.add_argument("-n", "--min-distance", dest="n_min", type=int, default=None,
                   help="smallest loop size y - x in bins (default 30)")
    p.add_argument("-x", "--max-distance", dest="x_max", default=None, help="largest loop size in bp (default: none)")
    p.add_argument("--trans", dest="trans", action="store_true",
                   help="pile up the inter-chromosomal rows, pair by pair (.hic / .cool; -ch keeps the pairs inside the list)")
    from .balance_genome import add_arguments
    add_arguments(p)                 # --balance-genome, --balance-pixels, --pairs-trans: with --trans, the genome-balanced map
    p.add_argument("--pairs-zero-based", dest="pairs_zero_based", action="store_true",
                   help="OPTIONAL: .pairs / .pairs.gz input only: positions are 0-based (bin = pos // res)")
    p.add_argument("--enrich", dest="enrich", action="store_true",
                   help="score every used loop against its donut, lower-left, horizontal and vertical neighbourhoods: "
                        "PREFIX.enrich.tsv and PREFIX.enrich.stats.tsv")
    p.add_argument("--peak", dest="peak", type=int, default=None, metavar="P",
                   help="with --enrich: half-width of the peak box the neighbourhoods leave out (default %d, below -w)" % DEFAULT_PEAK)
    p.add_argument("--min-enrichment", dest="min_enrichment", type=float, default=None, metavar="T",
                   help="with --enrich: also write PREFIX.enriched.tsv, the used rows with FE_MIN >= T as a loop list")
    p.add_argument("--poisson", dest="poisson", action="store_true",
                   help="with --enrich and --balance ICE|NEWTON on a .hic or pairs file: a Poisson p-value of every used loop's raw "
                        "centre count against each neighbourhood and BH q-values over the whole list: PREFIX.poisson.tsv")
    p.add_argument("--max-fdr", dest="max_fdr", type=float, default=None, metavar="T",
                   help="with --poisson: also write PREFIX.significant.tsv, the used rows with Q_MAX <= T as a loop list")
    p.add_argument("-f2", "--file2", dest="f2_path", default=None,
                   help="a second contact map: pile the list up on both maps and score what differs (PREFIX.1.*, PREFIX.2.*, "
                        "PREFIX.compare.tsv, PREFIX.diff.tsv, PREFIX.compare.stats.tsv; --peak sets the neighbourhoods)")
    p.add_argument("-b2", "--biases2", dest="biasfile2", default=None, help="with -f2: bias vector of the second text map")
    p.add_argument("--min-lfc", dest="min_lfc", type=float, default=None, metavar="T",
                   help="with -f2: also write PREFIX.up1.tsv (used rows with LFC >= T) and PREFIX.up2.tsv (LFC <= -T)")
    return p.parse_args(args)


def compare_request(args, world):
    """What -f2 / -b2 / --min-lfc ask: the peak half-width of a two-map run, None for a run without -f2; PileupError with the
    text of the `Error:` line for a combination that cannot be honoured.  Reads nothing and touches no GPU."""
    if args.f2_path is None:
        for flag, given in (("-b2", args.biasfile2), ("--min-lfc", args.min_lfc)):
            if given is not None:
                raise PileupError("%s without -f2: it belongs to the pile-up on two maps; give -f2 FILE" % flag)
        return None
    if world > 1:
        raise PileupError("the pile-up on two maps runs on one GPU only (this run has %d ranks)" % world)
    if not os.path.exists(args.f2_path):
        raise PileupError("Couldn't find the second contact file %s" % args.f2_path)
    if args.biasfile2 is not None and not os.path.exists(args.biasfile2):
        raise PileupError("Couldn't find the bias file of the second map %s" % args.biasfile2)
    if args.enrich or args.min_enrichment is not None:
        raise PileupError("-f2 with %s: the enrichment of every loop on one sample alone is what a run without -f2 gives; "
                          "the two-map run scores the difference (--peak, --min-lfc)"
                          % ("--enrich" if args.enrich else "--min-enrichment"))
    for flag, given in (("--balance-genome", args.balance_genome is not None), ("--balance-pixels", args.balance_pixels_given),
                        ("--pairs-trans", args.pairs_trans)):
        if given:
            raise PileupError("-f2 with %s: the pile-up on two genome-balanced maps is not built; pile each map up alone" % flag)
    if args.min_lfc is not None and not (math.isfinite(args.min_lfc) and args.min_lfc > 0):
        raise PileupError("--min-lfc %r: the threshold T must be finite and > 0 (up1 holds LFC >= T, up2 LFC <= -T)" % args.min_lfc)
    peak = DEFAULT_PEAK if args.peak is None else args.peak
    if not 0 <= peak < args.w:
        raise PileupError("--peak %d with -w %d: the peak half-width P must be in 0 .. w - 1 (P >= w leaves no neighbourhood)"
                          % (peak, args.w))
    return peak


POISSON_INPUT = "--poisson on %s: the significance needs raw integer counts, one record per pixel -- a .hic file or a .pairs / " \
                ".pairs.gz file (text counts may be fractional and may repeat a pixel; a .cool file is not read raw)"


def poisson_conflict(f, enrich, balance, bias=None, trans=False, genome=False, f2=None, world=1):
    """Why a run cannot take --poisson (the text of the `Error:` line), None when it can.  Reads nothing."""
    from .pairs import is_pairs
    if not enrich:
        return "--poisson without --enrich: the p-values are taken against the four neighbourhoods of the enrichment; give --enrich"
    if f2 is not None:
        return "--poisson with -f2: the significance of a loop on two maps is not built; pile each map up alone"
    if genome:
        return "--poisson with --balance-genome: the genome-balanced pile-up keeps no raw counts beside the map"
    if trans:
        return "--poisson with --trans: inter-chromosomal pile-ups keep no raw counts beside the map; it is for intra-chromosomal loops"
    if not balance or str(balance).upper() not in ("ICE", "NEWTON"):
        return "--poisson without --balance ICE|NEWTON: stored vectors and -b leave no raw counts in hand; give --balance" \
            + (" (and drop -b)" if bias else "")
    if not (is_pairs(f) or str(f).endswith(".hic")):
        return POISSON_INPUT % f
    if world > 1:
        return "--poisson in a multi-rank run (world size %d): the q-values are taken over the whole list on one GPU" % world
    return None


def poisson_request(args, f, world):
    """What --poisson / --max-fdr ask: (True, the threshold or None), (False, None) for a run without them; PileupError with
    the text of the `Error:` line for a combination that cannot be honoured.  Reads nothing and touches no GPU."""
    if not args.poisson:
        if args.max_fdr is not None:
            raise PileupError("--max-fdr without --poisson: it selects by the q-values of the significance test; give --poisson")
        return False, None
    why = poisson_conflict(f, args.enrich, args.balance, args.biasfile, args.trans,
                           args.balance_genome is not None or args.balance_pixels_given or args.pairs_trans, args.f2_path, world)
    if why:
        raise PileupError(why)
    if args.max_fdr is not None and not 0.0 < args.max_fdr <= 1.0:              # a NaN fails both comparisons
        raise PileupError("--max-fdr %r: the threshold T must lie in (0, 1] (significant.tsv holds Q_MAX <= T)" % args.max_fdr)
    return True, args.max_fdr


def enrich_request(args):
    """What --enrich / --peak / --min-enrichment ask: the peak half-width, None for a run without them; PileupError with the
    text of the `Error:` line for a combination that cannot be honoured.  Reads nothing and touches no GPU."""
    if not args.enrich:
        for flag, given in (("--peak", args.peak), ("--min-enrichment", args.min_enrichment)):
            if given is not None:
                raise PileupError("%s without --enrich: it belongs to the enrichment of every loop; give --enrich" % flag)
        return None
    peak = DEFAULT_PEAK if args.peak is None else args.peak
    if not 0 <= peak < args.w:
        raise PileupError("--peak %d with -w %d: the peak half-width P must be in 0 .. w - 1 (P >= w leaves no neighbourhood)"
                          % (peak, args.w))
    return peak


def genome_request(args, f, world):
    """What --balance-genome / --balance-pixels / --pairs-trans / --pairs-zero-based ask of a pile-up: (method, pixels) of a
    genome-mode run, None for a run without them; PileupError with the text of the `Error:` line for a combination that cannot
    be honoured.  Reads nothing and touches no GPU."""
    from .balance import BalanceError
    from .balance_genome import check_genome_request
    from .pairs import is_pairs
    pairs_file = is_pairs(f)
    if args.pairs_trans and not pairs_file:
        raise PileupError("--pairs-trans is for .pairs / .pairs.gz input (%s is none)" % f)
    if args.pairs_zero_based and not pairs_file:
        raise PileupError("--pairs-zero-based is for .pairs / .pairs.gz input (%s is none)" % f)
    if args.pairs_zero_based and not args.pairs_trans:
        raise PileupError("--pairs-zero-based without --pairs-trans: only the genome-balanced pile-up (--trans --pairs-trans "
                          "--balance-genome ICE|NEWTON) bins a pairs file with it")
    asked = args.balance_genome is not None or args.balance_pixels_given
    if pairs_file and (args.trans or asked) and not args.pairs_trans:
        raise PileupError("%s without --pairs-trans: only intra-chromosomal loops are piled up from a pairs file without it; give "
                          "--trans --pairs-trans --balance-genome ICE|NEWTON" % f)
    if args.pairs_trans and args.balance_genome is None:
        raise PileupError("--pairs-trans without --balance-genome: %s holds raw read pairs; give --balance-genome ICE|NEWTON" % f)
    if not asked:
        return None
    if args.balance_genome is not None and not args.trans:
        raise PileupError("--balance-genome without --trans: it balances the whole genome's map for inter-chromosomal "
                          "pile-ups; use --balance for one chromosome's own map")
    try:
        return check_genome_request(args.balance_genome, args.balance_pixels, [f], args.biasfile, args.norm_method, args.balance,
                                    world, "all" if args.trans else "none", pairs_trans=args.pairs_trans)
    except BalanceError as e:
        raise PileupError(str(e))


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    from .mustache import parseBP
    from .sharding import init_from_env
    _rank, world = init_from_env()
    if world > 1:
        print("Error: pile-ups run on one GPU only (this run has %d ranks); start a single process" % world)
        return
    f = args.f_path
    if not f or not os.path.exists(f):
        print("Error: Couldn't find the specified contact files")
        return
    if not os.path.exists(args.loops):
        print("Error: Couldn't find the loop list %s" % args.loops)
        return
    res = parseBP(args.resolution)
    if not res:
        print("Error: Invalid resolution")
        return
    if args.biasfile and not os.path.exists(args.biasfile):
        print("Error: Couldn't find specified bias file")
        return
    try:
        two = compare_request(args, world)
        genome = genome_request(args, f, world)
        peak = enrich_request(args) if two is None else None         # with -f2, --peak is the two-map run's own
        poisson, max_fdr = poisson_request(args, f, world)
    except PileupError as e:
        print("Error: %s" % e)
        return
    balance = None
    if args.balance is not None:
        from .balance import BalanceError, check_request
        try:
            balance = check_request(args.balance, f, args.biasfile, args.norm_method, world)
            if two is not None:                          # --balance applies to both maps alike
                check_request(args.balance, args.f2_path, args.biasfile2, args.norm_method, world, bias_flag="-b2")
        except BalanceError as e:
            print("Error: %s" % e)
            return
    x_max = None
    if args.x_max is not None:
        x_max = parseBP(str(args.x_max))
        if not x_max:
            print("Error: Invalid -x distance %s" % args.x_max)
            return
    from .hicfile import HicError
    from .trans import TransError
    try:
        check_window(args.w, args.q)
        if two is not None:
            pair = pileup_pair(f, args.f2_path, args.loops, res, chromosomes=args.chromosome, norm=args.norm_method,
                               bias=args.biasfile or False, balance=balance, w=args.w, q=args.q, n_min=args.n_min, x_max=x_max,
                               verbose=True, trans=args.trans, peak=two, bias2=args.biasfile2 or False)
            write_outputs(args.prefix + ".1", pair.first)
            write_outputs(args.prefix + ".2", pair.second)
            kept = write_compare(args.prefix, pair, args.min_lfc)
            print("%d of %d loops piled up on both maps, peak half-width %d%s: LFC_P2LL %r -> %s.{1,2}.{apa,oe,stats,loops}.tsv, "
                  "%s.{compare,diff,compare.stats}.tsv%s"
                  % (sum(u for _, u, _ in pair.chromosomes), len(pair.table), two,
                     "" if kept is None else "; %d loops with LFC >= %r, %d with LFC <= %r" % (kept[0], args.min_lfc, kept[1],
                                                                                                -args.min_lfc),
                     pair.all["lfc_p2ll"], args.prefix, args.prefix, "" if kept is None else ", %s.{up1,up2}.tsv" % args.prefix))
            return
        res_ = pileup(f, args.loops, res, chromosomes=args.chromosome, norm=args.norm_method, bias=args.biasfile or False,
                      balance=balance, w=args.w, q=args.q, n_min=args.n_min, x_max=x_max, verbose=True, trans=args.trans,
                      balance_genome=genome[0] if genome else None, balance_pixels=genome[1] if genome else "all",
                      pairs_zero_based=args.pairs_zero_based, peak=peak, **({"poisson": True} if poisson else {}))
    except (PileupError, TransError) as e:
        print("Error: %s" % e)
        return
    except HicError as e:
        if not args.trans:
            raise
        print("Error: %s" % e)                           # a `.hic` file of version 6: the trans reader's own refusal
        return
    write_outputs(args.prefix, res_)
    a = res_.all["metrics"]
    print("%d of %d loops piled up: P2LL %r, ZscoreLL %r, P2M %r -> %s.{apa,oe,stats,loops}.tsv"
          % (sum(u for _, _, u, _ in res_.chromosomes), len(res_.table), a["P2LL"], a["ZscoreLL"], a["P2M"], args.prefix))
    if peak is not None:
        kept = write_enrichment(args.prefix, res_, args.min_enrichment)
        print("enrichment with peak half-width %d: aggregate over DONUT, LL, H, V %s -> %s.enrich.tsv, %s.enrich.stats.tsv%s"
              % (peak, ", ".join(_r(v) for v in res_.all["enrich_agg"]), args.prefix, args.prefix,
                 "" if kept is None else "; %d loops with FE_MIN >= %r -> %s.enriched.tsv" % (kept, args.min_enrichment, args.prefix)))
    if poisson:
        used, defined, kept = write_poisson(args.prefix, res_, max_fdr)
        print("significance of %d used loops: %d with a defined P_MAX%s%s -> %s.poisson.tsv%s"
              % (used, defined, "" if kept is None else ", %d with Q_MAX <= %r" % (kept, max_fdr),
                 "" if not res_.poisson_unconverged else " (%d tails did not converge: NaN)" % res_.poisson_unconverged,
                 args.prefix, "" if kept is None else ", %s.significant.tsv" % args.prefix))


if __name__ == "__main__":
    main()
