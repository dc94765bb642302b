"""Two-sample (differential) loop calling for MANY inter-chromosomal pairs in shared launches.

The rules are those of mustache_amd/diff_trans.py, pair by pair, and this module is the one host path they run on: a pair
alone (diff_trans.call_diff_trans_coo, `-ch A -ch2 B`) is a batch of one pair.  Every row of a pair is the row of that pair
run alone (tests/trans_pair_alone.py keeps the independent single-pair form).  How the work reaches the GPU is what
mustache_amd/trans_genome.py does for one sample (trans_genome.PairBatcher is the one body of both), with two samples per pair:

* A held pair costs RECORD_BYTES per record of BOTH samples against the budget.  At a flush each sample's held records are
  concatenated and ONE mst_trans_zscore_segmented per sample normalises every pair by that sample's own mean and std and
  brings the statistics and extents to the host in one copy per sample.
* Rule 2: a pair of which either sample is empty, has std = 0 or a non-finite mean or std is not tiled and yields [].
* Rule 3: n1, n2 of a pair are the maxima over both samples' extents; trans_genome.pair_table on these joint dimensions is the
  one table both samples use.
* The skip rule: mst_trans_count_tiles runs once per sample against the joint table, and a tile pair is dropped before the
  scatter when EITHER sample holds fewer than 10 000 records with v' != 0 in its window.  Rule 4 empties all four lists of a
  tile pair of which either sample has fewer than 10 000 tested pixels, and a sample's tested pixels are never more than its
  records with v' != 0 (trans_genome.py), so the rule never drops a tile pair that could report a row; a tile pair it keeps
  still meets rule 4 in the tail.
* The kept tile pairs are cut into launch groups (trans_genome.launch_groups: runs of up to `tiles_per_launch` tile pairs of
  equal C).  A group of B tile pairs is one buffer of 2 B tiles, sample 1 in [0, B), sample 2 in [B, 2 B): one
  mst_trans_scatter_worklist per sample writes into its half (the table and the slot array are shared), and everything after
  the scatter is diff_trans.pair_tile_loops.
"""
from .diff_trans import pair_tile_loops, row_order, tagged_owned_rows, tile_pair_bytes
from .trans import TRANS_CHUNK
from .trans_genome import PairBatcher, default_budget


class DiffTransGenomeCaller(PairBatcher):
    """add(index, rec1, rec2, label) pair by pair, flush() at the end; `emit(index, rows)` receives every pair's rows
    [x, y, fdr, sigma, tag] in the order the pairs were added.  `budget_bytes` bounds the records held (RECORD_BYTES each, both
    samples); the partition into batches changes no bit of the output.  `stats` counts tile PAIRS.
    run_pair([rec1, rec2], label): one pair alone (`emit` may be None)."""

    SAMPLES = 2
    UNIT = "tile pairs"
    # tile PAIRS per launch when the caller names none.  A pair of 2000 x 2000 tiles at two octaves holds 2 x 32 MB of tiles,
    # 2 x 4 MB of masks and 2 x 32 MB of D_2 in HBM, 136 MB before the record buffers (tile_pair_bytes): 32 pairs = the 64 tiles
    # of the one-sample caller's launch, ~4.4 GB.
    PAIRS_PER_LAUNCH = 32

    def __init__(self, octave_values, st, pt, pt2, emit, chunk=TRANS_CHUNK, tiles_per_launch=None, budget_bytes=None,
                 stats=None, verbose=False):
        super().__init__(octave_values, emit, chunk, tiles_per_launch or self.PAIRS_PER_LAUNCH, budget_bytes, stats,
                         verbose)
        self.st, self.pt, self.pt2 = st, pt, pt2
        self.n_octaves = len(octave_values)

    def default_budget(self):
        # per pixel of a tile pair what tile_pair_bytes counts: the tile buffers of one two-sample launch
        return default_budget(self.device, self.chunk, self.tiles_per_launch, tile_pair_bytes(1, self.n_octaves))

    def add(self, index, rec1, rec2, label=None):
        """rec: (x, y, v) host arrays or device tensors, or None / empty for a sample without a record of the pair"""
        self.hold(index, [rec1, rec2], label)

    def no_contact(self, label):
        if label is not None:
            print("There is no contact in the chromosome pair %s of one of the samples to work on." % label)

    def tile_rows(self, B, C, fill):
        return pair_tile_loops(self.eng, self.device, B, C, fill, self.st, self.pt, self.pt2)

    def owned(self, res4, tiling, i, j):
        return tagged_owned_rows(res4, tiling, i, j)

    def row_order(self, r):
        return row_order(r)


def call_diff_trans_genome(pairs, octave_values, st, pt, pt2, chunk=TRANS_CHUNK, tiles_per_launch=None, budget_bytes=None,
                           stats=None, verbose=False, labels=None):
    """Differential loops of every chromosome pair of `pairs` (pairs[p] = (rec1, rec2), rec = (x, y, v) as host arrays or
    device tensors, None or empty for a sample without records): a list with, per pair, [[x, y, fdr, sigma, tag], ...] sorted
    by (tag, x, y) -- the rows of that pair alone.  A pair of which a sample has no record, a
    non-finite mean / std or std = 0 yields [] (and, when `labels` names the pairs, the "There is no contact ..." line).
    `stats`, a dict, receives tiles_total, tiles_skipped (tile pairs), launches and batches."""
    pairs = list(pairs)
    result = [None] * len(pairs)

    def emit(i, rows):
        result[i] = rows

    caller = DiffTransGenomeCaller(octave_values, st, pt, pt2, emit, chunk=chunk, tiles_per_launch=tiles_per_launch,
                                   budget_bytes=budget_bytes, stats=stats, verbose=verbose)
    for i, (rec1, rec2) in enumerate(pairs):
        caller.add(i, rec1, rec2, None if labels is None else labels[i])
    caller.flush()
    return result
