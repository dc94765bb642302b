"""Two-sample (differential) loop calling for one inter-chromosomal pair (A, B) on the GPU: the rules and what one launch of
tile pairs runs.  The host path from records to rows is diff_trans_genome.py's (trans_genome.PairBatcher), for one pair
(call_diff_trans_coo: a batch of one) as for many.

The reference's two-sample caller is dead on a trans pair (diff_mustache.py:687-690 only prints), so the semantics are fixed
here, from trans.py's rules for one sample and diff_mustache.py:260-569 for what two samples add;
tests/diff_trans_reference.py restates them in NumPy / SciPy.

1. Input: each sample contributes every record of its A x B matrix (trans.py rule 1; `.hic`, `.cool`, `.mcool` through
   read_trans_contacts).
2. Normalisation: each sample is z-scored on its own (trans.py rule 2, mst_trans_zscore).  A sample that is empty or has
   std = 0 or a non-finite std: no rows for the pair.
3. Tiling: n1 = max over both samples of max(x) + 1, n2 likewise (the cis n = max(n1, n2)); trans_tiling(n1, n2) is the one
   tiling of both samples; ownership as in trans.py rule 3.
4. Per tile pair:
   - nz_s = c_s != 0 over the whole tile (no triangle masks, no fills); nz = nz_1 & nz_2; cd = c_1 - c_2 on nz, 0 elsewhere;
   - either sample with fewer than 50, or fewer than 10 000, tested pixels: the pair's four lists are empty.  The skip rule:
     a sample's tested pixels are its distinct pixels with v' != 0, never more than its records with v' != 0, so a tile
     pair of which either sample holds fewer than 10 000 such records in its window (mst_trans_count_tiles) has four empty
     lists and is dropped before it is scattered; the rule never drops a tile pair that could report a row, and one it
     keeps still meets the thresholds in the tail;
   - per sample the sigma loop on nz_s, BH over its found set, q < pt, the sparsity filter (x != 0, the cis windows), no
     diagonal-mean filter; a sample without a surviving candidate empties all four lists (diff_mustache.py:507); clustering
     as in trans.py rule 5;
   - pair p-value: per octave D_2 = G(sigma_2) - G(sigma_3) of cd -- the reference's quirk kept, EVERY tested level of an
     octave scores against D_2 (diff_mustache.py:336 vs :363) --, norm.fit over nz, the two-sided normal p-value at each found
     pixel (mst_diff_dog_tiles, mst_pair_pvalues_dog);
   - differential subset: the representative has pair < pt2 and v_self > v_other, v_other = 1 off the other sample's nz, its
     winning DoG value where it found the pixel, 0 where it tested it and did not;
   - a representative counts only if its tile owns it.
5. Output rows [x, y, fdr, sigma, tag], tag 1..4 = loops1, diffloops1, loops2, diffloops2, sorted by (tag, x, y) within the
   pair; the command line writes them to .loop1 / .diffloop1 / .loop2 / .diffloop2 with A in column 1 and B in column 4.
"""
from .trans import TRANS_CHUNK, TransError, owned_rows, prepared_tiles, read_trans_contacts


def pair_tile_loops(eng, dev, B, C, fill, st, pt, pt2):
    """Rule 4 on the B tile PAIRS of one launch: `fill(s, half)` scatters sample s's records into its half of one buffer of
    2 B tiles (sample 1 in [0, B), sample 2 in [B, 2 B)), then one prologue, one fused scale-space launch over both samples'
    tiles with the pair p-values (mst_diff_dog_tiles) and one batched tail.  Per tile pair its (loops1, diff_loops1, loops2,
    diff_loops2), rows [x, y, fdr, sigma] in TILE coordinates."""
    import torch
    from .diff_mustache import _pair_tails

    def both(c):
        fill(0, c[:B])
        fill(1, c[B:])
    c, nz, nzc = prepared_tiles(eng, dev, 2 * B, C, both)
    with torch.cuda.device(dev):
        batch = eng.run_filled_pairs(c, nz, nzc, tiles=True)
    return _pair_tails(batch, [(k, B + k, 0) for k in range(B)], pt, pt2, st, False)


def tagged_owned_rows(res4, tiling, i, j):
    """the map rows [x, y, fdr, sigma, tag] of tile pair (i, j)'s four lists that the tile owns (rule 3), tag 1..4"""
    return [row + [tag] for tag, loops in enumerate(res4, start=1) for row in owned_rows(loops, tiling, i, j)]


def row_order(r):
    """rule 5's order of a pair's rows: (tag, x, y)"""
    return (r[4], int(r[0]), int(r[1]))


def tile_pair_bytes(C, n_octaves=2):
    """HBM of one tile pair of C x C in a launch, before the record buffers: two tiles (float64), two masks (bytes) and D_2 of
    the difference image per octave (float64) -- 34 C^2 at two octaves, 136 MB at C = 2000"""
    return (2 * 8 + 2 * 1 + 8 * int(n_octaves)) * int(C) * int(C)


def call_diff_trans_coo(rec1, rec2, octave_values, st, pt, pt2, chunk=TRANS_CHUNK, tiles_per_launch=None, verbose=False,
                        label=""):
    """Differential loops of one chromosome pair from the two samples' records rec = (x, y, v) (x = bins of A, y = bins of B,
    v > 0; host arrays or device tensors, which are not written): rules 2-5 of this module, as a batch of one pair
    (trans_genome.PairBatcher.run_pair).  Returns [[x, y, fdr, sigma, tag], ...] sorted by (tag, x, y)."""
    from .diff_trans_genome import DiffTransGenomeCaller
    caller = DiffTransGenomeCaller(octave_values, st, pt, pt2, None, chunk=chunk, tiles_per_launch=tiles_per_launch,
                                   verbose=verbose)
    return caller.run_pair([rec1, rec2], label)


def regulate(f1, f2, norm_method, res, octave_values, st, pt, pt2, chromosome, chromosome2, verbose=True, balance=None):
    """diff_mustache.regulator()'s body for a trans pair: read both samples (rule 1), call.  Rows [x, y, fdr, sigma, tag].
    Refuses text input and `balance` (TransError, the rules of request.py).  It runs on the current device alone and knows
    nothing of ranks: a multi-rank caller (and -ch2 without -ch) is the command line's to refuse, before it gets here
    (request.plan)."""
    from .request import balance_on_trans, trans_input
    why = trans_input((f1, f2)) or balance_on_trans(balance or None)
    if why:
        raise TransError(why)
    if verbose:
        print("Reading contact map...")
    recs = []
    for f in (f1, f2):
        got = read_trans_contacts(f, norm_method, chromosome, chromosome2, res)
        if got is None:
            print("There is no contact in the chromosome pair %s,%s of %s to work on." % (chromosome, chromosome2, f))
            return []
        if recs and got[3] != recs[0][3]:
            raise ValueError('Both contact maps should have the same resolution.')
        recs.append(got)
    return call_diff_trans_coo(recs[0][:3], recs[1][:3], octave_values, st, pt, pt2, verbose=verbose,
                               label="%s,%s" % (chromosome, chromosome2))
