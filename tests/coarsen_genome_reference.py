"""The genome rule of mustache_amd/multires.py restated in NumPy and plain Python, for the tests to compare the package with.

Trans: a record (x, y, c) of the pair (A, B) with the factor k goes to X = x // k, Y = y // k; a record with a negative bin,
X >= n'_A or Y >= n'_B is dropped and counted, BEFORE any key is formed; a coarse pixel's count is the integer sum of c over its
records (Python integers); a pixel whose counts sum to 0 is no pixel.  n'_c = length_c // R + 1.

Cis (`all`): multires_reference.coarsen on (x, dist), then D >= 2 and X + D < n'_c.

Merge: multires_reference.merge per chromosome pair -- loops of different pairs never meet."""
import numpy as np

import multires_reference as mr

IGNORE_DIAGS = 2


def layout(lengths, res):
    return [int(length) // int(res) + 1 for length in lengths]


def coarsen_pair(x, y, c, k, n_a, n_b):
    """one pair's records -> ({(X, Y): count} with counts > 0, records dropped as outside)"""
    out, outside = {}, 0
    for xi, yi, ci in zip(np.asarray(x).tolist(), np.asarray(y).tolist(), np.asarray(c).tolist()):
        xi, yi = int(xi), int(yi)
        if xi < 0 or yi < 0 or xi // k >= n_a or yi // k >= n_b:
            outside += 1
            continue
        cell = (xi // k, yi // k)
        out[cell] = out.get(cell, 0) + int(ci)
    return {cell: v for cell, v in out.items() if v != 0}, outside


def coarsen_pairs(x, y, c, seg_off, n_a, n_b, k):
    """the concatenated records of P pairs -> ({p: {(X, Y): count}} of the pairs with a pixel, records dropped)"""
    out, outside = {}, 0
    for p in range(len(seg_off) - 1):
        s, e = int(seg_off[p]), int(seg_off[p + 1])
        px, o = coarsen_pair(x[s:e], y[s:e], c[s:e], k, int(n_a[p]), int(n_b[p]))
        outside += o
        if px:
            out[p] = px
    return out, outside


def pixels_to_records(px):
    """{(X, Y): count} -> (x, y, v) arrays sorted by (X, Y): int64, int64, float64"""
    cells = sorted(px)
    return (np.array([c[0] for c in cells], np.int64), np.array([c[1] for c in cells], np.int64),
            np.array([px[c] for c in cells], np.float64))


def coarsen_cis(x, y, v, k, n_c, n_fine=None):
    """a chromosome's pixels (x <= y) as read_genome keeps them at r (dist >= 2, inside n_fine bins) -> (X, Y, count) at R"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    keep = (y - x >= IGNORE_DIAGS) & (x >= 0)
    if n_fine is not None:
        keep &= y < n_fine
    X, D, C = mr.coarsen(x[keep], (y - x)[keep], np.asarray(v)[keep], k)
    keep = (D >= IGNORE_DIAGS) & (X + D < n_c)
    return X[keep], (X + D)[keep], C[keep].astype(np.float64)


def coarsen_genome(lengths, res, cis, trans, k):
    """(cis, trans) as balance_genome_reference.assemble takes them, at `res` -> the same at res * k.  Every cis pixel set of
    the result is what enters the assembly (D >= 2); pairs and chromosomes left without a pixel are absent."""
    fine, coarse = layout(lengths, res), layout(lengths, res * k)
    out_cis, out_trans = {}, {}
    for c, (x, y, v) in cis.items():
        X, Y, C = coarsen_cis(x, y, v, k, coarse[c], fine[c])
        if len(X):
            out_cis[c] = (X, Y, C)
    for (a, b), (x, y, v) in trans.items():
        px, _ = coarsen_pair(x, y, v, k, coarse[a], coarse[b])
        if px:
            out_trans[(a, b)] = pixels_to_records(px)
    return out_cis, out_trans


def merge_tsv(texts, resolutions, M=2, pair_order=None):
    """The single-resolution runs' TSV files of trans pairs (as text, ascending resolution) -> (the merged file's text,
    [(pair label "A,B", resolution, kept, called)] for the coarser resolutions in the order their lines are printed).  A
    pair is (BIN1_CHR, BIN2_CHROMOSOME): only rows of one pair are merged with each other.  pair_order: the run's pairs in run
    order (None: order of appearance, the finest file first).  Rows stay the text they are."""
    per, seen = [], []
    for text, r in zip(texts, resolutions):
        lines = text.splitlines(keepends=True)
        assert lines[0] == mr.HEADER
        rows = {}
        for line in lines[1:]:
            f = line.split("\t")
            assert int(f[2]) - int(f[1]) == r and f[0] != f[3]
            rows.setdefault((f[0], f[3]), []).append((int(f[1]) // r, int(f[4]) // r, line))
            if (f[0], f[3]) not in seen:
                seen.append((f[0], f[3]))
        per.append(rows)
    out, counts = [mr.HEADER], []
    for pair in (seen if pair_order is None else pair_order):
        kept = mr.merge([rows.get(pair, []) for rows in per], resolutions, M)
        for j, r in enumerate(resolutions):
            out += [lp[2] for lp in kept[j]]
            if j:
                counts.append(("%s,%s" % pair, r, len(kept[j]), len(per[j].get(pair, []))))
    return "".join(out), counts
