"""The two rules of mustache_amd/multires.py restated in NumPy and plain Python, for the tests to compare the package with.

Coarsening: a record (x, d, c) with the factor k goes to X = x // k, Y = (x + d) // k; a coarse pixel's count is the integer
sum of c over its records (np.unique on X * n' + Y, sums in Python integers); a pixel whose counts sum to 0 is no pixel.

Merge: the accepted set starts as the finest list; a loop of a coarser list at bins (X, Y) of resolution r_i is dropped when
some accepted loop at bins (x, y) of resolution r_a has |2 x r_a + r_a - 2 X r_i - r_i| <= 2 M r_i and the same with y and Y;
the survivors of a list join the accepted set after the whole list has been judged.  The literal double loop."""
import numpy as np


def coarsen(x, d, c, k):
    """records -> (X, D, count) of the coarse pixels sorted by (X, Y): int64 arrays, counts summed as Python integers"""
    x, d = np.asarray(x, np.int64), np.asarray(d, np.int64)
    c = [int(v) for v in np.asarray(c).tolist()]
    if len(x) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    X, Y = x // k, (x + d) // k
    n = int(Y.max()) + 1
    keys, inverse = np.unique(X * n + Y, return_inverse=True)
    sums = [0] * len(keys)
    for j, v in zip(inverse.tolist(), c):
        sums[j] += v
    sums = np.array(sums, dtype=object)
    keep = np.array([s != 0 for s in sums], dtype=bool)
    keys = keys[keep]
    return keys // n, keys % n - keys // n, np.array([int(s) for s in sums[keep]], dtype=np.int64)


def triples(x, d, c):
    """(x, dist, count) arrays -> the sorted list of triples of Python integers"""
    return sorted(zip(np.asarray(x).tolist(), np.asarray(d).tolist(), np.asarray(c).tolist()))


def merge(lists, resolutions, M=2):
    """-> the kept rows of each list, in input order"""
    accepted = [(int(lp[0]), int(lp[1]), int(resolutions[0])) for lp in lists[0]]
    kept = [list(lists[0])]
    for loops, r in zip(lists[1:], resolutions[1:]):
        r = int(r)
        stay = []
        for lp in loops:
            X, Y = int(lp[0]), int(lp[1])
            near = False
            for x, y, ra in accepted:
                if abs(2 * x * ra + ra - 2 * X * r - r) <= 2 * M * r and abs(2 * y * ra + ra - 2 * Y * r - r) <= 2 * M * r:
                    near = True
                    break
            if not near:
                stay.append(lp)
        kept.append(stay)
        accepted += [(int(lp[0]), int(lp[1]), r) for lp in stay]
    return kept


HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE\n"


def merge_tsv(texts, resolutions, M=2):
    """The single-resolution runs' TSV files (as text, ascending resolution, each of ONE chromosome or of the same chromosomes
    in the same order) -> (the merged file's text, [(chromosome, resolution, kept, called)] for the coarser resolutions in
    the order their lines are printed).  Rows stay the text they are."""
    per = []                                 # per resolution: {chromosome: [(x, y, line)]}, chromosomes in order of appearance
    order = []
    for text, r in zip(texts, resolutions):
        lines = text.splitlines(keepends=True)
        assert lines[0] == HEADER
        rows = {}
        for line in lines[1:]:
            f = line.split("\t")
            assert int(f[2]) - int(f[1]) == r and f[0] == f[3]
            rows.setdefault(f[0], []).append((int(f[1]) // r, int(f[4]) // r, line))
            if f[0] not in order:
                order.append(f[0])
        per.append(rows)
    out, counts = [HEADER], []
    for c in order:
        kept = merge([rows.get(c, []) for rows in per], resolutions, M)
        for j, r in enumerate(resolutions):
            out += [lp[2] for lp in kept[j]]
            if j:
                counts.append((c, r, len(kept[j]), len(per[j].get(c, []))))
    return "".join(out), counts
