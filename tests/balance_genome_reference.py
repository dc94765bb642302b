"""NumPy restatement of whole-genome balancing for inter-chromosomal calling (mustache_amd/balance_genome.py states the rule).

Genome: the chromosomes in file order, n_c = length_c // res + 1 bins, off_c = the bins before c, n = sum n_c.
Pixels: `all` = every cis and every trans matrix, `inter` = the trans matrices only.  A cis pixel (i <= j) with j - i < 2 is
dropped; a trans pixel never is, whatever its genome distance; a record with a bin outside its chromosome is dropped.  The
assembled (lo, hi, v) go through steps 2-6 of balance.py with ignore_diags = 0 -- tests/balance_reference.py (ICE) and
tests/newton_reference.py (NEWTON), imported as they are.
Application: v' = (v / b[off_A + x]) / b[off_B + y] in float64, b = +inf for a NaN bias, a bias < 0.2 and a bin outside the
genome; v' > 0 kept.
"""
import numpy as np

import balance_reference as br
import newton_reference as nr

IGNORE_DIAGS = 2


def layout(lengths, res):
    """(bins, offsets, n) of chromosome lengths in bp"""
    bins = [int(length) // int(res) + 1 for length in lengths]
    offsets = [int(o) for o in np.concatenate([[0], np.cumsum(bins)[:-1]])]
    return bins, offsets, int(sum(bins))


def assemble(bins, offsets, cis, trans, pixels="all"):
    """cis: {c: (x, y, v)} with x <= y in bins of chromosome c (index into bins); trans: {(a, b): (x, y, v)} with x = bins of
    a, y = bins of b, a != b in either order.  -> (lo, hi, v) genome coordinates, int64 / int64 / float64."""
    assert pixels in ("all", "inter")
    los, his, vs = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float64)]
    if pixels == "all":
        for c in sorted(cis):
            x, y, v = (np.asarray(a) for a in cis[c])
            x, y = x.astype(np.int64), y.astype(np.int64)
            i, j = np.minimum(x, y), np.maximum(x, y)
            keep = (j - i >= IGNORE_DIAGS) & (i >= 0) & (j < bins[c])
            los.append(offsets[c] + i[keep])
            his.append(offsets[c] + j[keep])
            vs.append(np.asarray(v, np.float64)[keep])
    for a, b in sorted(trans):
        assert a != b
        x, y, v = (np.asarray(t) for t in trans[(a, b)])
        x, y = x.astype(np.int64), y.astype(np.int64)
        keep = (x >= 0) & (x < bins[a]) & (y >= 0) & (y < bins[b])
        ga, gb = offsets[a] + x[keep], offsets[b] + y[keep]
        los.append(np.minimum(ga, gb))
        his.append(np.maximum(ga, gb))
        vs.append(np.asarray(v, np.float64)[keep])
    return np.concatenate(los), np.concatenate(his), np.concatenate(vs)


def balance(method, lo, hi, v, n, **kw):
    """steps 2-6 on the assembled pixels -> (bias [n], info)"""
    f = {"ICE": br.ice, "NEWTON": nr.newton}[method]
    return f(lo, hi, v, n, ignore_diags=0, **kw)


def genome_bias(method, bins, offsets, cis, trans, pixels="all"):
    lo, hi, v = assemble(bins, offsets, cis, trans, pixels)
    return balance(method, lo, hi, v, int(sum(bins)))


def bias_factor(bias, g):
    """b of the application rule at genome bins g"""
    bias = np.asarray(bias, np.float64)
    g = np.asarray(g, np.int64)
    inside = (g >= 0) & (g < len(bias))
    b = np.where(inside, bias[np.where(inside, g, 0)], np.inf) if len(bias) else np.full(len(g), np.inf)
    return np.where(b >= 0.2, b, np.inf)                       # NaN >= 0.2 is False


def apply(bias, off_a, off_b, x, y, v):
    """v' of every record (float64), no record removed; a negative x or y counts as a bin outside the genome"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    bx = np.where(x >= 0, bias_factor(bias, off_a + x), np.inf)
    by = np.where(y >= 0, bias_factor(bias, off_b + y), np.inf)
    with np.errstate(invalid="ignore"):
        return (np.asarray(v, np.float64) / bx) / by


def balanced(bias, off_a, off_b, x, y, v):
    """(x, y, v') with v' > 0 only"""
    vb = apply(bias, off_a, off_b, x, y, v)
    keep = vb > 0
    return np.asarray(x)[keep], np.asarray(y)[keep], vb[keep]


def synth_genome(bins=(70, 50, 40), seed=0, thinned=(7, 83, 131)):
    """The shared case: cis counts Poisson(200 / (1 + d)), trans counts Poisson(1.5), a log-normal true bias, three thinned
    bins (their counts multiplied by 0.02 before the draw).  -> (cis, trans) as assemble takes them, zero counts left out."""
    rng = np.random.default_rng(seed)
    n = int(sum(bins))
    off = np.concatenate([[0], np.cumsum(bins)[:-1]])
    true = np.exp(rng.normal(0.0, 0.3, n))
    true[list(thinned)] *= 0.02
    cis, trans = {}, {}
    for c, nc in enumerate(bins):
        i, j = np.triu_indices(nc)
        lam = 200.0 / (1.0 + (j - i)) * true[off[c] + i] * true[off[c] + j]
        cnt = rng.poisson(lam).astype(np.float64)
        k = cnt > 0
        cis[c] = (i[k], j[k], cnt[k])
    for a in range(len(bins)):
        for b in range(a + 1, len(bins)):
            x, y = (t.ravel() for t in np.meshgrid(np.arange(bins[a]), np.arange(bins[b]), indexing="ij"))
            cnt = rng.poisson(1.5 * true[off[a] + x] * true[off[b] + y]).astype(np.float64)
            k = cnt > 0
            trans[(a, b)] = (x[k], y[k], cnt[k])
    return cis, trans


CALL_BINS = (180, 140, 40)


def synth_call_genome(pair01, seed=7, bins=CALL_BINS):
    """The end-to-end case: `pair01` = (x, y, v), the records of the pair (chromosome 0, chromosome 1) -- the smallest
    loop-returning construction of tests/trans_reference.py is synth_trans(180, 140, density=0.6, nloops=6, seed=41): one tile
    of about 15 000 records -- wrapped as a three-chromosome genome with small cis bands (9 diagonals, Poisson(50 / (1 + d)))
    and Poisson(1.5) counts on the two other pairs.  Values are rounded to float32, as a `.hic` file stores them.
    -> (cis, trans) as assemble takes them."""
    rng = np.random.default_rng(seed)
    cis, trans = {}, {}
    for c, nc in enumerate(bins):
        i, j = np.triu_indices(nc)
        k = (j - i) <= 8
        i, j = i[k], j[k]
        cnt = rng.poisson(50.0 / (1 + (j - i))).astype(np.float64)
        k = cnt > 0
        cis[c] = (i[k], j[k], cnt[k])
    x, y, v = pair01
    trans[(0, 1)] = (np.asarray(x), np.asarray(y), np.asarray(v, np.float32).astype(np.float64))
    for a, b in ((0, 2), (1, 2)):
        x, y = (t.ravel() for t in np.meshgrid(np.arange(bins[a]), np.arange(bins[b]), indexing="ij"))
        cnt = rng.poisson(1.5, len(x)).astype(np.float64)
        k = cnt > 0
        trans[(a, b)] = (x[k], y[k], cnt[k])
    return cis, trans


def hic_arguments(bins, res, cis, trans, extra=()):
    """(chroms, matrices) of hic_trans_writer.write_hic_pairs for a genome of `bins` (chromosome c is named str(c + 1) and is
    bins[c] * res - 1 bp long); extra: names of further chromosomes of one bin that hold no record"""
    chroms = [("All", 1000)] + [(str(c + 1), nc * res - 1) for c, nc in enumerate(bins)] + [(str(e), res - 1) for e in extra]
    mats = {(c + 1, c + 1): {res: cis[c]} for c in cis}
    mats.update({(a + 1, b + 1): {res: trans[(a, b)]} for a, b in trans})
    return chroms, mats
