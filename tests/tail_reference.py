"""Plain NumPy / SciPy restatements of what the tail kernels (mustache_amd/csrc/mst_tail.hip) compute, for the tests that hold
each kernel to them (tests/test_gpu_tail_kernels.py).  No project kernel and no product code is used here: the dense block and
its fills come from the oracle, the window counts are NumPy slices, the p-values are scipy.stats.expon, the components are
scipy.ndimage.label.  tests/test_tail_reference.py holds these restatements to what the project already trusts."""
import numpy as np


def window_counts(nz, pixels, halfs):
    """(cnt1, cnt2) per candidate: np.sum(nz[x-s:x+s+1, y-s:y+s+1]) with s = half and s = 2 * half (mustache.py:803-807).
    The slices are Python's: a negative start wraps to CH + start (empty unless CH < 2s+1), a stop past the edge truncates."""
    CH = nz.shape[0]
    cnt1 = np.empty(len(pixels), np.uint32)
    cnt2 = np.empty(len(pixels), np.uint32)
    for i, (p, s) in enumerate(zip(pixels, halfs)):
        x, y, s = int(p) // CH, int(p) % CH, int(s)
        cnt1[i] = np.sum(nz[x - s:x + s + 1, y - s:y + s + 1])
        cnt2[i] = np.sum(nz[x - 2 * s:x + 2 * s + 1, y - 2 * s:y + 2 * s + 1])
    return cnt1, cnt2


def block_from_coo(x, y, v, start, CH, dpx, n):
    """(c, nz) of the block [start, start + CH) of a chromosome of n bins: the dense block (oracle.dense_block) after the
    prologue (oracle.block_prologue: 2 where off <= 4 or off >= dpx + 1, nz = (c != 0) & (off >= 4) taken before the fills).
    Entries with y - x > dpx + 1 are left out, as in the band, which has no row for them."""
    import oracle
    x, y, v = np.asarray(x), np.asarray(y), np.asarray(v)
    near = y - x <= dpx + 1
    c = oracle.dense_block(x[near], y[near], v[near], start, min(start + CH, n), CH)
    nz = oracle.block_prologue(c, dpx)
    return c, nz


def diagonals(c, ks):
    """Row i = np.diagonal(c, ks[i]) zero-padded to CH; all zeros for k < 0 or k >= CH (mustache.py:816-820 only asks for
    k = y - x >= 0)."""
    CH = c.shape[0]
    out = np.zeros((len(ks), CH))
    for i, k in enumerate(ks):
        k = int(k)
        if 0 <= k < CH:
            d = np.diagonal(c, k)
            out[i, :len(d)] = d
    return out


def expon_fit(min_abs, sum_abs, nz_count):
    """scipy.stats.expon.fit of the |DoG| values of a level: (loc, scale) = (min, mean - min) (mustache.py:755), from the
    level's minimum and sum and the block's tested-pixel count.  nz_count broadcasts against the statistics."""
    mn = np.asarray(min_abs, dtype=np.float64)
    sm = np.asarray(sum_abs, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return mn, sm / np.asarray(nz_count, dtype=np.float64) - mn


def expon_pvalues(value, level, loc, scale):
    """1 - expon.cdf(|value|, loc, scale) with the fit of each record's level (1-based) (mustache.py:756)."""
    from scipy.stats import expon
    k = np.asarray(level).astype(np.int64) - 1
    with np.errstate(all="ignore"):
        return 1 - expon.cdf(np.abs(value), np.asarray(loc)[k], np.asarray(scale)[k])


def cluster_by_label(CH, sel_pix, sel_q, cand_idx):
    """Clustering as the reference does it (mustache.py:830-848), on a painted CH x CH matrix: every candidate and its eight
    neighbours (clipped to the block), scipy.ndimage.label with the 3 x 3 structure, and per label -- in label order -- the
    FIRST arg-min in raster order of o over the component's pixels, o = q at the selected records and >= 1 everywhere else.
    sel_pix (ascending), sel_q: the selected records; cand_idx: which of them are candidates.  Returns the indices into
    sel_pix of the representatives.  (Row 0 never holds a candidate, mustache.py:800, so the clipping never moves a
    component's first pixel in front of another's.)"""
    from scipy.ndimage import label
    if CH > 512:
        raise ValueError("cluster_by_label paints a dense matrix: CH <= 512 only")
    sel_pix = np.asarray(sel_pix).astype(np.int64)
    cand = sel_pix[np.asarray(cand_idx, dtype=np.int64)]
    if len(cand) == 0:
        return []
    x, y = cand // CH, cand % CH
    paint = np.zeros((CH, CH), dtype=bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            xx, yy = x + dx, y + dy
            ok = (xx >= 0) & (xx < CH) & (yy >= 0) & (yy < CH)
            paint[xx[ok], yy[ok]] = True
    lab, ncomp = label(paint, structure=np.ones((3, 3)))
    o = np.full(CH * CH, 1.5)
    o[sel_pix] = sel_q
    flat = np.flatnonzero(lab)                       # the painted pixels in raster order
    labs = lab.ravel()[flat]
    reps = []
    for lb in range(1, ncomp + 1):
        member = flat[labs == lb]                    # raster order within the component
        p = member[np.argmin(o[member])]             # np.argmin: the first minimum
        k = int(np.searchsorted(sel_pix, p))
        if k >= len(sel_pix) or sel_pix[k] != p:
            raise AssertionError("component without a selected record")
        reps.append(k)
    return reps
