"""Test infrastructure: rules 2-6 of mustache_amd/trans.py (inter-chromosomal pairs) restated in NumPy / SciPy.

The sigma loop is oracle.scale_space.scale_space_levels on the trans tested-pixel mask (nz = c != 0, no fills); BH is
oracle.tail.benjamini_hochberg; the sparsity windows are oracle.tail._window_density (the cis arithmetic).  The clustering is
this module's own: oracle.tail.block_tail builds a label matrix of size max(y) + 2 that assumes x < y.
"""
import math

import numpy as np
from scipy.ndimage import label

from oracle.scale_space import scale_space_levels
from oracle.tail import _window_density, benjamini_hochberg

CHUNK = 2000
OVERLAP = 256


def zscore(v):
    """rule 2: (v', mean, std); None for N = 0 (and v' is meaningless when std = 0)"""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return None
    mean = np.mean(v)
    std = np.std(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (v - mean) / std
    z[~np.isfinite(z)] = 0.0
    return z, mean, std


def axis_tiles(n, chunk, overlap=OVERLAP):
    """rule 3 along one axis: the cis start formula with CHUNK = chunk"""
    if n <= chunk:
        return [0], [n]
    start, end = [0], [chunk]
    while end[-1] < n:
        start.append(end[-1] - overlap)
        end.append(start[-1] + chunk)
    end[-1] = n
    start[-1] = max(0, n - chunk)
    return start, end


def tiling(n1, n2, chunk=CHUNK):
    C = min(chunk, max(n1, n2))
    return C, axis_tiles(n1, C), axis_tiles(n2, C)


def ownership_counts(n1, n2, chunk=CHUNK):
    """how many tiles own each map pixel (rule 3: one), and how many hold it inside their window (>= 1)"""
    C, (rs, re), (cs, ce) = tiling(n1, n2, chunk)
    own = np.zeros((n1, n2), np.int32)
    held = np.zeros((n1, n2), np.int32)
    for i in range(len(rs)):
        for j in range(len(cs)):
            own[(re[i - 1] if i else 0):re[i], (ce[j - 1] if j else 0):ce[j]] += 1
            held[rs[i]:rs[i] + C, cs[j]:cs[j] + C] += 1
    return own, held


def cluster(o, cand_x, cand_y):
    """rule 5 on one tile: components of the candidates' 3 x 3 halos (clipped at the tile edges, no wrap-around), the first
    minimum of o in row-major order per component.  Returns [(x, y)] in label order."""
    H, W = o.shape
    mask = np.zeros((H, W), bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            xx, yy = cand_x + dx, cand_y + dy
            ok = (xx >= 0) & (xx < H) & (yy >= 0) & (yy < W)
            mask[xx[ok], yy[ok]] = True
    lab, nf = label(mask, structure=np.ones((3, 3)))
    out = []
    for lb in range(1, nf + 1):
        px = np.argwhere(lab == lb)                      # row-major order
        i = int(np.argmin(o[px[:, 0], px[:, 1]]))
        out.append((int(px[i, 0]), int(px[i, 1])))
    return out


def tile_loops(c, st, pt, octave_values):
    """rule 4 + rule 5 on one tile (c: the tile of normalised values, 0 = no record).  [[x, y, q, sigma]] in tile coordinates."""
    nz = c != 0
    nnz = int(nz.sum())
    if nnz < 50:
        return []
    ss = scale_space_levels(c, nz, octave_values)
    pval = ss.pval.copy()
    found = pval != 2
    if nnz < 10000:
        return []
    pval[found] = benjamini_hochberg(pval[found])
    o = np.ones_like(c)
    o[nz] = pval
    so = np.ones_like(c)
    so[nz] = ss.scale
    x, y = np.nonzero(o < pt)
    keep = x != 0
    for i in range(x.size):
        s = math.ceil(so[x[i], y[i]])
        if _window_density(nz, x[i], y[i], s) < st or _window_density(nz, x[i], y[i], 2 * s) < 0.6:
            keep[i] = False
    x, y = x[keep], y[keep]
    if x.size == 0:
        return []
    return [[rx, ry, o[rx, ry], so[rx, ry]] for rx, ry in cluster(o, x, y)]


def trans_loops_normalized(x, y, vz, st, pt, octave_values, chunk=CHUNK):
    """rules 3-6 on normalised records: [[x, y, q, sigma]] sorted by (x, y)"""
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    n1, n2 = int(x.max()) + 1, int(y.max()) + 1
    C, (rs, re), (cs, ce) = tiling(n1, n2, chunk)
    out = []
    for i in range(len(rs)):
        for j in range(len(cs)):
            c = np.zeros((C, C))
            sel = (x >= rs[i]) & (x < rs[i] + C) & (y >= cs[j]) & (y < cs[j] + C)
            c[x[sel] - rs[i], y[sel] - cs[j]] = vz[sel]
            rlo, clo = (re[i - 1] if i else 0), (ce[j - 1] if j else 0)
            for lx, ly, q, sg in tile_loops(c, st, pt, octave_values):
                gx, gy = lx + rs[i], ly + cs[j]
                if rlo <= gx < re[i] and clo <= gy < ce[j]:
                    out.append([gx, gy, q, sg])
    out.sort(key=lambda r: (r[0], r[1]))
    return out


def trans_loops(x, y, v, st, pt, octave_values, chunk=CHUNK):
    """rules 2-6 on a pair's records"""
    z = zscore(v)
    if z is None or z[2] == 0 or not np.isfinite(z[2]):
        return []
    return trans_loops_normalized(x, y, z[0], st, pt, octave_values, chunk)


def _fsum(a):
    """the exactly rounded sum; a total beyond the largest double rounds to +-inf, as the kernel's conversion does"""
    try:
        return math.fsum(a.tolist())
    except OverflowError:
        with np.errstate(over="ignore"):
            return math.copysign(math.inf, float(np.sum(a)))


def zscore_exact(v):
    """rule 2 to the bit, as mst_trans_zscore computes it: both sums exact and rounded once (math.fsum), the division and the
    square root correctly rounded, (v - mean) ** 2 as d * d in float64.  (v', mean, std); None for N = 0.  The kernel counts
    non-finite addends instead of adding them: a NaN / inf record makes mean and std NaN, a square that overflows makes std
    NaN (both the caller's "no contact" path), and every v' is then 0."""
    v = np.asarray(v, dtype=np.float64)
    n = int(v.size)
    if n == 0:
        return None
    if not np.isfinite(v).all():
        return np.zeros(n), math.nan, math.nan
    mean = _fsum(v) / n
    with np.errstate(over="ignore", invalid="ignore"):
        d = v - mean
        sq = d * d
    if not np.isfinite(sq).all():
        return np.zeros(n), mean, math.nan
    std = math.sqrt(_fsum(sq) / n)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = d / np.float64(std)
    z[~np.isfinite(z)] = 0.0
    return z, mean, std


def overlap_strips(starts, ends):
    """the [lo, hi) ranges of one axis that two or more tile windows hold (window i = [start_i, end_i))"""
    return [(starts[i], ends[i - 1]) for i in range(1, len(starts)) if starts[i] < ends[i - 1]]


def loop_geometry(loops, n1, n2, chunk=CHUNK):
    """(number of loops with a coordinate inside an overlap strip, number owned by a tile that is first on neither axis)"""
    C, (rs, re), (cs, ce) = tiling(n1, n2, chunk)
    sx, sy = overlap_strips(rs, re), overlap_strips(cs, ce)
    in_overlap = sum(1 for a, b, _, _ in loops if any(lo <= a < hi for lo, hi in sx) or any(lo <= b < hi for lo, hi in sy))
    inner = sum(1 for a, b, _, _ in loops if a >= re[0] and b >= ce[0])
    return in_overlap, inner


def synth_trans(n1, n2, density=0.3, nloops=12, seed=0, blobs=()):
    """a rectangular map: log-normal background on a random `density` share of the pixels plus Gaussian blobs (`nloops` at
    random places, then `blobs` = [(cx, cy, s)] at given ones), each evaluated on the window that holds its > 0.5 part.
    Returns (x, y, v) with v > 0, x < n1, y < n2, max(x) = n1 - 1 and max(y) = n2 - 1."""
    rng = np.random.default_rng(seed)
    m = np.where(rng.random((n1, n2)) < density, np.exp(rng.normal(0.0, 0.5, (n1, n2))), 0.0)
    spots = []
    for _ in range(nloops):
        cx, cy = rng.integers(8, n1 - 8), rng.integers(8, n2 - 8)
        spots.append((int(cx), int(cy), rng.uniform(1.2, 3.0)))
    for cx, cy, s in list(spots) + [tuple(b) for b in blobs]:
        r = int(math.ceil(s * math.sqrt(2.0 * math.log(50.0)))) + 1       # 25 exp(-d^2 / 2 s^2) > 0.5 <=> d < 2.797 s
        x0, x1, y0, y1 = max(0, cx - r), min(n1, cx + r + 1), max(0, cy - r), min(n2, cy + r + 1)
        gx, gy = np.mgrid[x0:x1, y0:y1]
        blob = 25.0 * np.exp(-((gx - cx) ** 2 + (gy - cy) ** 2) / (2 * s * s))
        w = m[x0:x1, y0:y1]
        m[x0:x1, y0:y1] = np.where(blob > 0.5, w + blob, w)
    m[n1 - 1, n2 - 1] = 1.0
    x, y = np.nonzero(m > 0)
    return x.astype(np.int64), y.astype(np.int64), m[x, y]


# ---- the production geometry (C = 2000, several tiles): cases shared by the CPU and the GPU tests -------------------------
# name -> synth_trans arguments and octaves.  `blobs` puts loops into the small region the last tile owns.
PRODUCTION_CASES = {
    # 2 x 2 tiles near the 10 000-tested-pixel threshold (10 244 .. 10 908 records per tile), both last overlaps long
    "sparse_2x2": dict(n1=2300, n2=2100, density=0.0015, nloops=40, seed=4, oct=[1.6, 3.2],
                       blobs=[(2150, 2050, 2.0), (2250, 2030, 2.5)]),
    # 2 x 2 tiles, rows 0 / 1700 (a last overlap of 300), columns 0 / 300 (one of 1700); the density of a real trans map
    "short_long_2x2": dict(n1=3700, n2=2300, density=0.05, nloops=60, seed=1, oct=[1.6, 3.2],
                           blobs=[(3000, 2150, 2.0), (3500, 2250, 2.5)]),
    # 3 x 2 tiles, rows 0 / 1744 / 1900, the wide-radius octave list
    "three_rows_oc3": dict(n1=3900, n2=2200, density=0.05, nloops=60, seed=2, oct=[1.6, 3.2, 6.4],
                           blobs=[(3800, 2100, 2.0), (3000, 2100, 2.5)]),
    # dense: 1.2 million records in each full-square tile
    "dense_2x2": dict(n1=2100, n2=2050, density=0.3, nloops=40, seed=3, oct=[1.6, 3.2],
                      blobs=[(2050, 2025, 2.0), (2080, 2010, 2.5)]),
}
_AHEAD = {}
_POOL = None


def production_records(name):
    c = PRODUCTION_CASES[name]
    return synth_trans(c["n1"], c["n2"], density=c["density"], nloops=c["nloops"], seed=c["seed"], blobs=c["blobs"])


def production_job(name, st=0.88, pt=0.2):
    """the restatement's loops of a production case on the exactly normalised records (what the device must reproduce bit for
    bit: zscore_exact), NumPy / SciPy only"""
    x, y, v = production_records(name)
    return trans_loops_normalized(x, y, zscore_exact(v)[0], st, pt, PRODUCTION_CASES[name]["oct"])


def start_ahead(names, workers=4):
    """run production_job(name) in worker processes (as tests/fuzz_cases.py does for the cis oracle); production_reference
    collects the results"""
    global _POOL
    import concurrent.futures as cf
    import multiprocessing as mp
    if _POOL is None:
        _POOL = cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn"))
    for n in names:
        if n not in _AHEAD:
            _AHEAD[n] = _POOL.submit(production_job, n)


def stop_ahead():
    global _POOL
    if _POOL is not None:
        _POOL.shutdown(wait=False, cancel_futures=True)
        _POOL = None
    _AHEAD.clear()


def production_reference(name):
    fut = _AHEAD.get(name)
    if fut is not None:
        try:
            return fut.result()
        except Exception as e:            # a broken pool must not fail a parity test: the restatement runs inline instead
            print("trans_reference: worker failed (%r), running inline" % (e,), flush=True)
            _AHEAD.pop(name, None)
    return production_job(name)


def assert_production_conditions(name, loops):
    """what a production case must offer before a device result is compared with it: loops, at least 5 with a coordinate in an
    overlap strip, at least one owned by a tile that is first on neither axis"""
    c = PRODUCTION_CASES[name]
    in_overlap, inner = loop_geometry(loops, c["n1"], c["n2"])
    assert len(loops) > 0 and in_overlap >= 5 and inner >= 1, (name, len(loops), in_overlap, inner)
