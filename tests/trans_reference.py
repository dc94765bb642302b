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


def synth_trans(n1, n2, density=0.3, nloops=12, seed=0):
    """a rectangular map: log-normal background on a random `density` share of the pixels plus Gaussian blobs.
    Returns (x, y, v) with v > 0, x < n1, y < n2, max(x) = n1 - 1 and max(y) = n2 - 1."""
    rng = np.random.default_rng(seed)
    m = np.where(rng.random((n1, n2)) < density, np.exp(rng.normal(0.0, 0.5, (n1, n2))), 0.0)
    gx, gy = np.mgrid[0:n1, 0:n2]
    for _ in range(nloops):
        cx, cy = rng.integers(8, n1 - 8), rng.integers(8, n2 - 8)
        s = rng.uniform(1.2, 3.0)
        blob = 25.0 * np.exp(-((gx - cx) ** 2 + (gy - cy) ** 2) / (2 * s * s))
        m = np.where(blob > 0.5, m + blob, m)
    m[n1 - 1, n2 - 1] = 1.0
    x, y = np.nonzero(m > 0)
    return x.astype(np.int64), y.astype(np.int64), m[x, y]
