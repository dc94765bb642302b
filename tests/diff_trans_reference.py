"""Test infrastructure: rules 2-5 of mustache_amd/diff_trans.py (two samples, one inter-chromosomal pair) restated in NumPy /
SciPy, and the synthetic sample pairs the CPU and GPU tests share.

Built from tests/trans_reference.py (tiling, ownership, cluster, zscore_exact), oracle.scale_space.scale_space_levels (each
sample's sigma loop on its own tested-pixel mask) and oracle.tail (BH, the sparsity windows).  What is this module's own: the
difference image of rule 4, its D_2 per octave, norm.fit over the doubly tested pixels, the two-sided normal p-value and the
differential subset.
"""
import math

import numpy as np
import scipy.special as sc

import trans_reference as tr
from oracle.scale_space import blur_scipy, level_table, scale_space_levels
from oracle.tail import _window_density, benjamini_hochberg

S = 10                           # the reference's hard-wired levels per octave (s + 2 blurs, s - 1 tested)
BRANCHES = ("off_nz", "found", "tested_not_found")


def two_sided_normal(x, loc, scale):
    """2 min(cdf, 1 - cdf) of N(loc, scale) with the reference's non-finite handling (diff_mustache.py:372-385)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        cdf = sc.ndtr((np.asarray(x, dtype=np.float64) - loc) / scale)
    cdf = np.nan_to_num(cdf, posinf=1, neginf=1, nan=1)
    cdf = np.where(cdf > 0.5, 1 - cdf, cdf)
    return cdf * 2


def _sample(c, nz, st, pt, octave_values):
    """one sample's half of rule 4 on its tile: the full-tile images o (q, 1 off nz, 2 tested and not found), so (sigma), v
    (winning DoG value, 0 tested and not found, 1 off nz), octave (of the winning level, -1 where none) and the candidates that
    survive q < pt, x != 0 and the sparsity windows"""
    ss = scale_space_levels(c, nz, octave_values, s=S)
    pval = ss.pval.copy()
    found = pval != 2
    pval[found] = benjamini_hochberg(pval[found])
    o = np.ones_like(c)
    o[nz] = pval
    so = np.ones_like(c)
    so[nz] = ss.scale
    v = np.ones_like(c)
    v[nz] = ss.best
    octave = np.full(c.shape, -1, np.int64)
    octave[nz] = np.where(ss.level > 0, (ss.level.astype(np.int64) - 1) // (S - 1), -1)
    fnd = np.zeros(c.shape, bool)
    fnd[nz] = found
    x, y = np.nonzero(o < pt)
    keep = x != 0
    for i in range(x.size):
        s = math.ceil(so[x[i], y[i]])
        if _window_density(nz, x[i], y[i], s) < st or _window_density(nz, x[i], y[i], 2 * s) < 0.6:
            keep[i] = False
    return dict(o=o, so=so, v=v, octave=octave, found=fnd, x=x[keep], y=y[keep])


def diff_dog(cd, octave_values):
    """D_2 = G(sigma_2) - G(sigma_3) of the difference image, per octave (SciPy's gaussian_filter, as the reference calls it)"""
    levels = level_table(octave_values, S)
    per_oct = S + 2
    return [blur_scipy(cd, levels[o * per_oct + 1]["sigma"], levels[o * per_oct + 1]["truncate"]) -
            blur_scipy(cd, levels[o * per_oct + 2]["sigma"], levels[o * per_oct + 2]["truncate"])
            for o in range(len(octave_values))]


def tile_pair(c1, c2, st, pt, pt2, octave_values, nz1=None, nz2=None, branches=None):
    """rule 4 on one tile pair (c_s: the tile of sample s's normalised values, 0 = no record): (loops1, diff1, loops2, diff2),
    each [[x, y, q, sigma]] in tile coordinates, in the clustering's label order.  nz1 / nz2: tested-pixel masks other than
    rule 4's c_s != 0 (only the comparison with the cis oracle passes them).  branches: a dict that receives how many
    representatives took each branch of v_other (BRANCHES)."""
    nz1 = c1 != 0 if nz1 is None else nz1
    nz2 = c2 != 0 if nz2 is None else nz2
    empty = ([], [], [], [])
    n1, n2 = int(nz1.sum()), int(nz2.sum())
    if n1 < 50 or n2 < 50 or n1 < 10000 or n2 < 10000:
        return empty
    nzb = nz1 & nz2
    cd = np.zeros(c1.shape)
    cd[nzb] = c1[nzb] - c2[nzb]
    s1 = _sample(c1, nz1, st, pt, octave_values)
    s2 = _sample(c2, nz2, st, pt, octave_values)
    if s1["x"].size == 0 or s2["x"].size == 0:                  # (diff_mustache.py:507)
        return empty
    D = diff_dog(cd, octave_values)
    with np.errstate(invalid="ignore", divide="ignore"):
        fits = []
        for d in D:
            vals = d[nzb]
            loc = float(np.mean(vals)) if vals.size else math.nan             # norm.fit (:371)
            fits.append((loc, float(np.sqrt(np.mean((vals - loc) ** 2))) if vals.size else math.nan))
    out = []
    for me, other, nz_other in ((s1, s2, nz2), (s2, s1, nz1)):
        reps = tr.cluster(me["o"], me["x"], me["y"])
        loops, diff = [], []
        for rx, ry in reps:
            row = [rx, ry, me["o"][rx, ry], me["so"][rx, ry]]
            loops.append(row)
            oc = int(me["octave"][rx, ry])
            pair = float(two_sided_normal(D[oc][rx, ry], *fits[oc]))
            if branches is not None:
                b = "off_nz" if not nz_other[rx, ry] else ("found" if other["found"][rx, ry] else "tested_not_found")
                branches[b] = branches.get(b, 0) + 1
            if pair < pt2 and me["v"][rx, ry] > other["v"][rx, ry]:          # (:567-568)
                diff.append(row)
        out.extend([loops, diff])
    return tuple(out)


def diff_trans_rows_normalized(rec1, rec2, st, pt, pt2, octave_values, chunk=tr.CHUNK, branches=None):
    """rules 3-5 on two samples' normalised records rec = (x, y, vz): rows [x, y, q, sigma, tag] sorted by (tag, x, y)"""
    recs = [(np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(vz, np.float64)) for x, y, vz in (rec1, rec2)]
    n1 = max(int(r[0].max()) for r in recs) + 1
    n2 = max(int(r[1].max()) for r in recs) + 1
    C, (rs, re), (cs, ce) = tr.tiling(n1, n2, chunk)
    out = []
    for i in range(len(rs)):
        for j in range(len(cs)):
            cc = []
            for x, y, vz in recs:
                c = np.zeros((C, C))
                sel = (x >= rs[i]) & (x < rs[i] + C) & (y >= cs[j]) & (y < cs[j] + C)
                c[x[sel] - rs[i], y[sel] - cs[j]] = vz[sel]
                cc.append(c)
            rlo, clo = (re[i - 1] if i else 0), (ce[j - 1] if j else 0)
            for tag, loops in enumerate(tile_pair(cc[0], cc[1], st, pt, pt2, octave_values, branches=branches), start=1):
                for lx, ly, q, sg in loops:
                    gx, gy = lx + rs[i], ly + cs[j]
                    if rlo <= gx < re[i] and clo <= gy < ce[j]:
                        out.append([gx, gy, q, sg, tag])
    out.sort(key=lambda r: (r[4], r[0], r[1]))
    return out


def diff_trans_rows(rec1, rec2, st, pt, pt2, octave_values, chunk=tr.CHUNK, branches=None):
    """rules 2-5 on two samples' records rec = (x, y, v)"""
    norm = []
    for x, y, v in (rec1, rec2):
        z = tr.zscore_exact(v)
        if z is None or z[2] == 0 or not np.isfinite(z[2]):
            return []
        norm.append((x, y, z[0]))
    return diff_trans_rows_normalized(norm[0], norm[1], st, pt, pt2, octave_values, chunk, branches)


def rows_by_tag(rows):
    return {t: [r[:4] for r in rows if r[4] == t] for t in (1, 2, 3, 4)}


# ---- synthetic sample pairs ----------------------------------------------------------------------------------------------
def _stamp(m, spots):
    """tr.synth_trans's blobs: 25 exp(-d^2 / 2 s^2) added where it exceeds 0.5"""
    n1, n2 = m.shape
    for cx, cy, s in spots:
        r = int(math.ceil(s * math.sqrt(2.0 * math.log(50.0)))) + 1
        x0, x1, y0, y1 = max(0, cx - r), min(n1, cx + r + 1), max(0, cy - r), min(n2, cy + r + 1)
        gx, gy = np.mgrid[x0:x1, y0:y1]
        blob = 25.0 * np.exp(-((gx - cx) ** 2 + (gy - cy) ** 2) / (2 * s * s))
        w = m[x0:x1, y0:y1]
        m[x0:x1, y0:y1] = np.where(blob > 0.5, w + blob, w)


def _records(m):
    x, y = np.nonzero(m > 0)
    return x.astype(np.int64), y.astype(np.int64), m[x, y]


def synth_pair(n1, n2, density=0.3, nloops=12, seed=0, blobs=(), redraw=0.25, removed=0.3, added=4, blobs2=()):
    """two samples of one rectangular map.  Sample 1 is tr.synth_trans's map (log-normal background on a `density` share of
    the pixels, `nloops` Gaussian blobs at random places, then `blobs` at given ones).  Sample 2 is sample 1 with the
    background drawn again, independently, on a `redraw` share of the pixels, a `removed` share of the random blobs left out
    and `added` new random blobs (then `blobs2` at given places) put in; the given `blobs` are in both.  Returns
    ((x, y, v) of sample 1, (x, y, v) of sample 2); both hold the corner record (n1 - 1, n2 - 1)."""
    rng = np.random.default_rng(seed)
    bg = np.where(rng.random((n1, n2)) < density, np.exp(rng.normal(0.0, 0.5, (n1, n2))), 0.0)
    spots = [(int(rng.integers(8, n1 - 8)), int(rng.integers(8, n2 - 8)), float(rng.uniform(1.2, 3.0))) for _ in range(nloops)]
    again = rng.random((n1, n2)) < redraw
    bg2 = np.where(again, np.where(rng.random((n1, n2)) < density, np.exp(rng.normal(0.0, 0.5, (n1, n2))), 0.0), bg)
    gone = rng.random(nloops) < removed
    new = [(int(rng.integers(8, n1 - 8)), int(rng.integers(8, n2 - 8)), float(rng.uniform(1.2, 3.0))) for _ in range(added)]
    given = [tuple(b) for b in blobs]
    m1, m2 = bg, bg2
    _stamp(m1, spots + given)
    _stamp(m2, [s for s, g in zip(spots, gone) if not g] + new + given + [tuple(b) for b in blobs2])
    m1[n1 - 1, n2 - 1] = m2[n1 - 1, n2 - 1] = 1.0
    return _records(m1), _records(m2)


# name -> synth_pair arguments, tile size and octaves: the cases the CPU and the GPU tests share
CASES = {
    # 2 x 3 tile pairs of 600, ragged last tiles on both axes
    "tiles_2x3": dict(n1=900, n2=1200, chunk=600, oct=[1.6, 3.2], seed=2, nloops=40, added=12),
    # 6 x 6 tile pairs of 300 that advance by 44 (the overlap of 256 nearly fills a tile), the difference kernel's 14-tile
    "tiles_6x6_sz2": dict(n1=500, n2=520, chunk=300, oct=[2.0, 4.0], seed=5, nloops=30, added=10),
    # the production tile size: 2 x 2 tile pairs of 2000 (rows 0 / 300, columns 0 / 100), loops in what the last tile owns
    "production_2x2": dict(n1=2300, n2=2100, chunk=2000, oct=[1.6, 3.2], seed=4, nloops=60, added=20, density=0.3,
                           blobs=[(2150, 2050, 2.0)], blobs2=[(2250, 2030, 2.5)]),
}
ST, PT, PT2 = 0.88, 0.2, 0.1
_AHEAD = {}
_POOL = None


def case_records(name):
    c = CASES[name]
    kw = {k: v for k, v in c.items() if k not in ("chunk", "oct")}
    return synth_pair(**kw)


def case_job(name):
    """(rows, branch counts) of a shared case on the exactly normalised records (zscore_exact is the device's z-score, bit
    for bit), NumPy / SciPy only"""
    rec1, rec2 = case_records(name)
    branches = {}
    rows = diff_trans_rows(rec1, rec2, ST, PT, PT2, CASES[name]["oct"], chunk=CASES[name]["chunk"], branches=branches)
    return rows, branches


def start_ahead(names, workers=4):
    """run case_job(name) in worker processes, as trans_reference.start_ahead does; case_reference collects the results"""
    global _POOL
    import concurrent.futures as cf
    import multiprocessing as mp
    if _POOL is None:
        _POOL = cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn"))
    for n in names:
        if n not in _AHEAD:
            _AHEAD[n] = _POOL.submit(case_job, n)


def stop_ahead():
    global _POOL
    if _POOL is not None:
        _POOL.shutdown(wait=False, cancel_futures=True)
        _POOL = None
    _AHEAD.clear()


def case_reference(name):
    fut = _AHEAD.get(name)
    if fut is not None:
        try:
            return fut.result()
        except Exception as e:            # a broken pool must not fail a parity test: the restatement runs inline instead
            print("diff_trans_reference: worker failed (%r), running inline" % (e,), flush=True)
            _AHEAD.pop(name, None)
    return case_job(name)


def assert_case_conditions(name, rows):
    """what a shared case must offer before a device result is compared with it: all four lists non-empty, at least 5
    representatives with a coordinate in an overlap strip, at least one owned by a tile that is first on neither axis"""
    c = CASES[name]
    by = rows_by_tag(rows)
    assert all(len(by[t]) > 0 for t in (1, 2, 3, 4)), (name, {t: len(v) for t, v in by.items()})
    reps = {(r[0], r[1]): r[:4] for r in rows if r[4] in (1, 3)}          # the diff lists are subsets
    in_overlap, inner = tr.loop_geometry(list(reps.values()), c["n1"], c["n2"], c["chunk"])
    assert in_overlap >= 5 and inner >= 1, (name, in_overlap, inner)


def assert_branches_covered(all_branches):
    """each of the three v_other branches is taken at least once across the cases"""
    total = {b: sum(d.get(b, 0) for d in all_branches) for b in BRANCHES}
    assert all(total[b] >= 1 for b in BRANCHES), total
