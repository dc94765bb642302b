"""NumPy restatement of the aggregate peak analysis (APA) of mustache_amd/pileup.py -- the definition the device kernels
(mustache_amd/csrc/mst_pileup.hip) are tested against.  Host arrays only, no GPU.

band: the diagonal-major raw band of one chromosome, band[d, i] = pixel (i, i + d), at least D + 1 rows and n columns.
"""
import numpy as np


def valid_bins(band, n, D):
    """valid[i]: some non-zero pixel (i, j) with |i - j| <= D touches bin i."""
    B = np.asarray(band)
    valid = np.zeros(n, bool)
    for d in range(min(D, n - 1) + 1):
        idx = np.nonzero(B[d, :n - d] != 0)[0]
        valid[idx] = True
        valid[idx + d] = True
    return valid


def expected(band, n, D, valid):
    """E[d] = sum of band[d, i] over i with i + d < n and both ends valid / their count; 0 when the count is 0."""
    B = np.asarray(band)
    E = np.zeros(D + 1)
    for d in range(min(D, n - 1) + 1):
        ok = valid[:n - d] & valid[d:n]
        c = int(ok.sum())
        if c:
            E[d] = B[d, :n - d][ok].sum() / c
    return E


def windows(band, n, D, E, xs, ys, w):
    """obs, oe [L, 2w+1, 2w+1]: cell [a + w, b + w] = pixel (x + a, y + b), mirrored below the diagonal, NaN off the
    chromosome; oe = obs / E[distance], NaN where E is 0."""
    B = np.asarray(band)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    off = np.arange(-w, w + 1)
    I = xs[:, None, None] + off[None, :, None]
    J = ys[:, None, None] + off[None, None, :]
    on = (I >= 0) & (J >= 0) & (I < n) & (J < n)
    lo, dd = np.minimum(I, J), np.abs(J - I)
    on &= dd <= D
    obs = np.full(on.shape, np.nan)
    obs[on] = B[dd[on], lo[on]]
    ex = np.zeros(on.shape)
    ex[on] = E[dd[on]]
    oe = np.full(on.shape, np.nan)
    ok = on & (ex != 0)
    oe[ok] = obs[ok] / ex[ok]
    return obs, oe


def corners(w, q):
    """(row slice, column slice) of the four q x q corners; rows are the a index, columns the b index."""
    near, far = slice(0, q), slice(2 * w - q + 1, 2 * w + 1)
    return {"LL": (far, near), "UL": (near, near), "UR": (near, far), "LR": (far, far)}


def per_loop(obs, oe, w, q):
    """(obs centre, oe centre, P2LL) per loop: P2LL = centre / mean of the loop's own non-NaN LL cells, NaN when there is
    none or the mean is 0."""
    rs, cs = corners(w, q)["LL"]
    ll = obs[:, rs, cs].reshape(len(obs), -1)
    cnt = (~np.isnan(ll)).sum(1)
    s = np.nansum(ll, 1)
    c = obs[:, w, w]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0)
        p2ll = np.where((cnt > 0) & (mean != 0), c / np.where(mean != 0, mean, 1.0), np.nan)
    return c, oe[:, w, w], p2ll


def aggregate(obs, oe, xs, ys):
    """Per cell: (sum obs, count obs, sum oe, count oe) over the loops sorted by (x, y), NaN excluded."""
    order = np.lexsort((np.asarray(ys), np.asarray(xs)))
    o, e = obs[order], oe[order]
    return (np.nansum(o, 0), (~np.isnan(o)).sum(0).astype(np.float64), np.nansum(e, 0),
            (~np.isnan(e)).sum(0).astype(np.float64))


def mean_map(s, c):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, s / np.where(c > 0, c, 1.0), np.nan)


def metrics(M, w, q):
    """P2LL, P2UL, P2UR, P2LR (centre / corner mean), ZscoreLL ((centre - mean LL) / population std LL), P2M (centre / mean of
    every other cell)."""
    M = np.asarray(M, np.float64)
    c = M[w, w]
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, (rs, cs) in corners(w, q).items():
            out["P2" + name] = c / np.mean(M[rs, cs])
        ll = M[corners(w, q)["LL"]]
        out["ZscoreLL"] = (c - np.mean(ll)) / np.std(ll)
        rest = np.delete(M.reshape(-1), w * (2 * w + 1) + w)
        out["P2M"] = c / np.mean(rest) if len(rest) else np.nan
    return out


def pileup_band(band, n, D, xs, ys, w=10, q=6):
    """The whole pile-up of one chromosome, in the layout mustache_amd.pileup.pileup_band returns (host arrays)."""
    if w > 64:
        raise ValueError("window half-width w = %d is above the limit of 64" % w)
    B = np.asarray(band)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    S = 2 * w + 1
    if len(xs) == 0:
        z = np.zeros((S, S))
        M = np.full((S, S), np.nan)
        return {"valid": None, "expected": None, "obs": np.zeros((0, S, S)), "oe": np.zeros((0, S, S)),
                "sum_obs": z, "count_obs": z.copy(), "sum_oe": z.copy(), "count_oe": z.copy(), "apa": M, "apa_oe": M.copy(),
                "center_obs": np.zeros(0), "center_oe": np.zeros(0), "p2ll": np.zeros(0),
                "metrics": metrics(M, w, q), "metrics_oe": metrics(M, w, q)}
    valid = valid_bins(B, n, D)
    E = expected(B, n, D, valid)
    obs, oe = windows(B, n, D, E, xs, ys, w)
    so, co, se, ce = aggregate(obs, oe, xs, ys)
    c_obs, c_oe, p2ll = per_loop(obs, oe, w, q)
    apa, apa_oe = mean_map(so, co), mean_map(se, ce)
    return {"valid": valid, "expected": E, "obs": obs, "oe": oe, "sum_obs": so, "count_obs": co, "sum_oe": se,
            "count_oe": ce, "apa": apa, "apa_oe": apa_oe, "center_obs": c_obs, "center_oe": c_oe, "p2ll": p2ll,
            "metrics": metrics(apa, w, q), "metrics_oe": metrics(apa_oe, w, q)}
