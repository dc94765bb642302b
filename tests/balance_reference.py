"""NumPy restatement of the ICE balancing of mustache_amd/balance.py (steps 1-7 of its docstring): the authority the device
result is held to.  Plain float64 NumPy; no GPU."""
import numpy as np


def kept_pixels(x, y, v, n, ignore_diags=2):
    """Steps 0-1: valid entries (v > 0, finite, inside [0, n)), repeated pixels resolved last-wins, j - i >= ignore_diags.
    -> (i, j, v) with i <= j, sorted by (i, j)."""
    x, y, v = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(v, np.float64)
    ok = (v > 0) & np.isfinite(v)
    i, j = np.minimum(x, y), np.maximum(x, y)
    ok &= (i >= 0) & (j < n)
    i, j, v = i[ok], j[ok], v[ok]
    key = i * np.int64(n) + j
    order = np.argsort(key, kind="stable")
    last = np.ones(len(key), bool)
    last[:-1] = key[order][1:] != key[order][:-1]
    sel = order[last]
    i, j, v = i[sel], j[sel], v[sel]
    far = (j - i) >= ignore_diags
    return i[far], j[far], v[far]


def _sym(i, j, v):
    off = i != j
    return np.concatenate([i, j[off]]), np.concatenate([j, i[off]]), np.concatenate([v, v[off]])


def marginals(rows, cols, vals, w, n):
    return w * np.bincount(rows, weights=vals * w[cols], minlength=n)


def filter_mask(i, j, v, n, min_nnz=10, mad_max=5.0, details=False):
    """Steps 2-4 -> masked (bool [n]); details=True also returns (m, cut-off)."""
    rows, cols, vals = _sym(i, j, v)
    nnz = np.bincount(rows, minlength=n)
    w = (nnz >= min_nnz).astype(np.float64)
    m = marginals(rows, cols, vals, w, n)
    pos = m > 0
    if not pos.any():
        masked, cut = np.ones(n, bool), np.nan
    else:
        logm = np.log(m[pos])
        med = np.median(logm)
        mad = np.median(np.abs(logm - med))
        cut = np.exp(med - mad_max * mad)
        masked = (m < cut) | (m == 0)
    return (masked, m, cut) if details else masked


def iterate(rows, cols, vals, w, n, tol=1e-5, max_iter=200, trace=None):
    """Step 5 on the symmetric entries -> (w, iterations, variance, converged).  When no s is non-zero, r = 1 everywhere
    (w stays), the variance is 0 and the iteration has converged."""
    var, it, conv = np.nan, 0, False
    for it in range(1, max_iter + 1):
        s = marginals(rows, cols, vals, w, n)
        nz = s != 0
        r = np.ones(n)
        if nz.any():
            mu = s[nz].mean()
            r[nz] = s[nz] / mu
            var = r[nz].var()
        else:
            var = 0.0
        w = w / r
        if trace is not None:
            trace.append(var)
        if var < tol:
            conv = True
            break
    return w, it, var, conv


def ice(x, y, v, n, ignore_diags=2, min_nnz=10, mad_max=5.0, tol=1e-5, max_iter=200, trace=None):
    """-> (bias [n], info) like mustache_amd.balance.ice.  trace: a list that receives the variance of every iteration."""
    i, j, vv = kept_pixels(x, y, v, n, ignore_diags)
    masked = filter_mask(i, j, vv, n, min_nnz, mad_max)
    info = {"masked": masked}
    if masked.all():
        info.update(iterations=0, variance=np.nan, converged=True, kappa=np.nan)
        return np.full(n, np.nan), info
    rows, cols, vals = _sym(i, j, vv)
    w, it, var, conv = iterate(rows, cols, vals, (~masked).astype(np.float64), n, tol, max_iter, trace)
    kappa = np.sqrt(np.sum(vv * w[i] * w[j]) / np.sum(vv))
    bias = np.full(n, np.nan)
    bias[~masked] = kappa / w[~masked]
    info.update(iterations=it, variance=var, converged=conv, kappa=kappa)
    return bias, info


def apply_bias(p1, p2, cnt, bias, res, distance_in_bp):
    """Step 7 for text records (positions in bp): read_pd's arithmetic with the vector in place of a -b file."""
    p1, p2, cnt = (np.asarray(a, np.float64) for a in (p1, p2, cnt))
    keep = np.abs(p1 - p2) <= ((distance_in_bp / res + 1) * res)
    a, b, c = np.floor_divide(p1[keep], res), np.floor_divide(p2[keep], res), cnt[keep]

    def f(k):
        k = int(k)
        if k < 0 or k >= len(bias):
            return 1.0
        val = bias[k]
        return val if (not np.isnan(val) and val >= 0.2) else np.inf
    c = c / np.array([f(k) for k in a]) if len(a) else c
    c = c / np.array([f(k) for k in b]) if len(b) else c
    pos = c > 0
    a, b, c = a[pos].astype(np.int64), b[pos].astype(np.int64), c[pos]
    return np.minimum(a, b), np.maximum(a, b), c


def synth_full_map(n, seed, ignore_gap=False, loops=20, sparse=2000, empty=10, low=10, depth=40.0, band=200):
    """A full intra-chromosomal raw map: power-law decay near the diagonal (up to `band` diagonals), loops, sparse
    long-range pixels, empty bins and low-coverage bins.  -> (x, y, v) integer-valued float64 counts, x <= y, unique."""
    rng = np.random.default_rng(seed)
    cov = rng.uniform(0.5, 1.5, n)
    xs, ys = [], []
    for d in range(0, min(band, n)):
        x = np.arange(n - d)
        lam = depth * (1.0 + d) ** -1.0 * cov[x] * cov[x + d]
        c = rng.poisson(lam)
        k = c > 0
        xs.append(np.stack([x[k], x[k] + d, c[k]], 1))
    for _ in range(loops):
        a = int(rng.integers(0, n - 60)); b = a + int(rng.integers(20, 60))
        xs.append(np.array([[a, b, int(rng.integers(20, 60))]]))
    a = rng.integers(0, n, sparse); b = rng.integers(0, n, sparse)
    xs.append(np.stack([np.minimum(a, b), np.maximum(a, b), rng.integers(1, 4, sparse)], 1))
    m = np.concatenate(xs).astype(np.int64)
    emp = rng.choice(n, empty, replace=False)
    lowb = rng.choice(np.setdiff1d(np.arange(n), emp), low, replace=False)
    drop = np.isin(m[:, 0], emp) | np.isin(m[:, 1], emp)
    # low-coverage bins keep only a few pixels
    lowp = (np.isin(m[:, 0], lowb) | np.isin(m[:, 1], lowb)) & (rng.random(len(m)) > 0.03)
    m = m[~drop & ~lowp]
    key = m[:, 0] * n + m[:, 1]
    _, first = np.unique(key, return_index=True)
    m = m[np.sort(first)]
    return m[:, 0], m[:, 1], m[:, 2].astype(np.float64)


def add_hubs(x, y, v, n, lengths, seed, min_gap=3):
    """Rows longer than one 1024-entry chunk of the device CSR: every pixel touching a hub bin is removed, then hub h gets
    exactly lengths[k] partners, drawn among the non-hub bins at distance >= min_gap (so ignore_diags <= min_gap keeps them
    all), nearer partners more often.  -> (x, y, v, hubs)."""
    rng = np.random.default_rng(seed)
    x, y, v = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(v, np.float64)
    hubs = np.linspace(n // 10, n - n // 10, len(lengths)).astype(np.int64)
    touch = np.isin(x, hubs) | np.isin(y, hubs)
    x, y, v = x[~touch], y[~touch], v[~touch]
    xs, ys, vs = [x], [y], [v]
    other = np.setdiff1d(np.arange(n), hubs)
    for h, L in zip(hubs, lengths):
        cand = other[np.abs(other - h) >= min_gap]
        p = 1.0 / (1.0 + np.abs(cand - h)) ** 0.5
        j = rng.choice(cand, int(L), replace=False, p=p / p.sum())
        xs.append(np.minimum(j, h))
        ys.append(np.maximum(j, h))
        vs.append(rng.integers(1, 30, int(L)).astype(np.float64))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(vs), hubs
