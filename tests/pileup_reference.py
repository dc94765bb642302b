"""NumPy restatement of the aggregate peak analysis (APA) of mustache_amd/pileup.py -- the definition the device kernels
(mustache_amd/csrc/mst_pileup.hip, mst_pileup_reduce.hip) are tested against.  Host arrays only, no GPU.

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


def order_sensitive(rng, shape, nan=0.2):
    """test data on which a different order of additions shows in the bits: normal * 10 ** uniform(-6, 6), a share `nan` of NaN"""
    v = rng.normal(size=shape) * 10.0 ** rng.uniform(-6.0, 6.0, shape)
    v[rng.random(shape) < nan] = np.nan
    return v


def ordered_aggregate(stacks, order, loop_off=None, joint=False):
    """The device reduce (mustache_amd/csrc/mst_pileup_reduce.hip), addition by addition in float64.  stacks: two stacks of
    windows [L, ...]; order: positions -> loop indices; loop_off: the segments' P + 1 offsets into `order` (None: the one segment
    [0, len(order))).  Per segment [l0, l1) its positions of `order` go in chunks of 512, a chunk in four runs of 128; a run
    starts at 0.0 and takes acc = acc + v, in order, for the counted cells of every entry inside [l0, l1) (the others are
    skipped); a count grows by 1.0.  joint=False: rows sum a, count a, sum b, count b, a cell counted where that stack is not
    NaN; joint=True: rows sum a, sum b, count, a cell counted where neither is NaN.  Then t = run0; t = t + run1; ... over the
    four runs, and t = 0.0; t = t + chunk over the chunks in order.  -> [rows, cells] (loop_off None) or [P, rows, cells]; a
    segment without a loop gives zeros."""
    a, b = (np.asarray(s, np.float64).reshape(len(s), -1) for s in stacks)
    order = np.asarray(order, np.int64).reshape(-1)
    off = [0, len(order)] if loop_off is None else [int(o) for o in loop_off]
    rows, one = 3 if joint else 4, np.float64(1.0)
    out = np.zeros((len(off) - 1, rows, a.shape[1]))
    for seg, (l0, l1) in enumerate(zip(off[:-1], off[1:])):
        total = np.zeros((rows, a.shape[1]))
        for k0 in range(l0, l1, 512):
            runs = []
            for r0 in range(k0, k0 + 512, 128):
                run = np.zeros((rows, a.shape[1]))
                for l in order[r0:min(r0 + 128, l1)]:
                    if l < l0 or l >= l1:
                        continue
                    va, vb = a[l], b[l]
                    ma, mb = ~np.isnan(va), ~np.isnan(vb)
                    if joint:
                        m = ma & mb
                        run[0] = np.where(m, run[0] + va, run[0])
                        run[1] = np.where(m, run[1] + vb, run[1])
                        run[2] = np.where(m, run[2] + one, run[2])
                    else:
                        run[0] = np.where(ma, run[0] + va, run[0])
                        run[1] = np.where(ma, run[1] + one, run[1])
                        run[2] = np.where(mb, run[2] + vb, run[2])
                        run[3] = np.where(mb, run[3] + one, run[3])
                runs.append(run)
            t = runs[0]
            for run in runs[1:]:
                t = t + run
            total = total + t
        out[seg] = total
    return out[0] if loop_off is None else out


# the cases the order-exact tests run (tests/test_gpu_pileup*.py on the device, tests/test_pileup_reference.py for the inputs):
# L at the edges of the look-ahead (8), of a wave's 64 order entries, of a run (128) and of a chunk (512); 16 641 cells = 260
# blocks of 64 and one more
REDUCE_SEED = 150                                          # chosen on the CPU: test_pileup_reference.py checks what it is for
REDUCE_L = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)
REDUCE_SINGLE = [(w, L) for w in (0, 1, 10) for L in REDUCE_L] + [(64, L) for L in (1, 129, 513)]
REDUCE_SEGMENTED = [(w, counts) for w in (0, 1, 10) for counts in ((3, 0, 600), (511, 1, 512, 513, 1))] + [(64, (3, 0, 600))]


def reduce_case(w, counts):
    """(stack a, stack b [L, 2w+1, 2w+1], order int32 [L], loop_off int64 [P + 1]) for segments of `counts` loops: order_sensitive
    values, the NaNs of the two stacks drawn independently, a permutation inside every segment.  Planted: with one segment of 8
    loops or more the entries -1 and L; with several, at position 1 a loop of segment 2 (foreign to segment 0)."""
    rng = np.random.default_rng([REDUCE_SEED, w] + list(counts))
    L, S = int(sum(counts)), 2 * w + 1
    loop_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    a, b = order_sensitive(rng, (L, S, S)), order_sensitive(rng, (L, S, S))
    order = np.concatenate([rng.permutation(c) + o for c, o in zip(counts, loop_off)]).astype(np.int32)
    if len(counts) > 1:
        order[1] = loop_off[2] + 2
    elif L >= 8:
        order[2], order[L - 3] = -1, L
    return a, b, order, loop_off


def plain_aggregate(a, b, order, l0, l1, joint):
    """the sums of ordered_aggregate for one segment as np.nansum adds them: the same loops in the same order, one run"""
    a, b = (np.asarray(s, np.float64).reshape(len(s), -1) for s in (a, b))
    sel = [l for l in order[l0:l1] if l0 <= l < l1]
    va, vb = a[sel], b[sel]
    if joint:
        m = np.isnan(va) | np.isnan(vb)
        va, vb = np.where(m, np.nan, va), np.where(m, np.nan, vb)
    return np.nansum(va, 0), np.nansum(vb, 0)


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
