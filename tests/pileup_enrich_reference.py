"""NumPy restatement of the enrichment of every loop of a pile-up over its local background ("Enrichment" in
mustache_amd/pileup.py) -- the definition mst_pileup_enrich (mustache_amd/csrc/mst_pileup_enrich.hip) and the host ratios are
tested against.  Plain loops over the cells of a window; host arrays only, no GPU, and nothing of mustache_amd.pileup.

A window is [2w+1, 2w+1]: cell [a + w, b + w] = pixel (x + a, y + b), NaN off the chromosome.  The neighbourhoods come in the
fixed order DONUT, LL, H, V.
"""
import math

import numpy as np

NEIGHBOURHOODS = ("DONUT", "LL", "H", "V")


def member(a, b, w, p):
    """(DONUT, LL, H, V): the neighbourhoods cell (a, b), |a|, |b| <= w, belongs to."""
    outside = abs(a) > p or abs(b) > p                    # of the peak box
    return (outside and a != 0 and b != 0,
            outside and 1 <= a <= w and -w <= b <= -1,
            abs(a) <= 1 and p < abs(b) <= w,
            abs(b) <= 1 and p < abs(a) <= w)


def masks(w, p):
    """bool [4, 2w+1, 2w+1]"""
    if not 0 <= p < w:
        raise ValueError("peak half-width p = %d is outside 0 .. w - 1 = %d" % (p, w - 1))
    out = np.zeros((4, 2 * w + 1, 2 * w + 1), bool)
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            out[:, a + w, b + w] = member(a, b, w, p)
    return out


def _sums(obs, w, p, e_of):
    """sums [L, 4, 3] = S_o, S_e, cnt: cell by cell in row-major order, every loop at once.  e_of(a, b) = the cell's expected
    value per loop (float64 [L]); a cell counts when its obs is not NaN and its e is not 0."""
    obs = np.asarray(obs, np.float64)
    out = np.zeros((len(obs), 4, 3))
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            inside = member(a, b, w, p)
            if not any(inside):
                continue
            o, e = obs[:, a + w, b + w], e_of(a, b)
            counted = ~np.isnan(o) & (e != 0)
            for k in range(4):
                if inside[k]:
                    out[counted, k, 0] += o[counted]
                    out[counted, k, 1] += e[counted]
                    out[counted, k, 2] += 1.0
    return out


def cis_sums(obs, w, p, E, D, xs, ys):
    """cis: e = E[|(y + b) - (x + a)|]; a cell farther than D from the diagonal does not count."""
    E = np.asarray(E, np.float64)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)

    def e_of(a, b):
        d = np.abs((ys + b) - (xs + a))
        return np.where(d <= D, E[np.minimum(d, D)], 0.0)
    return _sums(obs, w, p, e_of)


def trans_sums(obs, w, p, E):
    """trans: e is the pair's scalar E, or one value per loop"""
    e = np.broadcast_to(np.asarray(E, np.float64), (len(obs),))
    return _sums(obs, w, p, lambda a, b: e)


def ratios(sums, centre_obs, centre_e):
    """(EXP [L, 4], FE [L, 4], FE_MIN [L]), one loop and one neighbourhood at a time."""
    sums = np.asarray(sums, np.float64).reshape(-1, 4, 3)
    L = len(sums)
    exp, fe, fe_min = np.full((L, 4), np.nan), np.full((L, 4), np.nan), np.full(L, np.nan)
    for l in range(L):
        c, ec = float(centre_obs[l]), float(centre_e[l])
        for k in range(4):
            so, se, cnt = (float(t) for t in sums[l, k])
            if cnt > 0 and se != 0 and not math.isnan(c):
                exp[l, k] = ec * so / se
            if not math.isnan(exp[l, k]) and exp[l, k] != 0:
                fe[l, k] = c / exp[l, k]
        if not any(math.isnan(t) for t in fe[l]):
            fe_min[l] = min(fe[l])
    return exp, fe, fe_min


def aggregate(apa_oe, w, p):
    """[4]: apa_oe[w, w] / mean of apa_oe over each neighbourhood's non-NaN cells; NaN when there is none or the mean is 0."""
    M = np.asarray(apa_oe, np.float64)
    out = np.full(4, np.nan)
    for k, m in enumerate(masks(w, p)):
        cells = [float(t) for t in M[m] if not math.isnan(t)]
        if cells and math.fsum(cells) != 0:
            out[k] = M[w, w] / (sum(cells) / len(cells))
    return out
