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


def ordered_neighbourhood_sums(counted, first, second, w, p):
    """The device walk (neighbourhood_sums, mustache_amd/csrc/mst_pileup_sums.h), addition by addition in float64.  counted
    (bool), first, second (float64): [L, 2w+1, 2w+1].  Lane t of 64 adds its cells t, t + 64, ... (row-major) in order into the
    four neighbourhoods' accumulators, where the cell is counted and belongs to the neighbourhood; then the butterfly a = a +
    a[lane ^ o] for o = 32, 16, 8, 4, 2, 1, and lane 0 is the result.  The counts are integers.  -> [L, 4, 3] = sum first, sum
    second, count.  It serves the enrichment (obs and e under "obs not NaN and e not 0") and the comparison of two maps (oe1 and
    oe2 under the joint mask)."""
    L, cells = len(counted), (2 * w + 1) ** 2
    counted = np.asarray(counted, bool).reshape(L, cells)
    first, second = (np.asarray(v, np.float64).reshape(L, cells) for v in (first, second))
    inside = masks(w, p).reshape(4, cells)
    acc = np.zeros((2, L, 4, 64))
    cnt = np.zeros((L, 4), np.int64)
    for c0 in range(0, cells, 64):
        n = min(64, cells - c0)
        take = counted[:, None, c0:c0 + n] & inside[None, :, c0:c0 + n]                # [L, 4, n]
        for s, v in enumerate((first, second)):
            acc[s, :, :, :n] = np.where(take, acc[s, :, :, :n] + v[:, None, c0:c0 + n], acc[s, :, :, :n])
        cnt += take.sum(2)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return np.stack([acc[0, :, :, 0], acc[1, :, :, 0], cnt.astype(np.float64)], axis=2)


# the cases the order-exact tests run: at most 64 cells, 64 .. 128, more than 128, 2w + 1 = 63 and 65 around the walk's carry
# rule, the largest window
NEIGHBOURHOOD_SEED = 0
NEIGHBOURHOOD_CASES = ((1, 0), (3, 1), (4, 1), (5, 2), (10, 2), (31, 5), (32, 5), (64, 2))
NEIGHBOURHOOD_L = (1, 3, 4, 5)


def cis_e(w, E, D, xs, ys):
    """[L, 2w+1, 2w+1]: the expected value of every cell of every window, E[|(y + b) - (x + a)|], 0 beyond D"""
    off = np.arange(-w, w + 1)
    d = np.abs((np.asarray(ys, np.int64)[:, None, None] + off[None, None, :]) - (np.asarray(xs, np.int64)[:, None, None] + off[None, :, None]))
    return np.where(d <= D, np.asarray(E, np.float64)[np.minimum(d, D)], 0.0)


def neighbourhood_case(w, p):
    """five loops on pileup_reference.order_sensitive values: {"a", "b": two stacks [5, 2w+1, 2w+1] with independent NaNs; "xs",
    "ys": loops with y - x in 0 .. 40, the first at 40 (some of its cells lie beyond D) and the second at 0; "E" [D + 1] with a
    zero diagonal, D = 37 + 2w; "e_loop" [5]}"""
    import pileup_reference as pr
    rng = np.random.default_rng([NEIGHBOURHOOD_SEED, w, p])
    L, S, D = 5, 2 * w + 1, 37 + 2 * w
    sep = rng.integers(0, 41, L)
    sep[:2] = 40, 0
    xs = rng.integers(w, 1000, L).astype(np.int64)
    E = np.abs(pr.order_sensitive(rng, D + 1, nan=0.0))
    E[7] = 0.0
    return {"a": pr.order_sensitive(rng, (L, S, S)), "b": pr.order_sensitive(rng, (L, S, S)), "xs": xs, "ys": xs + sep, "E": E,
            "D": D, "e_loop": np.abs(pr.order_sensitive(rng, L, nan=0.0))}


def neighbourhood_inputs(case, w, kind):
    """(counted, first, second) of ordered_neighbourhood_sums for the three device calls on a neighbourhood_case: "cis" and
    "trans" (mst_pileup_enrich on stack a) and "compare" (mst_pileup_compare on the two stacks)"""
    a, b = case["a"], case["b"]
    if kind == "compare":
        return ~np.isnan(a) & ~np.isnan(b), a, b
    e = cis_e(w, case["E"], case["D"], case["xs"], case["ys"]) if kind == "cis" \
        else np.broadcast_to(case["e_loop"][:, None, None], a.shape)
    return ~np.isnan(a) & (e != 0), a, e


def plain_neighbourhood_sums(counted, first, second, w, p):
    """[L, 4, 2]: the two sums of ordered_neighbourhood_sums as a plain masked NumPy sum over the window adds them"""
    take = np.asarray(counted, bool)[:, None] & masks(w, p)[None]
    return np.stack([np.where(take, np.asarray(v, np.float64)[:, None], 0.0).sum((2, 3)) for v in (first, second)], axis=2)


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
