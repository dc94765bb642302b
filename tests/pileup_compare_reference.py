"""NumPy restatement of one loop list piled up on two maps ("Two maps" in mustache_amd/pileup.py) -- the definition
mst_pileup_compare (mustache_amd/csrc/mst_pileup_compare.hip), mst_pileup_reduce_pair (mst_pileup_reduce.hip) and the host ratios are tested
against.  Plain loops over the cells of a window and over the loops; host arrays only, no GPU, and nothing of
mustache_amd.pileup.

A window is [2w+1, 2w+1]: cell [a + w, b + w] = pixel (x + a, y + b), NaN where the sample has no value.  A cell of loop l is
shared when neither oe1[l] nor oe2[l] is NaN there.  The neighbourhoods come in the fixed order DONUT, LL, H, V.
"""
import math

import numpy as np

import pileup_enrich_reference as er
import pileup_reference as pr

NEIGHBOURHOODS = er.NEIGHBOURHOODS


def sums(oe1, oe2, w, p):
    """[L, 4, 3] = S_1, S_2, cnt over the shared cells of each neighbourhood: cell by cell in row-major order, every loop at once."""
    oe1, oe2 = np.asarray(oe1, np.float64), np.asarray(oe2, np.float64)
    out = np.zeros((len(oe1), 4, 3))
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            inside = er.member(a, b, w, p)
            u, v = oe1[:, a + w, b + w], oe2[:, a + w, b + w]
            shared = ~np.isnan(u) & ~np.isnan(v)
            for k in range(4):
                if inside[k]:
                    out[shared, k, 0] += u[shared]
                    out[shared, k, 1] += v[shared]
                    out[shared, k, 2] += 1.0
    return out


def log2_ratio(a, b):
    """log2(a / b), NaN unless both are finite and > 0"""
    a, b = float(a), float(b)
    if not (math.isfinite(a) and math.isfinite(b) and a > 0 and b > 0):
        return math.nan
    r = a / b
    return math.log2(r) if 0 < r < math.inf else (-math.inf if r == 0 else math.inf)


def ratios(s, c1, c2):
    """(R1 [L, 4], R2 [L, 4], LFC_N [L, 4]), one loop and one neighbourhood at a time."""
    s = np.asarray(s, np.float64).reshape(-1, 4, 3)
    L = len(s)
    r = [np.full((L, 4), np.nan), np.full((L, 4), np.nan)]
    lfc = np.full((L, 4), np.nan)
    for l in range(L):
        for k in range(4):
            cnt = float(s[l, k, 2])
            for i, c in enumerate((float(c1[l]), float(c2[l]))):
                if cnt > 0 and not math.isnan(c):
                    bg = float(s[l, k, i]) / cnt
                    if bg != 0:
                        r[i][l, k] = c / bg
            lfc[l, k] = log2_ratio(r[0][l, k], r[1][l, k])
    return r[0], r[1], lfc


def summary(lfc_n):
    """[L]: NaN when any LFC_N is NaN; the smallest when all four are > 0, the largest when all four are < 0, 0.0 otherwise."""
    out = []
    for row in np.asarray(lfc_n, np.float64).reshape(-1, 4):
        row = [float(t) for t in row]
        if any(math.isnan(t) for t in row):
            out.append(math.nan)
        elif all(t > 0 for t in row):
            out.append(min(row))
        elif all(t < 0 for t in row):
            out.append(max(row))
        else:
            out.append(0.0)
    return np.array(out, np.float64).reshape(-1)


def paired(oe1, oe2, xs, ys):
    """(T_1, T_2, C) [2w+1, 2w+1]: the loops sorted by (x, y), chunks of 512 -- four runs of 128 loops each added in order, the
    four added in order -- and the chunks added in chunk order; a loop adds to a cell only where the cell is shared."""
    oe1, oe2 = np.asarray(oe1, np.float64), np.asarray(oe2, np.float64)
    order = np.lexsort((np.asarray(ys), np.asarray(xs)))
    shape = oe1.shape[1:]
    tot = [np.zeros(shape) for _ in range(3)]
    for k0 in range(0, len(order), 512):
        chunk = [np.zeros(shape) for _ in range(3)]
        for r0 in range(k0, min(k0 + 512, len(order)), 128):
            run = [np.zeros(shape) for _ in range(3)]
            for l in order[r0:min(r0 + 128, k0 + 512)]:
                shared = ~np.isnan(oe1[l]) & ~np.isnan(oe2[l])
                run[0][shared] += oe1[l][shared]
                run[1][shared] += oe2[l][shared]
                run[2][shared] += 1.0
            for t, r in zip(chunk, run):
                t += r
        for t, c in zip(tot, chunk):
            t += c
    return tuple(tot)


def diff(T1, T2, C):
    """log2(M_1 / M_2), M_s = T_s / C (NaN where C = 0), NaN unless both are > 0"""
    m1, m2 = pr.mean_map(np.asarray(T1, np.float64), np.asarray(C, np.float64)), pr.mean_map(np.asarray(T2, np.float64),
                                                                                         np.asarray(C, np.float64))
    out = np.full(m1.shape, np.nan)
    for i in np.ndindex(*m1.shape):
        out[i] = log2_ratio(m1[i], m2[i])
    return out


def aggregate(T1, T2, C, w, q, p):
    """{"m1", "m2", "diff", "p2ll_1", "p2ll_2", "lfc_p2ll", "agg_lfc" [4]} of the paired sums."""
    T1, T2, C = (np.asarray(t, np.float64).reshape(2 * w + 1, 2 * w + 1) for t in (T1, T2, C))
    m1, m2 = pr.mean_map(T1, C), pr.mean_map(T2, C)
    p1, p2 = float(pr.metrics(m1, w, q)["P2LL"]), float(pr.metrics(m2, w, q)["P2LL"])
    e1, e2 = er.aggregate(m1, w, p), er.aggregate(m2, w, p)
    return {"m1": m1, "m2": m2, "diff": diff(T1, T2, C), "p2ll_1": p1, "p2ll_2": p2, "lfc_p2ll": log2_ratio(p1, p2),
            "agg_lfc": np.array([log2_ratio(a, b) for a, b in zip(e1, e2)])}


def joint_status(ys, n1, n2):
    """`no_chrom` when a map lacks the chromosome (n is None), `off_map` when y >= min(n1, n2), `used` otherwise"""
    if n1 is None or n2 is None:
        return ["no_chrom" for _ in ys]
    return ["off_map" if y >= min(n1, n2) else "used" for y in ys]
