"""Restatement of the significance of every loop of a pile-up ("Significance" in mustache_amd/pileup.py) -- the definition
mst_pileup_centre_counts, mst_pileup_poisson (mustache_amd/csrc/mst_pileup_poisson.hip) and the genome-wide BH are tested
against.  Plain Python, one loop and one neighbourhood at a time; host values only, no GPU, and nothing of mustache_amd.pileup.
The sums S_o, S_e, cnt of the four neighbourhoods (DONUT, LL, H, V) are tests/pileup_enrich_reference.py's.

The tail is the classical split (cephes igam / igamc, Numerical Recipes gser / gcf) in float64, the same operations in the same
order as the kernel; what differs from the device is the library behind log, exp and lgamma.
"""
import math

import numpy as np

TAIL_MAX_ITER = 131072           # kTailMaxIter of mst_pileup_poisson.hip
EPS = 2.0 ** -53
BIG, BIG_INV = 2.0 ** 52, 2.0 ** -52
BIAS_MIN = 0.2                   # balance.py: a bias that is NaN or < 0.2 counts as +inf


def lower_gamma(a, x, max_iter=TAIL_MAX_ITER):
    """(P(a, x), iterations) for a >= 1 and 0 < x < inf: the power series for x <= 1 or x <= a, 1 - Q by the continued fraction
    otherwise, each stopped at a relative term of 2^-53.  (NaN, max_iter) when the iteration has not converged under max_iter."""
    a, x = float(a), float(x)
    pre = math.exp(a * math.log(x) - x - math.lgamma(a))          # x^a e^-x / Gamma(a) < sqrt(a): no overflow
    if x <= 1.0 or x <= a:
        r, c, ans, it = a, 1.0, 1.0, 0
        while True:
            r = r + 1.0
            c = c * (x / r)
            ans = ans + c
            it += 1
            if it >= max_iter:
                return math.nan, it
            if not c / ans > EPS:
                return ans * pre / a, it
    y, z, c = 1.0 - a, x + (1.0 - a) + 1.0, 0.0
    pkm2, qkm2, pkm1, qkm1 = 1.0, x, x + 1.0, z * x
    ans, it = pkm1 / qkm1, 0
    while True:
        c = c + 1.0
        y = y + 1.0
        z = z + 2.0
        yc = y * c
        pk = pkm1 * z - pkm2 * yc
        qk = qkm1 * z - qkm2 * yc
        if qk != 0.0:
            r = pk / qk
            t = abs((ans - r) / r)
            ans = r
        else:
            t = 1.0
        pkm2, pkm1, qkm2, qkm1 = pkm1, pk, qkm1, qk
        if abs(pk) > BIG:
            pkm2, pkm1, qkm2, qkm1 = pkm2 * BIG_INV, pkm1 * BIG_INV, qkm2 * BIG_INV, qkm1 * BIG_INV
        it += 1
        if it >= max_iter:
            return math.nan, it
        if not t > EPS:
            return 1.0 - ans * pre, it


def poisson_tail(c, lam):
    """P(Poisson(lam) >= c) for an integer count c >= 0: NaN when lam is NaN (or negative); else 1 when c = 0; else 0 when
    lam = 0; else 1 when lam = +inf; else P(c, lam)."""
    lam = float(lam)
    if not lam >= 0.0:
        return math.nan
    if int(c) <= 0:
        return 1.0
    if lam == 0.0:
        return 0.0
    if lam == math.inf:
        return 1.0
    return lower_gamma(float(int(c)), lam)[0]


def centre_counts(x, dist, count, xs, ys):
    """the raw count of every loop's centre pixel (xs, ys): a dict of the records, a repeated pixel's counts added; 0 when the set
    has no such pixel.  Python integers -> int64 [L]."""
    have = {}
    for i, d, c in zip(np.asarray(x).tolist(), np.asarray(dist).tolist(), np.asarray(count).tolist()):
        if c != int(c):
            raise ValueError("count %r of pixel (%d, %d) is not an integer" % (c, i, i + d))
        have[(i, d)] = have.get((i, d), 0) + int(c)
    return np.array([have.get((int(a), int(b) - int(a)), 0) for a, b in zip(xs, ys)], np.int64).reshape(-1)


def significance(exp, counts, bias, xs, ys):
    """(bias1 [L], bias2 [L], LAMBDA [L, 4], P [L, 4], P_MAX [L]) from EXP [L, 4] (pileup_enrich_reference.ratios), each loop's
    raw centre count and the bias vector."""
    exp = np.asarray(exp, np.float64).reshape(-1, 4)
    bias = np.asarray(bias, np.float64)
    L = len(exp)
    b1, b2 = np.full(L, np.nan), np.full(L, np.nan)
    lam, p, p_max = np.full((L, 4), np.nan), np.full((L, 4), np.nan), np.full(L, np.nan)
    for l in range(L):
        b1[l], b2[l] = bias[int(xs[l])], bias[int(ys[l])]
        usable = not math.isnan(b1[l]) and b1[l] >= BIAS_MIN and not math.isnan(b2[l]) and b2[l] >= BIAS_MIN
        for k in range(4):
            if usable and not math.isnan(exp[l, k]):
                lam[l, k] = (exp[l, k] * b1[l]) * b2[l]
            p[l, k] = poisson_tail(counts[l], lam[l, k])
        if not any(math.isnan(t) for t in p[l]):
            p_max[l] = max(p[l])
    return b1, b2, lam, p, p_max


def bh(p):
    """Benjamini-Hochberg q-values of the non-NaN entries of p (NaN stays NaN): ascending sort, p * m / rank, the minimum over
    the ranks behind, clipped at 1."""
    p = np.asarray(p, np.float64).reshape(-1)
    q = np.full(len(p), np.nan)
    idx = [i for i in range(len(p)) if not math.isnan(p[i])]
    m = len(idx)
    idx.sort(key=lambda i: p[i])
    running = math.inf
    for rank in range(m, 0, -1):
        i = idx[rank - 1]
        running = min(running, p[i] * m / rank)
        q[i] = min(running, 1.0)
    return q


def q_values(p):
    """(Q [rows, 4], Q_MAX [rows]) of P [rows, 4], the whole run's used loops together: BH per neighbourhood over the non-NaN
    entries; Q_MAX is NaN when one of the four is."""
    p = np.asarray(p, np.float64).reshape(-1, 4)
    q = np.stack([bh(p[:, k]) for k in range(4)], axis=1) if len(p) else np.zeros((0, 4))
    q_max = np.array([math.nan if any(math.isnan(t) for t in row) else max(row) for row in q], np.float64).reshape(-1)
    return q, q_max
