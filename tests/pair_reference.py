"""High-precision restatements of the two-sample path's statistics (reference diff_mustache.py:371-385), shared by the GPU
tests of the pair kernels (tests/test_gpu_pair_kernels.py) and the CPU check of these references themselves
(tests/test_pair_reference.py).  Test infrastructure only.

  pvalue_exact(z)      the reference's pair p-value of one z = (x - loc) / scale, from mpmath at 50 digits with the reference's
                       own roundings restated: for z <= 0, p = erfc(|z| / sqrt 2); for z > 0, cdf = fl(1 - erfc(z / sqrt 2) / 2)
                       (ONE rounding) and p = 2 (1 - cdf), as `cdf > 0.5 -> 1 - cdf` gives it; p = 0 for a non-finite z
                       (nan_to_num(nan=1, posinf=1, neginf=1), then 1 - 1).
  pvalue_tolerance     the allowed absolute error of a computed p against pvalue_exact (the split bounds below).
  exact_normfit(x)     norm.fit(x) = (mean, sqrt(mean((x - mean)^2))) of float64 data in exact integer arithmetic, each rounded
                       once to float64 (the square root adds half an ulp).
"""
import math

import numpy as np

# below this the exact p is under any threshold: SciPy's erfc returns 0 from z ~ -37.68 on while the exact value is still
# ~1e-310, and a libm may return subnormals there
P_TINY = 2.3e-308
# z >= Z_ZERO: 1 - ndtr(-z) rounds to 1 (ndtr(-8.3) = 5.2e-17 < 2^-54), so the reference's p is exactly 0
Z_ZERO = 8.3


def _mp():
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.dps = 50
    return ctx


def pvalue_exact(z):
    """the reference's pair p-value of each z (array in, float64 array out)"""
    mp = _mp()
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    out = np.empty(z.shape)
    r2 = mp.sqrt(2)
    for i, v in enumerate(z.ravel()):
        v = float(v)
        if not math.isfinite(v) or abs(v) > 60.0:                   # (erfc(60 / sqrt 2) ~ 1e-785: 0 in float64)
            out.flat[i] = 0.0
        elif v <= 0:
            out.flat[i] = float(mp.erfc(-mp.mpf(v) / r2))
        else:
            cdf = float(1 - mp.erfc(mp.mpf(v) / r2) / 2)           # the one rounding of ndtr's result
            out.flat[i] = 2.0 * (1.0 - cdf)                          # both steps exact in float64 (cdf in [0.5, 1])
    return out


def pvalue_tolerance(z, p_exact):
    """allowed |p - p*|: z <= -1 relative 4 (1 + z^2) 2^-53 while p* >= P_TINY, absolute P_TINY below; -1 < z < Z_ZERO absolute
    5e-16; z >= Z_ZERO and every non-finite z exact (p* = 0)."""
    z = np.asarray(z, dtype=np.float64)
    p_exact = np.asarray(p_exact, dtype=np.float64)
    tol = np.full(z.shape, 5e-16)
    with np.errstate(invalid="ignore", over="ignore"):
        tail = z <= -1
        rel = 4.0 * (1.0 + z * z) * 2.0 ** -53 * p_exact
        tol = np.where(tail, np.where(p_exact >= P_TINY, rel, P_TINY), tol)
        tol = np.where((z >= Z_ZERO) | ~np.isfinite(z), 0.0, tol)
    return tol


def pvalue_check(z, got, p_exact=None):
    """(indices that break the bounds, worst relative error in the tail z <= -1, p* >= P_TINY, worst absolute error elsewhere)"""
    z = np.asarray(z, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    if p_exact is None:
        p_exact = pvalue_exact(z)
    err = np.abs(got - p_exact)
    bad = np.flatnonzero(~(err <= pvalue_tolerance(z, p_exact)))      # (a NaN p fails)
    with np.errstate(invalid="ignore"):
        tail = (z <= -1) & (p_exact >= P_TINY)
    worst_rel = float(np.max(err[tail] / p_exact[tail], initial=0.0))
    worst_abs = float(np.max(np.where(tail | ~np.isfinite(err), 0.0, err), initial=0.0))
    return bad, worst_rel, worst_abs


def z_grid():
    """the z values the pair p-value is pinned at"""
    one = [1.0]
    for _ in range(4):
        one.append(np.nextafter(one[-1], 2.0))
    below = [1.0]
    for _ in range(4):
        below.append(np.nextafter(below[-1], 0.0))
    near_one = np.array(one + below[1:])
    tiny = np.array([0.0, 5e-324, 1e-300, 1e-17, 1e-9])
    sweep = np.linspace(0.5, Z_ZERO, 780)
    tail = np.linspace(Z_ZERO, 38.6, 400)
    far = np.linspace(Z_ZERO, 40.0, 120)
    z = np.concatenate([tiny, -tiny[1:], near_one, -near_one, sweep, -sweep, -tail, far,
                        [-37.5, -37.68, -37.7, -38.0, -38.5, 1e300, -1e300, np.inf, -np.inf, np.nan]])
    return z


def _ints(x):
    """x (float64, finite) -> integers X and a power of two den with x = X / den exactly"""
    nums, dens = zip(*(float(v).as_integer_ratio() for v in x))
    den = max(dens)                                                   # a power of two; every other divides it
    return [a * (den // d) for a, d in zip(nums, dens)], den


def exact_normfit(x):
    """(loc*, scale*) of norm.fit(x) from exact sums: loc* = fl(sum x / N), scale* = sqrt(fl((N sum x^2 - (sum x)^2) / N^2))"""
    from fractions import Fraction
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size == 0:
        return float("nan"), float("nan")
    X, den = _ints(x)
    N = len(X)
    sx = sum(X)
    sxx = sum(v * v for v in X)
    loc = float(Fraction(sx, N * den))
    var = Fraction(N * sxx - sx * sx, N * N * den * den)
    return loc, math.sqrt(float(var))


def fit_errors(loc, scale, loc_exact, scale_exact):
    """(|loc - loc*| / scale*, |scale - scale*| / scale*)"""
    return abs(loc - loc_exact) / scale_exact, abs(scale - scale_exact) / scale_exact


LOC_BOUND, SCALE_BOUND = 1e-13, 1e-12
