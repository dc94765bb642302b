"""The references of tests/test_gpu_pair_kernels.py checked without a GPU: the mpmath pair p-value against SciPy's own ndtr
(oracle.diff._two_sided_normal, the reference's arithmetic) under the same split bounds the device is held to, and the exact
norm.fit against scipy.stats.norm.fit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_reference as pr      # noqa: E402


def test_exact_pvalue_matches_scipy_within_the_split_bounds():
    from oracle.diff import _two_sided_normal
    z = pr.z_grid()
    exact = pr.pvalue_exact(z)
    with np.errstate(invalid="ignore", divide="ignore"):
        scipy_p = _two_sided_normal(z.copy(), 0.0, 1.0)
    bad, worst_rel, worst_abs = pr.pvalue_check(z, scipy_p, exact)
    assert bad.size == 0, [(z[i], scipy_p[i], exact[i]) for i in bad[:10]]
    assert worst_rel < 1e-12 and worst_abs <= 2.3e-16, (worst_rel, worst_abs)
    # the grid reaches what it is meant to reach: the subnormal tail, the exact zeros on both sides, the erf / erfc switch
    assert ((exact > 0) & (exact < pr.P_TINY)).any() and (exact[z < -38.5] == 0).all()
    assert (exact[(z >= pr.Z_ZERO) | ~np.isfinite(z)] == 0).all() and (exact[(z > 8.0) & (z < pr.Z_ZERO)] > 0).all()
    assert (z == 1.0).sum() == 1 and (np.abs(np.abs(z) - 1.0) < 1e-15).sum() == 18
    # the rounding the reference keeps: p on the positive side is 2 (1 - cdf) with cdf a float64
    pos = (z > 0) & np.isfinite(z)
    assert np.array_equal(exact[pos], 2.0 * (1.0 - (1.0 - exact[pos] / 2.0)))
    # scale 0 and NaN parameters: the reference's p is 0
    with np.errstate(invalid="ignore", divide="ignore"):
        deg = _two_sided_normal(np.array([0.3, 0.5, 0.1, 0.2, 0.2]), np.array([0.3, 0.3, np.nan, 0.0, 0.0]),
                                np.array([0.0, 0.0, 1.0, np.nan, 0.0]))
    assert (deg == 0).all()


def test_exact_normfit_matches_scipy_norm_fit():
    from scipy.stats import norm
    rng = np.random.default_rng(5)
    for n, loc, scale in ((1, 0.0, 1.0), (7, 0.0, 1.0), (5000, 1e-3, 1.0), (20000, 3.0, 0.01), (1234, -2.5e-4, 7e-5)):
        x = rng.normal(loc, scale, n)
        x[::11] *= 1e3 if n > 100 else 1.0        # heavy tails: a DoG of a difference image has them
        ls, ss = norm.fit(x)
        le, se = pr.exact_normfit(x)
        if n == 1:
            assert le == x[0] and se == 0.0 and ss == 0.0
            continue
        el, es = pr.fit_errors(ls, ss, le, se)
        assert el <= pr.LOC_BOUND and es <= pr.SCALE_BOUND, (n, el, es)
    # exact where float sums are not: a sum that cancels to the last bit
    x = np.array([1e16, 1.0, -1e16, 1.0])
    assert pr.exact_normfit(x)[0] == 0.5
    assert all(np.isnan(pr.exact_normfit(np.zeros(0))))
    assert pr.exact_normfit(np.full(9, 0.1)) == (0.1, 0.0)
