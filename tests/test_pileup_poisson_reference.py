"""The restatement of the pile-up's significance (tests/pileup_poisson_reference.py) against SciPy, its edge rules, the
iteration cap, and what the header, the binding and the Makefile must say about the two new entry points.  No GPU.

Tolerance of the tail: relative 1e-9 against scipy.special.gammainc, the project's standing p-value tolerance.  Measured for this
algorithm with glibc's lgamma, worst relative error against SciPy: 1.4e-13 for c < 100, 1.7e-11 for c < 5 000, 2.7e-10 for
c < 70 000 (it grows like c * 2^-53 through the prefactor), so 1e-9 has a margin of about 50 on the grid below.  Below 1e-290
both values must be below 1e-290, nothing more."""
import math
import os

import numpy as np
import pytest

import pileup_poisson_reference as ref

FACTORS = (0.01, 0.05, 0.2, 0.5, 0.8, 0.95, 0.999, 1, 1.001, 1.05, 1.3, 2, 4)
TINY = 1e-290
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid():
    """[(c, lambda)]: c over 1 .. 39 and 60 seeded draws up to 5 000, lambda = c * f"""
    rng = np.random.default_rng(20)
    cs = list(range(1, 40)) + sorted(int(c) for c in rng.integers(40, 5001, 60))
    return [(c, c * f) for c in cs for f in FACTORS]


def check_tail(got, want, tol=1e-9):
    """the rule both tail tests apply: -> the relative error where the reference is a number >= TINY, 0 below it"""
    if want < TINY:
        assert got < TINY, (got, want)
        return 0.0
    err = abs(got - want) / want
    assert err <= tol, (got, want, err)
    return err


def test_the_tail_against_scipy():
    from scipy.special import gammainc
    worst, deep = 0.0, 0
    for c, lam in grid():
        want = float(gammainc(c, lam))
        got, it = ref.lower_gamma(c, lam)
        assert it < ref.TAIL_MAX_ITER
        worst = max(worst, check_tail(got, want))
        deep += want < TINY
    print("worst relative error against SciPy %.3g over %d cases, %d below 1e-290" % (worst, len(grid()), deep))
    assert deep > 0 and deep < len(grid()) // 2                           # both rules are exercised


def test_both_branches_and_their_border():
    from scipy.special import gammainc
    for a, x in ((1, 1.0), (1, 0.5), (1, 1.0000001), (5, 5.0), (5, math.nextafter(5.0, 6.0)), (3, 0.9), (1, 50.0), (40, 39.999)):
        assert check_tail(ref.lower_gamma(a, x)[0], float(gammainc(a, x))) <= 1e-9
    assert ref.lower_gamma(1, 1.0)[0] == pytest.approx(1.0 - math.exp(-1.0), rel=1e-15)


def test_edge_rules():
    nan, inf = math.nan, math.inf
    assert ref.poisson_tail(0, 3.5) == 1.0 and ref.poisson_tail(0, 0.0) == 1.0          # c = 0
    assert ref.poisson_tail(1, 0.0) == 0.0 and ref.poisson_tail(300, 0.0) == 0.0        # lambda = 0, c >= 1
    assert math.isnan(ref.poisson_tail(0, nan)) and math.isnan(ref.poisson_tail(7, nan))
    assert math.isnan(ref.poisson_tail(7, -1.0)) and ref.poisson_tail(7, inf) == 1.0
    assert ref.poisson_tail(1, 2.0) == pytest.approx(1.0 - math.exp(-2.0), rel=1e-14)
    exp = np.array([[1.0, 2.0, nan, 4.0], [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.0]])
    bias = np.array([1.0, 0.5, nan, 0.19, 0.2, 2.0])
    xs, ys, counts = [0, 0, 1, 4, 0], [1, 2, 3, 5, 5], [3, 3, 3, 0, 2]
    b1, b2, lam, p, p_max = ref.significance(exp, counts, bias, xs, ys)
    assert lam[0].tolist()[:2] == [0.5, 1.0] and math.isnan(lam[0, 2]) and lam[0, 3] == 2.0       # a NaN EXP
    assert math.isnan(p[0, 2]) and math.isnan(p_max[0]) and not math.isnan(p[0, 0])               # P_MAX with one NaN
    assert np.isnan(lam[1]).all() and np.isnan(p[1]).all() and math.isnan(b2[1])                  # a NaN bias
    assert np.isnan(lam[2]).all() and b2[2] == 0.19                                               # a bias < 0.2
    assert (lam[3] == 0.4).all() and (p[3] == 1.0).all() and p_max[3] == 1.0                      # 0.2 itself is usable; c = 0
    assert lam[4, 0] == 0.0 and p[4, 0] == 0.0 and p_max[4] == p[4, 1] > 0                        # lambda = 0 with c >= 1
    q, q_max = ref.q_values(np.array([[0.01, 0.02, 0.03, 0.04], [0.5, nan, 0.5, 0.5]]))
    assert math.isnan(q[1, 1]) and math.isnan(q_max[1]) and q_max[0] == q[0].max() and q[0, 1] == 0.02      # m = 1 in column 1


def test_bh_against_scipy():
    from scipy.stats import false_discovery_control
    rng = np.random.default_rng(5)
    p = rng.uniform(0, 1, 200) ** 3
    p[10:20] = p[10]                                                      # ties
    p[20:25] = 0.0
    p[25:30] = 1.0
    for sample in (p, p[:1], np.array([0.3, 0.3, 0.3]), np.array([1.0])):
        assert np.allclose(ref.bh(sample), false_discovery_control(sample, method="bh"), rtol=1e-15, atol=0.0)
    with_nan = np.concatenate([p[:50], [np.nan, np.nan], p[50:60]])
    got = ref.bh(with_nan)
    assert np.isnan(got[50:52]).all()
    assert np.allclose(np.delete(got, [50, 51]), false_discovery_control(p[:60], method="bh"), rtol=1e-15, atol=0.0)
    assert np.isnan(ref.bh(np.array([np.nan]))).all() and len(ref.bh(np.zeros(0))) == 0


def test_the_cap_is_enough_at_the_largest_exact_float32_count():
    c = 2.0 ** 24
    p, series = ref.lower_gamma(c, c)                                     # the series, at its slowest: x = a
    assert series < ref.TAIL_MAX_ITER // 2 and abs(p - 0.5) < 1e-4
    above = math.nextafter(c, 2 * c)
    p2, fraction = ref.lower_gamma(c, above)                              # the continued fraction, at its slowest: just above a
    assert fraction < ref.TAIL_MAX_ITER // 2 and abs(p2 - 0.5) < 1e-3
    assert math.isnan(ref.lower_gamma(c, c, max_iter=1000)[0])            # under a cap that is too small: NaN, not a wrong number
    assert math.isnan(ref.lower_gamma(c, above, max_iter=100)[0])
    print("c = lambda = 2^24: %d terms of the series; one ulp above: %d steps of the continued fraction" % (series, fraction))
    src = open(os.path.join(ROOT, "mustache_amd", "csrc", "mst_pileup_poisson.hip")).read()
    assert "constexpr int kTailMaxIter = %d;" % ref.TAIL_MAX_ITER in src


def test_centre_counts_of_the_restatement():
    x, d, c = [0, 0, 3, 3, 7], [0, 5, 2, 2, 1], [4.0, 1.0, 2.0, 3.0, 9.0]
    assert ref.centre_counts(x, d, c, [0, 0, 3, 7, 1, 3], [0, 5, 5, 8, 2, 5]).tolist() == [4, 1, 5, 9, 0, 5]
    with pytest.raises(ValueError):
        ref.centre_counts([0], [1], [1.5], [0], [1])


def test_the_entry_points_are_declared_bound_and_built():
    from mustache_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mustache_hip.h")).read()
    assert "MST_STABLE int mst_pileup_centre_counts(" in hdr and "MST_STABLE int mst_pileup_poisson(" in hdr
    assert "#define MST_ABI_REVISION 1" in hdr and _lib.MST_ABI_REVISION == 1
    assert {"mst_pileup_centre_counts", "mst_pileup_poisson"} <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert hasattr(lib, "mst_pileup_centre_counts") and hasattr(lib, "mst_pileup_poisson")
    srcs = [ln for ln in open(os.path.join(ROOT, "mustache_amd", "csrc", "Makefile")) if ln.startswith("SRCS")]
    assert len(srcs) == 1 and "mst_pileup_poisson.hip" in srcs[0].split()


def test_the_columns_and_the_docstring():
    from mustache_amd import pileup as pl
    assert pl.POISSON_COLUMNS == ("STATUS", "RAW_CENTER", "BIAS1", "BIAS2", "LAMBDA_DONUT", "LAMBDA_LL", "LAMBDA_H", "LAMBDA_V",
                                  "P_DONUT", "P_LL", "P_H", "P_V", "P_MAX", "Q_DONUT", "Q_LL", "Q_H", "Q_V", "Q_MAX")
    assert "\nSignificance (" in pl.__doc__ and "NOT HiCCUPS's lambda-chunked" in pl.__doc__
