"""tests/tail_reference.py -- the NumPy / SciPy restatements the tail kernels are tested against -- held to what the project
already trusts (the host test double of tests/test_host_logic.py, the oracle pinned to the reference's fixtures, the host
clustering pinned to the reference's loop lists), so they cannot drift.  CPU only."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import tail_reference as tr
from test_host_logic import _FakeBatch

FIXTURES = ["block_320.npz", "block_512.npz"]


def _fixture(golden_dir, name):
    import oracle
    g = np.load(os.path.join(golden_dir, name), allow_pickle=True)
    n, dpx = int(g["n"]), int(g["dpx"])
    c = np.zeros((n, n))
    c[g["x"], g["y"]] = g["v"]
    nz = oracle.block_prologue(c, dpx)
    assert np.array_equal(nz, np.unpackbits(g["loc_nz"]).astype(bool)[:c.size].reshape(c.shape))
    return g, c, nz, n, dpx


@pytest.mark.parametrize("name", FIXTURES)
def test_window_counts_equal_the_host_double(golden_dir, name):
    g, c, nz, n, dpx = _fixture(golden_dir, name)
    found = np.flatnonzero(nz.ravel())[g["loc_pAll"] != 2].astype(np.uint32)
    assert len(found) == len(g["bh_in"])
    fake = _FakeBatch(c, nz, None, None)
    for half in range(1, 8):
        halfs = np.full(len(found), half, np.int64)
        c1, c2 = tr.window_counts(nz, found, halfs)
        e1, e2, _ = fake.candidate_features(0, found, halfs)
        assert np.array_equal(c1, e1) and np.array_equal(c2, e2), half
        assert c1.max() > 0 and c2.max() > c1.max()


@pytest.mark.parametrize("name", FIXTURES)
def test_block_from_coo_equals_the_fixture_block(golden_dir, name):
    g, c, nz, n, dpx = _fixture(golden_dir, name)
    c2, nz2 = tr.block_from_coo(g["x"], g["y"], g["v"], 0, n, dpx, n)
    near = g["y"] - g["x"] <= dpx + 1
    assert near.all(), "the fixtures hold no entry beyond the band"
    assert np.array_equal(c2, c) and np.array_equal(nz2, nz)
    # a block that reaches past the chromosome end: nothing but the fills there
    c3, nz3 = tr.block_from_coo(g["x"], g["y"], g["v"], n - 100, 160, dpx, n)
    assert np.array_equal(c3[:100, :100], c[n - 100:, n - 100:]) and np.array_equal(nz3[:100, :100], nz[n - 100:, n - 100:])
    assert not nz3[100:].any() and not nz3[:, 100:].any() and set(np.unique(c3[:, 100:])) <= {0.0, 2.0}


@pytest.mark.parametrize("name", FIXTURES)
def test_diagonals_equal_the_host_double_and_the_band_rule(golden_dir, name):
    g, c, nz, n, dpx = _fixture(golden_dir, name)
    ks = [-1, 0, 3, 4, 5, dpx - 1, dpx, dpx + 1, dpx + 2, n - 2, n - 1, n, n + 5]
    got = tr.diagonals(c, ks)
    inside = [k for k in ks if 0 <= k < n]
    assert np.array_equal(got[[ks.index(k) for k in inside]], _FakeBatch(c, nz, None, None).diagonals(0, inside))
    assert not got[[ks.index(k) for k in ks if k not in inside]].any()
    # what a diagonal of the filled block is in terms of the band (used where a dense block would be too large to build):
    # the constant 2 for k <= 4 and k >= dpx + 1, the raw values in between
    raw = np.zeros((n, n))
    raw[g["x"], g["y"]] = g["v"]
    for i, k in enumerate(ks):
        if 0 <= k < n:
            exp = np.full(n - k, 2.0) if (k <= 4 or k >= dpx + 1) else np.diagonal(raw, k)
            assert np.array_equal(got[i, :n - k], exp) and not got[i, n - k:].any()


@pytest.mark.parametrize("name", FIXTURES)
def test_expon_pvalues_equal_the_oracle_bitwise(golden_dir, name):
    from oracle.scale_space import expon_pvalue
    g = np.load(os.path.join(golden_dir, name), allow_pickle=True)
    found = g["loc_pAll"] != 2
    value = g["loc_vAll"][found]
    import oracle
    lv = oracle.level_table([1.6, 3.2], 10)                                  # 12 levels per octave, levels 3..11 are tested
    sigma = np.array([lv[o * 12 + i - 1]["sigma"] for o in range(2) for i in range(3, 12)])
    level = np.searchsorted(sigma, g["loc_Scales"][found]) + 1
    assert np.array_equal(sigma[level - 1], g["loc_Scales"][found]) and len(np.unique(level)) > 10
    loc, scale = g["fit"][:, 0], g["fit"][:, 1]
    p = tr.expon_pvalues(value, level, loc, scale)
    assert np.array_equal(p, expon_pvalue(np.abs(value), loc[level - 1], scale[level - 1]))
    assert np.array_equal(p, g["bh_in"]), "and both are the reference's own p-values"
    # the same through negated values, and outside the support / with a degenerate fit
    assert np.array_equal(tr.expon_pvalues(-value, level, loc, scale), p)
    one = tr.expon_pvalues(np.array([loc[0], loc[0] / 2]), np.array([1, 1]), loc, scale)
    assert np.array_equal(one, [1.0, 1.0])
    assert np.isnan(tr.expon_pvalues(np.array([1.0, 1.0]), np.array([1, 2]), np.array([0.5, 0.5]), np.array([0.0, -1.0]))).all()


def test_expon_fit_is_min_and_mean_minus_min():
    rng = np.random.default_rng(3)
    a = np.abs(rng.normal(size=(7, 1000))) + 0.01
    loc, scale = tr.expon_fit(a.min(axis=1), a.sum(axis=1), 1000)
    assert np.array_equal(loc, a.min(axis=1)) and np.array_equal(scale, a.sum(axis=1) / 1000.0 - a.min(axis=1))
    from scipy.stats import expon
    for row, lo, sc in zip(a, loc, scale):
        np.testing.assert_allclose(expon.fit(row), (lo, sc), rtol=1e-12)


def _by_label(CH, rec, q, cand, pt=0.1):
    """record indices of the representatives through cluster_by_label"""
    sel = np.nonzero(q < pt)[0]
    reps = tr.cluster_by_label(CH, rec["pixel"][sel], q[sel], np.searchsorted(sel, cand))
    return [int(sel[k]) for k in reps]


def test_cluster_by_label_equals_the_host_clustering():
    from mustache_amd.tail import cluster_representatives
    from test_gpu_cluster import _case
    CH = 100

    def rec_of(pixels, qs):
        o = np.argsort(pixels)
        return {"pixel": np.asarray(pixels, np.uint32)[o], "level": np.ones(len(pixels), np.uint32), "q": np.asarray(qs, float)[o]}
    P = lambda x, y: x * CH + y
    crafted = [                                        # the blocks of test_device_clustering_crafted_cases
        (rec_of([P(10, 20), P(10, 23), P(10, 27), P(50, 60)], [0.05, 0.04, 0.03, 0.02]), [0, 1, 2, 3], [1, 2, 3]),
        (rec_of([P(30, 40), P(31, 41)], [0.05, 0.01]), [0], [1]),
        (rec_of([P(5, 9)], [0.05]), [], []),
        (rec_of([P(70, 80), P(70, 81), P(71, 80)], [0.02, 0.02, 0.02]), [1, 2], [0]),
        (rec_of([P(1, 5), P(98, 99), P(99, 99)], [0.03, 0.02, 0.01]), [0, 1], [0, 2]),
    ]
    for rec, cand, exp in crafted:
        cand = np.asarray(cand, dtype=np.int64)
        assert _by_label(CH, rec, rec["q"], cand) == exp
        if len(cand):
            assert cluster_representatives(SimpleNamespace(CH=CH, found=[rec]), 0, rec["q"], cand) == exp
    rng = np.random.default_rng(11)
    total = multi = 0
    for i in range(20):
        n_sel, spread, frac, quantum = ((150, 3, 0.5, 0.0), (400, 5, 0.3, 0.01), (60, 1, 1.0, 0.0), (600, 8, 0.8, 0.02))[i % 4]
        rec, q, cand = _case(rng, 200, n_sel, spread, frac, quantum)
        exp = cluster_representatives(SimpleNamespace(CH=200, found=[rec]), 0, q, cand)
        assert _by_label(200, rec, q, cand) == exp, i
        total += len(exp)
        multi += len(cand) - len(exp)
    assert total > 200 and multi > 200, "many components, and many of them with several candidates"
