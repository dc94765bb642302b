"""CPU tests of the pile-up (APA) rules: the NumPy restatement (tests/pileup_reference.py) on hand-computed maps, loop-list
parsing and statuses, the command line's refusals, and its four output files with the device calls replaced by the
restatement.  No GPU."""
import math
import os

import numpy as np
import pytest

import pileup_enrich_reference as er
import pileup_reference as pr


def _band(pixels, n, rows):
    """{(i, j): v} -> band [rows, n], band[d, i] = pixel (i, i + d)"""
    B = np.zeros((rows, n))
    for (i, j), v in pixels.items():
        lo, hi = min(i, j), max(i, j)
        B[hi - lo, lo] = v
    return B


def test_expected_with_invalid_bins():
    # bins 0..2 touched, bin 3 touched by nothing, bin 4 only by a pixel beyond D
    B = _band({(0, 0): 1.0, (0, 1): 2.0, (1, 2): 4.0, (1, 4): 9.0}, 5, 4)
    valid = pr.valid_bins(B, 5, 2)
    assert valid.tolist() == [True, True, True, False, False]
    E = pr.expected(B, 5, 2, valid)
    assert E[0] == 1.0 / 3.0                      # (1 + 0 + 0) over bins 0, 1, 2
    assert E[1] == 3.0                            # (2 + 4) over (0, 1), (1, 2)
    assert E[2] == 0.0                            # (0, 2) is valid on both ends and empty
    assert pr.valid_bins(B, 5, 3).tolist() == [True, True, True, False, True]


def test_windows_mirror_off_chromosome_and_oe():
    n, D, w = 6, 5, 2
    rng = np.random.default_rng(3)
    B = np.zeros((D + 1, n))
    for d in range(D + 1):
        B[d, :n - d] = rng.integers(1, 9, n - d)
    E = np.array([2.0, 4.0, 0.0, 8.0, 1.0, 5.0])
    obs, oe = pr.windows(B, n, D, E, [1], [2], w)
    o, e = obs[0], oe[0]
    assert o[w, w] == B[1, 1]                                    # pixel (1, 2)
    assert o[w + 1, w - 1] == B[1, 1]                            # (2, 1) read at its mirror (1, 2)
    assert o[w + 2, w - 2] == B[3, 0]                            # (3, 0) -> (0, 3)
    assert np.isnan(o[0]).all()                                  # row x - 2 = -1 is off the chromosome
    assert not np.isnan(o[1]).any()
    assert o[w - 1, w + 2] == B[4, 0]                            # (0, 4)
    assert e[w, w] == B[1, 1] / 4.0
    assert np.isnan(e[w - 1, w])                                 # pixel (0, 2): distance 2, E[2] = 0
    assert e[w - 1, w + 1] == B[3, 0] / 8.0
    obs, _ = pr.windows(B, n, D, E, [3], [5], 1)
    assert np.isnan(obs[0][:, 2]).all() and not np.isnan(obs[0][:, :2]).any()     # column 6 = n is off the chromosome


def test_metrics_hand_computed():
    M = np.arange(1.0, 26.0).reshape(5, 5)                       # w = 2
    M[2, 2] = 100.0
    m = pr.metrics(M, 2, 2)
    assert m["P2LL"] == 100.0 / np.mean([16.0, 17.0, 21.0, 22.0])
    assert m["P2UL"] == 100.0 / np.mean([1.0, 2.0, 6.0, 7.0])
    assert m["P2UR"] == 100.0 / np.mean([4.0, 5.0, 9.0, 10.0])
    assert m["P2LR"] == 100.0 / np.mean([19.0, 20.0, 24.0, 25.0])
    ll = np.array([16.0, 17.0, 21.0, 22.0])
    assert m["ZscoreLL"] == (100.0 - ll.mean()) / ll.std()
    assert math.isclose(m["P2M"], 100.0 / ((325.0 - 13.0) / 24.0), rel_tol=1e-15)
    from mustache_amd.pileup import metrics
    got = metrics(M, 2, 2)
    for k in m:
        assert math.isclose(got[k], m[k], rel_tol=1e-14), k


def test_aggregate_per_loop_and_order():
    n, D, w, q = 40, 20, 3, 2
    rng = np.random.default_rng(5)
    B = rng.integers(0, 5, (D + 1, n)).astype(np.float64)
    for d in range(D + 1):
        B[d, n - d:] = 0.0
    xs, ys = np.array([0, 10, 30, 12]), np.array([8, 20, 38, 14])
    r = pr.pileup_band(B, n, D, xs, ys, w, q)
    obs = r["obs"]
    assert np.array_equal(r["count_obs"], (~np.isnan(obs)).sum(0))
    assert r["count_obs"][0, 0] == 3 and r["count_obs"][w, w] == 4       # the loop at x = 0 has no row -3
    assert np.allclose(r["sum_obs"], np.nansum(obs, 0), rtol=0, atol=0)
    c, _, p2 = pr.per_loop(obs, r["oe"], w, q)
    ll = obs[1, 2 * w - q + 1:, :q]
    assert p2[1] == c[1] / ll.mean()
    perm = [2, 0, 3, 1]
    again = pr.pileup_band(B, n, D, xs[perm], ys[perm], w, q)
    for k in ("sum_obs", "count_obs", "sum_oe", "count_oe"):
        assert np.array_equal(again[k], r[k])
    empty = pr.pileup_band(B, n, D, [], [], w, q)
    assert empty["count_obs"].sum() == 0 and np.isnan(empty["metrics"]["P2LL"])


# ---- loop lists ----------------------------------------------------------------------------------------------------------
HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"


def _loops(path, rows, header=HEADER, extra=""):
    with open(path, "w") as fh:
        fh.write(header + extra + "\n")
        for r in rows:
            fh.write("\t".join(str(v) for v in r) + "\n")
    return str(path)


def test_midpoint_rule_and_other_resolutions(tmp_path):
    from mustache_amd.pileup import read_loops
    p = _loops(tmp_path / "a.tsv", [("chr1", 5000, 10000, "chr1", 250000, 255000, 0.01, 1.6),
                                    ("1", 2000, 2500, "1", 1000, 1500, 0.2, 3.2, "extra")], extra="\tEXTRA")
    t = read_loops(p)
    assert len(t) == 2 and t.header == HEADER + "\tEXTRA" and t.lines[1].endswith("extra")
    x, y = t.bins(5000)
    assert x.tolist() == [1, 0] and y.tolist() == [50, 0]        # (5000 + 10000) // 2 = 7500 -> bin 1; swapped anchors
    x, y = t.bins(1000)
    assert x.tolist() == [7, 1] and y.tolist() == [252, 2]
    x, y = t.bins(10000)
    assert x.tolist() == [0, 0] and y.tolist() == [25, 0]


def test_statuses_before_the_map(tmp_path):
    from mustache_amd.pileup import classify, read_loops
    rows = [("chr1", 0, 5000, "chr1", 500000, 505000, 0, 1),      # 100 bins: kept
            ("chr1", 0, 5000, "chr2", 500000, 505000, 0, 1),      # trans
            ("1", 0, 5000, "1", 100000, 105000, 0, 1),            # 20 bins: short
            ("chr1", 0, 5000, "chr1", 5000000, 5005000, 0, 1),    # 1000 bins: long under -x 2 Mb
            ("chr3", 0, 5000, "chr3", 500000, 505000, 0, 1),      # cis chromosome, not selected by -ch
            ("2", 0, 5000, "2", 500000, 505000, 0, 1)]
    t = read_loops(_loops(tmp_path / "b.tsv", rows))
    st, x, y, sel = classify(t, 5000, None, 30, 2000000 // 5000)
    assert sel == ["chr1", "chr3", "2"]
    assert st == [None, "trans", "short", "long", None, None]
    st, _, _, sel = classify(t, 5000, ["1", "chr1", "2"], 30, None)
    assert sel == ["1", "2"] and st == [None, "trans", "short", None, "no_chrom", None]


# ---- the command line ----------------------------------------------------------------------------------------------------
@pytest.fixture
def inputs(tmp_path):
    res, n = 5000, 400
    rng = np.random.default_rng(11)
    lines = []
    for i in range(n):
        for d in range(0, 90):
            if i + d < n and rng.random() < 0.7:
                lines.append("%d\t%d\t%d\n" % (i * res, (i + d) * res, rng.integers(1, 50)))
    t = tmp_path / "map.txt"
    t.write_text("".join(lines))
    b = tmp_path / "bias.txt"
    b.write_text("".join("%r\n" % float(v) for v in rng.uniform(0.5, 1.5, n)))
    rows = [("chr1", 50 * res, 51 * res, "chr1", 90 * res, 91 * res, 0.01, 1.6),
            ("chr1", 10 * res, 11 * res, "chr1", 70 * res, 71 * res, 0.02, 1.6),
            ("chr1", 2 * res, 3 * res, "chr1", 40 * res, 41 * res, 0.02, 1.6),      # window reaches past bin 0
            ("chr1", 10 * res, 11 * res, "chr2", 70 * res, 71 * res, 0.02, 1.6),    # trans
            ("chr1", 100 * res, 101 * res, "chr1", 110 * res, 111 * res, 0.1, 3.2),  # short
            ("chr1", 390 * res, 391 * res, "chr1", 450 * res, 451 * res, 0.1, 3.2),  # off the map
            ("chr1", 300 * res, 301 * res, "chr1", 395 * res, 396 * res, 0.1, 3.2)]  # window reaches past bin n - 1
    lp = _loops(tmp_path / "loops.tsv", rows)
    return str(t), str(b), lp, str(tmp_path / "out"), res


def _refused(capsys, out, needle):
    text = capsys.readouterr().out
    assert "Error:" in text and needle in text, text
    assert not any(os.path.exists(out + s) for s in (".apa.tsv", ".oe.tsv", ".stats.tsv", ".loops.tsv"))


def test_cli_refusals(inputs, capsys, monkeypatch):
    from mustache_amd import sharding
    from mustache_amd.pileup import main
    t, b, lp, out, res = inputs
    main(["-f", t, "-l", lp, "-r", str(res), "-o", out, "-b", b, "--balance", "ICE"])
    _refused(capsys, out, "-b")
    main(["-f", t, "-l", lp, "-r", str(res), "-o", out, "-b", b, "-w", "65"])
    _refused(capsys, out, "64")
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))
    main(["-f", t, "-l", lp, "-r", str(res), "-o", out, "-b", b])
    _refused(capsys, out, "one GPU")


def _host_read_band(f, chromosome, res, D, norm=False, bias=False, balance=None, device=None, verbose=False):
    """pileup._read_band on the host: the caller's text reader, then the band in NumPy"""
    from mustache_amd.mustache import read_pd
    x, y, v = read_pd(f, D * res, bias, chromosome, res)
    x, y, v = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(v)
    n = int(max(x.max(), y.max())) + 1
    B = np.zeros((D + 2, n))
    keep = (y - x) <= D + 1
    B[(y - x)[keep], x[keep]] = v[keep]
    return B, n


def _read_matrix(path):
    return np.array([[float(v) for v in line.split("\t")] for line in open(path).read().splitlines()])


def test_cli_output_files(inputs, monkeypatch):
    from mustache_amd import pileup as pl
    t, b, lp, out, res = inputs
    monkeypatch.setattr(pl, "_read_band", _host_read_band)
    monkeypatch.setattr(pl, "pileup_band", pr.pileup_band)
    pl.main(["-f", t, "-l", lp, "-r", str(res), "-o", out, "-b", b, "-ch", "1"])
    # the restatement on the same band
    w, q = 10, 6
    used = [0, 1, 2, 6]
    xs, ys = np.array([50, 10, 2, 300]), np.array([90, 70, 40, 395])
    D = int((ys - xs).max()) + 2 * w
    B, n = _host_read_band(t, "1", res, D, bias=b)
    assert n == 400
    want = pr.pileup_band(B, n, D, xs, ys, w, q)
    apa, oe = _read_matrix(out + ".apa.tsv"), _read_matrix(out + ".oe.tsv")
    assert apa.shape == (21, 21)
    assert np.array_equal(apa, want["apa"]) and np.array_equal(oe, want["apa_oe"])
    stats = open(out + ".stats.tsv").read().splitlines()
    assert stats[0].split("\t") == ["CHR", "ROWS_IN", "LOOPS_USED", "P2LL", "P2UL", "P2UR", "P2LR", "ZscoreLL", "P2M", "OE_P2LL"]
    one, allr = stats[1].split("\t"), stats[2].split("\t")
    assert one[:3] == ["1", "6", "4"] and allr[:3] == ["all", "7", "4"]
    assert float(one[3]) == want["metrics"]["P2LL"] == float(allr[3])
    assert float(one[9]) == want["metrics_oe"]["P2LL"]
    loops = open(out + ".loops.tsv").read().splitlines()
    assert loops[0] == HEADER + "\tSTATUS\tOBS_CENTER\tOE_CENTER\tP2LL"
    body = [r.split("\t") for r in loops[1:]]
    assert [r[8] for r in body] == ["used", "used", "used", "trans", "short", "off_map", "used"]
    assert [r[:8] for r in body] == [r.split("\t") for r in open(lp).read().splitlines()[1:]]
    for j, k in enumerate(used):
        assert float(body[k][9]) == want["center_obs"][j] and float(body[k][11]) == want["p2ll"][j]
    assert all(math.isnan(float(body[k][9])) for k in (3, 4, 5))


# ---- the order-exact restatements: their inputs tell one order of additions from another --------------------------------------
def _bits_differ(a, b):
    return bool((np.ascontiguousarray(a, np.float64).view(np.int64) != np.ascontiguousarray(b, np.float64).view(np.int64)).any())


@pytest.mark.parametrize("w,counts", [(w, (L,)) for w, L in pr.REDUCE_SINGLE if L > 256] + pr.REDUCE_SEGMENTED)
def test_the_reduce_cases_tell_the_device_order_from_nansum(w, counts):
    """Up to 129 loops the four runs of 128 are one sequential sum, which np.nansum over the sorted loops is too; in every
    segment of more than 256 loops each sum row of ordered_aggregate must differ from it in some cell, and the counts never."""
    a, b, order, loop_off = pr.reduce_case(w, counts)
    for joint in (False, True):
        got = pr.ordered_aggregate((a, b), order, loop_off, joint)
        for seg, c in enumerate(counts):
            l0, l1 = int(loop_off[seg]), int(loop_off[seg + 1])
            sa, sb = pr.plain_aggregate(a, b, order, l0, l1, joint)
            ra, rb = (got[seg][0], got[seg][1]) if joint else (got[seg][0], got[seg][2])
            assert np.allclose(ra, sa, rtol=0, atol=1e-4) and np.allclose(rb, sb, rtol=0, atol=1e-4)
            if c > 256:
                assert _bits_differ(ra, sa) and _bits_differ(rb, sb), (seg, joint)
            elif c <= 129:
                assert not _bits_differ(ra, sa) and not _bits_differ(rb, sb), (seg, joint)


@pytest.mark.parametrize("w,p", er.NEIGHBOURHOOD_CASES)
def test_the_neighbourhood_cases_tell_the_lane_order_from_a_plain_sum(w, p):
    case = er.neighbourhood_case(w, p)
    for kind in ("cis", "trans", "compare"):
        counted, first, second = er.neighbourhood_inputs(case, w, kind)
        got = er.ordered_neighbourhood_sums(counted, first, second, w, p)
        plain = er.plain_neighbourhood_sums(counted, first, second, w, p)
        assert np.allclose(got[:, :, :2], plain, rtol=0, atol=1e-4)
        assert np.array_equal(got[:, :, 2], (np.asarray(counted)[:, None] & er.masks(w, p)[None]).sum((2, 3)))
        assert _bits_differ(got[:, :, 0], plain[:, :, 0]) and _bits_differ(got[:, :, 1], plain[:, :, 1]), kind
        assert (got[:, :, 2] > 0).all() or w == 1
