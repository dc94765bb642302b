"""CPU tests of the inter-chromosomal pile-up rules: the NumPy restatement (tests/pileup_trans_reference.py) on tiny maps, the
statuses of `classify` in trans mode, the refusals, and a `--trans` run with the reader and the device call replaced by host
stand-ins.  No GPU."""
import math
import os

import numpy as np
import pytest

import pileup_trans_reference as ptr

HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"


def _tiny(n1=5, n2=4, seed=1):
    """every pixel of a tiny map present, distinct values"""
    rng = np.random.default_rng(seed)
    x, y = (a.reshape(-1) for a in np.mgrid[0:n1, 0:n2])
    return x, y, rng.permutation(n1 * n2).astype(np.float64) + 1.0


def test_nan_frame_at_the_four_map_corners():
    n1, n2, w = 5, 4, 1
    x, y, v = _tiny(n1, n2)
    m = np.zeros((n1, n2))
    m[x, y] = v
    obs, oe = ptr.windows(x, y, v, n1, n2, 2.0, [0, 0, n1 - 1, n1 - 1], [0, n2 - 1, 0, n2 - 1], w)
    nan = np.isnan(obs)
    assert nan[0][0].all() and nan[0][:, 0].all() and not nan[0][1:, 1:].any()         # (0, 0): row -1 and column -1
    assert nan[1][0].all() and nan[1][:, 2].all() and not nan[1][1:, :2].any()         # (0, n2-1): row -1 and column n2
    assert nan[2][2].all() and nan[2][:, 0].all() and not nan[2][:2, 1:].any()         # (n1-1, 0)
    assert nan[3][2].all() and nan[3][:, 2].all() and not nan[3][:2, :2].any()         # (n1-1, n2-1)
    assert np.array_equal(obs[0][1:, 1:], m[0:2, 0:2]) and np.array_equal(obs[3][:2, :2], m[n1 - 2:, n2 - 2:])
    assert np.array_equal(np.isnan(oe), nan) and oe[0][1, 1] == m[0, 0] / 2.0
    # a pixel without a record is 0.0, not NaN; E = 0 makes every oe NaN
    obs, oe = ptr.windows([0, 4], [0, 3], [3.0, 5.0], n1, n2, 0.0, [2], [2], 1)
    assert np.array_equal(obs[0], np.zeros((3, 3))) and np.isnan(oe).all()


def test_repeated_pixels_take_the_largest_value():
    x, y, v = np.array([1, 1, 1, 2]), np.array([2, 2, 2, 0]), np.array([3.0, 7.0, 5.0, 1.0])
    for perm in ([0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 1, 0], [3, 2, 0, 1]):
        obs, _ = ptr.windows(x[perm], y[perm], v[perm], 3, 3, 1.0, [1], [2], 0)
        assert obs[0, 0, 0] == 7.0
    key, val = ptr.pixels(x, y, v, 3)
    assert key.tolist() == [5, 6] and val.tolist() == [7.0, 1.0]


def test_expected_is_fsum_over_valid_rows_times_valid_columns():
    x = np.array([0, 0, 3, 3, 3, 5])
    y = np.array([1, 1, 1, 4, 6, 6])
    v = np.array([1e16, 1.0, 1.0, 0.1, 0.2, 0.3])           # a sum that a left-to-right addition gets wrong
    rows, cols = ptr.valid_bins(x, y, 7, 8)
    assert rows.tolist() == [True, False, False, True, False, True, False]
    assert cols.tolist() == [False, True, False, False, True, False, True, False]
    E = ptr.expected(x, y, v, 7, 8)
    assert E == math.fsum(v.tolist()) / 9 and E != float(np.sum(v)) / 9   # the repeated pixel (0, 1) counts with both records
    assert ptr.expected([], [], [], 7, 8) == 0.0
    r = ptr.pileup_trans_records(x, y, v, 7, 8, [3], [4], 1, 1)
    assert r["expected"] == E and r["center_oe"][0] == 0.1 / E


def test_a_swapped_row_equals_its_swapped_twin():
    res = 1000
    x, y, v = _tiny(30, 20, 4)
    recs = {("chr1", "chr2"): (x, y, v)}
    rows_ab = [("chr1", 5 * res, 6 * res, "chr2", 7 * res, 8 * res), ("chr1", 12 * res, 13 * res, "chr2", 3 * res, 4 * res)]
    rows_mixed = [rows_ab[0], ("chr2", 3 * res, 4 * res, "chr1", 12 * res, 13 * res)]
    a = ptr.pileup_trans(rows_ab, lambda A, B: recs.get((A, B)), res, 2, 1)
    b = ptr.pileup_trans(rows_mixed, lambda A, B: recs.get((A, B)), res, 2, 1)
    assert a[0] == b[0] == ["used", "used"]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3]["sum_obs"], b[3]["sum_obs"])
    assert a[1][1][0] == v[12 * 20 + 3]


# ---- classify in trans mode ----------------------------------------------------------------------------------------------
def _loops(path, rows):
    with open(path, "w") as fh:
        fh.write(HEADER + "\n")
        for r in rows:
            fh.write("\t".join(str(v) for v in r) + "\t0.01\t1.6\n")
    return str(path)


ROWS = [("chr2", 10000, 15000, "chr1", 500000, 505000),     # the pair {1, 2}, oriented (chr2, chr1) by this row
        ("chr1", 0, 5000, "chr1", 500000, 505000),          # cis
        ("1", 20000, 25000, "2", 40000, 45000),             # written (1, 2): swapped
        ("chr3", 5000, 10000, "chr2", 70000, 75000),        # the pair {2, 3} as (chr3, chr2)
        ("chr2", 10000, 15000, "chr1", 500000, 505000),     # the first row again
        ("chr1", 0, 5000, "chr4", 0, 5000)]                 # the pair {1, 4}


def test_classify_in_trans_mode(tmp_path):
    from mustache_amd.pileup import classify, read_loops
    t = read_loops(_loops(tmp_path / "t.tsv", ROWS))
    st, a, b, pairs = classify(t, 5000, trans=True)
    assert st == [None, "cis", None, None, None, None]
    assert pairs == [("chr2", "chr1"), ("chr3", "chr2"), ("chr1", "chr4")]
    assert (a[0], b[0]) == (2, 100) and (a[4], b[4]) == (2, 100)
    assert (a[2], b[2]) == (8, 4)                          # chr2's anchor (bin 8) first: no min / max across chromosomes
    assert (a[3], b[3]) == (1, 14)
    st, a, b, pairs = classify(t, 5000, ["1", "chr2", "3"], trans=True)
    assert st == [None, "cis", None, None, None, "no_pair"]
    assert pairs == [("chr2", "chr1"), ("chr3", "chr2")]
    st, _, _, pairs = classify(t, 5000, ["chr2", "3"], trans=True)
    assert st == ["no_pair", "cis", "no_pair", None, "no_pair", "no_pair"] and pairs == [("chr3", "chr2")]
    ref = ptr.pileup_trans([r for r in ROWS], lambda A, B: None, 5000, chromosomes=["1", "chr2", "3"])
    assert ref[0] == ["no_pair", "cis", "no_pair", "no_pair", "no_pair", "no_pair"]
    assert [p[0] for p in ref[2]] == ["chr2,chr1", "chr3,chr2"]


def test_distance_limits_are_refused_in_trans_mode(tmp_path):
    from mustache_amd.pileup import PileupError, classify, read_loops
    t = read_loops(_loops(tmp_path / "t.tsv", ROWS))
    with pytest.raises(PileupError, match="no distance"):
        classify(t, 5000, n_min=30, trans=True)
    with pytest.raises(PileupError, match="no distance"):
        classify(t, 5000, x_max=400, trans=True)


def test_classify_without_the_switch_is_unchanged(tmp_path):
    from mustache_amd.pileup import classify, read_loops
    t = read_loops(_loops(tmp_path / "t.tsv", ROWS))
    st, x, y, sel = classify(t, 5000, None, 30, None)
    assert st == ["trans", None, "trans", "trans", "trans", "trans"] and sel == ["chr1"]
    assert x.tolist() == [2, 0, 4, 1, 2, 0] and y.tolist() == [100, 100, 8, 14, 100, 0]
    again = classify(t, 5000)                              # the default n is still 30 bins
    assert again[0] == st and again[3] == sel
    assert classify(t, 5000, None, 101)[0][1] == "short"


# ---- the command line ------------------------------------------------------------------------------------------------------
def _refused(capsys, out, needle):
    text = capsys.readouterr().out
    assert "Error:" in text and needle in text, text
    assert not any(os.path.exists(out + s) for s in (".apa.tsv", ".oe.tsv", ".stats.tsv", ".loops.tsv"))


def test_cli_refusals_in_trans_mode(tmp_path, capsys):
    from mustache_amd.pileup import main
    lp = _loops(tmp_path / "t.tsv", ROWS)
    out = str(tmp_path / "o")
    txt, hic, bias = tmp_path / "m.txt", tmp_path / "m.hic", tmp_path / "b.txt"
    for p in (txt, hic, bias):
        p.write_text("0\t0\t1\n")
    main(["-f", str(txt), "-l", lp, "-r", "5000", "-o", out, "--trans"])
    _refused(capsys, out, "only supported for .hic and .cool")
    main(["-f", str(hic), "-l", lp, "-r", "5000", "-o", out, "--trans", "--balance", "ICE"])
    _refused(capsys, out, "--balance does not apply to inter-chromosomal pairs")
    main(["-f", str(hic), "-l", lp, "-r", "5000", "-o", out, "--trans", "-b", str(bias)])
    _refused(capsys, out, "-b does not apply")
    main(["-f", str(hic), "-l", lp, "-r", "5000", "-o", out, "--trans", "-n", "30"])
    _refused(capsys, out, "no distance")
    main(["-f", str(hic), "-l", lp, "-r", "5000", "-o", out, "--trans", "-x", "2Mb"])
    _refused(capsys, out, "no distance")


def test_cli_trans_output_files_with_host_stand_ins(tmp_path, monkeypatch):
    from mustache_amd import pileup as pl
    res, w, q = 5000, 3, 2
    x, y, v = _tiny(40, 120, 7)
    x2, y2, v2 = _tiny(30, 9, 8)
    recs = {("chr2", "chr1"): (x, y, v), ("chr3", "chr2"): (x2, y2, v2)}
    monkeypatch.setattr(pl, "_read_pair", lambda f, norm, A, B, res_, dev: None if (A, B) not in recs else recs[(A, B)] + (res_,))
    monkeypatch.setattr(pl, "pileup_trans_records", ptr.pileup_trans_records)
    lp = _loops(tmp_path / "t.tsv", ROWS)
    hic = tmp_path / "m.hic"
    hic.write_text("stand-in")
    out = str(tmp_path / "o")
    pl.main(["-f", str(hic), "-l", lp, "-r", str(res), "-o", out, "--trans", "-w", str(w), "-q", str(q)])
    status, centre, parts, whole = ptr.pileup_trans(ROWS, lambda A, B: recs.get((A, B)), res, w, q)
    assert status == ["used", "cis", "used", "off_map", "used", "no_pair"]
    body = [r.split("\t") for r in open(out + ".loops.tsv").read().splitlines()[1:]]
    assert [r[8] for r in body] == status
    for k, r in enumerate(body):
        assert np.array_equal([float(r[9]), float(r[10]), float(r[11])], centre[k], equal_nan=True)
    stats = [r.split("\t") for r in open(out + ".stats.tsv").read().splitlines()[1:]]
    assert [r[:3] for r in stats] == [["chr2,chr1", "3", "3"], ["chr3,chr2", "1", "0"], ["chr1,chr4", "1", "0"], ["all", "6", "3"]]
    assert float(stats[0][8]) == parts[0][3]["metrics"]["P2M"] == float(stats[3][8])
    apa = np.array([[float(c) for c in line.split("\t")] for line in open(out + ".apa.tsv").read().splitlines()])
    assert apa.shape == (7, 7) and np.array_equal(apa, whole["apa"], equal_nan=True)
