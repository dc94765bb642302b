"""The rules of the pile-up on two maps ("Two maps" in mustache_amd/pileup.py) on the host: a case worked by hand, the joint NaN
mask, the ratios and the summary at every NaN rule, pileup.py's NumPy functions against the cell-by-cell restatement
(tests/pileup_compare_reference.py), the writers on a hand-made result, the joint status and the command line's refusals.
No GPU."""
import math
import os

import numpy as np
import pytest

import pileup_compare_reference as cr

HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"
NAN = math.nan


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_a_three_by_three_window_by_hand():
    """w = 1, p = 0.  Map 1: centre 8, every other cell 1; map 2: centre 2, every other cell 1.  Every background mean is 1 on
    both, R_1N = 8, R_2N = 2, LFC_N = log2(4) = 2 exactly, LFC = 2."""
    from mustache_amd.pileup import compare_ratios, lfc_summary
    one = np.ones((1, 3, 3))
    m1, m2 = one.copy(), one.copy()
    m1[0, 1, 1], m2[0, 1, 1] = 8.0, 2.0
    s = cr.sums(m1, m2, 1, 0)
    assert s[0].tolist() == [[4.0, 4.0, 4.0], [1.0, 1.0, 1.0], [6.0, 6.0, 6.0], [6.0, 6.0, 6.0]]
    for r1, r2, lfc_n in (compare_ratios(s, [8.0], [2.0]), cr.ratios(s, [8.0], [2.0])):
        assert r1.tolist() == [[8.0] * 4] and r2.tolist() == [[2.0] * 4] and lfc_n.tolist() == [[2.0] * 4]
        assert lfc_summary(lfc_n).tolist() == [2.0] and cr.summary(lfc_n).tolist() == [2.0]


def test_a_nan_on_either_map_takes_the_cell_from_both():
    """w = 2, p = 0: a NaN of map 1 at (a, b) = (0, 2) (H only) and one of map 2 at (2, 0) (V only): cnt of H and of V drops by one,
    and S of BOTH samples loses that cell."""
    rng = np.random.default_rng(0)
    m1, m2 = rng.uniform(1, 2, (1, 5, 5)), rng.uniform(1, 2, (1, 5, 5))
    full = cr.sums(m1, m2, 2, 0)
    h1, h2, v1, v2 = m1[0, 2, 4], m2[0, 2, 4], m1[0, 4, 2], m2[0, 4, 2]
    m1[0, 2, 4] = NAN
    m2[0, 4, 2] = NAN
    s = cr.sums(m1, m2, 2, 0)
    assert s[0, :, 2].tolist() == [full[0, 0, 2], full[0, 1, 2], full[0, 2, 2] - 1, full[0, 3, 2] - 1]
    assert _same(s[0, :2], full[0, :2])                                   # DONUT and LL hold neither cell
    assert np.allclose(s[0, 2, :2], [full[0, 2, 0] - h1, full[0, 2, 1] - h2], rtol=1e-14)
    assert np.allclose(s[0, 3, :2], [full[0, 3, 0] - v1, full[0, 3, 1] - v2], rtol=1e-14)
    T1, T2, C = cr.paired(m1, m2, [0], [0])
    assert C[2, 4] == C[4, 2] == 0 and C.sum() == 23 and T1[4, 2] == 0 and T2[2, 4] == 0


def test_the_summary_on_literal_rows():
    from mustache_amd.pileup import lfc_summary
    rows = [[1.0, 0.5, 2.0, 3.0], [-1.0, -0.25, -2.0, -3.0], [1.0, -1.0, 2.0, 3.0], [1.0, NAN, 2.0, 3.0], [1.0, 0.0, 2.0, 3.0],
            [0.0, 0.0, 0.0, 0.0], [-1.0, NAN, NAN, NAN], [math.inf, 1.0, 2.0, 3.0]]
    want = [0.5, -0.25, 0.0, NAN, 0.0, 0.0, NAN, 1.0]
    assert _same(lfc_summary(rows), want) and _same(cr.summary(rows), want)
    assert lfc_summary(np.zeros((0, 4))).shape == (0,)


def test_the_ratios_at_every_nan_rule():
    from mustache_amd.pileup import compare_ratios
    s = np.zeros((6, 4, 3))
    s[:] = [6.0, 3.0, 3.0]                                                # background means 2 and 1
    s[1, :, 2] = 0.0                                                      # cnt = 0 (the sums are then 0 too)
    s[1, :, :2] = 0.0
    s[4, :, 0] = 0.0                                                      # the background of sample 1 is 0
    c1 = [4.0, 4.0, 0.0, NAN, 4.0, 4.0]
    c2 = [1.0, 1.0, 1.0, 1.0, 1.0, NAN]
    for r1, r2, lfc in (compare_ratios(s, c1, c2), cr.ratios(s, c1, c2)):
        assert r1[0].tolist() == [2.0] * 4 and r2[0].tolist() == [1.0] * 4 and lfc[0].tolist() == [1.0] * 4
        assert np.isnan(r1[1]).all() and np.isnan(r2[1]).all() and np.isnan(lfc[1]).all()          # cnt = 0
        assert r1[2].tolist() == [0.0] * 4 and r2[2].tolist() == [1.0] * 4 and np.isnan(lfc[2]).all()   # centre 0: R = 0, no LFC
        assert np.isnan(r1[3]).all() and r2[3].tolist() == [1.0] * 4 and np.isnan(lfc[3]).all()    # centre NaN
        assert np.isnan(r1[4]).all() and r2[4].tolist() == [1.0] * 4 and np.isnan(lfc[4]).all()    # background 0
        assert r1[5].tolist() == [2.0] * 4 and np.isnan(r2[5]).all() and np.isnan(lfc[5]).all()    # centre NaN on sample 2


@pytest.mark.parametrize("w,q,p", [(1, 1, 0), (3, 2, 1), (10, 6, 2)])
def test_the_host_functions_against_the_restatement(w, q, p):
    from mustache_amd.pileup import compare_aggregate, compare_ratios, diff_map, lfc_summary
    rng = np.random.default_rng(w)
    S = 2 * w + 1
    C = rng.integers(0, 4, (S, S)).astype(np.float64)
    T1, T2 = rng.uniform(0, 3, (S, S)) * C, rng.uniform(0, 3, (S, S)) * C
    T2[0, 0] = 0.0                                                        # a mean of 0: no ratio there
    C[0, 0] = 2.0
    d = diff_map(T1, T2, C)
    assert np.isnan(d[0, 0]) and np.isnan(d[C == 0]).all() and not np.isnan(d[(C > 0) & (T1 > 0) & (T2 > 0)]).any()
    assert np.allclose(d, cr.diff(T1, T2, C), rtol=1e-14, atol=1e-15, equal_nan=True)
    got, want = compare_aggregate(T1, T2, C, w, q, p), cr.aggregate(T1, T2, C, w, q, p)
    for k in ("m1", "m2", "diff", "p2ll_1", "p2ll_2", "lfc_p2ll", "agg_lfc"):
        assert np.allclose(got[k], want[k], rtol=1e-13, atol=1e-14, equal_nan=True), k
    assert np.array_equal(np.isnan(got["agg_lfc"]), np.isnan(want["agg_lfc"]))
    oe1, oe2 = rng.uniform(0, 2, (40, S, S)), rng.uniform(0, 2, (40, S, S))
    oe1[rng.random(oe1.shape) < 0.2] = NAN
    oe2[rng.random(oe2.shape) < 0.2] = NAN
    oe1[rng.random(oe1.shape) < 0.1] = 0.0
    s = cr.sums(oe1, oe2, w, p)
    got, want = compare_ratios(s, oe1[:, w, w], oe2[:, w, w]), cr.ratios(s, oe1[:, w, w], oe2[:, w, w])
    for g, t in zip(got, want):
        assert np.array_equal(np.isnan(g), np.isnan(t)) and np.allclose(g, t, rtol=1e-15, atol=0, equal_nan=True)
    assert _same(lfc_summary(got[2]), cr.summary(got[2]))
    empty = compare_aggregate(np.zeros((S, S)), np.zeros((S, S)), np.zeros((S, S)), w, q, p)
    assert np.isnan(empty["diff"]).all() and math.isnan(empty["lfc_p2ll"]) and np.isnan(empty["agg_lfc"]).all()


def test_the_joint_status():
    from mustache_amd.pileup import joint_status, joint_status_trans
    ys = [0, 99, 100, 119, 120]
    assert joint_status(ys, 120, 100) == joint_status(ys, 100, 120) == ["used", "used", "off_map", "off_map", "off_map"]
    assert joint_status(ys, 120, 121) == ["used"] * 4 + ["off_map"] == cr.joint_status(ys, 120, 121)
    assert joint_status(ys, 100, 120) == cr.joint_status(ys, 100, 120)
    assert joint_status(ys, None, 120) == joint_status(ys, 120, None) == ["no_chrom"] * 5 == cr.joint_status(ys, None, 120)
    assert joint_status([], 5, 5) == []
    a, b = [0, 37, 38, 39, 5], [0, 49, 10, 10, 50]
    assert joint_status_trans(a, b, (40, 50), (38, 50)) == ["used", "used", "off_map", "off_map", "off_map"]
    assert joint_status_trans(a, b, (38, 60), (40, 50)) == ["used", "used", "off_map", "off_map", "off_map"]
    assert joint_status_trans(a, b, None, (40, 50)) == joint_status_trans(a, b, (40, 50), None) == ["no_pair"] * 5


# ---- the writers ---------------------------------------------------------------------------------------------------------------
def _hand_result():
    from mustache_amd.pileup import LoopTable, PileupPairResult, compare_aggregate
    lines = ["1\t%d\t%d\t1\t%d\t%d\t0.01\t1.6" % (k * 10, k * 10 + 10, k * 10 + 500, k * 10 + 510) for k in range(6)]
    cols = [ln.split("\t") for ln in lines]
    table = LoopTable(HEADER, lines, [c[0] for c in cols], [int(c[1]) for c in cols], [int(c[2]) for c in cols],
                      [c[3] for c in cols], [int(c[4]) for c in cols], [int(c[5]) for c in cols])
    status = ["used", "short", "used", "used", "off_map", "used"]
    res = PileupPairResult(table, status, 1, 1, 0)
    lfc = {0: 1.5, 2: -0.5, 3: NAN, 5: -2.0}
    for k, v in lfc.items():
        res.first.oe_center[k], res.second.oe_center[k] = 3.0 + k, 1.0 + k
        res.r1[k], res.r2[k] = [2.0, 2.5, 3.0, 3.5], [1.0, 1.25, 1.5, 1.75]
        res.lfc_n[k], res.lfc[k] = [v, v, v, v], v
    res.lfc[4] = 9.0                                                      # a row that is not `used` never reaches a list
    T1 = np.arange(1.0, 10.0).reshape(3, 3)
    part = compare_aggregate(T1, 2 * T1, np.full((3, 3), 2.0), 1, 1, 0)
    res.chromosomes.append(("1", 4, part))
    res.all = part
    return res, lines


def test_write_compare_on_a_hand_made_result(tmp_path):
    from mustache_amd.pileup import COMPARE_COLUMNS, COMPARE_STATS_HEADER, write_compare
    res, lines = _hand_result()
    assert COMPARE_COLUMNS == ("STATUS", "OE_CENTER_1", "OE_CENTER_2", "R1_DONUT", "R1_LL", "R1_H", "R1_V", "R2_DONUT", "R2_LL",
                               "R2_H", "R2_V", "LFC_DONUT", "LFC_LL", "LFC_H", "LFC_V", "LFC")
    assert COMPARE_STATS_HEADER == "CHR\tLOOPS_USED\tP2LL_1\tP2LL_2\tLFC_P2LL\tAGG_LFC_DONUT\tAGG_LFC_LL\tAGG_LFC_H\tAGG_LFC_V\n"
    prefix = str(tmp_path / "o")
    assert write_compare(prefix, res) is None
    assert sorted(os.listdir(tmp_path)) == ["o.compare.stats.tsv", "o.compare.tsv", "o.diff.tsv"]
    body = open(prefix + ".compare.tsv").read().splitlines()
    assert body[0] == HEADER + "\t" + "\t".join(COMPARE_COLUMNS)
    rows = [ln.split("\t") for ln in body[1:]]
    assert ["\t".join(f[:8]) for f in rows] == lines and [f[8] for f in rows] == res.status
    assert all(len(f) == 8 + len(COMPARE_COLUMNS) for f in rows)
    assert rows[1][9:] == ["nan"] * 15 and rows[4][9:23] == ["nan"] * 14
    assert rows[0][9:] == ["3.0", "1.0", "2.0", "2.5", "3.0", "3.5", "1.0", "1.25", "1.5", "1.75", "1.5", "1.5", "1.5", "1.5", "1.5"]
    assert rows[3][-1] == "nan" and rows[5][-1] == "-2.0"
    assert open(prefix + ".diff.tsv").read() == "-1.0\t-1.0\t-1.0\n" * 3                    # log2(T / 2T) in every cell
    stats = [ln.split("\t") for ln in open(prefix + ".compare.stats.tsv").read().splitlines()]
    assert [s[0] for s in stats] == ["CHR", "1", "all"] and stats[1][1:] == stats[2][1:] and stats[1][1] == "4"
    assert stats[1][2:] == [repr(5.0 / 7.0), repr(5.0 / 7.0)] + ["0.0"] * 5   # centre 5, LL 7 (w = q = 1); every ratio is scale-free
    # the thresholded lists: exactly the used rows by the LFC as written
    assert write_compare(prefix, res, 0.5) == (1, 2)
    assert open(prefix + ".up1.tsv").read().splitlines() == [HEADER, lines[0]]
    assert open(prefix + ".up2.tsv").read().splitlines() == [HEADER, lines[2], lines[5]]     # -0.5 <= -T counts, NaN does not
    assert write_compare(prefix, res, 1.75) == (0, 1)
    assert open(prefix + ".up1.tsv").read() == HEADER + "\n"
    written = {k: float(f[-1]) for k, f in enumerate(rows) if f[8] == "used"}
    assert [lines[k] for k, v in written.items() if v <= -1.75] == open(prefix + ".up2.tsv").read().splitlines()[1:]


# ---- the command line ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def files(tmp_path, monkeypatch):
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    out = {}
    for name in ("m.hic", "m2.hic", "m.txt", "m2.txt", "m.pairs", "bias.txt", "bias2.txt"):
        out[name] = str(tmp_path / name)
        with open(out[name], "wb") as fh:
            fh.write(b"not read\n")                          # a refusal comes before any read
    out["absent.hic"], out["absent.txt"] = str(tmp_path / "absent.hic"), str(tmp_path / "absent.txt")
    out["loops"] = str(tmp_path / "l.tsv")
    with open(out["loops"], "w") as fh:
        fh.write(HEADER + "\n1\t100000\t110000\t1\t900000\t910000\t0.01\t1.6\n")
    out["dir"] = tmp_path
    return out


F2 = ["-f2", "m2.hic"]
CASES = [
    ("m.hic", ["-b2", "bias2.txt"], "-b2 without -f2"),
    ("m.hic", ["--min-lfc", "1"], "--min-lfc without -f2"),
    ("m.hic", ["-f2", "absent.hic"], "Couldn't find the second contact file"),
    ("m.txt", ["-f2", "m2.txt", "-b", "bias.txt", "-b2", "absent.txt"], "Couldn't find the bias file of the second map"),
    ("m.hic", F2 + ["--min-lfc", "0"], "--min-lfc 0.0"),
    ("m.hic", F2 + ["--min-lfc", "-1"], "--min-lfc -1.0"),
    ("m.hic", F2 + ["--min-lfc", "nan"], "--min-lfc nan"),
    ("m.hic", F2 + ["--min-lfc", "inf"], "--min-lfc inf"),
    ("m.hic", F2 + ["--peak", "10"], "--peak 10 with -w 10"),
    ("m.hic", F2 + ["--peak", "-1"], "--peak -1 with -w 10"),
    ("m.hic", F2 + ["-w", "2"], "--peak 2 with -w 2"),                                     # the default P = 2 needs w >= 3
    ("m.hic", F2 + ["--enrich"], "-f2 with --enrich"),
    ("m.hic", F2 + ["--min-enrichment", "1.5"], "-f2 with --min-enrichment"),
    ("m.hic", F2 + ["--trans", "--balance-genome", "NEWTON"], "-f2 with --balance-genome"),
    ("m.hic", F2 + ["--trans", "--balance-pixels", "inter"], "-f2 with --balance-pixels"),
    ("m.pairs", F2 + ["--trans", "--pairs-trans", "--balance-genome", "ICE"], "-f2 with --balance-genome"),
    ("m.pairs", F2 + ["--pairs-trans"], "-f2 with --pairs-trans"),
]


@pytest.mark.parametrize("name,extra,text", CASES, ids=["%s %s" % (c[0], " ".join(c[1])) for c in CASES])
def test_refusals_are_one_error_line_and_no_file(files, name, extra, text, capsys):
    from mustache_amd.pileup import main
    prefix = str(files["dir"] / "out")
    extra = [files[a] if a in files else a for a in extra]
    main(["-f", files[name], "-l", files["loops"], "-r", "10kb", "-o", prefix] + extra)
    said = capsys.readouterr().out.splitlines()
    errors = [ln for ln in said if ln.startswith("Error:")]
    assert len(errors) == 1 and said == errors, said
    assert text in errors[0], errors[0]
    assert not [f for f in os.listdir(files["dir"]) if f.startswith("out")]


def test_the_parser_knows_the_flags_and_a_plain_request_asks_for_nothing(files):
    from mustache_amd.pileup import DEFAULT_PEAK, PileupError, compare_request, enrich_request, parse_args
    base = ["-f", files["m.hic"], "-l", "l.tsv", "-r", "10kb", "-o", "o"]
    a = parse_args(base)
    assert a.f2_path is None and a.biasfile2 is None and a.min_lfc is None and compare_request(a, 1) is None
    a = parse_args(base + ["--file2", files["m2.hic"]])
    assert compare_request(a, 1) == DEFAULT_PEAK == 2
    a = parse_args(base + ["-f2", files["m2.hic"], "--peak", "0", "--min-lfc", "0.25", "--biases2", files["bias2.txt"]])
    assert compare_request(a, 1) == 0 and a.min_lfc == 0.25 and a.biasfile2 == files["bias2.txt"]
    with pytest.raises(PileupError, match="--peak without --enrich"):      # without -f2 --peak still belongs to --enrich
        enrich_request(parse_args(base + ["--peak", "1"]))
    with pytest.raises(PileupError, match="one GPU only"):
        compare_request(a, 2)


def test_the_entry_points_are_declared_bound_and_built():
    from mustache_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mustache_hip.h")).read()
    assert "MST_STABLE int mst_pileup_compare(" in hdr and "MST_STABLE int mst_pileup_reduce_pair(" in hdr
    assert "#define MST_ABI_REVISION 1" in hdr and _lib.MST_ABI_REVISION == 1
    assert {"mst_pileup_compare", "mst_pileup_reduce_pair"} <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert hasattr(lib, "mst_pileup_compare") and hasattr(lib, "mst_pileup_reduce_pair")
    assert "mst_pileup_compare.hip" in open(os.path.join(root, "mustache_amd", "csrc", "Makefile")).read()
