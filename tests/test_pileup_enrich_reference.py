"""The enrichment rules of mustache_amd/pileup.py on the host: the neighbourhood masks against their closed forms, the ratios
against a case worked by hand and at every NaN rule, pileup.py's NumPy functions against the cell-by-cell restatement
(tests/pileup_enrich_reference.py), and the command line's three refusals.  No GPU."""
import math
import os

import numpy as np
import pytest

import pileup_enrich_reference as er

HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"


@pytest.mark.parametrize("w,p", [(1, 0), (10, 2), (64, 63)])
def test_mask_sizes_have_their_closed_forms(w, p):
    from mustache_amd.pileup import NEIGHBOURHOODS, enrichment_masks
    assert NEIGHBOURHOODS == er.NEIGHBOURHOODS == ("DONUT", "LL", "H", "V")
    m = enrichment_masks(w, p)
    assert m.shape == (4, 2 * w + 1, 2 * w + 1) and m.dtype == bool
    assert [int(k.sum()) for k in m] == [(2 * w) ** 2 - (2 * p) ** 2, w * w - p * p, 6 * (w - p), 6 * (w - p)]
    assert np.array_equal(m, er.masks(w, p))
    assert not m[:, w - p:w + p + 1, w - p:w + p + 1].any()          # nothing inside the peak box
    assert m[1, w + 1:, :w].sum() == m[1].sum()                      # LL: a >= 1 and b <= -1, the LL corner's side


def test_masks_refuse_a_peak_that_leaves_no_neighbourhood():
    from mustache_amd.pileup import PileupError, enrichment_masks
    for w, p in [(3, 3), (3, 4), (3, -1), (0, 0)]:
        with pytest.raises(PileupError, match="peak half-width"):
            enrichment_masks(w, p)


def test_a_three_by_three_window_by_hand():
    """w = 1, p = 0, trans (e = 2 everywhere).  Rows a = -1, 0, 1, columns b = -1, 0, 1:
           1    2    NaN
           4    12   6
           8    3    5
    DONUT = the corners (a != 0, b != 0) 1, NaN, 8, 5: S_o = 14, cnt = 3, S_e = 6.  LL = (a, b) = (1, -1): 8.  H = |b| = 1, every
    row: 1, NaN, 4, 6, 8, 5: S_o = 24, cnt = 5, S_e = 10.  V = |a| = 1, every column: 1, 2, NaN, 8, 3, 5: S_o = 19, cnt = 5.
    EXP = 2 * S_o / S_e = 14 / 3, 8, 4.8, 3.8; FE = 12 / EXP."""
    from mustache_amd.pileup import enrichment
    win = np.array([[[1.0, 2.0, np.nan], [4.0, 12.0, 6.0], [8.0, 3.0, 5.0]]])
    sums = er.trans_sums(win, 1, 0, 2.0)
    assert sums.tolist() == [[[14.0, 6.0, 3.0], [8.0, 2.0, 1.0], [24.0, 10.0, 5.0], [19.0, 10.0, 5.0]]]
    for exp, fe, fe_min in (enrichment(sums, [12.0], [2.0]), er.ratios(sums, [12.0], [2.0])):
        assert exp.shape == fe.shape == (1, 4) and fe_min.shape == (1,)
        assert np.allclose(exp[0], [14.0 / 3.0, 8.0, 4.8, 3.8], rtol=1e-15)
        assert np.allclose(fe[0], [12.0 * 3.0 / 14.0, 1.5, 2.5, 12.0 / 3.8], rtol=1e-15)
        assert fe_min[0] == fe[0, 1] == 1.5


def test_cis_cells_take_the_expected_value_of_their_own_distance():
    """w = 1, p = 0, loop (x, y) = (5, 7): cell (a, b) lies at distance 2 + b - a.  E[4] = 0 takes (a, b) = (-1, 1) out; D = 3
    would too."""
    from mustache_amd.pileup import enrichment
    win = np.arange(1.0, 10.0).reshape(1, 3, 3)
    E = np.array([10.0, 8.0, 6.0, 4.0, 0.0])
    s = er.cis_sums(win, 1, 0, E, 4, [5], [7])
    assert s[0, 0].tolist() == [1.0 + 7.0 + 9.0, 6.0 + 10.0 + 6.0, 3.0]          # corners (-1,-1), (1,-1), (1,1): d = 2, 0, 2
    assert s[0, 1].tolist() == [7.0, 10.0, 1.0]
    exp, fe, _fe_min = enrichment(s, [5.0], [E[2]])                              # E_centre = E[y - x] = 6
    assert exp[0, 1] == 6.0 * 7.0 / 10.0 and fe[0, 1] == 5.0 / (6.0 * 7.0 / 10.0)
    assert np.array_equal(exp, er.ratios(s, [5.0], [E[2]])[0])
    assert np.array_equal(er.cis_sums(win, 1, 0, np.array([10.0, 8.0, 6.0, 4.0]), 3, [5], [7]), s)
    near = er.cis_sums(win, 1, 0, E, 4, [5], [5])                               # y - x < 2w: mirrored cells, d = |b - a|
    assert near[0, 0].tolist() == [1.0 + 3.0 + 7.0 + 9.0, 10.0 + 6.0 + 6.0 + 10.0, 4.0]


def test_the_nan_rules():
    from mustache_amd.pileup import enrichment
    ok = [10.0, 5.0, 4.0]
    sums = np.array([[ok, ok, ok, ok],
                     [[0.0, 0.0, 0.0], ok, ok, ok],              # an empty neighbourhood
                     [ok, [3.0, 0.0, 2.0], ok, ok],              # S_e = 0
                     [ok, ok, ok, ok],                           # a NaN centre
                     [ok, ok, ok, ok],                           # E_centre = 0
                     [ok, ok, [0.0, 5.0, 4.0], ok]])             # S_o = 0: EXP = 0
    c = np.array([8.0, 8.0, 8.0, np.nan, 8.0, 8.0])
    e = np.array([2.0, 2.0, 2.0, 2.0, 0.0, 2.0])
    for exp, fe, fe_min in (enrichment(sums, c, e), er.ratios(sums, c, e)):
        assert exp[0].tolist() == [4.0] * 4 and fe[0].tolist() == [2.0] * 4 and fe_min[0] == 2.0
        assert np.isnan(exp[1]).tolist() == [True, False, False, False] and np.isnan(fe[1]).tolist() == [True, False, False, False]
        assert np.isnan(exp[2]).tolist() == [False, True, False, False] and np.isnan(fe[2]).tolist() == [False, True, False, False]
        assert np.isnan(exp[3]).all() and np.isnan(fe[3]).all()
        assert exp[4].tolist() == [0.0] * 4 and np.isnan(fe[4]).all()
        assert exp[5].tolist() == [4.0, 4.0, 0.0, 4.0] and np.isnan(fe[5]).tolist() == [False, False, True, False]
        assert np.isnan(fe_min).tolist() == [False, True, True, True, True, True]


def test_fe_min_is_the_smallest_and_one_nan_spoils_it():
    from mustache_amd.pileup import enrichment
    sums = np.zeros((3, 4, 3))
    sums[:, :, 1], sums[:, :, 2] = 1.0, 1.0
    sums[0, :, 0] = [4.0, 2.0, 8.0, 16.0]                        # EXP = S_o with E_centre = 1: FE = 8 / S_o
    sums[1, :, 0] = [16.0, 8.0, 4.0, 1.0]
    sums[2, :, 0] = [4.0, 2.0, 8.0, 16.0]
    sums[2, 3, 2] = 0.0                                          # V empty
    for _exp, fe, fe_min in (enrichment(sums, [8.0] * 3, [1.0] * 3), er.ratios(sums, [8.0] * 3, [1.0] * 3)):
        assert fe[0].tolist() == [2.0, 4.0, 1.0, 0.5] and fe_min[0] == 0.5
        assert fe_min[1] == 0.5 and fe[1, 0] == 0.5
        assert fe[2, :3].tolist() == [2.0, 4.0, 1.0] and math.isnan(fe[2, 3]) and math.isnan(fe_min[2])
    exp, fe, fe_min = enrichment(np.zeros((0, 4, 3)), np.zeros(0), np.zeros(0))
    assert exp.shape == fe.shape == (0, 4) and fe_min.shape == (0,)


def test_the_aggregate_on_the_mean_map():
    from mustache_amd.pileup import aggregate_enrichment
    rng = np.random.default_rng(5)
    w, p = 4, 1
    M = rng.uniform(0.5, 2.0, (2 * w + 1, 2 * w + 1))
    M[w, w] = 3.0
    M[0, :] = np.nan                                             # a row no loop reached
    got, want = aggregate_enrichment(M, w, p), er.aggregate(M, w, p)
    assert np.allclose(got, want, rtol=1e-14) and not np.isnan(got).any()
    m = er.masks(w, p)
    assert math.isclose(got[1], 3.0 / np.nanmean(M[m[1]]), rel_tol=1e-14)
    M[m[2]] = np.nan                                             # H without a cell
    M[m[3] & ~m[2]] = 0.0                                        # what is left of V: mean 0
    got = aggregate_enrichment(M, w, p)
    assert np.isnan(got).tolist() == [False, False, True, True]
    assert np.isnan(er.aggregate(M, w, p)).tolist() == [False, False, True, True]
    assert np.isnan(aggregate_enrichment(np.full((3, 3), np.nan), 1, 0)).all()


@pytest.fixture()
def files(tmp_path, monkeypatch):
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    out = {"dir": tmp_path, "map": str(tmp_path / "m.txt"), "bias": str(tmp_path / "b.txt"), "loops": str(tmp_path / "l.tsv")}
    for name in ("map", "bias"):
        with open(out[name], "wb") as fh:
            fh.write(b"not read\n")                              # a refusal comes before any read
    with open(out["loops"], "w") as fh:
        fh.write(HEADER + "\n1\t100000\t110000\t1\t900000\t910000\t0.01\t1.6\n")
    return out


@pytest.mark.parametrize("extra,text", [
    (["--peak", "2"], "--peak without --enrich"),
    (["--min-enrichment", "1.5"], "--min-enrichment without --enrich"),
    (["--enrich", "--peak", "10"], "--peak 10 with -w 10"),
    (["--enrich", "-w", "2"], "--peak 2 with -w 2"),             # the default peak against a small window
    (["--enrich", "--peak", "-1"], "--peak -1 with -w 10"),
], ids=["peak", "min-enrichment", "P = w", "default P = w", "P < 0"])
def test_refusals_are_one_error_line_and_no_file(files, extra, text, capsys):
    from mustache_amd.pileup import main
    prefix = str(files["dir"] / "out")
    main(["-f", files["map"], "-b", files["bias"], "-l", files["loops"], "-r", "10kb", "-o", prefix] + extra)
    said = capsys.readouterr().out.splitlines()
    assert len(said) == 1 and said[0].startswith("Error:") and text in said[0], said
    assert not [f for f in os.listdir(files["dir"]) if f.startswith("out")]


def test_the_parser_and_a_plain_request():
    from mustache_amd.pileup import DEFAULT_PEAK, ENRICH_COLUMNS, enrich_request, parse_args
    base = ["-f", "m.hic", "-l", "l.tsv", "-r", "10kb", "-o", "o"]
    a = parse_args(base)
    assert not a.enrich and a.peak is None and a.min_enrichment is None and enrich_request(a) is None
    assert enrich_request(parse_args(base + ["--enrich"])) == DEFAULT_PEAK == 2
    a = parse_args(base + ["--enrich", "--peak", "0", "--min-enrichment", "1.25", "-w", "1"])
    assert enrich_request(a) == 0 and a.min_enrichment == 1.25
    assert ENRICH_COLUMNS == ("STATUS", "OBS_CENTER", "E_CENTER", "EXP_DONUT", "EXP_LL", "EXP_H", "EXP_V", "FE_DONUT", "FE_LL",
                              "FE_H", "FE_V", "FE_MIN")


def test_the_entry_point_is_declared_and_bound_without_a_new_revision():
    from mustache_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mustache_hip.h")).read()
    assert "MST_STABLE int mst_pileup_enrich(" in hdr and "#define MST_ABI_REVISION 1" in hdr
    assert "mst_pileup_enrich" in _lib.exported_symbols() and _lib.MST_ABI_REVISION == 1
    assert hasattr(_lib.load(), "mst_pileup_enrich")
    assert "mst_pileup_enrich.hip" in open(os.path.join(root, "mustache_amd", "csrc", "Makefile")).read()
