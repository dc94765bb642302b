"""Whole-genome balancing for inter-chromosomal calling, without a GPU: the NumPy restatement (tests/balance_genome_reference.py)
-- assembly, both methods on both pixel sets, the application -- and every refusal of `--balance-genome` / `--balance-pixels` on
both command lines (each is decided before the GPU is touched)."""
import os

import numpy as np
import pytest

import balance_genome_reference as gr
import balance_reference as br
import newton_reference as nr
from hic_trans_writer import write_hic_pairs

RES = 10000
LENGTHS = [69 * RES + 5, 49 * RES, 39 * RES + 9999]          # 70 / 50 / 40 bins


# ---- 1. assembly ------------------------------------------------------------------------------------------------------------
def test_layout_and_assembly():
    bins, off, n = gr.layout(LENGTHS, RES)
    assert bins == [70, 50, 40] and off == [0, 70, 120] and n == 160
    from mustache_amd.balance_genome import genome_layout
    assert genome_layout(LENGTHS, RES) == (bins, off, n)
    cis = {0: ([5, 5, 5, 0], [6, 7, 5, 69], [3.0, 4.0, 9.0, 1.0]), 2: ([1], [39], [2.0])}
    trans = {(0, 1): ([69, 3], [0, 49], [7.0, 8.0]), (1, 2): ([49], [0], [5.0])}
    lo, hi, v = gr.assemble(bins, off, cis, trans, "all")
    cells = sorted(zip(lo.tolist(), hi.tolist(), v.tolist()))
    # the cis pixels (5, 6) and (5, 5) are dropped, (5, 7) is kept; (bin 69 of chr 1, bin 0 of chr 2) is kept at genome distance 1
    assert cells == [(0, 69, 1.0), (3, 119, 8.0), (5, 7, 4.0), (69, 70, 7.0), (119, 120, 5.0), (121, 159, 2.0)]
    assert (69, 70, 7.0) in cells and (5, 6, 3.0) not in cells
    lo_i, hi_i, v_i = gr.assemble(bins, off, cis, trans, "inter")
    inter = sorted(zip(lo_i.tolist(), hi_i.tolist(), v_i.tolist()))
    assert inter == [(3, 119, 8.0), (69, 70, 7.0), (119, 120, 5.0)]                  # no cis pixel
    # a pair stored as (B, A) lands in the same cells
    swapped = {(1, 0): (trans[(0, 1)][1], trans[(0, 1)][0], trans[(0, 1)][2]), (1, 2): trans[(1, 2)]}
    lo_s, hi_s, v_s = gr.assemble(bins, off, cis, swapped, "all")
    assert sorted(zip(lo_s.tolist(), hi_s.tolist(), v_s.tolist())) == cells
    # a record outside its chromosome is dropped, not moved into the next one
    lo_o, _, _ = gr.assemble(bins, off, {}, {(0, 1): ([70, 2], [1, 50], [1.0, 1.0])}, "inter")
    assert len(lo_o) == 0


# ---- 2. both methods, both pixel sets ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome():
    bins, off, n = gr.layout(LENGTHS, RES)
    cis, trans = gr.synth_genome()
    return bins, off, n, cis, trans


# measured with this restatement: all = 10 227 pixels, inter = 6 105; NEWTON 28 / 29 mat-vecs, ICE 14 / 14 iterations; bins 7, 83
# and 131 masked in all four runs; NEWTON's residual 2.5e-7 / 3.2e-7
@pytest.mark.parametrize("pixels", ["all", "inter"])
def test_both_methods_converge(genome, pixels):
    """NEWTON is held to newton_reference.condition's residual.  condition() measures 1 - x (A x), which only Newton's scale
    makes zero; ICE solves x (A x) = const, so it is held to its own stop test on the same matrix instead: the variance of
    s / mean(s), s the balanced marginals, below its tol of 1e-5."""
    bins, off, n, cis, trans = genome
    lo, hi, v = gr.assemble(bins, off, cis, trans, pixels)
    assert (len(v) > 9000) if pixels == "all" else (5000 < len(v) < 7000)
    if pixels == "inter":
        chrom = np.searchsorted(np.asarray(off), lo, side="right"), np.searchsorted(np.asarray(off), hi, side="right")
        assert (chrom[0] != chrom[1]).all()
    masks = {}
    for method in ("NEWTON", "ICE"):
        bias, info = gr.balance(method, lo, hi, v, n)
        assert info["converged"], (method, pixels)
        masked = info["masked"]
        assert 0 < int(masked.sum()) < n
        assert np.isnan(bias[masked]).all() and np.isfinite(bias[~masked]).all()
        masks[method] = masked
        if method == "NEWTON":
            res, kappa, act = nr.condition(lo, hi, v, n, bias, info, ignore_diags=0)
            print(method, pixels, len(v), info["matvecs"], int(masked.sum()), float(np.linalg.norm(res)))
            assert np.linalg.norm(res) <= 1.001e-6
            assert abs(kappa / info["kappa"] - 1.0) <= 1e-12
        else:
            i, j, vv = br.kept_pixels(lo, hi, v, n, 0)
            rows, cols, vals = br._sym(i, j, vv)
            w = np.where(masked, 0.0, info["kappa"] / np.where(masked, 1.0, bias))
            s = br.marginals(rows, cols, vals, w, n)
            s = s[s != 0]
            print(method, pixels, len(v), info["iterations"], int(masked.sum()), float(np.var(s / s.mean())))
            assert np.var(s / s.mean()) < 1e-5
    assert np.array_equal(masks["NEWTON"], masks["ICE"])


# ---- 3. application ---------------------------------------------------------------------------------------------------------
def test_application_against_hand_values():
    #          0    1    2       3     4    5    6
    bias = [1.0, 2.0, np.nan, 0.1, 0.5, 4.0, 0.2]
    # pair (A, B) with off_A = 0 (3 bins), off_B = 3
    x = np.array([0, 1, 2, 1, 0, 1, 1, -1])
    y = np.array([1, 2, 1, 0, 3, 3, 4, 1])
    v = np.array([3.0, 8.0, 5.0, 6.0, 1.0, 1.0, 1.0, 1.0])
    got = gr.apply(bias, 0, 3, x, y, v)
    # (3 / 1) / 0.5; (8 / 2) / 4; NaN bin of A: 0; bias 0.1 < 0.2: 0; bias 0.2 is kept: (1 / 1) / 0.2; bin 7 is past n: 0;
    # a negative bin: 0
    assert got.tolist() == [6.0, 1.0, 0.0, 0.0, 5.0, 2.5, 0.0, 0.0]
    bx, by, bv = gr.balanced(bias, 0, 3, x, y, v)
    assert bx.tolist() == [0, 1, 0, 1] and by.tolist() == [1, 2, 3, 3] and bv.tolist() == [6.0, 1.0, 5.0, 2.5]
    assert np.isnan(gr.apply(bias, 0, 3, [0], [1], [np.nan])[0])
    # float64 throughout: (v / bx) / by, not v / (bx * by) and not rounded to float32
    b = np.array([0.3, 0.7])
    assert gr.apply(b, 0, 1, [0], [0], [1.0])[0] == (1.0 / 0.3) / 0.7


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def _tiny_hic(path):
    chroms = [("All", 1000), ("1", 200000), ("2", 150000)]
    write_hic_pairs(str(path), chroms, {(1, 2): {10000: ([0, 1], [2, 3], [5.0, 6.0])}}, version=8)
    return str(path)


OLD_LINE = "Error: --balance does not apply to inter-chromosomal pairs"
NOT_TRANS = "Error: --balance-genome is for inter-chromosomal calls; use --balance"
TEXT_LINE = "Error: Interchromosomal analysis is only supported for .hic and .cool input formats."

# (extra arguments, what the Error: line holds, the input: hic / cool / text, ranks)
REFUSALS = [
    (["-ch", "1", "--balance-genome", "NEWTON"], NOT_TRANS, "hic", 1),
    (["-ch", "1", "1", "-ch2", "1", "2", "--balance-genome", "NEWTON"], NOT_TRANS, "hic", 1),
    (["-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON", "-norm", "KR"], "Error: --balance-genome NEWTON and -norm KR", "hic", 1),
    (["--trans-all", "--balance-genome", "ICE", "-norm", "VC"], "Error: --balance-genome ICE and -norm VC", "hic", 1),
    (["-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON", "BIAS"], "give either a bias file or --balance-genome", "hic", 1),
    (["--trans-all", "--balance-genome", "NEWTON", "BIAS"], "give either a bias file or --balance-genome", "hic", 1),
    (["-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON"], ".cool/.mcool files carry their own `weight` column", "cool", 1),
    (["-ch", "1", "2", "--trans-all", "--balance-genome", "NEWTON"], ".cool/.mcool files carry their own `weight` column", "cool", 1),
    (["-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON"], TEXT_LINE, "text", 1),
    (["-ch", "1", "2", "--trans-all", "--balance-genome", "NEWTON"], TEXT_LINE, "text", 1),
    (["-ch", "1", "-ch2", "2", "--balance-genome", "KR"], "Error: --balance-genome KR: unknown method (supported: ICE, NEWTON)", "hic", 1),
    (["--trans-all", "--balance-genome", "NEWTON", "--balance-pixels", "cis"],
     "Error: --balance-pixels cis: unknown value (supported: all, inter)", "hic", 1),
    (["-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON"], "Error: inter-chromosomal pairs run on one GPU only", "hic", 2),
    (["--trans-all", "--balance-genome", "NEWTON"], "Error: inter-chromosomal pairs run on one GPU only", "hic", 2),
    (["-ch", "1", "-ch2", "2", "--balance-pixels", "inter"], "Error: --balance-pixels inter without --balance-genome", "hic", 1),
    (["--trans-all", "--balance-pixels", "all"], "Error: --balance-pixels all without --balance-genome", "hic", 1),
    (["-ch", "1", "--balance-pixels", "inter"], "Error: --balance-pixels inter without --balance-genome", "hic", 1),
    (["-ch", "1", "-ch2", "2", "--balance", "ICE", "--balance-genome", "NEWTON"], OLD_LINE, "hic", 1),
    (["--trans-all", "--balance", "ICE", "--balance-genome", "NEWTON"], OLD_LINE, "hic", 1),
]


def _input(tmp_path, kind, name):
    if kind == "hic":
        return _tiny_hic(tmp_path / (name + ".hic"))
    p = tmp_path / (name + (".cool" if kind == "cool" else ".txt"))
    p.write_text("1\t10000\t2\t20000\t5\n")          # never opened: the refusal comes first
    return str(p)


@pytest.mark.parametrize("extra,line,kind,ranks", REFUSALS)
def test_one_sample_refusals_write_nothing(tmp_path, capsys, monkeypatch, extra, line, kind, ranks):
    import mustache_amd.sharding as sh
    from mustache_amd.mustache import main
    monkeypatch.setattr(sh, "init_from_env", lambda: (0, ranks))
    bias = tmp_path / "bias.txt"
    bias.write_text("1\t0\t1.0\n")
    extra = [a for e in extra for a in (["-b", str(bias)] if e == "BIAS" else [e])]
    out = tmp_path / "o.tsv"
    capsys.readouterr()
    main(["-f", _input(tmp_path, kind, "p"), "-r", "10kb", "-o", str(out)] + extra)
    said = capsys.readouterr().out
    assert line in said and said.count("Error:") == 1, said
    assert not out.exists()


@pytest.mark.parametrize("extra,line,kind,ranks", REFUSALS)
def test_two_sample_refusals_write_nothing(tmp_path, capsys, monkeypatch, extra, line, kind, ranks):
    import mustache_amd.sharding as sh
    from mustache_amd.diff_mustache import SUFFIX, main
    monkeypatch.setattr(sh, "init_from_env", lambda: (0, ranks))
    bias = tmp_path / "bias.txt"
    bias.write_text("1\t0\t1.0\n")
    extra = [a for e in extra for a in (["-b2", str(bias)] if e == "BIAS" else [e])]
    out = tmp_path / "o"
    capsys.readouterr()
    # the second file is the one of the kind under test: each file is checked, not only the first
    main(["-f1", _input(tmp_path, "hic", "a"), "-f2", _input(tmp_path, kind, "b"), "-r", "10kb", "-o", str(out)] + extra)
    said = capsys.readouterr().out
    assert line in said and said.count("Error:") == 1, said
    assert not any(os.path.exists(str(out) + suf) for suf in SUFFIX.values())


def test_check_genome_request():
    from mustache_amd.balance import BalanceError
    from mustache_amd.balance_genome import check_genome_request
    assert check_genome_request("newton", "INTER", ["a.hic", "b.hic"], None, "NONE", None, 1, True) == ("NEWTON", "inter")
    assert check_genome_request("ICE", "all", "a.hic", None, False, None, 1, "all") == ("ICE", "all")
    for args, text in (
            (("ICE", "all", "a.hic", None, None, None, 1, False), "--balance-genome is for inter-chromosomal calls; use --balance"),
            (("ICE", "all", "a.hic", None, None, None, 1, "some"), "--balance-genome is for inter-chromosomal calls; use --balance"),
            (("ICE", "all", "a.hic", None, None, "ICE", 1, True), "--balance does not apply to inter-chromosomal pairs"),
            (("ICE", "all", "a.hic", None, None, None, 4, True), "multi-rank run (world size 4)"),
            (("ICE", "all", "a.mcool", None, None, None, 1, True), "a.mcool: .cool/.mcool files"),
            (("ICE", "all", "a.hic", "b.txt", None, None, 1, True), "not both"),
            ((None, "inter", "a.hic", None, None, None, 1, True), "without --balance-genome")):
        with pytest.raises(BalanceError) as e:
            check_genome_request(*args)
        assert text in str(e.value)


def test_positional_signatures_are_kept(tmp_path):
    """what diff_mustache.trans_all_request and diff_trans.refusal answered before the rules moved, through request.plan()"""
    from mustache_amd.request import Request, plan

    def ask(files, ch, ch2, balance, ranks, trans_all):
        for f in files:
            (tmp_path / f).write_bytes(b"")
        run = plan(Request([str(tmp_path / f) for f in files], [(None, ""), (None, "")], "-b1/-b2", False, balance, None, "all",
                           False, False, False, trans_all, ch, ch2, ranks, False), 10000)
        return run if isinstance(run, str) else run.trans
    assert ask(("a.hic", "b.hic"), ["1", "2"], 'n', None, 1, True) == [("1", "2")]
    assert ask(("a.hic", "b.hic"), ["1", "2"], 'n', "ICE", 1, True) == OLD_LINE
    assert ask(("a.hic", "b.hic"), ["1"], ["2"], None, 1, False) == [("1", "2")]
    assert ask(("a.hic", "b.hic"), ["1"], ["2"], "ICE", 1, False) == OLD_LINE


# ---- 5. defaults ------------------------------------------------------------------------------------------------------------
def test_parse_args_defaults():
    from mustache_amd import diff_mustache, mustache
    for args in (mustache.parse_args(["-o", "x", "-r", "10kb"]), diff_mustache.parse_args(["-o", "x", "-r", "10kb"])):
        assert args.balance_genome is None and args.balance_pixels == "all" and args.balance_pixels_given is False
    args = mustache.parse_args(["-o", "x", "-r", "10kb", "--balance-genome", "ICE", "--balance-pixels", "all"])
    assert args.balance_genome == "ICE" and args.balance_pixels == "all" and args.balance_pixels_given is True


def test_the_library_exports_the_new_entry_point():
    from mustache_amd import _lib
    assert "mst_balance_apply_pairs" in _lib.exported_symbols()
    lib = _lib.load()
    assert hasattr(lib, "mst_balance_apply_pairs")
    assert lib.mst_abi_revision() == _lib.MST_ABI_REVISION >= 1 and lib.mst_abi_version() == _lib.MST_ABI_VERSION == 3
