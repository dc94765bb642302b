"""The two-sample inter-chromosomal caller without a GPU: the restatement of its rules (tests/diff_trans_reference.py) checked
against itself and against the pieces it is built from, the conditions its shared cases must offer, and the command line's
refusals."""
import numpy as np
import pytest

import diff_trans_reference as dr
import trans_reference as tr
from hic_trans_writer import write_hic_pairs

_JOBS = {}


def _job(name):
    if name not in _JOBS:
        _JOBS[name] = dr.case_job(name)
    return _JOBS[name]


def _key(rows):
    return [(int(r[0]), int(r[1]), float(r[2]), float(r[3])) for r in rows]


# ---- the restatement against itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,chunk,seed", [(260, 180, 2000, 3), (300, 420, 300, 1)])
def test_identical_samples_give_the_one_sample_loops_and_no_differential_loop(n1, n2, chunk, seed):
    x, y, v = tr.synth_trans(n1, n2, density=0.35, nloops=8, seed=seed)
    rows = dr.diff_trans_rows((x, y, v), (x, y, v), 0.88, 0.2, 0.1, [1.6, 3.2], chunk=chunk)
    by = dr.rows_by_tag(rows)
    one = tr.trans_loops_normalized(x, y, tr.zscore_exact(v)[0], 0.88, 0.2, [1.6, 3.2], chunk=chunk)
    assert len(one) > 0
    assert _key(by[1]) == _key(by[3]) == _key(one)
    assert by[2] == [] and by[4] == []
    # and trans_loops itself (NumPy's mean and std instead of the exactly rounded ones): the same loops, q to rounding
    plain = tr.trans_loops(x, y, v, 0.88, 0.2, [1.6, 3.2], chunk=chunk)
    assert [r[:2] + [r[3]] for r in plain] == [r[:2] + [r[3]] for r in one]
    np.testing.assert_allclose([r[2] for r in plain], [r[2] for r in one], rtol=1e-9)


def test_swapping_the_samples_swaps_the_tags():
    rec1, rec2 = dr.synth_pair(420, 300, density=0.3, nloops=14, seed=7, added=5)
    a = dr.rows_by_tag(dr.diff_trans_rows(rec1, rec2, 0.88, 0.2, 0.1, [1.6, 3.2]))
    b = dr.rows_by_tag(dr.diff_trans_rows(rec2, rec1, 0.88, 0.2, 0.1, [1.6, 3.2]))
    assert len(a[1]) > 0 and len(a[3]) > 0 and len(a[2]) + len(a[4]) > 0
    assert _key(a[1]) == _key(b[3]) and _key(a[3]) == _key(b[1])
    assert _key(a[2]) == _key(b[4]) and _key(a[4]) == _key(b[2])


def test_one_tile_equals_the_cis_oracle_without_its_distance_fill():
    """oracle.diff.diff_block(intra=False) keeps the cis triangle mask (col - row >= 4) and the fill of 2 on col - row <= 4, which
    rule 4 drops.  Given the filled tiles and that mask, tile_pair is the same computation: everything after the masks -- both
    sigma loops, BH, the filters, D_2 of the difference image, norm.fit, the pair p-value, the differential subset -- must
    agree, and the clusterings agree because every tested pixel has x < y.  nz1 / nz2 exist for this test alone: it validates
    the pipeline behind the masks, under masks the trans rules never use; rule 4's own mask (c != 0) is held by the other tests."""
    import oracle
    rec1, rec2 = dr.synth_pair(330, 330, density=0.5, nloops=20, seed=11, added=6)
    z1, z2 = tr.zscore_exact(rec1[2])[0], tr.zscore_exact(rec2[2])[0]
    c1 = np.zeros((330, 330)); c1[rec1[0], rec1[1]] = z1
    c2 = np.zeros((330, 330)); c2[rec2[0], rec2[1]] = z2
    off = np.arange(330)[None, :] - np.arange(330)[:, None]
    nz1, nz2 = (c1 != 0) & (off >= 4), (c2 != 0) & (off >= 4)
    exp = oracle.diff_block(c1, c2, 0, 10 ** 6, [1.6, 3.2], 0.88, 0.2, 0.1, intra=False)      # fills c1, c2 in place
    assert (c1[off <= 4] == 2).all() and (c2[off <= 4] == 2).all()
    got = dr.tile_pair(c1, c2, 0.88, 0.2, 0.1, [1.6, 3.2], nz1=nz1, nz2=nz2)
    assert len(exp[0]) > 0 and len(exp[2]) > 0 and len(exp[1]) + len(exp[3]) > 0
    for g, e in zip(got, exp):
        assert _key(g) == _key(e)


def test_thresholds_apply_to_either_sample():
    rng = np.random.default_rng(5)
    big = np.where(rng.random((120, 120)) < 0.8, rng.normal(0.0, 1.0, (120, 120)), 0.0)
    small = big.copy()
    small[np.unravel_index(rng.choice(120 * 120, 120 * 120 - 9999, replace=False), (120, 120))] = 0.0
    assert (big != 0).sum() >= 10000 and (small != 0).sum() <= 9999
    assert dr.tile_pair(big, small, 0.88, 0.2, 0.1, [1.6, 3.2]) == ([], [], [], [])
    assert dr.tile_pair(small, big, 0.88, 0.2, 0.1, [1.6, 3.2]) == ([], [], [], [])


def test_an_empty_or_constant_sample_gives_no_rows():
    x, y, v = tr.synth_trans(80, 60, density=0.3, nloops=2, seed=1)
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    flat = (x, y, np.full(len(v), 3.0))
    for other in (none, flat):
        assert dr.diff_trans_rows((x, y, v), other, 0.88, 0.2, 0.1, [1.6, 3.2]) == []
        assert dr.diff_trans_rows(other, (x, y, v), 0.88, 0.2, 0.1, [1.6, 3.2]) == []


def test_two_sided_normal_handles_the_degenerate_fits():
    assert dr.two_sided_normal(0.0, 0.0, 0.0) == 0.0               # identical samples: z = NaN -> cdf 1 -> p 0
    assert dr.two_sided_normal(1.0, 0.0, 0.0) == 0.0
    assert dr.two_sided_normal(0.3, np.nan, np.nan) == 0.0         # nothing tested in both
    assert dr.two_sided_normal(0.0, 0.0, 1.0) == 1.0
    np.testing.assert_allclose(dr.two_sided_normal([-1.0, 1.0], 0.0, 1.0), [0.31731050786291415] * 2, rtol=1e-15)


def test_synth_pair_shares_background_and_given_blobs():
    (x1, y1, v1), (x2, y2, v2) = dr.synth_pair(200, 150, density=0.3, nloops=6, seed=3, blobs=[(100, 75, 2.0)])
    m1 = np.zeros((200, 150)); m1[x1, y1] = v1
    m2 = np.zeros((200, 150)); m2[x2, y2] = v2
    assert m1[199, 149] == 1.0 and m2[199, 149] == 1.0
    same = (m1 == m2).mean()
    assert 0.7 < same < 0.99                                       # ~ a quarter of the pixels drawn again, most of them empty twice
    assert m1[100, 75] >= 25.0 and m2[100, 75] >= 25.0


# ---- what the shared cases must offer -------------------------------------------------------------------------------------
def test_shared_cases_have_the_tilings_they_are_named_for():
    t = {n: tr.tiling(c["n1"], c["n2"], c["chunk"]) for n, c in dr.CASES.items()}
    assert [len(t["tiles_2x3"][k][0]) for k in (1, 2)] == [2, 3] and t["tiles_2x3"][0] == 600
    assert [len(t["tiles_6x6_sz2"][k][0]) for k in (1, 2)] == [6, 6] and t["tiles_6x6_sz2"][0] == 300
    assert t["production_2x2"][0] == 2000 and t["production_2x2"][1][0] == [0, 300] and t["production_2x2"][2][0] == [0, 100]


@pytest.mark.slow
@pytest.mark.parametrize("name", [n for n in dr.CASES if dr.CASES[n]["chunk"] < 2000])
def test_small_shared_cases_meet_their_conditions(name):
    rows, branches = _job(name)
    print(name, {t: len(v) for t, v in dr.rows_by_tag(rows).items()}, branches)
    dr.assert_case_conditions(name, rows)


@pytest.mark.slow
def test_small_shared_cases_take_every_v_other_branch():
    dr.assert_branches_covered([_job(n)[1] for n in dr.CASES if dr.CASES[n]["chunk"] < 2000])


@pytest.mark.slow
def test_production_shared_case_meets_its_conditions():
    rows, branches = _job("production_2x2")
    print({t: len(v) for t, v in dr.rows_by_tag(rows).items()}, branches)
    dr.assert_case_conditions("production_2x2", rows)


# ---- the command line's refusals ----------------------------------------------------------------------------------------
def _tiny_hic(path):
    chroms = [("All", 1000), ("1", 200000), ("2", 150000)]
    write_hic_pairs(str(path), chroms, {(1, 2): {10000: ([0, 1], [2, 3], [5.0, 6.0])}}, version=8)
    return str(path)


def _no_output(prefix):
    from mustache_amd.diff_mustache import SUFFIX
    import os
    return not any(os.path.exists(str(prefix) + suf) for suf in SUFFIX.values())


def test_cli_refuses_text_input_for_a_trans_pair(tmp_path, capsys):
    from mustache_amd.diff_mustache import main
    f = tmp_path / "contacts.txt"
    f.write_text("1\t10000\t2\t20000\t5\n")
    h = _tiny_hic(tmp_path / "p.hic")
    for f1, f2 in ((str(f), h), (h, str(f))):
        main(["-f1", f1, "-f2", f2, "-ch", "1", "-ch2", "2", "-r", "10kb", "-o", str(tmp_path / "o")])
        assert "Error: Interchromosomal analysis is only supported for .hic and .cool input formats." in capsys.readouterr().out
    assert _no_output(tmp_path / "o")


def test_cli_refuses_balance_with_a_trans_pair(tmp_path, capsys):
    from mustache_amd.diff_mustache import main
    a, b = _tiny_hic(tmp_path / "a.hic"), _tiny_hic(tmp_path / "b.hic")
    main(["-f1", a, "-f2", b, "-ch", "1", "-ch2", "2", "-r", "10kb", "-o", str(tmp_path / "o"), "--balance", "ICE"])
    assert "Error: --balance does not apply to inter-chromosomal pairs" in capsys.readouterr().out
    assert _no_output(tmp_path / "o")


def test_cli_refuses_a_trans_pair_in_a_multi_rank_run(tmp_path, capsys, monkeypatch):
    import mustache_amd.sharding as sh
    from mustache_amd.diff_mustache import main
    monkeypatch.setattr(sh, "init_from_env", lambda: (0, 2))
    a, b = _tiny_hic(tmp_path / "a.hic"), _tiny_hic(tmp_path / "b.hic")
    main(["-f1", a, "-f2", b, "-ch", "1", "-ch2", "2", "-r", "10kb", "-o", str(tmp_path / "o")])
    assert "Error: inter-chromosomal pairs run on one GPU only" in capsys.readouterr().out
    assert _no_output(tmp_path / "o")


def test_cli_refuses_ch2_without_ch(tmp_path, capsys, monkeypatch):
    import mustache_amd.readers as rd
    from mustache_amd.diff_mustache import main
    monkeypatch.setattr(rd, "list_chromosomes", lambda f, res: ["1"])
    a, b = _tiny_hic(tmp_path / "a.hic"), _tiny_hic(tmp_path / "b.hic")
    main(["-f1", a, "-f2", b, "-ch2", "2", "-r", "10kb", "-o", str(tmp_path / "o")])
    assert "Error: inter-chromosomal pairs need -ch and -ch2" in capsys.readouterr().out
    assert _no_output(tmp_path / "o")


def test_library_call_refuses_what_the_command_line_refuses(tmp_path):
    from mustache_amd.diff_mustache import regulator
    from mustache_amd.trans import TransError
    h = _tiny_hic(tmp_path / "p.hic")
    with pytest.raises(TransError):
        regulator("contacts.txt", h, False, False, "o", res=10000, chromosome="1", chromosome2="2")
    with pytest.raises(TransError):
        regulator(h, h, False, False, "o", res=10000, chromosome="1", chromosome2="2", balance="ICE")


def test_read_pair_still_refuses_a_trans_pair():
    from mustache_amd.diff_mustache import read_pair
    with pytest.raises(NotImplementedError):
        read_pair("a.hic", "b.hic", "KR", False, 10000, 2000000, False, False, "1", "2")
