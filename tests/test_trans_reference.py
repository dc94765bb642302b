"""Inter-chromosomal pairs without a GPU: the tiling and ownership of rule 3 (mustache_amd/trans.py) against the restatement
(tests/trans_reference.py), the z-score rules, the restatement's clustering on tiles where x > y, and the command line's
refusals (rule 7 and text input)."""
import numpy as np
import pytest

import trans_reference as tr
from hic_trans_writer import expected_trans, write_hic_pairs


@pytest.mark.parametrize("n1,n2", [(4100, 2300), (2300, 4100), (2001, 3745), (5231, 1999), (1500, 700), (2000, 2000),
                                   (3744, 2257)])
def test_every_pixel_is_owned_by_exactly_one_tile(n1, n2):
    from mustache_amd.trans import trans_tiling
    own, held = tr.ownership_counts(n1, n2)
    assert (own == 1).all()
    assert (held >= 1).all()
    C, rows, cols = trans_tiling(n1, n2)
    Cr, rows_r, cols_r = tr.tiling(n1, n2)
    assert (C, rows, cols) == (Cr, rows_r, cols_r)
    assert C == min(2000, max(n1, n2))
    for starts, ends, n in ((rows[0], rows[1], n1), (cols[0], cols[1], n2)):
        assert ends[-1] == n and starts[0] == 0
        for i, (s, e) in enumerate(zip(starts, ends)):
            lo = ends[i - 1] if i else 0
            assert s <= lo and e <= s + C                     # the owned range lies inside the tile's window


def test_axis_with_n_at_most_c_has_one_tile():
    from mustache_amd.trans import trans_axis_tiles, trans_tiling
    assert trans_axis_tiles(700, 2000) == ([0], [700])
    C, rows, cols = trans_tiling(1500, 700)
    assert C == 1500 and rows == ([0], [1500]) and cols == ([0], [700])
    C, rows, cols = trans_tiling(2300, 700)
    assert C == 2000 and len(rows[0]) == 2 and cols == ([0], [700])


def test_zscore_rules():
    v = np.array([1.0, 2.0, 4.0, 8.0])
    z, mean, std = tr.zscore(v)
    assert mean == 3.75 and std == np.std(v)
    np.testing.assert_allclose(z, (v - 3.75) / np.std(v), rtol=0, atol=0)
    assert tr.zscore(np.zeros(0)) is None
    z, _, std = tr.zscore(np.full(5, 3.0))                   # std = 0: every v' is NaN -> 0, and the pair yields no loops
    assert std == 0 and (z == 0).all()
    assert tr.trans_loops(np.arange(5), np.arange(5), np.full(5, 3.0), 0.88, 0.2, [1.6, 3.2]) == []
    assert tr.trans_loops(np.zeros(0, int), np.zeros(0, int), np.zeros(0), 0.88, 0.2, [1.6, 3.2]) == []


def test_clustering_works_below_the_diagonal_and_never_wraps():
    o = np.ones((12, 10))
    # candidates with x > y, in column 0 and in the last column of the same rows: the reference's label matrix would wrap
    # column -1 onto its last column and join them
    cand = [(6, 0), (6, 9), (10, 5), (11, 7)]
    q = [0.01, 0.02, 0.05, 0.03]
    for (x, y), qq in zip(cand, q):
        o[x, y] = qq
    o[7, 1] = 0.005                                          # a selected non-candidate inside the first halo wins its component
    cx = np.array([c[0] for c in cand])
    cy = np.array([c[1] for c in cand])
    reps = tr.cluster(o, cx, cy)
    # (10, 5) and (11, 7) are 2 columns apart: their halos touch -> one component, represented by the lower q (11, 7), whose
    # halo is clipped at the last row
    assert sorted(reps) == [(6, 9), (7, 1), (11, 7)]


def test_clustering_ties_go_to_the_first_pixel_in_row_major_order():
    o = np.ones((8, 8))
    o[3, 5] = o[4, 4] = 0.01
    reps = tr.cluster(o, np.array([3, 4]), np.array([5, 4]))
    assert reps == [(3, 5)]


def test_restatement_finds_loops_on_a_rectangular_map():
    x, y, v = tr.synth_trans(260, 180, density=0.35, nloops=6, seed=3)
    loops = tr.trans_loops(x, y, v, 0.88, 0.2, [1.6, 3.2])
    assert loops, "the synthetic map should hold loops"
    assert [(a, b) for a, b, _, _ in loops] == sorted((a, b) for a, b, _, _ in loops)
    assert all(0 <= a < 260 and 0 <= b < 180 for a, b, _, _ in loops)


def _synth_trans_whole_map(n1, n2, density=0.3, nloops=12, seed=0):
    """synth_trans as it was first written: every blob evaluated over the whole map"""
    rng = np.random.default_rng(seed)
    m = np.where(rng.random((n1, n2)) < density, np.exp(rng.normal(0.0, 0.5, (n1, n2))), 0.0)
    gx, gy = np.mgrid[0:n1, 0:n2]
    for _ in range(nloops):
        cx, cy = rng.integers(8, n1 - 8), rng.integers(8, n2 - 8)
        s = rng.uniform(1.2, 3.0)
        blob = 25.0 * np.exp(-((gx - cx) ** 2 + (gy - cy) ** 2) / (2 * s * s))
        m = np.where(blob > 0.5, m + blob, m)
    m[n1 - 1, n2 - 1] = 1.0
    x, y = np.nonzero(m > 0)
    return x.astype(np.int64), y.astype(np.int64), m[x, y]


@pytest.mark.parametrize("n1,n2,density,nloops,seed", [(260, 180, 0.35, 6, 3), (97, 310, 0.05, 40, 8), (420, 300, 0.3, 10, 1),
                                                       (40, 40, 0.0, 30, 5)])
def test_windowed_synth_trans_draws_the_same_map(n1, n2, density, nloops, seed):
    a = tr.synth_trans(n1, n2, density=density, nloops=nloops, seed=seed)
    b = _synth_trans_whole_map(n1, n2, density=density, nloops=nloops, seed=seed)
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and np.array_equal(p, q)
    # given blobs come after the random ones and reach the map's edge
    x, y, v = tr.synth_trans(60, 50, density=0.0, nloops=0, seed=0, blobs=[(0, 49, 2.0)])
    m = np.zeros((60, 50))
    m[x, y] = v
    assert m[0, 49] == 25.0 and m[1, 48] == 25.0 * np.exp(-2 / 8.0) and m[59, 49] == 1.0 and np.count_nonzero(m) == len(v)


def test_zscore_exact_is_pinned_by_rational_arithmetic():
    import math
    from fractions import Fraction
    rng = np.random.default_rng(12)
    cases = [[1.0, 2.0, 4.0, 8.0], [0.1] * 10, [1e16, 1.0, -1e16, 1.0], [2.0 ** -1074, 2.0 ** -1074 * 3, 2.0 ** -1060],
             [2.0 ** 64, 2.0 ** 11, 1e-300], [2.0 ** 64, 2.0 ** 11, -1e-300], [2.0 ** 64 + 2.0 ** 12, 2.0 ** 11, 0.0],
             [1e8 + 2.0 ** -20, 1e8 - 2.0 ** -21, 1e8], [-3.5, 2.25, -1e-5, 7.0, 1e5]]
    cases += [list(rng.uniform(-1, 1, int(rng.integers(1, 12))) * 2.0 ** rng.integers(-300, 300)) for _ in range(200)]
    cases += [list(rng.uniform(0, 1, 5) * 2.0 ** rng.integers(-60, 60, 5).astype(np.float64)) for _ in range(200)]
    for v in cases:
        v = np.array(v, np.float64)
        assert math.fsum(v.tolist()) == float(sum(Fraction(a) for a in v.tolist()))
        z, mean, std = tr.zscore_exact(v)
        # the squares (d * d in float64) are rounded, as in the kernel; their sum is not
        d = v - np.float64(mean)
        sq = d * d
        m_ref = float(sum(Fraction(a) for a in v.tolist())) / len(v)
        s_ref = math.sqrt(float(sum(Fraction(a) for a in sq.tolist())) / len(v))
        assert mean == m_ref and std == s_ref
        if std > 0:
            assert np.array_equal(z, d / std)
    assert tr.zscore_exact(np.zeros(0)) is None
    z, mean, std = tr.zscore_exact([1.0, np.inf, 2.0])
    assert np.isnan(mean) and np.isnan(std) and (z == 0).all()
    z, mean, std = tr.zscore_exact([1e200, -1e200, 3.0])                  # a square overflows: std NaN, mean kept
    assert mean == 1.0 and np.isnan(std) and (z == 0).all()
    # the tie cases the device test relies on: to even both ways, tie + tiny up
    assert math.fsum([2.0 ** 64, 2.0 ** 11]) == 2.0 ** 64 and math.fsum([2.0 ** 64, 2.0 ** 11, 1e-300]) == 2.0 ** 64 + 2.0 ** 12
    assert math.fsum([2.0 ** 64 + 2.0 ** 12, 2.0 ** 11]) == 2.0 ** 64 + 2.0 ** 13
    # and it agrees with the NumPy form of rule 2 to rounding
    v = np.exp(rng.normal(0.0, 1.5, 5000))
    z, mean, std = tr.zscore_exact(v)
    zn, mn, sn = tr.zscore(v)
    assert abs(mean - mn) <= 1e-12 * mn and abs(std - sn) <= 1e-12 * sn
    np.testing.assert_allclose(z, zn, rtol=0, atol=1e-12)


@pytest.mark.slow
def test_smallest_production_case_meets_its_conditions():
    """C = 2000, 2 x 2 tiles: the restatement alone returns loops, >= 5 in an overlap strip, >= 1 owned by the last tile"""
    name = "sparse_2x2"
    c = tr.PRODUCTION_CASES[name]
    C, (rs, re), (cs, ce) = tr.tiling(c["n1"], c["n2"])
    assert C == 2000 and len(rs) == 2 and len(cs) == 2
    x, y, v = tr.production_records(name)
    per_tile = [int(((x >= r) & (x < r + C) & (y >= q) & (y < q + C)).sum()) for r in rs for q in cs]
    assert all(10000 <= k < 11000 for k in per_tile), per_tile      # every tile just above rule 4's second threshold
    loops = tr.production_job(name)
    tr.assert_production_conditions(name, loops)
    assert tr.overlap_strips(rs, re) == [(300, 2000)] and tr.overlap_strips(cs, ce) == [(100, 2000)]


def test_production_cases_have_the_tilings_they_are_named_for():
    for name, c in tr.PRODUCTION_CASES.items():
        C, (rs, re), (cs, ce) = tr.tiling(c["n1"], c["n2"])
        assert C == 2000, name
    t = {n: tr.tiling(c["n1"], c["n2"]) for n, c in tr.PRODUCTION_CASES.items()}
    assert t["short_long_2x2"][1][0] == [0, 1700] and t["short_long_2x2"][2][0] == [0, 300]
    assert t["three_rows_oc3"][1][0] == [0, 1744, 1900] and t["three_rows_oc3"][2][0] == [0, 200]
    assert t["dense_2x2"][1][0] == [0, 100] and t["dense_2x2"][2][0] == [0, 50]


def test_expected_trans_reading_transposes_and_filters():
    x, y, c = expected_trans([0, 1, 2], [3, 0, 1], [2.0, 0.0, 5.0], np.array([1.0, 2.0, 0.5]), np.array([1.0, 0.5, 2.0, 4.0]))
    assert list(x) == [0, 2] and list(y) == [3, 1]           # the zero count is dropped, rows sorted by (x, y)
    np.testing.assert_array_equal(c, [0.5, 20.0])


# ---- the command line's refusals ----------------------------------------------------------------------------------------
def _tiny_hic(path):
    chroms = [("All", 1000), ("1", 200000), ("2", 150000)]
    write_hic_pairs(str(path), chroms, {(1, 2): {10000: ([0, 1], [2, 3], [5.0, 6.0])}}, version=8)
    return str(path)


def test_cli_text_input_keeps_its_refusal(tmp_path, capsys):
    from mustache_amd.mustache import main
    f = tmp_path / "contacts.txt"
    f.write_text("1\t10000\t2\t20000\t5\n")
    with pytest.raises(FileNotFoundError):
        main(["-f", str(f), "-ch", "1", "-ch2", "2", "-r", "10kb", "-o", str(tmp_path / "o.tsv")])
    assert "Interchromosomal analysis is only supported for .hic and .cool input formats." in capsys.readouterr().out


def test_cli_refuses_balance_with_a_trans_pair(tmp_path, capsys):
    from mustache_amd.mustache import main
    f = _tiny_hic(tmp_path / "p.hic")
    out = tmp_path / "o.tsv"
    main(["-f", f, "-ch", "1", "-ch2", "2", "-r", "10kb", "-o", str(out), "--balance", "ICE"])
    assert "Error: --balance does not apply to inter-chromosomal pairs" in capsys.readouterr().out
    assert not out.exists()


def test_cli_refuses_a_trans_pair_in_a_multi_rank_run(tmp_path, capsys, monkeypatch):
    import mustache_amd.sharding as sh
    from mustache_amd.mustache import main
    monkeypatch.setattr(sh, "init_from_env", lambda: (0, 2))
    f = _tiny_hic(tmp_path / "p.hic")
    out = tmp_path / "o.tsv"
    main(["-f", f, "-ch", "1", "-ch2", "2", "-r", "10kb", "-o", str(out)])
    assert "Error: inter-chromosomal pairs run on one GPU only" in capsys.readouterr().out
    assert not out.exists()


def test_cli_refuses_all_pairs_without_ch(tmp_path, capsys, monkeypatch):
    import mustache_amd.readers as rd
    from mustache_amd.mustache import main
    monkeypatch.setattr(rd, "list_chromosomes", lambda f, res: ["1"])
    f = _tiny_hic(tmp_path / "p.hic")
    out = tmp_path / "o.tsv"
    main(["-f", f, "-ch2", "2", "-r", "10kb", "-o", str(out)])
    assert "Error: inter-chromosomal pairs need -ch and -ch2" in capsys.readouterr().out
    assert not out.exists()


def test_diff_mustache_keeps_refusing_trans_pairs():
    from mustache_amd.diff_mustache import read_pair
    with pytest.raises(NotImplementedError):
        read_pair("a.hic", "b.hic", "KR", False, 10000, 2000000, False, False, "1", "2")


def test_io_library_exports_the_trans_read():
    import ctypes
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "mustache_amd", "libmustache_io.so"))
    names = set(re.findall(r"\b(mst_hic_\w+)\s*\(", open(os.path.join(root, "include", "mustache_io_trans.h")).read()))
    assert names == {"mst_hic_rawstream_open_trans", "mst_hic_rawstream_info_trans"}
    for n in names:
        assert hasattr(lib, n), n


def test_the_trans_raw_stream_refuses_one_chromosome_and_unknown_names(tmp_path):
    from mustache_amd.hicfile import HicError, HicFile, HicTransRawStream
    import ctypes
    f = _tiny_hic(tmp_path / "p.hic")
    mem = ctypes.create_string_buffer(4 * 8192 + 16)
    base = (ctypes.addressof(mem) + 15) // 16 * 16
    with HicFile(f) as h:
        with pytest.raises(HicError):
            HicTransRawStream(h, "1", "1", 10000, "NONE", base, 4, 8192)
        with pytest.raises(HicError):
            HicTransRawStream(h, "1", "7", 10000, "NONE", base, 4, 8192)
        st = HicTransRawStream(h, "2", "1", 10000, "NONE", base, 4, 8192)
        assert st.transposed
        na, nb, la, lb = st.info()
        assert na is None and nb is None and (la, lb) == (150000, 200000)
        rows = 0
        while True:
            got = st.next(-1)
            if got is False:
                break
            if got:
                rows += got[2]
                st.release(got[0])
        st.close()
        assert rows == 2 and st.blocks_total == 1
