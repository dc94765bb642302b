"""The host side of the all-pairs trans run without a GPU: the pair table and the arithmetic window rule against
trans_axis_tiles, the launch grouping, and the `--trans-all` pair enumeration with its refusals."""
import numpy as np
import pytest

GEOMETRIES = [(900, 1200, 600), (300, 500, 300), (605, 300, 300), (2300, 2100, 2000), (420, 300, 2000)]


def test_pair_table_agrees_with_the_tiling():
    from mustache_amd.trans import trans_tiling
    from mustache_amd.trans_genome import PAIR_DTYPE, pair_table
    assert PAIR_DTYPE.itemsize == 32 and PAIR_DTYPE.fields["tile_base"][1] == 24       # mst_trans_pair
    base = 0
    for n1, n2, chunk in GEOMETRIES:
        table, T = pair_table([None, (n1, n2), None, (n1, n2)], chunk)
        C, (rs, _), (cs, _) = trans_tiling(n1, n2, chunk)
        assert T == 2 * len(rs) * len(cs)
        assert [int(table[1][k]) for k in ("C", "K1", "K2", "n1", "n2", "tile_base")] == [C, len(rs), len(cs), n1, n2, 0]
        assert int(table[3]["tile_base"]) == len(rs) * len(cs)
        assert [int(table[p]["K1"]) * int(table[p]["K2"]) for p in (0, 2)] == [0, 0]
        assert int(table[2]["tile_base"]) == len(rs) * len(cs)                         # an untiled pair takes no index
        base += T
    assert base == 2 * (6 + 6 + 8 + 4 + 1)
    with pytest.raises(ValueError):
        pair_table([(600, 100)], 256)                                                  # windows of 256 cannot overlap by 256


def test_the_window_rule_names_exactly_the_windows_that_hold_a_coordinate():
    from mustache_amd.trans import trans_axis_tiles, trans_tiling
    from mustache_amd.trans_genome import window_start, windows_holding
    most = 0
    for n1, n2, chunk in GEOMETRIES:
        C = trans_tiling(n1, n2, chunk)[0]
        for n in (n1, n2):
            starts, _ = trans_axis_tiles(n, C)
            K = len(starts)
            assert [window_start(i, n, C, K) for i in range(K)] == starts
            for a in range(n):
                held = [i for i, s in enumerate(starts) if s <= a < s + C]
                assert windows_holding(a, n, C, K) == held, (n, C, a)
                most = max(most, len(held))
            assert windows_holding(-1, n, C, K) == [] and windows_holding(n, n, C, K) == []
    assert most == 7                                     # (605, 300, 300): bins 264 .. 299 lie in all seven regular windows


def test_launch_groups_are_runs_of_equal_tile_size_over_contiguous_pairs():
    from mustache_amd.trans_genome import launch_groups, pair_table
    # pairs: 2 x 3 tiles of 600, one tile of 420, untiled, 2 x 2 of 600, one of 420
    table, T = pair_table([(900, 1200), (420, 300), None, (900, 700), (300, 420)], 600)
    assert T == 12 and [int(c) for c in table["C"]] == [600, 420, 0, 600, 420]
    counts = np.array([10000, 9999, 20000, 10000, 0, 10001,   10000,   50000, 9999, 10000, 123456,   9999], np.uint32)
    assert launch_groups(table, counts, 64) == [([0, 2, 3, 5], 600, 0, 0), ([6], 420, 1, 1), ([7, 9, 10], 600, 3, 3)]
    assert launch_groups(table, counts, 3) == [([0, 2, 3], 600, 0, 0), ([5], 600, 0, 0), ([6], 420, 1, 1),
                                               ([7, 9, 10], 600, 3, 3)]
    # pair 1 wholly below the threshold: the tiles of 600 on both sides of it are consecutive kept tiles, one group over the
    # pair range 0 .. 3 (the scatter passes over the pairs of another tile size inside it)
    counts[6] = 9999
    assert launch_groups(table, counts, 64) == [([0, 2, 3, 5, 7, 9, 10], 600, 0, 3)]
    assert launch_groups(table, counts, 5) == [([0, 2, 3, 5, 7], 600, 0, 3), ([9, 10], 600, 3, 3)]
    assert launch_groups(table, np.zeros(T, np.uint32), 64) == []
    for tiles, C, p0, p1 in launch_groups(table, np.full(T, 10000, np.uint32), 4):
        assert 1 <= len(tiles) <= 4 and tiles == sorted(tiles) and p0 <= p1
        assert all(int(table[p]["C"]) == C for p in range(p0, p1 + 1) if any(
            int(table[p]["tile_base"]) <= t < int(table[p]["tile_base"]) + int(table[p]["K1"]) * int(table[p]["K2"]) for t in tiles))


def test_trans_all_pairs_and_refusals(monkeypatch, tmp_path, capsys):
    from mustache_amd import readers
    from mustache_amd.mustache import main, parse_args
    from mustache_amd.request import trans_all_pairs
    monkeypatch.setattr(readers, "list_chromosomes", lambda f, res: ["1", "2", "X"])
    assert trans_all_pairs("g.hic", 10000, 'n', 'n') == [("1", "2"), ("1", "X"), ("2", "X")]
    assert trans_all_pairs("g.mcool", 10000, None, 'n') == [("1", "2"), ("1", "X"), ("2", "X")]
    assert trans_all_pairs("g.cool", 10000, ["3", "1", "2"], 'n') == [("3", "1"), ("3", "2"), ("1", "2")]    # list order
    assert trans_all_pairs("g.hic", 10000, ["7"], 'n') == []
    assert trans_all_pairs("g.hic", 10000, ["1", "2"], ["2", "1"]) == \
        "Error: --trans-all pairs the -ch list with itself; give -ch2 without it"
    assert trans_all_pairs("g.txt", 10000, ["1", "2"], 'n') == \
        "Error: Interchromosomal analysis is only supported for .hic and .cool input formats."
    assert parse_args(["-o", "o", "-r", "10kb", "--trans-all"]).trans_all is True
    assert parse_args(["-o", "o", "-r", "10kb"]).trans_all is False
    # through main: the refusals print their line and write nothing
    f = tmp_path / "g.hic"
    f.write_bytes(b"")
    out = tmp_path / "o.tsv"
    for extra, line in ((["-ch", "1", "-ch2", "2"], "Error: --trans-all pairs the -ch list with itself; give -ch2 without it"),
                        (["--balance", "ICE"], "Error: --balance does not apply to inter-chromosomal pairs")):
        capsys.readouterr()
        main(["-f", str(f), "-r", "10kb", "--trans-all", "-o", str(out)] + extra)
        assert line in capsys.readouterr().out and not out.exists()
    t = tmp_path / "c.txt"
    t.write_text("10000\t20000\t3\n")
    main(["-f", str(t), "-r", "10kb", "--trans-all", "-o", str(out)])
    assert "Error: Interchromosomal analysis is only supported" in capsys.readouterr().out and not out.exists()
