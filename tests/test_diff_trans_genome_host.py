"""The host side of the two-sample all-pairs trans run without a GPU: the `--trans-all` flag of diff_mustache with its
refusals, the joint pair table of two samples' extents, and the keep rule on two count vectors."""
import numpy as np

SUFFIXES = (".loop1", ".diffloop1", ".loop2", ".diffloop2")


def test_the_flag_parses_and_defaults_to_false():
    from mustache_amd.diff_mustache import parse_args
    assert parse_args(["-o", "o", "-r", "10kb", "--trans-all"]).trans_all is True
    assert parse_args(["-o", "o", "-r", "10kb"]).trans_all is False


def test_refusals_print_their_line_and_write_no_file(monkeypatch, tmp_path, capsys):
    from mustache_amd import readers, sharding
    from mustache_amd.diff_mustache import main
    import mustache_amd.diff_trans_genome                                   # noqa: F401  (the module the run drives)
    monkeypatch.setattr(readers, "list_chromosomes", lambda f, res: ["1", "2", "X"])
    hic1, hic2, text = tmp_path / "a.hic", tmp_path / "b.hic", tmp_path / "c.txt"
    hic1.write_bytes(b"")
    hic2.write_bytes(b"")
    text.write_text("10000\t20000\t3\n")
    out = str(tmp_path / "o")
    fmt = "Error: Interchromosomal analysis is only supported for .hic and .cool input formats."
    cases = [
        ((hic1, hic2), ["-ch", "1", "-ch2", "2"], "Error: --trans-all pairs the -ch list with itself; give -ch2 without it"),
        ((text, hic2), [], fmt),
        ((hic1, text), [], fmt),                                            # the second file passes the same check
        ((hic1, text), ["-ch", "1", "2"], fmt),
        ((hic1, hic2), ["--balance", "ICE"], "Error: --balance does not apply to inter-chromosomal pairs"),
    ]
    for (f1, f2), extra, line in cases:
        capsys.readouterr()
        main(["-f1", str(f1), "-f2", str(f2), "-r", "10kb", "--trans-all", "-o", out] + extra)
        said = capsys.readouterr().out.splitlines()
        assert said.count(line) == 1 and sum(ln.startswith("Error:") for ln in said) == 1, (extra, said)
        assert not any((tmp_path / ("o" + suf)).exists() for suf in SUFFIXES)
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))
    capsys.readouterr()
    main(["-f1", str(hic1), "-f2", str(hic2), "-r", "10kb", "--trans-all", "-o", out])
    said = capsys.readouterr().out.splitlines()
    assert said.count("Error: inter-chromosomal pairs run on one GPU only (this run has 2 ranks)") == 1
    assert sum(ln.startswith("Error:") for ln in said) == 1
    assert not any((tmp_path / ("o" + suf)).exists() for suf in SUFFIXES)


def test_the_request_names_the_pairs_of_the_first_file_in_order(monkeypatch, tmp_path):
    from mustache_amd import readers
    from mustache_amd.request import Request, plan
    for name in ("a.hic", "b.hic", "b.mcool", "b.txt"):
        (tmp_path / name).write_bytes(b"")

    def trans_all_request(f1, f2, res, ch, ch2, balance, world_size):
        """the two-sample --trans-all request through request.plan(): the pairs, or the Error: line"""
        run = plan(Request(files=[str(tmp_path / f1), str(tmp_path / f2)], bias=[(None, ""), (None, "")], bias_flag="-b1/-b2",
                           norm_method=False, balance=balance, balance_genome=None, balance_pixels="all",
                           balance_pixels_given=False, pairs_trans=False, pairs_zero_based=False, trans_all=True, ch=ch, ch2=ch2,
                           ranks=world_size, text_pair_raises=False), res)
        return run if isinstance(run, str) else run.trans
    monkeypatch.setattr(readers, "list_chromosomes", lambda f, res: ["1", "2", "X"] if f.endswith("a.hic") else ["9"])
    assert trans_all_request("a.hic", "b.mcool", 10000, 'n', 'n', None, 1) == [("1", "2"), ("1", "X"), ("2", "X")]
    assert trans_all_request("a.hic", "b.hic", 10000, ["3", "1", "2"], 'n', None, 1) == [("3", "1"), ("3", "2"), ("1", "2")]
    assert trans_all_request("a.hic", "b.hic", 10000, ["7"], 'n', None, 1) == []
    # a run that is refused reads no chromosome list
    def never(f, res):
        raise AssertionError("a refused run read %s" % f)
    monkeypatch.setattr(readers, "list_chromosomes", never)
    assert trans_all_request("a.hic", "b.txt", 10000, 'n', 'n', None, 1).startswith("Error: Interchromosomal analysis")
    assert trans_all_request("a.hic", "b.hic", 10000, 'n', 'n', "ICE", 1) == "Error: --balance does not apply to inter-chromosomal pairs"
    assert trans_all_request("a.hic", "b.hic", 10000, 'n', 'n', None, 4).endswith("(this run has 4 ranks)")
    assert trans_all_request("a.hic", "b.hic", 10000, ["1"], ["2"], None, 1).startswith("Error: --trans-all pairs the -ch list")


def test_the_joint_pair_table_is_the_table_of_the_maxima():
    from mustache_amd.trans_genome import joint_dims, pair_table
    # pair 0: sample 1 supplies n1 (900 > 640), sample 2 supplies n2 (1200 > 1100); pair 1: a sample with nothing to tile;
    # pair 2: sample 2 supplies both; pair 3: equal
    a = [(900, 1100), (300, 300), (100, 200), (420, 300)]
    b = [(640, 1200), None, (650, 700), (420, 300)]
    dims = joint_dims([a, b])
    assert dims == [(900, 1200), None, (650, 700), (420, 300)]
    assert joint_dims([b, a]) == dims
    assert joint_dims([[None, (5, 6)], [(1, 2), (7, 3)]]) == [None, (7, 6)]
    assert joint_dims([a]) == a                                             # one sample: its own dimensions
    table, T = pair_table(dims, 600)
    want, T_want = pair_table([(900, 1200), None, (650, 700), (420, 300)], 600)
    assert T == T_want == 6 + 0 + 4 + 1 and table.tobytes() == want.tobytes()
    assert [int(table[0][k]) for k in ("C", "K1", "K2", "n1", "n2")] == [600, 2, 3, 900, 1200]
    # neither sample alone gives pair 0's table
    assert pair_table([a[0]], 600)[0].tobytes() != table[:1].tobytes() != pair_table([b[0]], 600)[0].tobytes()


def test_a_tile_pair_is_kept_when_the_smaller_count_reaches_ten_thousand():
    from mustache_amd.trans_genome import TRANS_MIN_TESTED, joint_counts, launch_groups, pair_table
    assert TRANS_MIN_TESTED == 10000
    table, T = pair_table([(900, 1200), (420, 300)], 600)
    assert T == 7
    c1 = np.array([10000, 9999, 10000, 9999, 50000, 10000, 123456], np.uint32)
    c2 = np.array([10000, 10000, 9999, 9999, 10000, 0, 10001], np.uint32)
    joint = joint_counts([c1, c2])
    assert joint.tolist() == [10000, 9999, 9999, 9999, 10000, 0, 10001] and joint_counts([c2, c1]).tolist() == joint.tolist()
    assert joint_counts([c1]).tolist() == c1.tolist()
    # 10 000 / 10 000 kept; 9 999 on either side or both dropped; 0 on one side dropped
    assert launch_groups(table, joint, 32) == [([0, 4], 600, 0, 0), ([6], 420, 1, 1)]
    kept = [t for g in launch_groups(table, joint, 1) for t in g[0]]
    assert kept == [0, 4, 6] == np.nonzero(np.minimum(c1, c2) >= 10000)[0].tolist()


def test_the_two_sample_launch_is_priced_from_its_shapes():
    from mustache_amd.diff_trans import tile_pair_bytes
    # two float64 tiles, two byte masks, D_2 per octave: 136 MB at C = 2000 and two octaves
    assert tile_pair_bytes(2000, 2) == 2 * 32_000_000 + 2 * 4_000_000 + 2 * 32_000_000 == 136_000_000
    assert tile_pair_bytes(1, 2) == 34 and tile_pair_bytes(600, 3) == (16 + 2 + 24) * 360000
