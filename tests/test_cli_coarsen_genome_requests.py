"""What `mustache` refuses of --coarser-genome (mustache_amd/request.py, the rule `multires_genome`): one `Error:` line, no
output file and no GPU, through request.plan() and through mustache.main(argv), in the rule's order.  The inputs and the way of
asking are those of tests/test_cli_multires_requests.py.  No GPU."""
import gzip
import os

import pytest

from hic_trans_writer import write_hic_pairs

PAIRS = "## pairs format v1.0\n#chromsize: chr1 1000\n#chromsize: chr2 500\n" + \
        "".join("r\t%s\t%d\t%s\t%d\t+\t-\n" % r for r in [("chr1", 10, "chr1", 700), ("chr1", 20, "chr2", 30), ("chr2", 5, "chr2", 400)])


@pytest.fixture
def F(tmp_path, monkeypatch):
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    chroms = [("All", 1000), ("1", 200000), ("2", 150000)]
    write_hic_pairs(str(tmp_path / "a.hic"), chroms, {(1, 2): {10000: ([0, 1], [2, 3], [5.0, 6.0])}}, version=8)
    (tmp_path / "m.cool").write_bytes(b"")
    (tmp_path / "m.txt").write_text("1\t10000\t2\t20000\t5\n")
    (tmp_path / "m.pairs").write_text(PAIRS)
    (tmp_path / "m.pairs.gz").write_bytes(gzip.compress(PAIRS.encode()))
    t = str(tmp_path)
    return {"hic": t + "/a.hic", "cool": t + "/m.cool", "txt": t + "/m.txt", "p": t + "/m.pairs", "g": t + "/m.pairs.gz",
            "out": t + "/out"}


def C(name, files, extra, line, ranks=1):
    return pytest.param(files, extra.split(), line, ranks, id=name)


BOTH = "Error: --coarser-genome and --coarser: give one of them (--coarser coarsens each chromosome's own map, " \
       "--coarser-genome the whole genome's)"
NO_GENOME = "Error: --coarser-genome without --balance-genome: coarsening the genome's map sums raw integer counts; give " \
            "--balance-genome ICE|NEWTON"
ALONE = "Error: --merge-distance without --coarser: it is the tolerance of the multi-resolution merge and nothing else"
G = "--trans-all --balance-genome NEWTON "

# -r is 10kb for the .hic, text and .cool files and 100 for the pairs files
CASES = [
    # ---- 1. together with --coarser: before everything else of the rule
    C("both", "hic", G + "--coarser-genome 20kb --coarser 20kb", BOTH),
    C("both-no-genome", "hic", "-ch 1 --balance ICE --coarser 20kb --coarser-genome abc --merge-distance -1", BOTH),
    # ---- 2. without --balance-genome
    C("no-genome", "hic", "--trans-all --coarser-genome 20kb", NO_GENOME),
    C("no-genome-pair", "hic", "-ch 1 -ch2 2 --coarser-genome 20kb", NO_GENOME),
    C("no-genome-cis", "hic", "-ch 1 --balance ICE --coarser-genome 20kb", NO_GENOME),
    C("no-genome-before-distance", "hic", "--trans-all --coarser-genome abc --merge-distance -1", NO_GENOME),
    # ---- 3. a negative --merge-distance, before the resolutions are looked at
    C("distance-negative", "hic", G + "--coarser-genome abc --merge-distance -1",
      "Error: --merge-distance -1: the distance is a number of bins >= 0"),
    # ---- 4. a value that does not parse, is not greater than -r, is no multiple of it, or is given twice
    C("unparsable", "hic", G + "--coarser-genome 20kb abc",
      "Error: --coarser-genome abc: not a resolution (give base pairs, or a number with kb or mb)"),
    C("zero", "hic", G + "--coarser-genome 0", "Error: --coarser-genome 0: not a resolution (give base pairs, or a number with kb or mb)"),
    C("equal", "hic", G + "--coarser-genome 10000", "Error: --coarser-genome 10000: a coarser resolution is greater than -r (10000 bp)"),
    C("finer", "hic", "-ch 1 -ch2 2 --balance-genome ICE --coarser-genome 20kb 5kb",
      "Error: --coarser-genome 5kb: a coarser resolution is greater than -r (10000 bp)"),
    C("no-multiple", "hic", G + "--coarser-genome 25kb", "Error: --coarser-genome 25kb: 25000 bp is not an integer multiple of -r (10000 bp)"),
    C("no-multiple-pairs", "g", G + "--pairs-trans --coarser-genome 200 250",
      "Error: --coarser-genome 250: 250 bp is not an integer multiple of -r (100 bp)"),
    C("twice", "hic", G + "--coarser-genome 20kb 50kb 20000", "Error: --coarser-genome 20000: 20000 bp is given twice"),
    # ---- --merge-distance alone keeps the sentence of --coarser
    C("distance-alone", "hic", G + "--merge-distance 1", ALONE),
    C("distance-alone-cis", "hic", "-ch 1 --balance ICE --merge-distance 0", ALONE),
    # ---- what --balance-genome itself refuses keeps its own sentence
    C("not-all-trans", "hic", "-ch 1 1 -ch2 1 2 --balance-genome ICE --coarser-genome 20kb",
      "Error: --balance-genome is for inter-chromosomal calls; use --balance"),
    C("cis-run", "hic", "-ch 1 --balance-genome ICE --coarser-genome 20kb",
      "Error: --balance-genome is for inter-chromosomal calls; use --balance"),
    C("text", "txt", "-ch 1 -ch2 2 --balance-genome ICE --coarser-genome 20kb",
      "Error: Interchromosomal analysis is only supported for .hic and .cool input formats."),
    C("cool", "cool", "-ch 1 -ch2 2 --balance-genome ICE --coarser-genome 20kb",
      "Error: --balance-genome ICE and {cool}: .cool/.mcool files carry their own `weight` column; --balance-genome is for .hic input"),
    C("ranks", "hic", G + "-ch 1 2 --coarser-genome 20kb", "Error: inter-chromosomal pairs run on one GPU only (this run has 2 ranks)", ranks=2),
    C("pairs-without-pairs-trans", "p", G + "--coarser-genome 200",
      "Error: --trans-all and {p}: without --pairs-trans only intra-chromosomal loops are called from a pairs file"),
]


def _argv(F, files, extra):
    return ["-f", F[files], "-r", "10kb" if files in ("hic", "txt", "cool") else "100", "-o", F["out"]] + [e.format(**F) for e in extra]


@pytest.mark.parametrize("files,extra,line,ranks", CASES)
def test_the_refusal_and_no_output_file(F, capsys, monkeypatch, files, extra, line, ranks):
    from mustache_amd import mustache, pairs, sharding
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, ranks))
    want = line.format(**F)
    capsys.readouterr()
    try:
        mustache.main(_argv(F, files, extra))
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    said = capsys.readouterr().out.splitlines()
    print("\n".join(said))
    assert said.count(want) == 1 and sum(ln.startswith("Error:") for ln in said) == 1, said
    assert not os.path.exists(F["out"])


@pytest.mark.parametrize("files,extra,line,ranks", CASES)
def test_the_same_line_from_plan(F, files, extra, line, ranks):
    """request.plan() on the Request the command line builds: the same sentence, as a return value"""
    from mustache_amd import mustache, pairs
    from mustache_amd.request import plan, request_of
    args = mustache.parse_args(_argv(F, files, extra))
    try:
        got = plan(request_of(args, [args.f_path], [(args.biasfile, "")], "-b", ranks), mustache.parseBP(args.resolution))
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    assert got == line.format(**F)


def test_the_order_of_the_rule():
    """multires_genome on bare requests: the four refusals fire in the stated order, each masking the later ones"""
    from mustache_amd.request import Request, multires, multires_genome

    def rq(**kw):
        balance_genome = kw.pop("balance_genome", "NEWTON")
        return Request(["a.hic"], [(None, "")], "-b", False, None, balance_genome, "all", False, False, False, True, ["1", "2"], 'n', 1,
                       False, **kw)
    bad = dict(coarser_genome=["abc"], merge_distance=-1)
    assert multires_genome(rq(), 10000) is None and multires(rq(), 10000) is None
    assert "Error: " + multires_genome(rq(coarser=["20kb"], balance_genome=None, **bad), 10000) == BOTH
    assert "Error: " + multires_genome(rq(balance_genome=None, **bad), 10000) == NO_GENOME
    assert multires_genome(rq(**bad), 10000) == "--merge-distance -1: the distance is a number of bins >= 0"
    assert multires_genome(rq(coarser_genome=["abc"], merge_distance=0), 10000).startswith("--coarser-genome abc: not a resolution")
    assert multires_genome(rq(coarser_genome=["20kb"], merge_distance=0), 10000) is None
    # --merge-distance alone: multires()'s sentence, verbatim, only when NEITHER flag is given
    assert "Error: " + multires(rq(merge_distance=1), 10000) == ALONE
    assert multires(rq(coarser_genome=["20kb"], merge_distance=1), 10000) is None


def test_parse_resolutions_names_the_flag():
    from mustache_amd.multires import MultiresError, parse_resolutions
    assert parse_resolutions(10000, ["50kb", "20kb"], flag="--coarser-genome") == [20000, 50000]
    with pytest.raises(MultiresError, match=r"^--coarser 15kb: 15000 bp is not an integer multiple of -r \(10000 bp\)$"):
        parse_resolutions(10000, ["15kb"])
    with pytest.raises(MultiresError, match=r"^--coarser-genome 15kb: 15000 bp is not an integer multiple"):
        parse_resolutions(10000, ["15kb"], flag="--coarser-genome")


def test_a_legal_request_reaches_the_plan(F):
    from mustache_amd import diff_mustache, mustache, pairs
    from mustache_amd.request import Plan, Request, coarser_genome_resolutions, coarser_resolutions, plan, request_of
    # behind the tuple, by keyword, with a default: a positional caller keeps working
    rq = Request([F["hic"]], [(None, "")], "-b", False, None, "ICE", "all", False, False, False, True, ["1", "2"], 'n', 1, False)
    assert rq.coarser_genome is None and coarser_genome_resolutions(rq, 10000) == [] and "coarser_genome" in Request.EXTRA
    assert rq._replace(ranks=1).coarser_genome is None
    assert rq._replace(coarser_genome=["20kb"]).coarser_genome == ["20kb"]
    assert mustache.parse_args(["-o", "x", "-r", "10kb"]).coarser_genome is None
    assert not hasattr(diff_mustache.parse_args(["-o", "x", "-r", "10kb"]), "coarser_genome")
    with pytest.raises(SystemExit):
        diff_mustache.parse_args(["-o", "x", "-r", "10kb", "--coarser-genome", "20kb"])
    for extra, want in ((["--coarser-genome", "20kb"], [20000]), (["--coarser-genome", "50kb", "20000", "--merge-distance", "0"], [20000, 50000]),
                        (["--coarser-genome", "1mb", "--downsample-genome", "0.5", "--seed", "3", "--balance-pixels", "inter"], [1000000])):
        pixels = "inter" if "inter" in extra else "all"
        for run, pairs_of in ((["--trans-all", "-ch", "1", "2"], [("1", "2")]), (["-ch", "2", "-ch2", "1"], [("2", "1")])):
            args = mustache.parse_args(["-f", F["hic"], "-o", F["out"], "-r", "10kb", "--balance-genome", "newton"] + run + extra)
            rq = request_of(args, [F["hic"]], [(None, "")], "-b", 1)
            assert plan(rq, 10000) == Plan([], pairs_of, "--trans-all" in run, None, ("NEWTON", pixels))
            assert coarser_genome_resolutions(rq, 10000) == want and coarser_resolutions(rq, 10000) == []
            assert rq._replace(ranks=2).coarser_genome == rq.coarser_genome
    # a pairs file under --pairs-trans: its one parse happens in plan(), and the request goes ahead
    args = mustache.parse_args(["-f", F["p"], "-o", F["out"], "-r", "100", "--trans-all", "--pairs-trans", "--balance-genome", "ICE",
                                "--coarser-genome", "200", "500"])
    rq = request_of(args, [F["p"]], [(None, "")], "-b", 1)
    try:
        assert plan(rq, 100) == Plan([], [("chr1", "chr2")], True, None, ("ICE", "all"))
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    assert coarser_genome_resolutions(rq, 100) == [200, 500]
    assert not os.path.exists(F["out"])
