"""What both command lines refuse of --downsample-genome / --match-depth-genome (mustache_amd/request.py, the rule
`thinning_genome`): one `Error:` line, no output file and no GPU, through request.plan() and through mustache.main(argv) /
diff_mustache.main(argv).  The inputs and the way of asking are those of tests/test_cli_downsample_requests.py.  No GPU."""
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
    for name in ("a.hic", "b.hic"):
        write_hic_pairs(str(tmp_path / name), chroms, {(1, 2): {10000: ([0, 1], [2, 3], [5.0, 6.0])}}, version=8)
    (tmp_path / "m.cool").write_bytes(b"")
    (tmp_path / "m.txt").write_text("1\t10000\t2\t20000\t5\n")
    (tmp_path / "m.pairs").write_text(PAIRS)
    (tmp_path / "m.pairs.gz").write_bytes(gzip.compress(PAIRS.encode()))
    t = str(tmp_path)
    return {"hic": t + "/a.hic", "hic2": t + "/b.hic", "cool": t + "/m.cool", "txt": t + "/m.txt", "p": t + "/m.pairs",
            "g": t + "/m.pairs.gz", "out": t + "/out"}


def C(name, cli, files, extra, line):
    return pytest.param(cli, files, extra.split(), line, id="%s-%s" % (cli, name))


NEED = "Error: %s without --balance-genome: thinning the genome's map needs raw integer counts; give --balance-genome ICE|NEWTON"
BOTH = "Error: --match-depth-genome and --downsample-genome: give one of them (--match-depth-genome thins the deeper sample's " \
       "genome to the other's depth)"
MIXED = "Error: {0} and {1}: give one of them ({0} thins each chromosome's own map, {1} the whole genome's)"
FRACTION = "Error: --downsample-genome %s: the fraction to keep must lie strictly between 0 and 1"
SEED = "Error: --seed %s: the seed is a 32-bit unsigned integer (0 .. 4294967295)"
G = "--trans-all --balance-genome NEWTON "

CASES = [
    # ---- without --balance-genome: the genome thinning needs raw integer counts
    C("no-balance-genome", "m", ("hic",), "--trans-all --downsample-genome 0.5", NEED % "--downsample-genome"),
    C("no-balance-genome", "d", ("hic", "hic2"), "--trans-all --downsample-genome 0.5", NEED % "--downsample-genome"),
    C("no-balance-genome-pair", "m", ("hic",), "-ch 1 -ch2 2 --downsample-genome 0.5 --seed 3", NEED % "--downsample-genome"),
    C("no-balance-genome-cis", "m", ("hic",), "-ch 1 --balance ICE --downsample-genome 0.5", NEED % "--downsample-genome"),
    C("match-no-balance-genome", "d", ("hic", "hic2"), "--trans-all --match-depth-genome", NEED % "--match-depth-genome"),
    C("match-no-balance-genome-cis", "d", ("hic", "hic2"), "-ch 1 --balance ICE --match-depth-genome", NEED % "--match-depth-genome"),
    # ---- both new flags
    C("both", "d", ("hic", "hic2"), G + "--match-depth-genome --downsample-genome 0.5", BOTH),
    # ---- a flag of the one-chromosome thinning beside a new one
    C("downsample-too", "m", ("hic",), G + "--downsample-genome 0.5 --downsample 0.5", MIXED.format("--downsample", "--downsample-genome")),
    C("downsample-too", "d", ("hic", "hic2"), G + "--downsample-genome 0.5 --downsample 0.25",
      MIXED.format("--downsample", "--downsample-genome")),
    C("downsample-and-match-genome", "d", ("hic", "hic2"), G + "--match-depth-genome --downsample 0.5",
      MIXED.format("--downsample", "--match-depth-genome")),
    C("match-too", "d", ("hic", "hic2"), G + "--downsample-genome 0.5 --match-depth", MIXED.format("--match-depth", "--downsample-genome")),
    C("match-and-match-genome", "d", ("hic", "hic2"), "-ch 1 -ch2 2 --balance-genome ICE --match-depth-genome --match-depth",
      MIXED.format("--match-depth", "--match-depth-genome")),
    # ---- P outside (0, 1)
    C("p-zero", "m", ("hic",), G + "--downsample-genome 0", FRACTION % "0.0"),
    C("p-one", "m", ("p",), G + "--pairs-trans --downsample-genome 1", FRACTION % "1.0"),
    C("p-negative", "d", ("hic", "hic2"), G + "--downsample-genome -0.25", FRACTION % "-0.25"),
    C("p-large", "d", ("p", "g"), G + "--pairs-trans --downsample-genome 1.5", FRACTION % "1.5"),
    C("p-nan", "m", ("hic",), "-ch 1 -ch2 2 --balance-genome ICE --downsample-genome nan", FRACTION % "nan"),
    C("p-tiny", "m", ("hic",), G + "--downsample-genome 1e-10",
      "Error: --downsample-genome 1e-10: the fraction is below 2^-32, nothing would be kept"),
    C("p-tiny", "d", ("hic", "hic2"), G + "--downsample-genome 1e-10",
      "Error: --downsample-genome 1e-10: the fraction is below 2^-32, nothing would be kept"),
    # ---- --seed
    C("seed-negative", "m", ("hic",), G + "--downsample-genome 0.5 --seed -1", SEED % "-1"),
    C("seed-large", "m", ("hic",), G + "--downsample-genome 0.5 --seed 4294967296", SEED % "4294967296"),
    C("seed-large", "d", ("hic", "hic2"), G + "--match-depth-genome --seed 4294967296", SEED % "4294967296"),
    C("seed-negative", "d", ("p", "g"), G + "--pairs-trans --match-depth-genome --seed -5", SEED % "-5"),
    # ---- what --balance-genome itself refuses keeps its sentences
    C("cis-only", "m", ("hic",), "-ch 1 --balance-genome ICE --downsample-genome 0.5",
      "Error: --balance-genome is for inter-chromosomal calls; use --balance"),
    C("cis-only", "d", ("hic", "hic2"), "-ch 1 --balance-genome ICE --match-depth-genome",
      "Error: --balance-genome is for inter-chromosomal calls; use --balance"),
    C("text", "m", ("txt",), "-ch 1 -ch2 2 --balance-genome ICE --downsample-genome 0.5",
      "Error: Interchromosomal analysis is only supported for .hic and .cool input formats."),
    C("cool", "d", ("hic", "cool"), "-ch 1 -ch2 2 --balance-genome ICE --match-depth-genome",
      "Error: --balance-genome ICE and {cool}: .cool/.mcool files carry their own `weight` column; --balance-genome is for .hic input"),
    C("pairs-without-pairs-trans", "m", ("p",), G + "--downsample-genome 0.5",
      "Error: --trans-all and {p}: without --pairs-trans only intra-chromosomal loops are called from a pairs file"),
    C("pairs-without-pairs-trans", "d", ("p", "g"), "-ch chr1 -ch2 chr2 --balance-genome ICE --match-depth-genome",
      "Error: --balance-genome and {p}: without --pairs-trans only intra-chromosomal loops are called from a pairs file; use --balance"),
]
RANKS = [
    C("ranks", "m", ("hic",), G + "--downsample-genome 0.5", "Error: inter-chromosomal pairs run on one GPU only (this run has 2 ranks)"),
    C("ranks", "d", ("hic", "hic2"), "-ch 1 -ch2 2 --balance-genome ICE --match-depth-genome",
      "Error: inter-chromosomal pairs run on one GPU only (this run has 2 ranks)"),
]


def _argv(F, cli, files, extra):
    flags = ("-f",) if cli == "m" else ("-f1", "-f2")
    argv = [a for flag, key in zip(flags, files) for a in (flag, F[key])]
    return argv + ["-r", "10kb" if "hic" in files[0] or files[0] in ("txt", "cool") else "100", "-o", F["out"]] + [e.format(**F) for e in extra]


def _plan(F, cli, files, extra, ranks=1):
    from mustache_amd import diff_mustache, mustache, pairs
    from mustache_amd.request import plan, request_of
    mod = mustache if cli == "m" else diff_mustache
    args = mod.parse_args(_argv(F, cli, files, extra))
    paths = [args.f_path] if cli == "m" else [args.f_path1, args.f_path2]
    bias = [(args.biasfile, "")] if cli == "m" else [(args.biasfile1, ""), (args.biasfile2, "")]
    try:
        return plan(request_of(args, paths, bias, "-b" if cli == "m" else "-b1/-b2", ranks), mustache.parseBP(args.resolution))
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()


@pytest.mark.parametrize("cli,files,extra,line", CASES)
def test_the_refusal_and_no_output_file(F, capsys, monkeypatch, cli, files, extra, line):
    from mustache_amd import diff_mustache, mustache, pairs, sharding
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 1))
    main = mustache.main if cli == "m" else diff_mustache.main
    want = line.format(**F)
    capsys.readouterr()
    try:
        main(_argv(F, cli, files, extra))
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    said = capsys.readouterr().out.splitlines()
    print("\n".join(said))
    assert said.count(want) == 1 and sum(ln.startswith("Error:") for ln in said) == 1, said
    assert not any(os.path.exists(F["out"] + suf) for suf in ("", ".loop1", ".diffloop1", ".loop2", ".diffloop2"))


@pytest.mark.parametrize("cli,files,extra,line", CASES)
def test_the_same_line_from_plan(F, cli, files, extra, line):
    """request.plan() on the Request the command line builds: the same sentence, as a return value"""
    assert _plan(F, cli, files, extra) == line.format(**F)


@pytest.mark.parametrize("cli,files,extra,line", RANKS)
def test_a_multi_rank_run_keeps_its_sentence(F, cli, files, extra, line):
    assert _plan(F, cli, files, extra, ranks=2) == line


def test_match_depth_genome_is_diff_mustaches(F, capsys):
    """argparse of `mustache` does not know the flag; a one-file Request that carries it is refused by the rule"""
    from mustache_amd import mustache
    from mustache_amd.request import Request, plan
    with pytest.raises(SystemExit):
        mustache.parse_args(["-f", F["hic"], "-r", "10kb", "-o", F["out"], "--trans-all", "--balance-genome", "ICE", "--match-depth-genome"])
    assert "--match-depth-genome" in capsys.readouterr().err
    rq = Request([F["hic"]], [(None, "")], "-b", False, None, "ICE", "all", False, False, False, True, 'n', 'n', 1, True,
                 match_depth_genome=True)
    assert plan(rq, 10000) == "Error: --match-depth-genome matches the depths of two samples: it is diff_mustache's"
    assert not os.path.exists(F["out"])


def test_the_defaults_ask_for_nothing_and_accepted_requests_plan_as_without_the_flags(F):
    from mustache_amd import diff_mustache, mustache
    from mustache_amd.request import Plan, Request, genome_thinning_of, plan, request_of
    assert Request._fields[-3:] == ("downsample", "seed", "match_depth")              # the tuple is as it was
    rq = Request([F["hic"]], [(None, "")], "-b", False, None, "ICE", "all", False, False, False, True, ["1", "2"], 'n', 1, False)
    assert (rq.downsample_genome, rq.match_depth_genome) == (None, False) and genome_thinning_of(rq) is None
    assert rq._replace(ranks=2).downsample_genome is None
    kept = rq._replace(downsample_genome=0.25, seed=9)._replace(ranks=1)
    assert kept.downsample_genome == 0.25 and genome_thinning_of(kept) == (1 << 30, 9)
    args = mustache.parse_args(["-o", "x", "-r", "10kb"])
    assert args.downsample_genome is None and not hasattr(args, "match_depth_genome")
    args = diff_mustache.parse_args(["-o", "x", "-r", "10kb"])
    assert args.downsample_genome is None and args.match_depth_genome is False
    base = ["-f", F["hic"], "-o", F["out"], "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON"]
    want = plan(request_of(mustache.parse_args(base), [F["hic"]], [(None, "")], "-b", 1), 10000)
    assert want == Plan([], [("1", "2")], True, None, ("NEWTON", "all"))
    for extra, thin in ((["--downsample-genome", "0.5"], (1 << 31, 0)), (["--downsample-genome", "0.5", "--seed", "4294967295"],
                                                                       (1 << 31, 4294967295))):
        asked = request_of(mustache.parse_args(base + extra), [F["hic"]], [(None, "")], "-b", 1)
        assert plan(asked, 10000) == want and genome_thinning_of(asked) == thin
    two = ["-f1", F["hic"], "-f2", F["hic2"], "-o", F["out"], "-r", "10kb", "-ch", "1", "-ch2", "2", "--balance-genome", "ICE",
           "--balance-pixels", "inter", "--match-depth-genome", "--seed", "3"]
    asked = request_of(diff_mustache.parse_args(two), [F["hic"], F["hic2"]], [(None, ""), (None, "")], "-b1/-b2", 1)
    assert plan(asked, 10000) == Plan([], [("1", "2")], False, None, ("ICE", "inter")) and genome_thinning_of(asked) == ("match", 3)
    # --seed alone keeps its sentence, with or without --balance-genome
    alone = request_of(mustache.parse_args(base + ["--seed", "7"]), [F["hic"]], [(None, "")], "-b", 1)
    assert plan(alone, 10000) == "Error: --seed without --downsample or --match-depth: it seeds the thinning and nothing else"


CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from mustache_amd import diff_mustache, mustache
from mustache_amd.request import plan, request_of
said = []
for cli, argv in json.load(open(sys.argv[2])):
    mod = mustache if cli == "m" else diff_mustache
    args = mod.parse_args(argv)
    paths = [args.f_path] if cli == "m" else [args.f_path1, args.f_path2]
    bias = [(args.biasfile, "")] if cli == "m" else [(args.biasfile1, ""), (args.biasfile2, "")]
    said.append(plan(request_of(args, paths, bias, "-b" if cli == "m" else "-b1/-b2", 1), mustache.parseBP(args.resolution)))
print(json.dumps({"said": said, "torch": "torch" in sys.modules}))
"""


def test_plan_refuses_without_importing_torch(F, tmp_path):
    """every row once more, in a fresh interpreter: the lines are the same and torch was never imported"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jobs = [(p.values[0], _argv(F, p.values[0], p.values[1], p.values[2])) for p in CASES]
    (tmp_path / "jobs.json").write_text(json.dumps(jobs))
    done = subprocess.run([sys.executable, "-c", CHILD, root, str(tmp_path / "jobs.json")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    got = json.loads(done.stdout.strip().splitlines()[-1])
    assert got["torch"] is False
    assert got["said"] == [p.values[3].format(**F) for p in CASES]
