"""What both command lines refuse of --downsample / --seed / --match-depth (mustache_amd/request.py, the rule `thinning`): one
`Error:` line, no output file and no GPU, through request.plan() and through mustache.main(argv) / diff_mustache.main(argv).
The inputs and the way of asking are those of tests/test_cli_requests.py.  No GPU."""
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
    (tmp_path / "bias.txt").write_text("1.0\n1.0\n1.0\n")
    t = str(tmp_path)
    return {"hic": t + "/a.hic", "hic2": t + "/b.hic", "cool": t + "/m.cool", "txt": t + "/m.txt", "p": t + "/m.pairs",
            "g": t + "/m.pairs.gz", "b": t + "/bias.txt", "out": t + "/out"}


def C(name, cli, files, extra, line):
    return pytest.param(cli, files, extra.split(), line, id="%s-%s" % (cli, name))


RAW = "thinning needs raw integer counts"
TRANS = "Error: %s on a run with an inter-chromosomal pair: only intra-chromosomal maps are thinned"
INPUT = "Error: %s and {%s}: raw counts are thinned from .hic and .pairs / .pairs.gz input only"
FRACTION = "Error: --downsample %s: the fraction to keep must lie strictly between 0 and 1"
SEED = "Error: --seed %s: the seed is a 32-bit unsigned integer (0 .. 4294967295)"
SEED_ALONE = "Error: --seed without --downsample or --match-depth: it seeds the thinning and nothing else"
BOTH = "Error: --match-depth and --downsample: give one of them (--match-depth thins the deeper sample to the other's depth)"

CASES = [
    # ---- without --balance: thinning needs raw integer counts
    C("no-balance", "m", ("hic",), "-ch 1 --downsample 0.5", "Error: --downsample without --balance: %s; give --balance ICE|NEWTON" % RAW),
    C("no-balance", "d", ("hic", "hic2"), "-ch 1 --downsample 0.5",
      "Error: --downsample without --balance: %s; give --balance ICE|NEWTON" % RAW),
    C("match-no-balance", "d", ("hic", "hic2"), "-ch 1 --match-depth",
      "Error: --match-depth without --balance: %s; give --balance ICE|NEWTON" % RAW),
    # ---- input other than .hic or .pairs[.gz]
    C("text", "m", ("txt",), "-ch 1 --balance ICE --downsample 0.5", INPUT % ("--downsample", "txt")),
    C("text-second", "d", ("hic", "txt"), "-ch 1 --balance ICE --downsample 0.5", INPUT % ("--downsample", "txt")),
    C("match-text", "d", ("txt", "hic"), "-ch 1 --balance NEWTON --match-depth", INPUT % ("--match-depth", "txt")),
    C("cool", "m", ("cool",), "-ch 1 --balance ICE --downsample 0.5", INPUT % ("--downsample", "cool")),
    C("match-cool", "d", ("hic", "cool"), "-ch 1 --balance ICE --match-depth", INPUT % ("--match-depth", "cool")),
    # ---- together with -b or -norm
    C("bias", "m", ("hic",), "-ch 1 --balance ICE --downsample 0.5 -b {b}",
      "Error: --downsample with -b or -norm: %s; give --balance ICE|NEWTON alone" % RAW),
    C("bias2", "d", ("hic", "hic2"), "-ch 1 --balance ICE --match-depth -b2 {b}",
      "Error: --match-depth with -b1/-b2 or -norm: %s; give --balance ICE|NEWTON alone" % RAW),
    C("norm", "m", ("hic",), "-ch 1 --downsample 0.5 -norm KR", "Error: --downsample with -b or -norm: %s; give --balance ICE|NEWTON alone" % RAW),
    C("norm", "d", ("hic", "hic2"), "-ch 1 --downsample 0.5 -norm KR",
      "Error: --downsample with -b1/-b2 or -norm: %s; give --balance ICE|NEWTON alone" % RAW),
    # ---- a run with an inter-chromosomal pair
    C("trans-all", "m", ("hic",), "--trans-all -ch 1 2 --downsample 0.5", TRANS % "--downsample"),
    C("trans-all", "d", ("hic", "hic2"), "--trans-all -ch 1 2 --match-depth", TRANS % "--match-depth"),
    C("pair", "m", ("hic",), "-ch 1 -ch2 2 --downsample 0.5", TRANS % "--downsample"),
    C("pair", "d", ("hic", "hic2"), "-ch 1 -ch2 2 --match-depth", TRANS % "--match-depth"),
    C("mixed-pairs", "m", ("hic",), "-ch 1 1 -ch2 1 2 --balance ICE --downsample 0.5", TRANS % "--downsample"),
    C("balance-genome", "m", ("hic",), "-ch 1 -ch2 2 --balance-genome ICE --downsample 0.5", TRANS % "--downsample"),
    C("balance-genome", "d", ("hic", "hic2"), "--trans-all --balance-genome ICE --downsample 0.5", TRANS % "--downsample"),
    C("pairs-trans", "m", ("p",), "--trans-all --pairs-trans --balance-genome ICE --downsample 0.5", TRANS % "--downsample"),
    C("pairs-trans", "d", ("p", "g"), "-ch chr1 -ch2 chr2 --pairs-trans --balance-genome ICE --match-depth", TRANS % "--match-depth"),
    # ---- P outside (0, 1)
    C("p-zero", "m", ("hic",), "-ch 1 --balance ICE --downsample 0", FRACTION % "0.0"),
    C("p-one", "m", ("p",), "-ch chr1 --balance ICE --downsample 1", FRACTION % "1.0"),
    C("p-negative", "d", ("hic", "hic2"), "-ch 1 --balance ICE --downsample -0.25", FRACTION % "-0.25"),
    C("p-large", "d", ("p", "g"), "-ch chr1 --balance ICE --downsample 1.5", FRACTION % "1.5"),
    C("p-nan", "m", ("hic",), "-ch 1 --balance ICE --downsample nan", FRACTION % "nan"),
    C("p-tiny", "m", ("hic",), "-ch 1 --balance ICE --downsample 1e-10",
      "Error: --downsample 1e-10: the fraction is below 2^-32, nothing would be kept"),
    # ---- --seed
    C("seed-negative", "m", ("hic",), "-ch 1 --balance ICE --downsample 0.5 --seed -1", SEED % "-1"),
    C("seed-large", "d", ("hic", "hic2"), "-ch 1 --balance ICE --match-depth --seed 4294967296", SEED % "4294967296"),
    C("seed-alone", "m", ("hic",), "-ch 1 --balance ICE --seed 7", SEED_ALONE),
    C("seed-alone", "d", ("hic", "hic2"), "-ch 1 --balance ICE --seed 0", SEED_ALONE),
    # ---- --match-depth together with --downsample
    C("both", "d", ("hic", "hic2"), "-ch 1 --balance ICE --match-depth --downsample 0.5", BOTH),
]


def _argv(F, cli, files, extra):
    flags = ("-f",) if cli == "m" else ("-f1", "-f2")
    argv = [a for flag, key in zip(flags, files) for a in (flag, F[key])]
    return argv + ["-r", "10kb" if "hic" in files[0] or files[0] in ("txt", "cool") else "100", "-o", F["out"]] + [e.format(**F) for e in extra]


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
    from mustache_amd import diff_mustache, mustache, pairs
    from mustache_amd.request import plan, request_of
    mod = mustache if cli == "m" else diff_mustache
    args = mod.parse_args(_argv(F, cli, files, extra))
    paths = [args.f_path] if cli == "m" else [args.f_path1, args.f_path2]
    bias = [(args.biasfile, "")] if cli == "m" else [(args.biasfile1, ""), (args.biasfile2, "")]
    try:
        got = plan(request_of(args, paths, bias, "-b" if cli == "m" else "-b1/-b2", 1), mustache.parseBP(args.resolution))
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    assert got == line.format(**F)


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


def test_the_defaults_ask_for_nothing(F):
    from mustache_amd import diff_mustache, mustache
    from mustache_amd.request import Plan, Request, plan, request_of
    assert Request._fields[-3:] == ("downsample", "seed", "match_depth")              # appended: positional callers keep working
    rq = Request([F["hic"]], [(None, "")], "-b", False, "ICE", None, "all", False, False, False, False, ["1"], 'n', 1, False)
    assert (rq.downsample, rq.seed, rq.match_depth) == (None, None, False)
    assert plan(rq, 10000) == Plan([("1", "1")], [], False, "ICE", None)
    args = mustache.parse_args(["-o", "x", "-r", "10kb"])
    assert args.downsample is None and args.seed is None and not hasattr(args, "match_depth")
    args = diff_mustache.parse_args(["-o", "x", "-r", "10kb"])
    assert args.downsample is None and args.seed is None and args.match_depth is False
    # an accepted request: the plan is the one of the run without the flags
    for extra in (["--downsample", "0.5"], ["--downsample", "0.5", "--seed", "4294967295"]):
        args = mustache.parse_args(["-f", F["hic"], "-o", F["out"], "-r", "10kb", "-ch", "1", "--balance", "ICE"] + extra)
        assert plan(request_of(args, [F["hic"]], [(None, "")], "-b", 1), 10000) == Plan([("1", "1")], [], False, "ICE", None)
    args = diff_mustache.parse_args(["-f1", F["p"], "-f2", F["hic"], "-o", F["out"], "-r", "10kb", "-ch", "1", "--balance", "NEWTON",
                                     "--match-depth", "--seed", "3"])
    assert plan(request_of(args, [F["p"], F["hic"]], [(None, ""), (None, "")], "-b1/-b2", 1), 10000) == \
        Plan([("1", "1")], [], False, "NEWTON", None)


def test_the_library_guards_say_the_same():
    """read_contacts / read_pair / regulator called directly: the keyword arguments are refused where the command line would be"""
    from mustache_amd import diff_mustache, mustache
    from mustache_amd.downsample import DownsampleError
    from mustache_amd.trans import TransError
    with pytest.raises(DownsampleError, match="raw integer counts"):
        mustache.read_sample("a.hic", False, False, 5000, 1000000, False, "1", downsample=0.5)
    with pytest.raises(DownsampleError, match=r"\.hic and \.pairs"):
        mustache.read_sample("a.txt", False, False, 5000, 1000000, False, "1", balance="ICE", downsample=0.5)
    with pytest.raises(DownsampleError, match="one of them"):
        diff_mustache.read_pair("a.hic", "b.hic", False, False, 5000, 1000000, False, False, "1", "1", verbose=False, balance="ICE",
                                downsample=0.5, match_depth=True)
    with pytest.raises(DownsampleError, match="inter-chromosomal"):
        diff_mustache.regulator("a.hic", "b.hic", False, False, "o", chromosome="1", chromosome2="2", match_depth=True)
    with pytest.raises(TransError, match="inter-chromosomal"):
        mustache.read_contacts("a.hic", False, False, 5000, 1000000, False, "1", "2", verbose=False, downsample=0.5)
