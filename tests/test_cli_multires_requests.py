"""What `mustache` refuses of --coarser / --merge-distance (mustache_amd/request.py, the rule `multires`): one `Error:` line, no
output file and no GPU, through request.plan() and through mustache.main(argv).  The inputs and the way of asking are those of
tests/test_cli_downsample_requests.py.  No GPU."""
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
    (tmp_path / "bias.txt").write_text("1.0\n1.0\n1.0\n")
    t = str(tmp_path)
    return {"hic": t + "/a.hic", "cool": t + "/m.cool", "txt": t + "/m.txt", "p": t + "/m.pairs", "g": t + "/m.pairs.gz",
            "b": t + "/bias.txt", "out": t + "/out"}


def C(name, files, extra, line, ranks=1):
    return pytest.param(files, extra.split(), line, ranks, id=name)


RAW = "coarsening sums raw integer counts; give --balance ICE|NEWTON alone"
TRANS = "Error: --coarser on a run with an inter-chromosomal pair: only intra-chromosomal maps are coarsened"
INPUT = "Error: --coarser and {%s}: raw counts are coarsened from .hic and .pairs / .pairs.gz input only"
ALONE = "Error: --merge-distance without --coarser: it is the tolerance of the multi-resolution merge and nothing else"

# -r is 10kb for the .hic, text and .cool files and 100 for the pairs files
CASES = [
    # ---- a value that does not parse, is not greater than -r, is no multiple of it, or is given twice
    C("unparsable", "hic", "-ch 1 --balance ICE --coarser 20kb abc", "Error: --coarser abc: not a resolution (give base pairs, or a number with kb or mb)"),
    C("zero", "p", "-ch chr1 --balance ICE --coarser 0", "Error: --coarser 0: not a resolution (give base pairs, or a number with kb or mb)"),
    C("equal", "hic", "-ch 1 --balance ICE --coarser 10000", "Error: --coarser 10000: a coarser resolution is greater than -r (10000 bp)"),
    C("finer", "hic", "-ch 1 --balance NEWTON --coarser 20kb 5kb", "Error: --coarser 5kb: a coarser resolution is greater than -r (10000 bp)"),
    C("no-multiple", "hic", "-ch 1 --balance ICE --coarser 25kb", "Error: --coarser 25kb: 25000 bp is not an integer multiple of -r (10000 bp)"),
    C("no-multiple-pairs", "g", "-ch chr1 --balance ICE --coarser 200 250", "Error: --coarser 250: 250 bp is not an integer multiple of -r (100 bp)"),
    C("twice", "hic", "-ch 1 --balance ICE --coarser 20kb 50kb 20000", "Error: --coarser 20000: 20000 bp is given twice"),
    # ---- --merge-distance without --coarser, or negative
    C("distance-alone", "hic", "-ch 1 --balance ICE --merge-distance 1", ALONE),
    C("distance-alone-pairs", "p", "-ch chr1 --balance ICE --merge-distance 0", ALONE),
    C("distance-negative", "hic", "-ch 1 --balance ICE --coarser 20kb --merge-distance -1",
      "Error: --merge-distance -1: the distance is a number of bins >= 0"),
    # ---- without --balance, or together with -b / -norm
    C("no-balance", "hic", "-ch 1 --coarser 20kb", "Error: --coarser without --balance: %s" % RAW),
    C("bias", "hic", "-ch 1 --balance ICE --coarser 20kb -b {b}", "Error: --coarser with -b or -norm: %s" % RAW),
    C("bias-no-balance", "hic", "-ch 1 --coarser 20kb -b {b}", "Error: --coarser with -b or -norm: %s" % RAW),
    C("norm", "hic", "-ch 1 --coarser 20kb -norm KR", "Error: --coarser with -b or -norm: %s" % RAW),
    # ---- input other than .hic or .pairs[.gz]
    C("text", "txt", "-ch 1 --balance ICE --coarser 20kb", INPUT % "txt"),
    C("cool", "cool", "-ch 1 --balance ICE --coarser 20kb", INPUT % "cool"),
    # ---- a run with an inter-chromosomal pair
    C("trans-all", "hic", "--trans-all -ch 1 2 --coarser 20kb", TRANS),
    C("pair", "hic", "-ch 1 -ch2 2 --coarser 20kb", TRANS),
    C("mixed-pairs", "hic", "-ch 1 1 -ch2 1 2 --balance ICE --coarser 20kb", TRANS),
    C("balance-genome", "hic", "-ch 1 -ch2 2 --balance-genome ICE --coarser 20kb", TRANS),
    C("pairs-trans", "p", "--trans-all --pairs-trans --balance-genome ICE --coarser 200", TRANS),
    # ---- a multi-rank run
    C("ranks", "hic", "-ch 1 --balance ICE --coarser 20kb",
      "Error: --coarser in a multi-rank run (world size 2): every resolution of a chromosome is called on one GPU; start a single process",
      ranks=2),
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


CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from mustache_amd import mustache
from mustache_amd.request import plan, request_of
said = []
for argv, ranks in json.load(open(sys.argv[2])):
    args = mustache.parse_args(argv)
    said.append(plan(request_of(args, [args.f_path], [(args.biasfile, "")], "-b", ranks), mustache.parseBP(args.resolution)))
print(json.dumps({"said": said, "torch": "torch" in sys.modules}))
"""


def test_plan_refuses_without_importing_torch(F, tmp_path):
    """every row once more, in a fresh interpreter: the lines are the same and torch was never imported"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jobs = [(_argv(F, p.values[0], p.values[1]), p.values[3]) for p in CASES]
    (tmp_path / "jobs.json").write_text(json.dumps(jobs))
    done = subprocess.run([sys.executable, "-c", CHILD, root, str(tmp_path / "jobs.json")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    got = json.loads(done.stdout.strip().splitlines()[-1])
    assert got["torch"] is False
    assert got["said"] == [p.values[2].format(**F) for p in CASES]


def test_the_defaults_ask_for_nothing(F):
    from mustache_amd import diff_mustache, mustache
    from mustache_amd.request import Plan, Request, coarser_resolutions, plan, request_of
    # behind the tuple, by keyword, with defaults: a positional caller keeps working
    rq = Request([F["hic"]], [(None, "")], "-b", False, "ICE", None, "all", False, False, False, False, ["1"], 'n', 1, False)
    assert (rq.coarser, rq.merge_distance) == (None, None) and coarser_resolutions(rq, 10000) == []
    assert plan(rq, 10000) == Plan([("1", "1")], [], False, "ICE", None)
    kept = rq._replace(ranks=1)
    assert (kept.coarser, kept.merge_distance) == (None, None) and kept == rq
    args = mustache.parse_args(["-o", "x", "-r", "10kb"])
    assert args.coarser is None and args.merge_distance is None and args.resolution == "10kb"
    args = diff_mustache.parse_args(["-o", "x", "-r", "10kb"])
    assert not hasattr(args, "coarser") and not hasattr(args, "merge_distance")
    with pytest.raises(SystemExit):
        diff_mustache.parse_args(["-o", "x", "-r", "10kb", "--coarser", "20kb"])
    # an accepted request: the plan is the one of the run without the flags, the resolutions come in ascending order
    for extra, want in ((["--coarser", "20kb"], [20000]), (["--coarser", "50kb", "20000", "--merge-distance", "0"], [20000, 50000]),
                        (["--coarser", "1mb", "--downsample", "0.5", "--seed", "3"], [1000000])):
        for key, ch in (("hic", "1"), ("p", "chr1"), ("g", "chr1")):
            args = mustache.parse_args(["-f", F[key], "-o", F["out"], "-r", "10kb", "-ch", ch, "--balance", "NEWTON"] + extra)
            rq = request_of(args, [F[key]], [(None, "")], "-b", 1)
            assert plan(rq, 10000) == Plan([(ch, ch)], [], False, "NEWTON", None)
            assert coarser_resolutions(rq, 10000) == want
            assert rq._replace(ranks=2).coarser == rq.coarser
