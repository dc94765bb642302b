"""What both command lines refuse, one row per rule: the `Error:` line in stdout (or the exception plus the printed sentence)
and no output file.  The table drives only mustache.main(argv) and diff_mustache.main(argv); its lines are what the command
lines printed before the rules moved into mustache_amd/request.py, pasted.  A row with `parent=` holds an argument list with two
conflicts of which the one order of request.plan() names another than the command line used to: `parent` is the old line, and
is what the row expects of a tree without mustache_amd/request.py.  No GPU."""
import gzip
import importlib.util
import os

import pytest

from hic_trans_writer import write_hic_pairs

ONE_ORDER = importlib.util.find_spec("mustache_amd.request") is not None

PAIRS_HEADER = "## pairs format v1.0\n#chromsize: chr1 1000\n#chromsize: chr2 500\n"
PAIRS_ROWS = "".join("r%d\t%s\t%d\t%s\t%d\t+\t-\n" % ((k,) + r) for k, r in enumerate(
    [("chr1", 10, "chr1", 700), ("chr1", 20, "chr2", 30), ("chr2", 40, "chr1", 50), ("chr2", 5, "chr2", 400), ("chr1", 1, "chr2", 1)]))


@pytest.fixture
def F(tmp_path, monkeypatch):
    """the inputs by key; `{key}` in a row's arguments and line stands for the path"""
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    chroms = [("All", 1000), ("1", 200000), ("2", 150000)]
    for name in ("a.hic", "b.hic"):                           # two chromosomes, one 10 kb trans matrix of two records
        write_hic_pairs(str(tmp_path / name), chroms, {(1, 2): {10000: ([0, 1], [2, 3], [5.0, 6.0])}}, version=8)
    (tmp_path / "e.hic").write_bytes(b"")                     # a refusal that reads nothing
    (tmp_path / "m.cool").write_bytes(b"")
    (tmp_path / "m.txt").write_text("1\t10000\t2\t20000\t5\n")
    (tmp_path / "m.pairs").write_text(PAIRS_HEADER + PAIRS_ROWS)
    (tmp_path / "m.pairs.gz").write_bytes(gzip.compress((PAIRS_HEADER + PAIRS_ROWS).encode()))
    (tmp_path / "bare.pairs").write_text(PAIRS_ROWS)
    (tmp_path / "bias.txt").write_text("1.0\n1.0\n1.0\n")
    t = str(tmp_path)
    return {"hic": t + "/a.hic", "hic2": t + "/b.hic","ehic": t + "/e.hic", "cool": t + "/m.cool", "txt": t + "/m.txt",
            "p": t + "/m.pairs", "g": t + "/m.pairs.gz", "bare": t + "/bare.pairs", "b": t + "/bias.txt",
            "missing": t + "/not_there", "out": t + "/out"}


def C(name, cli, files, extra, line, ranks=1, raises=None, res="10kb", parent=None):
    return pytest.param(cli, files, extra.split(), line, ranks, raises, res, parent, id="%s-%s" % (cli, name))


BALANCE_ON_TRANS = "Error: --balance does not apply to inter-chromosomal pairs"
TEXT = "Error: Interchromosomal analysis is only supported for .hic and .cool input formats."
TEXT_SAID = TEXT[len("Error: "):]                              # the sentence alone: what the raising refusal prints
ONE_GPU = "Error: inter-chromosomal pairs run on one GPU only (this run has 2 ranks)"
NEED_CH = "Error: inter-chromosomal pairs need -ch and -ch2 (all-pairs runs are not supported)"
NO_FILES = "Error: Couldn't find the specified contact files"
NOT_TRANS = "Error: --balance-genome is for inter-chromosomal calls; use --balance"
WITHOUT = "without --pairs-trans only intra-chromosomal loops are called from a pairs file"
PT_BALANCE = "Error: --pairs-trans with --balance, %s or -norm: the trans rows of {p} are raw read pairs and are balanced with " \
             "the whole genome; give --balance-genome ICE|NEWTON alone"

CASES = [
    # ---- the inputs
    C("no-file", "m", (), "-ch 1", NO_FILES),
    C("missing-file", "m", ("missing",), "-ch 1", NO_FILES),
    C("no-second-file", "d", ("hic",), "-ch 1", NO_FILES),
    C("missing-second-file", "d", ("hic", "missing"), "-ch 1", NO_FILES),
    C("invalid-r", "m", ("hic",), "-ch 1", "Error: Invalid resolution", res="fine"),
    C("invalid-r", "d", ("hic", "hic2"), "-ch 1", "Error: Invalid resolution", res="fine"),
    C("missing-b", "m", ("txt",), "-ch 1 -b {missing}", "Error: Couldn't find specified bias file"),
    C("missing-b1", "d", ("txt", "txt"), "-ch 1 -b1 {missing}", "Error: Couldn't find the specified bias file1"),
    C("missing-b2", "d", ("txt", "txt"), "-ch 1 -b2 {missing}", "Error: Couldn't find the specified bias file2"),
    # ---- --balance
    C("balance-unknown", "m", ("txt",), "-ch 1 --balance KR", "Error: --balance KR: unknown method (supported: ICE, NEWTON)"),
    C("balance-unknown", "d", ("txt", "txt"), "-ch 1 --balance KR", "Error: --balance KR: unknown method (supported: ICE, NEWTON)"),
    C("balance-b", "m", ("txt",), "-ch 1 --balance ICE -b {b}",
      "Error: --balance ICE and -b: give either a bias file or --balance, not both"),
    C("balance-b2", "d", ("txt", "txt"), "-ch 1 --balance ICE -b2 {b}",
      "Error: --balance ICE and -b1/-b2: give either a bias file or --balance, not both"),
    C("balance-norm", "m", ("txt",), "-ch 1 --balance newton -norm KR",
      "Error: --balance NEWTON and -norm KR: --balance reads raw counts; leave -norm unset or NONE"),
    C("balance-norm", "d", ("txt", "txt"), "-ch 1 --balance ICE -norm KR",
      "Error: --balance ICE and -norm KR: --balance reads raw counts; leave -norm unset or NONE"),
    C("balance-cool", "m", ("cool",), "-ch 1 --balance ICE",
      "Error: --balance ICE and {cool}: .cool/.mcool files carry their own `weight` column; --balance is for text and .hic input"),
    C("balance-cool-second", "d", ("txt", "cool"), "-ch 1 --balance ICE",
      "Error: --balance ICE and {cool}: .cool/.mcool files carry their own `weight` column; --balance is for text and .hic input"),
    C("balance-ranks", "m", ("txt",), "-ch 1 --balance ICE", ranks=2,
      line="Error: --balance ICE in a multi-rank run (world size 2): balancing runs on one GPU; start a single process"),
    C("balance-ranks", "d", ("txt", "txt"), "-ch 1 --balance ICE", ranks=2,
      line="Error: --balance ICE in a multi-rank run (world size 2): balancing runs on one GPU; start a single process"),
    C("balance-pair", "m", ("hic",), "-ch 1 -ch2 2 --balance ICE", BALANCE_ON_TRANS),
    C("balance-pair", "d", ("hic", "hic2"), "-ch 1 -ch2 2 --balance ICE", BALANCE_ON_TRANS),
    C("balance-trans-all", "m", ("ehic",), "--trans-all -ch 1 2 --balance ICE", BALANCE_ON_TRANS),
    C("balance-trans-all", "d", ("ehic", "ehic"), "--trans-all -ch 1 2 --balance ICE", BALANCE_ON_TRANS),
    # ---- -ch / -ch2
    C("ch2-without-ch", "m", ("hic",), "-ch2 2 1", NEED_CH),
    C("ch2-without-ch", "d", ("hic", "hic2"), "-ch2 2 1", NEED_CH),
    C("ch-ch2-lengths", "m", ("hic",), "-ch 1 2 -ch2 1", "Error: the same number of chromosome1 and chromosome2 should be provided."),
    C("ch-ch2-lengths", "d", ("hic", "hic2"), "-ch 1 2 -ch2 1",
      "Error: the same number of chromosome1 and chromosome2 should be provided."),
    C("no-ch-text", "m", ("txt",), "", "Error: Please enter the chromosome name."),
    C("no-ch-text", "d", ("txt", "txt"), "", "Error: Please enter the chromosome name."),
    # ---- a trans pair or --trans-all: text input, ranks, -ch2
    C("pair-text", "m", ("txt",), "-ch 1 -ch2 2", TEXT_SAID, raises=FileNotFoundError),
    C("pair-text", "d", ("txt", "hic"), "-ch 1 -ch2 2", TEXT),
    C("pair-text-second", "d", ("hic", "txt"), "-ch 1 -ch2 2", TEXT),
    C("trans-all-text", "m", ("txt",), "--trans-all -ch 1 2", TEXT),
    C("trans-all-text", "d", ("txt", "ehic"), "--trans-all -ch 1 2", TEXT),
    C("trans-all-text-second", "d", ("ehic", "txt"), "--trans-all -ch 1 2", TEXT),
    C("pair-ranks", "m", ("hic",), "-ch 1 -ch2 2", ONE_GPU, ranks=2),
    C("pair-ranks", "d", ("hic", "hic2"), "-ch 1 -ch2 2", ONE_GPU, ranks=2),
    C("trans-all-ranks", "m", ("ehic",), "--trans-all -ch 1 2", ONE_GPU, ranks=2),
    C("trans-all-ranks", "d", ("ehic", "ehic"), "--trans-all -ch 1 2", ONE_GPU, ranks=2),
    C("trans-all-ch2", "m", ("ehic",), "--trans-all -ch 1 -ch2 2", "Error: --trans-all pairs the -ch list with itself; give -ch2 without it"),
    C("trans-all-ch2", "d", ("ehic", "ehic"), "--trans-all -ch 1 -ch2 2",
      "Error: --trans-all pairs the -ch list with itself; give -ch2 without it"),
    # ---- --balance-genome / --balance-pixels
    C("pixels-alone", "m", ("hic",), "-ch 1 -ch2 2 --balance-pixels inter",
      "Error: --balance-pixels inter without --balance-genome: it chooses the pixels --balance-genome balances on"),
    C("pixels-alone", "d", ("hic", "hic2"), "--trans-all -ch 1 2 --balance-pixels all",
      "Error: --balance-pixels all without --balance-genome: it chooses the pixels --balance-genome balances on"),
    C("genome-unknown", "m", ("hic",), "-ch 1 -ch2 2 --balance-genome KR",
      "Error: --balance-genome KR: unknown method (supported: ICE, NEWTON)"),
    C("genome-unknown", "d", ("hic", "hic2"), "--trans-all -ch 1 2 --balance-genome KR",
      "Error: --balance-genome KR: unknown method (supported: ICE, NEWTON)"),
    C("pixels-unknown", "m", ("hic",), "--trans-all -ch 1 2 --balance-genome ICE --balance-pixels cis",
      "Error: --balance-pixels cis: unknown value (supported: all, inter)"),
    C("pixels-unknown", "d", ("hic", "hic2"), "-ch 1 -ch2 2 --balance-genome ICE --balance-pixels cis",
      "Error: --balance-pixels cis: unknown value (supported: all, inter)"),
    C("genome-cis", "m", ("hic",), "-ch 1 --balance-genome ICE", NOT_TRANS),
    C("genome-cis", "d", ("hic", "hic2"), "-ch 1 --balance-genome ICE", NOT_TRANS),
    C("genome-mixed", "m", ("hic",), "-ch 1 1 -ch2 1 2 --balance-genome ICE", NOT_TRANS),
    C("genome-mixed", "d", ("hic", "hic2"), "-ch 1 1 -ch2 1 2 --balance-genome ICE", NOT_TRANS),
    C("genome-b", "m", ("hic",), "-ch 1 -ch2 2 --balance-genome ICE -b {b}",
      "Error: --balance-genome ICE and a bias file (-b / -b1 / -b2): give either a bias file or --balance-genome, not both"),
    C("genome-b1", "d", ("hic", "hic2"), "--trans-all -ch 1 2 --balance-genome ICE -b1 {b}",
      "Error: --balance-genome ICE and a bias file (-b / -b1 / -b2): give either a bias file or --balance-genome, not both"),
    C("genome-norm", "m", ("hic",), "--trans-all -ch 1 2 --balance-genome ICE -norm KR",
      "Error: --balance-genome ICE and -norm KR: --balance-genome reads raw counts; leave -norm unset or NONE"),
    C("genome-norm", "d", ("hic", "hic2"), "-ch 1 -ch2 2 --balance-genome ICE -norm KR",
      "Error: --balance-genome ICE and -norm KR: --balance-genome reads raw counts; leave -norm unset or NONE"),
    C("genome-cool", "m", ("cool",), "-ch 1 -ch2 2 --balance-genome ICE",
      "Error: --balance-genome ICE and {cool}: .cool/.mcool files carry their own `weight` column; --balance-genome is for .hic input"),
    C("genome-cool-second", "d", ("hic", "cool"), "--trans-all -ch 1 2 --balance-genome ICE",
      "Error: --balance-genome ICE and {cool}: .cool/.mcool files carry their own `weight` column; --balance-genome is for .hic input"),
    C("genome-ranks", "m", ("hic",), "-ch 1 -ch2 2 --balance-genome ICE", ONE_GPU, ranks=2),          # pinned: the pairs' own rule first
    C("genome-ranks", "d", ("hic", "hic2"), "--trans-all -ch 1 2 --balance-genome ICE", ONE_GPU, ranks=2),
    # ---- pairs input, --pairs-trans, --pairs-zero-based
    C("pairs-trans-no-pairs", "m", ("txt",), "-ch 1 --pairs-trans", "Error: --pairs-trans is for .pairs / .pairs.gz input ({txt} is none)"),
    C("pairs-trans-no-pairs", "d", ("txt", "hic"), "-ch 1 --pairs-trans",
      "Error: --pairs-trans is for .pairs / .pairs.gz input ({txt}, {hic} is none)"),
    C("zero-based-no-pairs", "m", ("hic",), "-ch 1 --pairs-zero-based",
      "Error: --pairs-zero-based is for .pairs / .pairs.gz input ({hic} is none)"),
    C("zero-based-no-pairs", "d", ("hic", "txt"), "-ch 1 --pairs-zero-based",
      "Error: --pairs-zero-based is for .pairs / .pairs.gz input ({hic}, {txt} is none)"),
    C("pairs-trans-cis", "m", ("p",), "-ch chr1 --pairs-trans --balance-genome ICE", res="100",
      line="Error: --pairs-trans on a run with no inter-chromosomal pair: give --trans-all, or -ch A -ch2 B"),
    C("pairs-trans-cis", "d", ("hic", "p"), "-ch chr1 -ch2 chr1 --pairs-trans --balance-genome ICE", res="100",
      line="Error: --pairs-trans on a run with no inter-chromosomal pair: give --trans-all, or -ch A -ch2 B"),
    C("pairs-trans-balance", "m", ("p",), "--trans-all --pairs-trans --balance-genome ICE --balance ICE", PT_BALANCE % "-b", res="100"),
    C("pairs-trans-balance", "d", ("p", "g"), "--trans-all --pairs-trans --balance-genome ICE -norm KR", PT_BALANCE % "-b1/-b2",
      res="100"),
    C("pairs-trans-no-genome", "m", ("p",), "-ch chr1 -ch2 chr2 --pairs-trans", res="100",
      line="Error: --pairs-trans without --balance-genome: {p} holds raw read pairs; give --balance-genome ICE|NEWTON"),
    C("pairs-trans-no-genome", "d", ("hic", "p"), "--trans-all --pairs-trans", res="100",
      line="Error: --pairs-trans without --balance-genome: {p} holds raw read pairs; give --balance-genome ICE|NEWTON"),
    C("pairs-trans-ranks", "m", ("p",), "--trans-all --pairs-trans --balance-genome ICE", ranks=2, res="100",
      line="Error: --pairs-trans in a multi-rank run (world size 2): the genome is balanced on one GPU; start a single process"),
    C("pairs-trans-ranks", "d", ("p", "g"), "-ch chr1 -ch2 chr2 --pairs-trans --balance-genome ICE", ranks=2, res="100",
      line="Error: --pairs-trans in a multi-rank run (world size 2): the genome is balanced on one GPU; start a single process"),
    C("pairs-trans-all", "m", ("p",), "--trans-all --balance ICE", "Error: --trans-all and {p}: " + WITHOUT, res="100"),
    C("pairs-trans-all", "d", ("hic", "p"), "--trans-all --balance ICE", "Error: --trans-all and {p}: " + WITHOUT, res="100"),
    C("pairs-genome", "m", ("g",), "-ch chr1 --balance-genome ICE", "Error: --balance-genome and {g}: " + WITHOUT + "; use --balance",
      res="100"),
    C("pairs-genome", "d", ("g", "p"), "-ch chr1 --balance-genome ICE", "Error: --balance-genome and {g}: " + WITHOUT + "; use --balance",
      res="100"),
    C("pairs-other-ch2", "m", ("p",), "-ch chr1 -ch2 chr2 --balance ICE", "Error: -ch2 with another chromosome and {p}: " + WITHOUT,
      res="100"),
    C("pairs-other-ch2", "d", ("p", "p"), "-ch chr1 -ch2 chr2 --balance ICE", "Error: -ch2 with another chromosome and {p}: " + WITHOUT,
      res="100"),
    C("pairs-no-balance", "m", ("p",), "-ch chr1", "Error: {p} holds raw read pairs: give --balance ICE|NEWTON", res="100"),
    C("pairs-no-balance", "d", ("txt", "p"), "-ch chr1", "Error: {p} holds raw read pairs: give --balance ICE|NEWTON", res="100"),
    C("pairs-balance-b", "m", ("p",), "-ch chr1 --balance ICE -b {b}", res="100",
      line="Error: --balance ICE and -b: give either a bias file or --balance, not both"),
    C("pairs-balance-ranks", "m", ("p",), "-ch chr1 --balance ICE", ranks=2, res="100",
      line="Error: --balance ICE in a multi-rank run (world size 2): balancing runs on one GPU; start a single process"),
    C("pairs-balance-ranks", "d", ("p", "g"), "-ch chr1 --balance ICE", ranks=2, res="100",
      line="Error: --balance ICE in a multi-rank run (world size 2): balancing runs on one GPU; start a single process"),
    # ---- two conflicts that existing tests pin
    C("balance-and-genome-pair", "m", ("hic",), "-ch 1 -ch2 2 --balance ICE --balance-genome NEWTON", BALANCE_ON_TRANS),
    C("balance-and-genome-trans-all", "d", ("hic", "hic2"), "--trans-all --balance ICE --balance-genome NEWTON", BALANCE_ON_TRANS),
    C("genome-pair-text", "m", ("txt",), "-ch 1 -ch2 2 --balance-genome NEWTON", TEXT),
    C("genome-pair-text-second", "d", ("hic", "txt"), "-ch 1 -ch2 2 --balance-genome NEWTON", TEXT),
    C("genome-trans-all-text", "m", ("txt",), "--trans-all -ch 1 2 --balance-genome NEWTON", TEXT),
    C("pairs-trans-cis-balance", "m", ("p",), "-ch chr1 --pairs-trans --balance ICE", res="100",
      line="Error: --pairs-trans on a run with no inter-chromosomal pair: give --trans-all, or -ch A -ch2 B"),
    C("pairs-trans-all-genome", "m", ("p",), "--trans-all --balance-genome ICE", "Error: --trans-all and {p}: " + WITHOUT, res="100"),
    # ---- two conflicts, to state the one order: a trans pair's rules are -ch, --balance, the ranks, --balance-genome, the input
    C("trans-all-balance-ranks", "m", ("ehic",), "--trans-all -ch 1 2 --balance ICE", BALANCE_ON_TRANS, ranks=2, parent=ONE_GPU),
    C("trans-all-balance-ranks", "d", ("ehic", "ehic"), "--trans-all -ch 1 2 --balance ICE", BALANCE_ON_TRANS, ranks=2),
    C("pair-balance-ranks", "m", ("hic",), "-ch 1 -ch2 2 --balance ICE", ranks=2,
      line="Error: --balance ICE in a multi-rank run (world size 2): balancing runs on one GPU; start a single process"),
    C("pair-text-balance", "m", ("txt",), "-ch 1 -ch2 2 --balance ICE", BALANCE_ON_TRANS),
    C("pair-text-balance", "d", ("hic", "txt"), "-ch 1 -ch2 2 --balance ICE", BALANCE_ON_TRANS, parent=TEXT),
    C("pair-text-ranks", "m", ("txt",), "-ch 1 -ch2 2", ONE_GPU, ranks=2),
    C("pair-text-ranks", "d", ("txt", "hic"), "-ch 1 -ch2 2", ONE_GPU, ranks=2, parent=TEXT),
    C("pair-text-genome-unknown", "m", ("txt",), "-ch 1 -ch2 2 --balance-genome KR",
      "Error: --balance-genome KR: unknown method (supported: ICE, NEWTON)"),
    C("pair-text-genome-unknown", "d", ("hic", "txt"), "-ch 1 -ch2 2 --balance-genome KR",
      "Error: --balance-genome KR: unknown method (supported: ICE, NEWTON)", parent=TEXT),
]


def _argv(F, cli, files, extra, res):
    flags = ("-f",) if cli == "m" else ("-f1", "-f2")
    argv = [a for flag, key in zip(flags, files) for a in (flag, F[key])]
    return argv + ["-r", res, "-o", F["out"]] + [e.format(**F) for e in extra]


@pytest.mark.parametrize("cli,files,extra,line,ranks,raises,res,parent", CASES)
def test_the_refusal_and_no_output_file(F, capsys, monkeypatch, cli, files, extra, line, ranks, raises, res, parent):
    from mustache_amd import diff_mustache, mustache, pairs, sharding
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, ranks))       # what torchrun's WORLD_SIZE would make it return
    if ranks > 1:
        monkeypatch.setenv("WORLD_SIZE", str(ranks))
    main = mustache.main if cli == "m" else diff_mustache.main
    want = (line if ONE_ORDER or parent is None else parent).format(**F)
    capsys.readouterr()
    try:
        if raises:
            with pytest.raises(raises):
                main(_argv(F, cli, files, extra, res))
        else:
            main(_argv(F, cli, files, extra, res))
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    said = capsys.readouterr().out.splitlines()
    print("\n".join(said))
    assert said.count(want) == 1 and sum(ln.startswith("Error:") for ln in said) == (0 if raises else 1), said
    assert not any(os.path.exists(F["out"] + suf) for suf in ("", ".loop1", ".diffloop1", ".loop2", ".diffloop2"))


# the pairs file without `#chromsize` lines under --pairs-trans: refused by its parse, which is the one parse of the run
NO_TABLE = [
    ("m", ("bare",), "--trans-all --pairs-trans --balance-genome ICE"),
    ("m", ("bare",), "-ch chr1 -ch2 chr2 --pairs-trans --balance-genome ICE"),
    ("d", ("p", "bare"), "--trans-all --pairs-trans --balance-genome ICE"),
    ("d", ("bare", "g"), "-ch chr1 -ch2 chr2 --pairs-trans --balance-genome ICE"),
]


@pytest.mark.parametrize("cli,files,extra", NO_TABLE)
def test_a_pairs_file_without_a_table_is_refused_by_its_one_parse(F, capsys, cli, files, extra):
    from mustache_amd import diff_mustache, mustache, pairs
    main = mustache.main if cli == "m" else diff_mustache.main
    pairs.close_pairs_handles()
    before = pairs.PairsFile.OPENS
    try:
        main(_argv(F, cli, files, extra.split(), "100"))
        said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Error:")]
        assert len(said) == 1 and "#chromsize" in said[0] and F["bare"] in said[0], said
        # the files before the offending one were parsed once each, with their trans rows; the offending one opened none
        assert pairs.PairsFile.OPENS == before + list(files).index("bare")
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    assert not any(os.path.exists(F["out"] + suf) for suf in ("", ".loop1", ".diffloop1", ".loop2", ".diffloop2"))
