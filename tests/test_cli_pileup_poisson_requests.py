"""What `python -m mustache_amd.pileup` refuses around --poisson / --max-fdr: every refusal is exactly one `Error:` line and no
output file, decided before anything is read and before the GPU is touched (`_lib.require_gpu` raises here, so a refusal that
reached the device fails; the map files hold no map, so one that reached a reader fails too).  No GPU."""
import os

import pytest

HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"
OK = ["--enrich", "--poisson", "--balance", "NEWTON"]


@pytest.fixture()
def files(tmp_path, monkeypatch):
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    out = {}
    for name in ("m.hic", "m2.hic", "m.cool", "m.mcool", "m.txt", "m.pairs", "m.pairs.gz", "bias.txt"):
        out[name] = str(tmp_path / name)
        with open(out[name], "wb") as fh:
            fh.write(b"not read\n")                          # a refusal comes before any read
    out["loops"] = str(tmp_path / "l.tsv")
    with open(out["loops"], "w") as fh:
        fh.write(HEADER + "\n1\t100000\t110000\t1\t900000\t910000\t0.01\t1.6\n")
    out["dir"] = tmp_path
    return out


CASES = [
    ("m.hic", ["--poisson", "--balance", "NEWTON"], "--poisson without --enrich"),
    ("m.pairs", ["--poisson", "--balance", "ICE", "--max-fdr", "0.1"], "--poisson without --enrich"),
    ("m.hic", ["--enrich", "--poisson"], "--poisson without --balance ICE|NEWTON"),
    ("m.hic", ["--enrich", "--poisson", "-norm", "KR"], "--poisson without --balance ICE|NEWTON"),
    ("m.txt", ["--enrich", "--poisson", "-b", "bias.txt"], "--poisson without --balance ICE|NEWTON"),
    ("m.hic", OK + ["--trans"], "--poisson with --trans"),
    ("m.hic", ["--enrich", "--poisson", "--trans", "--balance-genome", "NEWTON"], "--poisson with --balance-genome"),
    ("m.hic", ["--poisson", "--balance", "NEWTON", "-f2", "m2.hic"], "--poisson without --enrich"),
    ("m.hic", OK + ["-f2", "m2.hic"], "-f2 with --enrich"),
    ("m.txt", OK, "--poisson on"),
    ("m.cool", ["--enrich", "--poisson"], "--poisson without --balance ICE|NEWTON"),
    ("m.hic", ["--enrich", "--balance", "NEWTON", "--max-fdr", "0.1"], "--max-fdr without --poisson"),
    ("m.hic", ["--max-fdr", "0.1"], "--max-fdr without --poisson"),
    ("m.hic", OK + ["--max-fdr", "0"], "--max-fdr 0.0: the threshold T must lie in (0, 1]"),
    ("m.hic", OK + ["--max-fdr", "1.5"], "--max-fdr 1.5: the threshold T must lie in (0, 1]"),
    ("m.pairs.gz", OK + ["--max-fdr", "nan"], "the threshold T must lie in (0, 1]"),
    ("m.hic", OK + ["--max-fdr", "-0.1"], "the threshold T must lie in (0, 1]"),
]


def _run(files, name, extra, capsys):
    from mustache_amd.pileup import main
    prefix = str(files["dir"] / "out")
    extra = [files[a] if a in ("bias.txt", "m2.hic") else a for a in extra]
    main(["-f", files[name], "-l", files["loops"], "-r", "10kb", "-o", prefix] + extra)
    said = capsys.readouterr().out.splitlines()
    errors = [ln for ln in said if ln.startswith("Error:")]
    assert len(errors) == 1 and said == errors, said
    assert not [f for f in os.listdir(files["dir"]) if f.startswith("out")]
    return errors[0]


@pytest.mark.parametrize("name,extra,text", CASES, ids=["%s %s" % (c[0], " ".join(c[1])) for c in CASES])
def test_refusals_are_one_error_line_and_no_file(files, name, extra, text, capsys):
    line = _run(files, name, extra, capsys)
    assert text in line, line


def test_a_cool_file_is_refused_whatever_comes_first(files, capsys):
    # --balance itself refuses .cool input; either way it is one line and nothing is read
    line = _run(files, "m.cool", OK, capsys)
    assert "--poisson on" in line or ".cool/.mcool" in line, line
    assert "--poisson on" in _run(files, "m.mcool", OK, capsys)


def test_a_multi_rank_run_is_refused(files, capsys, monkeypatch):
    from mustache_amd import pileup as pl, sharding
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))
    assert "2 ranks" in _run(files, "m.hic", OK, capsys)
    a = pl.parse_args(["-f", "m.hic", "-l", "l", "-r", "10kb", "-o", "o"] + OK)
    with pytest.raises(pl.PileupError, match="--poisson in a multi-rank run"):
        pl.poisson_request(a, "m.hic", 2)


def test_the_parser_knows_the_flags_and_a_plain_request_asks_for_nothing():
    from mustache_amd.pileup import PileupError, parse_args, pileup, poisson_request
    base = ["-f", "m.hic", "-l", "l.tsv", "-r", "10kb", "-o", "o"]
    a = parse_args(base)
    assert a.poisson is False and a.max_fdr is None and poisson_request(a, "m.hic", 1) == (False, None)
    assert poisson_request(parse_args(base + ["--enrich"]), "m.hic", 1) == (False, None)
    assert poisson_request(parse_args(base + OK), "m.hic", 1) == (True, None)
    assert poisson_request(parse_args(base + OK + ["--max-fdr", "1"]), "m.pairs.gz", 1) == (True, 1.0)
    a = parse_args(base + ["--enrich", "--poisson", "--balance", "ice", "--max-fdr", "0.05"])
    assert poisson_request(a, "m.pairs", 1) == (True, 0.05)
    with pytest.raises(PileupError, match="--poisson without --enrich"):          # the Python interface refuses alike, reading nothing
        pileup("m.hic", "no such list", 10000, balance="NEWTON", poisson=True)
    with pytest.raises(PileupError, match="--poisson without --balance"):
        pileup("m.hic", "no such list", 10000, peak=2, poisson=True)
