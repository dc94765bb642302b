"""What `python -m mustache_amd.pileup` refuses around --balance-genome / --balance-pixels / --pairs-trans / --pairs-zero-based:
every refusal is exactly one `Error:` line and no output file, decided before anything is read and before the GPU is touched
(`_lib.require_gpu` raises here, so a refusal that reached the device fails).  No GPU."""
import os

import pytest

HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"
GENOME = ["--balance-genome", "NEWTON"]


@pytest.fixture()
def files(tmp_path, monkeypatch):
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    out = {}
    for name in ("m.hic", "m.cool", "m.mcool", "m.txt", "m.pairs", "m.pairs.gz", "bias.txt"):
        out[name] = str(tmp_path / name)
        with open(out[name], "wb") as fh:
            fh.write(b"not read\n")                          # a refusal comes before any read
    out["loops"] = str(tmp_path / "l.tsv")
    with open(out["loops"], "w") as fh:
        fh.write(HEADER + "\n1\t100000\t110000\t2\t200000\t210000\t0.01\t1.6\n")
    out["dir"] = tmp_path
    return out


CASES = [
    ("m.hic", GENOME, "--balance-genome without --trans"),
    ("m.hic", ["--trans", "--balance", "ICE"] + GENOME, "--balance does not apply to inter-chromosomal pairs"),
    ("m.hic", ["--balance", "ICE"] + GENOME, "--balance-genome without --trans"),
    ("m.hic", ["--trans", "-b", "bias.txt"] + GENOME, "--balance-genome NEWTON and a bias file"),
    ("m.hic", ["--trans", "-norm", "KR"] + GENOME, "--balance-genome NEWTON and -norm KR"),
    ("m.cool", ["--trans"] + GENOME, ".cool/.mcool files carry their own `weight` column"),
    ("m.mcool", ["--trans"] + GENOME, ".cool/.mcool files carry their own `weight` column"),
    ("m.txt", ["--trans"] + GENOME, "Interchromosomal analysis is only supported for .hic and .cool input formats."),
    ("m.hic", ["--trans", "--balance-pixels", "inter"], "--balance-pixels inter without --balance-genome"),
    ("m.hic", ["--balance-pixels", "all"], "--balance-pixels all without --balance-genome"),
    ("m.hic", ["--trans", "--balance-genome", "KR"], "--balance-genome KR: unknown method"),
    ("m.hic", ["--trans", "--balance-pixels", "cis"] + GENOME, "--balance-pixels cis: unknown value"),
    ("m.pairs", ["--trans"], "m.pairs without --pairs-trans"),
    ("m.pairs.gz", ["--trans"] + GENOME, "m.pairs.gz without --pairs-trans"),
    ("m.pairs", GENOME, "m.pairs without --pairs-trans"),
    ("m.pairs", ["--trans", "--pairs-trans"], "--pairs-trans without --balance-genome"),
    ("m.pairs", ["--pairs-trans"] + GENOME, "--balance-genome without --trans"),
    ("m.hic", ["--trans", "--pairs-trans"] + GENOME, "--pairs-trans is for .pairs / .pairs.gz input"),
    ("m.cool", ["--trans", "--pairs-trans"], "--pairs-trans is for .pairs / .pairs.gz input"),
    ("m.hic", ["--trans", "--pairs-zero-based"] + GENOME, "--pairs-zero-based is for .pairs / .pairs.gz input"),
    ("m.pairs", ["--balance", "ICE", "--pairs-zero-based"], "--pairs-zero-based without --pairs-trans"),     # a cis pile-up would ignore it
    ("m.pairs.gz", ["--trans", "--pairs-zero-based"] + GENOME, "--pairs-zero-based without --pairs-trans"),
]


@pytest.mark.parametrize("name,extra,text", CASES, ids=["%s %s" % (c[0], " ".join(c[1])) for c in CASES])
def test_refusals_are_one_error_line_and_no_file(files, name, extra, text, capsys):
    from mustache_amd.pileup import main
    prefix = str(files["dir"] / "out")
    extra = [files["bias.txt"] if a == "bias.txt" else a for a in extra]
    main(["-f", files[name], "-l", files["loops"], "-r", "10kb", "-o", prefix] + extra)
    said = capsys.readouterr().out.splitlines()
    errors = [ln for ln in said if ln.startswith("Error:")]
    assert len(errors) == 1 and said == errors, said
    assert text in errors[0], errors[0]
    assert not [f for f in os.listdir(files["dir"]) if f.startswith("out")]


def test_the_parser_knows_the_flags_and_a_plain_request_asks_for_nothing():
    from mustache_amd.pileup import genome_request, parse_args
    base = ["-f", "m.hic", "-l", "l.tsv", "-r", "10kb", "-o", "o"]
    a = parse_args(base)
    assert a.balance_genome is None and a.balance_pixels == "all" and not a.balance_pixels_given
    assert not a.pairs_trans and not a.pairs_zero_based
    assert genome_request(a, "m.hic", 1) is None and genome_request(parse_args(base + ["--trans"]), "m.hic", 1) is None
    assert genome_request(parse_args(base + ["--balance", "ICE"]), "m.pairs", 1) is None     # a cis pile-up from a pairs file: as before
    a = parse_args(base + ["--trans", "--balance-genome", "ice", "--balance-pixels", "INTER"])
    assert genome_request(a, "m.hic", 1) == ("ICE", "inter")
    a = parse_args(["-f", "m.pairs.gz"] + base[2:] + ["--trans", "--pairs-trans", "--pairs-zero-based"] + GENOME)
    assert a.pairs_trans and a.pairs_zero_based and genome_request(a, "m.pairs.gz", 1) == ("NEWTON", "all")
