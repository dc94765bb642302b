"""--downsample / --seed / --match-depth end to end on the MI355X, at the geometry of tests/test_gpu_pairs_cli.py (600 and 450
bins at 5 kb, -d 1000000, -pt 0.2) with synthetic depth 200: the half-depth map is then the depth-100 map that file shows to
yield loops.  The check that the feature does what it says: the NumPy restatement (tests/downsample_reference.py) thins the
pixel sets and writes them as a new pairs file, one row per kept read, and a plain --balance run on that file must give the
same bytes as the thinned run on the full file."""
import gzip
import os
import re

import numpy as np
import pytest

import downsample_reference as ref

pytestmark = pytest.mark.gpu

RES = 5000
DIST = "1000000"
SIZES = {"chr1": 600, "chr2": 450}  # bins
LINE = re.compile(r"^downsample (\S+) \(sample (\d)\): (\d+) of (\d+) contacts kept, p = (\S+), seed (\d+)$", re.M)


def _map(n, seed, nloops, depth):
    """integer counts near the diagonal with planted loops, plus sparse long-range pixels"""
    from mustache_amd.synth import synth_coo
    x, y, v = synth_coo(n, 100, depth=depth, seed=seed, nloops=nloops)
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    far = np.abs(a - b) > 105
    fx, fy = np.minimum(a, b)[far], np.maximum(a, b)[far]
    _, first = np.unique(fx * n + fy, return_index=True)
    x = np.concatenate([np.asarray(x), fx[first]])
    y = np.concatenate([np.asarray(y), fy[first]])
    v = np.concatenate([np.maximum(np.round(np.asarray(v)), 1.0), rng.integers(1, 4, len(first)).astype(np.float64)])
    return x.astype(np.int64), y.astype(np.int64), v.astype(np.int64)


def _write_pairs(path, maps, seed):
    """one row per contact: a random position inside each bin (1-based), either orientation, shuffled; a trans row, a row of a
    chromosome the header does not name and a row out of range in between"""
    rng = np.random.default_rng(seed)
    head = "## pairs format v1.0\n" + "".join("#chromsize: %s %d\n" % (c, SIZES[c] * RES) for c in maps) + \
           "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
    names, p1, p2 = [], [], []
    for c, (x, y, v) in maps.items():
        bx, by = np.repeat(x, v), np.repeat(y, v)
        a = bx * RES + rng.integers(1, RES + 1, len(bx))
        b = by * RES + rng.integers(1, RES + 1, len(by))
        swap = rng.random(len(a)) < 0.5
        p1.append(np.where(swap, b, a))
        p2.append(np.where(swap, a, b))
        names.append(np.full(len(a), c))
    names, p1, p2 = np.concatenate(names), np.concatenate(p1), np.concatenate(p2)
    order = rng.permutation(len(p1))
    lines = ["r\t%s\t%d\t%s\t%d\t+\t-\n" % (c, a, c, b) for c, a, b in zip(names[order].tolist(), p1[order].tolist(), p2[order].tolist())]
    for k, e in enumerate(["t\tchr1\t77\tchr2\t99\t+\t-\n", "u\tchrM\t5\tchrM\t9\t+\t-\n", "o\tchr1\t0\tchr1\t5\t+\t-\n"]):
        lines.insert((k + 1) * len(lines) // 4, e)
    with open(path, "w") as f:
        f.write(head + "".join(lines))


def _write_hic(path, maps):
    from hic_writer import write_hic
    chroms = [("All", 1000)] + [(c, SIZES[c] * RES) for c in maps]
    write_hic(path, chroms, {i + 1: {RES: (x, y, v.astype(np.float64))} for i, (x, y, v) in enumerate(maps.values())}, {}, version=8,
              block_bin_count=200, float_counts=True)


def _thinned(maps, T, seed, sample):
    """the restatement on every chromosome of `maps`: {chromosome: (x, y, k)} of the pixels with k > 0, and the kept totals"""
    out, kept = {}, {}
    for c, (x, y, v) in maps.items():
        k = ref.thin_counts(x, y, v, ref.chromosome_tag(c), T, seed, sample)
        out[c], kept[c] = (x[k > 0], y[k > 0], k[k > 0]), int(k.sum())
    return out, kept


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("downsample_cli")
    out = {"dir": str(d)}
    a = {"chr1": _map(SIZES["chr1"], 31, 14, 200.0), "chr2": _map(SIZES["chr2"], 32, 10, 200.0)}
    b = {"chr1": _map(SIZES["chr1"], 41, 14, 100.0)}                         # the second sample, at half the depth
    out["depth"] = {"a": {c: int(m[2].sum()) for c, m in a.items()}, "b": {c: int(m[2].sum()) for c, m in b.items()}}
    for tag, maps in (("a", a), ("b", b)):
        out[tag + ".pairs"], out[tag + ".hic"] = str(d / (tag + ".pairs")), str(d / (tag + ".hic"))
        _write_pairs(out[tag + ".pairs"], maps, 7)
        _write_hic(out[tag + ".hic"], maps)
    out["a.pairs.gz"] = str(d / "a.pairs.gz")
    with open(out["a.pairs"], "rb") as f, open(out["a.pairs.gz"], "wb") as g:
        data = f.read()
        g.write(gzip.compress(data[:len(data) // 3], 1) + gzip.compress(data[len(data) // 3:], 1))     # two members
    # what the restatement keeps: --downsample 0.5 --seed 7 (and --seed 8: the totals only), and --match-depth on chr1 with a
    # as -f1 (sample 0) and as -f2 (sample 1)
    half, out["kept_half"] = _thinned(a, 1 << 31, 7, 0)
    _, out["kept_seed8"] = _thinned(a, 1 << 31, 8, 0)
    na, nb = out["depth"]["a"]["chr1"], out["depth"]["b"]["chr1"]
    assert nb < na
    out["T_match"] = (nb << 32) // na
    out["half.pairs"] = str(d / "half.pairs")
    _write_pairs(out["half.pairs"], half, 17)
    for sample in (0, 1):
        thin, kept = _thinned({"chr1": a["chr1"]}, out["T_match"], 0, sample)
        out["matched%d.pairs" % sample], out["kept_match%d" % sample] = str(d / ("matched%d.pairs" % sample)), kept["chr1"]
        _write_pairs(out["matched%d.pairs" % sample], thin, 27 + sample)
    return out


def _run(files, name, out, *extra):
    from mustache_amd.mustache import main
    path = os.path.join(files["dir"], out)
    main(["-f", files[name], "-r", str(RES), "-d", DIST, "-o", path, "-pt", "0.2"] + list(extra))
    with open(path) as f:
        return f.read()


def _diff(files, f1, f2, out, *extra):
    from mustache_amd.diff_mustache import SUFFIX, main
    path = os.path.join(files["dir"], out)
    main(["-f1", files[f1], "-f2", files[f2], "-r", str(RES), "-d", DIST, "-ch", "chr1", "-o", path, "--balance", "ICE"] + list(extra))
    return [open(path + suf).read() for suf in SUFFIX.values()]


@pytest.fixture(scope="module")
def half_runs(files):
    """--downsample 0.5 --seed 7 --balance ICE on chr1 of the pairs file, its .gz and the .hic: {name: (tsv, printed lines)}"""
    import contextlib
    import io
    got = {}
    for name in ("a.pairs", "a.pairs.gz", "a.hic"):
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            tsv = _run(files, name, "half_%s.tsv" % name, "-ch", "chr1", "--balance", "ICE", "--downsample", "0.5", "--seed", "7")
        got[name] = (tsv, LINE.findall(said.getvalue()))
    return got


def test_three_inputs_one_result(files, half_runs):
    want = ("chr1", "1", str(files["kept_half"]["chr1"]), str(files["depth"]["a"]["chr1"]), "0.5", "7")
    for name, (tsv, lines) in half_runs.items():
        print(name, lines)
        assert lines == [want], name                             # one line, and the totals are the restatement's
        assert tsv == half_runs["a.pairs"][0], name


def test_the_thinned_run_equals_a_plain_run_on_the_thinned_file(files, half_runs, capsys):
    want = _run(files, "half.pairs", "plain_half.tsv", "-ch", "chr1", "--balance", "ICE")
    said = capsys.readouterr().out
    assert not LINE.findall(said) and "%d kept" % files["kept_half"]["chr1"] in said, said
    assert want.count("\n") > 1                                  # a header and at least one loop
    assert half_runs["a.pairs"][0] == want
    full = _run(files, "a.pairs", "full.tsv", "-ch", "chr1", "--balance", "ICE")
    assert full != want                                          # and the thinning changed the result


def test_another_seed_and_every_chromosome(files, capsys):
    _run(files, "a.hic", "seed8.tsv", "-ch", "chr1", "--balance", "ICE", "--downsample", "0.5", "--seed", "8")
    lines = LINE.findall(capsys.readouterr().out)
    assert lines == [("chr1", "1", str(files["kept_seed8"]["chr1"]), str(files["depth"]["a"]["chr1"]), "0.5", "8")]
    assert files["kept_seed8"]["chr1"] != files["kept_half"]["chr1"]
    both = {}
    for name in ("a.pairs", "a.hic"):
        both[name] = _run(files, name, "both_%s.tsv" % name, "--balance", "ICE", "--downsample", "0.5", "--seed", "7")
        lines = LINE.findall(capsys.readouterr().out)
        assert lines == [(c, "1", str(files["kept_half"][c]), str(files["depth"]["a"][c]), "0.5", "7") for c in ("chr1", "chr2")], name
    assert both["a.pairs"] == both["a.hic"]
    chroms = {line.split("\t")[0] for line in both["a.hic"].splitlines()[1:]}
    assert chroms == {"chr1", "chr2"}
    # without --seed the seed is 0
    _run(files, "a.hic", "seed0.tsv", "-ch", "chr2", "--balance", "NEWTON", "--downsample", "0.25")
    (line,) = LINE.findall(capsys.readouterr().out)
    assert line[0] == "chr2" and line[4:] == ("0.25", "0")
    assert int(line[2]) == _thinned({"chr2": _map(SIZES["chr2"], 32, 10, 200.0)}, 1 << 30, 0, 0)[1]["chr2"]


@pytest.mark.parametrize("a_is", [1, 2])
def test_match_depth(files, capsys, a_is):
    """sample a (depth 200, a pairs file) against sample b (depth 100, a .hic file): a is the one thinned, whichever argument
    it is, with its place in the key"""
    sample = a_is - 1
    order = ("a.pairs", "b.hic") if a_is == 1 else ("b.hic", "a.pairs")
    got = _diff(files, *order, "match%d" % a_is, "--match-depth")
    lines = LINE.findall(capsys.readouterr().out)
    na = files["depth"]["a"]["chr1"]
    assert lines == [("chr1", str(a_is), str(files["kept_match%d" % sample]), str(na), repr(files["T_match"] / 4294967296), "0")]
    plain = tuple(("matched%d.pairs" % sample) if f == "a.pairs" else f for f in order)
    want = _diff(files, *plain, "plain_match%d" % a_is)
    assert not LINE.findall(capsys.readouterr().out)
    assert len(got) == 4 and got == want
    assert sum(t.count("\n") - 1 for t in (got[0], got[2])) > 0              # the two samples' own loop lists are not empty
    if a_is == 1:
        unmatched = _diff(files, *order, "unmatched")
        assert unmatched != got


def test_match_depth_of_equal_depths_thins_neither(files, capsys):
    got = _diff(files, "b.hic", "b.hic", "same_matched", "--match-depth", "--seed", "5")
    assert not LINE.findall(capsys.readouterr().out)
    want = _diff(files, "b.hic", "b.hic", "same_plain")
    assert got == want and got[0].count("\n") > 1
    # the same contacts as a pairs file: equal depths again
    got = _diff(files, "b.pairs", "b.hic", "same_formats", "--match-depth")
    assert not LINE.findall(capsys.readouterr().out) and got == want


def test_a_hic_file_of_fractional_counts_is_refused(files, tmp_path, capsys):
    x, y, v = _map(SIZES["chr2"], 32, 10, 100.0)
    path = str(tmp_path / "frac.hic")
    from hic_writer import write_hic
    write_hic(path, [("All", 1000), ("chr2", SIZES["chr2"] * RES)], {1: {RES: (x, y, v.astype(np.float64) * 0.5)}}, {}, version=8,
              block_bin_count=200, float_counts=True)
    from mustache_amd.mustache import main
    out = str(tmp_path / "frac.tsv")
    main(["-f", path, "-r", str(RES), "-d", DIST, "-o", out, "-ch", "chr2", "--balance", "ICE", "--downsample", "0.5"])
    said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Error:")]
    assert len(said) == 1 and "chr2" in said[0] and "not an integer" in said[0], said
    assert not os.path.exists(out)
