"""`.pairs` input end to end on the MI355X: `python -m mustache_amd -f x.pairs --balance ...` and diff_mustache's -f1 / -f2
against the same contacts aggregated into a `.hic` file -- the outputs must be byte-identical, since from the pixel set onward
both inputs run the same code (balance.balance_records_device)."""
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES = 5000
DIST = "1000000"                    # 200 bins: the smallest -d the command line accepts at this resolution
SIZES = {"chr1": 600, "chr2": 450}  # bins


def _map(n, seed, nloops):
    """integer counts near the diagonal with planted loops, plus sparse long-range pixels (all far below 2^24)"""
    from mustache_amd.synth import synth_coo
    x, y, v = synth_coo(n, 100, depth=100.0, seed=seed, nloops=nloops)
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    far = np.abs(a - b) > 105
    fx, fy = np.minimum(a, b)[far], np.maximum(a, b)[far]
    _, first = np.unique(fx * n + fy, return_index=True)
    x = np.concatenate([np.asarray(x), fx[first]])
    y = np.concatenate([np.asarray(y), fy[first]])
    v = np.concatenate([np.maximum(np.round(np.asarray(v)), 1.0), rng.integers(1, 4, len(first)).astype(np.float64)])
    return x.astype(np.int64), y.astype(np.int64), v


def _pairs_text(maps, seed):
    """one row per contact: a random position inside each bin (1-based), either orientation, shuffled; trans rows and rows of
    a chromosome the header does not name in between"""
    rng = np.random.default_rng(seed)
    head = "## pairs format v1.0\n" + "".join("#chromsize: %s %d\n" % (c, SIZES[c] * RES) for c in maps) + \
           "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
    names, p1, p2 = [], [], []
    for c, (x, y, v) in maps.items():
        reps = v.astype(np.int64)
        bx, by = np.repeat(x, reps), np.repeat(y, reps)
        a = bx * RES + rng.integers(1, RES + 1, len(bx))
        b = by * RES + rng.integers(1, RES + 1, len(by))
        swap = rng.random(len(a)) < 0.5
        p1.append(np.where(swap, b, a))
        p2.append(np.where(swap, a, b))
        names.append(np.full(len(a), c))
    names, p1, p2 = np.concatenate(names), np.concatenate(p1), np.concatenate(p2)
    order = rng.permutation(len(p1))
    lines = ["r\t%s\t%d\t%s\t%d\t+\t-\n" % (c, a, c, b) for c, a, b in zip(names[order].tolist(), p1[order].tolist(), p2[order].tolist())]
    extra = ["t\tchr1\t77\tchr2\t99\t+\t-\n", "u\tchrM\t5\tchrM\t9\t+\t-\n", "o\tchr1\t0\tchr1\t5\t+\t-\n"]
    for k, e in enumerate(extra):
        lines.insert((k + 1) * len(lines) // 4, e)
    return head + "".join(lines), len(lines)


def _hic(path, maps):
    from hic_writer import write_hic
    chroms = [("All", 1000)] + [(c, SIZES[c] * RES) for c in maps]
    write_hic(path, chroms, {i + 1: {RES: m} for i, m in enumerate(maps.values())}, {}, version=8, block_bin_count=200,
              float_counts=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs_cli")
    out = {"dir": str(d)}
    samples = {"a": {"chr1": _map(SIZES["chr1"], 31, 14), "chr2": _map(SIZES["chr2"], 32, 10)},
               "b": {"chr1": _map(SIZES["chr1"], 41, 14)}}                  # the second sample of the two-sample run
    for tag, maps in samples.items():
        text, rows = _pairs_text(maps, 7)
        out[tag + ".pairs"], out[tag + ".hic"] = str(d / (tag + ".pairs")), str(d / (tag + ".hic"))
        with open(out[tag + ".pairs"], "w") as f:
            f.write(text)
        out[tag + ".rows"] = rows
        _hic(out[tag + ".hic"], maps)
        assert max(float(m[2].max()) for m in maps.values()) < 1 << 24
    out["a.pairs.gz"] = str(d / "a.pairs.gz")
    with open(out["a.pairs"], "rb") as f, open(out["a.pairs.gz"], "wb") as g:
        data = f.read()
        g.write(gzip.compress(data[:len(data) // 3], 1) + gzip.compress(data[len(data) // 3:], 1))     # two members
    return out


def _run(files, name, out, *extra):
    from mustache_amd.mustache import main
    path = os.path.join(files["dir"], out)
    main(["-f", files[name], "-r", str(RES), "-d", DIST, "-o", path, "-pt", "0.2"] + list(extra))
    with open(path) as f:
        return f.read()


@pytest.mark.parametrize("method", ["ICE", "NEWTON"])
def test_pairs_equal_hic(files, method, capsys):
    want = _run(files, "a.hic", "hic_%s.tsv" % method, "-ch", "chr1", "--balance", method)
    capsys.readouterr()
    got = _run(files, "a.pairs", "pairs_%s.tsv" % method, "-ch", "chr1", "--balance", method)
    said = capsys.readouterr().out
    assert got == want
    assert want.count("\n") > 1                              # a header and at least one loop: the comparison shows something
    assert "%d rows read" % files["a.rows"] in said and "1 trans, 1 out of range" in said, said
    gz = _run(files, "a.pairs.gz", "gz_%s.tsv" % method, "-ch", "chr1", "--balance", method)
    assert gz == want


def test_every_chromosome_in_header_order_from_one_parse(files, capsys):
    from mustache_amd import pairs
    pairs.close_pairs_handles()
    before = pairs.PairsFile.OPENS
    got = _run(files, "a.pairs", "all_pairs.tsv", "--balance", "ICE")
    assert pairs.PairsFile.OPENS == before + 1               # the file was parsed once for both chromosomes
    want = _run(files, "a.hic", "all_hic.tsv", "--balance", "ICE")
    assert got == want
    chroms = [line.split("\t")[0] for line in got.splitlines()[1:]]
    assert "chr1" in chroms and "chr2" in chroms
    assert chroms == sorted(chroms, key=["chr1", "chr2"].index)            # header order


def test_zero_based_positions(files, tmp_path):
    """the same contacts written 0-based and read with --pairs-zero-based give the same loops"""
    shifted = str(tmp_path / "z.pairs")
    with open(files["a.pairs"]) as f, open(shifted, "w") as g:
        for line in f:
            if line.startswith("#"):
                g.write(line)
                continue
            c = line.split("\t")
            c[2], c[4] = str(int(c[2]) - 1), str(int(c[4]) - 1)
            g.write("\t".join(c))
    files = dict(files, **{"z.pairs": shifted})
    want = _run(files, "a.pairs", "one_based.tsv", "-ch", "chr2", "--balance", "ICE")
    got = _run(files, "z.pairs", "zero_based.tsv", "-ch", "chr2", "--balance", "ICE", "--pairs-zero-based")
    assert got == want and want.count("\n") > 1


def test_diff_mustache_pairs_equal_hic(files):
    from mustache_amd.diff_mustache import SUFFIX, main
    outs = {}
    for kind in ("pairs", "hic"):
        out = os.path.join(files["dir"], "diff_" + kind)
        main(["-f1", files["a." + kind], "-f2", files["b." + kind], "-r", str(RES), "-d", DIST, "-ch", "chr1", "-o", out,
              "--balance", "ICE"])
        outs[kind] = [open(out + suf).read() for suf in SUFFIX.values()]
    assert len(outs["pairs"]) == 4 and outs["pairs"] == outs["hic"]
    assert sum(t.count("\n") - 1 for t in outs["hic"][:2]) > 0             # the two samples' own loop lists are not empty
