"""--coarser / --merge-distance end to end on the MI355X, at the geometry of tests/test_gpu_downsample_cli.py (600 and 450 bins
at 5 kb, -d 1000000, -pt 0.2, the synth_coo maps with planted loops).  The pairs file and the `.hic` file hold the 5 kb
resolution only.  The check that the feature does what it says: the output of `-r 5000 --coarser 10000` must be, byte for byte,
the restated merge (tests/multires_reference.py) of two plain --balance runs on the pairs file, at 5 kb and at 10 kb.

The maps: synth_coo seeds 31 (chr1, 14 planted loops) and 32 (chr2, 10 planted loops) at depth 200, the maps of
tests/test_gpu_downsample_cli.py; chosen on the GPU, where both plain runs of either chromosome call loops, the default merge
distance drops coarse loops (the planted loops show at both resolutions) and distance 0 keeps every coarse loop."""
import contextlib
import gzip
import io
import os
import re

import numpy as np
import pytest

import downsample_reference as thin_ref
import multires_reference as ref

pytestmark = pytest.mark.gpu

RES, COARSE = 5000, 10000
DIST = "1000000"
SIZES = {"chr1": 600, "chr2": 450}  # bins at 5 kb
SEEDS = {"chr1": (31, 14), "chr2": (32, 10)}
DEPTH = 200.0
LINE = re.compile(r"^multires (\S+): (\d+) bp: (\d+) of (\d+) loops kept \(merge distance (\d+) bins\)$", re.M)
THIN = re.compile(r"^downsample (\S+) \(sample (\d)\): (\d+) of (\d+) contacts kept, p = (\S+), seed (\d+)$", re.M)


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
    """one row per contact: a random position inside each 5 kb bin (1-based), either orientation, shuffled"""
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
    with open(path, "w") as f:
        f.write(head + "".join(lines))


def _write_hic(path, maps, scale=1.0):
    from hic_writer import write_hic
    chroms = [("All", 1000)] + [(c, SIZES[c] * RES) for c in maps]
    write_hic(path, chroms, {i + 1: {RES: (x, y, v.astype(np.float64) * scale)} for i, (x, y, v) in enumerate(maps.values())}, {},
              version=8, block_bin_count=200, float_counts=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("multires_cli")
    out = {"dir": str(d)}
    maps = {c: _map(SIZES[c], seed, nloops, DEPTH) for c, (seed, nloops) in SEEDS.items()}
    out["depth"] = {c: int(m[2].sum()) for c, m in maps.items()}
    for name in ("a.pairs", "a.pairs.gz", "a.hic", "half.pairs"):
        out[name] = str(d / name)
    _write_pairs(out["a.pairs"], maps, 7)
    _write_hic(out["a.hic"], maps)                                   # 5 kb is the only resolution the file stores
    with open(out["a.pairs"], "rb") as f, open(out["a.pairs.gz"], "wb") as g:
        data = f.read()
        g.write(gzip.compress(data[:len(data) // 3], 1) + gzip.compress(data[len(data) // 3:], 1))     # two members
    # what the restatement of the thinning keeps under --downsample 0.5 --seed 7, written as a pairs file of its own
    half, out["kept_half"] = {}, {}
    for c, (x, y, v) in maps.items():
        k = thin_ref.thin_counts(x, y, v, thin_ref.chromosome_tag(c), 1 << 31, 7, 0)
        half[c], out["kept_half"][c] = (x[k > 0], y[k > 0], k[k > 0]), int(k.sum())
    _write_pairs(out["half.pairs"], half, 17)
    return out


def _run(files, name, out, *extra):
    """mustache.main -> (the TSV's text, what was printed)"""
    from mustache_amd.mustache import main
    path = os.path.join(files["dir"], out)
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        main(["-f", files[name], "-d", DIST, "-o", path, "-pt", "0.2", "--balance", "ICE"] + list(extra))
    print(said.getvalue())
    with open(path) as f:
        return f.read(), said.getvalue()


@pytest.fixture(scope="module")
def plain(files):
    """the single-resolution runs on the pairs file: {(chromosome, resolution): TSV text}"""
    return {(c, r): _run(files, "a.pairs", "plain_%s_%d.tsv" % (c, r), "-r", str(r), "-ch", c)[0]
            for c in SIZES for r in (RES, COARSE)}


def _rows(text):
    return text.splitlines(keepends=True)[1:]


def test_the_plain_runs_leave_something_to_merge(plain):
    for c in SIZES:
        fine, coarse = plain[(c, RES)], plain[(c, COARSE)]
        want, counts = ref.merge_tsv([fine, coarse], (RES, COARSE), 2)
        apart, counts0 = ref.merge_tsv([fine, coarse], (RES, COARSE), 0)
        print(c, "loops at 5 kb:", len(_rows(fine)), "at 10 kb:", len(_rows(coarse)), "merged:", counts, "at distance 0:", counts0)
        assert len(_rows(fine)) >= 1 and len(_rows(coarse)) >= 1         # each plain run has a loop
        assert all(int(row.split("\t")[2]) - int(row.split("\t")[1]) == COARSE for row in _rows(coarse))
        (_, _, kept, called), (_, _, kept0, called0) = counts[0], counts0[0]
        assert called == called0 == len(_rows(coarse))
        assert kept < called                                             # the planted loops show at both resolutions
        assert kept0 >= 1
        assert kept0 == called0 and apart == fine + "".join(_rows(coarse))       # factor 2: no two centres coincide


@pytest.mark.parametrize("name", ["a.pairs", "a.pairs.gz", "a.hic"])
def test_the_merged_output_is_the_restated_merge_of_two_plain_runs(files, plain, name):
    want, counts = ref.merge_tsv([plain[("chr1", RES)], plain[("chr1", COARSE)]], (RES, COARSE), 2)
    got, said = _run(files, name, "merged_%s.tsv" % name, "-r", str(RES), "--coarser", str(COARSE), "-ch", "chr1")
    assert got == want
    assert LINE.findall(said) == [("chr1", str(COARSE), str(counts[0][2]), str(counts[0][3]), "2")]
    resolutions = {int(row.split("\t")[2]) - int(row.split("\t")[1]) for row in _rows(got)}
    assert resolutions <= {RES, COARSE} and RES in resolutions
    if name == "a.pairs":
        from mustache_amd.pairs import PairsFile, close_pairs_handles
        close_pairs_handles()
        before = PairsFile.OPENS
        again, _ = _run(files, name, "merged_again.tsv", "-r", "5kb", "--coarser", "10kb", "-ch", "chr1")
        assert again == want and PairsFile.OPENS == before + 1           # both resolutions from one parse of the file


def test_merge_distance_zero_is_the_concatenation(files, plain):
    got, said = _run(files, "a.hic", "apart.tsv", "-r", str(RES), "--coarser", "10kb", "--merge-distance", "0", "-ch", "chr1")
    called = len(_rows(plain[("chr1", COARSE)]))
    assert got == plain[("chr1", RES)] + "".join(_rows(plain[("chr1", COARSE)]))
    assert LINE.findall(said) == [("chr1", str(COARSE), str(called), str(called), "0")] and called >= 1
    # a distance in between merges less than the default
    one, said = _run(files, "a.pairs", "one.tsv", "-r", str(RES), "--coarser", "10kb", "--merge-distance", "1", "-ch", "chr1")
    want, counts = ref.merge_tsv([plain[("chr1", RES)], plain[("chr1", COARSE)]], (RES, COARSE), 1)
    assert one == want and LINE.findall(said) == [("chr1", str(COARSE), str(counts[0][2]), str(counts[0][3]), "1")]


def test_a_run_on_both_chromosomes_writes_both(files, plain):
    want = ref.HEADER
    lines = []
    for c in SIZES:
        text, counts = ref.merge_tsv([plain[(c, RES)], plain[(c, COARSE)]], (RES, COARSE), 2)
        want += "".join(_rows(text))
        lines += [(c, str(r), str(kept), str(called), "2") for _, r, kept, called in counts]
    for name in ("a.pairs", "a.hic"):
        got, said = _run(files, name, "both_%s.tsv" % name, "-r", str(RES), "--coarser", str(COARSE))
        assert got == want, name
        assert LINE.findall(said) == lines
        assert {row.split("\t")[0] for row in _rows(got)} == {"chr1", "chr2"}


def test_with_downsample_every_resolution_sees_the_same_kept_reads(files):
    got, said = _run(files, "a.pairs", "thin.tsv", "-r", str(RES), "--coarser", str(COARSE), "--downsample", "0.5", "--seed", "7")
    assert THIN.findall(said) == [(c, "1", str(files["kept_half"][c]), str(files["depth"][c]), "0.5", "7") for c in SIZES]
    want, plain_said = _run(files, "half.pairs", "thin_plain.tsv", "-r", str(RES), "--coarser", str(COARSE))
    assert not THIN.findall(plain_said)
    assert got == want and len(_rows(got)) >= 1
    assert LINE.findall(said) == LINE.findall(plain_said) and len(LINE.findall(said)) == 2
    hic, hic_said = _run(files, "a.hic", "thin_hic.tsv", "-r", str(RES), "--coarser", str(COARSE), "--downsample", "0.5", "--seed", "7")
    assert hic == want and THIN.findall(hic_said) == THIN.findall(said)


def test_a_hic_file_of_fractional_counts_is_refused(files, tmp_path, capsys):
    x, y, v = _map(SIZES["chr2"], 32, 10, 100.0)
    path = str(tmp_path / "frac.hic")
    _write_hic(path, {"chr2": (x, y, v)}, scale=0.5)
    from mustache_amd.mustache import main
    out = str(tmp_path / "frac.tsv")
    main(["-f", path, "-r", str(RES), "-d", DIST, "-o", out, "-ch", "chr2", "--balance", "ICE", "--coarser", "10kb"])
    said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Error:")]
    assert len(said) == 1 and "chr2" in said[0] and "not an integer" in said[0], said
    assert not os.path.exists(out)
