"""--coarser-genome end to end on the MI355X: a three-chromosome genome at r = 10 kb with R = 20 kb, bins (360, 280, 40), integer
counts.  The cis bands and the two small pairs are balance_genome_reference.synth_call_genome's; the pair (0, 1) is
trans_reference.synth_trans(360, 280, density=1.0, nloops=4, seed=41) plus two weak wide blobs 3 exp(-d^2 / (2 5^2)) at
(70, 70) and (281, 141), drawn as default_rng(141).poisson(0.5 m): 41 665 records at 10 kb and 22 194 at 20 kb.  Through the CPU
restatements alone, WITH the genome's NEWTON bias applied (genome_bias + balanced + trans_loops, st 0.88, pt 0.2, octaves
[1.6, 3.2]), it gives 3 loops at 10 kb -- (64, 250), (81, 100), (99, 136) -- and 6 at 20 kb, of which the merge at M = 2 keeps
3 -- (35, 35), (100, 50), (140, 71): the two blobs show at 20 kb only -- and drops 3; the fixture asserts the conditions the
test needs before anything runs on the GPU.

The `.hic` file holds BOTH zooms (the 20 kb records come from the restatement, tests/coarsen_genome_reference.py), the pairs
file the reads.  The yardstick of the command line is existing behaviour: the plain `-r 10kb` and `-r 20kb` runs."""
import gzip
import re
import sys

import numpy as np
import pytest

import balance_genome_reference as gr
import coarsen_genome_reference as cg
import downsample_genome_reference as gref
import multires_reference as mr
import pairs_trans_reference as ptr
import trans_reference as tr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

RES, COARSE = 10000, 20000
BINS = (360, 280, 40)
NAMES = ["1", "2", "3"]
LENGTHS = [b * RES - 1 for b in BINS]
PAIRS = [("1", "2"), ("1", "3"), ("2", "3")]
RUN = ["--trans-all", "--balance-genome", "NEWTON", "-r", "10kb"]
LINE = re.compile(r"^multires (\S+): (\d+) bp: (\d+) of (\d+) loops kept \(merge distance (\d+) bins\)$", re.M)
FOUND = re.compile(r"^(\d+) loops found for chrmosome pair=(\S+) at (\d+) bp, fdr<", re.M)


def _pair01():
    x, y, v = tr.synth_trans(360, 280, density=1.0, nloops=4, seed=41)
    m = np.zeros((360, 280))
    m[x, y] = v
    ii, jj = np.meshgrid(np.arange(360), np.arange(280), indexing="ij")
    for cx, cy in ((70, 70), (281, 141)):
        m += 3.0 * np.exp(-((ii - cx) ** 2 + (jj - cy) ** 2) / (2 * 5.0 ** 2))
    cnt = np.random.default_rng(141).poisson(0.5 * m)
    k = cnt > 0
    return ii[k], jj[k], cnt[k].astype(np.float64)


def _full_cis(cis, k):
    """every cis pixel at k r, the diagonals below 2 included: what a file's zoom at R holds"""
    out = {}
    for c, (i, j, v) in cis.items():
        X, D, C = mr.coarsen(i, j - i, v, k)
        out[c] = (X, X + D, C.astype(np.float64))
    return out


def _write_hic(path, cis, trans, both=True):
    chroms, mats = gr.hic_arguments(BINS, RES, cis, trans)
    if both:
        for c, rec in _full_cis(cis, 2).items():
            mats[(c + 1, c + 1)][COARSE] = rec
        for (a, b), rec in cg.coarsen_genome(LENGTHS, RES, cis, trans, 2)[1].items():
            mats[(a + 1, b + 1)][COARSE] = rec
    write_hic_pairs(str(path), chroms, mats, version=8)
    return str(path)


def _write_pairs(path, cis, trans, seed):
    text, _ = ptr.pairs_text(NAMES, LENGTHS, RES, cis, trans, seed)
    with open(str(path), "wb") as fh:
        fh.write(gzip.compress(text.encode(), 1))
    return str(path)


def _cpu_loops(cis, trans, res):
    bins, off, _ = gr.layout(LENGTHS, res)
    bias, _ = gr.genome_bias("NEWTON", bins, off, cis, trans, "all")
    return tr.trans_loops(*gr.balanced(bias, off[0], off[1], *trans[(0, 1)]), 0.88, 0.2, [1.6, 3.2])


def _main(argv):
    from mustache_amd import pairs
    from mustache_amd.mustache import main
    try:
        main(argv)
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()


@pytest.fixture(scope="module")
def G(tmp_path_factory):
    d = tmp_path_factory.mktemp("coarsen_genome_cli")
    cis, trans = gr.synth_call_genome(_pair01(), seed=7, bins=BINS)
    coarse = cg.coarsen_genome(LENGTHS, RES, cis, trans, 2)
    # the conditions of the test, through the CPU restatements alone
    fine_loops, coarse_loops = _cpu_loops(cis, trans, RES), _cpu_loops(*coarse, COARSE)
    kept = mr.merge([fine_loops, coarse_loops], [RES, COARSE], 2)[1]
    print("restatement: %d records at 10 kb, %d at 20 kb; %d loops at 10 kb, %d at 20 kb, %d kept"
          % (len(trans[(0, 1)][2]), len(coarse[1][(0, 1)][2]), len(fine_loops), len(coarse_loops), len(kept)))
    assert len(fine_loops) >= 1 and len(kept) >= 1 and len(coarse_loops) - len(kept) >= 1
    assert len(coarse[1][(0, 1)][2]) >= 10000
    out = dict(dir=d, cis=cis, trans=trans, coarse=coarse, hic=_write_hic(d / "g.hic", cis, trans),
               pairs=_write_pairs(d / "g.pairs.gz", cis, trans, 23))
    # the yardstick: the plain runs at either resolution, on the `.hic` file (existing behaviour)
    for tag, r in (("plain10", "10kb"), ("plain20", "20kb")):
        _main(["-f", out["hic"], "-o", str(d / tag), "--trans-all", "--balance-genome", "NEWTON", "-r", r])
        out[tag] = open(str(d / tag)).read()
    return out


def _sorted(rec):
    x, y, v = (np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in rec)
    o = np.lexsort((y, x))
    return x[o].astype(np.int64), y[o].astype(np.int64), v[o].astype(np.float64)


def _same_read(a, b):
    assert (a.bins, a.offsets, a.n, a.names, a.lengths, a.pixels, a.res) == (b.bins, b.offsets, b.n, b.names, b.lengths, b.pixels, b.res)
    assert sorted(a.records) == sorted(b.records) and sorted(p[0] for p in a.cis) == sorted(p[0] for p in b.cis)
    for key in a.records:
        assert all(np.array_equal(s, t) for s, t in zip(_sorted(a.records[key]), _sorted(b.records[key]))), key
    for (c, x, dd, v), (c2, x2, d2, v2) in zip(sorted(a.cis, key=lambda p: p[0]), sorted(b.cis, key=lambda p: p[0])):
        assert c == c2 and all(np.array_equal(s, t) for s, t in zip(_sorted((x, x + dd, v)), _sorted((x2, x2 + d2, v2)))), c


@pytest.mark.parametrize("pixels", ["all", "inter"])
@pytest.mark.parametrize("source", ["hic", "pairs"])
def test_coarsen_genome_equals_the_read_at_R(G, source, pixels):
    from mustache_amd import pairs
    from mustache_amd.balance_genome import coarsen_genome, read_genome, solve_genome
    try:
        fine = read_genome(G[source], RES, pixels)
        before = {key: tuple(t.clone() for t in rec) for key, rec in fine.records.items()}
        got, want = coarsen_genome(fine, 2), read_genome(G[source], COARSE, pixels)
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    assert got.res == COARSE and got.bins == [180, 140, 20] and len(got.cis) == (3 if pixels == "all" else 0)
    _same_read(got, want)
    # against the restatement too, and the fine read is left untouched
    for (a, b), rec in G["coarse"][1].items():
        assert all(np.array_equal(s, t) for s, t in zip(_sorted(got.records[(a, b)]), _sorted(rec)))
    for c, x, dd, v in got.cis:
        assert all(np.array_equal(s, t) for s, t in zip(_sorted((x, x + dd, v)), _sorted(G["coarse"][0][c])))
    assert fine.res == RES and fine.bins == list(BINS) and sorted(fine.records) == sorted(before)
    for key, rec in before.items():
        assert all(bool((s == t).all()) for s, t in zip(rec, fine.records[key]))
    # small batches give the same records
    small = coarsen_genome(fine, 2, max_records=20000)
    for key in got.records:
        assert all(np.array_equal(s, t) for s, t in zip(_sorted(small.records[key]), _sorted(got.records[key])))
    a, b = solve_genome(got, "NEWTON"), solve_genome(want, "NEWTON")
    assert a.bias.tobytes() == b.bias.tobytes() and a.info["records"] == b.info["records"]
    assert int(np.isfinite(a.bias).sum()) > 300


def _by_pair(text):
    lines = text.splitlines(keepends=True)
    assert lines[0] == mr.HEADER
    rows = {}
    for line in lines[1:]:
        f = line.split("\t")
        rows.setdefault((f[0], f[3]), []).append(line)
    return rows


def _concatenation(G):
    """pair by pair, the rows of the plain 10 kb run followed by the rows of the plain 20 kb run"""
    fine, coarse = _by_pair(G["plain10"]), _by_pair(G["plain20"])
    return mr.HEADER + "".join("".join(fine.get(p, []) + coarse.get(p, [])) for p in PAIRS)


def test_merge_distance_0_is_the_concatenation_of_the_plain_runs(G, tmp_path, capsys):
    fine, coarse = _by_pair(G["plain10"]), _by_pair(G["plain20"])
    assert len(fine.get(("1", "2"), [])) >= 1 and len(coarse.get(("1", "2"), [])) >= 2
    out = tmp_path / "m0.tsv"
    capsys.readouterr()
    _main(["-f", G["hic"], "-o", str(out), "--coarser-genome", "20kb", "--merge-distance", "0"] + RUN)
    said = capsys.readouterr().out
    assert "Error" not in said
    assert open(str(out)).read() == _concatenation(G)
    # one line per pair and resolution, one report line per pair and coarser resolution, one balancing per resolution
    found = [(int(n), p, int(r)) for n, p, r in FOUND.findall(said)]
    assert found == [(len(rows.get(p, [])), "%s,%s" % p, r) for r, rows in ((RES, fine), (COARSE, coarse)) for p in PAIRS]
    assert [(p, int(r), int(k), int(n), int(m)) for p, r, k, n, m in LINE.findall(said)] == \
        [("%s,%s" % p, COARSE, len(coarse.get(p, [])), len(coarse.get(p, [])), 0) for p in PAIRS]
    assert sum("NEWTON balancing of the genome (all pixels)" in ln for ln in said.splitlines()) == 2, said


def test_the_default_merge_and_both_sources(G, tmp_path, capsys):
    want, counts = cg.merge_tsv([G["plain10"], G["plain20"]], [RES, COARSE], 2, pair_order=PAIRS)
    kept12 = [c for c in counts if c[0] == "1,2"][0]
    print(counts)
    assert 1 <= kept12[2] < kept12[3]                               # something is kept and something is dropped
    assert want != _concatenation(G)
    outs = {}
    for tag, extra in (("hic", []), ("pairs", ["--pairs-trans"])):
        out = tmp_path / (tag + ".tsv")
        capsys.readouterr()
        _main(["-f", G[tag], "-o", str(out), "--coarser-genome", "20kb"] + RUN + extra)
        said = capsys.readouterr().out
        assert "Error" not in said
        assert [(p, int(r), int(k), int(n)) for p, r, k, n, m in LINE.findall(said) if int(m) == 2] == counts
        outs[tag] = open(str(out), "rb").read()
    assert outs["hic"].decode() == want
    assert outs["pairs"] == outs["hic"]
    # one pair alone: exactly that pair's rows of the --trans-all output
    one = tmp_path / "one.tsv"
    _main(["-f", G["hic"], "-o", str(one), "-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON", "-r", "10kb", "--coarser-genome", "20kb"])
    rows = want.splitlines(keepends=True)
    assert open(str(one)).read() == rows[0] + "".join(r for r in rows[1:] if r.split("\t")[0] == "1" and r.split("\t")[3] == "2")
    assert {int(r.split("\t")[2]) - int(r.split("\t")[1]) for r in rows[1:]} == {RES, COARSE}      # a row's resolution


def test_with_downsample_genome(G, tmp_path, capsys):
    tc, tt, totals = gref.thin_genome(NAMES, BINS, G["cis"], G["trans"], 1 << 31, seed=7, sample=0)
    thinned = _write_hic(tmp_path / "thinned.hic", tc, tt, both=False)
    want, got = tmp_path / "want.tsv", tmp_path / "got.tsv"
    _main(["-f", thinned, "-o", str(want), "--coarser-genome", "20kb"] + RUN)
    capsys.readouterr()
    _main(["-f", G["hic"], "-o", str(got), "--coarser-genome", "20kb", "--downsample-genome", "0.5", "--seed", "7"] + RUN)
    said = capsys.readouterr().out
    assert "Error" not in said and said.splitlines().count(gref.line(0, totals, 1 << 31, 7)) == 1
    assert open(str(got), "rb").read() == open(str(want), "rb").read()
    assert open(str(got)).read().startswith(mr.HEADER)


@pytest.mark.parametrize("where", ["trans", "cis"])
def test_a_float_count_ends_the_run_before_anything_is_written(G, tmp_path, capsys, where):
    cis, trans = dict(G["cis"]), dict(G["trans"])
    if where == "trans":
        x, y, v = trans[(1, 2)]
        trans[(1, 2)] = (x, y, np.where(np.arange(len(v)) == 5, 2.5, v))
        sentence = "Error: the genome holds an inter-chromosomal count that is not an integer between 0 and 4294967295"
    else:
        i, j, v = cis[1]
        cis[1] = (i, j, np.where(np.arange(len(v)) == int(np.argmax(j - i)), 7.5, v))       # a pixel far from the diagonal: it enters
        sentence = "Error: chromosome 2 holds a count that is not an integer between 0 and 4294967295"
    f = _write_hic(tmp_path / "float.hic", cis, trans, both=False)
    out = tmp_path / "out.tsv"
    capsys.readouterr()
    _main(["-f", f, "-o", str(out), "--coarser-genome", "20kb"] + RUN)
    said = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("Error:") for ln in said) == 1 and sum(ln.startswith(sentence) for ln in said) == 1, said
    assert not any("loops found" in ln for ln in said)              # nothing was called
    assert not out.exists()


def test_a_memory_refusal_ends_the_run_before_anything_is_written(G, tmp_path, capsys, monkeypatch):
    import torch
    real = torch.cuda.mem_get_info

    def little_for_the_coarsening(*args):
        if sys._getframe(1).f_code.co_name == "_check_coarsen_memory":
            return (1000, real(*args)[1])
        return real(*args)
    monkeypatch.setattr(torch.cuda, "mem_get_info", little_for_the_coarsening)
    out = tmp_path / "out.tsv"
    for pixels in ("all", "inter"):
        capsys.readouterr()
        _main(["-f", G["hic"], "-o", str(out), "--coarser-genome", "20kb", "--balance-pixels", pixels] + RUN)
        said = capsys.readouterr().out.splitlines()
        errors = [ln for ln in said if ln.startswith("Error:")]
        assert len(errors) == 1 and re.match(r"^Error: --balance-genome: coarsening \d+ pixels needs about \d+ bytes of device memory "
                                             r"beside the \d+ resident ones, 1000 bytes are free$", errors[0]), said
        assert not any("loops found" in ln for ln in said) and not out.exists()
