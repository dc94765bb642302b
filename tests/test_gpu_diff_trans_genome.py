"""Differential trans loops of many chromosome pairs in shared launches (mustache_amd/diff_trans_genome.py) on the MI355X:
every pair's rows equal the rows of that pair alone (tests/trans_pair_alone.py: the single-pair kernels, every tile pair, no
skip rule) -- under every launch grouping and batch partition,
over the joint extents of two samples, with tile pairs and whole pairs skipped below 10 000 tested records in either sample,
beside degenerate pairs, and through `diff_mustache --trans-all`.

The row counts stated below are those of the NumPy restatement (tests/diff_trans_reference.py on zscore_exact's values, st
0.88, pt 0.2, pt2 0.1, octaves [1.6, 3.2]) run once on the CPU, per tag 1..4."""
import itertools

import numpy as np
import pytest

import diff_trans_reference as dr
import trans_reference as tr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

OCT = [1.6, 3.2]
ST, PT, PT2 = 0.88, 0.2, 0.1
FDR_BOUND = 1e-9               # the project's stated p-value / FDR bound (as tests/test_gpu_diff_trans.py)
NONE = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))


def _rows(rows):
    return [[int(r[0]), int(r[1]), float(r[2]), float(r[3]), int(r[4])] for r in rows]


def _per_tag(rows):
    return [sum(1 for r in rows if r[4] == t) for t in (1, 2, 3, 4)]


def _alone(pairs, chunk):
    from trans_pair_alone import diff_pair_alone
    out = []
    for rec1, rec2 in pairs:
        out.append(_rows(diff_pair_alone(NONE if rec1 is None else rec1, NONE if rec2 is None else rec2, OCT, ST, PT, PT2,
                                         chunk=chunk)))
    return out


def _genome(pairs, **kw):
    from mustache_amd.diff_trans_genome import call_diff_trans_genome
    return [_rows(r) for r in call_diff_trans_genome(pairs, OCT, ST, PT, PT2, **kw)]


def _compare(got, ref):
    """coordinates, sigma and tags equal; fdr within FDR_BOUND"""
    assert len(ref) > 0, "the case should produce rows"
    assert [(int(r[0]), int(r[1]), int(r[4])) for r in got] == [(int(r[0]), int(r[1]), int(r[4])) for r in ref]
    assert [float(r[3]) for r in got] == [float(r[3]) for r in ref]
    for g, r in zip(got, ref):
        assert abs(float(g[2]) - float(r[2])) <= FDR_BOUND, (g, r)


# ---- the maps (NumPy only) ---------------------------------------------------------------------------------------------------
G1_BINS = [420, 300, 340, 360]
G1_COUNTS = [[11, 9, 14, 2], [8, 0, 6, 4], [10, 1, 9, 7], [11, 8, 12, 0], [8, 7, 11, 1], [11, 8, 13, 0]]   # the restatement, per tag


def g1_pairs():
    """six pairs of one tile pair each, C = 420, 420, 420, 340, 360, 360"""
    return [dr.synth_pair(G1_BINS[a], G1_BINS[b], density=0.3, nloops=14, seed=10 + k, added=5)
            for k, (a, b) in enumerate(itertools.combinations(range(4), 2))]


def joint_extent_pair():
    """sample 1 without its last 20 rows, sample 2 without its last 30 columns: n1 = 420 comes from sample 2, n2 = 300 from
    sample 1"""
    (x1, y1, v1), (x2, y2, v2) = dr.synth_pair(420, 300, density=0.3, nloops=14, seed=7, added=5)
    k1, k2 = x1 < 400, y2 < 270
    return (x1[k1], y1[k1], v1[k1]), (x2[k2], y2[k2], v2[k2])


JOINT_COUNTS = [6, 1, 9, 4]


def g2_pairs():
    """bins 900, 1200, 700 at tiles of 600: 2 x 3, 2 x 2 and 3 x 2 tile pairs; the middle pair is dense in sample 1 and holds
    a 0.02 share of its pixels in sample 2"""
    return [dr.synth_pair(900, 1200, density=0.3, nloops=30, seed=31, added=10),
            (tr.synth_trans(900, 700, density=0.3, nloops=20, seed=32), tr.synth_trans(900, 700, density=0.02, nloops=10, seed=33)),
            dr.synth_pair(1200, 700, density=0.3, nloops=30, seed=34, added=10)]


G2_COUNTS = [[22, 13, 23, 9], [0, 0, 0, 0], [22, 17, 23, 3]]


def _trimmed(rec, count, seed):
    """rec with background records (not the corner record) dropped until `count` are left (tests/test_gpu_diff_trans.py)"""
    x, y, v = rec
    n1, n2 = int(x.max()) + 1, int(y.max()) + 1
    free = np.nonzero((v < 3.0) & ~((x == n1 - 1) & (y == n2 - 1)))[0]
    extra = len(v) - count
    assert 0 <= extra <= len(free)
    keep = np.ones(len(v), bool)
    keep[np.random.default_rng(seed).choice(free, extra, replace=False)] = False
    return x[keep], y[keep], v[keep]


def threshold_pairs(which, count):
    """a 300 x 300 pair of which sample `which` is trimmed to exactly `count` records, then a live 300 x 300 pair"""
    rec = list(dr.synth_pair(300, 300, density=0.12, nloops=8, seed=1, added=3))
    rec[which] = _trimmed(rec[which], count, 11 + which)
    return [tuple(rec), dr.synth_pair(300, 300, density=0.3, nloops=10, seed=5, added=4)]


THRESHOLD_COUNTS = {(0, 10000): [4, 0, 5, 4], (1, 10000): [5, 3, 4, 0], "live": [8, 0, 7, 5]}


@pytest.fixture(scope="module")
def g1():
    pairs = g1_pairs()
    return pairs, _alone(pairs, 2000)


# ---- 1. one tile pair per pair, several tile sizes -----------------------------------------------------------------------------
def test_one_tile_pair_per_pair_and_several_tile_sizes(g1):
    from mustache_amd.trans import zscore_device
    pairs, alone = g1
    assert [_per_tag(r) for r in alone] == G1_COUNTS
    assert all(c[0] > 0 and c[2] > 0 for c in G1_COUNTS) and sum(1 for c in G1_COUNTS if c[1] + c[3] > 0) >= 2
    stats = {}
    genome = _genome(pairs, chunk=2000, stats=stats)                       # the default: 32 tile pairs per launch
    assert genome == alone
    assert stats == dict(tiles_total=6, tiles_skipped=0, launches=3, batches=1)
    for tpl, launches in ((1, 6), (2, 4)):                                # runs of equal C: 420 x 3, 340, 360 x 2
        stats = {}
        assert _genome(pairs, chunk=2000, tiles_per_launch=tpl, stats=stats) == alone, tpl
        assert stats["launches"] == launches, (tpl, stats)
    # one pair against the NumPy restatement on the device-normalised values
    norm = [(x, y, zscore_device(v)[0].cpu().numpy()) for x, y, v in pairs[3]]
    _compare(genome[3], dr.diff_trans_rows_normalized(norm[0], norm[1], ST, PT, PT2, OCT, chunk=2000))


def test_the_partition_into_batches_changes_nothing(g1):
    import torch
    from mustache_amd.trans_genome import RECORD_BYTES
    pairs, alone = g1
    n = [len(a[2]) + len(b[2]) for a, b in pairs]                         # a held pair costs both samples' records
    # 1 byte: every pair is over the budget by itself.  The first two pairs' bytes: pairs 0 + 1, 2 + 3, 4 + 5 fit, a third never
    two = RECORD_BYTES * (n[0] + n[1])
    assert n[2] + n[3] <= n[0] + n[1] and n[4] + n[5] <= n[0] + n[1] and min(n) * 3 > n[0] + n[1]
    for budget, batches in ((1, 6), (two, 3), (two - 1, 4)):       # one byte less: [0] [1] [2 3] [4 5]
        stats = {}
        assert _genome(pairs, chunk=2000, budget_bytes=budget, stats=stats) == alone, budget
        assert stats["batches"] == batches and stats["tiles_total"] == 6 and stats["tiles_skipped"] == 0, (budget, stats)
    # device tensors in, the same rows out
    dev_pairs = [tuple(tuple(torch.as_tensor(a).cuda() for a in rec) for rec in p) for p in pairs[:2]]
    assert _genome(dev_pairs, chunk=2000) == alone[:2]


# ---- 2. joint extents --------------------------------------------------------------------------------------------------------
def test_the_tiling_spans_both_samples_extents():
    rec1, rec2 = joint_extent_pair()
    assert rec2[0].max() == 419 > rec1[0].max() == 399 and rec1[1].max() == 299 > rec2[1].max() == 269
    alone = _alone([(rec1, rec2)], 2000)
    assert _per_tag(alone[0]) == JOINT_COUNTS
    stats = {}
    # beside a pair of another shape, and on several tile pairs of its own (tiles of 300: 4 x 1 over 420 x 300)
    other = g1_pairs()[3]
    assert _genome([other, (rec1, rec2)], chunk=2000, stats=stats)[1] == alone[0]
    assert stats["tiles_total"] == 2 and stats["tiles_skipped"] == 0
    assert _genome([(rec1, rec2), other], chunk=300, stats=stats)[0] == _alone([(rec1, rec2)], 300)[0]
    assert stats["tiles_total"] == 4 + 2                                  # 4 x 1 windows of 300 over 420 x 300, 1 x 2 over 300 x 340


# ---- 3. several tile pairs per pair, a wholly skipped pair ----------------------------------------------------------------------
def test_several_tile_pairs_per_pair_and_a_wholly_skipped_pair():
    pairs = g2_pairs()
    alone = _alone(pairs, 600)
    assert [_per_tag(r) for r in alone] == G2_COUNTS
    stats = {}
    genome = _genome(pairs, chunk=600, stats=stats)
    assert genome == alone and genome[1] == []
    # the middle pair's four windows hold fewer than 10 000 records of sample 2 (13 384 in all; 0.02 x 360 000 = 7 200 a
    # window), every other window more than 100 000 of either sample
    assert stats == dict(tiles_total=16, tiles_skipped=4, launches=1, batches=1)
    assert _genome(pairs, chunk=600, tiles_per_launch=5) == alone


# ---- 4. the threshold on either side -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [9999, 10000])
@pytest.mark.parametrize("which", [0, 1])
def test_a_skipped_tile_pair_beside_a_live_one(which, count):
    pairs = threshold_pairs(which, count)
    assert len(pairs[0][which][2]) == count and len(pairs[0][1 - which][2]) > 10000
    assert int((tr.zscore_exact(pairs[0][which][2])[0] != 0).sum()) == count          # every record is tested
    alone = _alone(pairs, 2000)
    assert _per_tag(alone[0]) == ([0, 0, 0, 0] if count == 9999 else THRESHOLD_COUNTS[(which, count)])
    assert _per_tag(alone[1]) == THRESHOLD_COUNTS["live"]
    stats = {}
    assert _genome(pairs, chunk=2000, stats=stats) == alone
    assert stats["tiles_total"] == 2 and stats["tiles_skipped"] == (1 if count == 9999 else 0), stats


# ---- 5. degenerate pairs -------------------------------------------------------------------------------------------------------
def test_degenerate_pairs_between_live_ones(g1, capsys):
    from mustache_amd.diff_trans_genome import call_diff_trans_genome
    pairs, alone = g1
    rng = np.random.default_rng(8)
    equal = (np.arange(10), np.arange(10), np.full(10, 4.0))                           # std = 0
    few = (rng.integers(0, 60, 49), rng.integers(0, 60, 49), np.exp(rng.normal(0.0, 0.5, 49)))
    full = pairs[1]
    batch = [pairs[0], (None, full[1]), (full[0], NONE), (equal, full[1]), (full[0], few), (few, full[1]), (full[0], None),
             pairs[3]]
    labels = ["a,b", "a,c", "a,d", "b,c", "b,d", "b,e", "c,d", "c,e"]
    capsys.readouterr()
    stats = {}
    got = call_diff_trans_genome(batch, OCT, ST, PT, PT2, chunk=2000, stats=stats, labels=labels)
    said = capsys.readouterr().out
    assert [_rows(r) for r in got] == [alone[0], [], [], [], [], [], [], alone[3]]
    for lb in ("a,c", "a,d", "b,c", "c,d"):
        assert said.count("There is no contact in the chromosome pair %s of one of the samples to work on.\n" % lb) == 1
    for lb in ("a,b", "b,d", "b,e", "c,e"):
        assert "pair %s of one" % lb not in said
    assert stats["tiles_total"] == 4 and stats["tiles_skipped"] == 2                   # the 49-record samples' tile pairs
    assert _alone(batch[1:7], 2000) == [[]] * 6
    assert call_diff_trans_genome([(None, NONE), (NONE, full[1])], OCT, ST, PT, PT2) == [[], []]
    assert call_diff_trans_genome([], OCT, ST, PT, PT2) == []


# ---- 6. the command line -------------------------------------------------------------------------------------------------------
SUFFIXES = (".loop1", ".diffloop1", ".loop2", ".diffloop2")


@pytest.fixture(scope="module")
def sample_files(tmp_path_factory):
    """two `.hic` samples: chromosomes 1-3 of 400 / 300 / 350 bins at 10 kb, and a chromosome 4 of 90 bins whose matrices hold
    records in sample 1 and none in sample 2"""
    res = 10000
    tmp = tmp_path_factory.mktemp("diff_trans_all")
    chroms = [("All", 1000), ("1", 400 * res), ("2", 300 * res), ("3", 350 * res), ("4", 90 * res)]
    n = {1: 400, 2: 300, 3: 350}
    both = {(a, b): dr.synth_pair(n[a], n[b], density=0.3, nloops=14, seed=s, added=5)
            for (a, b), s in (((1, 2), 21), ((1, 3), 23), ((2, 3), 22))}
    paths = []
    for s in (0, 1):
        mats = {ab: {res: rec[s]} for ab, rec in both.items()}
        for a in (1, 2, 3):
            mats[(a, 4)] = {res: tr.synth_trans(n[a], 90, density=0.3, nloops=2, seed=40 + a) if s == 0 else ([], [], [])}
        paths.append(str(tmp / ("s%d.hic" % (s + 1))))
        write_hic_pairs(paths[-1], chroms, mats, version=8)
    return paths


def test_trans_all_writes_the_rows_of_the_pair_runs(sample_files, tmp_path, capsys):
    from mustache_amd.diff_mustache import main
    f1, f2 = sample_files
    common = ["-f1", f1, "-f2", f2, "-r", "10kb", "-norm", "NONE"]
    names = ["1", "2", "3", "4"]
    six = list(itertools.combinations(names, 2))
    header, data = {}, {}
    for a, b in six:                                                       # one `-ch A -ch2 B` run per pair
        out = str(tmp_path / ("p_%s_%s" % (a, b)))
        main(common + ["-ch", a, "-ch2", b, "-o", out])
        for suf in SUFFIXES:
            lines = open(out + suf).read().splitlines(keepends=True)
            assert lines[0].startswith("BIN1_CHR")
            header[suf], data[(a, b, suf)] = lines[0], "".join(lines[1:])
    expected = {suf: header[suf] + "".join(data[(a, b, suf)] for a, b in six) for suf in SUFFIXES}
    assert all(len(data[(a, b, suf)]) > 0 for a, b in six[:1] + six[3:4] + six[1:2] for suf in (".loop1", ".loop2"))
    assert sum(len(expected[suf].splitlines()) - 1 for suf in (".diffloop1", ".diffloop2")) > 0
    out_all = str(tmp_path / "all")
    capsys.readouterr()
    main(common + ["--trans-all", "-o", out_all])
    said = capsys.readouterr().out
    for suf in SUFFIXES:
        assert open(out_all + suf).read() == expected[suf], suf
    for a, b in six:
        n = {suf: len(data[(a, b, suf)].splitlines()) for suf in SUFFIXES}
        assert "(%d,%d) loops and (%d,%d) differential-loops found in chrmosome=%s,%s for detection-fdr<0.2 and " \
               "difference-fdr<0.1" % (n[".loop1"], n[".loop2"], n[".diffloop1"], n[".diffloop2"], a, b) in said
    for a in names[:3]:
        assert "There is no contact in the chromosome pair %s,4 of one of the samples to work on." % a in said
    # -ch 1 2 3: the rows of its three pairs (chromosome 4's pairs have none, so the same files)
    out3 = str(tmp_path / "three")
    main(common + ["--trans-all", "-ch", "1", "2", "3", "-o", out3])
    three = list(itertools.combinations(names[:3], 2))
    for suf in SUFFIXES:
        assert open(out3 + suf).read() == header[suf] + "".join(data[(a, b, suf)] for a, b in three) == expected[suf], suf
