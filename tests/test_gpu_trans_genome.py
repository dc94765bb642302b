"""Trans loops of many chromosome pairs in shared launches (mustache_amd/trans_genome.py) on the MI355X: every pair's rows equal
the rows of that pair alone (tests/trans_pair_alone.py: the single-pair kernels, every tile, no skip rule) -- under every
launch grouping and batch partition, with tiles and whole pairs skipped below 10 000 tested records, at the production tile
size, beside degenerate pairs, and through `--trans-all`.

The loop counts stated below are those of the NumPy restatement (tests/trans_reference.py on zscore_exact's values, st 0.88,
pt 0.2, octaves [1.6, 3.2]) run once on the CPU."""
import itertools

import numpy as np
import pytest

import trans_reference as tr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

OCT = [1.6, 3.2]
ST, PT = 0.88, 0.2


def _rows(loops):
    return [[int(a), int(b), float(q), float(s)] for a, b, q, s in loops]


def _compare(got, ref):
    assert len(ref) > 0, "the case should produce loops"
    assert [(int(a), int(b)) for a, b, _, _ in got] == [(int(a), int(b)) for a, b, _, _ in ref]
    assert [float(s) for _, _, _, s in got] == [float(s) for _, _, _, s in ref]
    for g, r in zip(got, ref):
        assert abs(float(g[2]) - float(r[2])) <= 1e-9, (g, r)


def _genome_pairs(bins, densities):
    return [tr.synth_trans(bins[a], bins[b], density=densities[k], nloops=10, seed=10 + k)
            for k, (a, b) in enumerate(itertools.combinations(range(len(bins)), 2))]


def _alone(pairs, chunk):
    from trans_pair_alone import pair_alone
    return [_rows(pair_alone(x, y, v, OCT, ST, PT, chunk=chunk)) for x, y, v in pairs]


@pytest.fixture(scope="module")
def g1():
    """bins 420, 300, 340, 360: six pairs of one tile each, C = 420, 420, 420, 340, 360, 360"""
    pairs = _genome_pairs([420, 300, 340, 360], [0.3] * 6)
    return pairs, _alone(pairs, 2000)


# ---- 4. G1 ---------------------------------------------------------------------------------------------------------------
def test_one_tile_per_pair_and_several_tile_sizes(g1):
    from mustache_amd.trans import zscore_device
    from mustache_amd.trans_genome import call_trans_genome
    pairs, alone = g1
    assert [len(r) for r in alone] == [7, 5, 8, 7, 5, 9]                  # the restatement's counts
    stats = {}
    genome = call_trans_genome(pairs, OCT, ST, PT, chunk=2000, stats=stats)
    for k in range(6):
        assert _rows(genome[k]) == alone[k] and len(alone[k]) > 0, k
    assert stats["tiles_total"] == 6 and stats["tiles_skipped"] == 0 and stats["batches"] == 1
    for tpl, launches in ((1, 6), (2, 4), (64, 3)):                       # runs of equal C: 420 x 3, 340, 360 x 2
        stats = {}
        again = call_trans_genome(pairs, OCT, ST, PT, chunk=2000, tiles_per_launch=tpl, stats=stats)
        assert [_rows(r) for r in again] == alone, tpl
        assert stats["launches"] == launches, (tpl, stats)
    # one pair against the NumPy restatement on the device-normalised values
    x, y, v = pairs[3]
    vz = zscore_device(v)[0].cpu().numpy()
    _compare(genome[3], tr.trans_loops_normalized(x, y, vz, ST, PT, OCT, chunk=2000))


def test_the_partition_into_batches_changes_nothing(g1):
    from mustache_amd.trans_genome import RECORD_BYTES, call_trans_genome
    pairs, alone = g1
    n = [len(p[2]) for p in pairs]
    # 1 byte: every pair is over the budget by itself.  The first two pairs' bytes: pairs 0 + 1, 2 + 3, 4 + 5 fit, a third never
    two = RECORD_BYTES * (n[0] + n[1])
    assert n[2] + n[3] <= n[0] + n[1] and n[4] + n[5] <= n[0] + n[1] and min(n) * 3 > n[0] + n[1]
    for budget, batches in ((1, 6), (two, 3)):
        stats = {}
        got = call_trans_genome(pairs, OCT, ST, PT, chunk=2000, budget_bytes=budget, stats=stats)
        assert [_rows(r) for r in got] == alone, budget
        assert stats["batches"] == batches and stats["tiles_total"] == 6 and stats["tiles_skipped"] == 0, (budget, stats)
    # device tensors in, the same rows out
    import torch
    dev_pairs = [tuple(torch.as_tensor(a).cuda() for a in p) for p in pairs[:2]]
    assert [_rows(r) for r in call_trans_genome(dev_pairs, OCT, ST, PT, chunk=2000)] == alone[:2]


# ---- 5. G2 ---------------------------------------------------------------------------------------------------------------
def test_several_tiles_per_pair_and_a_wholly_skipped_pair():
    from mustache_amd.trans_genome import call_trans_genome
    pairs = _genome_pairs([900, 1200, 700], [0.3, 0.02, 0.3])
    alone = _alone(pairs, 600)
    assert [len(r) for r in alone] == [8, 0, 7]
    stats = {}
    genome = call_trans_genome(pairs, OCT, ST, PT, chunk=600, stats=stats)
    assert [_rows(r) for r in genome] == alone
    # the middle pair's four tiles hold 7 760 .. 7 874 tested records, every other tile more than 107 000
    assert stats["tiles_total"] == 16 and stats["tiles_skipped"] == 4 and genome[1] == []
    assert stats["launches"] == 1 and stats["batches"] == 1              # twelve tiles of 600 from pairs 0 and 2, pair 1 between
    assert [_rows(r) for r in call_trans_genome(pairs, OCT, ST, PT, chunk=600, tiles_per_launch=5)] == alone


# ---- 6. G3 ---------------------------------------------------------------------------------------------------------------
def _threshold_map(n1, n2, count, seed, window_cols=None):
    """synth_trans records trimmed (background records left of the last 300 columns only) until the window [0, n1) x
    [0, window_cols) holds exactly `count` records (tests/test_gpu_trans.py)"""
    x, y, v = tr.synth_trans(n1, n2, density=0.12, nloops=8, seed=seed)
    wc = n2 if window_cols is None else window_cols
    inside = y < wc
    free = inside & (y < (n2 - 300 if n2 > 300 else n2)) & (v < 3.0) & ~((x == n1 - 1) & (y == n2 - 1))
    extra = int(inside.sum()) - count
    assert 0 <= extra <= int(free.sum())
    drop = np.random.default_rng(seed + 100).choice(np.nonzero(free)[0], extra, replace=False)
    keep = np.ones(len(v), bool)
    keep[drop] = False
    return x[keep], y[keep], v[keep]


def _tiles_below_threshold(x, y, v, chunk):
    """per tile of the pair (row-major) whether fewer than 10 000 of its records have v' != 0, from NumPy masks"""
    vz = tr.zscore_exact(v)[0]
    C, (rs, _), (cs, _) = tr.tiling(int(x.max()) + 1, int(y.max()) + 1, chunk)
    return [int(((x >= r) & (x < r + C) & (y >= q) & (y < q + C) & (vz != 0)).sum()) < 10000 for r in rs for q in cs]


@pytest.mark.parametrize("count", [9999, 10000])
def test_a_skipped_tile_beside_a_live_one(count):
    from mustache_amd.trans_genome import call_trans_genome
    first = _threshold_map(300, 500, count, 3, window_cols=300)
    second = tr.synth_trans(300, 310, 0.3, seed=5)
    pairs = [first, second]
    alone = _alone(pairs, 300)
    assert len(alone[0]) > 0 and len(alone[1]) > 0
    # the window of the first column tile is [0, 300): exactly `count` records, all tested
    below = _tiles_below_threshold(*first, 300) + _tiles_below_threshold(*second, 300)
    assert below[0] == (count == 9999)
    assert any(b < 300 for _, b, _, _ in alone[0]) == (count == 10000)    # tests/test_gpu_trans.py: the left tile's own loops
    stats = {}
    genome = call_trans_genome(pairs, OCT, ST, PT, chunk=300, stats=stats)
    assert [_rows(r) for r in genome] == alone
    assert stats["tiles_total"] == len(below) and stats["tiles_skipped"] == sum(below), (stats, below)


# ---- 7. the production tile size --------------------------------------------------------------------------------------------
def test_production_tiles_of_two_pairs_in_one_call():
    from mustache_amd.trans_genome import call_trans_genome
    pairs = [tr.production_records("sparse_2x2"), tr.production_records("short_long_2x2")]
    alone = _alone(pairs, 2000)
    stats = {}
    genome = call_trans_genome(pairs, OCT, ST, PT, stats=stats)           # the default chunk
    assert [_rows(r) for r in genome] == alone and all(len(r) > 0 for r in alone)
    # every sparse_2x2 tile holds 10 244 .. 10 908 records, just above the threshold: nothing is skipped
    assert stats == dict(tiles_total=8, tiles_skipped=0, launches=1, batches=1)


# ---- 8. degenerate pairs --------------------------------------------------------------------------------------------------
def test_degenerate_pairs_between_live_ones(g1, capsys):
    from mustache_amd.trans_genome import call_trans_genome
    pairs, alone = g1
    rng = np.random.default_rng(8)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    equal = (np.arange(10), np.arange(10), np.full(10, 4.0))                           # std = 0
    few = (rng.integers(0, 60, 49), rng.integers(0, 60, 49), np.exp(rng.normal(0.0, 0.5, 49)))
    batch = [pairs[0], None, empty, equal, few, pairs[3]]
    labels = ["a,b", "a,c", "a,d", "b,c", "b,d", "c,d"]
    capsys.readouterr()
    stats = {}
    got = call_trans_genome(batch, OCT, ST, PT, chunk=2000, stats=stats, labels=labels)
    said = capsys.readouterr().out
    assert [_rows(r) for r in got] == [alone[0], [], [], [], [], alone[3]]
    for lb in ("a,c", "a,d", "b,c"):
        assert "There is no contact in the chromosome pair %s to work on." % lb in said
    for lb in ("a,b", "b,d", "c,d"):
        assert "pair %s to work on" % lb not in said
    assert stats["tiles_total"] == 3 and stats["tiles_skipped"] == 1                   # the 49-record pair's one tile
    assert call_trans_genome([None, empty], OCT, ST, PT) == [[], []]
    assert call_trans_genome([], OCT, ST, PT) == []


# ---- 9. the command line ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome_file(tmp_path_factory):
    res = 10000
    path = tmp_path_factory.mktemp("trans_all") / "g.hic"
    chroms = [("All", 1000), ("1", 400 * res), ("2", 300 * res), ("3", 350 * res), ("4", 90 * res)]
    n = {1: 400, 2: 300, 3: 350}
    mats = {(a, b): {res: tr.synth_trans(n[a], n[b], density=0.3, nloops=10, seed=s)}
            for (a, b), s in (((1, 2), 21), ((1, 3), 22), ((2, 3), 23))}
    for a in (1, 2, 3):
        mats[(a, 4)] = {res: ([], [], [])}
    write_hic_pairs(str(path), chroms, mats, version=8)
    return path


def _pair_runs(main, f, tmp_path, pairs):
    """header + the data rows of one `-ch A -ch2 B` run per pair, in pair order"""
    text = None
    for a, b in pairs:
        out = tmp_path / ("p_%s_%s.tsv" % (a, b))
        main(["-f", str(f), "-ch", a, "-ch2", b, "-r", "10kb", "-norm", "NONE", "-o", str(out)])
        lines = out.read_text().splitlines()
        assert lines[0].startswith("BIN1_CHR")
        text = (lines[0] + "\n" if text is None else text) + "".join(ln + "\n" for ln in lines[1:])
    return text


def test_trans_all_writes_the_rows_of_the_pair_runs(genome_file, tmp_path, capsys):
    from mustache_amd.mustache import main
    names = ["1", "2", "3", "4"]
    six = list(itertools.combinations(names, 2))
    expected = _pair_runs(main, genome_file, tmp_path, six)
    assert len(expected.splitlines()) > 10
    out_all = tmp_path / "all.tsv"
    capsys.readouterr()
    main(["-f", str(genome_file), "-r", "10kb", "--trans-all", "-norm", "NONE", "-o", str(out_all)])
    said = capsys.readouterr().out
    assert out_all.read_text() == expected
    for a, b in six:
        assert "loops found for chrmosome pair=%s,%s, fdr<0.2" % (a, b) in said
    # -ch 1 2 3: the rows of its three pairs
    three = list(itertools.combinations(names[:3], 2))
    out3 = tmp_path / "three.tsv"
    main(["-f", str(genome_file), "-r", "10kb", "-ch", "1", "2", "3", "--trans-all", "-norm", "NONE", "-o", str(out3)])
    assert out3.read_text() == _pair_runs(main, genome_file, tmp_path, three) == expected


def test_trans_all_refusals_write_nothing(genome_file, tmp_path, capsys):
    from mustache_amd.mustache import main
    out = tmp_path / "none.tsv"
    capsys.readouterr()
    main(["-f", str(genome_file), "-r", "10kb", "--trans-all", "-ch", "1", "-ch2", "2", "-norm", "NONE", "-o", str(out)])
    assert "Error: --trans-all pairs the -ch list with itself; give -ch2 without it" in capsys.readouterr().out
    assert not out.exists()
    text = tmp_path / "contacts.txt"
    text.write_text("10000\t20000\t3\n20000\t40000\t1\n")
    main(["-f", str(text), "-r", "10kb", "--trans-all", "-o", str(out)])
    assert "Error: Interchromosomal analysis is only supported for .hic and .cool input formats." in capsys.readouterr().out
    assert not out.exists()
    main(["-f", str(genome_file), "-r", "10kb", "--trans-all", "--balance", "ICE", "-o", str(out)])
    assert "Error: --balance does not apply to inter-chromosomal pairs" in capsys.readouterr().out
    assert not out.exists()
