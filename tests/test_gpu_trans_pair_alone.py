"""A pair alone is a batch of one pair: trans.call_trans_coo and diff_trans.call_diff_trans_coo (trans_genome.PairBatcher.run_pair:
the segmented z-score, the tile counts and the skip rule, the work-list scatter) against the independent single-pair form of
tests/trans_pair_alone.py (mst_trans_zscore, every tile, mst_trans_scatter_tiles), row for row and bit for bit -- on one tile,
on many tiles with a shifted last window, with a tile the skip rule drops, over two samples of different extents, from host
arrays and device tensors (which are left as they were), on the degenerate inputs, and through both command lines."""
import numpy as np
import pytest

import diff_trans_reference as dr
import trans_reference as tr
from trans_pair_alone import diff_pair_alone, pair_alone

pytestmark = pytest.mark.gpu

OCT = [1.6, 3.2]
ST, PT, PT2 = 0.88, 0.2, 0.1
NONE = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
ONE_LINE = "There is no contact in the chromosome pair %s to work on.\n"
TWO_LINE = "There is no contact in the chromosome pair %s of one of the samples to work on.\n"


def _rows(rows):
    """plain Python values, every field: == on two of these is bit equality of x, y, fdr, sigma (and tag)"""
    return [[int(r[0]), int(r[1]), float(r[2]), float(r[3])] + [int(t) for t in r[4:]] for r in rows]


def _one(rec, **kw):
    from mustache_amd.trans import call_trans_coo
    return _rows(call_trans_coo(rec[0], rec[1], rec[2], OCT, ST, PT, **kw))


def _two(rec1, rec2, **kw):
    from mustache_amd.diff_trans import call_diff_trans_coo
    return _rows(call_diff_trans_coo(rec1, rec2, OCT, ST, PT, PT2, **kw))


def _records_per_tile(rec, n1, n2, chunk):
    """per tile of the n1 x n2 tiling (row-major) its records with v' != 0, from NumPy masks"""
    x, y, v = rec
    vz = tr.zscore_exact(v)[0]
    C, (rs, _), (cs, _) = tr.tiling(n1, n2, chunk)
    return [int(((x >= r) & (x < r + C) & (y >= q) & (y < q + C) & (vz != 0)).sum()) for r in rs for q in cs]


def _thinned(rec, rows_below, keep_share, seed):
    """rec with only `keep_share` of its background records (v < 3) of the rows [0, rows_below) kept"""
    x, y, v = rec
    drop = (x < rows_below) & (v < 3.0) & (np.random.default_rng(seed).random(len(v)) >= keep_share)
    return x[~drop], y[~drop], v[~drop]


# ---- the maps (NumPy only) and the oracle's rows, computed once --------------------------------------------------------------
@pytest.fixture(scope="module")
def one_tile():
    """180 x 140 at the default chunk: one tile of C = 180 with about 15 000 records, above the 10 000 threshold"""
    rec = tr.synth_trans(180, 140, density=0.6, nloops=6, seed=41)
    assert 14000 < len(rec[2]) < 16500
    return rec, _rows(pair_alone(*rec, OCT, ST, PT))


@pytest.fixture(scope="module")
def many_tiles():
    """700 x 330 at chunk 300: 11 x 2 windows, the last of each axis at n - C (400 after 396, 30 after 0)"""
    rec = tr.synth_trans(700, 330, density=0.3, nloops=24, seed=42)
    C, (rs, _), (cs, _) = tr.tiling(700, 330, 300)
    assert (C, len(rs), len(cs), rs[-2:], cs) == (300, 11, 2, [396, 400], [0, 30])
    assert min(_records_per_tile(rec, 700, 330, 300)) >= 10000                 # nothing to skip
    return rec, _rows(pair_alone(*rec, OCT, ST, PT, chunk=300))


@pytest.fixture(scope="module")
def two_extents():
    """two samples over 700 x 330 at chunk 300: sample 1 without its last 30 columns, sample 2 without its last 44 rows -- one
    whole row window.  Alone sample 1 tiles 11 x 1 and sample 2 10 x 2; the pair tiles 11 x 2 over the maxima"""
    (x1, y1, v1), (x2, y2, v2) = dr.synth_pair(700, 330, density=0.3, nloops=30, seed=43, added=10)
    k1, k2 = y1 < 300, x2 < 656
    rec1, rec2 = (x1[k1], y1[k1], v1[k1]), (x2[k2], y2[k2], v2[k2])
    assert (rec1[0].max(), rec1[1].max(), rec2[0].max(), rec2[1].max()) == (699, 299, 655, 329)
    shapes = [tuple(len(a[0]) for a in tr.tiling(n1, n2, 300)[1:]) for n1, n2 in ((700, 300), (656, 330), (700, 330))]
    assert shapes == [(11, 1), (10, 2), (11, 2)]
    return rec1, rec2, _rows(diff_pair_alone(rec1, rec2, OCT, ST, PT, PT2, chunk=300))


# ---- one sample --------------------------------------------------------------------------------------------------------------
def test_one_tile_above_the_threshold(one_tile):
    rec, alone = one_tile
    assert len(alone) > 0
    assert _one(rec) == alone


@pytest.mark.parametrize("tpl", [1, 4, None])
def test_many_tiles_with_a_shifted_last_window(many_tiles, tpl):
    rec, alone = many_tiles
    assert len(alone) > 0 and any(r[1] >= 300 for r in alone)                 # columns only the shifted last window owns
    assert _one(rec, chunk=300, tiles_per_launch=tpl) == alone
    if tpl is not None:
        assert _rows(pair_alone(*rec, OCT, ST, PT, chunk=300, tiles_per_launch=tpl)) == alone


def test_a_skipped_tile_beside_a_live_one(many_tiles):
    """rows [0, 300) thinned to a third of their background: tile (0, 0), columns [0, 300), holds 9 893 records and is dropped
    before the scatter (the oracle runs it to no rows); tile (0, 1), columns [30, 330), holds 10 145, stays and reports the
    rows it owns in the columns [300, 330)"""
    from mustache_amd.trans_genome import TransGenomeCaller
    rec = _thinned(many_tiles[0], 300, 1.0 / 3.0, 7)
    counts = _records_per_tile(rec, 700, 330, 300)
    below = [c < 10000 for c in counts]
    assert below[:2] == [True, False] and sum(below) == 1, counts
    alone = _rows(pair_alone(*rec, OCT, ST, PT, chunk=300))
    assert any(r[0] < 300 for r in alone) and all(r[1] >= 300 for r in alone if r[0] < 300)
    assert _one(rec, chunk=300) == alone
    stats = {}
    again = TransGenomeCaller(OCT, ST, PT, None, chunk=300, tiles_per_launch=4, stats=stats).run_pair([rec], "")
    assert _rows(again) == alone
    assert stats == dict(tiles_total=22, tiles_skipped=1, launches=6, batches=1)


def _on_device(rec, index_dtype):
    import torch
    return (torch.as_tensor(rec[0]).to("cuda", dtype=index_dtype), torch.as_tensor(rec[1]).to("cuda", dtype=index_dtype),
            torch.as_tensor(rec[2]).to("cuda"))


def _same_bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_device_tensors_give_the_same_rows_and_are_left_as_they_were(one_tile, many_tiles):
    import torch
    for (rec, alone), kw in ((one_tile, {}), (many_tiles, dict(chunk=300))):
        for index_dtype in (torch.int32, torch.int64):                        # int32: the batch adopts x and y as they are
            dev = _on_device(rec, index_dtype)
            before = [a.clone() for a in dev]
            assert _one(dev, **kw) == alone
            assert _one(dev, **kw) == alone                                   # and again, on the same tensors
            assert all(_same_bits(a, b) for a, b in zip(dev, before))


def test_one_sample_degenerate_inputs_say_the_line_and_return_nothing(capsys):
    from mustache_amd.trans import call_trans_coo
    x, y, v = tr.synth_trans(80, 60, density=0.3, nloops=2, seed=1)
    bad = v.copy()
    bad[5] = np.inf
    capsys.readouterr()
    for rec in (NONE, (x, y, np.full(len(v), 3.0)), (x, y, bad)):
        for kw, label in ((dict(), ""), (dict(label="7,9"), "7,9"), (dict(label="7,9", verbose=True), "7,9")):
            assert call_trans_coo(rec[0], rec[1], rec[2], OCT, ST, PT, **kw) == []
            assert capsys.readouterr().out == ONE_LINE % label
        assert pair_alone(*rec, OCT, ST, PT) == []


# ---- two samples -------------------------------------------------------------------------------------------------------------
def test_two_samples_on_one_tile_pair():
    rec1, rec2 = dr.synth_pair(180, 140, density=0.6, nloops=8, seed=44, added=3)
    alone = _rows(diff_pair_alone(rec1, rec2, OCT, ST, PT, PT2))
    assert all(any(r[4] == t for r in alone) for t in (1, 3))
    assert _two(rec1, rec2) == alone


@pytest.mark.parametrize("tpl", [1, 4, None])
def test_two_samples_with_different_extents(two_extents, tpl):
    rec1, rec2, alone = two_extents
    assert all(any(r[4] == t for r in alone) for t in (1, 3)) and any(r[4] in (2, 4) for r in alone)
    assert _two(rec1, rec2, chunk=300, tiles_per_launch=tpl) == alone
    if tpl is not None:
        assert _rows(diff_pair_alone(rec1, rec2, OCT, ST, PT, PT2, chunk=300, tiles_per_launch=tpl)) == alone


@pytest.mark.parametrize("which", [0, 1])
def test_a_tile_pair_skipped_for_either_sample(two_extents, which):
    """rows [0, 300) of one sample thinned until its first row of tile pairs is below 10 000 records: both are dropped for that
    sample alone (the other holds more than 25 000 there), the second row of tile pairs (rows 44 .. 343) stays"""
    recs = list(two_extents[:2])
    recs[which] = _thinned(recs[which], 300, 0.28, 8 + which)
    counts = [_records_per_tile(r, 700, 330, 300) for r in recs]
    below = [min(a, b) < 10000 for a, b in zip(*counts)]
    assert below[:4] == [True, True, False, False] and sum(below) == 2 and min(counts[1 - which]) >= 10000, counts
    alone = _rows(diff_pair_alone(recs[0], recs[1], OCT, ST, PT, PT2, chunk=300))
    assert len(alone) > 0
    assert _two(recs[0], recs[1], chunk=300) == alone


def test_two_samples_device_tensors_give_the_same_rows_and_are_left_as_they_were(two_extents):
    import torch
    rec1, rec2, alone = two_extents
    for index_dtype in (torch.int32, torch.int64):
        dev1, dev2 = _on_device(rec1, index_dtype), _on_device(rec2, index_dtype)
        before = [a.clone() for a in dev1 + dev2]
        assert _two(dev1, dev2, chunk=300) == alone
        assert _two(dev1, rec2, chunk=300) == alone                           # one sample on the device, one on the host
        assert all(_same_bits(a, b) for a, b in zip(dev1 + dev2, before))


def test_two_sample_degenerate_inputs_say_the_line_and_return_nothing(capsys):
    from mustache_amd.diff_trans import call_diff_trans_coo
    x, y, v = tr.synth_trans(80, 60, density=0.3, nloops=2, seed=1)
    bad = v.copy()
    bad[5] = np.nan
    full = (x, y, v)
    capsys.readouterr()
    for rec in (NONE, (x, y, np.full(len(v), 3.0)), (x, y, bad)):
        for a, b in ((rec, full), (full, rec), (rec, rec)):
            for kw, label in ((dict(), ""), (dict(label="7,9", verbose=True), "7,9")):
                assert call_diff_trans_coo(a, b, OCT, ST, PT, PT2, **kw) == []
                assert capsys.readouterr().out == TWO_LINE % label
            assert diff_pair_alone(a, b, OCT, ST, PT, PT2) == []


# ---- the command lines ---------------------------------------------------------------------------------------------------------
def _tsv_rows(path):
    """(chr1, chr2, x, y, fdr, sigma) per data row of a loops file at 10 kb"""
    with open(path) as fh:
        lines = fh.read().splitlines()
    assert lines[0].startswith("BIN1_CHR")
    out = []
    for r in (ln.split("\t") for ln in lines[1:]):
        assert int(r[2]) == int(r[1]) + 10000 and int(r[5]) == int(r[4]) + 10000
        out.append((r[0], r[3], int(r[1]) // 10000, int(r[4]) // 10000, float(r[6]), float(r[7])))
    return out


def _file_records(f, a, b):
    from mustache_amd.trans import read_hic_trans
    return read_hic_trans(f, "NONE", a, b, 10000)


def test_the_one_sample_command_line_on_a_pair(tmp_path, capsys):
    from mustache_amd.mustache import main
    from test_gpu_trans import _trans_file
    f = tmp_path / "m.hic"
    _trans_file(f)
    out = tmp_path / "t.tsv"
    capsys.readouterr()
    main(["-f", str(f), "-ch", "2", "-ch2", "1", "-r", "10kb", "-norm", "NONE", "-o", str(out)])
    said = capsys.readouterr().out
    alone = _rows(pair_alone(*_file_records(str(f), "2", "1"), OCT, ST, PT))
    assert len(alone) > 0
    assert _tsv_rows(out) == [("2", "1", a, b, q, s) for a, b, q, s in alone]
    assert "Loop calling (trans 2,1: 400 x 300 bins, 1 tiles of 400)...\n" in said
    assert "trans batch" not in said


def test_the_two_sample_command_line_on_a_pair(tmp_path, capsys):
    from mustache_amd.diff_mustache import main
    from test_gpu_diff_trans import SUFFIXES, _sample_files
    f1, f2 = _sample_files(tmp_path)
    out = str(tmp_path / "d")
    capsys.readouterr()
    main(["-f1", f1, "-f2", f2, "-ch", "2", "-ch2", "1", "-r", "10kb", "-norm", "NONE", "-o", out])
    said = capsys.readouterr().out
    alone = _rows(diff_pair_alone(_file_records(f1, "2", "1"), _file_records(f2, "2", "1"), OCT, ST, PT, PT2))
    assert any(r[4] == 1 for r in alone) and any(r[4] == 3 for r in alone)
    for tag, suf in enumerate(SUFFIXES, start=1):
        assert _tsv_rows(out + suf) == [("2", "1", a, b, q, s) for a, b, q, s, t in alone if t == tag], suf
    assert "Loop calling (trans 2,1: 400 x 300 bins, 1 tile pairs of 400)...\n" in said
    assert "trans batch" not in said
