"""The restatement of the genome's coarsening rule (tests/coarsen_genome_reference.py) against what it promises: coarsening the
binned read pairs at r equals binning them at R = k r, the outside rule aliases nothing, and the merge keeps pairs apart.
No GPU, no package code."""
import numpy as np
import pytest

import coarsen_genome_reference as cg
import multires_reference as mr
import pairs_trans_reference as ptr

RES = 100
NAMES = ["chr1", "chr2", "chr3"]
LENGTHS = [4250, 2999, 701]                       # last bins of 50, 99 and 1 bp at r = 100; partial at every R below


def _genome(seed=3):
    rng = np.random.default_rng(seed)
    bins = cg.layout(LENGTHS, RES)
    cis, trans = {}, {}
    for c, n in enumerate(bins):
        i, j = np.triu_indices(n)
        cnt = rng.poisson(6.0 / (1 + (j - i)))
        k = cnt > 0
        cis[c] = (i[k], j[k], cnt[k])
    for a in range(3):
        for b in range(a + 1, 3):
            x, y = (t.ravel() for t in np.meshgrid(np.arange(bins[a]), np.arange(bins[b]), indexing="ij"))
            cnt = rng.poisson(0.7, len(x))
            cnt[-1] = 3                           # the corner pixel (last bin, last bin) is there
            k = cnt > 0
            trans[(a, b)] = (x[k], y[k], cnt[k])
    return cis, trans


@pytest.fixture(scope="module")
def parsed(tmp_path_factory):
    cis, trans = _genome()
    text, _ = ptr.pairs_text(NAMES, LENGTHS, RES, cis, trans, seed=11)
    path = tmp_path_factory.mktemp("cg") / "g.pairs"
    path.write_text(text)
    return ptr.parse_trans(str(path)), cis, trans


@pytest.mark.parametrize("k", [2, 3, 7])
def test_coarsening_the_binned_pairs_equals_binning_at_R(parsed, k):
    rows, cis, trans = parsed
    fine, _ = ptr.genome_pixels(rows, RES)
    coarse, _ = ptr.genome_pixels(rows, RES * k)
    assert {p: ptr.records_to_pixels(*rec) for p, rec in trans.items()} == fine            # the text holds the genome
    n = cg.layout(LENGTHS, RES * k)
    assert n == [length // (RES * k) + 1 for length in LENGTHS]
    got = {}
    for (a, b), px in fine.items():
        x, y, v = cg.pixels_to_records(px)
        out, outside = cg.coarsen_pair(x, y, v, k, n[a], n[b])
        assert outside == 0                       # positions inside the lengths: nothing is dropped
        assert max(c[0] for c in out) == n[a] - 1 and max(c[1] for c in out) == n[b] - 1   # the last, partial bin is used
        got[(a, b)] = out
    assert got == coarse
    # the same through coarsen_genome, and the cis parts against a direct binning of the cis pixels
    out_cis, out_trans = cg.coarsen_genome(LENGTHS, RES, cis, trans, k)
    assert {p: ptr.records_to_pixels(*rec) for p, rec in out_trans.items()} == coarse
    for c, (x, y, v) in cis.items():
        direct = {}
        for xi, yi, vi in zip(x.tolist(), y.tolist(), v.tolist()):
            if yi - xi >= 2:
                cell = (xi // k, yi // k)
                direct[cell] = direct.get(cell, 0) + vi
        direct = {cell: s for cell, s in direct.items() if cell[1] - cell[0] >= 2}
        assert (ptr.records_to_pixels(*out_cis[c]) if c in out_cis else {}) == direct       # chr3 at k = 7: two bins, no pixel
        # D >= 2 implies dist >= k + 1 >= 2: the fine pixels read_genome dropped could not have entered
        every = {}
        for xi, yi, vi in zip(x.tolist(), y.tolist(), v.tolist()):
            cell = (xi // k, yi // k)
            every[cell] = every.get(cell, 0) + vi
        assert {cell: s for cell, s in every.items() if cell[1] - cell[0] >= 2} == direct


def test_outside_records_alias_nothing():
    k, n_a, n_b = 2, 5, 3
    # Y == n_b would read as (X + 1, 0); X == n_a as the first row of the next pair; both stay out
    x = np.array([0, 0, 2, 10, 11, -1, 3, 9])
    y = np.array([1, 6, 7, 0, 5, 2, -4, 5])
    c = np.array([5, 7, 11, 13, 17, 19, 23, 29])
    out, outside = cg.coarsen_pair(x, y, c, k, n_a, n_b)
    assert out == {(0, 0): 5, (4, 2): 29} and outside == 6
    assert (1, 0) not in out and (2, 0) not in out
    # two pairs with the same rectangle: the record with X == n_a of pair 0 does not become (0, 0) of pair 1
    xs, ys, cs = np.array([10, 1]), np.array([0, 1]), np.array([13, 2])
    got, outside = cg.coarsen_pairs(xs, ys, cs, [0, 1, 2], [n_a, n_a], [n_b, n_b], k)
    assert got == {1: {(0, 0): 2}} and outside == 1
    # duplicates add twice, zero sums are no pixel, Python integers do not wrap
    big = 2 ** 32 - 1
    out, outside = cg.coarsen_pair([0, 1, 0, 4, 5], [0, 1, 0, 4, 4], [big, big, big, 0, 0], 2, 5, 3)
    assert out == {(0, 0): 3 * big} and outside == 0


def test_the_merge_keeps_pairs_apart():
    row = "%s\t%d\t%d\t%s\t%d\t%d\t0.01\t1.6\n"
    line = lambda a, b, x, y, r: row % (a, x * r, (x + 1) * r, b, y * r, (y + 1) * r)
    r, R = 100, 200
    fine = mr.HEADER + line("1", "2", 10, 20, r) + line("1", "3", 40, 8, r)
    coarse = mr.HEADER + line("1", "2", 5, 10, R) + line("1", "2", 20, 4, R) + line("1", "3", 5, 10, R) + line("1", "3", 20, 4, R) + \
        line("2", "3", 5, 10, R)
    text, counts = cg.merge_tsv([fine, coarse], [r, R], M=2)
    # (5, 10) at 200 bp lies on the 100 bp loop (10, 20) of pair 1,2 only; (20, 4) on (40, 8) of pair 1,3 only
    assert text == mr.HEADER + line("1", "2", 10, 20, r) + line("1", "2", 20, 4, R) + line("1", "3", 40, 8, r) + \
        line("1", "3", 5, 10, R) + line("2", "3", 5, 10, R)
    assert counts == [("1,2", R, 1, 2), ("1,3", R, 1, 2), ("2,3", R, 1, 1)]
    # the run's pair order decides the order of the rows; a pair without a row changes nothing
    text2, counts2 = cg.merge_tsv([fine, coarse], [r, R], M=2, pair_order=[("1", "2"), ("1", "3"), ("1", "4"), ("2", "3")])
    assert text2 == text and counts2 == counts[:2] + [("1,4", R, 0, 0)] + counts[2:]
    # M = 0 with centres that never coincide (r and 2 r): the concatenation, pair by pair
    text0, _ = cg.merge_tsv([fine, coarse], [r, R], M=0)
    assert sorted(text0.splitlines()) == sorted((fine + coarse[len(mr.HEADER):]).splitlines())
