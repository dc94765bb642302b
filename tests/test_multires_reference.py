"""The rules of mustache_amd/multires.py on the host: the NumPy restatement of the coarsening (tests/multires_reference.py)
against the binning identity floor(floor((p - 1) / r) / k) == floor((p - 1) / (r k)), and multires.merge_loops (a sort and
searchsorted) against the restatement's literal double loop.  Every comparison is exact.  No GPU."""
import numpy as np
import pytest

import multires_reference as ref
import pairs_reference


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("zero_based", [False, True])
def test_coarsening_the_binned_pairs_is_binning_them_coarser(k, zero_based):
    rng = np.random.default_rng(100 + k)
    r, length = 700, 700 * 301 + 13
    p1 = rng.integers(-3, length + 5, 20000)
    near = rng.random(20000) < 0.7
    p2 = np.where(near, np.clip(p1 + rng.integers(-9000, 9000, 20000), -3, length + 4), rng.integers(-3, length + 5, 20000))
    x, y, c, _ = pairs_reference.pixels(p1, p2, r, zero_based, length)
    X, Y, C, _ = pairs_reference.pixels(p1, p2, r * k, zero_based, length)
    assert len(X) < len(x)
    assert ref.triples(*ref.coarsen(x, y - x, c, k)) == ref.triples(X, Y - X, C)


def test_the_restated_coarsening_on_a_case_worked_by_hand():
    #          (0,0) (1,1) -> (0,0);  (1,2) -> (0,1);  (2,5) -> (1,2);  (4,5) twice -> (2,2);  a zero count alone -> no pixel
    x = [0, 1, 1, 2, 4, 4, 8]
    d = [0, 0, 1, 3, 1, 1, 0]
    c = [3, 4, 5, 6, 1 << 31, (1 << 32) - 1, 0]
    assert ref.triples(*ref.coarsen(x, d, c, 2)) == [(0, 0, 7), (0, 1, 5), (1, 1, 6), (2, 0, (1 << 31) + (1 << 32) - 1)]
    assert ref.triples(*ref.coarsen(x, d, c, 100)) == [(0, 0, 18 + (1 << 31) + (1 << 32) - 1)]
    assert ref.triples(*ref.coarsen([], [], [], 2)) == []


def _random_lists(rng, resolutions, rows, span_bp):
    lists = []
    for r in resolutions:
        x = rng.integers(0, span_bp // r, rows)
        y = np.minimum(x + rng.integers(0, 40, rows), span_bp // r - 1)
        lists.append([[int(a), int(b), float(rng.random()), 1.6] for a, b in zip(x, y)])
    return lists


@pytest.mark.parametrize("M", [0, 1, 2])
@pytest.mark.parametrize("resolutions", [(5000, 10000), (5000, 25000), (5000, 10000, 50000), (1000, 2000, 10000)])
def test_merge_loops_is_the_double_loop(M, resolutions):
    from mustache_amd.multires import merge_loops
    rng = np.random.default_rng(7 * M + len(resolutions) + resolutions[1])
    lists = _random_lists(rng, resolutions, 300, 1500000)
    want = ref.merge(lists, resolutions, M)
    got = merge_loops(lists, resolutions, M)
    assert got == want
    assert got[0] == lists[0]
    dropped = [len(a) - len(b) for a, b in zip(lists, want)]
    print(dropped)
    assert all(0 < len(k) for k in want[1:]) and (M == 0 or all(d > 0 for d in dropped[1:]))


@pytest.mark.parametrize("M", [0, 1, 2])
@pytest.mark.parametrize("factor", [2, 5])
def test_centres_on_the_boundary_and_one_past_it(M, factor):
    """a fine loop at bins (x, y); coarse loops whose doubled centres are exactly 2 M R away, and 2 M R + the smallest step on"""
    from mustache_amd.multires import merge_loops
    r, R = 5000, 5000 * factor
    # doubled centres: fine 2 x r + r, coarse 2 X R + R.  With x = X0 * factor + t the difference is (2 t + 1 - factor) r
    # + 2 (X0 - X) R, so t = (factor - 1) / 2 (factor odd) puts the centres M bins apart exactly; for factor 2 no centres
    # coincide and the nearest miss is r = R / 2.
    X0, Y0 = 40, 60
    fine, coarse, expect = [], [], []
    for t in range(factor):
        fine.append([X0 * factor + t, Y0 * factor + t, 0.01, 1.6])
    for dx in range(-M - 2, M + 3):
        for dy in (-M - 1, -M, 0, M, M + 1):
            coarse.append([X0 + dx, Y0 + dy, 0.02, 3.2])
    want = ref.merge([fine, coarse], (r, R), M)
    got = merge_loops([fine, coarse], (r, R), M)
    assert got == want
    # spelled out: a coarse loop stays exactly when every fine loop is more than 2 M R away (doubled centres) in x or in y
    for lp in coarse:
        far = all(abs(2 * f[0] * r + r - 2 * lp[0] * R - R) > 2 * M * R or abs(2 * f[1] * r + r - 2 * lp[1] * R - R) > 2 * M * R
                  for f in fine)
        assert (lp in got[1]) == far
    gaps = {abs(2 * f[0] * r + r - 2 * lp[0] * R - R) - 2 * M * R for f in fine for lp in coarse}
    assert 0 in gaps or factor == 2                       # a centre exactly on the boundary ...
    assert min(g for g in gaps if g > 0) in (r, 2 * r)    # ... and the smallest step past it
    if factor == 2:
        assert r in {abs(g) for g in gaps}


def test_exactly_on_the_boundary_drops_and_one_more_keeps():
    from mustache_amd.multires import merge_loops
    r, R, M = 5000, 25000, 2
    fine = [[102, 302, 0.01, 1.6]]                         # centre 2 * 102 * r + r = 205 r = 41 R: coarse bin 20's centre
    on = [[22, 62, 0.02, 3.2], [18, 58, 0.02, 3.2], [22, 58, 0.02, 3.2]]          # both coordinates exactly M bins away
    past = [[23, 60, 0.02, 3.2], [20, 63, 0.02, 3.2], [17, 57, 0.02, 3.2]]        # one coordinate M + 1 bins away
    assert abs(2 * 102 * r + r - 2 * 22 * R - R) == 2 * M * R and abs(2 * 302 * r + r - 2 * 62 * R - R) == 2 * M * R
    got = merge_loops([fine, on + past], (r, R), M)
    assert got == ref.merge([fine, on + past], (r, R), M) == [fine, past]
    # r apart from the boundary at factor 2: 2 M R + r keeps, 2 M R - r drops
    r, R, M = 5000, 10000, 1
    fine = [[81, 121, 0.01, 1.6]]                          # doubled centre 163 r; coarse bin X has (4 X + 2) r
    coarse = [[39, 59, 0.5, 3.2], [41, 60, 0.5, 3.2], [41, 61, 0.5, 3.2]]      # x one step past the boundary; the other two one step inside it
    got = merge_loops([fine, coarse], (r, R), M)
    assert abs(163 * r - (4 * 39 + 2) * r) == 2 * M * R + r and abs(163 * r - (4 * 41 + 2) * r) == 2 * M * R - r
    assert abs(243 * r - (4 * 60 + 2) * r) < 2 * M * R and abs(243 * r - (4 * 61 + 2) * r) == 2 * M * R - r
    assert got[1] == [[39, 59, 0.5, 3.2]] == ref.merge([fine, coarse], (r, R), M)[1]


def test_a_middle_survivor_suppresses_and_a_dropped_middle_loop_does_not():
    from mustache_amd.multires import merge_loops
    res = (5000, 10000, 20000)
    fine = [[100, 140, 0.01, 1.6]]                         # 5 kb: centre 502.5 kb, 702.5 kb
    middle = [[50, 70, 0.02, 1.6],                         # 10 kb, on the fine loop: dropped
              [200, 230, 0.02, 1.6]]                       # 10 kb, alone: survives
    coarse = [[100, 115, 0.03, 3.2],                       # 20 kb, centre 2.01 Mb, 2.31 Mb: near the middle survivor only
              [400, 420, 0.03, 3.2],                       # 20 kb, near nothing
              [27, 37, 0.03, 3.2]]                         # 20 kb, centre 550 kb, 750 kb: 47.5 kb from the fine loop -> kept at M = 2
    got = merge_loops([fine, middle, coarse], res, 2)
    assert got == ref.merge([fine, middle, coarse], res, 2)
    assert got == [fine, [middle[1]], [coarse[1], coarse[2]]]
    # the same coarse loop beside a middle loop that was itself dropped: the dropped loop suppresses nothing
    fine2 = [[100, 140, 0.01, 1.6]]
    middle2 = [[51, 71, 0.02, 1.6]]                        # centre 515 kb, 715 kb: 12.5 kb from the fine loop -> dropped
    coarse2 = [[28, 38, 0.03, 3.2]]                        # centre 570 kb, 770 kb: 55 kb from the dropped middle loop, within
    #                                                        the reach of M = 3 (60 kb), and 67.5 kb from the fine loop
    got = merge_loops([fine2, middle2, coarse2], res, 3)
    assert got == ref.merge([fine2, middle2, coarse2], res, 3)
    # fine -> coarse: |1005 - 1140| * 5 kb / 2 = 67.5 kb > 60 kb: the fine loop does not reach it; the middle loop would (55 kb)
    assert abs(2 * 100 * 5000 + 5000 - 2 * 28 * 20000 - 20000) > 2 * 3 * 20000
    assert abs(2 * 51 * 10000 + 10000 - 2 * 28 * 20000 - 20000) <= 2 * 3 * 20000
    assert abs(2 * 71 * 10000 + 10000 - 2 * 38 * 20000 - 20000) <= 2 * 3 * 20000
    assert got == [fine2, [], coarse2]


def test_an_empty_fine_list_gives_the_coarse_lists():
    from mustache_amd.multires import merge_loops
    rng = np.random.default_rng(5)
    lists = _random_lists(rng, (10000,), 200, 1500000)
    assert merge_loops([[], lists[0]], (5000, 10000), 2) == [[], lists[0]]
    assert merge_loops([[], []], (5000, 10000), 2) == [[], []]
    assert merge_loops([lists[0]], (10000,), 2) == [lists[0]]
    with pytest.raises(ValueError):
        merge_loops([[], []], (10000, 5000), 2)
    with pytest.raises(ValueError):
        merge_loops([[], []], (5000, 10000), -1)


def test_the_resolutions_of_the_command_line():
    from mustache_amd.multires import MultiresError, parse_resolutions
    assert parse_resolutions(5000, ["25kb", "10000"]) == [10000, 25000]
    for bad, what in ((["10kb", "x"], "not a resolution"), (["5kb"], "greater than -r"), (["2kb"], "greater than -r"),
                      (["12kb"], "integer multiple"), (["10kb", "10000"], "given twice")):
        with pytest.raises(MultiresError, match=what):
            parse_resolutions(5000, bad)
