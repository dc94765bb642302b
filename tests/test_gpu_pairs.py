"""Read pairs -> pixels on the MI355X (mustache_amd/pairs.bin_pairs_device, csrc/mst_pairs.hip) against the restatement
(tests/pairs_reference.py): the pixel set and the dropped-row count are exact integers and must be equal, not close."""
import numpy as np
import pytest

import pairs_reference as pr

pytestmark = pytest.mark.gpu

WIDTH = 1 << 20                    # keys of the comparison: x * WIDTH + y (every test stays below 2^20 bins)


def _pixel_set(px):
    """(keys ascending, counts) of a Pixels result; the keys must be unique"""
    x = px.x.cpu().numpy().astype(np.int64)
    y = x + px.dist.cpu().numpy().astype(np.int64)
    c = px.count.cpu().numpy()
    assert c.dtype == np.int64 and (c > 0).all()
    key = x * WIDTH + y
    order = np.argsort(key, kind="stable")
    key, c = key[order], c[order]
    assert (np.diff(key) > 0).all(), "a pixel appears twice"
    return key, c


def _check(pos1, pos2, res, zero_based=False, length=None, **kw):
    from mustache_amd.pairs import bin_pairs_device
    pos1, pos2 = np.asarray(pos1, np.int32), np.asarray(pos2, np.int32)
    x, y, count, dropped = pr.pixels(pos1, pos2, res, zero_based, length)
    px = bin_pairs_device(pos1, pos2, res, zero_based=zero_based, length=length, **kw)
    key, c = _pixel_set(px)
    assert np.array_equal(key, x * WIDTH + y) and np.array_equal(c, count)
    assert px.dropped == dropped
    assert int(c.sum()) + dropped == len(pos1)
    assert px.n == (int(y.max()) + 1 if len(y) else 0)
    return px


def _random_rows(n_rows, top, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, top + 1, n_rows), rng.integers(1, top + 1, n_rows)


# the grid is at most 2048 workgroups that take 2048 rows a trip (8 groups of 64 per wave): 513 and 2049 end inside a wave's
# trip and inside a workgroup's, the last size takes a second trip of the grid-stride loop and is no multiple of the stride
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 257, 513, 2049, 2048 * 2048 + 321])
@pytest.mark.parametrize("dense_diags", [None, 0])
def test_row_counts(n_rows, dense_diags):
    a, b = _random_rows(n_rows, 40000, n_rows)
    b = np.where(np.arange(n_rows) % 3 == 0, a, b)           # a third of the rows on the diagonal
    px = _check(a, b, 100, length=40000, dense_diags=dense_diags, distance_bins=50)
    if n_rows == 0:
        assert len(px) == 0 and px.n == 0


def test_a_thousand_rows_in_one_pixel():
    for K in (None, 0):                                     # runs cross wave and workgroup edges; the count is 1 000
        px = _check(np.full(1000, 250), np.full(1000, 980), 100, length=1000, dense_diags=K)
        assert len(px) == 1 and int(px.count[0]) == 1000 and int(px.x[0]) == 2 and int(px.dist[0]) == 7
        assert px.far_entries == (0 if K is None else 16)    # one entry per wave: 1 000 rows are 16 waves


def test_two_pixels_alternating():
    a = np.where(np.arange(777) % 2 == 0, 150, 950)          # no two adjacent rows share a pixel
    for K in (None, 0):
        px = _check(a, np.full(777, 420), 100, length=1000, dense_diags=K)
        assert len(px) == 2 and sorted(px.count.cpu().tolist()) == [388, 389]
        assert px.far_entries == (0 if K is None else 777)


def test_runs_that_end_at_lane_63_and_at_lane_0():
    # wave 0: one run of 64 (ends at lane 63); wave 1: a run of 1 at lane 0, then a run to lane 63 that goes on through lane 0
    # of wave 2; then runs of 63 + 1 and a dropped row inside a run
    bins = [5] * 64 + [6] + [7] * 63 + [7] + [8] * 62 + [9] + [9] * 63 + [3]
    a = np.array(bins) * 100 + 1
    b = a.copy()
    b[200] = 0                                              # dropped: splits the run it stands in
    for K in (None, 0, 1):
        px = _check(a, b, 100, length=1000, dense_diags=K)
        assert px.dropped == 1
    px = _check(a, a + 500, 100, length=2000, dense_diags=0)
    # [5]*64 | [6] [7]*63 | [7] [8]*62 [9] | [9]*63 [3]
    assert px.far_entries == 1 + 2 + 3 + 2


def test_one_bin():
    a, b = _random_rows(300, 100, 3)
    px = _check(a, b, 100, length=100)
    assert len(px) == 1 and px.n == 1 and int(px.count[0]) == 300
    _check(a, b, 100, length=100, dense_diags=0)
    _check(a - 1, b - 1, 100, zero_based=True, length=100)


def test_keys_beyond_32_bits():
    rng = np.random.default_rng(9)                          # n = 100 000, pixels near bin 99 000: x * n + y > 2^32
    a = rng.integers(98900, 99100, 3000)
    b = a + rng.integers(0, 40, 3000)
    far = rng.integers(10, 500, 200)                        # and some far from the diagonal
    a, b = np.concatenate([a, far]), np.concatenate([b, far + rng.integers(90000, 99000, 200)])
    for K in (None, 0, 5):
        px = _check(a, b, 1, length=100000, distance_bins=20, dense_diags=K)
        assert px.n_alloc == 100000
    assert 99000 * 100000 + 99000 > 1 << 32


@pytest.mark.parametrize("K", [0, 1, 3, 1000])
def test_dense_diagonals(K):
    n, res = 70, 100
    x = np.arange(0, 60)
    rows_a, rows_b = [], []
    for d in sorted({max(K - 1, 0), K, K + 1, 0, 69} - {1000, 1001, 999}):
        xs = x[x + d < n]
        rows_a.append(xs * res + 1)
        rows_b.append((xs + d) * res + res)                 # the last position of bin x + d
    a, b = np.concatenate(rows_a + rows_b), np.concatenate(rows_b + rows_a)      # both orientations
    px = _check(a, b, res, length=n * res, dense_diags=K)
    assert px.dense_diags == min(K, n)                      # K > n is clamped
    dist = np.abs((b - 1) // res - (a - 1) // res)
    assert (px.far_entries > 0) == bool((dist >= K).any())
    if K >= n:
        assert px.far_entries == 0


def test_budget_sets_the_dense_diagonals(monkeypatch):
    a, b = _random_rows(2000, 7000, 12)
    n = 70
    for budget, want in ((4 * n * 3 + 5, 3), (0, 0), (1 << 30, 21), (4 * n - 1, 0)):
        monkeypatch.setenv("MUSTACHE_PAIRS_DENSE_BYTES", str(budget))
        px = _check(a, b, 100, length=7000, distance_bins=20)
        assert px.dense_diags == want                       # min(D + 1, n, budget // (4 n))
    monkeypatch.delenv("MUSTACHE_PAIRS_DENSE_BYTES")
    assert _check(a, b, 100, length=7000, distance_bins=20).dense_diags == 21


def test_far_list_filled_exactly_to_its_capacity():
    from mustache_amd._lib import MstOverflow
    from mustache_amd.pairs import bin_pairs_device
    a = (np.arange(500) % 7) * 100 + 1                      # no two adjacent rows share a pixel: 500 entries
    b = a + 2000
    px = _check(a, b, 100, length=3000, dense_diags=0, far_capacity=500)
    assert px.far_entries == 500 and len(px) == 7
    with pytest.raises(MstOverflow):                        # one slot short: counted, not written
        bin_pairs_device(a.astype(np.int32), b.astype(np.int32), 100, length=3000, dense_diags=0, far_capacity=499)


def test_heavy_multiplicity_sorted_shuffled_and_twice():
    rng = np.random.default_rng(21)
    a, b = rng.integers(1, 7001, 5000), rng.integers(1, 7001, 5000)             # 5 000 rows on n = 70
    order = np.lexsort((np.maximum(a, b), np.minimum(a, b)))
    sets = []
    for rows in ((a[order], b[order]), (a, b), (a, b), (b, a)):
        for K in (None, 0, 4):
            px = _check(rows[0], rows[1], 100, length=7000, dense_diags=K)
            sets.append(_pixel_set(px))
    for key, c in sets[1:]:
        assert np.array_equal(key, sets[0][0]) and np.array_equal(c, sets[0][1])
    assert sets[0][1].max() >= 3


@pytest.mark.parametrize("zero_based", [False, True])
def test_edge_positions(zero_based):
    res, length = 100, 1000
    edges = [0, 1, res, res + 1, length, length + 1, -1, -(1 << 31), (1 << 31) - 1]
    a = np.array([e for e in edges for _ in range(3)])
    b = np.array([p for _ in edges for p in (1, 5, length - 1)])
    for K in (None, 0):
        px = _check(np.concatenate([a, b]), np.concatenate([b, a]), res, zero_based=zero_based, length=length, dense_diags=K)
        assert px.dropped == 2 * 3 * 5          # 1-based: 0, length + 1 and the last three; 0-based: length instead of 0
    # without a length: no upper limit, the bin count comes from the largest position
    px = _check([1, 5, 100000, 0, -7], [2, 100000, 100000, 5, 5], res, zero_based=zero_based, dense_diags=2)
    assert px.n == (100000 - (0 if zero_based else 1)) // res + 1
    # nothing but dropped rows
    px = _check([-1, -2, 0 if not zero_based else -3], [5, 5, 5], res, zero_based=zero_based, length=length)
    assert len(px) == 0 and px.dropped == 3 and px.n == 0


def test_compact_alone():
    import torch
    from mustache_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(2)
    for K, n in ((1, 1), (3, 700), (5, 2048), (7, 1171)):   # one tile, a partial last tile, whole tiles, rows that straddle tiles
        total = K * n
        dense = np.zeros(total, np.uint32)
        at = np.unique(np.concatenate([rng.integers(0, total, total // 3 + 1), [0, total - 1, min(2047, total - 1), min(2048, total - 1)]]))
        dense[at] = rng.integers(1, 1 << 32, len(at), dtype=np.uint64).astype(np.uint32)          # counts beyond 2^31 stay exact
        d = torch.from_numpy(dense.view(np.int32)).to(dev)
        ws = torch.empty(int(lib.mst_pairs_compact_workspace_bytes(K, n)), dtype=torch.uint8, device=dev)
        for cap in (len(at), len(at) - 1 if len(at) > 1 else 0):
            x = torch.full((len(at) + 8,), -7, dtype=torch.int32, device=dev)
            dist, cnt = x.clone(), x.clone()
            found = torch.full((1,), -1, dtype=torch.int64, device=dev)
            _lib.check(lib.mst_pairs_compact(_lib.ptr(d), K, n, _lib.ptr(x), _lib.ptr(dist), _lib.ptr(cnt), cap, _lib.ptr(found),
                                             _lib.ptr(ws), ws.numel(), _lib.stream()))
            assert int(found.item()) == len(at)              # the count goes on past the capacity, the writes do not
            assert np.array_equal(x.cpu().numpy()[:cap], (at % n)[:cap]) and np.array_equal(dist.cpu().numpy()[:cap], (at // n)[:cap])
            assert np.array_equal(cnt.cpu().numpy()[:cap].view(np.uint32), dense[at][:cap])
            assert (x.cpu().numpy()[cap:] == -7).all() and (cnt.cpu().numpy()[cap:] == -7).all()
    found = torch.full((1,), -1, dtype=torch.int64, device=dev)
    _lib.check(lib.mst_pairs_compact(None, 0, 70, None, None, None, 0, _lib.ptr(found), None, 0, _lib.stream()))
    assert int(found.item()) == 0                            # K = 0: nothing to compact
    assert lib.mst_pairs_compact(None, 3, 70, None, None, None, 0, _lib.ptr(found), None, 0, _lib.stream()) == _lib.MST_E_ARG
    assert lib.mst_pairs_bin(None, None, 5, 100, 0, 1000, 10, 0, None, None, None, 0, None, None) == _lib.MST_E_ARG
    c = torch.zeros(2, dtype=torch.int64, device=dev)
    assert lib.mst_pairs_bin(None, None, 0, 100, 0, 1000, 10, 0, None, None, None, 0, _lib.ptr(c), None) == 0
    assert lib.mst_pairs_bin(None, None, 0, 100, 0, 1000, 10, 11, None, None, None, 0, _lib.ptr(c), None) == _lib.MST_E_ARG    # K > n
    torch.cuda.synchronize()


def test_the_far_list_sum():
    import torch
    from mustache_amd.pairs import sum_far_list
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 50, 4000) + (1 << 33)
    mult = rng.integers(1, 65, 4000).astype(np.int32)
    uk, counts = sum_far_list(torch.from_numpy(keys).to(dev), torch.from_numpy(mult).to(dev))
    want_k = np.unique(keys)
    assert np.array_equal(uk.cpu().numpy(), want_k)
    assert np.array_equal(counts.cpu().numpy(), np.array([mult[keys == k].sum() for k in want_k]))
    uk, counts = sum_far_list(torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
    assert uk.numel() == 0 and counts.numel() == 0 and counts.dtype == torch.int64
