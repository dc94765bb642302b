"""mst_coarsen_pairs / mst_coarsen_pairs_compact (csrc/mst_coarsen_pairs.hip) and multires.coarsen_pairs on the MI355X against the
plain-Python restatement of the rule (tests/coarsen_genome_reference.py): per pair the coarse pixels {(X, Y): count}, keys and
counts equal exactly, and the number of records dropped as outside."""
import numpy as np
import pytest

import coarsen_genome_reference as ref

pytestmark = pytest.mark.gpu


def _tables(n_a, n_b):
    """the [5][P] table of pairs.trans_tables for arbitrary rectangles (the limits, rows 0 and 1, are not looked at)"""
    t = np.zeros((5, len(n_a)), np.int64)
    t[2], t[3] = n_a, n_b
    cells = t[2] * t[3]
    t[4] = np.cumsum(cells) - cells
    return t, int(cells.sum())


def _segments(lens, n_a, n_b, k, seed=5, ordered=True):
    """lens[p] records of pair p inside its fine rectangle [0, n_a k) x [0, n_b k), counts 0 .. 40 (zeros among them); ordered:
    in cell order, as binned and thinned records come, so that runs of up to k lanes share a coarse cell"""
    rng = np.random.default_rng(seed + 13 * len(lens) + int(np.sum(lens)) + k)
    xs, ys = [], []
    for p, m in enumerate(lens):
        x, y = rng.integers(0, n_a[p] * k, m), rng.integers(0, n_b[p] * k, m)
        if ordered:
            o = np.lexsort((y, x))
            x, y = x[o], y[o]
        xs.append(x), ys.append(y)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(seg[-1])
    return (np.concatenate(xs).astype(np.int32) if N else np.zeros(0, np.int32),
            np.concatenate(ys).astype(np.int32) if N else np.zeros(0, np.int32), rng.integers(0, 41, N).astype(np.int64), seg)


def _device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _coarsen(x, y, c, seg, n_a, n_b, k, dtype=None, **kw):
    """multires.coarsen_pairs -> ({p: {(X, Y): count}}, stats); the records of a pair must come back in key order"""
    import torch
    from mustache_amd.multires import coarsen_pairs
    dev = _device()
    t, _ = _tables(n_a, n_b)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(dev)
    cd = torch.from_numpy(np.ascontiguousarray(c)).to(device=dev, dtype=dtype or torch.int64)
    stats = {}
    got = coarsen_pairs(xd, yd, cd, seg, t, k, stats=stats, **kw)
    out = {}
    for p, (X, Y, V) in got.items():
        assert X.dtype == torch.int32 and Y.dtype == torch.int32 and V.dtype == torch.float64 and V.device == dev
        X, Y, V = X.cpu().numpy().astype(np.int64), Y.cpu().numpy().astype(np.int64), V.cpu().numpy()
        key = X * int(n_b[p]) + Y
        assert len(key) and np.all(np.diff(key) > 0)                    # key order, every cell once
        assert np.all(V == np.floor(V))
        out[p] = {(a, b): int(v) for a, b, v in zip(X.tolist(), Y.tolist(), V.tolist())}
    return out, stats


def _check(x, y, c, seg, n_a, n_b, k, **kw):
    got, stats = _coarsen(x, y, c, seg, n_a, n_b, k, **kw)
    want, outside = ref.coarsen_pairs(x, y, c, seg, n_a, n_b, k)
    print("records %d, pairs %d, factor %d -> %d pixels (restatement %d), %s"
          % (len(x), len(n_a), k, sum(len(v) for v in got.values()), sum(len(v) for v in want.values()), stats))
    assert got == want
    assert stats["outside"] == outside
    assert stats["total"] == sum(sum(px.values()) for px in want.values())
    return got, stats


# ---- grid, pair count and segment shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_blocks", [0, 1, 2, 3])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257])
def test_one_pair(N, max_blocks):
    n_a, n_b = [5], [3]
    for k in (1, 2, 3, 7):
        x, y, c, seg = _segments([N], n_a, n_b, k)
        got, stats = _check(x, y, c, seg, n_a, n_b, k, max_blocks=max_blocks)
        if N == 0:
            assert got == {} and stats["pixels"] == 0                   # nothing is launched


SIX = [0, 1, 63, 300, 0, 700]                    # an empty first and an empty middle pair; boundaries inside a wave and a tile
SIX_A, SIX_B = [5, 3, 4, 17, 9, 23], [3, 5, 4, 11, 2, 31]


@pytest.mark.parametrize("max_blocks", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_six_pairs(k, max_blocks):
    x, y, c, seg = _segments(SIX, SIX_A, SIX_B, k)
    c[0] = 5                                     # pair 1's only record
    full = _tables(SIX_A, SIX_B)[1]
    a, _ = _check(x, y, c, seg, SIX_A, SIX_B, k, max_blocks=max_blocks, dense_cells=full)
    b, stats = _check(x, y, c, seg, SIX_A, SIX_B, k, max_blocks=max_blocks, dense_cells=0)
    assert a == b and sorted(a) == [1, 2, 3, 5] and stats["dense_cells"] == 0


@pytest.mark.parametrize("k", [1, 3])
def test_forty_small_pairs(k):
    rng = np.random.default_rng(40)
    lens = rng.integers(1, 6, 40).tolist()       # 1 to 5 records each: one wave spans many pairs
    n_a, n_b = rng.integers(1, 7, 40).tolist(), rng.integers(1, 7, 40).tolist()
    x, y, c, seg = _segments(lens, n_a, n_b, k)
    c[:] = np.maximum(c, 1)
    got, _ = _check(x, y, c, seg, n_a, n_b, k, dense_cells=0)
    assert sorted(got) == list(range(40))
    assert _check(x, y, c, seg, n_a, n_b, k)[0] == got


def test_a_factor_larger_than_every_chromosome():
    lens, k = [70, 0, 5, 200], 1000
    x, y, c, seg = _segments(lens, [1] * 4, [1] * 4, k)
    c[:] = np.maximum(c, 1)
    for dense in (None, 0):
        got, _ = _check(x, y, c, seg, [1] * 4, [1] * 4, k, dense_cells=dense)
        assert got == {p: {(0, 0): int(c[seg[p]:seg[p + 1]].sum())} for p in (0, 2, 3)}      # one cell per pair


# ---- runs of equal keys ---------------------------------------------------------------------------------------------------------
def _heads(keys):
    """the runs a wave-wise combining sees: a record starts one at lane 0 and where its key differs from the one before"""
    keys = np.asarray(keys)
    start = np.ones(len(keys), bool)
    start[1:] = keys[1:] != keys[:-1]
    start[::64] = True
    return int(start.sum())


@pytest.mark.parametrize("dense", [0, None])
def test_runs_of_8_9_and_70_lanes(dense):
    n_a, n_b, k = [9], [7], 2
    cells = [(0, 0)] * 3 + [(1, 2)] * 8 + [(3, 3)] * 9 + [(8, 6)] * 70 + [(2, 5)] * 2 + [(1, 2)] * 5
    rng = np.random.default_rng(8)
    x = np.array([a * k + rng.integers(0, k) for a, _ in cells], np.int32)
    y = np.array([b * k + rng.integers(0, k) for _, b in cells], np.int32)
    c = rng.integers(1, 100, len(cells)).astype(np.int64)
    got, stats = _check(x, y, c, [0, len(cells)], n_a, n_b, k, dense_cells=dense)
    assert got[0][(1, 2)] == int(c[3:11].sum() + c[-5:].sum()) and got[0][(8, 6)] == int(c[20:90].sum())
    if dense == 0:                               # every count is > 0: one far entry per run of a wave, not one per record
        assert stats["far_entries"] == _heads([a * 7 + b for a, b in cells]) == 7 < len(cells)


@pytest.mark.parametrize("dense", [0, None])
def test_equal_cells_of_consecutive_pairs_do_not_combine(dense):
    n_a, n_b, k = [4, 4, 4], [3, 3, 3], 2
    x = np.array([2] * 10 + [3] * 10 + [2] * 30, np.int32)           # X = 1 everywhere
    y = np.array([2] * 10 + [2] * 10 + [3] * 30, np.int32)           # Y = 1 everywhere
    c = np.arange(1, 51, dtype=np.int64)
    got, _ = _check(x, y, c, [0, 10, 20, 50], n_a, n_b, k, dense_cells=dense)
    assert got == {0: {(1, 1): 55}, 1: {(1, 1): 155}, 2: {(1, 1): int(c[20:].sum())}}   # the runs meet inside one wave


# ---- outside records ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [0, None])
def test_outside_records_are_dropped_and_counted(dense):
    k, n_a, n_b = 2, [5, 5], [3, 3]
    # pair 0: Y == n_b (would read as (X + 1, 0)), X == n_a (would read as pair 1's first row), negative bins; pair 1: inside
    x = np.array([0, 0, 2, 10, 11, -1, 3, 9, 1, 0], np.int32)
    y = np.array([1, 6, 7, 0, 5, 2, -4, 5, 1, 3], np.int32)
    c = np.array([5, 7, 11, 13, 17, 19, 23, 29, 2, 31], np.int64)
    got, stats = _check(x, y, c, [0, 8, 10], n_a, n_b, k, dense_cells=dense)
    assert got == {0: {(0, 0): 5, (4, 2): 29}, 1: {(0, 0): 2, (0, 1): 31}} and stats["outside"] == 6
    # the last pair's X == n_a would lie past every cell: nothing is written there either
    got, stats = _check(np.array([10, 3], np.int32), np.array([0, 3], np.int32), np.array([4, 6], np.int64), [0, 0, 2], n_a, n_b, k,
                        dense_cells=dense)
    assert got == {1: {(1, 1): 6}} and stats["outside"] == 1


# ---- the dense split ------------------------------------------------------------------------------------------------------------
def test_the_dense_split_changes_nothing():
    from mustache_amd._lib import MstOverflow
    k = 3
    x, y, c, seg = _segments(SIX, SIX_A, SIX_B, k, ordered=False)
    c[:] = np.maximum(c, 1)
    t, full = _tables(SIX_A, SIX_B)
    cut = int(t[4][3] + SIX_A[3] * SIX_B[3] // 2 + 1)                # in the middle of pair 3, inside a row
    sets = []
    for dense in (0, full, cut, full + 1000, None):
        got, stats = _check(x, y, c, seg, SIX_A, SIX_B, k, dense_cells=dense)
        assert stats["dense_cells"] == (full if dense is None or dense > full else dense)
        assert (stats["far_entries"] == 0) == (stats["dense_cells"] == full)
        sets.append(got)
    assert all(s == sets[0] for s in sets)
    assert _check(x, y, c, seg, SIX_A, SIX_B, k, dense_bytes=8 * full - 1)[1]["dense_cells"] == 0       # 8 bytes per cell
    assert _check(x, y, c, seg, SIX_A, SIX_B, k, dense_bytes=8 * full)[1]["dense_cells"] == full
    with pytest.raises(MstOverflow, match="far list"):
        _coarsen(x, y, c, seg, SIX_A, SIX_B, k, dense_cells=0, far_capacity=5)
    assert _coarsen(x, y, c, seg, SIX_A, SIX_B, k, dense_cells=full, far_capacity=0)[0] == sets[0]


# ---- counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [0, None])
def test_large_counts_zeros_and_the_three_types(dense):
    import torch
    n_a, n_b, k = [3, 2], [2, 2], 2
    x = np.array([0, 1, 0, 4, 5, 2, 0, 1], np.int32)
    y = np.array([0, 1, 1, 2, 3, 0, 0, 0], np.int32)
    c = np.array([2 ** 31, 2 ** 31, 2 ** 31, 2 ** 32 - 1, 0, 0, 7, 0], np.int64)
    got, _ = _check(x, y, c, [0, 6, 8], n_a, n_b, k, dense_cells=dense)
    assert got == {0: {(0, 0): 3 * 2 ** 31, (2, 1): 2 ** 32 - 1}, 1: {(0, 0): 7}}          # count-0 records make no pixel
    assert _check(x, y, c, [0, 6, 8], n_a, n_b, k, dense_cells=dense, dtype=torch.float64)[0] == got
    c32 = np.array([2 ** 31, 2 ** 31, 2 ** 31, 2 ** 24, 0, 0, 7, 0], np.int64)             # what float32 holds exactly
    want = {0: {(0, 0): 3 * 2 ** 31, (2, 1): 2 ** 24}, 1: {(0, 0): 7}}
    assert _check(x, y, c32, [0, 6, 8], n_a, n_b, k, dense_cells=dense, dtype=torch.float32)[0] == want


def _raw(x, y, counts, seg, n_a, n_b, k, dense_cells):
    """the kernel itself -> (words, the dense counters, the far list's (key, count) sorted)"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr, stream
    from mustache_amd.multires import _COUNT_KIND
    lib, dev = _lib.require_gpu(), _device()
    t, _ = _tables(n_a, n_b)
    P, N = len(n_a), len(x)
    td = torch.from_numpy(np.concatenate([t[2], t[3], t[4], np.asarray(seg, np.int64)])).to(dev)
    xd, yd = torch.from_numpy(np.asarray(x, np.int32)).to(dev), torch.from_numpy(np.asarray(y, np.int32)).to(dev)
    cd = counts.to(dev)
    dense = torch.zeros(max(dense_cells, 1), dtype=torch.int64, device=dev)
    fk, fc = torch.full((N,), -7, dtype=torch.int64, device=dev), torch.full((N,), -7, dtype=torch.int64, device=dev)
    words = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.check(lib.mst_coarsen_pairs(ptr(xd), ptr(yd), ptr(cd), _COUNT_KIND[str(cd.dtype)], N, ptr(td[3 * P:]), ptr(td[:P]),
                                     ptr(td[P:2 * P]), ptr(td[2 * P:3 * P]), P, k, dense_cells, ptr(dense) if dense_cells else None,
                                     ptr(fk), ptr(fc), N, ptr(words), 0, stream()))
    torch.cuda.synchronize()
    w = words.cpu().tolist()
    return w, dense.cpu().numpy()[:dense_cells], sorted(zip(fk[:w[0]].cpu().tolist(), fc[:w[0]].cpu().tolist()))


@pytest.mark.parametrize("bad", [0.5, -1.0, float("nan"), 2.0 ** 32])
def test_a_bad_count_sets_the_flag_and_counts_as_zero(bad):
    import torch
    from mustache_amd.multires import MultiresError
    n_a, n_b, k = [3, 2], [2, 2], 2
    x, y, seg = [0, 1, 4, 2, 3], [0, 0, 3, 2, 3], [0, 3, 5]
    for dtype in (torch.float64, torch.float32) + ((torch.int64,) if bad == -1.0 else ()):
        good = torch.tensor([3, 4, 5, 6, 7], dtype=dtype)
        for at in (1, 3):
            c = good.clone()
            c[at] = bad
            zeroed = good.clone()
            zeroed[at] = 0
            for dense_cells in (0, 10):
                w, dense, far = _raw(x, y, c, seg, n_a, n_b, k, dense_cells)
                w0, dense0, far0 = _raw(x, y, zeroed, seg, n_a, n_b, k, dense_cells)
                assert w[2] == 1 and w0[2] == 0 and w[3] == w0[3] == 0
                assert w[1] == w0[1] == 25 - int(good[at]) and w[0] == w0[0]
                assert np.array_equal(dense, dense0) and far == far0
            with pytest.raises(MultiresError, match="not an integer between 0 and 4294967295"):
                _coarsen(x, y, c.numpy(), seg, n_a, n_b, k, dtype=dtype)


# ---- order ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [0, None])
def test_a_permutation_inside_each_segment_gives_the_same_set(dense):
    k = 3
    x, y, c, seg = _segments(SIX, SIX_A, SIX_B, k)
    want, _ = _check(x, y, c, seg, SIX_A, SIX_B, k, dense_cells=dense)
    rng = np.random.default_rng(1)
    order = np.concatenate([seg[p] + rng.permutation(int(seg[p + 1] - seg[p])) for p in range(len(SIX))]).astype(np.int64)
    assert _check(x[order], y[order], c[order], seg, SIX_A, SIX_B, k, dense_cells=dense)[0] == want


@pytest.mark.parametrize("k", [1, 2, 7])
def test_one_pair_above_the_diagonal_equals_coarsen_records(k):
    import torch
    from mustache_amd.multires import coarsen_records
    rng = np.random.default_rng(17)
    n = 90
    x = rng.integers(0, n, 3000)
    y = np.minimum(x + rng.integers(0, 25, 3000), n - 1)
    c = rng.integers(0, 9, 3000).astype(np.int64)
    m = (n - 1) // k + 1
    got, _ = _check(x.astype(np.int32), y.astype(np.int32), c, [0, 3000], [m], [m], k)
    dev = _device()
    X, D, C = coarsen_records(torch.from_numpy(x.astype(np.int32)).to(dev), torch.from_numpy((y - x).astype(np.int32)).to(dev),
                              torch.from_numpy(c).to(dev), k)
    X, D, C = X.cpu().numpy().astype(np.int64), D.cpu().numpy().astype(np.int64), C.cpu().numpy()
    assert got[0] == {(a, a + d): int(v) for a, d, v in zip(X.tolist(), D.tolist(), C.tolist())}


# ---- the library ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mst_coarsen_pairs", "mst_coarsen_pairs_compact", "mst_coarsen_pairs_compact_workspace_bytes"])
def test_a_library_without_the_entry_point_is_refused_by_name(monkeypatch, name):
    from mustache_amd import _lib
    assert name in _lib.exported_symbols()
    real = _lib.load()
    assert hasattr(real, name) and real.mst_abi_revision() == _lib.MST_ABI_REVISION == 1       # added without a new revision

    class Stale:
        def __getattr__(self, attr):
            if attr == name:
                raise AttributeError(attr)
            return getattr(real, attr)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(ImportError, match=r"lacks symbols \['%s'\] \(stale build\?\)" % name):
        _lib.load()
