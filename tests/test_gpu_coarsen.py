"""mst_coarsen_records / mst_coarsen_compact (csrc/mst_coarsen.hip) and multires.coarsen_records on the MI355X against the NumPy
restatement of the rule (tests/multires_reference.py): the coarse pixels as sorted (X, D, count) triples, exactly."""
import numpy as np
import pytest

import multires_reference as ref

pytestmark = pytest.mark.gpu

BINS = 1500


def _records(N, seed=3, bins=BINS):
    """N records, most of them near the diagonal, some anywhere, a few pixels listed twice; counts 1 .. 40 and a few zeros"""
    rng = np.random.default_rng(seed + N)
    x = rng.integers(0, bins, N)
    d = np.where(rng.random(N) < 0.8, rng.integers(0, 12, N), rng.integers(0, bins, N))
    d = np.minimum(d, bins - 1 - x)
    c = rng.integers(0, 41, N)
    if N > 10:
        x[N // 2], d[N // 2] = x[0], d[0]
    return x.astype(np.int32), d.astype(np.int32), c.astype(np.int64)


def _coarsen(x, d, c, k, dtype=None, **kw):
    """multires.coarsen_records -> (the sorted triples, stats)"""
    import torch
    from mustache_amd.multires import coarsen_records
    dev = torch.device("cuda", torch.cuda.current_device())
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    dd = torch.from_numpy(np.ascontiguousarray(d, dtype=np.int32)).to(dev)
    cd = torch.from_numpy(np.ascontiguousarray(c)).to(device=dev, dtype=dtype or torch.int64)
    stats = {}
    X, D, C = coarsen_records(xd, dd, cd, k, stats=stats, **kw)
    assert X.dtype == torch.int32 and D.dtype == torch.int32 and C.dtype == torch.int64 and X.device == dev
    return ref.triples(X.cpu().numpy(), D.cpu().numpy(), C.cpu().numpy()), stats


def _check(x, d, c, k, **kw):
    got, stats = _coarsen(x, d, c, k, **kw)
    want = ref.triples(*ref.coarsen(x, d, c, k))
    print("records %d, factor %d -> %d pixels (restatement %d), %s" % (len(x), k, len(got), len(want), stats))
    assert got == want
    if len(x):
        assert stats["total"] == int(np.sum(np.asarray(c, dtype=object))) == sum(t[2] for t in got)
    return got, stats


@pytest.mark.parametrize("k", [1, 2, 3, 5, BINS + 7])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 64 * 5 + 1, 20000])
def test_against_the_restatement(N, k):
    x, d, c = _records(N)
    got, _ = _check(x, d, c, k)
    if k > BINS and N:
        assert got == [(0, 0, int(c.sum()))] or c.sum() == 0            # a factor above n: everything lands in pixel (0, 0)
    if k == 1:                                                          # the identity, but for the pixels listed twice
        assert len(got) <= np.count_nonzero(c) and (N < 20000 or len(got) < np.count_nonzero(c))


@pytest.mark.parametrize("k", [2, 5])
def test_the_dense_split(k):
    x, d, c = _records(20000, seed=11)
    n = (BINS - 1) // k + 1
    all_far, s0 = _check(x, d, c, k, dense_diags=0)
    all_near, s1 = _check(x, d, c, k, dense_diags=n)
    some, s2 = _check(x, d, c, k, dense_diags=4)
    default, s3 = _check(x, d, c, k, distance_bins=6)
    assert all_far == all_near == some == default
    assert s0["dense_diags"] == 0 and s0["far_entries"] > 0
    assert s1["dense_diags"] == n == s1["n"] and s1["far_entries"] == 0
    assert s2["dense_diags"] == 4 and 0 < s2["far_entries"] < s0["far_entries"]
    assert s3["dense_diags"] == 7                                        # D + 1
    # a far list too small for its entries is an error, not a loss
    from mustache_amd._lib import MstOverflow
    with pytest.raises(MstOverflow):
        _coarsen(x, d, c, k, dense_diags=0, far_capacity=10)


def test_the_diagonals_at_the_split_and_the_coarse_boundaries():
    k, K = 5, 3
    # D = K - 1 and D = K from every offset inside the coarse bins; fine records with d > 0 whose ends share a coarse bin
    # (D = 0); records that straddle a coarse boundary by one fine bin (D = 1 with d = 1)
    x, d = [], []
    for X in (0, 7, 40):
        for a in range(k):
            for b in range(k):
                for D in (K - 1, K):
                    x.append(X * k + a)
                    d.append((X + D) * k + b - (X * k + a))
            for dd in range(1, k - a):
                x.append(X * k + a)                                      # ends share the coarse bin
                d.append(dd)
        x += [X * k + k - 1, X * k + k - 1]
        d += [1, 0]                                                      # the straddler (D = 1) and its neighbour on the diagonal
    x, d = np.array(x), np.array(d)
    c = np.arange(1, len(x) + 1)
    got, stats = _check(x, d, c, k, dense_diags=K)
    assert stats["dense_diags"] == K and stats["far_entries"] > 0
    by_pixel = {(t[0], t[1]): t[2] for t in got}
    assert {D for _, D in by_pixel} == {0, 1, K - 1, K}
    for X in (0, 7, 40):
        assert by_pixel[(X, K - 1)] == sum(int(cc) for xx, dd, cc in zip(x, d, c) if xx // k == X and (xx + dd) // k == X + K - 1)
        assert by_pixel[(X, K)] == sum(int(cc) for xx, dd, cc in zip(x, d, c) if xx // k == X and (xx + dd) // k == X + K)
    for K2 in (0, 1, 2, 4, 5):
        assert _check(x, d, c, k, dense_diags=K2)[0] == got


@pytest.mark.parametrize("K", [0, 4])
def test_runs_of_equal_keys_in_a_wave(K):
    # all 64 lanes of a wave on one key (two waves of it, then a third key)
    x = np.concatenate([np.arange(64), np.arange(64) + 64, [700]])
    d = np.zeros(len(x), np.int64)
    c = np.arange(1, len(x) + 1)
    got, _ = _check(x, d, c, 64, dense_diags=K)
    assert got == [(0, 0, sum(range(1, 65))), (1, 0, sum(range(65, 129))), (10, 0, 129)]
    # a run whose head is lane 63 and which continues in the next wave; before it 63 keys of their own
    x = np.concatenate([np.arange(63) * 3, np.full(9, 600)])
    c = np.arange(1, len(x) + 1)
    got, _ = _check(x, np.zeros(len(x), np.int64), c, 3, dense_diags=K)
    assert got[-1] == (200, 0, sum(range(64, 73))) and len(got) == 64
    # runs of every length from 1 to 20 in turn (short runs are summed lane by lane, long ones by log steps), twice over
    x = np.concatenate([np.full(length, 5 * j) for j, length in enumerate(list(range(1, 21)) * 2)])
    c = np.arange(1, len(x) + 1)
    got, _ = _check(x, np.zeros(len(x), np.int64), c, 5, dense_diags=K)
    assert len(got) == 40
    # alternating keys: no two neighbours share one
    x = np.tile([10, 20], 100)
    got, _ = _check(x, np.ones(200, np.int64), np.arange(200), 2, dense_diags=K)
    assert got == [(5, 0, sum(range(0, 200, 2))), (10, 0, sum(range(1, 200, 2)))]
    # far keys in runs: the same shapes off the dense diagonals
    x = np.repeat(np.arange(40) * 2, 2) + np.tile([0, 1], 40)
    got, stats = _check(x, np.full(80, 900), np.arange(1, 81), 2, dense_diags=K)
    assert len(got) == 40 and stats["far_entries"] == 40                 # one entry per run of two


def test_the_order_of_the_records_does_not_matter():
    x, d, c = _records(20000, seed=21)
    order = np.lexsort((x, d))                                           # as the binning's compaction emits them
    sorted_set, _ = _check(x[order], d[order], c[order], 5, dense_diags=8)
    rng = np.random.default_rng(1)
    for _ in range(2):
        p = rng.permutation(len(x))
        assert _coarsen(x[p], d[p], c[p], 5, dense_diags=8)[0] == sorted_set


def test_the_count_types_and_the_sums_beyond_32_bits():
    import torch
    x, d, c = _records(3001, seed=31)
    want, _ = _check(x, d, c, 3)
    for dtype in (torch.float32, torch.float64):
        assert _coarsen(x, d, c, 3, dtype=dtype)[0] == want
    # three records of 2^31 into one cell -> 3 * 2^31, dense and far, in a run and apart
    big = 1 << 31
    for xs in ([4, 5, 4], [4, 4, 5], [4, 900, 5, 901, 4]):
        cs = [big if v < 900 else 1 for v in xs]
        for K in (0, 2):
            for dtype in (torch.int64, torch.float32, torch.float64):
                got, _ = _coarsen(xs, [0] * len(xs), cs, 2, dtype=dtype, dense_diags=K)
                assert (2, 0, 3 * big) in got and sum(t[2] for t in got) == sum(cs)
    # the largest count there is, 64 times into one cell: a whole wave's run
    top = (1 << 32) - 1
    for K in (0, 1):
        got, stats = _coarsen(np.arange(64), np.zeros(64, np.int64), np.full(64, top), 64, dense_diags=K)
        assert got == [(0, 0, 64 * top)] and stats["total"] == 64 * top


@pytest.mark.parametrize("bad,dtype", [(0.5, "float32"), (2.25, "float64"), (-1, "int64"), (-1.0, "float64"), (1 << 32, "int64"),
                                       (4294967296.0, "float64"), (float("nan"), "float32"), (float("inf"), "float64")])
def test_a_count_that_is_no_integer_in_range_sets_the_flag(bad, dtype):
    import torch
    from mustache_amd.multires import MultiresError
    x, d, c = _records(500, seed=41)
    c = c.astype(np.float64 if "float" in dtype else np.int64)
    c[333] = bad
    with pytest.raises(MultiresError, match=r"chromosome chr7 holds a count that is not an integer between 0 and 4294967295"):
        _coarsen(x, d, c, 2, dtype=getattr(torch, dtype), chromosome="chr7")
    c[333] = (1 << 32) - 1                                               # the largest count is one
    _coarsen(x, d, c, 2, dtype=getattr(torch, dtype) if dtype != "float32" else torch.float64)


def test_the_entry_point_refuses_bad_arguments_and_records_outside_the_map():
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import MstError, ptr, stream
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    xd = torch.tensor([3, 9], dtype=torch.int32, device=dev)
    dd = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    cd = torch.tensor([5, 6], dtype=torch.int64, device=dev)
    words = torch.zeros(3, dtype=torch.int64, device=dev)
    key, cnt = torch.full((2,), -7, dtype=torch.int64, device=dev), torch.full((2,), -7, dtype=torch.int64, device=dev)
    for factor, n, K, kind in ((0, 5, 0, 0), (1, 0, 0, 0), (1, 5, 6, 0), (1, 5, 0, 3)):
        with pytest.raises(MstError, match="mst_coarsen_records"):
            _lib.check(lib.mst_coarsen_records(ptr(xd), ptr(dd), ptr(cd), kind, 2, factor, n, K, None, ptr(key), ptr(cnt), 2, ptr(words),
                                               stream()))
    # n = 3 coarse bins at factor 2: the pixel (3, 4) goes to (1, 2), the record at bin 9 lies outside; it is read, not written
    _lib.check(lib.mst_coarsen_records(ptr(xd), ptr(dd), ptr(cd), 0, 2, 2, 3, 0, None, ptr(key), ptr(cnt), 2, ptr(words), stream()))
    assert words.cpu().tolist() == [1, 11, 0]
    assert key.cpu().tolist() == [1 * 3 + 2, -7] and cnt.cpu().tolist() == [5, -7]
    from mustache_amd.multires import coarsen_records
    with pytest.raises(ValueError):
        coarsen_records(xd, dd, cd, 0)
    with pytest.raises(TypeError):
        coarsen_records(xd, dd, cd.to(torch.int32), 2)


@pytest.mark.parametrize("k", [2, 5])
def test_coarsening_the_binned_pairs_is_binning_them_coarser(k):
    """20 000 random read pairs in a 300-bin chromosome: coarsen_records(bin_pairs_device(pos, r), k) and
    bin_pairs_device(pos, r k) are the same pixel set"""
    from mustache_amd.pairs import bin_pairs_device
    rng = np.random.default_rng(50 + k)
    r, length = 700, 700 * 300 - 11
    p1 = rng.integers(1, length + 1, 20000)
    p2 = np.where(rng.random(20000) < 0.7, np.clip(p1 + rng.integers(-9000, 9000, 20000), 1, length), rng.integers(1, length + 1, 20000))
    fine = bin_pairs_device(p1.astype(np.int32), p2.astype(np.int32), r, length=length, distance_bins=20)
    coarse = bin_pairs_device(p1.astype(np.int32), p2.astype(np.int32), r * k, length=length, distance_bins=20 // k)
    assert len(fine) > len(coarse) > 0 and int(fine.count.sum()) == 20000
    from mustache_amd.multires import coarsen_records
    for K in (None, 0, 3):
        X, D, C = coarsen_records(fine.x, fine.dist, fine.count, k, dense_diags=K)
        assert ref.triples(X.cpu().numpy(), D.cpu().numpy(), C.cpu().numpy()) == \
            ref.triples(coarse.x.cpu().numpy(), coarse.dist.cpu().numpy(), coarse.count.cpu().numpy())


def test_a_library_without_the_entry_point_is_refused_by_name(monkeypatch):
    """a stub in place of the loaded library: everything but mst_coarsen_records, as a build from before this kernel has it"""
    from mustache_amd import _lib
    assert {"mst_coarsen_records", "mst_coarsen_compact", "mst_coarsen_compact_workspace_bytes"} <= set(_lib.exported_symbols())
    real = _lib.load()
    assert hasattr(real, "mst_coarsen_records") and real.mst_abi_revision() == _lib.MST_ABI_REVISION == 1   # added without a new revision

    class Stale:
        def __getattr__(self, name):
            if name == "mst_coarsen_records":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(ImportError, match=r"lacks symbols \['mst_coarsen_records'\] \(stale build\?\)"):
        _lib.load()
