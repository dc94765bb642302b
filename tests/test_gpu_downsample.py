"""mst_thin_counts (csrc/mst_thin.hip) and downsample.thin_records on the MI355X against the NumPy restatement of the rule
(tests/downsample_reference.py): the kept count of every pixel and the two totals, bit for bit."""
import numpy as np
import pytest

import downsample_reference as ref

pytestmark = pytest.mark.gpu

HEAVY = 256
# the places the kernel can go wrong: the 4-word boundary of a Philox call, the switch between the two paths, the masked last
# call of the heavy path, a heavy count that is not a multiple of 256
VALUES = [0, 1, 3, 4, 5, HEAVY - 1, HEAVY, HEAVY + 1, HEAVY + 2, 4 * 64 * 3 + 1, 100003]
THRESHOLDS = [1, 1 << 31, (1 << 32) - 1]


def _records(N, seed=5):
    """N pixels with distinct (x, dist) and counts cycling through VALUES (100 003 only among the first 130: the restatement
    draws every read)"""
    rng = np.random.default_rng(seed)
    key = rng.choice(4000 * 300, N, replace=False)
    counts = np.array([VALUES[i % len(VALUES)] if i < 130 or VALUES[i % len(VALUES)] < 100003 else 7 for i in range(N)], np.int64)
    return (key // 300).astype(np.int32), (key % 300).astype(np.int32), counts


def _thin(x, dist, counts, chromosome="chr1", T=1 << 31, seed=0, sample=0, dtype=None, draw=True):
    """the entry point itself -> (k, [sum in, sum kept, flag])"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr, stream
    from mustache_amd.downsample import chromosome_tag
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    dtype = dtype or torch.int64
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    dd = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.int32)).to(dev)
    cd = torch.from_numpy(np.ascontiguousarray(counts)).to(device=dev, dtype=dtype)
    kind = {torch.int64: 0, torch.float32: 1, torch.float64: 2}[dtype]
    words = torch.zeros(3, dtype=torch.int64, device=dev)
    k = torch.full((len(counts),), -7, dtype=torch.int64, device=dev) if draw else None
    _lib.check(lib.mst_thin_counts(ptr(xd), ptr(dd), ptr(cd), kind, len(counts), chromosome_tag(chromosome), seed, sample, T, ptr(k),
                                   ptr(words), stream()))
    return (k.cpu().numpy() if draw else None), words.cpu().tolist()


def _want(x, dist, counts, chromosome="chr1", T=1 << 31, seed=0, sample=0):
    x = np.asarray(x, np.int64)
    return ref.thin_counts(x, x + np.asarray(dist, np.int64), counts, ref.chromosome_tag(chromosome), T, seed, sample)


def _check(x, dist, counts, **kw):
    k, words = _thin(x, dist, counts, **kw)
    want = _want(x, dist, counts, **kw)
    print("pixels %d, reads %d, kept %d (restatement %d)" % (len(counts), words[0], words[1], int(want.sum())))
    assert np.array_equal(k, want)
    assert words == [int(np.sum(counts)), int(want.sum()), 0]
    return k


def test_header_constant():
    from mustache_amd import downsample
    assert downsample.HEAVY == HEAVY


@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 3001])
def test_against_the_restatement(N, T):
    x, dist, counts = _records(N)
    k = _check(x, dist, counts, T=T, seed=7)
    if T == 1:
        assert int(k.sum()) == 0 or int(k.sum()) < 3
    if T == (1 << 32) - 1:
        assert int((counts - k).sum()) < 3                     # all but the draws equal to 0xffffffff


@pytest.mark.parametrize("T", THRESHOLDS)
def test_a_wave_of_heavy_pixels(T):
    counts = np.array([HEAVY + 7 * i for i in range(64)], np.int64)
    _check(np.arange(64) + 100, np.arange(64) % 5, counts, T=T)


@pytest.mark.parametrize("lane", [0, 63])
@pytest.mark.parametrize("waves", [1, 5])
def test_one_heavy_lane(lane, waves):
    """one heavy lane in the first wave of each workgroup's worth of records, every other lane light"""
    counts = np.array([1, 3, 4, 5, HEAVY - 1, 0, 2, 9] * (8 * waves), np.int64)
    counts[lane] = 4 * 64 * 3 + 1
    if waves > 1:
        counts[64 * (waves - 1) + lane] = HEAVY + 2
    _check(np.arange(len(counts)) * 3, np.arange(len(counts)) % 11, counts, T=(1 << 31) + 12345, seed=1, sample=1)


def test_the_largest_bins():
    x = np.arange(189800, 190000)
    dist = 189999 - x                                          # every y is the last bin the project accepts
    counts = np.array(VALUES[:10] * 20, np.int64)
    _check(x, dist, counts, chromosome="chr2", T=3000000000)
    _check(np.full(10, 189999), np.zeros(10, np.int64), np.array(VALUES[:10], np.int64), T=1 << 30)


def test_tag_and_sample_change_the_result():
    x, dist, counts = _records(257)
    base = _check(x, dist, counts)
    other_tag = _check(x, dist, counts, chromosome="chr2")
    other_sample = _check(x, dist, counts, sample=1)
    other_seed = _check(x, dist, counts, seed=1)
    assert not np.array_equal(base, other_tag) and not np.array_equal(base, other_sample) and not np.array_equal(base, other_seed)
    assert np.array_equal(base, _thin(x, dist, counts, chromosome="1")[0])           # `chr1` and `1` are one chromosome


def test_order_and_repeats():
    x, dist, counts = _records(3001)
    k, words = _thin(x, dist, counts, seed=3)
    again, words_again = _thin(x, dist, counts, seed=3)
    assert np.array_equal(k, again) and words == words_again
    perm = np.random.default_rng(1).permutation(len(x))
    kp, words_p = _thin(x[perm], dist[perm], counts[perm], seed=3)
    assert np.array_equal(kp, k[perm]) and words_p == words


def test_float_counts_and_the_sum_alone():
    import torch
    x, dist, counts = _records(257)
    k, words = _thin(x, dist, counts)
    for dtype in (torch.float32, torch.float64):
        kf, wf = _thin(x, dist, counts.astype(np.float64), dtype=dtype)
        assert np.array_equal(kf, k) and wf == words
    none, only = _thin(x, dist, counts, draw=False)
    assert none is None and only == [int(counts.sum()), 0, 0]


@pytest.mark.parametrize("bad,dtype", [(-1, "int64"), (1 << 32, "int64"), (2.5, "float32"), (2.5, "float64"), (-3.0, "float32"),
                                       (float("nan"), "float64"), (float("inf"), "float32"), (4294967296.0, "float64")])
def test_a_bad_count_sets_the_flag(bad, dtype):
    import torch
    from mustache_amd.downsample import DownsampleError, depth_of, thin_records
    x, dist, counts = _records(130)
    good = _want(x, dist, counts)
    mixed = counts.astype(np.float64 if dtype != "int64" else np.int64)
    mixed[70] = bad
    k, words = _thin(x, dist, mixed, dtype=getattr(torch, dtype))
    expect = good.copy()
    expect[70] = 0                                             # a bad count counts as 0; the others are untouched
    assert np.array_equal(k, expect)
    assert words == [int(counts.sum()) - int(counts[70]), int(expect.sum()), 1]
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    args = (t(x, torch.int32), t(dist, torch.int32), t(mixed, getattr(torch, dtype)), "chr9")
    with pytest.raises(DownsampleError, match="chromosome chr9 holds a count that is not an integer"):
        thin_records(*args, 1 << 31)
    with pytest.raises(DownsampleError, match="chr9"):
        depth_of(*args)


def test_thin_records_drops_the_empty_pixels():
    import torch
    from mustache_amd.downsample import DownsampleError, depth_of, thin_records
    x, dist, counts = _records(3001)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    xd, dd, cd = t(x, torch.int32), t(dist, torch.int32), t(counts, torch.int64)
    want = _want(x, dist, counts, chromosome="chrX", T=1 << 30, seed=11, sample=1)
    (tx, td, tk), total, kept = thin_records(xd, dd, cd, "chrX", 1 << 30, seed=11, sample=1)
    keep = want > 0
    assert 0 < keep.sum() < len(want)
    assert np.array_equal(tx.cpu().numpy(), x[keep]) and np.array_equal(td.cpu().numpy(), dist[keep])
    assert np.array_equal(tk.cpu().numpy(), want[keep]) and tk.dtype == torch.int64
    assert (total, kept) == (int(counts.sum()), int(want.sum())) and depth_of(xd, dd, cd, "chrX") == total
    (fx, _, fk), ftotal, fkept = thin_records(xd, dd, cd.to(torch.float32), "chrX", 1 << 30, seed=11, sample=1)
    assert np.array_equal(fk.cpu().numpy(), want[keep]) and (ftotal, fkept) == (total, kept)
    for T in (0, 1 << 32):
        with pytest.raises(DownsampleError):
            thin_records(xd, dd, cd, "chrX", T)
    with pytest.raises(DownsampleError):
        thin_records(xd, dd, cd, "chrX", 1 << 31, seed=1 << 32)


def test_the_entry_point_refuses_a_threshold_out_of_range():
    from mustache_amd._lib import MstError
    x, dist, counts = _records(5)
    for T in (0, 1 << 32):
        with pytest.raises(MstError, match="mst_thin_counts"):
            _thin(x, dist, counts, T=T)


def test_a_library_without_the_entry_point_is_refused_by_name(monkeypatch):
    """a stub in place of the loaded library: everything but mst_thin_counts, as a build from before this kernel has it"""
    from mustache_amd import _lib
    assert "mst_thin_counts" in _lib.exported_symbols()
    real = _lib.load()
    assert hasattr(real, "mst_thin_counts") and real.mst_abi_revision() == _lib.MST_ABI_REVISION == 1       # added without a new revision

    class Stale:
        def __getattr__(self, name):
            if name == "mst_thin_counts":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(ImportError, match=r"lacks symbols \['mst_thin_counts'\] \(stale build\?\)"):
        _lib.load()
