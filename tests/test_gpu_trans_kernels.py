"""The trans kernels of csrc/mst_trans.hip one by one on the MI355X: mst_trans_zscore bit for bit against exactly rounded
arithmetic (trans_reference.zscore_exact: math.fsum, one rounding per sum), mst_trans_scatter_tiles and mst_trans_prologue
against a NumPy scatter, array for array."""
import math

import numpy as np
import pytest

import trans_reference as tr

pytestmark = pytest.mark.gpu


# ---- A. the z-score ------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _device(v):
    from mustache_amd.trans import zscore_device
    z, mean, std, n = zscore_device(np.asarray(v, np.float64))
    assert n == len(v)
    return z.cpu().numpy(), mean, std


def _same_bits(a, b):
    return bool(_bits([a])[0] == _bits([b])[0]) or (math.isnan(a) and math.isnan(b))


def _assert_exact(v, what):
    """device (z, mean, std) bit-identical to zscore_exact, for v, for a random permutation of v, and for v repeated (the
    same mean; the same std when the sum of squares doubles exactly, which it does: every term appears twice)"""
    v = np.asarray(v, np.float64)
    ze, me, se = tr.zscore_exact(v)
    z, m, s = _device(v)
    assert _same_bits(m, me), (what, "mean", float(m).hex(), float(me).hex())
    assert _same_bits(s, se), (what, "std", float(s).hex(), float(se).hex())
    assert np.array_equal(_bits(z), _bits(ze)), (what, "z", int((_bits(z) != _bits(ze)).sum()))
    perm = np.random.default_rng(len(v)).permutation(len(v))
    zp, mp, sp = _device(v[perm])
    assert _same_bits(mp, me) and _same_bits(sp, se), (what, "permuted")
    assert np.array_equal(_bits(zp), _bits(ze[perm])), (what, "permuted z")
    if 2 * len(v) < (1 << 23) and float(np.abs(v).max()) * 2 * len(v) < 1e308:
        v2 = np.concatenate([v, v])
        z2e, m2e, s2e = tr.zscore_exact(v2)
        z2, m2, s2 = _device(v2)
        assert _same_bits(m2, m2e) and _same_bits(s2, s2e), (what, "repeated")
        assert np.array_equal(_bits(z2), _bits(z2e)), (what, "repeated z")


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65537, 3000017])
def test_zscore_is_exact_at_every_size(n):
    rng = np.random.default_rng(n)
    _assert_exact(np.exp(rng.normal(0.0, 1.5, n)) * 10.0, "n=%d" % n)


def test_zscore_of_no_record_leaves_out_alone():
    import torch
    from mustache_amd import _lib
    from mustache_amd.engine import require_gpu
    from mustache_amd.trans import _ptr, _stream
    lib = require_gpu()
    out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    stats = torch.full((4,), 5.0, dtype=torch.float64, device="cuda")
    nb = int(lib.mst_trans_zscore_workspace_bytes())
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    _lib.check(lib.mst_trans_zscore(None, 0, None, _ptr(stats), _ptr(ws), nb, _stream()))
    _lib.check(lib.mst_trans_zscore(_ptr(out), 0, _ptr(out), _ptr(stats), _ptr(ws), nb, _stream()))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    assert (stats.cpu().numpy() == 0.0).all()


def _range_cases():
    rng = np.random.default_rng(5)
    tiny = 2.0 ** -1074
    yield "all subnormal", rng.integers(1, 1 << 50, 1000).astype(np.float64) * tiny
    yield "three subnormals", np.array([tiny, 3 * tiny, 5 * tiny])
    yield "1e-300 .. 1e300", 10.0 ** rng.uniform(-300, 300, 4099)          # squares overflow: std NaN on both sides
    yield "1e-150 .. 1e150", 10.0 ** rng.uniform(-150, 150, 4099)
    n = 1000
    yield "near DBL_MAX / n", rng.uniform(0.5, 0.999, n) * (np.finfo(np.float64).max / n)
    yield "squares near DBL_MAX / n", rng.uniform(0.5, 0.999, n) * 1e152
    yield "sum of squares past DBL_MAX", rng.uniform(0.5, 0.999, n) * 1e154      # std = inf, every v' = +-0
    yield "one huge among tiny", np.concatenate([[2.0 ** 400], rng.uniform(1.0, 2.0, 777) * 2.0 ** 347])
    # ulp(2^400) = 2^348: 1024 x 2^337 is half of it (a tie, to even: the tiny ones vanish), one more of them moves the bit
    yield "one huge, tiny ones add up to half its ulp", np.concatenate([[2.0 ** 400], np.full(1024, 2.0 ** 337)])
    yield "one huge, tiny ones add up past half its ulp", np.concatenate([[2.0 ** 400], np.full(1025, 2.0 ** 337)])
    yield "1e8 + noise", 1e8 + rng.normal(0.0, 1e-3, 50001)
    yield "1e8 + tiny noise", 1e8 + rng.integers(-3, 4, 4097) * 2.0 ** -26
    yield "all equal", np.full(1000, 0.1)
    yield "all equal, one record short of a workgroup", np.full(255, 1e300)
    yield "negative and positive", rng.normal(0.0, 3.0, 70001)
    yield "all negative", -np.exp(rng.normal(0.0, 2.0, 513))
    yield "cancelling to a small total", np.concatenate([rng.uniform(1, 2, 500) * 2.0 ** 80, -rng.uniform(1, 2, 500) * 2.0 ** 80, [3.0]])
    yield "signed zeros among values", np.array([0.0, -0.0, 1.5, -0.0, 2.5, 0.0])


@pytest.mark.parametrize("name,v", list(_range_cases()), ids=[c[0] for c in _range_cases()])
def test_zscore_is_exact_over_the_exponent_range(name, v):
    _assert_exact(v, name)


def test_zscore_of_equal_values_has_std_zero():
    for val, n in ((0.1, 1024), (4.0, 1000), (1e300, 256), (2.0 ** -1074, 4096), (-7.3, 65536)):
        z, m, s = _device(np.full(n, val))                    # n a power of two (or val a small integer): mean == val exactly
        ze, me, se = tr.zscore_exact(np.full(n, val))
        assert m == val and _same_bits(m, me) and s == 0.0 and se == 0.0 and not math.copysign(1.0, s) < 0
        assert (z == 0.0).all() and (ze == 0.0).all()


def _tie_vectors():
    """totals on a rounding tie of the sum, and a tie plus / minus a value far below it.  2^e (1 + k 2^-52) + 2^(e - 53) is
    the midpoint of two doubles; the total's top bit is bit (e + 1074) of the fixed-point number, so e + 1074 = 32 j + w - 1
    puts a top digit of w bits at digit j.  n = 4 records (a power of two: mean = sum / 4 keeps the sum's bits)."""
    for w in (1, 12, 22, 32):
        for j in (3, 34, 48):
            e = 32 * j + w - 1 - 1074
            for k in (0, 1, 2, 3):
                big = math.ldexp(1.0 + k * 2.0 ** -52, e)
                half = math.ldexp(1.0, e - 53)
                far = math.ldexp(1.0, e - 53 - 70) if e - 53 - 70 >= -1074 else 2.0 ** -1074
                pad = math.ldexp(1.0, e - 200) if e - 200 >= -1074 else 0.0
                yield (w, j, k, "tie"), [big, half, pad, -pad]
                yield (w, j, k, "tie+tiny"), [big, half, far, 0.0]
                yield (w, j, k, "tie-tiny"), [big, half, -far, 0.0]
                yield (w, j, k, "tie split over records"), [big, half / 2, half / 4, half / 4]


def test_zscore_sum_rounds_once_on_ties_and_next_to_them():
    wrong = []
    for key, vals in _tie_vectors():
        v = np.array(vals, np.float64)
        total = math.fsum(vals)
        w, j, k, kind = key
        big, half = vals[0], math.ldexp(1.0, 32 * j + w - 1 - 1074 - 53)
        up, down = big + 2 * half, big
        # the stated outcomes: a tie goes to the even neighbour, tie + tiny up, tie - tiny down
        if kind.startswith("tie+"):
            assert total == up, key
        elif kind.startswith("tie-"):
            assert total == down, key
        else:
            assert total == (down if k % 2 == 0 else up), key
        ze, me, se = tr.zscore_exact(v)
        assert me == total / 4
        z, m, s = _device(v)
        if not (_same_bits(m, me) and _same_bits(s, se) and np.array_equal(_bits(z), _bits(ze))):
            wrong.append((key, float(m).hex(), float(me).hex(), float(s).hex(), float(se).hex()))
        zp, mp, sp = _device(v[::-1].copy())
        if not (_same_bits(mp, me) and _same_bits(sp, se)):
            wrong.append((key, "reversed"))
    assert not wrong, (len(wrong), wrong[:6])


def test_zscore_of_thousands_of_short_sums():
    """the rare-event net: short vectors whose pieces straddle the 53-bit boundary at random alignments"""
    rng = np.random.default_rng(2024)
    wrong = []
    for t in range(3000):
        n = int(rng.integers(2, 9))
        e0 = int(rng.integers(-1000, 960))
        v = rng.uniform(-1.0 if t % 3 == 0 else 0.0, 1.0, n) * 2.0 ** (e0 + rng.integers(-60, 61, n))
        ze, me, se = tr.zscore_exact(v)
        z, m, s = _device(v)
        if not (_same_bits(m, me) and _same_bits(s, se) and np.array_equal(_bits(z), _bits(ze))):
            wrong.append((t, v.tolist(), float(m).hex(), float(me).hex(), float(s).hex(), float(se).hex()))
    assert not wrong, (len(wrong), wrong[:3])


@pytest.mark.parametrize("bad", [[np.nan], [np.inf], [-np.inf], [np.nan, np.inf, -np.inf], [np.inf, -np.inf]])
def test_zscore_with_non_finite_records_is_the_no_contact_case(bad, capsys):
    from mustache_amd.trans import call_trans_coo
    rng = np.random.default_rng(9)
    v = np.exp(rng.normal(0.0, 1.0, 70000))
    at = rng.choice(v.size, len(bad), replace=False)
    v[at] = bad
    ze, me, se = tr.zscore_exact(v)
    assert math.isnan(me) and math.isnan(se) and (ze == 0.0).all()
    z, m, s = _device(v)
    assert math.isnan(m) and math.isnan(s)
    assert np.array_equal(_bits(z), _bits(ze))               # NaN / inf -> +0.0, every record
    x = rng.integers(0, 300, v.size)
    y = rng.integers(0, 300, v.size)
    capsys.readouterr()
    assert call_trans_coo(x, y, v, [1.6, 3.2], 0.88, 0.2, label="1-2") == []
    assert "There is no contact in the chromosome pair 1-2 to work on." in capsys.readouterr().out
    with np.errstate(invalid="ignore"):
        assert tr.trans_loops(x, y, v, 0.88, 0.2, [1.6, 3.2]) == []


# ---- B. scatter and prologue ---------------------------------------------------------------------------------------------
def _scatter_device(x, y, v, row0, col0, C, expect_rc=0):
    """(c, nz, nz_count) of mst_trans_scatter_tiles + mst_trans_prologue called the way trans_pair_alone.pair_alone calls
    them"""
    import torch
    from mustache_amd import _lib
    from mustache_amd.engine import require_gpu
    from mustache_amd.trans import _ptr, _stream
    lib = require_gpu()
    dev = torch.device("cuda")
    B = len(row0)
    dx = torch.as_tensor(np.asarray(x, np.int32)).to(dev)
    dy = torch.as_tensor(np.asarray(y, np.int32)).to(dev)
    dv = torch.as_tensor(np.asarray(v, np.float64)).to(dev)
    r0 = torch.as_tensor(np.asarray(row0, np.int64)).to(dev)
    c0 = torch.as_tensor(np.asarray(col0, np.int64)).to(dev)
    c = torch.full((B, C, C), 9.0, dtype=torch.float64, device=dev)       # stale contents: the call clears them
    nz = torch.full((B, C, C), 7, dtype=torch.uint8, device=dev)
    nzc = torch.full((B,), 12345, dtype=torch.int32, device=dev)
    n = int(dv.numel())
    _lib.check(lib.mst_trans_scatter_tiles(_ptr(dx) if n else None, _ptr(dy) if n else None, _ptr(dv) if n else None, n, _ptr(r0),
                                           _ptr(c0), B, C, _ptr(c), _stream()))
    _lib.check(lib.mst_trans_prologue(_ptr(c), _ptr(nz), _ptr(nzc), B, C, _stream()))
    torch.cuda.synchronize()
    return c.cpu().numpy(), nz.cpu().numpy(), nzc.cpu().numpy().view(np.uint32).astype(np.int64)


def _scatter_numpy(x, y, v, row0, col0, C):
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    v = np.asarray(v, np.float64)
    c = np.zeros((len(row0), C, C))
    for b, (r, q) in enumerate(zip(row0, col0)):
        sel = (x >= r) & (x < r + C) & (y >= q) & (y < q + C)
        c[b, x[sel] - r, y[sel] - q] = v[sel]
    return c


def _check_scatter(x, y, v, row0, col0, C):
    c, nz, nzc = _scatter_device(x, y, v, row0, col0, C)
    ref = _scatter_numpy(x, y, v, row0, col0, C)
    assert np.array_equal(_bits(c), _bits(ref))               # bit for bit: a -0.0 record stays -0.0 (and is no record)
    assert np.array_equal(nz, (ref != 0).astype(np.uint8))
    assert nzc.tolist() == [int(np.count_nonzero(ref[b])) for b in range(len(row0))]
    return ref


def _map_records(n1, n2, k, rng):
    """k distinct pixels of an n1 x n2 map with signed values, some exactly zero, and the four map corners"""
    flat = rng.choice(n1 * n2, size=min(k, n1 * n2), replace=False)
    flat = np.union1d(flat, [0, n2 - 1, (n1 - 1) * n2, n1 * n2 - 1])
    x, y = flat // n2, flat % n2
    v = rng.normal(0.0, 1.0, flat.size)
    v[rng.random(flat.size) < 0.1] = 0.0
    v[rng.random(flat.size) < 0.02] = -0.0
    return x, y, v


@pytest.mark.parametrize("n1,n2,chunk", [
    (420, 300, 2000),      # one tile, C = 420 = n1, 120 padding columns
    (900, 1200, 600),      # 2 x 3 ragged
    (1000, 610, 600),      # last column start n2 - chunk = 10: an overlap of 590, far above 256
    (610, 1000, 600),      # the same on rows
    (350, 90, 2000),       # C = max(n1, n2) with the other axis much shorter
    (2300, 2100, 2000),    # the production tile: 4 tiles of 2000 x 2000
])
def test_scatter_and_prologue_match_numpy_on_the_tiling(n1, n2, chunk):
    from mustache_amd.trans import trans_tiling
    rng = np.random.default_rng(n1 * 7 + n2)
    C, (rs, re), (cs, ce) = trans_tiling(n1, n2, chunk)
    tiles = [(r, q) for r in rs for q in cs]
    x, y, v = _map_records(n1, n2, int(0.2 * n1 * n2), rng)
    # every window edge: first / last row and column of each tile, where the map has them
    ex = [(r + dr, q + dq) for r, q in tiles for dr in (0, C - 1) for dq in (0, C - 1, C // 2) if r + dr < n1 and q + dq < n2]
    ex += [(r + C // 2, q + dq) for r, q in tiles for dq in (0, C - 1) if r + C // 2 < n1 and q + dq < n2]
    ex = list(dict.fromkeys(ex))
    keep = ~np.isin(x * n2 + y, [a * n2 + b for a, b in ex])
    x = np.concatenate([x[keep], [a for a, _ in ex]])
    y = np.concatenate([y[keep], [b for _, b in ex]])
    v = np.concatenate([v[keep], np.arange(1, len(ex) + 1) * 0.5])
    perm = rng.permutation(len(v))
    x, y, v = x[perm], y[perm], v[perm]
    ref = _check_scatter(x, y, v, [t[0] for t in tiles], [t[1] for t in tiles], C)
    for b, (r, q) in enumerate(tiles):                        # padding outside the map stays zero
        assert not ref[b, max(0, n1 - r):, :].any() and not ref[b, :, max(0, n2 - q):].any()
    # the groups trans_pair_alone.pair_alone would launch with tiles_per_launch = 1 and 4
    for g in (1, 4):
        for g0 in range(0, len(tiles), g):
            grp = tiles[g0:g0 + g]
            if len(grp) < len(tiles):
                _check_scatter(x, y, v, [t[0] for t in grp], [t[1] for t in grp], C)


def test_scatter_records_outside_every_tile_and_empty_tiles():
    rng = np.random.default_rng(3)
    C = 64
    row0, col0 = [0, 500, 40, 1000], [0, 500, 30, 0]          # tile 1 receives nothing: an empty tile inside the group
    x = np.concatenate([rng.integers(0, 110, 3000), rng.integers(1000, 1064, 500), [63, 64, 499, 564, 2000000000]])
    y = np.concatenate([rng.integers(0, 100, 3000), rng.integers(0, 70, 500), [0, 0, 500, 500, 2000000000]])
    flat, first = np.unique(x * (1 << 32) + y, return_index=True)
    x, y = x[first], y[first]
    v = rng.normal(0.0, 1.0, x.size)
    v[::7] = 0.0
    ref = _check_scatter(x, y, v, row0, col0, C)
    assert not ref[1].any() and ref[0].any() and ref[2].any() and ref[3].any()
    # no record at all
    c, nz, nzc = _scatter_device([], [], [], row0, col0, C)
    assert not c.any() and not nz.any() and nzc.tolist() == [0, 0, 0, 0]
    # only zero values: scattered, and not records
    c, nz, nzc = _scatter_device([1, 2], [1, 2], [0.0, -0.0], [0], [0], C)
    assert not nz.any() and nzc.tolist() == [0]


def test_scatter_tile_count_limits():
    import torch
    from mustache_amd import _lib
    from mustache_amd.engine import require_gpu
    from mustache_amd.trans import _ptr, _stream
    rng = np.random.default_rng(4)
    C = 8
    for B in (1, 4096):
        row0 = (np.arange(B) // 64) * 5                       # windows of 8 every 5 bins: neighbours overlap by 3
        col0 = (np.arange(B) % 64) * 5
        x, y, v = _map_records(64 * 5 + 8, 64 * 5 + 8, 40000, rng)
        ref = _check_scatter(x, y, v, row0, col0, C)
        assert ref.any()
    lib = require_gpu()
    B = 4097
    dev = torch.device("cuda")
    r0 = torch.zeros(B, dtype=torch.int64, device=dev)
    c = torch.full((B, C, C), 9.0, dtype=torch.float64, device=dev)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    val = torch.ones(1, dtype=torch.float64, device=dev)
    rc = lib.mst_trans_scatter_tiles(_ptr(one), _ptr(one), _ptr(val), 1, _ptr(r0), _ptr(r0), B, C, _ptr(c), _stream())
    assert rc != 0
    assert b"mst_trans_scatter_tiles" in lib.mst_last_error() and b"4096" in lib.mst_last_error()
    with pytest.raises(Exception, match="mst_trans_scatter_tiles"):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert (c.cpu().numpy() == 9.0).all()                     # refused before the memset and the launch
    for B_bad in (0, -1):
        assert lib.mst_trans_scatter_tiles(_ptr(one), _ptr(one), _ptr(val), 1, _ptr(r0), _ptr(r0), B_bad, C, _ptr(c), _stream()) != 0
