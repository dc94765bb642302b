"""The kernels of csrc/mst_trans_genome.hip one by one on the MI355X, each against NumPy: the segmented z-score (per segment
bit for bit mst_trans_zscore of the segment alone), the tile counts and the work-list scatter of a batch of pairs."""
import numpy as np
import pytest

import trans_reference as tr

pytestmark = pytest.mark.gpu

GEOMETRIES = [(900, 1200, 600), (300, 500, 300), (605, 300, 300), (2300, 2100, 2000), (420, 300, 2000)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _segmented(xs, ys, vs):
    """(out, stats [P, 4], extent [P, 2]) of mst_trans_zscore_segmented over the concatenated segments"""
    import torch
    from mustache_amd import _lib
    from mustache_amd.engine import require_gpu
    from mustache_amd.trans import _ptr, _stream
    lib = require_gpu()
    dev = torch.device("cuda")
    P = len(vs)
    seg = np.zeros(P + 1, np.int64)
    np.cumsum([len(v) for v in vs], out=seg[1:])
    x = torch.as_tensor(np.concatenate(xs).astype(np.int32)).to(dev)
    y = torch.as_tensor(np.concatenate(ys).astype(np.int32)).to(dev)
    v = torch.as_tensor(np.concatenate(vs).astype(np.float64)).to(dev)
    out = torch.full_like(v, 7.0)
    stats = torch.full((4 * P,), 5.0, dtype=torch.float64, device=dev)
    extent = torch.full((2 * P,), 9, dtype=torch.int32, device=dev)
    nb = int(lib.mst_trans_zscore_segmented_workspace_bytes(P))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    seg_d = torch.as_tensor(seg).to(dev)
    _lib.check(lib.mst_trans_zscore_segmented(_ptr(x), _ptr(y), _ptr(v), int(seg[-1]), _ptr(seg_d), P, _ptr(out), _ptr(stats),
                                              _ptr(extent), _ptr(ws), nb, _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy().reshape(P, 4), extent.cpu().numpy().reshape(P, 2), seg


# ---- 1. the segmented z-score ---------------------------------------------------------------------------------------------
def test_segmented_zscore_equals_the_single_pair_zscore_per_segment():
    from mustache_amd.trans import zscore_device
    rng = np.random.default_rng(11)
    sizes = [1, 10, 70001, 0, 3, 200003]                       # an empty segment in the middle
    vs = [np.exp(rng.normal(0.0, 1.5, n)) * 10.0 for n in sizes]
    vs[1] = np.full(10, 4.0)                                   # all equal: std 0
    xs = [rng.integers(0, 5000, n) for n in sizes]
    ys = [rng.integers(0, 3000, n) for n in sizes]
    out, stats, extent, seg = _segmented(xs, ys, vs)
    alone = {}
    for p, v in enumerate(vs):
        o = out[seg[p]:seg[p + 1]]
        if len(v) == 0:
            assert stats[p].tolist() == [0.0, 0.0, 0.0, 0.0] and extent[p].tolist() == [-1, -1]
            continue
        z, mean, std, n = zscore_device(v)
        alone[p] = (z.cpu().numpy(), mean, std)
        assert np.array_equal(_bits(o), _bits(alone[p][0])), p
        assert _bits([stats[p, 0]])[0] == _bits([mean])[0] and _bits([stats[p, 1]])[0] == _bits([std])[0], p
        assert stats[p, 2] == len(v) and stats[p, 3] == 0.0
        assert extent[p].tolist() == [int(xs[p].max()), int(ys[p].max())], p
    assert stats[1, 1] == 0.0 and not out[seg[1]:seg[2]].any()
    # bit-identical under a permutation of the records within each segment
    perms = [rng.permutation(n) for n in sizes]
    out2, stats2, extent2, _ = _segmented([a[q] for a, q in zip(xs, perms)], [a[q] for a, q in zip(ys, perms)],
                                          [a[q] for a, q in zip(vs, perms)])
    assert np.array_equal(_bits(stats2), _bits(stats)) and np.array_equal(extent2, extent)
    for p in alone:
        assert np.array_equal(_bits(out2[seg[p]:seg[p + 1]]), _bits(alone[p][0][perms[p]])), p
    # a NaN record: NaN mean / std and all-zero out for that segment only
    vs3 = [v.copy() for v in vs]
    vs3[2][12345] = np.nan
    out3, stats3, extent3, _ = _segmented(xs, ys, vs3)
    assert np.isnan(stats3[2, 0]) and np.isnan(stats3[2, 1]) and stats3[2, 3] == 1.0
    assert not out3[seg[2]:seg[3]].any() and np.array_equal(_bits(out3[seg[2]:seg[3]]), np.zeros(sizes[2], np.uint64))
    for p in alone:
        if p != 2:
            assert np.array_equal(_bits(out3[seg[p]:seg[p + 1]]), _bits(alone[p][0])), p
            assert np.array_equal(_bits(stats3[p]), _bits(stats[p])), p
    assert np.array_equal(extent3, extent)


# ---- 2, 3. one batch of five pairs ------------------------------------------------------------------------------------------
def _map_records(n1, n2, rng, density=0.2):
    """distinct pixels of an n1 x n2 map with the map's last pixel among them, signed values, a tenth exactly zero"""
    flat = rng.choice(n1 * n2, size=int(density * n1 * n2), replace=False)
    flat = np.union1d(flat, [0, n1 * n2 - 1])
    v = rng.normal(0.0, 1.0, flat.size)
    v[rng.random(flat.size) < 0.1] = 0.0
    v[-1] = 1.5                                                # the extent's pixel is a record
    perm = rng.permutation(flat.size)
    return (flat // n2)[perm], (flat % n2)[perm], v[perm]


@pytest.fixture(scope="module")
def batch():
    """the five geometries as one batch on the device: records, the pair table, and per tile its (pair, row start, col start)"""
    import torch
    from mustache_amd.trans_genome import pair_table
    rng = np.random.default_rng(5)
    recs = [_map_records(n1, n2, rng, 0.05 if chunk == 2000 and n1 > 2000 else 0.2) for n1, n2, chunk in GEOMETRIES]
    # one table per chunk value would be the caller's; the kernels take any table, so the pairs keep their own C here
    table = np.concatenate([pair_table([(n1, n2)], chunk)[0] for n1, n2, chunk in GEOMETRIES])
    tiles = []
    base = 0
    for p, (n1, n2, chunk) in enumerate(GEOMETRIES):
        C, (rs, _), (cs, _) = tr.tiling(n1, n2, chunk)
        assert (C, len(rs), len(cs)) == (int(table[p]["C"]), int(table[p]["K1"]), int(table[p]["K2"]))
        table[p]["tile_base"] = base
        tiles += [(p, C, r, q) for r in rs for q in cs]
        base += len(rs) * len(cs)
    seg = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r[2]) for r in recs], out=seg[1:])
    dev = torch.device("cuda")
    d = dict(recs=recs, table=table, tiles=tiles, T=base, seg=seg, P=len(recs),
             x=torch.as_tensor(np.concatenate([r[0] for r in recs]).astype(np.int32)).to(dev),
             y=torch.as_tensor(np.concatenate([r[1] for r in recs]).astype(np.int32)).to(dev),
             v=torch.as_tensor(np.concatenate([r[2] for r in recs])).to(dev),
             seg_d=torch.as_tensor(seg).to(dev), table_d=torch.from_numpy(table.view(np.uint8)).to(dev))
    return d


def _window(batch, t):
    p, C, r, q = batch["tiles"][t]
    x, y, v = batch["recs"][p]
    return p, C, r, q, (x >= r) & (x < r + C) & (y >= q) & (y < q + C)


def test_tile_counts_match_boolean_masks(batch):
    import torch
    from mustache_amd import _lib
    from mustache_amd.engine import require_gpu
    from mustache_amd.trans import _ptr, _stream
    lib = require_gpu()
    T = batch["T"]
    assert T == 6 + 6 + 8 + 4 + 1                             # (605, 300, 300): eight row windows 44 bins apart
    counts = torch.full((T,), 77, dtype=torch.int32, device="cuda")
    _lib.check(lib.mst_trans_count_tiles(_ptr(batch["x"]), _ptr(batch["y"]), _ptr(batch["v"]), int(batch["seg"][-1]),
                                         _ptr(batch["seg_d"]), _ptr(batch["table_d"]), batch["P"], T, _ptr(counts), _stream()))
    torch.cuda.synchronize()
    got = counts.cpu().numpy().view(np.uint32).astype(np.int64)
    ref, with_zeros = [], []
    for t in range(T):
        p, C, r, q, sel = _window(batch, t)
        ref.append(int(np.count_nonzero(batch["recs"][p][2][sel])))
        with_zeros.append(int(sel.sum()))
    assert got.tolist() == ref
    assert all(a < b for a, b in zip(ref, with_zeros))         # every window holds records that are exactly 0.0: not counted


def test_worklist_scatter_matches_numpy_and_the_per_pair_scatter(batch):
    import torch
    from mustache_amd import _lib
    from mustache_amd.engine import require_gpu
    from mustache_amd.trans import _ptr, _stream
    lib = require_gpu()
    T, table = batch["T"], batch["table"]
    dev = torch.device("cuda")
    for C in sorted(set(int(c) for c in table["C"])):
        of_c = [t for t in range(T) if batch["tiles"][t][1] == C]
        chosen = of_c[::2]                                     # every second tile of this C
        B = len(chosen)
        slot = np.full(T, -1, np.int32)
        slot[chosen] = np.arange(B)
        p0, p1 = batch["tiles"][chosen[0]][0], batch["tiles"][chosen[-1]][0]
        guard = 2
        buf = torch.full((B + 2 * guard, C, C), 9.0, dtype=torch.float64, device=dev)
        c = buf[guard:guard + B]
        slot_d = torch.as_tensor(slot).to(dev)
        _lib.check(lib.mst_trans_scatter_worklist(_ptr(batch["x"]), _ptr(batch["y"]), _ptr(batch["v"]), _ptr(batch["seg_d"]),
                                                  _ptr(batch["table_d"]), p0, p1 + 1, int(batch["seg"][p1 + 1] - batch["seg"][p0]),
                                                  T, _ptr(slot_d), B, C, _ptr(c), _stream()))
        torch.cuda.synchronize()
        whole = buf.cpu().numpy()
        assert (whole[:guard] == 9.0).all() and (whole[guard + B:] == 9.0).all()       # nothing outside the B tiles
        got = whole[guard:guard + B]
        for b, t in enumerate(chosen):
            p, _, r, q, sel = _window(batch, t)
            x, y, v = batch["recs"][p]
            ref = np.zeros((C, C))
            ref[x[sel] - r, y[sel] - q] = v[sel]
            assert np.array_equal(_bits(got[b]), _bits(ref)), (C, t)
            # what mst_trans_scatter_tiles writes for the same tile from the pair's records alone
            one = torch.full((1, C, C), 9.0, dtype=torch.float64, device=dev)
            s0, s1 = int(batch["seg"][p]), int(batch["seg"][p + 1])
            r0 = torch.tensor([r], dtype=torch.int64, device=dev)
            c0 = torch.tensor([q], dtype=torch.int64, device=dev)
            _lib.check(lib.mst_trans_scatter_tiles(_ptr(batch["x"][s0:s1]), _ptr(batch["y"][s0:s1]), _ptr(batch["v"][s0:s1]),
                                                   s1 - s0, _ptr(r0), _ptr(c0), 1, C, _ptr(one), _stream()))
            torch.cuda.synchronize()
            assert np.array_equal(_bits(one.cpu().numpy()[0]), _bits(got[b])), (C, t)
