"""The segmented inter-chromosomal pile-up on the MI355X (csrc/mst_pileup_trans_batch.hip, pileup.pileup_trans_batch): for every
pair of a batch the bytes of a batch of that pair alone, on its records filtered by v > 0 (pileup.pileup_trans_records), and the
NumPy restatement (tests/pileup_trans_reference.py) with the comparisons test_gpu_pileup_trans.py makes.  Segment isolation, the
chunk cuts of the record pass and of the reduce, ignored record values, +inf, a repeated pixel, the row bits on both sides of
the LDS switch, determinism, argument errors; the single-pair C entry point (mst_pileup_trans_windows, then mst_pileup_reduce),
which Python no longer goes through.  test_gpu_pileup_trans_digests.py holds the batch of one to the bits of the single-pair
kernels that were there before it."""
import itertools

import numpy as np
import pytest

import pileup_reference as pr
import pileup_trans_reference as ptr

pytestmark = pytest.mark.gpu

DIMS = [(5, 7), (9, 4), (60, 45), (30, 20)]                 # n1 != n2 everywhere
KEYS = ("sum_obs", "count_obs", "sum_oe", "count_oe", "apa", "apa_oe", "center_obs", "center_oe", "p2ll")


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        ok = both_nan | (a == b) | (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all())


def _same_bits(a, b):
    a, b = np.atleast_1d(np.ascontiguousarray(a, np.float64)), np.atleast_1d(np.ascontiguousarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check(r, ref, w, q):
    """the comparisons of test_gpu_pileup_trans._check"""
    obs = r["obs"].cpu().numpy()
    assert np.array_equal(np.isnan(obs), np.isnan(ref["obs"]))
    assert np.array_equal(obs, ref["obs"], equal_nan=True)
    assert r["expected"] == ref["expected"]
    rows, cols = r["valid"]
    assert np.array_equal(rows.cpu().numpy().astype(bool), ref["valid"][0])
    assert np.array_equal(cols.cpu().numpy().astype(bool), ref["valid"][1])
    oe = r["oe"].cpu().numpy()
    assert np.array_equal(np.isnan(oe), np.isnan(ref["oe"])) and _close(oe, ref["oe"])
    assert np.array_equal(r["count_obs"], ref["count_obs"]) and np.array_equal(r["count_oe"], ref["count_oe"])
    assert _close(r["sum_obs"], ref["sum_obs"]) and _close(r["sum_oe"], ref["sum_oe"])
    assert _close(r["apa"], ref["apa"]) and _close(r["apa_oe"], ref["apa_oe"])
    assert _same_bits(r["center_obs"], ref["center_obs"]) and _close(r["center_oe"], ref["center_oe"])
    assert _close(r["p2ll"], ref["p2ll"])
    for k in ref["metrics"]:
        assert _close(r["metrics"][k], ref["metrics"][k]), (k, r["metrics"][k], ref["metrics"][k])
        assert _close(r["metrics_oe"][k], ref["metrics_oe"][k]), k


def _same_pair(got, want):
    """every output of one pair, byte for byte"""
    for i in (0, 1):
        assert got["valid"][i].cpu().numpy().tobytes() == want["valid"][i].cpu().numpy().tobytes()
    assert np.float64(got["expected"]).tobytes() == np.float64(want["expected"]).tobytes()
    for k in ("obs", "oe"):
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    for k in KEYS:                                           # loop_stats and agg, and what the host derives from them
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), k


def _records(n1, n2, count, rng):
    """`count` records on an n1 x n2 map (pixels may repeat), a tenth of them with values the batch must ignore"""
    x, y = rng.integers(0, n1, count), rng.integers(0, n2, count)
    v = np.exp(rng.normal(0.0, 0.5, count))
    bad = rng.random(count) < 0.1
    v[bad] = rng.choice([0.0, -1.5, np.nan, -0.0], int(bad.sum()))
    return x.astype(np.int32), y.astype(np.int32), v


def _edge_loops(n1, n2, w, extra, rng):
    """loops within w of every edge (the four corners, (0, 0) twice), the middle, and `extra` random ones"""
    fixed = [(0, 0), (n1 - 1, n2 - 1), (0, n2 - 1), (n1 - 1, 0), (0, 0), (n1 // 2, n2 // 2)]
    xs = np.concatenate([[f[0] for f in fixed], rng.integers(0, n1, extra)]).astype(np.int64)
    ys = np.concatenate([[f[1] for f in fixed], rng.integers(0, n2, extra)]).astype(np.int64)
    return xs, ys


def _concat(recs):
    seg = np.concatenate([[0], np.cumsum([len(r[2]) for r in recs])]).astype(np.int64)
    return tuple(np.concatenate([r[k] for r in recs]) for k in range(3)) + (seg,)


def _oracle(recs, dims, loops, w, q):
    """per pair: a batch of that pair alone (pileup_trans_records) on the records filtered by v > 0"""
    from mustache_amd.pileup import pileup_trans_records
    out = []
    for (x, y, v), (n1, n2), (xs, ys) in zip(recs, dims, loops):
        keep = v > 0
        out.append(pileup_trans_records(x[keep], y[keep], v[keep], n1, n2, xs, ys, w, q))
    return out


def _reference(recs, dims, loops, w, q):
    out = []
    for (x, y, v), (n1, n2), (xs, ys) in zip(recs, dims, loops):
        keep = v > 0
        out.append(ptr.pileup_trans_records(x[keep], y[keep], v[keep], n1, n2, xs, ys, w, q))
    return out


def _batch(recs, dims, loops, w, q):
    from mustache_amd.pileup import pileup_trans_batch
    x, y, v, seg = _concat(recs)
    return pileup_trans_batch(x, y, v, seg, dims, loops, w, q)


# ---- dimensions, windows, chunking: one batch per (w, q) ----------------------------------------------------------------------
def _main_case(w):
    """the four pairs; pair 2 holds 4097 records between small ones: a chunk cut at record 4096 of the pair and the segment cut one
    record later, so its second chunk is a single record.  Each of the batch's five chunks has a workgroup of its own; a
    workgroup that goes from one pair to the next is the business of the two tests on more than 2 048 chunks below.  Every pair
    has loops within w of every edge"""
    rng = np.random.default_rng(11)
    counts = [40, 30, 4097, 700]
    recs = [_records(n1, n2, c, rng) for (n1, n2), c in zip(DIMS, counts)]
    loops = [_edge_loops(n1, n2, w, 5, rng) for n1, n2 in DIMS]
    return recs, loops


@pytest.mark.parametrize("w,q", [(0, 1), (1, 1), (1, 3), (3, 1), (3, 7)])
def test_every_pair_has_the_bytes_of_the_single_pair_entry_points(w, q):
    recs, loops = _main_case(w)
    assert sum(int((~(r[2] > 0)).sum()) for r in recs) > 300 and all(np.isnan(r[2]).any() for r in recs[2:])
    got = _batch(recs, DIMS, loops, w, q)
    want, ref = _oracle(recs, DIMS, loops, w, q), _reference(recs, DIMS, loops, w, q)
    assert [g["kept"] for g in got] == [int((r[2] > 0).sum()) for r in recs]
    for p in range(4):
        _same_pair(got[p], want[p])
        _check(got[p], ref[p], w, q)
        assert np.isnan(ref[p]["obs"][:4]).any() == (w > 0) and ref[p]["expected"] > 0


# ---- segment isolation ----------------------------------------------------------------------------------------------------------
def test_neighbours_with_the_same_dims_and_loops_but_disjoint_records():
    """pairs 0 and 1: identical dims, identical loops, records on disjoint pixels (even / odd columns); pair 2 has no record,
    pair 3 no loop, both inside the batch"""
    rng = np.random.default_rng(12)
    n1, n2, w, q = 30, 20, 1, 2
    x, y = np.divmod(rng.permutation(n1 * n2)[:300], n2)
    v = np.exp(rng.normal(0.0, 0.5, 300))
    even = y % 2 == 0
    a = (x[even].astype(np.int32), y[even].astype(np.int32), v[even])
    b = (x[~even].astype(np.int32), y[~even].astype(np.int32), v[~even])
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    lp = _edge_loops(n1, n2, w, 10, rng)
    no_loop = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    recs = [a, b, none, a, _records(9, 4, 50, rng), b]
    dims = [(n1, n2)] * 4 + [(9, 4), (n1, n2)]
    loops = [lp, lp, lp, no_loop, _edge_loops(9, 4, w, 3, rng), lp]
    got, want, ref = _batch(recs, dims, loops, w, q), _oracle(recs, dims, loops, w, q), _reference(recs, dims, loops, w, q)
    for p in range(6):
        _same_pair(got[p], want[p])
        _check(got[p], ref[p], w, q)
    # a leak across a segment would show: where a has a record b has none
    oa, ob = got[0]["obs"].cpu().numpy(), got[1]["obs"].cpu().numpy()
    assert (np.nan_to_num(oa) > 0).any() and (np.nan_to_num(ob) > 0).any() and not ((oa > 0) & (ob > 0)).any()
    assert got[2]["kept"] == 0 and got[2]["expected"] == 0.0 and not got[2]["valid"][0].any().item()
    assert not np.nan_to_num(got[2]["obs"].cpu().numpy()).any() and np.isnan(got[2]["oe"].cpu().numpy()).all()
    assert got[3]["kept"] == len(a[2]) and got[3]["expected"] == got[0]["expected"] and len(got[3]["p2ll"]) == 0
    assert not got[3]["count_obs"].any() and np.isnan(got[3]["apa"]).all()
    _same_pair(got[5], got[1])                               # the same pair again, further down the batch


def test_a_batch_of_one_and_empty_batches():
    rng = np.random.default_rng(13)
    recs, loops = [_records(60, 45, 900, rng)], [_edge_loops(60, 45, 3, 20, rng)]
    got = _batch(recs, [(60, 45)], loops, 3, 2)
    _same_pair(got[0], _oracle(recs, [(60, 45)], loops, 3, 2)[0])
    from mustache_amd.pileup import pileup_trans_batch
    e = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    r = pileup_trans_batch(None, None, None, [0, 0, 0], [(50, 40), (5, 7)], [([0, 25], [0, 20]), e], 2, 2)      # N = 0
    want = _oracle([(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))] * 2, [(50, 40), (5, 7)], [([0, 25], [0, 20]), e], 2, 2)
    for p in (0, 1):
        _same_pair(r[p], want[p])
    assert r[0]["expected"] == 0.0 and r[0]["kept"] == 0 and np.isnan(r[0]["oe"].cpu().numpy()).all()
    x, y, v, seg = _concat(recs * 2)
    r = pileup_trans_batch(x, y, v, seg, [(60, 45)] * 2, [e, e], 3, 2)                                     # L = 0
    assert r[0]["expected"] == r[1]["expected"] == got[0]["expected"] > 0 and r[1]["kept"] == got[0]["kept"]
    assert r[1]["valid"][0].cpu().numpy().tobytes() == got[0]["valid"][0].cpu().numpy().tobytes()


# ---- a workgroup that serves more than one pair ------------------------------------------------------------------------------------
# The record pass launches min(chunks, 2 048) workgroups and workgroup c takes the chunks c, c + 2 048, ...: only a batch of more
# than 2 048 chunks makes a workgroup flush one pair's limbs and counts, zero them and load the next pair's row bits.
GRID = 2048


def _sparse_pair(n1, n2, xs, ys, rng):
    """records around the loops of a pair too large to fill, a few anywhere, some values the batch must ignore"""
    near = np.repeat(np.arange(len(xs)), 30)
    x = np.clip(xs[near] + rng.integers(-3, 4, near.size), 0, n1 - 1)
    y = np.clip(ys[near] + rng.integers(-3, 4, near.size), 0, n2 - 1)
    x, y = np.concatenate([x, rng.integers(0, n1, 100)]), np.concatenate([y, rng.integers(0, n2, 100)])
    v = np.exp(rng.normal(0.0, 0.5, x.size))
    v[::13] = 0.0
    return x.astype(np.int32), y.astype(np.int32), v


def _tiny_pairs(count, rng):
    """`count` pairs of 1-3 records (one in eight with an ignored value too) and two loops each, dims from DIMS in turn; the
    loops sit on the records' rows, so row bits left over from another pair would show in the windows"""
    recs, dims, loops = [], [], []
    for p in range(count):
        n1, n2 = DIMS[p % 4]
        k = 1 + p % 3
        x, y = rng.integers(0, n1, k).astype(np.int32), rng.integers(0, n2, k).astype(np.int32)
        v = np.exp(rng.normal(0.0, 0.5, k))
        if p % 8 == 5:
            x, y, v = np.append(x, x[0]), np.append(y, y[0]), np.append(v, np.nan)
        recs.append((x, y, v))
        dims.append((n1, n2))
        loops.append((np.array([x[0], (x[0] + 2) % n1], np.int64), np.array([y[0], 0], np.int64)))
    return recs, dims, loops


BIG = (140000, 50)                                          # more rows than the LDS row bits hold: read from global memory
BIG_LOOPS = (np.array([0, 70, 131070, 131075, 139999], np.int64), np.array([0, 10, 25, 28, 49], np.int64))


def test_a_workgroup_goes_from_pair_to_pair():
    """3 150 tiny pairs, one chunk each: workgroup c serves the pairs c and c + 2 048 for c < 1 102.  Pair 500 has 140 000 rows
    (workgroup 500: row bits from global memory, then pair 2 548's in LDS), pair 2 600 as well (workgroup 552: LDS, then global)"""
    rng = np.random.default_rng(21)
    w, q = 1, 1
    recs, dims, loops = _tiny_pairs(3150, rng)
    for at in (500, 2600):
        recs[at], dims[at], loops[at] = _sparse_pair(*BIG, *BIG_LOOPS, rng), BIG, BIG_LOOPS
    assert len(recs) > GRID + 1000 and all(len(r[2]) <= 4096 for r in recs)             # one chunk per pair
    got, want = _batch(recs, dims, loops, w, q), _oracle(recs, dims, loops, w, q)
    assert [g["kept"] for g in got] == [int((r[2] > 0).sum()) for r in recs]
    for p in range(len(recs)):
        _same_pair(got[p], want[p])
    assert all(np.nansum(got[at]["obs"].cpu().numpy()) > 0 for at in (500, 2600))                # their windows hold records
    ref = _reference(recs[498:502] + recs[2546:2550], dims[498:502] + dims[2546:2550], loops[498:502] + loops[2546:2550], w, q)
    for p, r in zip(list(range(498, 502)) + list(range(2546, 2550)), ref):
        _check(got[p], r, w, q)


def test_a_pair_of_many_chunks_and_then_other_pairs():
    """pair 0 has 2 060 chunks: workgroup c strides over its chunks c and, for c < 12, c + 2 048 without a flush between them.
    Chunk 2 060 is pair 1 with 140 000 rows (row bits from global memory), then 2 100 tiny pairs: workgroup 12 goes pair 0 (LDS) ->
    pair 1 (global) -> pair 2 049 (LDS), the workgroups beside it pair 0 -> a tiny pair -> a tiny pair"""
    rng = np.random.default_rng(22)
    w, q = 1, 2
    n = 2060 * 4096 - 5                                      # the last chunk of pair 0 is short
    x, y = rng.integers(0, 60, n).astype(np.int32), rng.integers(0, 45, n).astype(np.int32)
    v = np.exp(rng.normal(0.0, 0.5, n))
    v[rng.random(n) < 0.1] = 0.0
    v[5::1001] = np.nan
    tiny = _tiny_pairs(2100, rng)
    recs = [(x, y, v), _sparse_pair(*BIG, *BIG_LOOPS, rng)] + tiny[0]
    dims = [(60, 45), BIG] + tiny[1]
    loops = [_edge_loops(60, 45, w, 20, rng), BIG_LOOPS] + tiny[2]
    assert 2060 + 1 + 2100 > 2 * GRID + 12
    got, want = _batch(recs, dims, loops, w, q), _oracle(recs, dims, loops, w, q)
    assert [g["kept"] for g in got] == [int((r[2] > 0).sum()) for r in recs]
    for p in range(len(recs)):
        _same_pair(got[p], want[p])
    assert got[0]["expected"] > 1000 and np.nansum(got[1]["obs"].cpu().numpy()) > 0
    for p, r in zip((1, 2, 2049), _reference([recs[p] for p in (1, 2, 2049)], [dims[p] for p in (1, 2, 2049)],
                                             [loops[p] for p in (1, 2, 2049)], w, q)):
        _check(got[p], r, w, q)


# ---- the reduce's chunk edge --------------------------------------------------------------------------------------------------
def test_the_reduces_chunk_edge_inside_a_batch():
    """pairs with 511, 512 and 513 loops beside a pair with one loop: a pair's chunks never mix with a neighbour's"""
    rng = np.random.default_rng(14)
    w, q = 1, 1
    counts = [511, 1, 512, 513, 1]
    dims = [(60, 45), (5, 7), (30, 20), (60, 45), (9, 4)]
    recs = [_records(n1, n2, 600, rng) for n1, n2 in dims]
    loops = [(rng.integers(0, n1, c).astype(np.int64), rng.integers(0, n2, c).astype(np.int64)) for (n1, n2), c in zip(dims, counts)]
    got, want, ref = _batch(recs, dims, loops, w, q), _oracle(recs, dims, loops, w, q), _reference(recs, dims, loops, w, q)
    for p in range(5):
        _same_pair(got[p], want[p])
        _check(got[p], ref[p], w, q)


def test_reduce_segmented_alone_skips_foreign_indices_and_zeroes_empty_pairs():
    import torch
    from mustache_amd import _lib
    from mustache_amd.pileup import _host_ptr, reduce
    lib = _lib.require_gpu()
    rng = np.random.default_rng(15)
    w, S, counts = 1, 3, [3, 0, 600]
    L = sum(counts)
    loop_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    obs = rng.normal(size=(L, S, S))
    obs[rng.random(obs.shape) < 0.2] = np.nan
    oe = obs / 3.0
    order = np.concatenate([rng.permutation(c) + o for c, o in zip(counts, loop_off)]).astype(np.int32)
    order[1] = 5                                             # a loop of pair 2 in pair 0's range: skipped, as an index >= L is
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    obs_d, oe_d, order_d = d(obs), d(oe), d(order)
    ws = torch.empty(int(lib.mst_pileup_reduce_segmented_workspace_bytes(_host_ptr(loop_off), 3, w)), dtype=torch.uint8, device="cuda")
    agg = torch.full((3, 4, S * S), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.mst_pileup_reduce_segmented(_lib.ptr(obs_d), _lib.ptr(oe_d), _lib.ptr(order_d), L, _host_ptr(loop_off), 3, w,
                                               _lib.ptr(agg), _lib.ptr(ws), ws.numel(), None))
    agg = agg.cpu().numpy()
    assert not agg[1].any()
    for p in (0, 2):
        s, e = int(loop_off[p]), int(loop_off[p + 1])
        local = torch.from_numpy((order[s:e] - s).astype(np.int32)).cuda()     # pair 0: the foreign index becomes 5 >= L = 3
        ws1 = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        one = reduce(obs_d[s:e].contiguous(), oe_d[s:e].contiguous(), local, w, ws1).cpu().numpy()
        assert agg[p].tobytes() == one.tobytes(), p
    assert agg[0][1].max() <= 2.0                            # at most two of pair 0's three loops were added


@pytest.mark.parametrize("w,counts", pr.REDUCE_SEGMENTED)
def test_reduce_segmented_has_the_bytes_of_the_ordered_restatement(w, counts):
    """mst_pileup_reduce_segmented against pr.ordered_aggregate, byte for byte: values on which another order of
    additions shows, independent NaN masks, a foreign index in pair 0's range, a pair without a loop."""
    import torch
    from mustache_amd import _lib
    from mustache_amd.pileup import _host_ptr
    lib = _lib.require_gpu()
    a, b, order, loop_off = pr.reduce_case(w, counts)
    L, P, S = len(order), len(counts), 2 * w + 1
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    ad, bd, od = d(a), d(b), d(order)
    ws = torch.empty(int(lib.mst_pileup_reduce_segmented_workspace_bytes(_host_ptr(loop_off), P, w)), dtype=torch.uint8, device="cuda")
    agg = torch.full((P, 4, S * S), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.mst_pileup_reduce_segmented(_lib.ptr(ad), _lib.ptr(bd), _lib.ptr(od), L, _host_ptr(loop_off), P, w,
                                               _lib.ptr(agg), _lib.ptr(ws), ws.numel(), None))
    assert agg.cpu().numpy().tobytes() == pr.ordered_aggregate((a, b), order, loop_off).tobytes()


# ---- record values ---------------------------------------------------------------------------------------------------------------
def test_an_infinite_value_spoils_its_own_pair_only():
    w, q = 1, 2
    recs, loops = _main_case(w)
    clean = _batch(recs, DIMS, loops, w, q)
    x, y, v = (a.copy() for a in recs[1])
    v[np.flatnonzero(v > 0)[3]] = np.inf
    spoiled = recs[:1] + [(x, y, v)] + recs[2:]
    got, want = _batch(spoiled, DIMS, loops, w, q), _oracle(spoiled, DIMS, loops, w, q)
    assert np.isnan(got[1]["expected"]) and np.isnan(got[1]["oe"].cpu().numpy()).all() and got[1]["kept"] == clean[1]["kept"]
    for p in range(4):
        _same_pair(got[p], want[p])
        if p != 1:
            _same_pair(got[p], clean[p])


def test_a_repeated_pixel_takes_its_largest_value_in_every_order():
    base = (np.array([2, 9, 9]), np.array([3, 3, 11]), np.array([0.5, 1.5, 2.5]))
    other = (np.array([5, 5], np.int32), np.array([7, 7], np.int32), np.array([100.0, 200.0]))     # the same pixel next door
    for vals in itertools.permutations([0.75, 6.0, 3.25]):
        x = np.concatenate([base[0], [5, 5, 5, 5]]).astype(np.int32)
        y = np.concatenate([base[1], [7, 7, 7, 7]]).astype(np.int32)
        v = np.concatenate([base[2], vals, [-9.0]])
        r = _batch([other, (x, y, v), other], [(10, 12)] * 3, [([5, 4], [7, 6])] * 3, 1, 1)
        obs = r[1]["obs"].cpu().numpy()
        assert obs[0, 1, 1] == 6.0 and obs[1, 2, 2] == 6.0
        assert r[1]["expected"] == (0.5 + 1.5 + 2.5 + 10.0) / 9.0 and r[1]["kept"] == 6
        assert r[0]["obs"].cpu().numpy()[0, 1, 1] == 200.0 and r[2]["expected"] == 300.0


# ---- the row bits on both sides of the LDS switch -------------------------------------------------------------------------------
def test_row_flags_on_both_sides_of_the_lds_switch_point():
    """kLdsFlagWords = 4096 words = 131 072 rows: a pair of 131 072 rows keeps its row bits in LDS, one of 140 000 reads them
    from global memory, a small one follows; sparse records around the loops, as test_row_flags_beyond_the_lds_switch_point"""
    rng = np.random.default_rng(9)
    w, q = 2, 2

    def sparse(n1, n2, xs, ys):
        near = np.repeat(np.arange(len(xs)), 40)
        x = np.clip(xs[near] + rng.integers(-4, 5, near.size), 0, n1 - 1)
        y = np.clip(ys[near] + rng.integers(-4, 5, near.size), 0, n2 - 1)
        x = np.concatenate([x, rng.integers(0, n1, 300), [n1 - 1]])
        y = np.concatenate([y, rng.integers(0, n2, 300), [n2 - 1]])
        v = np.exp(rng.normal(0.0, 0.5, x.size))
        v[::17] = 0.0
        return x.astype(np.int32), y.astype(np.int32), v
    dims = [(131072, 50), (140000, 50), (30, 20)]
    loops = [(np.array([0, 70, 131070, 131071, 65536], np.int64), np.array([0, 10, 25, 49, 20], np.int64)),
             (np.array([0, 70, 131070, 131075, 139999, 139999, 65536], np.int64), np.array([0, 10, 25, 28, 49, 0, 20], np.int64)),
             _edge_loops(30, 20, w, 4, rng)]
    recs = [sparse(*dims[0], *loops[0]), sparse(*dims[1], *loops[1]), _records(30, 20, 200, rng)]
    got, want, ref = _batch(recs, dims, loops, w, q), _oracle(recs, dims, loops, w, q), _reference(recs, dims, loops, w, q)
    for p in range(3):
        assert p == 2 or np.nansum(ref[p]["obs"], (1, 2)).all()          # every window of the large pairs holds records
        _same_pair(got[p], want[p])
        _check(got[p], ref[p], w, q)


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_bit_identical_under_permutation_and_from_run_to_run():
    w, q = 3, 2
    recs, loops = _main_case(w)
    rng = np.random.default_rng(5)
    loops = [(np.concatenate([xs, rng.integers(0, n1, 300)]), np.concatenate([ys, rng.integers(0, n2, 300)]))
             for (xs, ys), (n1, n2) in zip(loops, DIMS)]
    loops[2] = (np.concatenate([loops[2][0], rng.integers(0, 60, 300)]), np.concatenate([loops[2][1], rng.integers(0, 45, 300)]))
    assert len(loops[2][0]) > 512                            # two chunks of the reduce
    a, b = _batch(recs, DIMS, loops, w, q), _batch(recs, DIMS, loops, w, q)
    pr_ = [rng.permutation(len(r[2])) for r in recs]
    pl_ = [rng.permutation(len(lp[0])) for lp in loops]
    c = _batch([tuple(t[o] for t in r) for r, o in zip(recs, pr_)], DIMS, [(xs[o], ys[o]) for (xs, ys), o in zip(loops, pl_)], w, q)
    for p in range(4):
        _same_pair(a[p], b[p])
        o = pl_[p]
        for k in ("sum_obs", "count_obs", "sum_oe", "count_oe", "apa", "apa_oe"):
            assert _same_bits(a[p][k], c[p][k]), k
        for k in ("center_obs", "center_oe", "p2ll"):
            assert _same_bits(a[p][k][o], c[p][k]), k
        for k in ("obs", "oe"):
            assert _same_bits(a[p][k].cpu().numpy()[o], c[p][k].cpu().numpy()), k
        assert a[p]["expected"] == c[p]["expected"] and a[p]["kept"] == c[p]["kept"]
        for i in (0, 1):
            assert np.array_equal(a[p]["valid"][i].cpu().numpy(), c[p]["valid"][i].cpu().numpy())


# ---- the single-pair C entry point ---------------------------------------------------------------------------------------------------
def _c_single(x, y, v, n1, n2, xs, ys, w, q, short=0):
    """lib.mst_pileup_trans_windows, then lib.mst_pileup_reduce on the same workspace (`short` bytes less than the size query
    reports) -> (return code of the first, {name: bytes of an output}); the outputs start out as 0xA5 bytes"""
    import torch
    from mustache_amd import _lib
    lib = _lib.require_gpu()
    N, L, S = len(v), len(xs), 2 * w + 1
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda() if len(a) else None
    xd, yd, vd, lx, ly = d(x, np.int32), d(y, np.int32), d(v, np.float64), d(xs, np.int64), d(ys, np.int64)
    order = d(np.lexsort((ys, xs)), np.int32)
    fill = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
    out = {"rows": fill(n1), "cols": fill(n2), "expected": fill(8), "agg": fill(4 * S * S * 8)}
    if L:
        out.update(obs=fill(L * S * S * 8), oe=fill(L * S * S * 8), stats=fill(L * 3 * 8))
    need = int(lib.mst_pileup_trans_workspace_bytes(n1, n2, L, w))
    assert need > 0
    ws = torch.empty(need - short, dtype=torch.uint8, device="cuda")
    rc = lib.mst_pileup_trans_windows(_lib.ptr(xd), _lib.ptr(yd), _lib.ptr(vd), N, n1, n2, _lib.ptr(lx), _lib.ptr(ly), L, w, q,
                                      _lib.ptr(out["rows"]), _lib.ptr(out["cols"]), _lib.ptr(out["expected"]), _lib.ptr(out.get("obs")),
                                      _lib.ptr(out.get("oe")), _lib.ptr(out.get("stats")), _lib.ptr(ws), ws.numel(), None)
    if rc == _lib.MST_OK:
        _lib.check(lib.mst_pileup_reduce(_lib.ptr(out.get("obs")), _lib.ptr(out.get("oe")), _lib.ptr(order), L, w, _lib.ptr(out["agg"]),
                                         _lib.ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    return rc, {k: t.cpu().numpy().tobytes() for k, t in out.items()}


def _batch_bytes(r):
    """the outputs of _c_single from a dict of pileup_trans_batch"""
    out = {"rows": r["valid"][0].cpu().numpy().tobytes(), "cols": r["valid"][1].cpu().numpy().tobytes(),
           "expected": np.float64(r["expected"]).tobytes(),
           "agg": np.stack([r[k] for k in ("sum_obs", "count_obs", "sum_oe", "count_oe")]).tobytes()}
    if len(r["p2ll"]):
        out.update(obs=r["obs"].cpu().numpy().tobytes(), oe=r["oe"].cpu().numpy().tobytes(),
                   stats=np.stack([r["center_obs"], r["center_oe"], r["p2ll"]], axis=1).tobytes())
    return out


def test_the_single_pair_c_entry_point_is_a_batch_of_one():
    from mustache_amd import _lib
    rng = np.random.default_rng(13)
    n1, n2, w, q = 60, 45, 3, 2
    x, y, v = _records(n1, n2, 900, rng)                      # a tenth of the values are 0.0, -1.5, NaN, -0.0
    xs, ys = _edge_loops(n1, n2, w, 20, rng)
    keep = v > 0
    assert 40 < int((~keep).sum()) < 200 and np.isnan(v).any() and (v < 0).any()
    clean = (x[keep], y[keep], v[keep])
    none, no_loop = (x[:0], y[:0], v[:0]), (xs[:0], ys[:0])
    for recs, loops in ((clean, (xs, ys)), (none, (xs, ys)), (clean, no_loop)):          # the pair, N = 0, L = 0
        rc, got = _c_single(*recs, n1, n2, *loops, w, q)
        want = _batch_bytes(_batch([recs], [(n1, n2)], [loops], w, q)[0])
        assert rc == _lib.MST_OK and sorted(got) == sorted(want)
        for k in want:
            assert got[k] == want[k], k
    rc, dirty = _c_single(x, y, v, n1, n2, xs, ys, w, q)     # ignored values: the result on the records filtered by v > 0
    assert rc == _lib.MST_OK and dirty == _c_single(*clean, n1, n2, xs, ys, w, q)[1]
    rc, untouched = _c_single(*clean, n1, n2, xs, ys, w, q, short=1)                     # a workspace one byte short
    assert rc == _lib.MST_E_ARG and "workspace" in _lib.require_gpu().mst_last_error().decode()
    assert all(set(b) == {0xA5} for b in untouched.values())                            # nothing was launched


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_with_a_message_and_launch_nothing():
    import torch
    from mustache_amd import _lib
    from mustache_amd.pileup import PileupError, _host_ptr, pileup_trans_batch
    lib = _lib.require_gpu()
    rng = np.random.default_rng(17)
    x, y, v = _records(5, 7, 20, rng)
    with pytest.raises(PileupError, match="64"):
        pileup_trans_batch(x, y, v, [0, 20], [(5, 7)], [([1], [1])], w=65)
    with pytest.raises(_lib.MstError, match="P = 0 pairs is outside 1 .. 65535"):
        pileup_trans_batch(None, None, None, [0], [], [], 1, 1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, yd, vd = d(x), d(y), d(v)
    rows, cols = torch.full((5,), 9, dtype=torch.uint8, device="cuda"), torch.full((7,), 9, dtype=torch.uint8, device="cuda")
    E, kept = torch.full((1,), -7.0, dtype=torch.float64, device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    seg, n1, n2, loop_off = (np.array(a, np.int64) for a in ([0, 20], [5], [7], [0, 0]))
    big = np.zeros(65537, np.int64)

    def call(P, w, q, seg=seg, loop_off=loop_off):
        return lib.mst_pileup_trans_batch(_lib.ptr(xd), _lib.ptr(yd), _lib.ptr(vd), 20, _host_ptr(seg), _host_ptr(n1), _host_ptr(n2),
                                          None, None, 0, _host_ptr(loop_off), P, w, q, _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(E),
                                          _lib.ptr(kept), None, None, None, _lib.ptr(ws), ws.numel(), None)
    for args, text in (((1, 65, 1), "w = 65"), ((0, 1, 1), "P = 0"), ((65536, 1, 1, big, big), "P = 65536"),
                       ((1, 1, 4), "q = 4"), ((1, 1, 1, np.array([0, 19], np.int64)), "rise from 0 to N = 20")):
        assert call(*args) == _lib.MST_E_ARG
        assert text in lib.mst_last_error().decode(), text
    assert lib.mst_pileup_reduce_segmented(None, None, None, 0, _host_ptr(loop_off), 0, 1, _lib.ptr(E), _lib.ptr(ws), ws.numel(),
                                           None) == _lib.MST_E_ARG
    assert "P = 0" in lib.mst_last_error().decode()
    assert lib.mst_pileup_trans_batch_workspace_bytes(_host_ptr(seg), _host_ptr(n1), _host_ptr(loop_off), 0, 1) == 0
    assert lib.mst_pileup_reduce_segmented_workspace_bytes(_host_ptr(loop_off), 65536, 1) == 0
    torch.cuda.synchronize()
    assert bool((rows == 9).all()) and bool((cols == 9).all()) and E.item() == -7.0 and kept.item() == -7      # nothing ran
    assert call(1, 1, 1) == _lib.MST_OK
    torch.cuda.synchronize()
    assert kept.item() == int((v > 0).sum()) and E.item() > 0
