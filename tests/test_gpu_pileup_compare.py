"""One loop list piled up on two maps on the MI355X (mst_pileup_compare, csrc/mst_pileup_compare.hip; mst_pileup_reduce_pair,
csrc/mst_pileup_reduce.hip;
and pileup_band_pair / pileup_trans_records_pair / `-f2` of mustache_amd/pileup.py) against the cell-by-cell restatement
(tests/pileup_compare_reference.py): cis at every window size the lanes walk differently and every L at which the loops fill
workgroups and chunks differently, the exact identities, trans pairs, and the command line end to end.

Bounds.  u = 2^-53, S = 2w + 1.  S_1 and S_2 are sums of at most S^2 non-negative terms: in any order each is within S^2 u of
the exact sum, relatively, so two orders differ by at most 2 S^2 u; 4 S^2 u is the enrichment test's bound for them, kept here.
R = c / (S_s / cnt) adds two roundings to one sum: within (2 S^2 + 2) u, inside the same 4 S^2 u.  LFC_N = log2(R_1 / R_2)
carries two R and the division, (4 S^2 + 5) u relatively in the ratio, which log2 turns into an absolute error of that times
1 / ln 2 < 1.45 -- below 8 S^2 u for every S >= 3 -- plus log2's own rounding, 2^-52 |LFC_N|.  LFC is a discontinuous function
of the four LFC_N (its value jumps between min, 0 and max where one of them changes sign), so it is checked on the device's own
LFC_N, to the bit.  T_1 and T_2 are sums of at most L non-negative terms in two orders: 2 L u relatively.  Counts and NaN
positions are exact: oe = obs / E is one IEEE division on the device and in the restatement, from the same obs and the same E.

The inputs (checked on the host with the restatement alone): of the 1000 loops 189 / 438 / 403 / 380 have a defined LFC at
(w, p) = (1, 0), (10, 2), (32, 5), (64, 63), at least 51 of them positive, 51 negative and 51 exactly 0 each time, and in every
case the shared cells are fewer than either map's own."""
import functools
import os

import numpy as np
import pytest

import pileup_compare_reference as cr
import pileup_enrich_reference as er
import pileup_reference as pr
import pileup_trans_reference as ptr

pytestmark = pytest.mark.gpu

N, SEP_MAX = 300, 60
RECIPE = {1: (100, 20, range(150, 156)), 2: (200, 33, range(90, 94))}    # sample: seed base, zeroed diagonal, invalid bins
CASES = [(1, 0), (10, 2), (32, 5), (64, 63)]
U = 2.0 ** -53


def _bound(w):
    return 4.0 * (2 * w + 1) ** 2 * U


def _within(a, b, rel, abs_=None):
    """the same NaN positions, and the rest within the relative bound (or the absolute one, an array or a number)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    err = np.abs(a[ok] - b[ok])
    lim = rel * np.maximum(np.abs(a[ok]), np.abs(b[ok])) if abs_ is None else np.broadcast_to(abs_, a.shape)[ok]
    assert (err <= lim).all(), float(err.max())


def _lfc_bound(w, lfc, extra=0.0):
    return 8.0 * (2 * w + 1) ** 2 * U + 2.0 ** -52 * np.abs(np.nan_to_num(np.asarray(lfc, np.float64), posinf=0.0, neginf=0.0)) + extra


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _band(w, sample):
    """(a raw band [D + 2, N] built with torch, D): values >= 0, a third of them zero, nothing beyond the chromosome's end, one
    diagonal zeroed whole (E = 0 there) and every pixel that touches an invalid bin removed; the two samples differ in all three"""
    import torch
    seed, zero_diagonal, bad_bins = RECIPE[sample]
    D = SEP_MAX + 2 * w
    g = torch.Generator().manual_seed(seed + w)
    B = torch.floor(torch.rand((D + 2, N), generator=g, dtype=torch.float64) * 3.0) \
        * (0.5 + torch.rand((D + 2, N), generator=g, dtype=torch.float64))
    for d in range(D + 2):
        B[d, N - d:] = 0.0
    B[zero_diagonal] = 0.0
    for m in bad_bins:
        B[:, m] = 0.0
        for d in range(min(D + 2, m + 1)):
            B[d, m - d] = 0.0
    return B.contiguous(), D


def _loops():
    """1000 loops, y - x <= SEP_MAX.  The first ones are placed: at bin 0 and at bin N - 1 (cells off the chromosome), y - x < 2w
    (mirrored cells, d = 0), on sample 1's zeroed diagonal, among its invalid bins."""
    rng = np.random.default_rng(11)
    placed = [(0, 40), (N - 36, N - 1), (N - 1, N - 1), (0, 0), (100, 101), (60, 60 + 20), (152, 190), (140, 153),
              (2, 58), (N - 2, N - 1)]
    sep = rng.integers(0, SEP_MAX + 1, 1000 - len(placed))
    x = rng.integers(0, N - sep)
    xs = np.concatenate([[a for a, _ in placed], x]).astype(np.int64)
    ys = np.concatenate([[b for _, b in placed], x + sep]).astype(np.int64)
    return xs, ys


def _run(w, p, xs, ys):
    """pileup_band_pair on the two bands: (dict 1, dict 2, compare dict, (E_1, E_2) on the host)"""
    from mustache_amd.pileup import pileup_band_pair
    (B1, D), (B2, _) = _band(w, 1), _band(w, 2)
    r1, r2, c = pileup_band_pair(B1.cuda(), N, B2.cuda(), N, D, xs, ys, w, 1, p)
    return r1, r2, c, (r1["expected"].cpu().numpy(), r2["expected"].cpu().numpy())


def _host_windows(w, sample, E, xs, ys):
    B, D = _band(w, sample)
    return np.concatenate([pr.windows(B.numpy(), N, D, E, xs[i:i + 250], ys[i:i + 250], w)[1] for i in range(0, len(xs), 250)])


@functools.lru_cache(maxsize=None)
def _case(w, p):
    """the 1000 loops once per (w, p): the device's result and the restatement on the device's own E of each band"""
    xs, ys = _loops()
    r1, r2, c, (E1, E2) = _run(w, p, xs, ys)
    oe1, oe2 = _host_windows(w, 1, E1, xs, ys), _host_windows(w, 2, E2, xs, ys)
    sums = cr.sums(oe1, oe2, w, p)
    ref = {"oe1": oe1, "oe2": oe2, "sums": sums, "c1": oe1[:, w, w].copy(), "c2": oe2[:, w, w].copy(), "E": (E1, E2)}
    ref["r1"], ref["r2"], ref["lfc_n"] = cr.ratios(sums, ref["c1"], ref["c2"])
    return (r1, r2, c), ref


def _check(got, ref, w, sl, xs, ys):
    from mustache_amd.pileup import lfc_summary
    r1, r2, c = got
    assert np.array_equal(c["sums"][:, :, 2], ref["sums"][sl][:, :, 2])                  # every cnt
    _within(c["sums"][:, :, :2], ref["sums"][sl][:, :, :2], _bound(w))
    assert _same_bits(r1["center_oe"], ref["c1"][sl]) and _same_bits(r2["center_oe"], ref["c2"][sl])
    _within(c["r1"], ref["r1"][sl], _bound(w))
    _within(c["r2"], ref["r2"][sl], _bound(w))
    _within(c["lfc_n"], ref["lfc_n"][sl], None, _lfc_bound(w, ref["lfc_n"][sl]))
    assert _same_bits(c["lfc"], lfc_summary(c["lfc_n"])) and _same_bits(c["lfc"], cr.summary(c["lfc_n"]))
    T1, T2, C = cr.paired(ref["oe1"][sl], ref["oe2"][sl], xs, ys)
    assert np.array_equal(c["count"], C)
    _within(c["t1"], T1, 2.0 * len(xs) * U)
    _within(c["t2"], T2, 2.0 * len(xs) * U)


@pytest.mark.parametrize("L", [1, 3, 4, 5, 511, 512, 513, 1000])
@pytest.mark.parametrize("w,p", CASES)
def test_cis_against_the_restatement(w, p, L):
    from mustache_amd.pileup import compare_windows, pileup_band
    full, ref = _case(w, p)
    xs, ys = (a[:L] for a in _loops())
    r1, r2, c, E = _run(w, p, xs, ys)
    assert _same_bits(E[0], ref["E"][0]) and _same_bits(E[1], ref["E"][1]) and E[0][20] == 0.0 and E[1][33] == 0.0
    _check((r1, r2, c), ref, w, slice(0, L), xs, ys)
    # each sample's dict is pileup_band's on that map, to the bit
    (B1, D), (B2, _) = _band(w, 1), _band(w, 2)
    for r, B in ((r1, B1), (r2, B2)):
        own = pileup_band(B.cuda(), N, D, xs, ys, w, 1)
        for k in ("sum_obs", "count_obs", "sum_oe", "count_oe", "apa", "apa_oe", "center_obs", "center_oe", "p2ll"):
            assert _same_bits(r[k], own[k]), k
        assert r["obs"] is None and bool((r["oe"] == own["oe"]).logical_or(r["oe"].isnan() & own["oe"].isnan()).all())
    # a second run: the same bits
    again = _run(w, p, xs, ys)[2]
    for k in ("sums", "r1", "r2", "lfc_n", "lfc", "t1", "t2", "count", "diff", "agg_lfc"):
        assert _same_bits(c[k], again[k]), k
    # a loop's twelve numbers do not depend on L or on where the loop sits: the list cut, the list reversed, loops alone
    assert _same_bits(c["sums"], full[2]["sums"][:L])
    oe1, oe2 = r1["oe"], r2["oe"]
    back = compare_windows(oe1.flip(0).contiguous(), oe2.flip(0).contiguous(), w, p).cpu().numpy()
    assert _same_bits(back[::-1], c["sums"])
    for k in sorted({0, L // 2, L - 1}):
        alone = compare_windows(oe1[k:k + 1].contiguous(), oe2[k:k + 1].contiguous(), w, p).cpu().numpy()
        assert _same_bits(alone[0], c["sums"][k]), k
    # the aggregate follows the sort, not the input: a permutation of the loops gives the same bits
    perm = np.random.default_rng(L).permutation(L)
    mixed = _run(w, p, xs[perm].copy(), ys[perm].copy())[2]
    for k in ("t1", "t2", "count", "diff", "lfc_p2ll", "agg_lfc"):
        assert _same_bits(c[k], mixed[k]), k
    assert _same_bits(mixed["sums"], c["sums"][perm])
    if L == 1000:                                                         # the inputs do what they are there for
        cnt, lfc_n, lfc = ref["sums"][:, :, 2], ref["lfc_n"], cr.summary(ref["lfc_n"])
        assert (~np.isnan(lfc_n)).all(axis=1).sum() >= 150
        assert (lfc > 0).sum() >= 40 and (lfc < 0).sum() >= 40 and (lfc == 0).sum() >= 40
        assert (cnt == 0).any()                                          # some neighbourhood without a shared cell
        shared = (~np.isnan(ref["oe1"]) & ~np.isnan(ref["oe2"])).sum()
        assert shared < (~np.isnan(ref["oe1"])).sum() and shared < (~np.isnan(ref["oe2"])).sum()
        for r in (r1, r2):                                               # and so in the aggregate
            assert (c["count"] <= r["count_oe"]).all() and (c["count"] < r["count_oe"]).any()


@pytest.mark.parametrize("w,p", [(10, 2), (32, 5)])
def test_exact_identities(w, p):
    import torch
    from mustache_amd._lib import require_gpu
    from mustache_amd.pileup import _workspace, compare_ratios, compare_windows, diff_map, reduce, reduce_pair
    (r1, _r2, _c), _ref = _case(w, p)
    xs, ys = _loops()
    oe1 = r1["oe"]
    L = oe1.shape[0]
    order = torch.from_numpy(np.lexsort((ys, xs)).astype(np.int32)).cuda()
    ws = _workspace(require_gpu(), 1, 0, L, w, oe1.device)
    # oe2 = 2 oe1, the same NaN mask: the three rows are mst_pileup_reduce's, to the bit, and everything scales exactly
    oe2 = oe1 * 2.0
    own1, own2 = reduce(oe1, oe1, order, w, ws).cpu().numpy(), reduce(oe2, oe2, order, w, ws).cpu().numpy()
    agg = reduce_pair(oe1, oe2, order, w, ws).cpu().numpy()
    assert _same_bits(agg[0], own1[2]) and _same_bits(agg[1], own2[2]) and _same_bits(agg[2], own1[3])
    assert _same_bits(agg[1], 2.0 * agg[0]) and agg[2].max() > 512
    d = diff_map(agg[0], agg[1], agg[2])
    both = (agg[0] > 0) & (agg[2] > 0)
    assert both.sum() > both.size // 2 and (d[both] == -1.0).all() and np.isnan(d[~both]).all()
    c1 = oe1[:, w, w].cpu().numpy()
    sums = compare_windows(oe1, oe2, w, p).cpu().numpy()
    lfc_n = compare_ratios(sums, c1, 2.0 * c1)[2]
    assert (~np.isnan(lfc_n)).sum() > 1000 and (lfc_n[~np.isnan(lfc_n)] == 0.0).all()
    # oe2 = oe1 with the centre cell times 4: the centre is in no neighbourhood, so R_2 = 4 R_1 exactly
    oe2 = oe1.clone()
    oe2[:, w, w] *= 4.0
    sums4 = compare_windows(oe1, oe2, w, p).cpu().numpy()
    assert _same_bits(sums4[:, :, 0], sums4[:, :, 1]) and _same_bits(sums4[:, :, 0], sums[:, :, 0])
    lfc_n = compare_ratios(sums4, c1, 4.0 * c1)[2]
    assert (~np.isnan(lfc_n)).sum() > 1000 and (lfc_n[~np.isnan(lfc_n)] == -2.0).all()
    # an order entry outside 0 .. L-1 is skipped; L = 0 zeroes agg
    holed = order.clone()
    holed[::7] = -1
    holed[3] = L
    keep = np.ones(L, bool)
    keep[::7] = False
    keep[3] = False
    ho = order.cpu().numpy()[keep]
    h1, h2 = oe1.cpu().numpy()[ho], (oe1 * 2.0).cpu().numpy()[ho]
    got = reduce_pair(oe1, oe1 * 2.0, holed, w, ws).cpu().numpy()
    assert np.array_equal(got[2].reshape(h1.shape[1:]), (~np.isnan(h1)).sum(0))
    _within(got[0].reshape(h1.shape[1:]), np.nansum(h1, 0), 2.0 * L * U)
    _within(got[1].reshape(h2.shape[1:]), np.nansum(h2, 0), 2.0 * L * U)
    assert not reduce_pair(oe1[:0], oe1[:0], order[:0], w, ws).cpu().numpy().any()


def test_argument_errors_come_with_a_message_and_launch_nothing():
    import torch
    from mustache_amd import _lib
    from mustache_amd.pileup import PileupError, compare_windows, pileup_band_pair
    oe = torch.zeros((2, 7, 7), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.MstError, match="peak half-width p = 3"):
        compare_windows(oe, oe, 3, 3)
    with pytest.raises(_lib.MstError, match="peak half-width p = -1"):
        compare_windows(oe, oe, 3, -1)
    with pytest.raises(_lib.MstError, match="w = 65"):
        compare_windows(oe, oe, 65, 2)
    with pytest.raises(_lib.MstError, match="null oe2 with L = 2"):
        compare_windows(oe, None, 3, 1)
    lib = _lib.load()
    sums = torch.zeros((2, 4, 3), dtype=torch.float64, device="cuda")
    assert lib.mst_pileup_compare(_lib.ptr(oe), None, 2, 3, 1, _lib.ptr(sums), None) == _lib.MST_E_ARG
    assert b"oe2" in lib.mst_last_error()
    assert lib.mst_pileup_compare(None, None, 0, 3, 1, None, None) == _lib.MST_OK          # L = 0
    B, D = _band(10, 1)
    with pytest.raises(PileupError, match="peak half-width p = 10"):
        pileup_band_pair(B.cuda(), N, B.cuda(), N, D, [10], [50], 10, 6, 10)
    torch.cuda.synchronize()
    assert not sums.cpu().numpy().any()


# ---- the neighbourhood sums, addition by addition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", er.NEIGHBOURHOOD_L)
@pytest.mark.parametrize("w,p", er.NEIGHBOURHOOD_CASES)
def test_mst_pileup_compare_has_the_bytes_of_the_ordered_restatement(w, p, L):
    """mst_pileup_compare under the joint mask of two independent NaN masks against er.ordered_neighbourhood_sums, byte for byte, on values on which another order of
    additions shows (tests/test_pileup_reference.py)"""
    import torch
    from mustache_amd.pileup import compare_windows
    case = er.neighbourhood_case(w, p)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v[:L])).cuda()
    got = compare_windows(d(case["a"]), d(case["b"]), w, p).cpu().numpy()
    counted, first, second = (v[:L] for v in er.neighbourhood_inputs(case, w, "compare"))
    assert got.tobytes() == er.ordered_neighbourhood_sums(counted, first, second, w, p).tobytes()


# ---- trans -----------------------------------------------------------------------------------------------------------------------
def _pair_records(n1, n2, count, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, n1, count).astype(np.int32), rng.integers(0, n2, count).astype(np.int32),
            np.floor(rng.uniform(1.0, 4.0, count)) * rng.uniform(0.5, 1.5, count))


def _pair_loops(n1, n2, extra, seed):
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (n1 - 1, n2 - 1), (0, n2 - 1), (n1 - 1, 0), (n1 // 2, n2 // 2)]
    return (np.concatenate([[f[0] for f in fixed], rng.integers(0, n1, extra)]).astype(np.int64),
            np.concatenate([[f[1] for f in fixed], rng.integers(0, n2, extra)]).astype(np.int64))


def test_trans_records_on_two_maps(monkeypatch):
    from mustache_amd import _lib
    from mustache_amd.pileup import joint_status_trans, pileup_trans_records, pileup_trans_records_pair
    dims1, dims2, w, q, p = (40, 50), (38, 50), 3, 2, 1
    rec1, rec2 = _pair_records(40, 50, 700, 4), _pair_records(38, 50, 700, 5)
    xs, ys = _pair_loops(40, 50, 40, 3)
    xs, ys = np.append(xs, 37), np.append(ys, 10)                         # its window reaches rows 38 .. 40
    status = joint_status_trans(xs, ys, dims1, dims2)
    assert status[1] == status[3] == "off_map" and status[0] == status[2] == "used"      # a = 39 is on map 1 alone
    assert [s == "off_map" for s in status] == [bool(a >= 38) for a in xs]
    used = np.array([s == "used" for s in status])
    xs, ys = xs[used], ys[used]
    r1, r2, c = pileup_trans_records_pair(rec1, dims1, rec2, dims2, xs, ys, w, q, p)
    for r, rec, dims in ((r1, rec1, dims1), (r2, rec2, dims2)):
        own = pileup_trans_records(*rec, *dims, xs, ys, w, q)
        for k in ("sum_oe", "count_oe", "apa_oe", "center_oe", "p2ll", "expected"):
            assert _same_bits(r[k], own[k]), k
    oe1 = ptr.windows(*rec1, *dims1, r1["expected"], xs, ys, w)[1]
    oe2 = ptr.windows(*rec2, *dims2, r2["expected"], xs, ys, w)[1]
    assert (np.isnan(oe1) != np.isnan(oe2)).any()                         # rows 38, 39 are on map 1 alone
    sums = cr.sums(oe1, oe2, w, p)
    ref = {"oe1": oe1, "oe2": oe2, "sums": sums, "c1": oe1[:, w, w].copy(), "c2": oe2[:, w, w].copy()}
    ref["r1"], ref["r2"], ref["lfc_n"] = cr.ratios(sums, ref["c1"], ref["c2"])
    _check((r1, r2, c), ref, w, slice(None), xs, ys)
    # a sparse map: most centres are 0.0 (R = 0, no LFC); the few that have a record on both maps are scored
    assert (c["r1"] == 0).any() and (c["r2"] == 0).any() and (~np.isnan(c["lfc"])).any() and np.isnan(c["lfc"]).any()
    want = cr.aggregate(c["t1"], c["t2"], c["count"], w, q, p)
    for k in ("diff", "lfc_p2ll", "agg_lfc"):
        assert np.allclose(c[k], want[k], rtol=1e-13, atol=1e-14, equal_nan=True), k
    # a sample without a record: E = 0, every oe is NaN, nothing is shared
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    _e1, e2, c = pileup_trans_records_pair(rec1, dims1, none, dims2, xs, ys, w, q, p)
    assert e2["expected"] == 0.0 and not c["sums"].any() and not c["count"].any()
    for k in ("r1", "r2", "lfc_n", "lfc", "diff", "agg_lfc"):
        assert np.isnan(c[k]).all(), k
    # L = 0: empty arrays, and neither entry point is called
    lib = _lib.load()
    calls = []
    for name in ("mst_pileup_compare", "mst_pileup_reduce_pair"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: calls.append(_n))
    _e1, _e2, c = pileup_trans_records_pair(rec1, dims1, rec2, dims2, [], [], w, q, p)
    assert calls == [] and c["sums"].shape == (0, 4, 3) and c["lfc"].shape == (0,) and c["r1"].shape == (0, 4)
    assert not c["count"].any() and np.isnan(c["diff"]).all()


# ---- the command line ------------------------------------------------------------------------------------------------------------
HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"


def _text_map(tmp_path, tag, n, seed, res):
    from mustache_amd.synth import synth_coo
    x, y, v = synth_coo(n, 90, depth=200.0, seed=seed, nloops=20)
    t, bf = str(tmp_path / ("m%s.txt" % tag)), str(tmp_path / ("b%s.txt" % tag))
    with open(t, "w") as fh:
        fh.write("".join("%d\t%d\t%d\n" % (a * res, b * res, max(1, round(c))) for a, b, c in zip(x, y, v)))
    with open(bf, "w") as fh:
        fh.write("".join("%r\n" % float(b) for b in np.random.default_rng(seed + 1).uniform(0.5, 1.5, n)))
    return t, bf


def _host_pileup(t, bf, D, res, xs, ys, w):
    """the restatement's pile-up of a text map, from the host reader's records: (its dict, n)"""
    from mustache_amd.mustache import read_pd
    rx, ry, rv = read_pd(t, D * res, bf, "1", res)
    rx, ry = np.asarray(rx, np.int64), np.asarray(ry, np.int64)
    nn = int(max(rx.max(), ry.max())) + 1
    B = np.zeros((D + 2, nn))
    keep = ry - rx <= D + 1
    B[(ry - rx)[keep], rx[keep]] = np.asarray(rv)[keep]
    return pr.pileup_band(B[:D + 1], nn, D, xs, ys, w, 6), nn


def test_cli_end_to_end(tmp_path, monkeypatch, capsys):
    """`PREFIX.1.*` against a single-map run of -f on the list cut to the jointly used rows: the two matrices byte for byte; the
    loops file line for line on the used rows and the stats file in every column but ROWS_IN -- those two files list every row
    of the list they were given, so the cut list's own are shorter by the rows that were cut."""
    from mustache_amd import _lib
    from mustache_amd.pileup import COMPARE_COLUMNS, main
    res, w, p, T = 10000, 10, 2, 0.25
    n1, n2 = 500, 470
    t1, b1 = _text_map(tmp_path, "1", n1, 9, res)
    t2, b2 = _text_map(tmp_path, "2", n2, 21, res)
    rng = np.random.default_rng(4)
    sep = rng.integers(30, 66, 60)
    sep[0] = 65                                                          # D comes from a used row, so the cut list has the same D
    xs = rng.integers(0, n2 - 10 - sep)
    xs[0], xs[1] = 0, n2 - 10 - sep[1]
    ys = xs + sep
    rows = ["1\t%d\t%d\t1\t%d\t%d\t0.0%d\t1.6" % (a * res, (a + 1) * res, b * res, (b + 1) * res, k % 7)
            for k, (a, b) in enumerate(zip(xs, ys))]
    used_rows = list(rows)
    rows.insert(3, "1\t1000000\t1010000\t1\t1050000\t1060000\t0.01\t1.6")               # short: 5 bins apart
    rows.insert(7, "1\t1000000\t1010000\t2\t2000000\t2010000\t0.01\t1.6")               # trans
    rows.insert(11, "1\t%d\t%d\t1\t%d\t%d\t0.01\t1.6" % (440 * res, 441 * res, 485 * res, 486 * res))   # on map 1, beyond map 2
    lp, cut = str(tmp_path / "l.tsv"), str(tmp_path / "cut.tsv")
    with open(lp, "w") as fh:
        fh.write(HEADER + "\n" + "".join(r + "\n" for r in rows))
    with open(cut, "w") as fh:
        fh.write(HEADER + "\n" + "".join(r + "\n" for r in used_rows))
    lib = _lib.load()
    calls = []
    for name in ("mst_pileup_compare", "mst_pileup_reduce_pair"):
        def counting(*a, _fn=getattr(lib, name), _n=name):
            calls.append(_n)
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)
    base = ["-l", lp, "-r", str(res), "-f", t1, "-b", b1]
    old, two, thr, single = (str(tmp_path / k) for k in ("old", "two", "thr", "single"))
    main(base + ["-o", old])                                              # without -f2: no new launch, the four old files
    assert calls == []
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("old.")) == ["old.apa.tsv", "old.loops.tsv", "old.oe.tsv",
                                                                               "old.stats.tsv"]
    main(base + ["-o", two, "-f2", t2, "-b2", b2])
    assert calls == ["mst_pileup_reduce_pair", "mst_pileup_compare"]     # one chromosome: one launch of each
    said = capsys.readouterr().out
    assert "Error" not in said and "LFC_P2LL" in said.splitlines()[-1] and "%d of %d loops" % (len(xs), len(rows)) in said.splitlines()[-1]
    eleven = sorted(["two.%s.%s.tsv" % (s, k) for s in "12" for k in ("apa", "oe", "stats", "loops")]
                    + ["two.compare.tsv", "two.diff.tsv", "two.compare.stats.tsv"])
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("two.")) == eleven
    main(base + ["-o", thr, "-f2", t2, "-b2", b2, "--min-lfc", str(T)])
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("thr.")) == sorted(
        [f.replace("two.", "thr.") for f in eleven] + ["thr.up1.tsv", "thr.up2.tsv"])
    for f in eleven:
        assert open(str(tmp_path / f), "rb").read() == open(str(tmp_path / f.replace("two.", "thr.")), "rb").read(), f
    # sample 1 alone on the jointly used rows
    main(["-l", cut, "-r", str(res), "-f", t1, "-b", b1, "-o", single])
    for ext in (".apa.tsv", ".oe.tsv"):
        assert open(two + ".1" + ext, "rb").read() == open(single + ext, "rb").read(), ext
    mine = [ln for ln in open(two + ".1.loops.tsv").read().splitlines() if ln.split("\t")[8] in ("used", "STATUS")]
    assert mine == open(single + ".loops.tsv").read().splitlines() and len(mine) == 1 + len(xs)
    a, b = ([ln.split("\t") for ln in open(f + ".stats.tsv").read().splitlines()] for f in (two + ".1", single))
    assert [f[:1] + f[2:] for f in a] == [f[:1] + f[2:] for f in b] and [f[1] for f in a[1:]] == ["62", "63"]
    # compare.tsv against the restatement, from the host reader's records of each map
    D = int(sep.max()) + 2 * w
    (want1, nn1), (want2, nn2) = _host_pileup(t1, b1, D, res, xs, ys, w), _host_pileup(t2, b2, D, res, xs, ys, w)
    assert nn2 < 486 <= nn1
    sums = cr.sums(want1["oe"], want2["oe"], w, p)
    r1, r2, lfc_n = cr.ratios(sums, want1["center_oe"], want2["center_oe"])
    extra = 4.0 * max(nn1, nn2) * U                                       # E: two orders of a sum of at most n non-negative terms
    lines = open(two + ".compare.tsv").read().splitlines()
    assert lines[0] == HEADER + "\t" + "\t".join(COMPARE_COLUMNS)
    body = [ln.split("\t") for ln in lines[1:]]
    assert ["\t".join(f[:8]) for f in body] == rows                       # the rows as read, in input order
    assert [body[k][8] for k in (3, 7, 11)] == ["short", "trans", "off_map"]
    for k in (3, 7, 11):
        assert all(s == "nan" for s in body[k][9:]) and len(body[k]) == 8 + len(COMPARE_COLUMNS)
    used = [f for f in body if f[8] == "used"]
    assert ["\t".join(f[:8]) for f in used] == used_rows
    got = np.array([[float(s) for s in f[9:]] for f in used])
    _within(got[:, 0], want1["center_oe"], _bound(w) + extra)
    _within(got[:, 1], want2["center_oe"], _bound(w) + extra)
    _within(got[:, 2:6], r1, _bound(w) + extra)
    _within(got[:, 6:10], r2, _bound(w) + extra)
    _within(got[:, 10:14], lfc_n, None, _lfc_bound(w, lfc_n, extra))
    assert _same_bits(got[:, 14], cr.summary(got[:, 10:14])) and (~np.isnan(got[:, 14])).sum() > len(xs) // 2
    # the thresholded lists: exactly the used rows by the LFC as written, unchanged and in input order
    up1, up2 = (open(thr + e).read().splitlines() for e in (".up1.tsv", ".up2.tsv"))
    assert up1[0] == up2[0] == HEADER
    assert up1[1:] == ["\t".join(f[:8]) for f in used if float(f[-1]) >= T]
    assert up2[1:] == ["\t".join(f[:8]) for f in used if float(f[-1]) <= -T]
    assert len(up1) + len(up2) > 2 and not set(up1[1:]) & set(up2[1:])
    stats = [ln.split("\t") for ln in open(two + ".compare.stats.tsv").read().splitlines()]
    assert [s[0] for s in stats] == ["CHR", "1", "all"] and stats[1][1:] == stats[2][1:] and stats[1][1] == str(len(xs))
    T1, T2, C = cr.paired(want1["oe"], want2["oe"], xs, ys)
    agg = cr.aggregate(T1, T2, C, w, 6, p)
    _within([float(s) for s in stats[2][2:4]], [agg["p2ll_1"], agg["p2ll_2"]], 1e-11)
    _within([float(s) for s in stats[2][4:]], [agg["lfc_p2ll"]] + list(agg["agg_lfc"]), None, 1e-11)
    d = np.array([[float(s) for s in ln.split("\t")] for ln in open(two + ".diff.tsv").read().splitlines()])
    _within(d, agg["diff"], None, 1e-11)
