"""The enrichment of every loop over its local background on the MI355X (mst_pileup_enrich, csrc/mst_pileup_enrich.hip, and
the `peak` keyword of mustache_amd/pileup.py) against the cell-by-cell restatement (tests/pileup_enrich_reference.py): cis at
every window size the lanes walk differently, trans pairs alone and in a batch, and the command line end to end.

Bounds.  S_o and S_e are sums of at most (2w+1)^2 non-negative terms: in any order each is within (2w+1)^2 * 2^-53 of the exact
sum, relatively, so two orders differ by at most twice that; EXP = E_centre * S_o / S_e carries both sums and two roundings, FE
one more.  4 * (2w+1)^2 * 2^-53 covers all of them.  Counts and NaN positions are exact."""
import functools
import os

import numpy as np
import pytest

import pileup_enrich_reference as er
import pileup_reference as pr
import pileup_trans_reference as ptr

pytestmark = pytest.mark.gpu

N, SEP_MAX, ZERO_DIAGONAL, BAD_BINS = 300, 60, 20, range(150, 156)
ENRICH_KEYS = ("center_e", "enrich_sums", "enrich_exp", "enrich_fe", "fe_min", "enrich_agg")


def _bound(w):
    return 4.0 * (2 * w + 1) ** 2 * 2.0 ** -53


def _within(a, b, rel):
    """the same NaN positions, and the rest within the relative bound"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    err = np.abs(a[ok] - b[ok])
    assert (err <= rel * np.maximum(np.abs(a[ok]), np.abs(b[ok]))).all(), float(err.max())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _band(w):
    """(a raw band [D + 2, N] built with torch, D): values >= 0, a third of them zero, nothing beyond the chromosome's end, one
    diagonal zeroed whole (E = 0 there) and every pixel that touches a BAD_BINS bin removed (those bins are invalid)"""
    import torch
    D = SEP_MAX + 2 * w
    g = torch.Generator().manual_seed(100 + w)
    B = torch.floor(torch.rand((D + 2, N), generator=g, dtype=torch.float64) * 3.0) \
        * (0.5 + torch.rand((D + 2, N), generator=g, dtype=torch.float64))
    for d in range(D + 2):
        B[d, N - d:] = 0.0
    B[ZERO_DIAGONAL] = 0.0
    for m in BAD_BINS:
        B[:, m] = 0.0
        for d in range(min(D + 2, m + 1)):
            B[d, m - d] = 0.0
    return B.contiguous(), D


def _loops():
    """1000 loops, y - x <= SEP_MAX.  The first ones are placed: at bin 0 and at bin N - 1 (cells off the chromosome; (N - 1, N - 1)
    has every cell with a >= 1 off it: its LL is empty), y - x < 2w (mirrored cells, d = 0), on the zeroed diagonal (E_centre =
    0), among the invalid bins."""
    rng = np.random.default_rng(11)
    placed = [(0, 40), (N - 36, N - 1), (N - 1, N - 1), (0, 0), (100, 101), (60, 60 + ZERO_DIAGONAL), (152, 190), (140, 153),
              (2, 58), (N - 2, N - 1)]
    sep = rng.integers(0, SEP_MAX + 1, 1000 - len(placed))
    x = rng.integers(0, N - sep)
    xs = np.concatenate([[a for a, _ in placed], x]).astype(np.int64)
    ys = np.concatenate([[b for _, b in placed], x + sep]).astype(np.int64)
    return xs, ys


def _run(w, p, xs, ys):
    from mustache_amd.pileup import pileup_band
    B, D = _band(w)
    r = pileup_band(B.cuda(), N, D, xs, ys, w, 1, peak=p)
    E = r["expected"].cpu().numpy()
    return {k: v for k, v in r.items() if k not in ("obs", "oe", "valid", "expected")}, E


@functools.lru_cache(maxsize=None)
def _case(w, p):
    """the 1000 loops once per (w, p): the device's result and the restatement on the device's own E"""
    xs, ys = _loops()
    r, E = _run(w, p, xs, ys)
    B, D = _band(w)
    obs = np.concatenate([pr.windows(B.numpy(), N, D, E, xs[i:i + 250], ys[i:i + 250], w)[0] for i in range(0, len(xs), 250)])
    sums = er.cis_sums(obs, w, p, E, D, xs, ys)
    centre, centre_e = obs[:, w, w].copy(), E[ys - xs]
    return r, {"sums": sums, "centre": centre, "centre_e": centre_e, "ratios": er.ratios(sums, centre, centre_e), "E": E}


def _check(r, ref, w, sl):
    assert np.array_equal(r["enrich_sums"][:, :, 2], ref["sums"][sl][:, :, 2])           # every cnt
    _within(r["enrich_sums"][:, :, :2], ref["sums"][sl][:, :, :2], _bound(w))
    assert _same_bits(r["center_obs"], ref["centre"][sl]) and _same_bits(r["center_e"], ref["centre_e"][sl])
    for got, want in zip((r["enrich_exp"], r["enrich_fe"], r["fe_min"]), ref["ratios"]):
        _within(got, want[sl], _bound(w))


@pytest.mark.parametrize("L", [1, 3, 4, 5, 1000])
@pytest.mark.parametrize("w,p", [(1, 0), (10, 2), (32, 5), (64, 63)])
def test_cis_against_the_restatement(w, p, L):
    full, ref = _case(w, p)
    xs, ys = (a[:L] for a in _loops())
    r, E = _run(w, p, xs, ys)
    assert _same_bits(E, ref["E"]) and E[ZERO_DIAGONAL] == 0.0
    _check(r, ref, w, slice(0, L))
    again, _ = _run(w, p, xs, ys)                                         # a second run: the same bits
    for k in ENRICH_KEYS:
        assert _same_bits(r[k], again[k]), k
    # a loop's twelve numbers do not depend on L or on where the loop sits: the list reversed, and loops alone
    assert _same_bits(r["enrich_sums"], full["enrich_sums"][:L])
    back, _ = _run(w, p, xs[::-1].copy(), ys[::-1].copy())
    assert _same_bits(back["enrich_sums"][::-1], r["enrich_sums"])
    for k in sorted({0, L // 2, L - 1}):
        alone, _ = _run(w, p, xs[k:k + 1], ys[k:k + 1])
        assert _same_bits(alone["enrich_sums"][0], r["enrich_sums"][k]), k
    if L == 1000:                                                         # the placements do what they are there for
        cnt, fe_min = ref["sums"][:, :, 2], ref["ratios"][2]
        assert cnt[2, 1] == 0 and (cnt[2] == 0).sum() >= 1                # (N - 1, N - 1): LL empty
        assert cnt[0, 0] < cnt[4, 0]                                      # bin 0 loses cells against an interior loop
        assert ref["centre_e"][5] == 0.0 and np.isnan(fe_min[5])          # E_centre = 0
        assert np.isnan(fe_min).any() and (~np.isnan(fe_min)).sum() > 300
        assert _same_bits(full["enrich_agg"], again["enrich_agg"]) and not np.isnan(full["enrich_agg"]).all()


def test_the_aggregate_is_the_host_rule_on_the_mean_map():
    full, _ref = _case(10, 2)
    assert np.allclose(full["enrich_agg"], er.aggregate(full["apa_oe"], 10, 2), rtol=1e-13, equal_nan=True)
    assert not np.isnan(full["enrich_agg"]).any()


def test_without_a_peak_nothing_is_added():
    from mustache_amd.pileup import pileup_band
    B, D = _band(10)
    xs, ys = (a[:20] for a in _loops())
    r = pileup_band(B.cuda(), N, D, xs, ys, 10, 6)
    assert not set(ENRICH_KEYS) & set(r)
    assert not set(ENRICH_KEYS) & set(pileup_band(B.cuda(), N, D, [], [], 10, 6))
    e = pileup_band(B.cuda(), N, D, [], [], 10, 6, peak=2)                # L = 0 with a peak: empty arrays, no launch
    assert e["enrich_sums"].shape == (0, 4, 3) and e["fe_min"].shape == (0,) and np.isnan(e["enrich_agg"]).all()


def test_argument_errors_come_with_a_message_and_launch_nothing():
    import torch
    from mustache_amd import _lib
    from mustache_amd.pileup import PileupError, enrich_windows, pileup_band
    obs = torch.zeros((2, 7, 7), dtype=torch.float64, device="cuda")
    e = torch.ones(2, dtype=torch.float64, device="cuda")
    E = torch.ones(5, dtype=torch.float64, device="cuda")
    xy = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.MstError, match="peak half-width p = 3"):
        enrich_windows(obs, 3, 3, e_loop=e)
    with pytest.raises(_lib.MstError, match="peak half-width p = -1"):
        enrich_windows(obs, 3, -1, e_loop=e)
    with pytest.raises(_lib.MstError, match="w = 65"):
        enrich_windows(obs, 65, 2, e_loop=e)
    lib = _lib.load()
    both = lib.mst_pileup_enrich(_lib.ptr(obs), 2, 3, 1, _lib.ptr(E), 4, _lib.ptr(xy), _lib.ptr(xy), _lib.ptr(e), _lib.ptr(e), None)
    none = lib.mst_pileup_enrich(_lib.ptr(obs), 2, 3, 1, None, 4, _lib.ptr(xy), _lib.ptr(xy), None, _lib.ptr(e), None)
    assert both == none == _lib.MST_E_ARG and b"exactly one" in lib.mst_last_error()
    assert lib.mst_pileup_enrich(None, 0, 3, 1, None, 0, None, None, None, None, None) == _lib.MST_OK     # L = 0
    B, D = _band(10)
    with pytest.raises(PileupError, match="peak half-width p = 10"):
        pileup_band(B.cuda(), N, D, [10], [50], 10, 6, peak=10)
    torch.cuda.synchronize()


# ---- the neighbourhood sums, addition by addition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", er.NEIGHBOURHOOD_L)
@pytest.mark.parametrize("w,p", er.NEIGHBOURHOOD_CASES)
def test_mst_pileup_enrich_has_the_bytes_of_the_ordered_restatement(w, p, L):
    """mst_pileup_enrich, cis (a zero diagonal in E, cells beyond D) and trans, against er.ordered_neighbourhood_sums, byte for byte, on values on which another order of
    additions shows (tests/test_pileup_reference.py)"""
    import torch
    from mustache_amd.pileup import enrich_windows
    case = er.neighbourhood_case(w, p)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v[:L])).cuda()
    got = {"cis": enrich_windows(d(case["a"]), w, p, E=torch.from_numpy(case["E"]).cuda(), xs=d(case["xs"]), ys=d(case["ys"])),
           "trans": enrich_windows(d(case["a"]), w, p, e_loop=d(case["e_loop"]))}
    for kind in ("cis", "trans"):
        counted, first, second = (v[:L] for v in er.neighbourhood_inputs(case, w, kind))
        assert got[kind].cpu().numpy().tobytes() == er.ordered_neighbourhood_sums(counted, first, second, w, p).tobytes(), kind


# ---- trans -------------------------------------------------------------------------------------------------------------------
def _pair_records(n1, n2, count, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, n1, count).astype(np.int32), rng.integers(0, n2, count).astype(np.int32),
            np.floor(rng.uniform(1.0, 4.0, count)) * rng.uniform(0.5, 1.5, count))


def _pair_loops(n1, n2, extra, seed):
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (n1 - 1, n2 - 1), (0, n2 - 1), (n1 - 1, 0), (n1 // 2, n2 // 2)]
    return (np.concatenate([[f[0] for f in fixed], rng.integers(0, n1, extra)]).astype(np.int64),
            np.concatenate([[f[1] for f in fixed], rng.integers(0, n2, extra)]).astype(np.int64))


def test_trans_records_with_and_without_records():
    from mustache_amd.pileup import pileup_trans_records
    n1, n2, w, p = 40, 50, 3, 1
    xs, ys = _pair_loops(n1, n2, 20, 3)
    none = np.zeros(0, np.int32)
    r = pileup_trans_records(none, none, np.zeros(0), n1, n2, xs, ys, w, 2, peak=p)      # N = 0: E = 0, nothing counts
    assert r["expected"] == 0.0 and not r["enrich_sums"].any() and not r["center_e"].any()
    for k in ("enrich_exp", "enrich_fe", "fe_min", "enrich_agg"):
        assert np.isnan(r[k]).all(), k
    x, y, v = _pair_records(n1, n2, 700, 4)
    r = pileup_trans_records(x, y, v, n1, n2, xs, ys, w, 2, peak=p)
    E = r["expected"]
    obs, _oe = ptr.windows(x, y, v, n1, n2, E, xs, ys, w)
    assert np.isnan(obs).any() and (obs == 0).any() and E > 0
    sums = er.trans_sums(obs, w, p, E)
    ref = {"sums": sums, "centre": obs[:, w, w].copy(), "centre_e": np.full(len(xs), E),
           "ratios": er.ratios(sums, obs[:, w, w], np.full(len(xs), E))}
    _check(r, ref, w, slice(None))
    assert np.allclose(r["enrich_agg"], er.aggregate(r["apa_oe"], w, p), rtol=1e-13, equal_nan=True)
    assert not set(ENRICH_KEYS) & set(pileup_trans_records(x, y, v, n1, n2, xs, ys, w, 2))
    e = pileup_trans_records(x, y, v, n1, n2, [], [], w, 2, peak=p)                       # L = 0
    assert e["enrich_sums"].shape == (0, 4, 3) and e["expected"] == E


def test_a_batch_gives_every_pair_the_bits_it_has_alone():
    from mustache_amd.pileup import pileup_trans_batch, pileup_trans_records
    w, q, p = 4, 2, 1
    dims = [(40, 50), (30, 30), (25, 35)]
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    recs = [_pair_records(40, 50, 600, 1), _pair_records(30, 30, 300, 2), none]           # pair 2 without a record
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    loops = [_pair_loops(40, 50, 30, 5), empty, _pair_loops(25, 35, 9, 6)]                # pair 1 without a loop
    seg = np.concatenate([[0], np.cumsum([len(r[2]) for r in recs])]).astype(np.int64)
    x, y, v = (np.concatenate([r[k] for r in recs]) for k in range(3))
    got = pileup_trans_batch(x, y, v, seg, dims, loops, w, q, peak=p)
    for i in range(3):
        alone = pileup_trans_records(*recs[i], dims[i][0], dims[i][1], loops[i][0], loops[i][1], w, q, peak=p)
        for k in ENRICH_KEYS + ("center_obs", "apa_oe"):
            assert _same_bits(got[i][k], alone[k]), (i, k)
    assert got[0]["enrich_sums"][:, :, 2].any() and not np.isnan(got[0]["fe_min"]).all()
    assert got[1]["enrich_sums"].shape == (0, 4, 3) and not got[2]["enrich_sums"].any()
    plain = pileup_trans_batch(x, y, v, seg, dims, loops, w, q)
    assert not set(ENRICH_KEYS) & set(plain[0])
    assert _same_bits(plain[0]["p2ll"], got[0]["p2ll"]) and _same_bits(plain[0]["sum_oe"], got[0]["sum_oe"])


# ---- the command line --------------------------------------------------------------------------------------------------------
HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"


def test_cli_end_to_end(tmp_path, monkeypatch, capsys):
    from mustache_amd import _lib
    from mustache_amd.mustache import read_pd
    from mustache_amd.pileup import ENRICH_COLUMNS, main
    from mustache_amd.synth import synth_coo
    n, dpx, res, w, p, T = 500, 90, 10000, 10, 2, 1.0
    x, y, v = synth_coo(n, dpx, depth=200.0, seed=9, nloops=20)
    t, bf, lp = str(tmp_path / "m.txt"), str(tmp_path / "b.txt"), str(tmp_path / "l.tsv")
    with open(t, "w") as fh:
        fh.write("".join("%d\t%d\t%d\n" % (a * res, b * res, max(1, round(c))) for a, b, c in zip(x, y, v)))
    with open(bf, "w") as fh:
        fh.write("".join("%r\n" % float(b) for b in np.random.default_rng(2).uniform(0.5, 1.5, n)))
    rng = np.random.default_rng(4)
    sep = rng.integers(30, 66, 60)
    xs = rng.integers(0, n - 10 - sep)
    xs[0], xs[1] = 0, n - 10 - sep[1]                                    # both ends: cells off the chromosome
    ys = xs + sep
    rows = ["1\t%d\t%d\t1\t%d\t%d\t0.0%d\t1.6" % (a * res, (a + 1) * res, b * res, (b + 1) * res, k % 7)
            for k, (a, b) in enumerate(zip(xs, ys))]
    rows.insert(3, "1\t1000000\t1010000\t1\t1050000\t1060000\t0.01\t1.6")               # short: 5 bins apart
    rows.insert(7, "1\t1000000\t1010000\t2\t2000000\t2010000\t0.01\t1.6")               # trans
    with open(lp, "w") as fh:
        fh.write(HEADER + "\n" + "".join(r + "\n" for r in rows))
    lib = _lib.load()
    calls, bound_fn = [], lib.mst_pileup_enrich

    def counting(*a):
        calls.append(a[1])
        return bound_fn(*a)
    monkeypatch.setattr(lib, "mst_pileup_enrich", counting)
    old, new = str(tmp_path / "old"), str(tmp_path / "new")
    main(["-f", t, "-l", lp, "-r", str(res), "-o", old, "-b", bf])
    assert calls == []                                                   # peak=None: no launch of the kernel
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("old")) == ["old.apa.tsv", "old.loops.tsv", "old.oe.tsv",
                                                                              "old.stats.tsv"]
    main(["-f", t, "-l", lp, "-r", str(res), "-o", new, "-b", bf, "--enrich", "--min-enrichment", str(T)])
    assert calls == [len(xs)]                                            # one chromosome, one launch, the used loops
    assert "Error" not in capsys.readouterr().out
    for ext in (".apa.tsv", ".oe.tsv", ".stats.tsv", ".loops.tsv"):
        assert open(old + ext, "rb").read() == open(new + ext, "rb").read(), ext
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("new")) == [
        "new.apa.tsv", "new.enrich.stats.tsv", "new.enrich.tsv", "new.enriched.tsv", "new.loops.tsv", "new.oe.tsv", "new.stats.tsv"]
    # the restatement, from the host reader's records
    D = int(sep.max()) + 2 * w
    rx, ry, rv = read_pd(t, D * res, bf, "1", res)
    rx, ry = np.asarray(rx, np.int64), np.asarray(ry, np.int64)
    nn = int(max(rx.max(), ry.max())) + 1
    B = np.zeros((D + 2, nn))
    keep = ry - rx <= D + 1
    B[(ry - rx)[keep], rx[keep]] = np.asarray(rv)[keep]
    want = pr.pileup_band(B[:D + 1], nn, D, xs, ys, w, 6)
    sums = er.cis_sums(want["obs"], w, p, want["expected"], D, xs, ys)
    centre_e = want["expected"][ys - xs]
    exp, fe, fe_min = er.ratios(sums, want["center_obs"], centre_e)
    # E of the restatement and of the device are two orders of one sum of at most nn non-negative terms: EXP carries E_centre
    # and the E's inside S_e, 4 * nn * 2^-53 for the two of them, on top of the bound above
    rel = _bound(w) + 4.0 * nn * 2.0 ** -53
    lines = open(new + ".enrich.tsv").read().splitlines()
    assert lines[0] == HEADER + "\t" + "\t".join(ENRICH_COLUMNS)
    body = [ln.split("\t") for ln in lines[1:]]
    assert ["\t".join(f[:8]) for f in body] == rows                       # the rows as read, in input order
    used = [f for f in body if f[8] == "used"]
    assert [f[8] for f in body[3:8:4]] == ["short", "trans"] and len(used) == len(xs)
    for f in (body[3], body[7]):
        assert all(s == "nan" for s in f[9:]) and len(f) == 8 + len(ENRICH_COLUMNS)
    got = np.array([[float(s) for s in f[9:]] for f in used])
    _within(got[:, 0], want["center_obs"], rel)
    _within(got[:, 1], centre_e, rel)
    _within(got[:, 2:6], exp, rel)
    _within(got[:, 6:10], fe, rel)
    _within(got[:, 10], fe_min, rel)
    assert (~np.isnan(fe_min)).sum() > len(xs) // 2
    # the filtered list: exactly the used rows whose FE_MIN (as written) is >= T, unchanged and in input order
    kept = open(new + ".enriched.tsv").read().splitlines()
    assert kept[0] == HEADER
    assert kept[1:] == ["\t".join(f[:8]) for f in used if float(f[19]) >= T]
    assert 0 < len(kept) - 1 < len(used)
    stats = [ln.split("\t") for ln in open(new + ".enrich.stats.tsv").read().splitlines()]
    assert [s[0] for s in stats] == ["CHR", "1", "all"] and stats[1][1:] == stats[2][1:] and stats[1][1] == str(len(xs))
    _within([float(s) for s in stats[2][2:]], er.aggregate(want["apa_oe"], w, p), 1e-11)
