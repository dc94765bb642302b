"""The significance of every loop of a pile-up on the MI355X (mst_pileup_centre_counts, mst_pileup_poisson,
csrc/mst_pileup_poisson.hip, the `poisson` keyword of mustache_amd/pileup.py and --poisson) against the restatement
(tests/pileup_poisson_reference.py) and SciPy: the pass over the raw records at every record and key count its paths change at,
the tail on the CPU test's grid, pileup_band on the enrichment test's set-up, and the command line end to end from a `.hic` and a
pairs file.

Bounds.  Counts, statuses and NaN positions are exact.  EXP and FE have the bits of pileup.enrichment() on the device's sums.
LAMBDA is within the enrichment test's bound, 4 (2w+1)^2 2^-53, of the restatement (it carries EXP and two more roundings), and
has the bits of (EXP * b1) * b2 on the device's EXP.  P is within 1e-9, relatively, of SciPy and of the restatement at the same
LAMBDA wherever it is >= 1e-290 (the argument is tests/test_pileup_poisson_reference.py's: the device's lgamma / log / exp
differ from glibc's by ulps, which the margin of 50 absorbs); below that both must be below 1e-290."""
import functools
import math
import os

import numpy as np
import pytest

import pileup_enrich_reference as er
import pileup_poisson_reference as ref
import pileup_reference as pr
import test_gpu_pileup_enrich as ge
from test_pileup_poisson_reference import check_tail, grid

pytestmark = pytest.mark.gpu

POISSON_KEYS = ("raw_center", "bias1", "bias2", "poisson_lambda", "poisson_p", "p_max", "poisson_unconverged")


def _p_max(p):
    """the largest of each row of P [L, 4], NaN when one of the four is"""
    p = np.asarray(p, np.float64).reshape(-1, 4)
    return np.array([math.nan if any(math.isnan(t) for t in row) else max(row) for row in p], np.float64).reshape(-1)


def _same_numbers(a, b):
    """the same NaN positions and the same bits everywhere else"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


# ---- the pass over the raw records ------------------------------------------------------------------------------------------
CN, CD = 500, 90


@functools.lru_cache(maxsize=None)
def _records(R):
    """R records of a map of CN bins, distances 0 .. CD: far fewer pixels than 100 000 records, so pixels repeat (counts add)"""
    rng = np.random.default_rng(1000 + R)
    d = rng.integers(0, CD + 1, R)
    x = rng.integers(0, CN - d) if R else np.zeros(0, np.int64)
    return x.astype(np.int32), d.astype(np.int32), rng.integers(1, 60, R).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _distinct(K):
    """K distinct centre pixels (x, y) sorted by key x << 32 | (y - x): bin 0, bin CN - 1, the diagonal and the largest distance
    first, then seeded draws -- pixels the record sets may or may not hold"""
    rng = np.random.default_rng(77)
    have = {(0, 35), (CN - 41, CN - 1), (0, 0), (CN - 1, CN - 1), (3, 3 + CD)}
    have = set(sorted(have)[:K])
    while len(have) < K:
        d = int(rng.integers(0, CD + 1))
        a = int(rng.integers(0, CN - d))
        have.add((a, a + d))
    px = sorted(have, key=lambda t: (t[0] << 32) | (t[1] - t[0]))
    return np.array([a for a, _ in px], np.int64), np.array([b for _, b in px], np.int64)


def _want(R, xs, ys):
    x, d, c = _records(R)
    return ref.centre_counts(x, d, c, xs, ys)


@pytest.mark.parametrize("kind", ["float32", "int64"])
@pytest.mark.parametrize("K", [0, 1, 64, 65, 9000])
@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 100000])
def test_centre_counts_against_a_dict(R, K, kind):
    import torch
    from mustache_amd.pileup import centre_counts
    x, d, c = _records(R)
    xs, ys = _distinct(K)
    keys = (xs << 32) | (ys - xs)
    assert (np.diff(keys) > 0).all()
    cd = torch.from_numpy(c.astype(np.float32) if kind == "float32" else c).cuda()
    xd, dd, kd = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(keys).cuda()
    lo, hi = (int((ys - xs).min()), int((ys - xs).max())) if K else (0, 0)
    got, flag = centre_counts(xd, dd, cd, kd, lo, hi)
    want = _want(R, xs, ys)
    assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == want.tolist() and int(flag.item()) == 0
    if R == 100000 and K >= 64:
        assert (want > 0).sum() > K // 4 and (want == 0).any()            # hits, and pixels the set does not hold
        assert max(want) > 59                                             # a pixel that several records name: the counts add
    if R > 1 and K:                                                       # any order of the records: the same bits
        perm = torch.from_numpy(np.random.default_rng(R + K).permutation(R)).cuda()
        again, _ = centre_counts(xd[perm], dd[perm], cd[perm], kd, lo, hi)
        assert torch.equal(again, got)


def test_a_list_that_names_a_pixel_twice_and_a_fractional_count():
    import torch
    from mustache_amd import _lib
    from mustache_amd.pileup import PileupError, PoissonInput, centre_counts, pileup_band
    x, d, c = _records(100000)
    w = 1
    B, D = ge._band(w)
    hit = int(np.flatnonzero((x < 200) & (d >= 1) & (d <= 60))[0])        # a pixel the set holds, inside the band of w = 1
    a, sep = int(x[hit]), int(d[hit])
    xs = np.array([a, 0, a, ge.N - 1, a], np.int64)
    ys = np.array([a + sep, 35, a + sep, ge.N - 1, a + sep - 1], np.int64)          # (a, a + sep) twice
    raw = PoissonInput(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), np.ones(CN))
    r = pileup_band(B.cuda(), ge.N, D, xs, ys, w, 1, peak=0, poisson=raw)
    want = _want(100000, xs, ys)
    assert r["raw_center"].tolist() == want.tolist() and want[0] == want[2] > 0
    # a float32 count that is no integer: the flag, and pileup_band's refusal; nothing is rounded
    bad = c.astype(np.float32)
    bad[hit] += 0.5
    keys = torch.from_numpy(np.array([(a << 32) | sep], np.int64)).cuda()
    _got, flag = centre_counts(raw.x, raw.dist, torch.from_numpy(bad).cuda(), keys, sep, sep)
    assert int(flag.item()) == 1
    for v in (np.nan, -1.0, np.inf):
        bad[hit] = v
        assert int(centre_counts(raw.x, raw.dist, torch.from_numpy(bad).cuda(), keys, sep, sep)[1].item()) == 1
    bad[hit] = 2.5
    with pytest.raises(PileupError, match="not an integer value"):
        pileup_band(B.cuda(), ge.N, D, xs, ys, w, 1, peak=0, poisson=PoissonInput(raw.x, raw.dist, torch.from_numpy(bad).cuda(), np.ones(CN)))
    with pytest.raises(PileupError, match="poisson= without peak="):
        pileup_band(B.cuda(), ge.N, D, xs, ys, w, 1, poisson=raw)
    lib = _lib.load()
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    assert lib.mst_pileup_centre_counts(None, None, None, 0, 0, None, 0, 0, 0, None, None, None) == _lib.MST_OK       # K = 0
    assert lib.mst_pileup_centre_counts(p(raw.x), p(raw.dist), p(raw.count), 2, 5, p(keys), 1, 0, 0, p(one), p(one), None) == _lib.MST_E_ARG
    assert b"count_kind 2" in lib.mst_last_error()
    assert lib.mst_pileup_centre_counts(p(raw.x), p(raw.dist), p(raw.count), 1, 5, p(keys), 1, 5, 4, p(one), p(one), None) == _lib.MST_E_ARG
    assert b"distance range [5, 4]" in lib.mst_last_error()
    assert lib.mst_pileup_centre_counts(None, p(raw.dist), p(raw.count), 1, 5, p(keys), 1, 0, 4, p(one), p(one), None) == _lib.MST_E_ARG
    assert lib.mst_pileup_poisson(None, None, None, None, None, 0, None, None, 0, None, None, None, None, None, None) == _lib.MST_OK
    assert lib.mst_pileup_poisson(None, None, None, None, None, 5, None, None, 2, None, None, None, None, None, None) == _lib.MST_E_ARG
    assert b"mst_pileup_poisson: bad argument" in lib.mst_last_error()
    torch.cuda.synchronize()


# ---- the tail ---------------------------------------------------------------------------------------------------------------
def test_the_tail_kernel_against_scipy_and_the_restatement():
    import torch
    from scipy.special import gammainc
    from mustache_amd.pileup import poisson_windows
    nan = math.nan
    cases = grid() + [(0, 3.5), (0, 0.0), (1, 0.0), (300, 0.0), (0, nan), (7, nan), (7, math.inf), (1, 1.0), (5, 5.0),
                      (5, math.nextafter(5.0, 6.0)), (2 ** 24, 2.0 ** 24), (2 ** 24, math.nextafter(2.0 ** 24, 2.0 ** 25))]
    L = len(cases)
    c = np.array([k for k, _ in cases], np.int64)
    lam = np.array([v for _, v in cases], np.float64)
    # EXP = 1 * S_o / 1 = lambda with S_o = lambda, and both bias values 1: the kernel's LAMBDA is the grid's, to the bit
    sums = np.zeros((L, 4, 3))
    sums[:, :, 0], sums[:, :, 1], sums[:, :, 2] = lam[:, None], 1.0, 1.0
    one = torch.ones(L, dtype=torch.float64, device="cuda")
    at = torch.zeros(L, dtype=torch.int64, device="cuda")
    out, unconverged = poisson_windows(torch.from_numpy(sums).cuda(), one, one, torch.from_numpy(c).cuda(),
                                       torch.ones(1, dtype=torch.float64, device="cuda"), at, at)
    out = out.cpu().numpy()
    assert int(unconverged.item()) == 0                                   # c = lambda = 2^24 converges under the cap
    assert _same_numbers(out[2], np.repeat(lam[:, None], 4, 1)) and _same_numbers(out[0], out[2])
    p = out[3]
    for k in range(1, 4):
        assert _same_numbers(p[:, k], p[:, 0])                            # the neighbourhood does not enter
    worst_scipy = worst_ref = 0.0
    for i, (k, v) in enumerate(cases):
        want = ref.poisson_tail(k, v)
        if math.isnan(want):
            assert math.isnan(p[i, 0]), (k, v)
            continue
        assert not math.isnan(p[i, 0]), (k, v)
        if k == 0 or v == 0.0 or v == math.inf:
            assert p[i, 0] == want, (k, v)                                # the edge rules are exact
            continue
        if k == 2 ** 24:                                                  # beyond the grid: convergence only (error ~ c * 2^-53)
            assert abs(p[i, 0] - 0.5) < 1e-3
            continue
        worst_scipy = max(worst_scipy, check_tail(p[i, 0], float(gammainc(k, v))))
        worst_ref = max(worst_ref, check_tail(p[i, 0], want, tol=2e-9))   # two values within 1e-9 of SciPy each
    print("device tail: worst relative distance from SciPy %.3g, from the restatement %.3g, %d cases"
          % (worst_scipy, worst_ref, L))


# ---- pileup_band with poisson= on the enrichment test's band and loops -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _counts_and_bias(w):
    """The enrichment test's band taken as the raw map: integer counts C = ceil(B) (0 where B is 0), a bias vector with NaN on
    the invalid bins, one bin below 0.2 and one at 0.2 exactly, and the balanced band (C / b[x]) / b[y] -- what
    balance_records_device leaves: a pixel at a bin whose bias is NaN or < 0.2 is gone, its raw record is not."""
    import torch
    B, D = ge._band(w)
    C = torch.ceil(B)
    rng = np.random.default_rng(5 + w)
    bias = rng.uniform(0.5, 1.5, ge.N)
    bias[list(ge.BAD_BINS)] = np.nan
    bias[40], bias[41] = 0.19, 0.2
    b = torch.from_numpy(np.where(np.isnan(bias) | (bias < 0.2), np.inf, bias))
    band = torch.zeros_like(B)
    for d in range(D + 2):
        m = ge.N - d
        band[d, :m] = (C[d, :m] / b[:m]) / b[d:d + m]
    dd, xx = torch.nonzero(C, as_tuple=True)
    return band.contiguous(), D, bias, xx.to(torch.int32), dd.to(torch.int32), C[dd, xx].contiguous()


def _loops():
    xs, ys = ge._loops()
    xs, ys = xs.copy(), ys.copy()
    # bias < 0.2, = 0.2, a partner below 0.2, the diagonal, and more loops at the bin the balancing dropped
    xs[10:18], ys[10:18] = [40, 41, 20, 41, 40, 40, 35, 40], [70, 71, 40, 41, 50, 60, 40, 45]
    return xs, ys


AT_DROPPED_BIN = (10, 12, 14, 15, 16, 17)


def _run(w, p, xs, ys, kind="float32"):
    import torch
    from mustache_amd.pileup import PoissonInput, pileup_band
    band, D, bias, x, d, c = _counts_and_bias(w)
    count = c.to(torch.float32) if kind == "float32" else c.to(torch.int64)
    raw = PoissonInput(x.cuda(), d.cuda(), count.cuda(), bias)
    r = pileup_band(band.cuda(), ge.N, D, xs, ys, w, 1, peak=p, poisson=raw)
    E = r["expected"].cpu().numpy()
    return {k: v for k, v in r.items() if k not in ("obs", "oe", "valid", "expected")}, E


@functools.lru_cache(maxsize=None)
def _case(w, p):
    """the 1000 loops once per (w, p): the device's result and the restatement on the device's own E"""
    xs, ys = _loops()
    r, E = _run(w, p, xs, ys)
    band, D, bias, x, d, c = _counts_and_bias(w)
    obs = np.concatenate([pr.windows(band.numpy(), ge.N, D, E, xs[i:i + 250], ys[i:i + 250], w)[0] for i in range(0, len(xs), 250)])
    sums = er.cis_sums(obs, w, p, E, D, xs, ys)
    exp, _fe, _fe_min = er.ratios(sums, obs[:, w, w], E[ys - xs])
    counts = ref.centre_counts(x.numpy(), d.numpy(), c.numpy(), xs, ys)
    return r, {"counts": counts, "sig": ref.significance(exp, counts, bias, xs, ys), "bias": bias}


@pytest.mark.parametrize("L", [1, 3, 4, 5, 1000])
@pytest.mark.parametrize("w,p", [(1, 0), (10, 2), (64, 63)])
def test_pileup_band_against_the_restatement(w, p, L):
    from mustache_amd.pileup import enrichment
    full, want = _case(w, p)
    xs, ys = (a[:L] for a in _loops())
    r, _E = _run(w, p, xs, ys)
    b1, b2, lam, pv, p_max = (a[:L] for a in want["sig"])
    assert r["raw_center"].dtype == np.int64 and r["raw_center"].tolist() == want["counts"][:L].tolist()
    assert _same_numbers(r["bias1"], b1) and _same_numbers(r["bias2"], b2) and r["poisson_unconverged"] == 0
    # EXP and FE: the bits of the host function on the device's own sums
    exp, fe, fe_min = enrichment(r["enrich_sums"], r["center_obs"], r["center_e"])
    assert _same_numbers(r["enrich_exp"], exp) and _same_numbers(r["enrich_fe"], fe) and _same_numbers(r["fe_min"], fe_min)
    # LAMBDA: the bits of (EXP * b1) * b2 on those, the restatement's NaN positions, and its values within the enrichment bound
    usable = ~np.isnan(b1) & (b1 >= 0.2) & ~np.isnan(b2) & (b2 >= 0.2)
    with np.errstate(invalid="ignore"):
        assert _same_numbers(r["poisson_lambda"], np.where(usable[:, None], (exp * b1[:, None]) * b2[:, None], np.nan))
    ge._within(r["poisson_lambda"], lam, ge._bound(w))
    # P: the restatement's NaN positions; within 1e-9 of the restatement at the device's LAMBDA
    assert np.array_equal(np.isnan(r["poisson_p"]), np.isnan(pv)) and np.array_equal(np.isnan(r["p_max"]), np.isnan(p_max))
    for l in range(L):
        for k in range(4):
            if not math.isnan(pv[l, k]):
                check_tail(r["poisson_p"][l, k], ref.poisson_tail(r["raw_center"][l], r["poisson_lambda"][l, k]))
    assert _same_numbers(r["p_max"], _p_max(r["poisson_p"]))
    # the independent cross-check: four roundings of 2^-53 each stay under one half below 2^50
    with np.errstate(invalid="ignore"):
        back = np.rint(r["center_obs"] * r["bias1"] * r["bias2"])
    assert (r["raw_center"][usable] == back[usable]).all()
    # a loop's numbers do not depend on L or on where it sits; int64 counts give what float32 counts give
    for key in POISSON_KEYS[:-1]:
        assert _same_numbers(r[key], full[key][:L]), key
    back_r, _ = _run(w, p, xs[::-1].copy(), ys[::-1].copy(), kind="int64")
    for key in POISSON_KEYS[:-1] + ("enrich_exp", "enrich_fe"):
        assert _same_numbers(back_r[key][::-1], r[key]), key
    if L == 1000:                                                         # the placements do what they are there for
        assert np.isnan(lam[10]).all() and not np.isnan(lam[11]).all() and np.isnan(lam[12]).all()
        assert all(math.isnan(p_max[i]) for i in AT_DROPPED_BIN)
        assert any(want["counts"][i] > 0 for i in AT_DROPPED_BIN)         # a raw count at a bin the balancing dropped
        assert (want["counts"] == 0).sum() > 100 and (pv[want["counts"] == 0][~np.isnan(pv[want["counts"] == 0])] == 1.0).all()
        assert (~np.isnan(p_max)).sum() > 300 and np.isnan(p_max).sum() > 10 and usable.sum() > 900
        if w < 64:
            assert (p_max[~np.isnan(p_max)] < 0.5).any()


def test_without_the_keyword_nothing_is_launched_and_no_key_is_added(monkeypatch):
    from mustache_amd import _lib
    from mustache_amd.pileup import pileup_band
    lib = _lib.load()
    calls = []
    for name in ("mst_pileup_centre_counts", "mst_pileup_poisson"):
        bound_fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _f=bound_fn, _n=name: (calls.append(_n), _f(*a))[1])
    band, D, _bias, _x, _d, _c = _counts_and_bias(10)
    xs, ys = (a[:20] for a in _loops())
    plain = pileup_band(band.cuda(), ge.N, D, xs, ys, 10, 1)              # q = 1, as _run
    peak = pileup_band(band.cuda(), ge.N, D, xs, ys, 10, 1, peak=2)
    assert calls == [] and not set(POISSON_KEYS) & (set(plain) | set(peak))
    assert set(peak) - set(plain) == set(ge.ENRICH_KEYS)
    got, _E = _run(10, 2, xs, ys)
    assert calls == ["mst_pileup_centre_counts", "mst_pileup_poisson"]
    assert set(got) - {"obs", "oe", "valid", "expected"} == (set(peak) - {"obs", "oe", "valid", "expected"}) | set(POISSON_KEYS)
    for key in ("sum_oe", "p2ll", "center_obs", "enrich_sums", "enrich_exp", "enrich_fe", "fe_min", "enrich_agg"):
        assert _same_numbers(got[key], peak[key]), key                    # what the run without the keyword gives, to the bit
    from mustache_amd.pileup import PoissonInput
    e = pileup_band(band.cuda(), ge.N, D, [], [], 10, 6, peak=2, poisson=PoissonInput(None, None, None, None))      # L = 0: no launch
    assert e["raw_center"].shape == (0,) and e["poisson_p"].shape == (0, 4) and len(calls) == 2


# ---- the command line --------------------------------------------------------------------------------------------------------
HEADER = ge.HEADER
RES, W, PEAK, T = 10000, 10, 2, 0.1
SIZES = {"chr1": 500, "chr2": 300}


def _map(n, seed):
    from mustache_amd.synth import synth_coo
    x, y, v = synth_coo(n, 90, depth=100.0, seed=seed, nloops=20)
    return np.asarray(x, np.int64), np.asarray(y, np.int64), np.maximum(np.round(np.asarray(v)), 1.0).astype(np.int64)


def _write_pairs(path, maps, seed):
    """one row per contact: a random position inside each bin (1-based), either orientation, shuffled"""
    rng = np.random.default_rng(seed)
    head = "## pairs format v1.0\n" + "".join("#chromsize: %s %d\n" % (c, SIZES[c] * RES) for c in maps) + \
           "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
    names, p1, p2 = [], [], []
    for c, (x, y, v) in maps.items():
        bx, by = np.repeat(x, v), np.repeat(y, v)
        a = bx * RES + rng.integers(1, RES + 1, len(bx))
        b = by * RES + rng.integers(1, RES + 1, len(by))
        swap = rng.random(len(a)) < 0.5
        p1.append(np.where(swap, b, a))
        p2.append(np.where(swap, a, b))
        names.append(np.full(len(a), c))
    names, p1, p2 = np.concatenate(names), np.concatenate(p1), np.concatenate(p2)
    order = rng.permutation(len(p1))
    with open(path, "w") as f:
        f.write(head + "".join("r\t%s\t%d\t%s\t%d\t+\t-\n" % (c, a, c, b)
                               for c, a, b in zip(names[order].tolist(), p1[order].tolist(), p2[order].tolist())))


def _write_hic(path, maps, fraction=None):
    from hic_writer import write_hic
    chroms = [("All", 1000)] + [(c, SIZES[c] * RES) for c in maps]
    mats = {}
    for i, (x, y, v) in enumerate(maps.values()):
        v = v.astype(np.float64)
        if fraction is not None:
            v[fraction] += 0.5
        mats[i + 1] = {RES: (x, y, v)}
    write_hic(path, chroms, mats, {}, version=8, block_bin_count=200, float_counts=True)


def _loop_rows(maps, seed, per_chrom):
    """loop rows on every chromosome of `maps` (named without the chr prefix), some on planted pixels of high count, both ends"""
    rng = np.random.default_rng(seed)
    rows, bins = [], []
    for c, (x, y, v) in maps.items():
        n = SIZES[c]
        sep = rng.integers(30, 66, per_chrom)
        xs = rng.integers(0, n - 10 - sep)
        xs[0], xs[1] = 0, n - 10 - sep[1]
        ys = xs + sep
        far = np.flatnonzero((y - x >= 30) & (y - x <= 65))
        top = far[np.argsort(v[far])[-per_chrom // 3:]]                   # the strongest far pixels: loops that should pass
        xs[2:2 + len(top)], ys[2:2 + len(top)] = x[top], y[top]
        for k, (a, b) in enumerate(zip(xs, ys)):
            rows.append("%s\t%d\t%d\t%s\t%d\t%d\t0.0%d\t1.6" % (c[3:], a * RES, (a + 1) * RES, c[3:], b * RES, (b + 1) * RES, k % 7))
            bins.append((c, int(a), int(b)))
    return rows, bins


def _restate(maps, bins, method="NEWTON"):
    """(per used loop: counts, b1, b2, lam, p, p_max) of the restatement, the chromosomes in order; the bias is balance.solve's
    on the raw map, the band what the bias leaves of it"""
    from mustache_amd.balance import solve
    out = []
    for c, (x, y, v) in maps.items():
        mine = [(a, b) for cc, a, b in bins if cc == c]
        xs, ys = np.array([a for a, _ in mine], np.int64), np.array([b for _, b in mine], np.int64)
        n = int(y.max()) + 1
        bias, _info = solve(method, x, y, v.astype(np.float64), n)
        f = np.where(np.isnan(bias) | (bias < 0.2), np.inf, bias)
        bal = (v / f[x]) / f[y]
        D = int((ys - xs).max()) + 2 * W
        keep = (bal > 0) & (y - x <= D)
        nn = int(y[keep].max()) + 1
        B = np.zeros((D + 2, nn))
        B[(y - x)[keep], x[keep]] = bal[keep]
        want = pr.pileup_band(B[:D + 1], nn, D, xs, ys, W, 6)
        sums = er.cis_sums(want["obs"], W, PEAK, want["expected"], D, xs, ys)
        exp, _fe, _m = er.ratios(sums, want["center_obs"], want["expected"][ys - xs])
        counts = ref.centre_counts(x, y - x, v, xs, ys)
        out.append((counts,) + ref.significance(exp, counts, bias, xs, ys) + (nn,))
    return out


def _files(prefix):
    d, base = os.path.dirname(prefix), os.path.basename(prefix)
    return sorted(f[len(base):] for f in os.listdir(d) if f.startswith(base + "."))


def _cli(f, loops, prefix, *extra):
    from mustache_amd.pileup import main
    main(["-f", f, "-l", loops, "-r", str(RES), "-o", prefix, "--balance", "NEWTON", "--enrich"] + list(extra))


SIX = [".apa.tsv", ".enrich.stats.tsv", ".enrich.tsv", ".loops.tsv", ".oe.tsv", ".stats.tsv"]


def _check_table(path, rows, restated, n_chrom_bound):
    """poisson.tsv against the restatement; returns (the body's fields, the used ones, their numbers)"""
    from mustache_amd.pileup import POISSON_COLUMNS
    lines = open(path).read().splitlines()
    assert lines[0] == HEADER + "\t" + "\t".join(POISSON_COLUMNS)
    body = [ln.split("\t") for ln in lines[1:]]
    assert ["\t".join(f[:8]) for f in body] == rows                       # the rows as read, in input order
    assert all(len(f) == 8 + len(POISSON_COLUMNS) for f in body)
    used = [f for f in body if f[8] == "used"]
    for f in body:
        if f[8] != "used":
            assert all(s == "nan" for s in f[9:]), f
    got = np.array([[float(s) for s in f[9:]] for f in used])
    counts = np.concatenate([r[0] for r in restated])
    b1, b2, lam, p, p_max = (np.concatenate([r[k] for r in restated]) for k in range(1, 6))
    assert len(got) == len(counts)
    assert got[:, 0].tolist() == counts.astype(np.float64).tolist()       # RAW_CENTER: exact
    assert _same_numbers(got[:, 1], b1) and _same_numbers(got[:, 2], b2)  # the bias solve() returned, to the bit
    rel = ge._bound(W) + 4.0 * n_chrom_bound * 2.0 ** -53                 # the enrichment CLI test's bound: E in two orders
    ge._within(got[:, 3:7], lam, rel)
    assert np.array_equal(np.isnan(got[:, 7:11]), np.isnan(p)) and np.array_equal(np.isnan(got[:, 11]), np.isnan(p_max))
    for l in range(len(got)):
        for k in range(4):
            if not math.isnan(p[l, k]):
                check_tail(got[l, 7 + k], ref.poisson_tail(counts[l], got[l, 3 + k]))
    assert _same_numbers(got[:, 11], _p_max(got[:, 7:11]))
    q, q_max = ref.q_values(got[:, 7:11])                                 # BH over the WHOLE run's used loops, on P as written
    ge._within(got[:, 12:16], q, 1e-15)
    ge._within(got[:, 16], q_max, 1e-15)
    return body, used, got


@pytest.fixture(scope="module")
def one(tmp_path_factory):
    d = tmp_path_factory.mktemp("pileup_poisson_one")
    maps = {"chr1": _map(SIZES["chr1"], 9)}
    rows, bins = _loop_rows(maps, 4, 60)
    rows.insert(3, "1\t1000000\t1010000\t1\t1050000\t1060000\t0.01\t1.6")               # short: 5 bins apart
    rows.insert(7, "1\t1000000\t1010000\t2\t2000000\t2010000\t0.01\t1.6")               # trans
    out = {"dir": d, "maps": maps, "rows": rows, "bins": bins, "pairs": str(d / "m.pairs"), "hic": str(d / "m.hic"),
           "loops": str(d / "l.tsv")}
    _write_pairs(out["pairs"], maps, 7)
    _write_hic(out["hic"], maps)
    with open(out["loops"], "w") as fh:
        fh.write(HEADER + "\n" + "".join(r + "\n" for r in rows))
    return out


def test_cli_end_to_end_from_a_hic_and_a_pairs_file(one, capsys):
    d = one["dir"]
    restated = _restate(one["maps"], one["bins"])
    texts = {}
    for kind in ("hic", "pairs"):
        old, new = str(d / (kind + "_old")), str(d / (kind + "_new"))
        _cli(one[kind], one["loops"], old)
        _cli(one[kind], one["loops"], new, "--poisson", "--max-fdr", str(T))
        said = capsys.readouterr().out
        assert "Error" not in said
        assert _files(old) == SIX and _files(new) == sorted(SIX + [".poisson.tsv", ".significant.tsv"])
        for ext in SIX:                                                   # byte for byte what the run without --poisson writes
            assert open(old + ext, "rb").read() == open(new + ext, "rb").read(), (kind, ext)
        body, used, got = _check_table(new + ".poisson.tsv", one["rows"], restated, restated[0][6])
        assert [f[8] for f in body[3:8:4]] == ["short", "trans"] and len(used) == len(one["bins"])
        # the filtered list: exactly the used rows the restatement selects, unchanged and in input order
        _q, q_max = ref.q_values(got[:, 7:11])
        kept = open(new + ".significant.tsv").read().splitlines()
        assert kept[0] == HEADER
        with np.errstate(invalid="ignore"):
            assert kept[1:] == ["\t".join(f[:8]) for f, qm in zip(used, q_max) if qm <= T]
            assert kept[1:] == ["\t".join(f[:8]) for f in used if float(f[25]) <= T]
        assert 0 < len(kept) - 1 < len(used)
        line = [ln for ln in said.splitlines() if ln.startswith("significance of")]
        assert len(line) == 1 and line[0].startswith("significance of %d used loops: %d with a defined P_MAX, %d with Q_MAX <= %r"
                                                     % (len(used), (~np.isnan(got[:, 11])).sum(), len(kept) - 1, T))
        texts[kind] = (open(new + ".poisson.tsv", "rb").read(), open(new + ".significant.tsv", "rb").read())
    assert texts["hic"] == texts["pairs"]                                 # whichever reader the raw counts came from


def test_q_is_taken_over_the_whole_run(tmp_path, capsys):
    maps = {"chr1": _map(SIZES["chr1"], 9), "chr2": _map(SIZES["chr2"], 10)}
    rows, bins = _loop_rows(maps, 6, 30)
    hic, loops, prefix = str(tmp_path / "two.hic"), str(tmp_path / "l.tsv"), str(tmp_path / "two")
    _write_hic(hic, maps)
    with open(loops, "w") as fh:
        fh.write(HEADER + "\n" + "".join(r + "\n" for r in rows))
    _cli(hic, loops, prefix, "--poisson")
    assert "Error" not in capsys.readouterr().out and ".significant.tsv" not in _files(prefix)
    restated = _restate(maps, bins)
    _body, used, got = _check_table(prefix + ".poisson.tsv", rows, restated, max(r[6] for r in restated))      # Q over all 60 loops
    first = [f[0] == "1" for f in used]
    assert sum(first) == 30 and len(used) == 60
    per_chrom = ref.q_values(got[first, 7:11])[0]                         # BH over chromosome 1 alone: not what is written
    ok = ~np.isnan(per_chrom) & (got[first, 12:16] < 1.0)
    assert ok.any() and (got[first, 12:16][ok] != per_chrom[ok]).any()


def test_a_hic_file_with_a_fractional_count_ends_the_run_with_one_error_line(tmp_path, capsys):
    maps = {"chr1": _map(SIZES["chr1"], 9)}
    rows, _bins = _loop_rows(maps, 4, 20)
    for sep in (30, 65):                                                  # the list's distance range holds [30, 65] whatever was drawn
        rows.append("1\t%d\t%d\t1\t%d\t%d\t0.01\t1.6" % (100 * RES, 101 * RES, (100 + sep) * RES, (101 + sep) * RES))
    x, y, _v = maps["chr1"]
    k = int(np.flatnonzero(y - x == 45)[0])                               # a pixel inside that range, named by no loop or by one
    hic, loops, prefix = str(tmp_path / "f.hic"), str(tmp_path / "l.tsv"), str(tmp_path / "out")
    _write_hic(hic, maps, fraction=k)
    with open(loops, "w") as fh:
        fh.write(HEADER + "\n" + "".join(r + "\n" for r in rows))
    _cli(hic, loops, prefix, "--poisson")
    said = capsys.readouterr().out.splitlines()
    errors = [ln for ln in said if ln.startswith("Error:")]
    assert len(errors) == 1 and "chromosome 1 holds a count that is not an integer value" in errors[0], said
    assert _files(prefix) == []
