"""The two-sample path's own device pieces through the C ABI, against float64 / extended-precision references:

  mst_diff_dog_band          the DoG of the difference image straight from the two bands, at each of its three tile
                             instantiations (largest sigma_2 / sigma_3 blur radius <= 8, 9-14, 15-28), against SciPy's
                             gaussian_filter of the reference's difference image (diff_mustache.py:262-276, :315-336): bit-identical
                             on every pixel a found record can address, tested-pixel counts exact, norm.fit (:371) against the
                             exact two-pass value; the dense route (mst_diff_image, mst_gauss_blur, mst_masked_normfit) on the
                             same cases
  mst_pair_pvalues(_dog)     the pair p-value (:372-385) on a z grid through both tails, the erf / erfc switch and the non-finite
                             cases, against mpmath; the level -> octave map, the second sample's rows and the overflow guard
  degenerate pairs           identical samples (scale 0) and disjoint supports (nothing tested in both: norm.fit of nothing)
                             end to end against the oracle's restatement of diff_mustache()
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_reference as pr      # noqa: E402
import radius_sweep as rs        # noqa: E402

pytestmark = pytest.mark.gpu

OCTAVE_LISTS = ([1.6, 3.2], [2.0, 4.0], [5.0], [3.2, 6.4], [1.6, 3.2, 6.4])
TILE_RADII = {8: (1, 8), 14: (9, 14), 28: (15, 28)}      # DiffTile8 / DiffTile14 / DiffTile28 of mst_diff.hip
WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _diff_radius(octaves):
    from mustache_amd.levels import LevelTable
    lt = LevelTable(octaves)
    lpo = lt.levels_per_octave
    return max(lt.radius[o * lpo + q] for o in range(len(octaves)) for q in (1, 2))


def _tile_of(radius):
    return next(t for t, (lo, hi) in TILE_RADII.items() if lo <= radius <= hi)


def test_octave_lists_cover_every_tile():
    tiles = {}
    for octs in OCTAVE_LISTS:
        tiles.setdefault(_tile_of(_diff_radius(octs)), []).append(octs)
    print("tile per octave list:", {t: v for t, v in sorted(tiles.items())})
    assert set(tiles) == set(TILE_RADII), tiles
    # and with the sweep lists every radius each tile is built for: one diff_blur<T, R> per (tile, radius) pair
    assert tuple(OCTAVE_LISTS) == tuple(rs.DIFF_BASE_LISTS)
    for octs in OCTAVE_LISTS:
        assert rs.diff_tile(rs.DiffLevels(octs)) == _tile_of(_diff_radius(octs)), octs
    wit = rs.diff_witnesses()
    print("witness of every (tile, radius):", {k: v for k, v in sorted(wit.items())})
    assert sorted(wit) == [(t, r) for t in sorted(TILE_RADII) for r in range(1, t + 1)] and len(wit) == 50


# ---- A: mst_diff_dog_band -----------------------------------------------------------------------------------------------
def _samples(n, dpx, seed, pattern=False):
    """two full upper-band matrices [n, n] (offsets 0 .. dpx + 1) of different depth and seed; `pattern`: pixels set in one
    sample only and rows where one sample is empty"""
    from mustache_amd.synth import synth_coo
    rng = np.random.default_rng(seed)
    out = []
    for k, depth in enumerate((300.0, 170.0)):
        x, y, v = synth_coo(n, max(dpx, 1), depth=depth, seed=seed * 10 + k, nloops=max(n // 30, 2))
        keep = (y - x >= 0) & (y - x <= dpx + 1)
        c = np.zeros((n, n))
        c[x[keep], y[keep]] = v[keep] * rng.uniform(0.5, 2.0, int(keep.sum()))     # not integers: every rounding shows
        out.append(c)
    if pattern:
        c1, c2 = out
        off = np.arange(n)[None, :] - np.arange(n)[:, None]
        band = (off >= 0) & (off <= dpx + 1)
        drop = band & (rng.random((n, n)) < 0.2)
        c2[drop] = 0.0                                            # set in sample 1 only
        only2 = band & (c1 == 0) & (rng.random((n, n)) < 0.3)
        c2[only2] = rng.uniform(0.1, 3.0, int(only2.sum()))       # set in sample 2 only
        rows = rng.choice(n, size=max(n // 10, 2), replace=False)
        c2[rows[: len(rows) // 2]] = 0.0                          # rows empty in one sample
        c1[rows[len(rows) // 2:]] = 0.0
    return out


def _band(c, n, dpx):
    import torch
    b = np.zeros((dpx + 2, n))
    for off in range(dpx + 2):
        if off < n:
            b[off, : n - off] = np.diagonal(c, off)
    return torch.from_numpy(b).cuda()


def _block(c, n, start, CH):
    """the dense block at `start`, zero past n (what the reference's dense block holds)"""
    cb = np.zeros((CH, CH))
    m = max(0, min(CH, n - start))
    cb[:m, :m] = c[start:start + m, start:start + m]
    return cb


def _reference(cb1, cb2, dpx, octaves, lt=None):
    """diff_mustache.py:262-276 then D = G(sigma_2) - G(sigma_3) per octave (:315-336), float64 SciPy"""
    import oracle
    from mustache_amd.levels import LevelTable
    CH = cb1.shape[0]
    off = np.arange(CH)[None, :] - np.arange(CH)[:, None]
    nzb = (cb1 != 0) & (off >= 4) & (cb2 != 0)
    f1, f2 = cb1.copy(), cb2.copy()
    for f in (f1, f2):
        f[off <= 4] = 2
        f[off >= dpx + 1] = 2
    cd = np.zeros((CH, CH))
    cd[nzb] = f1[nzb] - f2[nzb]
    lt = LevelTable(octaves) if lt is None else lt
    lpo = lt.levels_per_octave
    D = np.stack([oracle.blur_scipy(cd, lt.sigma[o * lpo + 1], lt.truncate[o * lpo + 1]) -
                  oracle.blur_scipy(cd, lt.sigma[o * lpo + 2], lt.truncate[o * lpo + 2]) for o in range(len(octaves))])
    return cd, nzb, D


def _launch_band(eng, bands, n, dpx, starts, CH, lt=None):
    """lt: a level table of its own (radius_sweep.DiffLevels) instead of the engine's"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    B, n_oct = len(starts), len((eng.levels if lt is None else lt).octave_values)
    lv_struct = eng._lv_struct if lt is None else lt.as_struct()
    lv = ctypes.byref(lv_struct)
    dog = torch.full((n_oct, B, CH, CH), float("nan"), dtype=torch.float64, device="cuda")
    fit = torch.full((n_oct, B, 2), float("nan"), dtype=torch.float64, device="cuda")
    cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    wsb = int(eng.lib.mst_diff_dog_workspace_bytes(B, CH, lv))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    st = (ctypes.c_int64 * B)(*starts)
    _lib.check(eng.lib.mst_diff_dog_band(_ptr(bands[0]), _ptr(bands[1]), n, dpx, st, B, CH, lv, _ptr(dog), _ptr(fit), _ptr(cnt),
                                         _ptr(ws), wsb, _stream()))
    return dog, fit, cnt, (ws, st, lv_struct)


def _check_fit(got, vals, what):
    """norm.fit from the device against the exact two-pass value of the reference's masked DoG values"""
    loc_x, scale_x = pr.exact_normfit(vals)
    if vals.size == 0:
        assert np.isnan(got).all(), (what, got)
        return
    el, es = pr.fit_errors(got[0], got[1], loc_x, scale_x)
    _note("fit loc / scale*", el)
    _note("fit scale / scale*", es)
    assert el <= pr.LOC_BOUND and es <= pr.SCALE_BOUND, (what, got, (loc_x, scale_x), el, es)


def _check_case(eng, octaves, case, results, lt=None):
    """results = (dog, fit, cnt) of mst_diff_dog_band for case = (c1, c2, n, dpx, starts, CH)"""
    c1, c2, n, dpx, starts, CH = case
    dog, fit, cnt = (t.cpu().numpy() for t in results)
    off = np.arange(CH)[None, :] - np.arange(CH)[:, None]
    addr = (off >= 4) & (off <= dpx + 1)          # every pixel a found record can address
    for b, s in enumerate(starts):
        cd, nzb, D = _reference(_block(c1, n, s, CH), _block(c2, n, s, CH), dpx, octaves, lt)
        what = (octaves, n, dpx, CH, s)
        assert int(cnt[b]) == int(nzb.sum()), what
        for o in range(len(octaves)):
            g = dog[o, b][addr]
            assert np.array_equal(g, D[o][addr]), (what, o, int((g != D[o][addr]).sum()),
                                                   float(np.nanmax(np.abs(g - D[o][addr]))))
            _check_fit(fit[o, b], D[o][nzb], (what, o))
    return cnt


def _dense_route(eng, case, octaves, band_dog, lt=None):
    """mst_diff_image -> mst_gauss_blur at sigma_2 / sigma_3 -> mst_masked_normfit on the same blocks: the same difference
    image, G_2 - G_3 bit-identical to the band route's DoG on the addressable pixels, norm.fit within the same bounds"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    c1, c2, n, dpx, starts, CH = case
    B = len(starts)
    raw = np.stack([_block(c1, n, s, CH) for s in starts] + [_block(c2, n, s, CH) for s in starts])
    c = torch.from_numpy(raw.copy()).cuda()
    nz, _ = eng.prologue(c, dpx, True)
    cd = torch.empty((B, CH, CH), dtype=torch.float64, device="cuda")
    nzb = torch.empty((B, CH, CH), dtype=torch.uint8, device="cuda")
    nzbc = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _lib.check(eng.lib.mst_diff_image(_ptr(c[:B]), _ptr(c[B:]), _ptr(nz[:B]), _ptr(nz[B:]), B, CH, _ptr(cd), _ptr(nzb), _ptr(nzbc),
                                      _stream()))
    lt = eng.levels if lt is None else lt
    lpo = lt.levels_per_octave
    ws = torch.empty(2048 * B, dtype=torch.uint8, device="cuda")
    off = np.arange(CH)[None, :] - np.arange(CH)[:, None]
    addr = (off >= 4) & (off <= dpx + 1)
    for o in range(len(octaves)):
        g2 = eng.gauss_blur(cd, lt.taps[o * lpo + 1])
        g3 = eng.gauss_blur(cd, lt.taps[o * lpo + 2])
        fit = torch.full((B, 2), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(eng.lib.mst_masked_normfit(_ptr(g2), _ptr(g3), _ptr(nzb), _ptr(nzbc), B, CH * CH, _ptr(fit), _ptr(ws), ws.numel(),
                                              _stream()))
        d = (g2 - g3).cpu().numpy()
        fit = fit.cpu().numpy()
        for b, s in enumerate(starts):
            ref_cd, ref_nzb, D = _reference(raw[b], raw[B + b], dpx, octaves, lt)
            if o == 0:
                assert np.array_equal(nzb[b].cpu().numpy().astype(bool), ref_nzb)
                assert int(nzbc[b]) == int(ref_nzb.sum())
                assert np.array_equal(cd[b].cpu().numpy(), ref_cd)
            assert np.array_equal(d[b][addr], band_dog[o, b][addr]), (octaves, CH, dpx, s, o)
            _check_fit(fit[b], D[o][ref_nzb], ("dense", octaves, CH, dpx, s, o))


def _cases():
    """(c1, c2, n, dpx, starts, CH): inner and reflected-border tiles at every instantiation, a block smaller than the blur
    radius, a band narrower than one halo, the whole upper triangle in the band, overlapping blocks that run past n"""
    cases = []
    c1, c2 = _samples(333, 100, 1)
    cases.append((c1, c2, 333, 100, [0], 333))
    c1, c2 = _samples(333, 6, 2, pattern=True)
    cases.append((c1, c2, 333, 6, [0], 333))
    c1, c2 = _samples(64, 40, 3, pattern=True)
    cases.append((c1, c2, 64, 40, [0], 64))
    c1, c2 = _samples(65, 64, 4)
    cases.append((c1, c2, 65, 64, [0], 65))
    c1, c2 = _samples(20, 19, 5, pattern=True)
    cases.append((c1, c2, 20, 19, [0], 20))
    c1, c2 = _samples(17, 6, 6)
    cases.append((c1, c2, 17, 6, [0], 17))
    c1, c2 = _samples(150, 30, 7, pattern=True)
    cases.append((c1, c2, 150, 30, [0, 40, 100], 65))        # 100 + 65 > 150: the last block is zero past n
    return cases


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.mark.parametrize("octaves", OCTAVE_LISTS, ids=lambda o: ",".join(map(str, o)))
def test_diff_dog_band_every_tile_vs_scipy(octaves, cases):
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine(octaves)
    masked = 0
    for case in cases:
        c1, c2, n, dpx, starts, CH = case
        bands = [_band(c1, n, dpx), _band(c2, n, dpx)]
        dog, fit, cnt, keep = _launch_band(eng, bands, n, dpx, starts, CH)
        cnt = _check_case(eng, octaves, case, (dog, fit, cnt))
        masked += int(cnt.sum())
        _dense_route(eng, case, octaves, dog.cpu().numpy())
    assert masked > 10000
    print("worst errors so far (after %s)" % octaves, WORST)


@pytest.mark.parametrize("name", list(rs.DIFF_SWEEP))
def test_diff_dog_band_every_radius_vs_scipy(name, cases):
    """The sweep lists (radius_sweep.DIFF_SWEEP) through the checks of the test above: with them every diff_blur<T, R>,
    R = 1 .. RMAX of DiffTile8 / 14 / 28, has run and its DoG is bit-identical to SciPy's.  Their level tables go to the
    entry point directly (DiffLevels): those of the widest tile hold sigma-loop levels wider than radius 28, which the
    package refuses.  Cases: the full-size block, the block of 20 x 20 (smaller than the wider radii), the three blocks that continue
    each other."""
    from mustache_amd.engine import ScaleSpaceEngine
    octaves = rs.DIFF_SWEEP[name]
    lt = rs.DiffLevels(octaves)
    eng = ScaleSpaceEngine([1.6, 3.2])                 # the library, the prologue and mst_gauss_blur; not its levels
    masked = 0
    assert len(cases[6][4]) == 3 and cases[4][5] == 20
    for case in (cases[0], cases[4], cases[6]):
        c1, c2, n, dpx, starts, CH = case
        bands = [_band(c1, n, dpx), _band(c2, n, dpx)]
        dog, fit, cnt, keep = _launch_band(eng, bands, n, dpx, starts, CH, lt)
        cnt = _check_case(eng, octaves, case, (dog, fit, cnt), lt)
        masked += int(cnt.sum())
        _dense_route(eng, case, octaves, dog.cpu().numpy(), lt)
    assert masked > 10000
    print("diff_blur instantiations run by %s: tile %d, radii %s" % (name, rs.diff_tile(lt), sorted(set(lt.diff_radii()))))


def test_diff_dog_band_back_to_back_calls(cases):
    """two calls with different CH and dpx (different tile lists through the thread-local table and its staged upload) on one
    stream, nothing waited for between them"""
    from mustache_amd.engine import ScaleSpaceEngine
    for octaves in ([1.6, 3.2], [3.2, 6.4]):
        eng = ScaleSpaceEngine(octaves)
        a, b = cases[0], cases[6]
        ba = [_band(a[0], a[2], a[3]), _band(a[1], a[2], a[3])]
        bb = [_band(b[0], b[2], b[3]), _band(b[1], b[2], b[3])]
        ra = _launch_band(eng, ba, a[2], a[3], a[4], a[5])
        rb = _launch_band(eng, bb, b[2], b[3], b[4], b[5])
        _check_case(eng, octaves, a, ra[:3])
        _check_case(eng, octaves, b, rb[:3])


# ---- B: the pair p-value kernels ----------------------------------------------------------------------------------------
def _found(rows, cap):
    """rows: per found row a list of (pixel, level) -> device mst_found [R, cap] (int64 pairs) and counts"""
    import torch
    R = len(rows)
    rec = np.zeros((R, cap, 2), dtype=np.int64)
    cnt = np.zeros(R, dtype=np.int32)
    for r, lst in enumerate(rows):
        for i, (pix, lvl) in enumerate(lst):
            rec[r, i, 0] = np.int64(pix) | (np.int64(lvl) << 32)
            rec[r, i, 1] = np.float64(-1.0).view(np.int64)
        cnt[r] = len(lst)
    return torch.from_numpy(rec).cuda(), torch.from_numpy(cnt).cuda()


def _pvalues(eng, dense, found, count, cap, dog, g3, fit, P, CH, n_oct, tpo):
    """both offsets (sample 1 rows [0, P), sample 2 rows [P, 2P)) into a NaN-poisoned ppair"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    ppair = torch.full((2 * P, cap), float("nan"), dtype=torch.float64, device="cuda")
    for off in (0, P):
        if dense:
            rc = eng.lib.mst_pair_pvalues(_ptr(found), cap, _ptr(count), _ptr(dog), _ptr(g3), _ptr(fit), P, CH, n_oct, tpo, off,
                                          _ptr(ppair), _stream())
        else:
            rc = eng.lib.mst_pair_pvalues_dog(_ptr(found), cap, _ptr(count), _ptr(dog), _ptr(fit), P, CH, n_oct, tpo, off, _ptr(ppair),
                                              _stream())
        _lib.check(rc)
    return ppair.cpu().numpy()


def _images(x, rng, dense):
    """device images whose difference is x: (dog, None) for the band route; (g2, g3) for the dense route, g3 a small multiple of
    1/8 wherever g2 = x + g3 gives back g2 - g3 == x exactly, else 0"""
    import torch
    if not dense:
        return torch.from_numpy(x.copy()).cuda(), None
    g3 = np.where(np.isfinite(x), rng.integers(-4, 5, x.shape) * 2.0 ** -3, 0.0)
    g2 = x + g3
    with np.errstate(invalid="ignore"):
        exact = (g2 - g3 == x) | ~np.isfinite(x)
    g3[~exact] = 0.0
    g2[~exact] = x[~exact]
    return torch.from_numpy(g2).cuda(), torch.from_numpy(g3).cuda()


@pytest.mark.parametrize("dense", [False, True], ids=["dog", "g2-g3"])
def test_pair_pvalue_z_grid_vs_mpmath(dense):
    """fit (0, 1) and the DoG value = z: every z of the grid, each on both samples' rows"""
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine([1.6, 3.2])
    z = pr.z_grid()
    CH = 48
    P, n_oct, tpo = 1, 2, eng.levels.s - 1
    assert z.size <= CH * CH
    rng = np.random.default_rng(3)
    x = np.zeros((n_oct, P, CH * CH))
    x[1, 0, : z.size] = z
    fit = np.array([[[0.5, 2.0]], [[0.0, 1.0]]])
    levels = rng.integers(tpo + 1, 2 * tpo + 1, z.size)                       # octave 1
    rows = [list(zip(range(z.size), levels.tolist())), list(zip(range(z.size)[::-1], levels.tolist()))]
    cap = z.size + 3
    found, count = _found(rows, cap)
    import torch
    dog, g3 = _images(x, rng, dense)
    pp = _pvalues(eng, dense, found, count, cap, dog, g3, torch.from_numpy(fit).cuda(), P, CH, n_oct, tpo)
    exact = pr.pvalue_exact(z)
    for r, order in ((0, np.arange(z.size)), (1, np.arange(z.size)[::-1])):
        got = pp[r, : z.size]
        bad, wr, wa = pr.pvalue_check(z[order], got, exact[order])
        _note("p rel (z <= -1)", wr)
        _note("p abs (z > -1)", wa)
        assert bad.size == 0, [(z[order][i], got[i], exact[order][i]) for i in bad[:8]]
        assert np.isnan(pp[r, z.size:]).all()
    print("worst p-value errors", WORST)


@pytest.mark.parametrize("dense", [False, True], ids=["dog", "g2-g3"])
def test_pair_pvalue_degenerate_fits_give_zero(dense):
    """scale 0 with x == loc (z = NaN) and x != loc (z = +-inf), loc NaN, scale NaN: p = 0 as the reference gets it"""
    import torch
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine([1.6, 3.2, 6.4])
    CH, P, n_oct, tpo = 8, 1, 3, eng.levels.s - 1
    x = np.zeros((n_oct, P, CH * CH))
    x[:, 0, :4] = [0.3, 0.5, -7.0, 0.3]
    fit = np.array([[[0.3, 0.0]], [[np.nan, 1.0]], [[0.0, np.nan]]])
    rows = [[(p, 1 + o * tpo + k) for o in range(n_oct) for k, p in enumerate(range(4))]]
    rows = [rows[0], rows[0][::-1]]
    found, count = _found(rows, 16)
    dog, g3 = _images(x, np.random.default_rng(1), dense)
    pp = _pvalues(eng, dense, found, count, 16, dog, g3, torch.from_numpy(fit).cuda(), P, CH, n_oct, tpo)
    assert (pp[:, :12] == 0).all(), pp[:, :12]
    assert np.isnan(pp[:, 12:]).all()


@pytest.mark.parametrize("dense", [False, True], ids=["dog", "g2-g3"])
def test_pair_pvalue_octave_map_second_sample_and_overflow_guard(dense):
    """records at levels 1, tpo, tpo + 1, 2 tpo, 2 tpo + 1, 3 tpo read octave (level - 1) // tpo; rows [P, 2P) read pair
    row - P; a row whose count exceeds the capacity is left as it was, the others are written"""
    import torch
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine([1.6, 3.2, 6.4])
    CH, P, n_oct, tpo = 24, 3, 3, eng.levels.s - 1
    rng = np.random.default_rng(11)
    x = rng.normal(0.0, 1.0, (n_oct, P, CH * CH)) * np.array([1.0, 3.0, 0.2])[:, None, None]
    fit = np.stack([np.stack([[0.1 * (o + 1) * (b - 1), 0.5 + o + 0.25 * b] for b in range(P)]) for o in range(n_oct)])
    levels = [1, tpo, tpo + 1, 2 * tpo, 2 * tpo + 1, 3 * tpo]
    cap = 64
    rows = []
    for r in range(2 * P):
        pix = rng.choice(CH * CH, size=40, replace=False)
        rows.append([(int(p), levels[i % len(levels)]) for i, p in enumerate(pix)])
    found, count = _found(rows, cap)
    count[4] = cap + 1                                   # sample 2, pair 1: overflowed
    dog, g3 = _images(x, rng, dense)
    pp = _pvalues(eng, dense, found, count, cap, dog, g3, torch.from_numpy(fit).cuda(), P, CH, n_oct, tpo)
    for r in range(2 * P):
        if r == 4:
            assert np.isnan(pp[r]).all()
            continue
        b = r if r < P else r - P
        pix = np.array([p for p, _ in rows[r]])
        oct_ = (np.array([l for _, l in rows[r]]) - 1) // tpo
        assert set(oct_.tolist()) == {0, 1, 2}
        z = (x[oct_, b, pix] - fit[oct_, b, 0]) / fit[oct_, b, 1]
        bad, _, _ = pr.pvalue_check(z, pp[r, :40])
        assert bad.size == 0, (r, bad)
        assert np.isnan(pp[r, 40:]).all()
        # and no other octave / pair would have given these values
        wrong = (x[(oct_ + 1) % n_oct, (b + 1) % P, pix] - fit[(oct_ + 1) % n_oct, (b + 1) % P, 0]) / fit[(oct_ + 1) % n_oct, (b + 1) % P, 1]
        assert pr.pvalue_check(wrong, pp[r, :40])[0].size > 30


# ---- D: fixtures the reference made at the wider tiles -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["diff_320_oc2", "diff_320_sz32"])
def test_wide_tile_pairs_vs_reference_fixture(golden_dir, name):
    """the reference's diff_mustache() at octaves [2.0, 4.0] (14 tile) and [3.2, 6.4] (28 tile): dense and band-direct routes,
    found sets and winning DoG values bit-identical to the reference's locals, norm.fit within the fit bounds of the reference's,
    pair p-values within the split bounds of the exact value at the device's z (and the reference's own within them at its z),
    the four loop lists equal"""
    import torch
    from mustache_amd.diff_mustache import _pair_tail, diff_mustache
    from mustache_amd.engine import ScaleSpaceEngine
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=True)
    octs = [float(o) for o in g["octaves"]]
    n, dpx, start = int(g["n"]), int(g["dpx"]), int(g["start"])
    c1 = np.zeros((n, n)); c1[g["xa"], g["ya"]] = g["va"]
    c2 = np.zeros((n, n)); c2[g["xb"], g["yb"]] = g["vb"]
    _, nzb, D = _reference(c1, c2, dpx, octs)
    eng = ScaleSpaceEngine(octs)
    tpo = eng.levels.s - 1
    ref_fit = g["norm_fit"]
    dense = eng.run_block_pairs(torch.from_numpy(np.stack([c1, c2])).cuda(), dpx)
    band = eng.run_band_pairs([_band(c1, n, dpx), _band(c2, n, dpx)], n, dpx, [0], n)
    for o in range(len(octs)):
        loc_r, scale_r = ref_fit[o * tpo]
        loc_x, scale_x = pr.exact_normfit(D[o][nzb])
        el, es = pr.fit_errors(loc_r, scale_r, loc_x, scale_x)
        assert el <= pr.LOC_BOUND and es <= pr.SCALE_BOUND, "the reference's own norm.fit"
        for form in (dense, band):
            _check_fit(form.norm_fit[o, 0], D[o][nzb], (name, o))
    assert list(band.nz_count) == list(dense.nz_count)
    for b, nm in ((0, "1"), (1, "2")):
        f = g["loc_pPair" + nm] != 2
        ref_pair = g["loc_pPair" + nm][f]
        for form in (dense, band):
            rec = form.found[b]
            assert len(rec["pixel"]) == int(f.sum())
            assert np.array_equal(rec["value"], g["loc_vAll" + nm][f]), "winning DoG values must be bit-identical"
            oct_ = (rec["level"].astype(np.int64) - 1) // tpo
            x = np.stack(D)[oct_, rec["pixel"].astype(np.int64) // n, rec["pixel"].astype(np.int64) % n]
            z_dev = (x - form.norm_fit[oct_, 0, 0]) / form.norm_fit[oct_, 0, 1]
            bad, wr, wa = pr.pvalue_check(z_dev, rec["pair"])
            assert bad.size == 0, (name, b, bad[:5])
            _note("fixture p rel (z <= -1)", wr)
            _note("fixture p abs (z > -1)", wa)
            z_ref = (x - ref_fit[oct_ * tpo, 0]) / ref_fit[oct_ * tpo, 1]
            assert pr.pvalue_check(z_ref, ref_pair)[0].size == 0, "the reference's pair p-values at its own z"
        for k in ("pixel", "level", "value", "pval", "q"):
            assert np.array_equal(dense.found[b][k], band.found[b][k]), k
    lists = (_pair_tail(band, 0, 1, start, float(g["pt"]), float(g["pt2"]), float(g["st"]), True),
             diff_mustache(c1.copy(), c2.copy(), "1", "1", 5000, start, start + n, 0, dpx, octs, float(g["st"]), float(g["pt"]),
                           float(g["pt2"])))
    for got_lists in lists:
        for got, key in zip(got_lists, ("loops1", "diff1", "loops2", "diff2")):
            exp = g[key]
            arr = np.array([[float(a), float(b), q, s] for a, b, q, s in got]).reshape(-1, 4)
            assert arr.shape == exp.shape, key
            assert np.array_equal(arr[:, :2], exp[:, :2]) and np.array_equal(arr[:, 3], exp[:, 3]), key
            np.testing.assert_allclose(arr[:, 2], exp[:, 2], rtol=1e-7)
    assert len(g["loops1"]) >= 5 and len(g["loops2"]) >= 5
    print("worst errors so far (after %s)" % name, WORST)


# ---- C: degenerate block pairs end to end -------------------------------------------------------------------------------
def _degenerate(kind):
    import oracle
    from mustache_amd.synth import synth_coo
    n, dpx = 420, 150
    x, y, v = synth_coo(n, dpx, depth=300.0, seed=91, nloops=20)
    oracle.normalize_sparse(x, y, v, 50000, dpx)
    c1 = np.zeros((n, n))
    c1[x, y] = v
    if kind == "identical":
        c2 = c1.copy()
    else:
        x2, y2, v2 = synth_coo(n, dpx, depth=260.0, seed=92, nloops=20)
        oracle.normalize_sparse(x2, y2, v2, 50000, dpx)
        c2 = np.zeros((n, n))
        c2[x2, y2] = v2
        c1[n // 2:] = 0.0                                # sample 1 on the top rows, sample 2 on the bottom rows
        c2[: n // 2] = 0.0
    return c1, c2, n, dpx


@pytest.mark.parametrize("kind", ["identical", "disjoint"])
def test_degenerate_pairs_end_to_end_vs_oracle(kind):
    import oracle
    from mustache_amd.diff_mustache import _pair_tail, diff_mustache
    from mustache_amd.engine import ScaleSpaceEngine
    c1, c2, n, dpx = _degenerate(kind)
    start, st, pt, pt2 = 300, 0.7, 0.3, 0.3
    off = np.arange(n)[None, :] - np.arange(n)[:, None]
    t1, t2 = (c1 != 0) & (off >= 4), (c2 != 0) & (off >= 4)
    if kind == "disjoint":
        assert t1.sum() >= 10000 and t2.sum() >= 10000 and not (t1 & t2).any()
    exp, mid = oracle.diff_block(c1.copy(), c2.copy(), start, dpx, [1.6, 3.2], st, pt, pt2, return_intermediate=True)
    assert mid is not None and all(np.isnan(f[1]) or f[1] == 0 for f in mid["fits"])
    assert len(exp[0]) >= 1 and len(exp[2]) >= 1
    for k in (1, 2):
        found = mid["p"][k] != 2
        assert found.sum() > 300 and (mid["pair"][k][found] == 0).all()

    def key(lists):
        return [[(int(a), int(b), float(s)) for a, b, _, s in l] for l in lists]

    eng = ScaleSpaceEngine([1.6, 3.2])
    bands = [_band(c1, n, dpx), _band(c2, n, dpx)]
    full = eng.run_band_pairs(bands, n, dpx, [0], n)
    assert np.isnan(full.norm_fit).all() if kind == "disjoint" else (full.norm_fit[..., 1] == 0).all()
    for b in (0, 1):
        assert len(full.found[b]["pair"]) == int((mid["p"][b + 1] != 2).sum())
        assert (full.found[b]["pair"] == 0).all()
    lean = eng.run_band_pairs(bands, n, dpx, [0], n, select_below=pt)
    for b in (0, 1):
        assert len(lean.found[b]["pair"]) > 0 and (lean.found[b]["pair"] == 0).all()
    for form in (full, lean):
        got = _pair_tail(form, 0, 1, start, pt, pt2, st, True)
        assert key(got) == key(exp)
        for g, e in zip(got, exp):
            np.testing.assert_allclose([r[2] for r in g], [r[2] for r in e], rtol=1e-6)
    dense = diff_mustache(c1.copy(), c2.copy(), "1", "1", 5000, start, start + n, 0, dpx, [1.6, 3.2], st, pt, pt2)
    assert key(dense) == key(exp)
    import torch
    blk = eng.run_block_pairs(torch.from_numpy(np.stack([c1, c2])).cuda(), dpx)
    for b in (0, 1):
        assert (blk.found[b]["pair"] == 0).all()
