"""mst_diff_dog_tiles (the difference kernel with a dense source: two stacks of inter-chromosomal tiles, no band) through the C
ABI, at each of its three tile instantiations:

  D_2 per octave          bit-identical on EVERY pixel to SciPy's gaussian_filter differences of cd = c1 - c2 on (c1 != 0) & (c2 != 0),
                          and to the dense route (mst_trans_prologue, mst_diff_image, mst_gauss_blur) on the same tiles
  norm.fit                within pair_reference's LOC_BOUND / SCALE_BOUND of the exact two-pass value; NaN where no pixel is set in both
  mask_count              exact
  launches                two back-to-back calls with different C equal each call alone; mst_diff_dog_band gives the same bytes
                          before and after a tile-direct call (the two share one kernel body and their host tables)

The octave lists are those of tests/test_gpu_pair_kernels.py: between them the largest sigma_2 / sigma_3 radius falls in 1..8,
9..14 and 15..28, one list at least per tile.  Tile stacks: inner tiles and reflected-border tiles of every instantiation (C = 333),
C one above a tile edge (65), C below the widest halo (20) and below every halo (5).
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

OCTAVE_LISTS = tuple(rs.DIFF_BASE_LISTS)             # ([1.6, 3.2], [2.0, 4.0], [5.0], [3.2, 6.4], [1.6, 3.2, 6.4])
TILE_RADII = {8: (1, 8), 14: (9, 14), 28: (15, 28)}  # DiffTile8 / DiffTile14 / DiffTile28 of mst_diff.hip


def _tiles(P, C, seed, density=0.5, pattern=True):
    """two stacks [P, C, C] of different depth: values that are no integers (every rounding shows), pixels set in one sample
    only, rows and columns empty in one sample; with pattern, the LAST pair has disjoint supports"""
    rng = np.random.default_rng(seed)
    c1 = np.where(rng.random((P, C, C)) < density, rng.normal(0.0, 1.0, (P, C, C)) * rng.uniform(0.5, 2.0, (P, C, C)), 0.0)
    c2 = np.where(rng.random((P, C, C)) < density, c1 * rng.uniform(0.7, 1.3, (P, C, C)) + rng.normal(0.0, 0.3, (P, C, C)), 0.0)
    c2 = np.where((c1 == 0) & (rng.random((P, C, C)) < 0.3), rng.uniform(0.1, 3.0, (P, C, C)), c2)
    if pattern:
        for p in range(P):
            rows = rng.choice(C, size=max(C // 10, 2), replace=False)
            c1[p, rows[: len(rows) // 2]] = 0.0
            c2[p, :, rows[len(rows) // 2:]] = 0.0
        if P > 1:
            c2[P - 1][c1[P - 1] != 0] = 0.0
    return c1, c2


def _reference(c1, c2, lt):
    """rule 4's difference image and D = G(sigma_2) - G(sigma_3) per octave, float64 SciPy"""
    import oracle
    both = (c1 != 0) & (c2 != 0)
    cd = np.where(both, c1 - c2, 0.0)
    lpo = lt.levels_per_octave
    D = np.stack([oracle.blur_scipy(cd, lt.sigma[o * lpo + 1], lt.truncate[o * lpo + 1]) -
                  oracle.blur_scipy(cd, lt.sigma[o * lpo + 2], lt.truncate[o * lpo + 2]) for o in range(len(lt.octave_values))])
    return cd, both, D


def _launch_tiles(eng, d1, d2):
    """mst_diff_dog_tiles on device stacks d1, d2 into poisoned outputs; nothing is waited for"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    P, C, _ = d1.shape
    n_oct = len(eng.levels.octave_values)
    lv = ctypes.byref(eng._lv_struct)
    dog = torch.full((n_oct, P, C, C), float("nan"), dtype=torch.float64, device="cuda")
    fit = torch.full((n_oct, P, 2), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    wsb = int(eng.lib.mst_diff_dog_tiles_workspace_bytes(P, C, lv))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    _lib.check(eng.lib.mst_diff_dog_tiles(_ptr(d1), _ptr(d2), P, C, lv, _ptr(dog), _ptr(fit), _ptr(cnt), _ptr(ws), wsb, _stream()))
    return dog, fit, cnt, ws


def _dense_route(eng, d1, d2):
    """mst_trans_prologue -> mst_diff_image -> mst_gauss_blur at sigma_2 / sigma_3: (cd, mask, count, G_2 - G_3 per octave)"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    P, C, _ = d1.shape
    c = torch.cat([d1, d2])
    nz = torch.empty((2 * P, C, C), dtype=torch.uint8, device="cuda")
    nzc = torch.empty(2 * P, dtype=torch.int32, device="cuda")
    _lib.check(eng.lib.mst_trans_prologue(_ptr(c), _ptr(nz), _ptr(nzc), 2 * P, C, _stream()))
    cd = torch.empty((P, C, C), dtype=torch.float64, device="cuda")
    nzb = torch.empty((P, C, C), dtype=torch.uint8, device="cuda")
    nzbc = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    _lib.check(eng.lib.mst_diff_image(_ptr(c[:P]), _ptr(c[P:]), _ptr(nz[:P]), _ptr(nz[P:]), P, C, _ptr(cd), _ptr(nzb), _ptr(nzbc),
                                      _stream()))
    lt = eng.levels
    lpo = lt.levels_per_octave
    d = [eng.gauss_blur(cd, lt.taps[o * lpo + 1]) - eng.gauss_blur(cd, lt.taps[o * lpo + 2]) for o in range(len(lt.octave_values))]
    return cd.cpu().numpy(), nzb.cpu().numpy().astype(bool), nzbc.cpu().numpy(), torch.stack(d).cpu().numpy()


def _check(eng, c1, c2, results, what):
    dog, fit, cnt = (t.cpu().numpy() for t in results[:3])
    P = c1.shape[0]
    masked = 0
    for p in range(P):
        cd, both, D = _reference(c1[p], c2[p], eng.levels)
        assert int(cnt[p]) == int(both.sum()), (what, p)
        masked += int(both.sum())
        for o in range(D.shape[0]):
            g = dog[o, p]
            assert np.array_equal(g, D[o]), (what, p, o, int((g != D[o]).sum()), float(np.nanmax(np.abs(g - D[o]))))
            vals = D[o][both]
            if vals.size == 0:
                assert np.isnan(fit[o, p]).all(), (what, p, o, fit[o, p])
                continue
            loc_x, scale_x = pr.exact_normfit(vals)
            el, es = pr.fit_errors(fit[o, p, 0], fit[o, p, 1], loc_x, scale_x)
            print("fit errors %s pair %d octave %d: loc %.3g scale %.3g (bounds %.0e / %.0e)" % (what, p, o, el, es, pr.LOC_BOUND,
                                                                                              pr.SCALE_BOUND))
            assert el <= pr.LOC_BOUND and es <= pr.SCALE_BOUND, (what, p, o, fit[o, p], (loc_x, scale_x))
    return masked


STACKS = [(2, 333, 1), (1, 65, 2), (3, 20, 3), (2, 5, 4), (1, 64, 5)]          # (P, C, seed)


def test_octave_lists_reach_every_tile():
    from mustache_amd.levels import LevelTable
    reached = set()
    for octs in OCTAVE_LISTS:
        lt = LevelTable(octs)
        lpo = lt.levels_per_octave
        r = max(lt.radius[o * lpo + q] for o in range(len(octs)) for q in (1, 2))
        reached.add(next(t for t, (lo, hi) in TILE_RADII.items() if lo <= r <= hi))
    assert reached == set(TILE_RADII)
    # C = 333 holds inner tiles (window inside the stack) and border tiles of the widest instantiation; 20 and 5 are below halos
    assert 333 - (32 + 2 * 28) > 32 and 20 < 28 and 5 < 8


@pytest.mark.parametrize("octaves", OCTAVE_LISTS, ids=lambda o: ",".join(map(str, o)))
def test_diff_dog_tiles_every_tile_vs_scipy_and_dense_route(octaves):
    import torch
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine(octaves)
    masked = 0
    for P, C, seed in STACKS:
        c1, c2 = _tiles(P, C, seed)
        d1, d2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
        res = _launch_tiles(eng, d1, d2)
        masked += _check(eng, c1, c2, res, (octaves, P, C))
        cd, nzb, nzbc, dense = _dense_route(eng, d1, d2)
        dog = res[0].cpu().numpy()
        for p in range(P):
            ref_cd, both, _ = _reference(c1[p], c2[p], eng.levels)
            assert np.array_equal(cd[p], ref_cd) and np.array_equal(nzb[p], both) and int(nzbc[p]) == int(both.sum())
        assert np.array_equal(dense, dog), (octaves, P, C, int((dense != dog).sum()))
        if P > 1:
            assert int(res[2][P - 1]) == 0 and (dog[:, P - 1] == 0).all()           # disjoint supports: nothing to blur
    assert masked > 10000


def test_diff_dog_tiles_back_to_back_calls_with_different_c():
    """two calls with different C and P on one stream, nothing waited for between them, against each call alone"""
    import torch
    from mustache_amd.engine import ScaleSpaceEngine
    for octaves in ([1.6, 3.2], [3.2, 6.4]):
        eng = ScaleSpaceEngine(octaves)
        a1, a2 = (torch.from_numpy(t).cuda() for t in _tiles(2, 333, 11))
        b1, b2 = (torch.from_numpy(t).cuda() for t in _tiles(3, 70, 12))
        alone_a = [t.clone() for t in _launch_tiles(eng, a1, a2)[:3]]
        torch.cuda.synchronize()
        alone_b = [t.clone() for t in _launch_tiles(eng, b1, b2)[:3]]
        torch.cuda.synchronize()
        ra = _launch_tiles(eng, a1, a2)
        rb = _launch_tiles(eng, b1, b2)
        torch.cuda.synchronize()
        for got, exp in ((ra, alone_a), (rb, alone_b)):
            for g, e in zip(got[:3], exp):
                assert np.array_equal(g.cpu().numpy().view(np.uint8), e.cpu().numpy().view(np.uint8))
        _check(eng, *(t.cpu().numpy() for t in (b1, b2)), rb, (octaves, "second call"))


@pytest.mark.parametrize("octaves", [[1.6, 3.2], [2.0, 4.0], [3.2, 6.4]], ids=lambda o: ",".join(map(str, o)))
def test_band_kernel_is_unchanged_around_a_tiles_call(octaves):
    """mst_diff_dog_band before and after mst_diff_dog_tiles on the same stream: the same bytes, and still SciPy's"""
    import torch
    import test_gpu_pair_kernels as pk
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine(octaves)
    c1, c2 = pk._samples(150, 30, 7, pattern=True)
    case = (c1, c2, 150, 30, [0, 40, 100], 65)
    bands = [pk._band(c1, 150, 30), pk._band(c2, 150, 30)]
    before = pk._launch_band(eng, bands, 150, 30, case[4], 65)
    t1, t2 = (torch.from_numpy(t).cuda() for t in _tiles(2, 65, 21))
    mid = _launch_tiles(eng, t1, t2)
    after = pk._launch_band(eng, bands, 150, 30, case[4], 65)
    torch.cuda.synchronize()
    for b, a in zip(before[:3], after[:3]):
        assert np.array_equal(b.cpu().numpy().view(np.uint8), a.cpu().numpy().view(np.uint8))
    pk._check_case(eng, octaves, case, after[:3])
    _check(eng, t1.cpu().numpy(), t2.cpu().numpy(), mid, (octaves, "between two band calls"))


def test_diff_dog_tiles_refuses_bad_arguments():
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine([1.6, 3.2])
    lv = ctypes.byref(eng._lv_struct)
    t = torch.zeros((1, 8, 8), dtype=torch.float64, device="cuda")
    dog = torch.zeros((2, 1, 8, 8), dtype=torch.float64, device="cuda")
    fit = torch.zeros((2, 1, 2), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    wsb = int(eng.lib.mst_diff_dog_tiles_workspace_bytes(1, 8, lv))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    assert eng.lib.mst_diff_dog_tiles_workspace_bytes(0, 8, lv) == 0
    for args in ((_ptr(t), _ptr(t), 0, 8, lv, _ptr(dog), _ptr(fit), _ptr(cnt), _ptr(ws), wsb, _stream()),
                 (_ptr(t), _ptr(t), 1, 8, lv, _ptr(dog), _ptr(fit), _ptr(cnt), _ptr(ws), wsb - 1, _stream()),
                 (None, _ptr(t), 1, 8, lv, _ptr(dog), _ptr(fit), _ptr(cnt), _ptr(ws), wsb, _stream())):
        assert eng.lib.mst_diff_dog_tiles(*args) == _lib.MST_E_ARG
