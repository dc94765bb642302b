"""The radius switch of the fused blur kernels at the edges of what each tile is built for (mst_scale_space.hip, blur_dispatch;
mst_diff.hip, diff_blur_dispatch).  The switch has no path without a case: a radius above the tile's RMAX is unreachable code,
so the HOST has to keep every launch inside its tile -- with_tile / build_list choose the tile from the level table's largest
radius, check_levels caps it at 28 and MST_FLAG_FMA is refused above 14.  Level tables whose largest radius is
    exactly 14   the last table the default tile takes (octaves 1.6, 3.2),
    15           the first that must go to the wide tile (1.7, 3.4),
    28           the wide tile's last (3.2, 6.4)
run ONE launch each of the band-source kernel on the block of tests/test_sieve_gate.py (140 x 140, distance limit 100: 5 x 3
tiles, the block edge inside the last tile row and column, a wave without a tested pixel inside a tested tile) against
oracle.block_prologue + oracle.scale_space_levels(blur="scipy"): pixels, levels and values with np.array_equal, loc exactly,
scale to 1e-12 and p-values to 1e-9 (the bounds of test_gpu_radius_sweep.py).  The 14 and 15 tables also go through the
two-sample difference kernel (mst_diff_dog_band, the checks of test_gpu_pair_kernels.py).  A table with radius 29, and
MST_FLAG_FMA with radius 15, are refused on the host with their messages, and nothing is launched: the launch's first kernel
zeroes the counters, which keep the pattern the test put there.

What the inputs hold is asserted on the oracle alone first (test_inputs_on_the_oracle_alone, no GPU; the GPU tests repeat it):
the radii are what the case claims and select the tile it claims; a found pixel lies in a thread whose wave's OTHER column group
owns no tested pixel (the in-place maxima of a wave that is tested in one half only); a found pixel lies in the second octave
(the state carried across the octave boundary)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radius_sweep as rs      # noqa: E402
import test_sieve_gate as sg   # noqa: E402

CH, DPX = sg.CH, sg.DPX
# name -> (octaves, largest radius, tile)
TABLES = {
    "radius-14": ([1.6, 3.2], 14, "default"),
    "radius-15": ([1.7, 3.4], 15, "wide"),
    "radius-28": ([3.2, 6.4], 28, "wide"),
}
DIFF_TABLES = ("radius-14", "radius-15")
REFUSED_29 = [6.7]             # one octave whose last level has radius 29
SENTINEL = 0x5A5A5A5A


def half_tested_wave_found(ref, K):
    """found pixels whose thread shares its wave with a column group that owns no tested pixel: a wave is two column groups
    of K columns (lanes = 32 region rows x 2 groups), tiles of 30 x 62 owned pixels on the lattice anchored at the block's origin"""
    nz, n = ref["nz"], 0
    for p in ref["pixel"]:
        y, x = divmod(int(p), CH)
        y0, x0 = (y // sg.ITR) * sg.ITR - 1, (x // sg.ITC) * sg.ITC - 1
        other = ((x - x0) // K) ^ 1
        cols = [x0 + other * K + k for k in range(K) if 1 <= other * K + k <= sg.ITC and x0 + other * K + k < CH]
        rows = [r for r in range(y0 + 1, y0 + sg.ITR + 1) if r < CH]
        n += int(not cols or not nz[np.ix_(rows, cols)].any())
    return n


@functools.lru_cache(maxsize=None)
def case(name):
    """(block, reference_found of it) -- computed once per table"""
    c = sg.block()
    return c, rs.reference_found(c, DPX, TABLES[name][0])


def check_reference(name):
    octaves, radius, tile = TABLES[name]
    lt = rs.level_table(octaves)
    assert max(lt.radius) == radius and rs.sigma_tile(lt) == tile
    assert radius in (rs.SIGMA_TILE_RMAX["default"], rs.SIGMA_TILE_RMAX["default"] + 1, rs.SIGMA_TILE_RMAX["wide"])
    c, ref = case(name)
    per_octave = lt.n_tested // len(octaves)
    assert len(ref["pixel"]) > 0, "the oracle finds pixels"
    assert (ref["level"] > per_octave).any(), "a found pixel in the second octave"
    assert half_tested_wave_found(ref, sg.TILE_K[tile]) > 0, "a found pixel in a wave whose other column group is untested"


def check_refused_tables():
    lt = rs.DiffLevels(REFUSED_29)
    assert max(lt.radius) == 29 and min(lt.radius) >= 1
    assert max(rs.level_table(TABLES["radius-15"][0]).radius) == 15


@pytest.mark.parametrize("name", list(TABLES))
def test_inputs_on_the_oracle_alone(name):
    check_reference(name)
    check_refused_tables()


def _band(c):
    import torch
    from mustache_amd.normalize import band_from_coo
    x, y = np.nonzero(c)
    band = band_from_coo(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(c[x, y]).cuda(), CH, DPX)
    assert np.array_equal(rs.block_from_band(band.cpu().numpy(), CH, DPX), c)
    return band


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLES))
def test_radius_edge_tables_vs_oracle(name):
    from mustache_amd.engine import ScaleSpaceEngine
    check_reference(name)
    c, ref = case(name)
    eng = ScaleSpaceEngine(TABLES[name][0])
    nt = eng.levels.n_tested
    found, fits, nzc = eng.sigma_loop_band(_band(c), CH, DPX, [0], CH, skip_empty=True)
    rec = found[0]
    tested = int(nzc.cpu().numpy().view(np.uint32)[0])
    print("%s: %d tested pixels, %d found (oracle %d)" % (name, tested, len(rec["pixel"]), len(ref["pixel"])))
    assert tested == ref["n_tested_pixels"]
    assert np.array_equal(rec["pixel"].astype(np.int64), ref["pixel"])
    assert np.array_equal(rec["level"].astype(np.int64), ref["level"].astype(np.int64))
    assert np.array_equal(rec["value"], ref["value"])
    assert np.array_equal(np.asarray(fits[0][0])[:nt], ref["loc"])
    np.testing.assert_allclose(np.asarray(fits[0][1])[:nt], ref["scale"], rtol=1e-12)
    np.testing.assert_allclose(rec["pval"], ref["pval"], rtol=1e-9, atol=0)


def _second_sample(c):
    """the block as a second sample: other depth, other noise, a tenth of its pixels missing"""
    rng = np.random.default_rng(23)
    c2 = c * 0.6 * rng.uniform(0.7, 1.4, c.shape)
    c2[rng.uniform(0.0, 1.0, c.shape) < 0.1] = 0.0
    return c2


@pytest.mark.gpu
@pytest.mark.parametrize("name", DIFF_TABLES)
def test_radius_edge_tables_through_the_difference_kernel(name):
    import test_gpu_pair_kernels as pk
    from mustache_amd.engine import ScaleSpaceEngine
    octaves = TABLES[name][0]
    eng = ScaleSpaceEngine(octaves)
    c1 = sg.block()
    c2 = _second_sample(c1)
    run = (c1, c2, CH, DPX, [0], CH)
    dog, fit, cnt, keep = pk._launch_band(eng, [pk._band(c1, CH, DPX), pk._band(c2, CH, DPX)], CH, DPX, [0], CH)
    cnt = pk._check_case(eng, octaves, run, (dog, fit, cnt))
    print("%s: difference kernel tile %d, %d doubly tested pixels" % (name, rs.diff_tile(rs.DiffLevels(octaves)), int(cnt.sum())))
    assert int(cnt.sum()) > 1000


def _refused_launch(eng, lv_struct, flag_word):
    """mst_scale_space_band on the block with `lv_struct`: (return code, message, whether any output changed)"""
    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    lib, T, cap = eng.lib, _lib.MST_MAX_TESTED, 4096
    band = _band(sg.block())
    valid = rs.level_table(TABLES["radius-28"][0]).as_struct()          # a workspace no smaller than any table's
    ws_bytes = max(int(lib.mst_scale_space_workspace_bytes(1, CH, ctypes.byref(lv_struct))),
                   int(lib.mst_scale_space_workspace_bytes(1, CH, ctypes.byref(valid))))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    outs = [torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda") for shape in ((1,), (1,), (1, T, 4), (1, cap, 4))]
    count, nzc, stats, found = outs
    st = (ctypes.c_int64 * 1)(0)
    torch.cuda.synchronize()
    rc = lib.mst_scale_space_band(_ptr(band), CH, DPX, st, 1, CH, ctypes.byref(lv_struct), _ptr(found), cap, _ptr(count),
                                  _ptr(stats), _ptr(nzc), flag_word, _ptr(ws), ws_bytes, _stream())
    msg = lib.mst_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    return rc, msg, any(bool((t != SENTINEL).any()) for t in outs)


@pytest.mark.gpu
def test_unsupported_radii_are_refused_on_the_host_and_launch_nothing():
    from mustache_amd import _lib
    from mustache_amd.engine import ScaleSpaceEngine
    check_refused_tables()
    eng = ScaleSpaceEngine([1.6, 3.2])                 # the library; not its levels
    rc, msg, touched = _refused_launch(eng, rs.DiffLevels(REFUSED_29).as_struct(), _lib.MST_FLAG_SKIP_EMPTY)
    assert rc == _lib.MST_E_ARG and "blur radius 29 outside the supported range [1, 28]" in msg, (rc, msg)
    assert not touched, "radius 29: a kernel ran"
    lv15 = rs.level_table(TABLES["radius-15"][0]).as_struct()
    rc, msg, touched = _refused_launch(eng, lv15, _lib.MST_FLAG_SKIP_EMPTY | _lib.MST_FLAG_FMA)
    assert rc == _lib.MST_E_ARG and "MST_FLAG_FMA is only built for blur radii <= 14" in msg, (rc, msg)
    assert not touched, "MST_FLAG_FMA at radius 15: a kernel ran"
    # the same table without the flag runs (the refusal is the flag's, not the table's)
    rc, msg, touched = _refused_launch(eng, lv15, _lib.MST_FLAG_SKIP_EMPTY)
    assert rc == _lib.MST_OK and touched, (rc, msg)
