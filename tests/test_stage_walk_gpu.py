"""The inner tile's diagonal walk (mst_stage_walk.h) through both kernels that call it: the fused kernel's band source
(mst_scale_space.hip) and the difference kernel's (mst_diff.hip).  An inner tile is one whose window, blur halo included, lies
inside the block: 60 x 92 at the default tile, 88 x 120 at the wide one.  A lane of the walk owns a tile ROW on every diagonal;
what can go wrong is the column range of a diagonal (tile edge, chromosome end), the band test and the fills per diagonal, the
lane-constant region test of the tested flags, and the addresses that move by a constant per diagonal and by a round.

Fused kernel: every case runs the band source and the dense source (which does not walk: the same results from the other
staging), with and without skip_empty, against oracle.block_prologue + oracle.scale_space_levels(blur="scipy")
(tests/radius_sweep.py) with the checks of test_tile_edges_outside_loop.py: tested-pixel counts exactly, pixels, levels and
values with np.array_equal, loc exactly, scale to 1e-12, p-values to 1e-9; with MUSTACHE_HIP_LIB naming another build, both
builds bit for bit.

Default-tile blocks are 200 x 200 with distance limit 60, the smallest block that holds inner tiles: tile column 1 only (window
columns 47 .. 138), tile rows 1 .. 5.  A window spans 151 diagonals, the band 4 .. 61 only 58, so at this distance limit no
window lies wholly inside the band; the kinds the block does hold are asserted below (crossing 4 / 5 and dpx + 1, crossing 4 / 5
only, constant below the diagonal).  A window wholly inside the band needs 151 diagonals of band: the 300 x 300 block at
distance limit 260 is added for it (tile (1, 3): diagonals 97 .. 247).

Difference kernel, at each of its three tiles (halo 8, 14, 28): a 200 x 200 pair against NumPy alone -- the difference image of
diff_mustache.py:262-276 and the two blurs per octave in SciPy's tap order, t = x[c] w0; for j = r..1: t += (x[c-j] + x[c+j])
w[j], axis 0 first, reflect -- on every pixel a record can address, bit for bit, and the doubly tested count exactly."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radius_sweep as rs                      # noqa: E402
import test_tile_edges_outside_loop as te      # noqa: E402

ITR, ITC = te.ITR, te.ITC
OCTAVES, WIDE_OCTAVES = te.OCTAVES, te.WIDE_OCTAVES


# ---- geometry: which tiles of a block are inner, and what their windows cross ------------------------------------------------
def inner_tiles(CH, rmax, start=0):
    """[(tile row, tile column, first diagonal, last diagonal)] of the inner tiles of the block at chromosome coordinate start:
    the lattice is anchored at coordinate 0, a region starts one pixel before the pixels its tile owns"""
    ctr, ctc = 32 + 2 * rmax, 64 + 2 * rmax
    out = []
    for ty in range(-1, CH // ITR + 2):
        for tx in range(-1, CH // ITC + 2):
            Y0, X0 = ty * ITR - start % ITR - 1 - rmax, tx * ITC - start % ITC - 1 - rmax
            if Y0 >= 0 and X0 >= 0 and Y0 + ctr <= CH and X0 + ctc <= CH:
                out.append((ty, tx, X0 - (Y0 + ctr - 1), X0 + ctc - 1 - Y0))
    return out


def kinds(CH, dpx, rmax):
    """{kind: tiles}: what the walked windows of a block cross.  A window whose diagonals all lie at 3 or below, or at dpx + 2 or
    above, is not walked (the constant path)"""
    out = {"both": [], "low": [], "high": [], "inside": [], "constant": []}
    for ty, tx, lo, hi in inner_tiles(CH, rmax):
        if hi <= 3 or lo >= dpx + 2:
            k = "constant"
        elif lo <= 4 and hi >= dpx + 1:
            k = "both"
        elif lo <= 4:
            k = "low"
        elif hi >= dpx + 1:
            k = "high"
        else:
            k = "inside"
        out[k].append((ty, tx))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def band60_chromosome():
    n, dpx = 200, 60
    return te._noise_block(n, dpx, 21, [(40, 70, 6.0, 1.5), (60, 95, 5.0, 1.2), (95, 120, 7.0, 1.6), (120, 150, 6.0, 1.4),
                                        (150, 170, 5.0, 1.3), (20, 30, 5.0, 1.5)]), n, dpx, [0], 200


@functools.lru_cache(maxsize=None)
def short_chromosome():
    """the same block cut from a chromosome of 120 bins: the chromosome ends at window column 120 - 47 = 73 of the inner tiles"""
    c, _, dpx, _, CH = band60_chromosome()
    return np.ascontiguousarray(c[:120, :120]), 120, dpx, [0], CH


@functools.lru_cache(maxsize=None)
def inside_chromosome():
    n, dpx = 300, 260
    return te._noise_block(n, dpx, 22, [(40, 100, 6.0, 1.5), (45, 230, 5.0, 1.2), (100, 260, 7.0, 1.6), (200, 280, 6.0, 1.4),
                                        (150, 170, 5.0, 1.3)]), n, dpx, [0], 300


@functools.lru_cache(maxsize=None)
def wide_chromosome():
    n, dpx = 300, 200
    return te._noise_block(n, dpx, 23, [(40, 100, 6.0, 1.5), (90, 230, 5.0, 1.2), (100, 260, 7.0, 1.6), (200, 280, 6.0, 1.4),
                                        (150, 170, 5.0, 1.3)]), n, dpx, [0], 300


CHROMOSOMES = {"band60": band60_chromosome, "short": short_chromosome, "inside": inside_chromosome, "wide": wide_chromosome}
te.CHROMOSOMES.update({"walk_" + k: v for k, v in CHROMOSOMES.items()})      # the references are cached under these names


def check_geometry():
    k = kinds(200, 60, 14)
    assert k == {"both": [(1, 1), (2, 1), (3, 1)], "low": [(4, 1)], "high": [], "inside": [], "constant": [(5, 1)]}, k
    c, n, dpx, starts, CH = short_chromosome()
    X0 = ITC - 1 - 14
    assert 0 < n - X0 < 92 and CH == 200, "the chromosome ends inside the inner tiles' windows"
    k = kinds(300, 260, 14)
    assert (1, 3) in k["inside"] and k["low"], k
    k = kinds(300, 200, 28)      # a wide window spans 207 diagonals: 4 / 5 and dpx + 1 = 201 in different windows
    assert k["low"] and k["high"], k
    assert max(rs.level_table(WIDE_OCTAVES).radius) == 15 and rs.sigma_tile(rs.level_table(WIDE_OCTAVES)) == "wide"
    for name in ("band60", "short", "inside"):
        for ref in te.references("walk_" + name):
            assert len(ref["pixel"]) > 0 and ref["n_tested_pixels"] > 0, name
    assert len(te.references("walk_wide", tuple(WIDE_OCTAVES))[0]["pixel"]) > 0


def test_blocks_hold_the_tiles_they_are_meant_to():
    check_geometry()


# ---- fused kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", te.SOURCES, ids=te.IDS)
def test_inner_tiles_across_both_band_edges(source, skip_empty):
    """200 x 200, distance limit 60: windows that cross diagonals 4 / 5 and dpx + 1, 4 / 5 alone, and a constant one"""
    check_geometry()
    te._check_case("walk_band60", source, skip_empty)


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", te.SOURCES, ids=te.IDS)
def test_chromosome_ends_inside_an_inner_tile(source, skip_empty):
    te._check_case("walk_short", source, skip_empty)


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", te.SOURCES, ids=te.IDS)
def test_inner_tile_wholly_inside_the_band(source, skip_empty):
    te._check_case("walk_inside", source, skip_empty)


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", te.SOURCES, ids=te.IDS)
def test_wide_tile_two_rows_per_lane(source, skip_empty):
    """radius 15: 88 x 120 windows, lanes 0 .. 23 own a second row, eight waves, three rounds"""
    te._check_case("walk_wide", source, skip_empty, tuple(WIDE_OCTAVES))


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", te.SOURCES, ids=te.IDS)
def test_shared_inner_tiles_of_two_overlapping_blocks(source, skip_empty):
    c, n, dpx, starts, CH = te.overlap_chromosome()
    assert CH == 300 and any(inner_tiles(CH, 14, s) for s in starts)
    if source == "band":
        for _, eng in te._engines(tuple(OCTAVES)):
            items, tiles, shared = eng.band_items(starts, CH, dpx, skip_empty=skip_empty, share=True)
            assert shared > 0 and items + shared == tiles
    te._check_case("overlap", source, skip_empty)


# ---- difference kernel --------------------------------------------------------------------------------------------------------
def numpy_blur(img, taps):
    """gaussian_filter(mode='reflect') in NumPy: SciPy's correlate1d order on a symmetric kernel, axis 0 then axis 1"""
    r = len(taps) - 1
    for axis in (0, 1):
        x = np.moveaxis(img, axis, 0)
        p = np.concatenate([x[:r][::-1], x, x[-r:][::-1]]) if r else x
        m = x.shape[0]
        t = p[r:r + m] * taps[0]
        for j in range(r, 0, -1):
            t = t + (p[r - j:r - j + m] + p[r + j:r + j + m]) * taps[j]
        img = np.moveaxis(t, 0, axis)
    return img


DIFF_OCTAVES = {8: [1.6, 3.2], 14: [5.0], 28: [3.2, 6.4]}      # the difference kernel's tile -> an octave list that selects it


def test_difference_kernel_tiles_and_their_inner_windows():
    for tile, octaves in DIFF_OCTAVES.items():
        assert rs.diff_tile(rs.DiffLevels(octaves)) == tile
        k = kinds(200, 60, tile)
        assert k["both"] or (k["low"] and k["high"]), (tile, k)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", sorted(DIFF_OCTAVES))
def test_diff_dog_band_on_inner_tiles_against_numpy(tile):
    import test_gpu_pair_kernels as pk
    from mustache_amd.engine import ScaleSpaceEngine
    n = CH = 200
    dpx = 60
    octaves = DIFF_OCTAVES[tile]
    c1, c2 = pk._samples(n, dpx, 31, pattern=True)
    eng = ScaleSpaceEngine(octaves)
    dog, fit, cnt, keep = pk._launch_band(eng, [pk._band(c1, n, dpx), pk._band(c2, n, dpx)], n, dpx, [0], CH)
    dog, cnt = dog.cpu().numpy(), cnt.cpu().numpy()
    off = np.arange(CH)[None, :] - np.arange(CH)[:, None]
    both = (c1 != 0) & (c2 != 0) & (off >= 4)
    f1, f2 = c1.copy(), c2.copy()
    for f in (f1, f2):
        f[(off <= 4) | (off >= dpx + 1)] = 2.0
    cd = np.where(both, f1 - f2, 0.0)
    lt, addr = eng.levels, (off >= 4) & (off <= dpx + 1)
    print("doubly tested pixels: %d (NumPy %d)" % (int(cnt[0]), int(both.sum())))
    assert int(cnt[0]) == int(both.sum()) > 1000
    for o in range(len(octaves)):
        D = numpy_blur(cd, lt.taps[o * lt.levels_per_octave + 1]) - numpy_blur(cd, lt.taps[o * lt.levels_per_octave + 2])
        bad = int((dog[o, 0][addr] != D[addr]).sum())
        print("octave %d: %d of %d addressable pixels differ" % (o, bad, int(addr.sum())))
        assert np.array_equal(dog[o, 0][addr], D[addr]), (o, bad)
