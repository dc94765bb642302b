"""CPU side of the radius sweeps (tests/radius_sweep.py): the octave lists reach every (tile, radius) instantiation of the
sigma-stack kernel and of the difference kernel, none of them can be dropped, the lists that double get level reuse and
the others do not -- all from the level tables alone -- and the reference's own output on the sweep's input block changes
when one outermost tap of a witness level moves by 2^-40 (a sweep that cannot see a wrong tap is no test)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radius_sweep as rs      # noqa: E402


def _radii(names):
    return set(r for name in names for r in rs.level_table(rs.SIGMA_SWEEP[name][0]).radius)


def test_sigma_sweep_reaches_every_radius_of_every_tile():
    default, wide = rs.sigma_lists_of("default"), rs.sigma_lists_of("wide")
    assert sorted(default + wide) == sorted(rs.SIGMA_SWEEP)
    assert _radii(default) == set(range(1, 15))
    assert _radii(wide) == set(range(1, 29))
    assert _radii([rs.FMA_LIST]) == set(range(1, 15)) and rs.FMA_LIST in default
    wit = rs.sigma_witnesses()
    assert sorted(wit) == sorted((t, r) for t, rmax in rs.SIGMA_TILE_RMAX.items() for r in range(1, rmax + 1))
    assert len(wit) == 56
    for (tile, r), (name, l) in wit.items():
        lt = rs.level_table(rs.SIGMA_SWEEP[name][0])
        assert lt.radius[l] == r and name in rs.sigma_lists_of(tile)


def test_long_sweep_lists_fill_the_level_limits():
    from mustache_amd import _lib
    for name, n_tested in rs.LONG_LISTS.items():
        lt = rs.level_table(rs.SIGMA_SWEEP[name][0])
        assert lt.n_tested == n_tested and n_tested in (36, 45) and n_tested <= _lib.MST_MAX_TESTED
        assert len(lt.sigma) == n_tested // 9 * 12 <= _lib.MST_MAX_LEVELS
        assert len(lt.octave_values) > 3
    assert any(len(rs.SIGMA_SWEEP[name][0]) == 5 for name in rs.sigma_lists_of("wide"))
    assert any(len(rs.SIGMA_SWEEP[name][0]) == 4 for name in rs.sigma_lists_of("default"))


def test_level_reuse_of_doubling_and_other_lists():
    """make_dev_levels keeps two blurs across an octave boundary exactly where the lists double"""
    for tile in ("default", "wide"):
        plain = [n for n in rs.sigma_lists_of(tile) if not rs.SIGMA_SWEEP[n][1]]
        assert plain and all(len(rs.SIGMA_SWEEP[n][0]) >= 2 for n in plain), tile
    for name, (octs, doubling) in rs.SIGMA_SWEEP.items():
        assert doubling == all(b == 2 * a for a, b in zip(octs, octs[1:])), name
        reuse = rs.level_reuse(rs.level_table(octs))
        assert len(reuse) == len(octs) - 1 >= 1
        assert all(reuse) if doubling else not any(reuse), (name, reuse)
    for octs in ([1.6, 3.2], [2.0, 4.0], [3.2, 6.4], [1.6, 3.2, 6.4]):       # the doubling lists of the other tests
        assert all(rs.level_reuse(rs.level_table(octs))), octs


def test_no_sigma_sweep_list_can_be_dropped():
    """without any one list a (tile, radius) pair is left out, or a tile has no list without level reuse"""
    for name in rs.SIGMA_SWEEP:
        rest = {k: v for k, v in rs.SIGMA_SWEEP.items() if k != name}
        gap = len(rs.sigma_witnesses(rest)) < 56
        for tile in ("default", "wide"):
            gap = gap or not any(not rest[n][1] for n in rs.sigma_lists_of(tile) if n in rest)
        assert gap, name


def test_diff_sweep_reaches_every_radius_of_every_tile():
    wit = rs.diff_witnesses()
    assert sorted(wit) == sorted((t, r) for t, rmax in rs.DIFF_TILE_RMAX.items() for r in range(1, rmax + 1))
    assert len(wit) == 50
    for name, octs in rs.diff_lists():
        lt = rs.DiffLevels(octs)
        assert 1 <= min(lt.diff_radii()) and max(lt.diff_radii()) <= 28, name
        assert len(lt.sigma) <= 64 and len(octs) <= 5, name
    # the lists of the other tests go through the package, whose level table holds the sigma loop's limits: same numbers
    for octs in rs.DIFF_BASE_LISTS:
        lt, ref = rs.DiffLevels(octs), rs.level_table(octs)
        assert lt.radius == ref.radius and lt.sigma == ref.sigma and lt.truncate == ref.truncate
        assert all(np.array_equal(a, b) for a, b in zip(lt.taps, ref.taps))
    # every tile has a sweep list of several octaves that do not double, and the widest one lists with a radius above 16
    for tile in rs.DIFF_TILE_RMAX:
        assert any(rs.diff_tile(rs.DiffLevels(o)) == tile and len(o) >= 2 for o in rs.DIFF_SWEEP.values()), tile
    assert all(max(rs.DiffLevels(o).diff_radii()) > 16 for n, o in rs.DIFF_SWEEP.items() if n.startswith("t28"))


def test_no_diff_sweep_list_can_be_dropped():
    for name in rs.DIFF_SWEEP:
        rest = [(n, o) for n, o in rs.diff_lists() if n != name]
        assert len(rs.diff_witnesses(rest)) < 50, name


# ---- sensitivity of the reference's output on the sweep's blocks --------------------------------------------------------
EPS = 1.0 + 2.0 ** -40


@pytest.mark.slow
def test_sigma_sweep_block_shows_one_tap_of_every_witness_level():
    """For the witness level of every (tile, radius): the reference (explicit blur: the NumPy restatement of SciPy's, which
    takes its taps as an argument) on the sweep's block, as it is and with that level's outermost tap times 1 + 2^-40.  What
    the GPU sweep compares bit for bit -- found pixels, levels, values, loc -- must differ.  Radius 28 occurs at k = 12 of
    the last octave only and radius 14 of the default tile likewise: those blurs reach the output through the sieve's D_n
    term alone, which the exact plane in the block (radius_sweep.sweep_block) makes decisive."""
    n, dpx = rs.SIGMA_GEOMETRY["wide"][0]
    assert (n, dpx) == rs.SIGMA_GEOMETRY["default"][0] and n <= 400
    c = rs.sweep_block(n, dpx)
    base, blind = {}, []
    wit = rs.sigma_witnesses()
    assert wit[("wide", 28)][1] % 12 == 11 and wit[("default", 14)][1] % 12 == 11
    for (tile, r), (name, l) in sorted(wit.items()):
        octs = rs.SIGMA_SWEEP[name][0]
        if name not in base:
            base[name] = rs.reference_found(c, dpx, octs, blur="explicit")
            assert len(base[name]["pixel"]) > 1000
        moved = rs.reference_found(c, dpx, octs, blur="explicit", perturb=(l, EPS))
        if rs.same_found(base[name], moved):
            blind.append((tile, r, name, l))
    assert not blind, blind


@pytest.mark.slow
def test_diff_sweep_case_shows_one_tap_of_every_witness_level():
    """the same for the difference kernel, whose tests compare the DoG G(sigma_2) - G(sigma_3) of every octave bit for bit
    on every addressable pixel: the explicit blur of the reference's difference image with one outermost tap moved"""
    import oracle
    import test_gpu_pair_kernels as pk
    c1, c2, n, dpx, starts, CH = pk._cases()[0]
    cd, nzb, _ = pk._reference(pk._block(c1, n, starts[0], CH), pk._block(c2, n, starts[0], CH), dpx, [1.6, 3.2])
    off = np.arange(CH)[None, :] - np.arange(CH)[:, None]
    addr = (off >= 4) & (off <= dpx + 1)
    assert nzb.sum() > 10000
    blind = []
    for (tile, r), (name, l) in sorted(rs.diff_witnesses().items()):
        lt = rs.DiffLevels(dict(rs.diff_lists())[name])
        w = np.concatenate([lt.taps[l][:0:-1], lt.taps[l]])
        assert np.array_equal(oracle.blur_explicit(cd, w, r), oracle.blur_scipy(cd, lt.sigma[l], lt.truncate[l])), (name, l)
        moved = w.copy()
        moved[0] *= EPS
        moved[-1] *= EPS
        if np.array_equal(oracle.blur_explicit(cd, w, r)[addr], oracle.blur_explicit(cd, moved, r)[addr]):
            blind.append((tile, r, name, l))
    assert not blind, blind
