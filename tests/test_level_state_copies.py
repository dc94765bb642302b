"""The fused kernel's level loop copies no per-pixel state it does not have to, in the BUILT library (no GPU needed: ROCm's
llvm-objdump and the code objects' metadata on libmustache_hip.so, through scripts/isa_census.py and kernel_resources.py).

What this guards, for all six scale_space_kernel instantiations (default, FMA and wide tile, band and dense source):
  * the radius switch of blur_dispatch has no path without a case.  With one (`default: break;`, an empty case above the
    tile's RMAX) the compiler keeps the axis-1 accumulators in registers of their own and copies them into g behind the join:
    K v_mov_b64 per thread and level between the last radius case and the DoG subtraction;
  * the 3 x 3 maxima live in one set of registers: the comparisons against the previous level's maxima are taken before the new
    ones are written over them.  With both sets live the level ends with K more copies (Mc = m), on every wave;
  * what is left per level is one rename each of D and G, 2 K copies: the floor with one static register assignment;
  * the registers this frees stay free: no more VGPRs than before the change (232 / 230 default and FMA tile, 153 / 151 wide
    tile; dense / band source), no scratch, no vector spills.
Results do not change either way, so only the code itself can show it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "scripts"))
import isa_census  # noqa: E402
import kernel_resources  # noqa: E402

# tile -> (pixels per thread, VGPRs of the dense-source and of the band-source kernel before the maxima were kept in place)
TILES = {"32,64,14,8,1,0,0": (8, 232, 230), "32,64,14,8,1,1,0": (8, 232, 230), "32,64,28,4,1,0,1": (4, 153, 151)}
EXPECTED = {"scale_space_kernel Tile<%s> %s source" % (t, s): (k, dense if s == "dense" else band)
            for t, (k, dense, band) in TILES.items() for s in ("dense", "band")}


def _built():
    if not os.path.exists(isa_census.LIB):
        pytest.skip("libmustache_hip.so is not built")
    if not os.path.exists(isa_census.OBJDUMP):
        pytest.skip("no llvm-objdump in this ROCm installation")


@pytest.fixture(scope="module")
def copies():
    _built()
    return {title: (K, per_level, behind) for title, K, per_level, behind in isa_census.state_copies()}


@pytest.fixture(scope="module")
def resources():
    _built()
    return {isa_census.kernel_title(k["name"]): k for k in kernel_resources.kernels(isa_census.LIB)
            if "scale_space_kernel" in k["name"]}


def test_every_instantiation_is_found(copies, resources):
    assert set(copies) == set(EXPECTED)
    assert set(resources) == set(EXPECTED)
    for title, (K, _, _) in copies.items():
        assert K == EXPECTED[title][0], title


@pytest.mark.parametrize("title", sorted(EXPECTED))
def test_no_scratch_and_no_more_registers_than_before(resources, title):
    k = resources[title]
    print(title, {f: k[f] for f in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")})
    assert k["private_segment_fixed_size"] == 0, title
    assert k["vgpr_spill_count"] == 0, title
    assert k["vgpr_count"] <= EXPECTED[title][1], (title, k["vgpr_count"])


@pytest.mark.parametrize("title", sorted(EXPECTED))
def test_no_copy_block_behind_the_radius_switch(copies, title):
    K, per_level, behind = copies[title]
    assert behind == 0, (title, behind)


@pytest.mark.parametrize("title", sorted(EXPECTED))
def test_two_renames_per_level_are_all_the_copies(copies, title):
    K, per_level, behind = copies[title]
    print(title, "copies per thread and level:", per_level)
    assert per_level <= 2 * K, (title, per_level)
