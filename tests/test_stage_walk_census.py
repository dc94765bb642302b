"""What the inner tile's diagonal walk (mst_stage_walk.h) costs in vector instructions, and that it costs no register -- no GPU
needed.

The walk's count is the path "staging: inner diagonal walk" of scripts/isa_census.py: the fused kernel of the default tile with
the band source, compiled from the tree's source with the product flags and line tables (the built library carries no line
tables, so the path cannot be booked there), straight-line instructions once and the round loop's twice.
profiles/r11_isa_census.txt holds the figure of the shipped form, WALK_SHIPPED = 463 vector instructions per thread (the form
before it: 1 524; the rejected scalar form: 979).
  bound  no more than WALK_SHIPPED plus 5 % for compiler drift.  Pinned here; not to be tuned.
  floor  WALK_SHIPPED itself lies below 979: a per-lane form that removes less than the scalar form did is not worth shipping.

Registers and spills come from the BUILT library's metadata (scripts/kernel_resources.py), for every instantiation of both
kernels that call the walk: no scratch, no vector spill, and VGPRs, SGPRs and scalar spills no higher than before the walk was
rewritten (PARENT; three instantiations spilled scalars before: the wide tile's fused band kernel 2, the wide difference
kernels 10)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "scripts"))
import isa_census  # noqa: E402
import kernel_resources  # noqa: E402

WALK_SHIPPED = 463                      # profiles/r11_isa_census.txt, "staging: inner diagonal walk", inner tile
WALK_BOUND = WALK_SHIPPED * 1.05
SCALAR_FORM = 979                       # LABBOOK, "Outside the level loop": measured 0.7 % slower than the per-lane walk
HIPCC = "/opt/rocm/bin/hipcc"

# title -> (VGPRs, SGPRs, scalar spills) of the parent's library
PARENT = {
    "diff_dog_kernel Tile<32,64,14,8,1,0,0> band source": (204, 98, 0),
    "diff_dog_kernel Tile<32,64,14,8,1,0,0> dense source": (204, 98, 0),
    "diff_dog_kernel Tile<32,64,28,4,1,0,1> band source": (193, 106, 10),
    "diff_dog_kernel Tile<32,64,28,4,1,0,1> dense source": (192, 106, 10),
    "diff_dog_kernel Tile<32,64,8,8,1,0,0> band source": (126, 100, 0),
    "diff_dog_kernel Tile<32,64,8,8,1,0,0> dense source": (122, 100, 0),
    "scale_space_kernel Tile<32,64,14,8,1,0,0> dense source": (214, 104, 0),
    "scale_space_kernel Tile<32,64,14,8,1,0,0> band source": (214, 104, 0),
    "scale_space_kernel Tile<32,64,14,8,1,1,0> dense source": (214, 104, 0),
    "scale_space_kernel Tile<32,64,14,8,1,1,0> band source": (214, 104, 0),
    "scale_space_kernel Tile<32,64,28,4,1,0,1> dense source": (142, 106, 0),
    "scale_space_kernel Tile<32,64,28,4,1,0,1> band source": (141, 106, 2),
}


def test_the_shipped_walk_is_below_the_rejected_scalar_form():
    assert WALK_SHIPPED < SCALAR_FORM


@pytest.fixture(scope="module")
def walk():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc in this ROCm installation")
    return isa_census.fused_walk()


def test_walk_within_five_percent_of_the_shipped_count(walk):
    print("staging: inner diagonal walk:", walk)
    assert walk["straight"] + walk["looped"] > 0, "the census no longer finds the walk"
    assert walk["weighted"] <= WALK_BOUND, walk


def test_difference_kernel_runs_the_same_body():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc in this ROCm installation")
    d = isa_census.diff_walk()
    print("diff_dog_kernel, inner diagonal walk:", d)
    # two loads per element and no fills: not the fused kernel's count, but of its order -- the walk it replaced took 1 613
    assert 0 < d["weighted"] <= SCALAR_FORM, d


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(isa_census.LIB):
        pytest.skip("libmustache_hip.so is not built")
    if not os.path.exists(isa_census.OBJDUMP):
        pytest.skip("no llvm-objdump in this ROCm installation")
    return {isa_census.kernel_title(k["name"]): k for k in kernel_resources.kernels(isa_census.LIB)
            if "scale_space_kernel" in k["name"] or "diff_dog_kernel" in k["name"]}


def test_every_instantiation_is_found(resources):
    assert set(resources) == set(PARENT)


@pytest.mark.parametrize("title", sorted(PARENT))
def test_no_scratch_no_new_spill_no_more_registers(resources, title):
    k = resources[title]
    got = (k["vgpr_count"], k["sgpr_count"], k["sgpr_spill_count"])
    print(title, got, "parent", PARENT[title])
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, title
    assert all(g <= p for g, p in zip(got, PARENT[title])), (title, got, PARENT[title])
