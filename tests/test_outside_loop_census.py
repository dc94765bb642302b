"""What the fused kernel issues OUTSIDE its level loop -- staging, tested mask, state initialisation, epilogue -- counted in the
BUILT library (no GPU needed: ROCm's llvm-objdump on libmustache_hip.so through scripts/isa_census.py, outside_valu()).

The bound is the count before the region was audited: 1 466 static vector instructions per thread for the default tile with
the band source (profiles/r09_isa_census.txt).  What the audit reached is in profiles/r10_isa_census.txt and LABBOOK.md and is
not fixed here.  The kernel still has no scratch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "scripts"))
import isa_census  # noqa: E402
import kernel_resources  # noqa: E402

DEFAULT_BAND = "scale_space_kernel Tile<32,64,14,8,1,0,0> band source"
OUTSIDE_VALU_BEFORE = 1466


def _built():
    if not os.path.exists(isa_census.LIB):
        pytest.skip("libmustache_hip.so is not built")
    if not os.path.exists(isa_census.OBJDUMP):
        pytest.skip("no llvm-objdump in this ROCm installation")


def test_outside_the_loop_no_more_vector_instructions_than_before():
    _built()
    counts = isa_census.outside_valu()
    print(counts)
    assert DEFAULT_BAND in counts
    assert counts[DEFAULT_BAND] <= OUTSIDE_VALU_BEFORE, counts[DEFAULT_BAND]


def test_the_kernel_still_has_no_scratch():
    _built()
    found = [k for k in kernel_resources.kernels(isa_census.LIB) if "scale_space_kernel" in k["name"]]
    assert any(isa_census.kernel_title(k["name"]) == DEFAULT_BAND for k in found)
    for k in found:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, isa_census.kernel_title(k["name"])
