"""The window loads of the blur passes are 16-byte ds_read_b128 in the BUILT library, at every radius of every kernel that
includes mst_fir.h (no GPU needed: ROCm's llvm-objdump on libmustache_hip.so, through scripts/isa_census.py).

What this guards: with OFF = 1 (odd RMAX - R in the axis-0 pass) a window's first and last element are never used; unless
fir_chunk names them as live, LLVM drops them and re-vectorises the window from its 8-byte aligned second element, and every
load of the window becomes a ds_read2_b64 (half the LDS rate, banks modulo 32).  Results do not change either way, so only
the code itself can show it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "scripts"))
import isa_census  # noqa: E402

# tile -> largest radius; each exists with a band and a dense source
FUSED = {"32,64,14,8,1,0,0": 14, "32,64,14,8,1,1,0": 14, "32,64,28,4,1,0,1": 28}
DIFF = {"32,64,8,8,1,0,0": 8, "32,64,14,8,1,0,0": 14, "32,64,28,4,1,0,1": 28}
EXPECTED = {"%s Tile<%s> %s source" % (k, t, s): r for k, tiles in (("scale_space_kernel", FUSED), ("diff_dog_kernel", DIFF))
            for t, r in tiles.items() for s in ("band", "dense")}


@pytest.fixture(scope="module")
def census():
    if not os.path.exists(isa_census.LIB):
        pytest.skip("libmustache_hip.so is not built")
    if not os.path.exists(isa_census.OBJDUMP):
        pytest.skip("no llvm-objdump in this ROCm installation")
    return {title: (rmax, cases) for title, rmax, cases in isa_census.window_loads()}


def test_every_radius_case_of_every_blur_kernel_is_found(census):
    assert set(census) == set(EXPECTED)
    for title, (rmax, cases) in census.items():
        assert rmax == EXPECTED[title]
        assert sorted(cases) == list(range(1, rmax + 1)), title
        for r, passes in cases.items():
            assert len(passes) == len(isa_census.PASSES)


@pytest.mark.parametrize("title", sorted(EXPECTED))
def test_no_pass_reads_its_window_in_8_byte_pairs(census, title):
    rmax, cases = census[title]
    for r in range(1, rmax + 1):
        for name, (reads, _) in zip(isa_census.PASSES, cases[r]):
            pairs = {op: n for op, n in reads.items() if op.startswith("ds_read2") or op == "ds_read_b64"}
            assert not pairs, "%s, radius %d, %s: %r" % (title, r, name, pairs)
            assert reads["ds_read_b128"] > 0, "%s, radius %d, %s: %r" % (title, r, name, dict(reads))
