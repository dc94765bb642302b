"""The NumPy restatement of the thinning rule (tests/downsample_reference.py) on its own, and the host helpers of
mustache_amd/downsample.py that turn --downsample and --match-depth into the threshold T.  No GPU."""
import zlib

import numpy as np
import pytest

import downsample_reference as ref

# counter, key, output: Philox4x32-10 known answers
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answers(counter, key, want):
    got = ref.philox4x32_10(*counter, *key)
    assert tuple(int(w) for w in got) == want


def test_known_answers_as_one_array():
    got = ref.philox4x32_10(*(np.array([c[0][i] for c in KAT]) for i in range(4)), *(np.array([c[1][i] for c in KAT]) for i in range(2)))
    for i, (_, _, want) in enumerate(KAT):
        assert tuple(int(w[i]) for w in got) == want


def test_k_is_at_most_n_and_grows_with_n():
    """u_0 .. u_{n-1} are a prefix of u_0 .. u_n: a property of the addressing by (x, y, j)"""
    tag = ref.chromosome_tag("chr7")
    for T in (1, 1 << 31, (1 << 32) - 1):
        n = np.arange(0, 70)
        k = ref.thin_counts(np.full(len(n), 12345), np.full(len(n), 12399), n, tag, T, seed=3, sample=1)
        assert (k <= n).all() and (k >= 0).all() and k[0] == 0
        assert (np.diff(k) >= 0).all() and (np.diff(k) <= 1).all()
    u = ref.draws(12345, 12399, 69, tag, 3, 1)
    assert np.array_equal(ref.draws(12345, 12399, 42, tag, 3, 1), u[:42])
    assert np.array_equal(np.cumsum(u < np.uint64(1 << 31))[[0, 3, 4, 41, 68]],
                          ref.thin_counts([12345] * 5, [12399] * 5, [1, 4, 5, 42, 69], tag, 1 << 31, seed=3, sample=1))


def test_the_largest_threshold_keeps_all_but_the_all_ones_draws():
    tag = ref.chromosome_tag("X")
    x = np.arange(3000)
    n = np.full(3000, 37)
    k = ref.thin_counts(x, x + 5, n, tag, (1 << 32) - 1)
    lost = np.array([int((ref.draws(a, a + 5, 37, tag, 0, 0) == np.uint64(0xFFFFFFFF)).sum()) for a in x[:50]])
    assert np.array_equal(k[:50], 37 - lost)
    assert int(k.sum()) >= 3000 * 37 - 1                      # 111 000 draws: one equal to 2^32 - 1 has probability 2.6e-5


def test_a_million_unit_pixels_at_one_half():
    x = np.arange(1000000) % 190000
    y = x + np.arange(1000000) // 190000
    k = ref.thin_counts(x, y, np.ones(1000000, np.int64), ref.chromosome_tag("chr1"), 1 << 31, seed=20261020)
    assert set(np.unique(k)) <= {0, 1}
    assert abs(int(k.sum()) - 500000) <= 2500                  # 5 standard deviations of Binomial(10^6, 1/2)


def test_tag_seed_and_sample_change_the_draws():
    base = ref.draws(5, 9, 64, ref.chromosome_tag("chr1"), 0, 0)
    assert not np.array_equal(base, ref.draws(5, 9, 64, ref.chromosome_tag("chr2"), 0, 0))
    assert not np.array_equal(base, ref.draws(5, 9, 64, ref.chromosome_tag("chr1"), 1, 0))
    assert not np.array_equal(base, ref.draws(5, 9, 64, ref.chromosome_tag("chr1"), 0, 1))
    assert not np.array_equal(base, ref.draws(9, 5, 64, ref.chromosome_tag("chr1"), 0, 0))


# ---- the helpers of mustache_amd/downsample.py ------------------------------------------------------------------------------
def test_the_tag_is_the_crc_of_the_name_without_a_leading_chr():
    from mustache_amd import downsample
    assert downsample.chromosome_tag("chr1") == downsample.chromosome_tag("1") == zlib.crc32(b"1") == ref.chromosome_tag("chr1")
    assert downsample.chromosome_tag(1) == zlib.crc32(b"1")
    assert downsample.chromosome_tag("chrX") == zlib.crc32(b"X") != downsample.chromosome_tag("Xchr")
    assert downsample.chromosome_tag("Xchr") == zlib.crc32(b"Xchr")       # only a leading `chr` is removed


def test_threshold_of_a_fraction():
    from mustache_amd.downsample import DownsampleError, threshold_of
    assert threshold_of(0.5) == 1 << 31 == ref.threshold_of(0.5)
    assert threshold_of(0.25) == 1 << 30 and threshold_of(2.0 ** -32) == 1
    for p in (0.1, 0.3, 0.999999, 1e-7, 1 - 2.0 ** -40):
        assert threshold_of(p) == int(p * 4294967296) == ref.threshold_of(p) and 0 < threshold_of(p) < 1 << 32
    for p in (0.0, 1.0, -0.5, 1.5, float("nan"), 2.0 ** -33):           # the last one gives T = 0
        with pytest.raises(DownsampleError):
            threshold_of(p)


def test_the_match_depth_quotient():
    from mustache_amd.downsample import match_depth, match_threshold
    assert match_depth(100, 100) == (None, None) == ref.match_depth(100, 100)
    assert match_depth(1, 2) == (None, 1 << 31) and match_depth(2, 1) == (1 << 31, None)
    for n1, n2 in ((1234567, 2469000), (2469000, 1234567), (3, 10 ** 12), (10 ** 12 - 1, 10 ** 12), (0, 5)):
        t1, t2 = match_depth(n1, n2)
        assert (t1, t2) == ref.match_depth(n1, n2)
        small, large = min(n1, n2), max(n1, n2)
        T = t2 if n1 < n2 else t1
        assert (t1 if n1 < n2 else t2) is None and T == (small << 32) // large == match_threshold(small, large) and 0 <= T < 1 << 32
    with pytest.raises(ValueError):
        match_threshold(5, 5)


def test_the_seed_is_a_uint32():
    from mustache_amd.downsample import DownsampleError, check_seed
    assert check_seed(0) == 0 and check_seed((1 << 32) - 1) == (1 << 32) - 1
    for s in (-1, 1 << 32):
        with pytest.raises(DownsampleError):
            check_seed(s)


def test_heavy_mirrors_the_header():
    import os
    import re
    from mustache_amd import downsample
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mustache_hip.h")).read()
    assert int(re.search(r"^#define MST_THIN_HEAVY (\d+)$", hdr, flags=re.M).group(1)) == downsample.HEAVY
