"""The host side of the genome thinning (mustache_amd/downsample.py: pair_tag and the trans draw) against its NumPy restatement
(tests/downsample_genome_reference.py).  No GPU."""
import zlib

import numpy as np
import pytest

import downsample_genome_reference as gref
import downsample_reference as ref


def test_pair_tag_is_the_restatements_and_ignores_the_order_and_the_prefix():
    from mustache_amd.downsample import pair_tag
    tag, swap = pair_tag("chr2", "chr10")
    other, other_swap = pair_tag("10", "2")
    assert tag == other == zlib.crc32(b"10\t2") and (swap, other_swap) == (1, 0)
    for a, b in (("chr2", "chr10"), ("10", "2"), ("X", "chrY"), ("chr1", "MT"), ("scaffold_12", "scaffold_2"), ("é", "z")):
        assert pair_tag(a, b) == gref.pair_tag(a, b)
        assert pair_tag(a, b)[0] == pair_tag(b, a)[0] and pair_tag(a, b)[1] + pair_tag(b, a)[1] == 1


@pytest.mark.parametrize("first,second", [("10", "2"), ("X", "Y"), ("2", "X"), ("1", "chr10"), ("chrM", "X")])
def test_the_orientation_follows_the_stripped_names_bytes(first, second):
    from mustache_amd.downsample import pair_tag
    want = zlib.crc32(gref.stripped(first) + b"\t" + gref.stripped(second))
    assert pair_tag(first, second) == (want, 0) and pair_tag(second, first) == (want, 1)
    assert pair_tag("chr" + gref.stripped(second).decode(), first) == (want, 1)


@pytest.mark.parametrize("a,b", [("chr1", "1"), ("X", "X"), ("chrchr2", "chr2")])
def test_equal_stripped_names_raise(a, b):
    from mustache_amd.downsample import DownsampleError, pair_tag
    if gref.stripped(a) != gref.stripped(b):                  # `chrchr2` loses one prefix only: another chromosome than `chr2`
        assert pair_tag(a, b)[0] == gref.pair_tag(a, b)[0]
        return
    with pytest.raises(DownsampleError, match="same name"):
        pair_tag(a, b)
    with pytest.raises(ValueError):
        gref.pair_tag(a, b)


def test_a_trans_draw_differs_from_the_cis_draw_of_the_same_counter():
    """the key words 2 and 3 keep the trans streams apart from every cis stream, whatever the tags"""
    x, y = np.arange(200), np.arange(200) + 3
    counts = np.full(200, 9, np.int64)
    tag = ref.chromosome_tag("chr1")
    for sample in (0, 1):
        cis = ref.thin_counts(x, y, counts, tag, 1 << 31, seed=7, sample=sample)
        trans = ref.thin_counts(x, y, counts, tag, 1 << 31, seed=7, sample=sample + 2)
        assert not np.array_equal(cis, trans)
        u_cis, u_trans = ref.draws(5, 8, 16, tag, 7, sample), ref.draws(5, 8, 16, tag, 7, sample + 2)
        assert not np.any(u_cis == u_trans)
    # thin_trans is that draw with the pair's tag, the bin on the first chromosome leading
    k = gref.thin_trans(x, y, counts, "chr2", "chr10", 1 << 31, seed=7, sample=1)
    assert np.array_equal(k, ref.thin_counts(y, x, counts, zlib.crc32(b"10\t2"), 1 << 31, seed=7, sample=3))
    assert np.array_equal(k, gref.thin_trans(y, x, counts, "10", "2", 1 << 31, seed=7, sample=1))


def test_threshold_sentences_name_the_flag():
    from mustache_amd.downsample import DownsampleError, threshold_of
    assert threshold_of(0.5, "--downsample-genome") == threshold_of(0.5) == 1 << 31
    with pytest.raises(DownsampleError, match=r"^--downsample-genome 1\.5: the fraction to keep must lie strictly between 0 and 1$"):
        threshold_of(1.5, "--downsample-genome")
    with pytest.raises(DownsampleError, match=r"^--downsample-genome 1e-10: the fraction is below 2\^-32, nothing would be kept$"):
        threshold_of(1e-10, "--downsample-genome")


def test_thin_genome_of_the_restatement():
    """the restatement on a small genome: totals add up, `inter` leaves the cis matrices alone, the dropped pixels are the
    ones with k = 0"""
    import balance_genome_reference as gr
    bins, names = (30, 20), ["chr1", "chr2"]
    cis, trans = gr.synth_genome(bins, thinned=(3,))
    n_cis, n_trans = gref.depth(names, bins, cis, trans)
    tc, tt, ((ck, ci), (tk, ti)) = gref.thin_genome(names, bins, cis, trans, 1 << 31, seed=7)
    assert (ci, ti) == (n_cis, n_trans) and 0 < ck < ci and 0 < tk < ti
    assert ck == sum(int(v.sum()) for _, _, v in tc.values()) and tk == sum(int(v.sum()) for _, _, v in tt.values())
    assert all((v > 0).all() for _, _, v in tt.values()) and len(tt[(0, 1)][2]) < len(trans[(0, 1)][2])
    ic, it, ((ick, ici), (itk, iti)) = gref.thin_genome(names, bins, cis, trans, 1 << 31, seed=7, pixels="inter")
    assert (ick, ici) == (0, 0) and (itk, iti) == (tk, ti) and ic[0] is cis[0]
    assert gref.depth(names, bins, cis, trans, "inter") == (0, n_trans)
    assert gref.line(1, ((ck, ci), (tk, ti)), 1 << 31, 7) == \
        "downsample genome (sample 2): %d of %d contacts kept (cis %d of %d, trans %d of %d), p = 0.5, seed 7" \
        % (ck + tk, ci + ti, ck, ci, tk, ti)
