"""The genome thinning on the MI355X (`--downsample-genome`, `--match-depth-genome`): mst_thin_pairs (csrc/mst_thin_pairs.hip)
against the NumPy restatement (tests/downsample_genome_reference.py) bit for bit, balance_genome's read / thin / solve phases,
and both command lines end to end against the flagless run on a file written from the restatement-thinned contacts."""
import gzip
import os

import numpy as np
import pytest

import balance_genome_reference as gr
import downsample_genome_reference as gref
import downsample_reference as ref
import pairs_trans_reference as ptr
import trans_reference as tr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

RES = 10000
NAMES = ["1", "2", "3"]
HEAVY = 256
SUFFIXES = (".loop1", ".diffloop1", ".loop2", ".diffloop2")

# ---- a. the kernel against the restatement ---------------------------------------------------------------------------------------
LENGTHS = [0, 1, 63, 300, 0, 700]             # boundaries inside a wave and inside a workgroup, an empty first and middle pair
PAIRS = [("2", "10"), ("chr1", "2"), ("X", "3"), ("1", "chr3"), ("Y", "X"), ("4", "5")]       # swap on pairs 0, 2 and 4
VALUES = [0, 1, 3, 4, 5, HEAVY - 1, HEAVY, HEAVY + 1, 1000]
T0, SEED = (1 << 31) + 12345, 7


def _case():
    rng = np.random.default_rng(11)
    n = sum(LENGTHS)
    seg = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    x, y = rng.integers(0, 5000, n).astype(np.int32), rng.integers(0, 4000, n).astype(np.int32)
    counts = np.asarray(VALUES, np.int64)[rng.integers(0, len(VALUES), n)]
    counts[900] = 70000
    counts[363], counts[364] = HEAVY + 1, 1000          # two heavy pixels on the two sides of the boundary at 364, in one wave
    counts[0], counts[1] = HEAVY, 1000                  # and of the boundary at 1
    assert seg[4] == 364 and 364 // 64 == 363 // 64 and [gref.pair_tag(*p)[1] for p in PAIRS] == [1, 0, 1, 0, 1, 0]
    return x, y, counts, seg


def _want(x, y, counts, seg, sample=0, T=T0, seed=SEED):
    k = np.zeros(len(x), np.int64)
    totals = []
    for p, (a, b) in enumerate(PAIRS):
        s, e = int(seg[p]), int(seg[p + 1])
        k[s:e] = gref.thin_trans(x[s:e], y[s:e], counts[s:e], a, b, T, seed, sample)
        totals.append((int(counts[s:e].sum()), int(k[s:e].sum())))
    return k, totals


@pytest.fixture(scope="module")
def case():
    x, y, counts, seg = _case()
    return dict(x=x, y=y, counts=counts, seg=seg, want=_want(x, y, counts, seg))


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def _launch(x, y, counts, seg, dtype="int64", sample=0, T=T0, seed=SEED, draw=True, max_blocks=0, table=None):
    import torch
    from mustache_amd.downsample import launch_pairs, pair_tag
    table = [pair_tag(a, b) for a, b in PAIRS] if table is None else table
    k, totals, bad = launch_pairs(_dev(x), _dev(y), _dev(counts, getattr(torch, dtype)), seg, table, seed, sample + 2, T, draw, max_blocks)
    return (None if k is None else k.cpu().numpy()), totals, bad


@pytest.mark.parametrize("dtype", ["int64", "float32", "float64"])
def test_the_kernel_against_the_restatement(case, dtype):
    k, totals, bad = _launch(case["x"], case["y"], case["counts"], case["seg"], dtype)
    want_k, want_totals = case["want"]
    print("records %d, reads %d, kept %d" % (len(k), sum(t[0] for t in totals), sum(t[1] for t in totals)))
    assert np.array_equal(k, want_k) and totals == want_totals and bad is False
    assert totals[0] == totals[4] == (0, 0) and all(t[1] > 0 for p, t in enumerate(totals) if p in (2, 3, 5))


def test_the_sample_word_and_the_swap_matter(case):
    k1 = _launch(case["x"], case["y"], case["counts"], case["seg"], sample=1)[0]
    assert np.array_equal(k1, _want(case["x"], case["y"], case["counts"], case["seg"], sample=1)[0])
    assert not np.array_equal(k1, case["want"][0])
    from mustache_amd.downsample import pair_tag
    unswapped = [(pair_tag(a, b)[0], 0) for a, b in PAIRS]
    k0 = _launch(case["x"], case["y"], case["counts"], case["seg"], table=unswapped)[0]
    seg = case["seg"]
    for p in (2, 3, 5):
        same = np.array_equal(k0[seg[p]:seg[p + 1]], case["want"][0][seg[p]:seg[p + 1]])
        assert same == (p == 3 or p == 5)


def test_a_permutation_inside_each_segment(case):
    rng = np.random.default_rng(2)
    seg = case["seg"]
    perm = np.concatenate([seg[p] + rng.permutation(LENGTHS[p]) for p in range(len(LENGTHS))]).astype(np.int64)
    k, totals, bad = _launch(case["x"][perm], case["y"][perm], case["counts"][perm], seg)
    assert np.array_equal(k, case["want"][0][perm]) and totals == case["want"][1] and not bad


@pytest.mark.parametrize("max_blocks", [1, 2, 3])
def test_a_capped_grid_makes_more_trips(case, max_blocks):
    """2 workgroups of 256 records: a second and a third trip for the 1064 records"""
    k, totals, bad = _launch(case["x"], case["y"], case["counts"], case["seg"], max_blocks=max_blocks)
    assert np.array_equal(k, case["want"][0]) and totals == case["want"][1] and not bad


def test_the_sum_alone_draws_nothing(case):
    k, totals, bad = _launch(case["x"], case["y"], case["counts"], case["seg"], draw=False, T=0)
    assert k is None and not bad and totals == [(t[0], 0) for t in case["want"][1]]


@pytest.mark.parametrize("value,dtype", [(2.5, "float32"), (2.5, "float64"), (-1, "int64"), (-1.0, "float64"), (float("nan"), "float64"),
                                         (float("nan"), "float32"), (1 << 32, "int64"), (4294967296.0, "float64")])
def test_a_bad_count_sets_the_flag(case, value, dtype):
    import torch
    from mustache_amd.downsample import DownsampleError, depth_of_pairs, thin_pairs
    mixed = case["counts"].astype(np.int64 if dtype == "int64" else np.float64)
    mixed[500] = value
    k, totals, bad = _launch(case["x"], case["y"], mixed, case["seg"], dtype)
    expect = case["want"][0].copy()
    expect[500] = 0                                           # a bad count counts as 0; the others are untouched
    assert bad is True and np.array_equal(k, expect)
    want_totals = list(case["want"][1])
    want_totals[5] = (want_totals[5][0] - int(case["counts"][500]), want_totals[5][1] - int(case["want"][0][500]))
    assert totals == want_totals
    assert _launch(case["x"], case["y"], mixed, case["seg"], dtype, draw=False)[2] is True
    args = (_dev(case["x"]), _dev(case["y"]), _dev(mixed, getattr(torch, dtype)), case["seg"], PAIRS)
    with pytest.raises(DownsampleError, match="inter-chromosomal count that is not an integer"):
        thin_pairs(*args, T0)
    with pytest.raises(DownsampleError, match="inter-chromosomal count that is not an integer"):
        depth_of_pairs(*args)


@pytest.mark.parametrize("sample", [0, 1])
def test_one_unswapped_pair_is_the_cis_entry(sample):
    """swap = 0, tag = chromosome_tag(c), key1 = sample: exactly mst_thin_counts' k for (x, dist = y - x) -- one draw behind both"""
    from mustache_amd.downsample import _launch as thin_counts, chromosome_tag
    rng = np.random.default_rng(4)
    n = 1000
    x = rng.integers(0, 9000, n).astype(np.int32)
    dist = rng.integers(0, 400, n).astype(np.int32)
    counts = np.asarray(VALUES, np.int64)[rng.integers(0, len(VALUES), n)]
    counts[77] = 5000
    import torch
    xd, dd, cd = _dev(x), _dev(dist), _dev(counts)
    k_cis, total, kept = thin_counts(xd, dd, cd, "chr7", T0, SEED, sample, None, True)
    # _launch passes key1 = sample + 2: sample - 2 makes the key word the cis one
    k, totals, bad = _launch(x, x + dist, counts, [0, n], sample=sample - 2, table=[(chromosome_tag("chr7"), 0)])
    assert np.array_equal(k, k_cis.cpu().numpy()) and totals == [(total, kept)] and not bad
    assert np.array_equal(k, ref.thin_counts(x, x.astype(np.int64) + dist, counts, ref.chromosome_tag("7"), T0, SEED, sample))
    torch.cuda.synchronize()


def test_thin_pairs_and_depth_of_pairs(case):
    import torch
    from mustache_amd.downsample import DownsampleError, depth_of_pairs, thin_pairs
    args = (_dev(case["x"]), _dev(case["y"]), _dev(case["counts"]).to(torch.float64), case["seg"], PAIRS)
    k, totals = thin_pairs(*args, T0, seed=SEED, sample=0)
    assert k.dtype == torch.int64 and np.array_equal(k.cpu().numpy(), case["want"][0]) and totals == case["want"][1]
    assert depth_of_pairs(*args) == [t[0] for t in case["want"][1]]
    for T in (0, 1 << 32):
        with pytest.raises(DownsampleError):
            thin_pairs(*args, T)
    with pytest.raises(DownsampleError, match="same name"):
        thin_pairs(*args[:4], PAIRS[:5] + [("chr4", "4")], T0)


def test_the_entry_point_refuses_bad_arguments(case):
    from mustache_amd._lib import MstError
    for T in (0, 1 << 32):
        with pytest.raises(MstError, match="mst_thin_pairs"):
            _launch(case["x"], case["y"], case["counts"], case["seg"], T=T)
    with pytest.raises(MstError, match="mst_thin_pairs"):
        _launch(case["x"], case["y"], case["counts"], case["seg"], max_blocks=-1)


def test_a_library_without_the_entry_point_is_refused_by_name(monkeypatch):
    from mustache_amd import _lib
    assert "mst_thin_pairs" in _lib.exported_symbols()
    real = _lib.load()
    assert hasattr(real, "mst_thin_pairs") and real.mst_abi_revision() == _lib.MST_ABI_REVISION == 1       # added without a new revision

    class Stale:
        def __getattr__(self, name):
            if name == "mst_thin_pairs":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(ImportError, match=r"lacks symbols \['mst_thin_pairs'\] \(stale build\?\)"):
        _lib.load()


# ---- b. genome_bias with a thinning between its two phases ------------------------------------------------------------------------
BINS = (70, 50, 40)


def _lengths(bins):
    return [b * RES - 1 for b in bins]


def _write_hic(path, bins, cis, trans):
    chroms, mats = gr.hic_arguments(bins, RES, cis, trans)
    write_hic_pairs(str(path), chroms, mats, version=8)
    return str(path)


def _write_pairs(path, bins, cis, trans, seed):
    text, _ = ptr.pairs_text(NAMES, _lengths(bins), RES, cis, trans, seed)
    with open(str(path), "wb") as fh:
        fh.write(gzip.compress(text.encode(), 1) if str(path).endswith(".gz") else text.encode())
    return str(path)


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("downsample_genome")
    cis, trans = gr.synth_genome(BINS)
    out = dict(cis=cis, trans=trans, hic=_write_hic(d / "g.hic", BINS, cis, trans), pairs=_write_pairs(d / "g.pairs", BINS, cis, trans, 5))
    for pixels in ("all", "inter"):
        tc, tt, totals = gref.thin_genome(NAMES, BINS, cis, trans, 1 << 31, seed=7, sample=0, pixels=pixels)
        out[pixels] = dict(cis=tc, trans=tt, totals=totals, hic=_write_hic(d / ("thin_%s.hic" % pixels), BINS, tc, tt))
    return out


def _sorted(rec):
    x, y, v = (np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in rec)
    o = np.lexsort((y, x))
    return x[o], y[o], v[o]


@pytest.mark.parametrize("pixels", ["all", "inter"])
def test_genome_bias_with_thinning(genome, pixels, capsys):
    from mustache_amd import pairs
    from mustache_amd.balance_genome import genome_bias, genome_depth, read_genome, solve_genome, thin_genome
    from mustache_amd.mustache import genome_biases_or_error
    want = genome[pixels]
    flagless = genome_bias(want["hic"], RES, method="NEWTON", pixels=pixels)
    biases = []
    for f in (genome["hic"], genome["pairs"]):
        read = read_genome(f, RES, pixels)
        assert genome_depth(read) == gref.depth(NAMES, BINS, genome["cis"], genome["trans"], pixels)
        totals = thin_genome(read, 1 << 31, seed=7, sample=0)
        print(pixels, os.path.basename(f), totals)
        assert totals == want["totals"] and (totals[0] == (0, 0)) == (pixels == "inter")
        assert sorted(read.records) == [(0, 1), (0, 2), (1, 2)] and len(read.cis) == (3 if pixels == "all" else 0)
        for key, rec in read.records.items():
            got, exp = _sorted(rec), _sorted(want["trans"][key])
            assert all(np.array_equal(g, e) for g, e in zip(got, exp)) and 100 < len(got[2]) < len(genome["trans"][key][2])
        for c, x, d, v in read.cis:
            i, j, k = want["cis"][c]
            o, q = np.lexsort(((x + d).cpu().numpy(), x.cpu().numpy())), np.lexsort((j, i))
            assert np.array_equal(x.cpu().numpy()[o], i[q]) and np.array_equal((x + d).cpu().numpy()[o], j[q])
            assert np.array_equal(v.cpu().numpy()[o], k[q])
        gb = solve_genome(read, "NEWTON")
        assert gb.bias.tobytes() == flagless.bias.tobytes() and gb.info["records"] == flagless.info["records"]
        assert all(np.array_equal(a, b) for a, b in zip(_sorted(gb.records("3", "1")), _sorted(flagless.records("3", "1"))))
        biases.append(gb.bias)
    assert biases[0].tobytes() == biases[1].tobytes() and int(np.isfinite(biases[0]).sum()) > 100
    # through the command lines' one place, with its printed line; sample 1 draws from another stream
    capsys.readouterr()
    gbs = genome_biases_or_error([genome["hic"], genome["hic"]], RES, ("NEWTON", pixels), verbose=False, thinning=(1 << 31, 7))
    said = capsys.readouterr().out.splitlines()
    assert said.count(gref.line(0, want["totals"], 1 << 31, 7)) == 1 and gbs[0].bias.tobytes() == flagless.bias.tobytes()
    second = gref.thin_genome(NAMES, BINS, genome["cis"], genome["trans"], 1 << 31, seed=7, sample=1, pixels=pixels)
    assert said.count(gref.line(1, second[2], 1 << 31, 7)) == 1 and sum(ln.startswith("downsample genome") for ln in said) == 2
    k0, k1 = _sorted(gbs[0].records("1", "2")), _sorted(gbs[1].records("1", "2"))
    assert not (len(k0[2]) == len(k1[2]) and np.array_equal(k0[2], k1[2]))
    assert all(np.array_equal(a, b) for a, b in zip(k1, _sorted(second[1][(0, 1)])))
    assert gbs[1].bias.tobytes() != gbs[0].bias.tobytes()
    pairs.close_pairs_handles()


def test_genome_bias_itself_is_unchanged(genome):
    """read_genome + solve_genome is genome_bias: same bytes, same records"""
    from mustache_amd.balance_genome import genome_bias, read_genome, solve_genome
    whole = genome_bias(genome["hic"], RES, method="ICE", pixels="all")
    parts = solve_genome(read_genome(genome["hic"], RES, "all"), "ICE")
    assert whole.bias.tobytes() == parts.bias.tobytes() and whole.info["records"] == parts.info["records"]
    none = genome_bias(genome["hic"], RES, method="ICE", pixels="all", keep_records=False)
    assert none.bias.tobytes() == whole.bias.tobytes() and none.records("1", "2") is None


# ---- c, d. both command lines end to end ------------------------------------------------------------------------------------------
def _integer(rec, factor):
    x, y, v = rec
    return np.asarray(x), np.asarray(y), np.maximum(np.round(factor * np.asarray(v)), 1.0)


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    """s1: the calling genome of tests/test_gpu_pairs_trans.py (integer counts), checked on the CPU to keep its six planted loops
    once the restatement has thinned it with p = 0.5, seed 7.  deep / shallow: the pair of --match-depth-genome, the deep one
    with 148 977 contacts, the other with 87 350."""
    import diff_trans_reference as dr
    d = tmp_path_factory.mktemp("downsample_genome_call")
    s1 = gr.synth_call_genome(_integer(tr.synth_trans(180, 140, density=0.6, nloops=6, seed=41), 2.0), seed=7)
    deep = gr.synth_call_genome(_integer(tr.synth_trans(180, 140, density=0.6, nloops=6, seed=41), 4.0), seed=7)
    deep = ({c: (i, j, 2.0 * v) for c, (i, j, v) in deep[0].items()}, deep[1])
    shallow = gr.synth_call_genome(_integer(dr.synth_pair(180, 140, density=0.6, nloops=6, seed=41)[1], 2.0), seed=8)
    return dict(dir=d, s1=s1, deep=deep, shallow=shallow, s1_hic=_write_hic(d / "s1.hic", gr.CALL_BINS, *s1),
                s1_pairs=_write_pairs(d / "s1.pairs.gz", gr.CALL_BINS, *s1, 21), deep_hic=_write_hic(d / "deep.hic", gr.CALL_BINS, *deep),
                shallow_hic=_write_hic(d / "shallow.hic", gr.CALL_BINS, *shallow))


def _numpy_loops_01(genome):
    cis, trans = genome
    bins, off, _ = gr.layout(_lengths(gr.CALL_BINS), RES)
    bias, _ = gr.genome_bias("NEWTON", bins, off, cis, trans, "all")
    return tr.trans_loops(*gr.balanced(bias, off[0], off[1], *trans[(0, 1)]), 0.88, 0.2, [1.6, 3.2])


def test_downsample_genome_end_to_end(samples, tmp_path, capsys):
    from mustache_amd import pairs
    from mustache_amd.mustache import main
    tc, tt, totals = gref.thin_genome(NAMES, gr.CALL_BINS, *samples["s1"], 1 << 31, seed=7, sample=0)
    assert len(_numpy_loops_01((tc, tt))) == 6                       # the thinned fixture still carries its planted loops
    thinned = _write_hic(tmp_path / "thinned.hic", gr.CALL_BINS, tc, tt)
    want, one_want = tmp_path / "want.tsv", tmp_path / "one_want.tsv"
    main(["-f", thinned, "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(want)])
    main(["-f", thinned, "-r", "10kb", "-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON", "-o", str(one_want)])
    rows = open(want).read().splitlines()
    assert len(rows) >= 2 and rows[0].startswith("BIN1_CHR")          # at least one loop
    flags = ["--balance-genome", "NEWTON", "--downsample-genome", "0.5", "--seed", "7", "-r", "10kb"]
    for tag, f, extra in (("hic", samples["s1_hic"], []), ("pairs", samples["s1_pairs"], ["--pairs-trans"])):
        out = tmp_path / (tag + ".tsv")
        capsys.readouterr()
        main(["-f", f, "--trans-all", "-o", str(out)] + flags + extra)
        said = capsys.readouterr().out
        assert "Error" not in said and said.splitlines().count(gref.line(0, totals, 1 << 31, 7)) == 1
        assert open(out, "rb").read() == open(want, "rb").read(), tag
        one = tmp_path / (tag + "_one.tsv")
        main(["-f", f, "-ch", "1", "-ch2", "2", "-o", str(one)] + flags + extra)
        assert open(one, "rb").read() == open(one_want, "rb").read(), tag
        pairs.close_pairs_handles()
    assert open(one_want).read().splitlines() == [rows[0]] + [r for r in rows[1:] if r.split("\t")[0] == "1" and r.split("\t")[3] == "2"]
    assert len(open(one_want).read().splitlines()) >= 2
    # the unthinned run says something else: the flag did something
    plain = tmp_path / "plain.tsv"
    main(["-f", samples["s1_hic"], "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(plain)])
    assert open(plain, "rb").read() != open(want, "rb").read()
    pairs.WANT_TRANS.clear()
    pairs.close_pairs_handles()


def _four(prefix):
    return [open(str(prefix) + suf, "rb").read() for suf in SUFFIXES]


def test_match_depth_genome_end_to_end(samples, tmp_path, capsys):
    from mustache_amd.diff_mustache import main
    n1, n2 = (sum(gref.depth(NAMES, gr.CALL_BINS, *samples[k])) for k in ("deep", "shallow"))
    T = (n2 << 32) // n1
    assert (n1, n2) == (148977, 87350) and ref.match_depth(n1, n2) == (T, None)
    run = ["-r", "10kb", "--trans-all", "--balance-genome", "NEWTON"]
    for sample, order in ((0, ("deep", "shallow")), (1, ("shallow", "deep"))):
        tc, tt, totals = gref.thin_genome(NAMES, gr.CALL_BINS, *samples["deep"], T, seed=0, sample=sample)
        thinned = _write_hic(tmp_path / ("thinned%d.hic" % sample), gr.CALL_BINS, tc, tt)
        files = {"deep": thinned, "shallow": samples["shallow_hic"]}
        want = tmp_path / ("want%d" % sample)
        main(["-f1", files[order[0]], "-f2", files[order[1]], "-o", str(want)] + run)
        assert sum(len(b.splitlines()) - 1 for b in _four(want)) >= 1            # the comparison is not empty
        out = tmp_path / ("got%d" % sample)
        capsys.readouterr()
        main(["-f1", samples[order[0] + "_hic"], "-f2", samples[order[1] + "_hic"], "-o", str(out), "--match-depth-genome"] + run)
        said = capsys.readouterr().out.splitlines()
        assert said.count(gref.line(sample, totals, T, 0)) == 1 and sum(ln.startswith("downsample genome") for ln in said) == 1
        assert ("p = %r" % (T / 4294967296)) in gref.line(sample, totals, T, 0) and totals[0][1] + totals[1][1] == n1
        depths = (n1, n2) if sample == 0 else (n2, n1)
        assert said.count("depth of the genome: sample 1 holds %d contacts, sample 2 holds %d" % depths) == 1
        assert _four(out) == _four(want), order
    # equal depths thin neither: the flagless output, no `downsample` line
    same, flagless = tmp_path / "same", tmp_path / "flagless"
    capsys.readouterr()
    main(["-f1", samples["deep_hic"], "-f2", samples["deep_hic"], "-o", str(same), "--match-depth-genome"] + run)
    said = capsys.readouterr().out
    assert "downsample" not in said and "Error" not in said
    main(["-f1", samples["deep_hic"], "-f2", samples["deep_hic"], "-o", str(flagless)] + run)
    assert _four(same) == _four(flagless)


# ---- e. float counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["trans", "cis"])
def test_a_float_count_file_ends_with_one_error_line(genome, tmp_path, capsys, where):
    from mustache_amd.diff_mustache import main as diff_main
    from mustache_amd.mustache import main
    cis, trans = dict(genome["cis"]), dict(genome["trans"])
    if where == "trans":
        x, y, v = trans[(0, 2)]
        trans[(0, 2)] = (x, y, np.where(np.arange(len(v)) == 5, 2.5, v))
        sentence = "Error: the genome holds an inter-chromosomal count that is not an integer between 0 and 4294967295"
    else:
        i, j, v = cis[1]
        cis[1] = (i, j, np.where(np.arange(len(v)) == int(np.argmax(j - i)), 7.5, v))       # a pixel far from the diagonal: it enters
        sentence = "Error: chromosome 2 holds a count that is not an integer between 0 and 4294967295"
    f = _write_hic(tmp_path / "float.hic", BINS, cis, trans)
    out = tmp_path / "out.tsv"
    capsys.readouterr()
    main(["-f", f, "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "--downsample-genome", "0.5", "-o", str(out)])
    said = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("Error:") for ln in said) == 1 and sum(ln.startswith(sentence) for ln in said) == 1, said
    assert not out.exists()
    diff_main(["-f1", genome["hic"], "-f2", f, "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "--match-depth-genome", "-o", str(out)])
    said = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("Error:") for ln in said) == 1 and sum(ln.startswith(sentence) for ln in said) == 1, said
    assert not any(os.path.exists(str(out) + suf) for suf in ("",) + SUFFIXES)
