"""Trans rows of a `.pairs` file: the host reader with keep_trans (csrc/pairs_reader.cpp through mustache_amd/pairs.py) against the
restatement (tests/pairs_trans_reference.py), the handle cache, the new symbols and what both command lines refuse around
--pairs-trans.  No GPU."""
import gzip
import os
import re

import numpy as np
import pytest

import pairs_reference as pr
import pairs_trans_reference as ptr
from test_pairs_reference import HEADER, LENGTH, _gz_copies, _rows, _text


def _trans_rows():
    """the cis rows of test_pairs_reference (they must come out unchanged) with trans rows in between: both orientations of a
    pair, every pair of the table but one, `chrM`, out of range on either side alone, beyond int32, signs and leading zeros"""
    rows = _rows()
    trans = [("chr1", 10, "chr2", 20), ("chr2", 30, "chr1", 40), ("chr2", 31, "chr1", 41), ("chr1", 11, "chr2", 21),
             ("chr1", 5, "chrM", 6), ("chrM", 5, "chr2", 6), ("chrM", 1, "chrUn", 2),
             ("chr1", LENGTH + 1, "chr2", 500), ("chr2", 500, "chr1", LENGTH + 1),              # the a side only
             ("chr1", LENGTH, "chr2", 501), ("chr2", 501, "chr1", LENGTH), ("chr1", 0, "chr2", 0),  # the b side only; both
             ("chr1", 1, "chr2", 1), ("chr1", LENGTH, "chr2", 500),                             # the edges, in range when 1-based
             ("chr3", 99999999999, "chr1", 7), ("chr1", 7, "chr3", 2147483648), ("chr3", 2147483647, "chr2", "+12"),
             ("chrE", "0012", "chr3", -5), ("chr3", 300, "chrE", 300), ("chrE", 299, "chr1", 1000), ("chr2", 3, "chr3", 4)]
    out = []
    for k, r in enumerate(rows):
        out.append(r)
        if k % 2 == 0 and trans:
            out.append(trans.pop(0))
    return out + trans


FILES = {
    "header": _text(_trans_rows()),
    "columns": _text(_trans_rows(), columns=["readID", "pos2", "chr2", "mapq", "strand1", "chr1", "pos1"]),
    "blanks": _text(_trans_rows(), sep="  "),
    "crlf_blank_lines": _text(_trans_rows(), eol="\r\n").replace("r7\t", "\r\n\r\nr7\t") + "\n\n#a comment behind the data\n",
    "no_final_newline": _text(_trans_rows())[:-1],
    "only_header": HEADER,
}


def _read(path, zero_based, threads=0, chunk_bytes=0):
    from mustache_amd.pairs import PairsFile
    with PairsFile(path, zero_based, threads=threads, chunk_bytes=chunk_bytes, keep_trans=True) as h:
        pa, pb, seg, oor = h.trans_rows()
        cis = [tuple(np.array(t) if isinstance(t, np.ndarray) else t for t in h.rows(i)) for i in range(len(h.chromosomes()))]
        return {"a": pa.copy(), "b": pb.copy(), "seg": seg, "oor": oor, "trans": h.trans_counters(), "counters": h.counters(),
                "chromosomes": h.chromosomes(), "cis": cis}


def _same(x, y):
    assert np.array_equal(x["a"], y["a"]) and np.array_equal(x["b"], y["b"]) and np.array_equal(x["seg"], y["seg"])
    assert np.array_equal(x["oor"], y["oor"]) and x["trans"] == y["trans"] and x["counters"] == y["counters"]


@pytest.mark.parametrize("zero_based", [False, True])
@pytest.mark.parametrize("name", sorted(FILES))
def test_the_reader_keeps_trans_rows_as_the_restatement_does(tmp_path, name, zero_based):
    from mustache_amd.pairs import PairsFile
    plain, one, two = _gz_copies(tmp_path, name, FILES[name])
    want = ptr.parse_trans(plain, zero_based)
    got = _read(plain, zero_based)
    assert got["a"].dtype == got["b"].dtype == np.int32 and got["seg"].dtype == got["oor"].dtype == np.int64
    P = len(want["rows"])
    assert P == 6 and got["seg"].shape == (P + 1,) and got["oor"].shape == (P,)
    assert np.array_equal(got["seg"], want["seg_off"]) and np.array_equal(got["oor"], want["out_of_range"])
    for p, pair in enumerate(ptr.pair_list(4)):                 # file order within the pair, the position on a first
        s, e = got["seg"][p], got["seg"][p + 1]
        assert np.array_equal(got["a"][s:e], want["rows"][pair][0]) and np.array_equal(got["b"][s:e], want["rows"][pair][1]), pair
    assert got["trans"] == want["counters"]
    assert got["trans"]["stored"] + got["trans"]["unknown"] == got["counters"]["trans"] == want["trans"]
    # every existing counter and the cis arrays: those of a handle opened the old way, and of the cis restatement
    old = pr.parse_pairs(plain, zero_based)
    assert got["counters"] == old["counters"] and got["chromosomes"] == old["chromosomes"]
    with PairsFile(plain, zero_based) as h:
        assert h.counters() == got["counters"]
        for i, (cname, _) in enumerate(h.chromosomes()):
            p1, p2, oor = h.rows(i)
            assert np.array_equal(p1, got["cis"][i][0]) and np.array_equal(p2, got["cis"][i][1]) and oor == got["cis"][i][2]
            assert np.array_equal(p1, old["rows"][cname][0])
    for path in (plain, one, two):
        for threads, chunk in ((1, 0), (3, 0), (1, 64), (3, 64)):
            _same(got, _read(path, zero_based, threads, chunk))
    if name == "header":
        assert want["counters"]["unknown"] == 4 and want["counters"]["stored"] == 20          # with the three trans rows of _rows()
        assert want["seg_off"][1] - want["seg_off"][0] == 13 and want["rows"][(0, 1)][0][:4].tolist() == [10, 40, 41, 11]
        assert want["rows"][(0, 3)][0].tolist() == [7, 7] and want["rows"][(0, 3)][1].tolist() == [-2 ** 31] * 2     # beyond int32
        assert want["out_of_range"].tolist() == ([5, 0, 2, 0, 0, 1] if not zero_based else [5, 1, 2, 0, 1, 2])
    if name == "only_header":
        assert got["seg"].tolist() == [0] * 7 and len(got["a"]) == 0


def test_many_rows_any_threads_any_chunks(tmp_path):
    rng = np.random.default_rng(11)
    names = ["chr1", "chr2", "chrE", "chr3", "chrM"]
    rows = [(names[int(rng.integers(0, 5))], int(rng.integers(-3, 1100)), names[int(rng.integers(0, 5))], int(rng.integers(-3, 1100)))
            for _ in range(4000)]
    plain, one, two = _gz_copies(tmp_path, "many", _text(rows))
    for zero_based in (False, True):
        want = ptr.parse_trans(plain, zero_based)
        base = _read(plain, zero_based, 1)
        assert np.array_equal(base["seg"], want["seg_off"]) and np.array_equal(base["oor"], want["out_of_range"])
        assert np.array_equal(base["a"], np.concatenate([want["rows"][p][0] for p in ptr.pair_list(4)]))
        assert np.array_equal(base["b"], np.concatenate([want["rows"][p][1] for p in ptr.pair_list(4)]))
        assert base["trans"] == want["counters"] and base["trans"]["unknown"] > 0 and base["trans"]["out_of_range"] > 0
        for path in (plain, one, two):
            for threads, chunk in ((3, 0), (1, 97), (3, 97), (3, 7), (1, 64)):
                _same(base, _read(path, zero_based, threads, chunk))


def test_what_the_reader_refuses(tmp_path):
    from mustache_amd.hicfile import HicError
    from mustache_amd.pairs import PairsFile
    for name, text in (("no_header", _text(_trans_rows(), header="")), ("empty", ""), ("comment", "## pairs format v1.0\n")):
        for path in _gz_copies(tmp_path, name, text):
            with pytest.raises(HicError, match="#chromsize") as e:
                PairsFile(path, keep_trans=True)
            assert e.value.code == -3                              # MST_IO_E_FORMAT
            PairsFile(path).close()                                # the old way still opens it
    p = tmp_path / "h.pairs"
    p.write_text(FILES["header"])
    with PairsFile(str(p)) as h:
        assert not h.keep_trans
        for call in (h.trans_rows, h.trans_counters):
            with pytest.raises(HicError, match="keep_trans") as e:
                call()
            assert e.value.code == -1                              # MST_IO_E_ARG


def test_the_handle_cache_parses_once_more_for_trans_rows(tmp_path):
    from mustache_amd import pairs
    p = tmp_path / "c.pairs"
    p.write_text(FILES["header"])
    pairs.close_pairs_handles()
    before = pairs.PairsFile.OPENS
    h = pairs.pairs_handle(str(p))
    assert not h.keep_trans and pairs.PairsFile.OPENS == before + 1
    t = pairs.pairs_handle(str(p), keep_trans=True)
    assert t.keep_trans and t is not h and pairs.PairsFile.OPENS == before + 2
    assert pairs.pairs_handle(str(p), keep_trans=True) is t and pairs.pairs_handle(str(p)) is t      # a cis request reuses it
    assert pairs.pairs_handle(str(p), False) is t and pairs.list_chromosomes(str(p)) == ["chr1", "chr2", "chrE", "chr3"]
    assert pairs.PairsFile.OPENS == before + 2
    z = pairs.pairs_handle(str(p), zero_based=True)                # the convention changes: the trans rows stay wanted
    assert z.keep_trans and pairs.PairsFile.OPENS == before + 3
    pairs.close_pairs_handles()
    # the command lines ask at the first parse: whoever opens the file first keeps the trans rows
    pairs.want_trans(str(p))
    try:
        assert pairs.pairs_handle(str(p)).keep_trans and pairs.pairs_handle(str(p), keep_trans=True) is pairs.pairs_handle(str(p))
        assert pairs.PairsFile.OPENS == before + 4
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()


def test_the_libraries_export_the_new_entry_points():
    from mustache_amd import _lib, hicfile, pairs
    new_io = {"mst_pairs_open_ex", "mst_pairs_trans_rows", "mst_pairs_trans_counters"}
    new_hip = {"mst_pairs_bin_trans", "mst_pairs_trans_compact", "mst_pairs_trans_compact_workspace_bytes", "mst_pairs_trans_decode"}
    assert new_io <= set(pairs.exported_symbols()) and new_hip <= set(_lib.exported_symbols())
    lib, hip = pairs.load(), _lib.load()
    assert all(hasattr(lib, s) for s in new_io) and all(hasattr(hip, s) for s in new_hip)
    assert lib.mst_io_abi_version() == hicfile.MST_IO_ABI_VERSION == 3 and hip.mst_abi_version() == _lib.MST_ABI_VERSION == 3
    assert hip.mst_abi_revision() == 1                              # only symbols were added
    assert hip.mst_pairs_trans_compact_workspace_bytes(5000) == 8 * 4 and hip.mst_pairs_trans_compact_workspace_bytes(0) == 8
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mustache_hip.h")).read()
    for s in new_hip:
        assert re.search(r"^MST_STABLE (?:int|uint64_t)\s+%s\s*\(" % s, hdr, flags=re.M), s
    io_hdr = open(os.path.join(root, "include", "mustache_io_pairs.h")).read()
    assert all(s + "(" in io_hdr for s in new_io)


def test_tables_and_pair_order():
    from mustache_amd.pairs import pair_list, trans_tables
    assert pair_list(4) == ptr.pair_list(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and pair_list(1) == []
    t, cells = trans_tables([99, -1, 30], [10, 7, 4])
    assert t.tolist() == [[99, 99, 1 << 31], [1 << 31, 30, 30], [10, 10, 7], [7, 4, 4], [0, 70, 110]] and cells == 138


@pytest.mark.parametrize("res", [1, 5000])
@pytest.mark.parametrize("zero_based", [False, True])
def test_the_vectorised_restatement_is_the_per_row_one(res, zero_based):
    """pair_keys (NumPy, for the GPU tests' millions of rows) against pair_pixels (a Python loop over the rows) on a 60 x 45 pair"""
    n_a, n_b = 60, 45
    len_a, len_b = (n_a - 1) * res + res // 4, (n_b - 1) * res + res // 7          # length // res + 1 = 60 and 45 bins
    rng = np.random.default_rng(17)
    pa, pb = rng.integers(1, len_a, 5000), rng.integers(1, len_b, 5000)            # [1, length - 1]: kept under both conventions
    special = [(-1, None), (None, -1),                                             # below the range on each side: dropped
               (0, None), (0, None), (0, None), (None, 0),                         # 0: dropped when positions are 1-based
               (len_a + 1, None), (None, len_b + 1),                               # above the range on each side: dropped
               (len_a, None), (None, len_b),                                       # the length itself: dropped when they are 0-based
               (-2 ** 31, None), (None, -2 ** 31),                                 # what the reader stores for a position beyond int32
               (1, 1), (len_a - 1, len_b - 1)]                                     # the edges both conventions keep
    for k, (a, b) in enumerate(special):
        row = 37 + 331 * k
        pa[row], pb[row] = (pa[row] if a is None else a), (pb[row] if b is None else b)
    pix, dropped = ptr.pair_pixels(pa, pb, res, zero_based, len_a, len_b, n_a, n_b)
    cells, counts, dropped_too = ptr.pair_keys(pa, pb, res, zero_based, len_a, len_b, n_a, n_b)
    assert dropped == dropped_too == (8 if zero_based else 10)
    assert cells.dtype == counts.dtype == np.int64 and np.all(np.diff(cells) > 0)
    assert dict(zip(cells.tolist(), counts.tolist())) == {x * n_b + y: c for (x, y), c in pix.items()}
    assert int(counts.sum()) == 5000 - dropped and len(cells) > 1000


# ---- what the command lines refuse ------------------------------------------------------------------------------------------
@pytest.fixture
def inputs(tmp_path, monkeypatch):
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    p = tmp_path / "m.pairs"
    p.write_text(FILES["header"])
    g = tmp_path / "m.pairs.gz"
    g.write_bytes(gzip.compress(FILES["header"].encode()))
    bare = tmp_path / "bare.pairs"
    bare.write_text(_text(_trans_rows(), header=""))
    t = tmp_path / "map.txt"
    t.write_text("0\t5000\t3\n5000\t10000\t4\n")
    b = tmp_path / "bias.txt"
    b.write_text("1.0\n1.0\n1.0\n")
    return {"p": str(p), "g": str(g), "bare": str(bare), "t": str(t), "b": str(b), "out": str(tmp_path / "out")}


def _refused(capsys, out, *needles):
    text = capsys.readouterr().out
    assert text.count("Error:") == 1 and all(n in text for n in needles), text
    assert not any(os.path.exists(out + s) for s in ("", ".loop1", ".diffloop1", ".loop2", ".diffloop2"))


# (input, the other arguments, needles): each is refused before the file is parsed
REFUSALS = [
    ("t", ["-ch", "1", "--pairs-trans"], ("--pairs-trans", ".pairs / .pairs.gz input")),
    ("p", ["--trans-all", "--pairs-trans"], ("--pairs-trans without --balance-genome",)),
    ("p", ["-ch", "chr1", "-ch2", "chr2", "--pairs-trans"], ("--pairs-trans without --balance-genome",)),
    ("p", ["-ch", "chr1", "--pairs-trans", "--balance-genome", "ICE"], ("--pairs-trans", "no inter-chromosomal pair")),
    ("p", ["-ch", "chr1", "--pairs-trans", "--balance", "ICE"], ("--pairs-trans", "no inter-chromosomal pair")),
    ("p", ["-ch", "chr1", "-ch2", "chr1", "--pairs-trans", "--balance-genome", "ICE"], ("--pairs-trans", "no inter-chromosomal pair")),
    ("p", ["--trans-all", "--pairs-trans", "--balance-genome", "ICE", "--balance", "ICE"], ("--pairs-trans with --balance",)),
    ("g", ["--trans-all", "--pairs-trans", "--balance-genome", "NEWTON", "-norm", "KR"], ("--pairs-trans with --balance", "-norm")),
    ("p", ["--trans-all", "--pairs-trans", "--balance-genome", "NEWTON", "-b", "{b}"], ("--pairs-trans with --balance",)),
    # without the flag the three pinned refusals say what is missing
    ("p", ["--trans-all", "--balance-genome", "ICE"], ("--trans-all", "without --pairs-trans only intra-chromosomal loops")),
    ("g", ["-ch", "chr1", "-ch2", "chr2", "--balance-genome", "ICE"], ("--balance-genome", "without --pairs-trans only intra-chromosomal")),
    ("p", ["-ch", "chr1", "-ch2", "chr2", "--balance", "ICE"], ("-ch2", "without --pairs-trans only intra-chromosomal loops")),
]


@pytest.mark.parametrize("which,extra,needles", REFUSALS)
def test_one_sample_refusals_write_nothing(inputs, capsys, which, extra, needles):
    from mustache_amd import pairs
    from mustache_amd.mustache import main
    before = pairs.PairsFile.OPENS
    main(["-f", inputs[which], "-r", "100", "-o", inputs["out"]] + [e.format(b=inputs["b"]) for e in extra])
    _refused(capsys, inputs["out"], *needles)
    assert pairs.PairsFile.OPENS == before and not pairs.WANT_TRANS


@pytest.mark.parametrize("which,extra,needles", REFUSALS)
@pytest.mark.parametrize("other", ["same", "t"])
def test_two_sample_refusals_write_nothing(inputs, capsys, which, extra, needles, other):
    from mustache_amd import pairs
    from mustache_amd.diff_mustache import main
    f1 = inputs[which]
    f2 = f1 if other == "same" else inputs["t"]
    extra = [{"-b": "-b2"}.get(e, e).format(b=inputs["b"]) for e in extra]
    before = pairs.PairsFile.OPENS
    main(["-f1", f1, "-f2", f2, "-r", "100", "-o", inputs["out"]] + extra)
    _refused(capsys, inputs["out"], *needles)
    assert pairs.PairsFile.OPENS == before and not pairs.WANT_TRANS


def test_a_multi_rank_run_is_refused(inputs, capsys, monkeypatch):
    from mustache_amd import pairs, sharding
    from mustache_amd.diff_mustache import main as diff_main
    from mustache_amd.mustache import main
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))          # what torchrun's WORLD_SIZE=2 would make it return
    monkeypatch.setenv("WORLD_SIZE", "2")
    before = pairs.PairsFile.OPENS
    main(["-f", inputs["p"], "-r", "100", "-o", inputs["out"], "--trans-all", "--pairs-trans", "--balance-genome", "ICE"])
    _refused(capsys, inputs["out"], "--pairs-trans in a multi-rank run", "world size 2")
    diff_main(["-f1", inputs["p"], "-f2", inputs["g"], "-r", "100", "-o", inputs["out"], "--trans-all", "--pairs-trans",
               "--balance-genome", "ICE"])
    _refused(capsys, inputs["out"], "--pairs-trans in a multi-rank run", "world size 2")
    assert pairs.PairsFile.OPENS == before


def test_a_file_without_a_table_is_refused_after_its_parse(inputs, capsys):
    from mustache_amd import pairs
    from mustache_amd.diff_mustache import main as diff_main
    from mustache_amd.mustache import main
    try:
        for extra in (["--trans-all"], ["-ch", "chr1", "-ch2", "chr2"]):
            main(["-f", inputs["bare"], "-r", "100", "-o", inputs["out"], "--pairs-trans", "--balance-genome", "ICE"] + extra)
            _refused(capsys, inputs["out"], "#chromsize")
        diff_main(["-f1", inputs["p"], "-f2", inputs["bare"], "-r", "100", "-o", inputs["out"], "--pairs-trans", "--balance-genome",
                   "ICE", "--trans-all"])
        _refused(capsys, inputs["out"], "#chromsize")
    finally:
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
