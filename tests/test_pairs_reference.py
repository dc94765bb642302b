"""The `.pairs` host reader (csrc/pairs_reader.cpp through mustache_amd/pairs.py) against the restatement
(tests/pairs_reference.py), and what both command lines refuse for pairs input.  No GPU."""
import gzip
import os

import numpy as np
import pytest

import pairs_reference as pr

RES = 100
LENGTH = 1000
EDGES = [0, 1, RES, RES + 1, LENGTH, LENGTH + 1]          # under both conventions: the ends of both ranges, a bin edge

HEADER = "## pairs format v1.0\n#sorted: chr1-chr2-pos1-pos2\n#shape: upper triangle\n" \
         "#chromsize: chr1 %d\n#chromsize: chr2 500\n#chromsize: chrE 300\n#chromsize: chr3 2147483647\n" % LENGTH


def _rows():
    """(readID, chr1, pos1, chr2, pos2, strand1, strand2) of the cases the issue lists"""
    rows = []
    for a in EDGES:                                         # every edge position on either side, and with pos1 > pos2
        for b in (1, 5, LENGTH):
            rows.append(("chr1", a, "chr1", b))
            rows.append(("chr1", b, "chr1", a))
    rows += [("chr1", 700, "chr1", 20), ("chr1", 20, "chr1", 700), ("chr1", 20, "chr1", 700)]
    rows += [("chr1", 10, "chr2", 20), ("chr2", 30, "chr1", 40), ("chr1", 5, "chrX", 6)]            # trans rows
    rows += [("chrX", 5, "chrX", 6), ("chrUn_1", 1, "chrUn_1", 2)]                                  # absent from the header
    rows += [("chr2", 500, "chr2", 1), ("chr2", 501, "chr2", 1), ("chr2", 499, "chr2", 250)]
    rows += [("chr3", 2147483647, "chr3", 1), ("chr3", 2147483648, "chr3", 1), ("chr3", 99999999999999999999, "chr3", 7),
             ("chr3", -5, "chr3", 7), ("chr3", "+12", "chr3", "0012")]
    return rows


def _text(rows, sep="\t", header=HEADER, columns=None, eol="\n"):
    """columns: the order of the fields of a row, named as in `#columns:` (None: the standard seven, no #columns: line)"""
    order = columns or ["readID", "chr1", "pos1", "chr2", "pos2", "strand1", "strand2"]
    out = [header]
    if columns:
        out.append("#columns: " + " ".join(columns) + "\n")
    for k, (c1, p1, c2, p2) in enumerate(rows):
        f = {"readID": "r%d" % k, "chr1": c1, "pos1": str(p1), "chr2": c2, "pos2": str(p2), "strand1": "+", "strand2": "-",
             "mapq": "60"}
        out.append(sep.join(f[c] for c in order) + eol)
    return "".join(out)


FILES = {
    "header": _text(_rows()),
    "no_header": _text(_rows(), header=""),
    "columns": _text(_rows(), columns=["readID", "pos2", "chr2", "mapq", "strand1", "chr1", "pos1"]),
    "blanks": _text(_rows(), sep="  "),
    "blank_and_tab": _text(_rows(), sep=" \t"),
    "crlf_blank_lines": _text(_rows(), eol="\r\n").replace("r7\t", "\r\n\r\nr7\t") + "\n\n#a comment behind the data\n",
    "no_final_newline": _text(_rows())[:-1],
    "only_header": HEADER,
    "empty": "",
}


def _compare(path, zero_based, threads=0, chunk_bytes=0):
    from mustache_amd.pairs import PairsFile
    want = pr.parse_pairs(path, zero_based)
    with PairsFile(path, zero_based, threads=threads, chunk_bytes=chunk_bytes) as h:
        assert h.chromosomes() == want["chromosomes"]
        assert h.counters() == want["counters"]
        c = h.counters()
        assert c["rows"] == c["kept"] + c["trans"] + c["out_of_range"] + c["unknown"]
        got = {}
        for i, (name, _) in enumerate(h.chromosomes()):
            p1, p2, oor = h.rows(i)
            assert p1.dtype == p2.dtype == np.int32
            assert np.array_equal(p1, want["rows"][name][0]) and np.array_equal(p2, want["rows"][name][1]), name
            assert oor == want["out_of_range"][name], name
            got[name] = (p1.copy(), p2.copy())
    return want, got


def _gz_copies(tmp_path, name, text):
    """the plain file, its .gz copy and a .gz of two concatenated members cut in the middle of a line"""
    data = text.encode()
    plain = tmp_path / (name + ".pairs")
    plain.write_bytes(data)
    one = tmp_path / (name + ".one.pairs.gz")
    one.write_bytes(gzip.compress(data))
    two = tmp_path / (name + ".two.pairs.gz")
    cut = len(data) // 2 + 3
    two.write_bytes(gzip.compress(data[:cut]) + gzip.compress(data[cut:]))
    return str(plain), str(one), str(two)


@pytest.mark.parametrize("zero_based", [False, True])
@pytest.mark.parametrize("name", sorted(FILES))
def test_reader_matches_the_restatement(tmp_path, name, zero_based):
    plain, one, two = _gz_copies(tmp_path, name, FILES[name])
    want, got = _compare(plain, zero_based)
    for gz in (one, two):                                   # exactly the arrays of the plain file
        _, again = _compare(gz, zero_based)
        assert set(again) == set(got)
        for k in got:
            assert np.array_equal(again[k][0], got[k][0]) and np.array_equal(again[k][1], got[k][1])
    if name == "header":
        assert [n for n, _ in want["chromosomes"]] == ["chr1", "chr2", "chrE", "chr3"]
        assert len(got["chrE"][0]) == 0                     # the empty chromosome
        assert want["counters"]["trans"] == 3 and want["counters"]["unknown"] == 2
    if name == "no_header":
        assert [n for n, _ in want["chromosomes"]][:2] == ["chr1", "chr2"] and want["counters"]["unknown"] == 0
        assert all(length == -1 for _, length in want["chromosomes"])


def test_the_edge_positions_are_judged_by_the_convention(tmp_path):
    from mustache_amd.pairs import PairsFile
    rows = [("chr1", a, "chr1", 5) for a in EDGES]
    p = tmp_path / "e.pairs"
    p.write_text(_text(rows))
    for zero_based, dropped in ((False, [0, LENGTH + 1]), (True, [LENGTH, LENGTH + 1])):
        with PairsFile(str(p), zero_based) as h:
            p1, p2, oor = h.rows(0)
            assert list(p1) == EDGES and oor == len(dropped)
        keep = pr.in_range(np.array(EDGES), np.full(len(EDGES), 5), LENGTH, zero_based)
        assert [a for a, k in zip(EDGES, keep) if not k] == dropped
    x, y, c, d = pr.pixels(EDGES, [5] * 6, RES, False, LENGTH)              # 1-based: 1 and 100 share bin 0, 101 opens bin 1
    assert list(zip(x, y, c)) == [(0, 0, 2), (0, 1, 1), (0, 9, 1)] and d == 2
    x, y, c, d = pr.pixels(EDGES, [5] * 6, RES, True, LENGTH)               # 0-based: 0 and 1 share bin 0, 100 opens bin 1
    assert list(zip(x, y, c)) == [(0, 0, 2), (0, 1, 2)] and d == 2


@pytest.mark.parametrize("bad,what", [("r\tchr1\t5\tchr1\n", "too few fields"), ("r\tchr1\t12x\tchr1\t7\t+\t-\n", "decimal integer"),
                                      ("r\tchr1\t5\tchr1\t1.5\t+\t-\n", "decimal integer"), ("r\tchr2\t\tchr1\t7\n", "too few fields"),
                                      ("r chr1 - chr1 7\n", "decimal integer")])
def test_a_malformed_line_is_an_error_that_names_the_line(tmp_path, bad, what):
    from mustache_amd.hicfile import HicError
    from mustache_amd.pairs import PairsFile
    good = _text([("chr1", 10 + k, "chr1", 20 + k) for k in range(300)])
    at = 120
    lines = good.split("\n")
    text = "\n".join(lines[:at] + [bad.rstrip("\n")] + lines[at:])
    # a second bad line further down: the first one is the one that is named, whatever the thread count
    text += "r\tchr1\tzz\tchr1\t3\n"
    number = at + 1
    with pytest.raises(pr.PairsFormatError) as ref:
        pr.parse_pairs(_gz_copies(tmp_path, "ref", text)[0])
    assert ref.value.line == number
    for path in _gz_copies(tmp_path, "bad", text):
        for threads, chunk in ((1, 0), (4, 200), (3, 64)):
            with pytest.raises(HicError) as e:
                PairsFile(path, False, threads=threads, chunk_bytes=chunk)
            assert "line %d:" % number in str(e.value) and what in str(e.value), str(e.value)
            assert e.value.code == -3


def test_a_malformed_header_is_an_error(tmp_path):
    from mustache_amd.hicfile import HicError
    from mustache_amd.pairs import PairsFile
    for text, line in (("#chromsize: chr1\nr\tchr1\t1\tchr1\t2\n", 1), ("## x\n#columns: readID chr1 pos1 chr2\nr\tchr1\t1\tchr1\t2\n", 2)):
        for path in _gz_copies(tmp_path, "h%d" % line, text):
            with pytest.raises(HicError) as e:
                PairsFile(path)
            assert "line %d:" % line in str(e.value)
            with pytest.raises(pr.PairsFormatError) as ref:
                pr.parse_pairs(path)
            assert ref.value.line == line


def test_thread_count_and_chunk_cuts_do_not_change_the_arrays(tmp_path):
    rng = np.random.default_rng(5)
    names = ["chr1", "chr2", "chrE", "chrX"]
    rows = []
    for _ in range(4000):
        c1 = names[int(rng.integers(0, 4))]
        c2 = c1 if rng.random() < 0.8 else names[int(rng.integers(0, 4))]
        rows.append((c1, int(rng.integers(-3, 1100)), c2, int(rng.integers(-3, 1100))))
    for header in (HEADER, ""):
        text = _text(rows, header=header)
        tag = "t%d" % len(header)
        plain, one, two = _gz_copies(tmp_path, tag, text)
        _, base = _compare(plain, False, threads=1)
        for path in (plain, one, two):
            for threads, chunk in ((1, 0), (4, 0), (1, 97), (4, 97), (4, 1000), (3, 7)):     # 97 bytes: every cut falls inside a line
                _, got = _compare(path, False, threads=threads, chunk_bytes=chunk)
                assert set(got) == set(base)
                for k in base:
                    assert np.array_equal(got[k][0], base[k][0]) and np.array_equal(got[k][1], base[k][1])


def test_a_header_longer_than_a_chunk(tmp_path):
    text = "".join("#chromsize: c%d %d\n" % (k, 100 + k) for k in range(200)) + _text([("c7", 5, "c7", 9), ("c3", 1, "c9", 2)], header="")
    for path in _gz_copies(tmp_path, "long", text):
        want, got = _compare(path, False, threads=2, chunk_bytes=50)
        assert len(want["chromosomes"]) == 200 and list(got["c7"][0]) == [5]


# ---- the binding ------------------------------------------------------------------------------------------------------------
def test_the_libraries_export_the_new_entry_points(monkeypatch):
    from mustache_amd import _lib, hicfile, pairs
    lib = pairs.load()
    for name in pairs.exported_symbols():
        assert hasattr(lib, name), name
    assert lib.mst_io_abi_version() == hicfile.MST_IO_ABI_VERSION == 3                   # only symbols were added
    assert {"mst_pairs_bin", "mst_pairs_compact", "mst_pairs_compact_workspace_bytes"} <= set(_lib.exported_symbols())
    hip = _lib.load()
    assert hasattr(hip, "mst_pairs_bin") and hip.mst_abi_version() == _lib.MST_ABI_VERSION == 3
    assert hip.mst_pairs_compact_workspace_bytes(3, 2048) == 8 * 4 and hip.mst_pairs_compact_workspace_bytes(0, 5) == 8
    # a library from before the reader: refused by the symbols it lacks
    monkeypatch.setattr(pairs, "_bound", None)
    monkeypatch.setitem(pairs._SIGNATURES, "mst_pairs_of_tomorrow", (None, []))
    with pytest.raises(ImportError, match=r"lacks symbols \['mst_pairs_of_tomorrow'\]"):
        pairs.load()


def test_dense_diagonals_and_the_far_list_sum():
    from mustache_amd.pairs import dense_diagonals, is_pairs
    assert dense_diagonals(50000, 400, 1 << 40) == 401                 # D + 1
    assert dense_diagonals(70, 400, 1 << 40) == 70                     # n
    assert dense_diagonals(50000, 400, 4 * 50000 * 3 + 7) == 3         # budget // (4 n)
    assert dense_diagonals(50000, 400, 100) == 0                       # K = 0 is legal
    assert is_pairs("a.pairs") and is_pairs("b/c.pairs.gz") and not is_pairs("a.pairs.txt") and not is_pairs("a.hic")


def test_the_handle_is_cached_per_path(tmp_path):
    from mustache_amd import pairs
    from mustache_amd.request import chromosome_pairs
    p = tmp_path / "c.pairs"
    p.write_text(FILES["header"])
    q = tmp_path / "d.pairs"
    q.write_text(FILES["no_header"])
    pairs.close_pairs_handles()
    before = pairs.PairsFile.OPENS
    assert chromosome_pairs(str(p), RES, 'n', 'n') == [(c, c) for c in ("chr1", "chr2", "chrE", "chr3")]      # header order
    h = pairs.pairs_handle(str(p))
    assert pairs.pairs_handle(str(p)) is h and pairs.pairs_handle(str(q)) is not h and pairs.pairs_handle(str(p)) is h
    assert pairs.PairsFile.OPENS == before + 2
    assert h.index("1") == 0 and h.index("chr2") == 1 and h.index("chrE") == 2 and h.index("7") is None
    assert pairs.pairs_handle(str(p), zero_based=True) is not h and pairs.PairsFile.OPENS == before + 3
    pairs.close_pairs_handles()
    assert chromosome_pairs(str(p), RES, ["chr2"], 'n') == [("chr2", "chr2")] and pairs.PairsFile.OPENS == before + 3
    bad = tmp_path / "bad.pairs"
    bad.write_text("r\tchr1\tx\tchr1\t2\n")
    assert chromosome_pairs(str(bad), RES, 'n', 'n').startswith("Error:") and "line 1:" in chromosome_pairs(str(bad), RES, 'n', 'n')


# ---- what the command lines refuse ------------------------------------------------------------------------------------------
@pytest.fixture
def inputs(tmp_path, monkeypatch):
    from mustache_amd import _lib

    def no_gpu():
        raise AssertionError("a refused run touched the GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    p = tmp_path / "m.pairs"
    p.write_text(FILES["header"])
    g = tmp_path / "m.pairs.gz"
    g.write_bytes(gzip.compress(FILES["header"].encode()))
    t = tmp_path / "map.txt"
    t.write_text("0\t5000\t3\n5000\t10000\t4\n")
    b = tmp_path / "bias.txt"
    b.write_text("1.0\n1.0\n1.0\n")
    return str(p), str(g), str(t), str(b), str(tmp_path / "out")


def _refused(capsys, out, *needles):
    text = capsys.readouterr().out
    assert "Error:" in text and all(n in text for n in needles), text
    assert not any(os.path.exists(out + s) for s in ("", ".loop1", ".diffloop1", ".loop2", ".diffloop2"))


REFUSALS = [
    (["-ch", "chr1"], ("raw read pairs", "--balance ICE|NEWTON")),
    (["-ch", "chr1", "-b", "{b}"], ("raw read pairs", "--balance ICE|NEWTON")),
    (["-ch", "chr1", "--balance", "ICE", "-b", "{b}"], ("--balance ICE and -b",)),
    (["-ch", "chr1", "--balance", "NEWTON", "-norm", "KR"], ("-norm KR",)),
    (["-ch", "chr1", "-ch2", "chr2", "--balance", "ICE"], ("-ch2", "intra-chromosomal")),
    (["-ch", "chr1", "chr2", "--trans-all"], ("--trans-all", "intra-chromosomal")),
    (["--trans-all", "--balance-genome", "ICE"], ("--trans-all", "intra-chromosomal")),
    (["-ch", "chr1", "-ch2", "chr2", "--balance-genome", "ICE"], ("--balance-genome", "intra-chromosomal")),
]


@pytest.mark.parametrize("extra,needles", REFUSALS)
@pytest.mark.parametrize("gz", [False, True])
def test_one_sample_refusals_write_nothing(inputs, capsys, extra, needles, gz):
    from mustache_amd import pairs
    from mustache_amd.mustache import main
    p, g, _t, b, out = inputs
    before = pairs.PairsFile.OPENS
    main(["-f", g if gz else p, "-r", "100", "-o", out] + [e.format(b=b) for e in extra])
    _refused(capsys, out, *needles)
    assert pairs.PairsFile.OPENS == before                  # refused before the file is parsed


@pytest.mark.parametrize("extra,needles", REFUSALS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_two_sample_refusals_write_nothing(inputs, capsys, extra, needles, which):
    from mustache_amd.diff_mustache import main
    p, g, t, b, out = inputs
    f1, f2 = [(p, g), (p, t), (t, g)][which]               # a pairs file as either sample
    extra = [{"-b": "-b2"}.get(e, e).format(b=b) for e in extra]
    needles = tuple("-b1/-b2" if n == "--balance ICE and -b" else n for n in needles)
    main(["-f1", f1, "-f2", f2, "-r", "100", "-o", out] + extra)
    _refused(capsys, out, *needles)


def test_zero_based_needs_a_pairs_file(inputs, capsys):
    from mustache_amd.diff_mustache import main as diff_main
    from mustache_amd.mustache import main
    _p, _g, t, _b, out = inputs
    main(["-f", t, "-r", "5000", "-ch", "1", "-o", out, "--pairs-zero-based"])
    _refused(capsys, out, "--pairs-zero-based")
    diff_main(["-f1", t, "-f2", t, "-r", "5000", "-ch", "1", "-o", out, "--pairs-zero-based"])
    _refused(capsys, out, "--pairs-zero-based")


def test_the_library_calls_refuse_pairs_without_balance(inputs):
    from mustache_amd.mustache import read_sample
    from mustache_amd.pairs import PairsError
    with pytest.raises(PairsError, match="raw read pairs"):
        read_sample(inputs[0], False, False, 100, 20000, False, "chr1")


def write_sanitizer_files(directory):
    """The files scripts/pairs_sanitize_main.cpp reads: every layout above as a plain file, a .gz copy and a two-member .gz
    (`good_*`), a few thousand rows for the chunk cuts, and files whose open must fail with a line number (`bad_*`)."""
    import pathlib
    d = pathlib.Path(directory)
    rng = np.random.default_rng(5)
    rows = [("chr%d" % rng.integers(1, 4), int(rng.integers(-3, 1100)), "chr%d" % rng.integers(1, 4), int(rng.integers(-3, 1100)))
            for _ in range(5000)]
    texts = dict(("good_" + k, v) for k, v in FILES.items())
    texts["good_many"] = _text(rows)
    texts["good_many_no_header"] = _text(rows, header="")
    texts["bad_short"] = _text(rows[:700]) + "r\tchr1\t5\n" + _text(rows[700:], header="")
    texts["bad_position"] = _text(rows[:900], header="") + "r\tchr1\t5\tchr1\t7x\n"
    texts["bad_header"] = "#chromsize: chr1\n" + _text(rows[:10], header="")
    out = []
    for name, text in texts.items():
        out.extend(_gz_copies(d, name, text))
    return out
