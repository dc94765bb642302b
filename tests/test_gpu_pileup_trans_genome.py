"""`python -m mustache_amd.pileup --trans --balance-genome` end to end on the MI355X: a three-chromosome genome of integer counts,
written once as a raw `.hic` file and once as a `.pairs` file, piled up around one loop list.  The four output files against
NumPy: balance_genome_reference.balanced on the run's bias, the records with v' > 0, pileup_trans_reference.pileup_trans_records
with n1, n2 = the genome layout's bins, the partials added in pair order.  Statuses and counts exact, values as
test_gpu_pileup_trans._check compares them."""
import numpy as np
import pytest

import balance_genome_reference as gr
import pairs_trans_reference as ptr_pairs
import pileup_reference as pr
import pileup_trans_reference as ptr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

RES, W, Q = 10000, 3, 2
BINS = (70, 50, 40)
NAMES = ["1", "2", "3"]
HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"
BALANCING = "NEWTON balancing of the genome (%s pixels):"


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        ok = both_nan | (a == b) | (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all())


def _lengths(bins):
    return [b * RES - 1 for b in bins]                      # those gr.hic_arguments uses


def _write_both(d, tag, bins, cis, trans, seed):
    """the helper of test_gpu_pairs_trans.py restated: the same contacts as a raw `.hic` file and as a pairs file"""
    chroms, mats = gr.hic_arguments(bins, RES, cis, trans)
    hic = str(d / (tag + ".hic"))
    write_hic_pairs(hic, chroms, mats, version=8)
    text, rows = ptr_pairs.pairs_text(NAMES, _lengths(bins), RES, cis, trans, seed)
    plain = str(d / (tag + ".pairs"))
    with open(plain, "w") as fh:
        fh.write(text)
    return {"hic": hic, "pairs": plain, "rows": rows}


def _row(c1, b1, c2, b2):
    return (c1, b1 * RES, (b1 + 1) * RES, c2, b2 * RES, (b2 + 1) * RES)


ROWS = [_row("1", 10, "2", 20),               # (1, 2)
        _row("1", 30, "3", 15),               # (1, 3)
        _row("3", 5, "2", 44),                # {2, 3} oriented (3, 2) by its first row
        _row("chr1", 69, "chr2", 49),         # (1, 2): the last bins, the window leaves the map on both axes
        _row("2", 10, "2", 40),               # cis
        _row("2", 13, "3", 39),               # written (2, 3): anchors swapped, a = 39 on chr3, b = 13 (a masked bin) on chr2
        _row("1", 5, "7", 5),                 # a chromosome the file does not hold
        _row("1", 70, "2", 3),                # bin 70 >= n_1 = 70: off the map
        _row("1", 7, "2", 0),                 # row 7 of chromosome 1 is masked: its records leave with the balancing
        _row("2", 49, "3", 0),                # written (2, 3) again
        _row("3", 39, "1", 0)]                # (1, 3) written (3, 1): swapped
STATUS = ["used", "used", "used", "used", "cis", "used", "no_pair", "off_map", "used", "used", "used"]


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("pileup_trans_genome")
    cis, trans = gr.synth_genome(BINS)
    out = _write_both(d, "g", BINS, cis, trans, 5)
    lp = str(d / "l.tsv")
    with open(lp, "w") as fh:
        fh.write(HEADER + "\n" + "".join("\t".join(str(c) for c in r) + "\t0.01\t1.6\n" for r in ROWS))
    out.update(cis=cis, trans=trans, loops=lp, dir=d)
    return out


def _run(genome, tag, source, extra, capsys):
    from mustache_amd import pairs
    from mustache_amd.pileup import main
    out = str(genome["dir"] / tag)
    capsys.readouterr()
    main(["-f", genome[source], "-l", genome["loops"], "-r", str(RES), "-o", out, "--trans", "-w", str(W), "-q", str(Q)] + extra)
    said = capsys.readouterr().out
    pairs.WANT_TRANS.clear()
    pairs.close_pairs_handles()
    assert "Error" not in said, said
    return out, said


def _files(prefix):
    return [open(prefix + suffix, "rb").read() for suffix in (".apa.tsv", ".oe.tsv", ".stats.tsv", ".loops.tsv")]


def _read_matrix(path):
    return np.array([[float(c) for c in line.split("\t")] for line in open(path).read().splitlines()])


def _restated(genome, bias, chromosomes=None, rows=None):
    """the genome mode of mustache_amd/pileup.py in NumPy: (status, centres [rows, 3], parts, whole)"""
    bins, off, _ = gr.layout(_lengths(BINS), RES)
    index = {n: i for i, n in enumerate(NAMES)}
    keys = None if not chromosomes else set(chromosomes)
    rows = ROWS if rows is None else rows
    n = len(rows)
    status, a, b = [None] * n, np.zeros(n, np.int64), np.zeros(n, np.int64)
    pairs, orient, members = [], {}, {}
    for k, (c1, s1, e1, c2, s2, e2) in enumerate(rows):
        k1, k2 = ptr._key(c1), ptr._key(c2)
        if k1 == k2:
            status[k] = "cis"
            continue
        if keys is not None and not (k1 in keys and k2 in keys):
            status[k] = "no_pair"
            continue
        p = frozenset((k1, k2))
        if p not in orient:
            orient[p] = k1
            pairs.append((p, c1, c2))
            members[p] = []
        members[p].append(k)
        b1, b2 = ((s1 + e1) // 2) // RES, ((s2 + e2) // 2) // RES
        a[k], b[k] = (b1, b2) if orient[p] == k1 else (b2, b1)
    S = 2 * W + 1
    centre = np.full((n, 3), np.nan)
    tot = [np.zeros((S, S)) for _ in range(4)]
    parts = []
    for p, A, B in pairs:
        ia, ib = index.get(ptr._key(A)), index.get(ptr._key(B))
        part, used = pr.pileup_band(np.zeros((1, 1)), 1, 0, [], [], W, Q), []
        if ia is None or ib is None:
            for k in members[p]:
                status[k] = "no_pair"
        else:
            x, y, v = genome["trans"][(min(ia, ib), max(ia, ib))]
            if ia > ib:
                x, y = y, x
            x, y, v = gr.balanced(bias, off[ia], off[ib], x, y, v)
            assert len(v) < len(genome["trans"][(min(ia, ib), max(ia, ib))][2])           # the balancing removed records
            for k in members[p]:
                status[k] = "off_map" if a[k] >= bins[ia] or b[k] >= bins[ib] else "used"
            if len(v) == 0:                                  # nothing is kept: every row of the pair, off_map ones included
                for k in members[p]:
                    status[k] = "no_pair"
            else:
                used = [k for k in members[p] if status[k] == "used"]
                part = ptr.pileup_trans_records(x, y, v, bins[ia], bins[ib], a[used], b[used], W, Q)
                for j, k in enumerate(used):
                    centre[k] = part["center_obs"][j], part["center_oe"][j], part["p2ll"][j]
        parts.append(("%s,%s" % (A, B), len(members[p]), len(used), part))
        for t, name in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
            t += part[name]
    apa, apa_oe = pr.mean_map(tot[0], tot[1]), pr.mean_map(tot[2], tot[3])
    whole = {"apa": apa, "apa_oe": apa_oe, "metrics": pr.metrics(apa, W, Q), "metrics_oe": pr.metrics(apa_oe, W, Q)}
    return status, centre, parts, whole


def _against(prefix, want, rows=ROWS):
    from mustache_amd.pileup import METRICS
    status, centre, parts, whole = want
    assert _close(_read_matrix(prefix + ".apa.tsv"), whole["apa"]) and _close(_read_matrix(prefix + ".oe.tsv"), whole["apa_oe"])
    body = [r.split("\t") for r in open(prefix + ".loops.tsv").read().splitlines()[1:]]
    assert [r[8] for r in body] == status
    assert _close([[float(c) for c in r[9:12]] for r in body], centre)
    stats = [r.split("\t") for r in open(prefix + ".stats.tsv").read().splitlines()[1:]]
    assert [r[:3] for r in stats] == [[name, str(rows), str(used)] for name, rows, used, _ in parts] + \
        [["all", str(len(rows)), str(sum(u for _, _, u, _ in parts))]]
    for r, (_name, _rows, _used, p) in zip(stats, parts + [("all", 0, 0, whole)]):
        assert _close([float(c) for c in r[3:9]], [p["metrics"][m] for m in METRICS]), r[0]
        assert _close(float(r[9]), p["metrics_oe"]["P2LL"]), r[0]


@pytest.fixture(scope="module")
def bias(genome):
    from mustache_amd.balance_genome import genome_bias
    return {px: genome_bias(genome["hic"], RES, method="NEWTON", pixels=px, keep_records=False).bias for px in ("all", "inter")}


def test_hic_run_against_numpy_and_the_pairs_run_byte_for_byte(genome, bias, capsys):
    assert np.isnan(bias["all"][[7, 83, 131]]).all()                               # the thinned bins are masked
    want = _restated(genome, bias["all"])
    assert want[0] == STATUS and [p[:3] for p in want[2]] == [("1,2", 4, 3), ("1,3", 2, 2), ("3,2", 3, 3), ("1,7", 1, 0)]
    assert not np.isnan(want[1][[0, 1, 2, 3, 5, 8, 9, 10], 0]).any()
    assert want[1][8, 0] == 0.0 and want[1][5, 0] == 0.0                           # centres on a masked bin: no record is left
    assert np.isnan(want[2][0][3]["obs"][1]).any()                                 # the window of (69, 49) leaves the map
    hic, said = _run(genome, "hic", "hic", ["--balance-genome", "NEWTON"], capsys)
    assert said.count(BALANCING % "all") == 1 and said.count("balancing of") == 1
    _against(hic, want)
    pairs, said = _run(genome, "pairs", "pairs", ["--balance-genome", "NEWTON", "--pairs-trans"], capsys)
    assert said.count(BALANCING % "all") == 1 and said.count("balancing of") == 1 and "trans pixels" in said
    assert _files(pairs) == _files(hic)


def test_inter_pixels_and_a_chromosome_list(genome, bias, capsys):
    inter, said = _run(genome, "inter", "hic", ["--balance-genome", "newton", "--balance-pixels", "inter"], capsys)
    assert said.count(BALANCING % "inter") == 1 and said.count("balancing of") == 1
    _against(inter, _restated(genome, bias["inter"]))
    assert not np.array_equal(bias["inter"], bias["all"], equal_nan=True)
    some, said = _run(genome, "some", "hic", ["--balance-genome", "NEWTON", "-ch", "1", "2"], capsys)
    assert said.count(BALANCING % "all") == 1                                      # the whole genome all the same
    want = _restated(genome, bias["all"], ["1", "2"])
    assert want[0] == ["used", "no_pair", "no_pair", "used", "cis", "no_pair", "no_pair", "off_map", "used", "no_pair", "no_pair"]
    _against(some, want)


def test_the_python_call_and_the_window_refusal(genome, bias, monkeypatch):
    from mustache_amd import pileup as pl
    r = pl.pileup(genome["hic"], genome["loops"], RES, w=W, q=Q, trans=True, balance_genome="NEWTON")
    want = _restated(genome, bias["all"])
    assert r.status == want[0] and _close(r.all["apa"], want[3]["apa"])
    assert [(name, rows, used) for name, rows, used, _ in r.chromosomes] == [p[:3] for p in want[2]]
    with pytest.raises(pl.PileupError, match="--trans"):
        pl.pileup(genome["hic"], genome["loops"], RES, w=W, q=Q, balance_genome="NEWTON")
    # one host wait per batch: a budget of four loops' windows cuts the three pairs into three batches with the same result
    calls = []
    real = pl.pileup_trans_batch
    monkeypatch.setattr(pl, "pileup_trans_batch", lambda *a, **k: (calls.append(len(a[4])), real(*a, **k))[1])
    r1 = pl.pileup(genome["hic"], genome["loops"], RES, w=W, q=Q, trans=True, balance_genome="NEWTON")
    assert calls == [3]
    monkeypatch.setattr(pl, "window_budget", lambda: 4 * pl.window_bytes(1, W))
    del calls[:]
    r2 = pl.pileup(genome["hic"], genome["loops"], RES, w=W, q=Q, trans=True, balance_genome="NEWTON")
    assert calls == [1, 1, 1]
    assert r2.status == r1.status and r2.all["sum_oe"].tobytes() == r1.all["sum_oe"].tobytes()
    assert r2.p2ll.tobytes() == r1.p2ll.tobytes()
    monkeypatch.setattr(pl, "window_budget", lambda: 2 * pl.window_bytes(1, W))
    with pytest.raises(pl.PileupError, match=r"1,2 \(3 loops, w = 3\) need %d bytes.*; %d bytes"
                       % (pl.window_bytes(3, W), 2 * pl.window_bytes(1, W))):
        pl.pileup(genome["hic"], genome["loops"], RES, w=W, q=Q, trans=True, balance_genome="NEWTON")


# ---- a pair of which the balancing keeps nothing ----------------------------------------------------------------------------------
MASKED_ROWS = [_row("1", 10, "2", 20),        # (1, 2): used
               _row("2", 13, "3", 11),        # (2, 3): raw records there, all on the masked bins 13 of chr2 and 11 of chr3
               _row("2", 50, "3", 5),         # (2, 3) off the map: `no_pair` all the same, nothing of the pair is kept
               _row("3", 20, "2", 30)]        # (2, 3) written (3, 2)


def test_a_pair_whose_records_all_leave_with_the_balancing_is_no_pair(genome, capsys):
    """the same genome, but the pair (2, 3) keeps only its raw records on row 13 of chromosome 2 or column 11 of chromosome 3,
    both masked: `kept` comes back 0, the device result is discarded, every row of the pair is `no_pair`, its partial is empty"""
    from mustache_amd.balance_genome import genome_bias
    d = genome["dir"]
    x, y, v = genome["trans"][(1, 2)]
    on_masked = (x == 13) | (y == 11)
    assert 0 < on_masked.sum() < 10
    trans = dict(genome["trans"])
    trans[(1, 2)] = (x[on_masked], y[on_masked], v[on_masked])
    files = _write_both(d, "masked", BINS, genome["cis"], trans, 6)
    lp = str(d / "masked.tsv")
    with open(lp, "w") as fh:
        fh.write(HEADER + "\n" + "".join("\t".join(str(c) for c in r) + "\t0.01\t1.6\n" for r in MASKED_ROWS))
    gb = genome_bias(files["hic"], RES, method="NEWTON", pixels="all")
    assert np.isnan(gb.bias[[83, 131]]).all() and gb.records("2", "3")[2].numel() == int(on_masked.sum())     # raw records exist
    want = _restated({"trans": trans}, gb.bias, rows=MASKED_ROWS)
    assert want[0] == ["used", "no_pair", "no_pair", "no_pair"] and [p[:3] for p in want[2]] == [("1,2", 1, 1), ("2,3", 3, 0)]
    assert not want[2][1][3]["count_obs"].any()
    out, said = _run(dict(genome, loops=lp, hic=files["hic"]), "masked_out", "hic", ["--balance-genome", "NEWTON"], capsys)
    _against(out, want, MASKED_ROWS)
    assert "pile-up of the pair 2,3: 0 of 3 rows used" in said
