"""Two-sample calling on an inter-chromosomal pair on the MI355X (mustache_amd/diff_trans.py) against the NumPy restatement
(tests/diff_trans_reference.py): every shared case, the launch grouping and the record order, the 10 000 threshold on
either sample (which subsumes the rule's 50), and the command line end to end (four files; cis rows, then trans rows)."""
import numpy as np
import pytest

import diff_trans_reference as dr
import trans_reference as tr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

FDR_BOUND = 1e-9               # the project's stated p-value / FDR bound (as tests/test_gpu_trans.py)


@pytest.fixture(scope="module")
def cases_ahead():
    """the restatement of every shared case in worker processes while the device tests run"""
    dr.start_ahead(list(dr.CASES))
    yield
    dr.stop_ahead()


def _compare(got, ref, need_rows=True):
    """coordinates, sigma and tags equal; fdr within FDR_BOUND"""
    if need_rows:
        assert len(ref) > 0, "the case should produce rows"
    assert [(int(r[0]), int(r[1]), int(r[4])) for r in got] == [(int(r[0]), int(r[1]), int(r[4])) for r in ref]
    assert [float(r[3]) for r in got] == [float(r[3]) for r in ref]
    worst = 0.0
    for g, r in zip(got, ref):
        worst = max(worst, abs(float(g[2]) - float(r[2])))
        assert abs(float(g[2]) - float(r[2])) <= FDR_BOUND, (g, r)
    return worst


def _rows(rows):
    return [[int(r[0]), int(r[1]), float(r[2]), float(r[3]), int(r[4])] for r in rows]


def _device_normalized(rec):
    from mustache_amd.trans import zscore_device
    return rec[0], rec[1], zscore_device(rec[2])[0].cpu().numpy()


@pytest.mark.parametrize("name", list(dr.CASES))
def test_shared_cases_match_the_restatement(name, cases_ahead):
    from mustache_amd.diff_trans import call_diff_trans_coo
    from mustache_amd.trans import trans_tiling
    case = dr.CASES[name]
    rec1, rec2 = dr.case_records(name)
    C, (rs, _), (cs, _) = trans_tiling(case["n1"], case["n2"], case["chunk"])
    npairs = len(rs) * len(cs)
    assert C == case["chunk"] and npairs >= 4
    # the restatement runs on zscore_exact's values: they ARE the device-normalised values, bit for bit
    for rec in (rec1, rec2):
        assert np.array_equal(_device_normalized(rec)[2].view(np.uint64), tr.zscore_exact(rec[2])[0].view(np.uint64))
    ref, branches = dr.case_reference(name)
    dr.assert_case_conditions(name, ref)                     # before any device comparison
    got = call_diff_trans_coo(rec1, rec2, case["oct"], dr.ST, dr.PT, dr.PT2, chunk=case["chunk"])
    worst = _compare(got, ref)
    print("%s: %d tile pairs, %d + %d records, rows per tag %r, v_other branches %r, worst |fdr - fdr*| %.3g" % (
        name, npairs, len(rec1[2]), len(rec2[2]), {t: len(v) for t, v in dr.rows_by_tag(ref).items()}, branches, worst))
    # bit-identical under the launch grouping (one tile pair per launch against all at once, a ragged last group) ...
    for tpl in (1, npairs - 1, npairs + 3):
        again = call_diff_trans_coo(rec1, rec2, case["oct"], dr.ST, dr.PT, dr.PT2, chunk=case["chunk"], tiles_per_launch=tpl)
        assert _rows(again) == _rows(got), tpl
    # ... and under a permutation of either sample's records
    rng = np.random.default_rng(1)
    p1, p2 = rng.permutation(len(rec1[2])), rng.permutation(len(rec2[2]))
    again = call_diff_trans_coo(tuple(a[p1] for a in rec1), tuple(a[p2] for a in rec2), case["oct"], dr.ST, dr.PT, dr.PT2,
                                chunk=case["chunk"])
    assert _rows(again) == _rows(got)


def test_every_v_other_branch_is_taken_across_the_shared_cases(cases_ahead):
    dr.assert_branches_covered([dr.case_reference(n)[1] for n in dr.CASES])


def test_swapped_samples_swap_the_tags_on_the_device():
    from mustache_amd.diff_trans import call_diff_trans_coo
    rec1, rec2 = dr.synth_pair(420, 300, density=0.3, nloops=14, seed=7, added=5)
    a = dr.rows_by_tag(_rows(call_diff_trans_coo(rec1, rec2, [1.6, 3.2], 0.88, 0.2, 0.1)))
    b = dr.rows_by_tag(_rows(call_diff_trans_coo(rec2, rec1, [1.6, 3.2], 0.88, 0.2, 0.1)))
    assert len(a[1]) > 0 and len(a[3]) > 0
    assert a[1] == b[3] and a[3] == b[1] and a[2] == b[4] and a[4] == b[2]


# ---- rule 4's thresholds on either sample ---------------------------------------------------------------------------------
def _device_and_reference(rec1, rec2, chunk=2000):
    from mustache_amd.diff_trans import call_diff_trans_coo
    ref = dr.diff_trans_rows_normalized(_device_normalized(rec1), _device_normalized(rec2), 0.88, 0.2, 0.1, [1.6, 3.2], chunk=chunk)
    got = call_diff_trans_coo(rec1, rec2, [1.6, 3.2], 0.88, 0.2, 0.1, chunk=chunk)
    return got, ref


def _trimmed(rec, count, seed):
    """rec with background records (not the corner record) dropped until `count` are left"""
    x, y, v = rec
    n1, n2 = int(x.max()) + 1, int(y.max()) + 1
    free = np.nonzero((v < 3.0) & ~((x == n1 - 1) & (y == n2 - 1)))[0]
    extra = len(v) - count
    assert 0 <= extra <= len(free)
    keep = np.ones(len(v), bool)
    keep[np.random.default_rng(seed).choice(free, extra, replace=False)] = False
    return x[keep], y[keep], v[keep]


def test_ten_thousand_tested_pixels_threshold_on_either_sample():
    rec1, rec2 = dr.synth_pair(300, 300, density=0.12, nloops=8, seed=1, added=3)
    assert len(rec1[2]) > 10000 and len(rec2[2]) > 10000
    full1, full2 = _trimmed(rec1, 10000, 11), _trimmed(rec2, 10000, 12)
    got, ref = _device_and_reference(full1, full2)
    by = dr.rows_by_tag(ref)
    assert len(by[1]) > 0 and len(by[3]) > 0                  # 10 000 in both: loops
    _compare(got, ref)
    for a, b in ((_trimmed(rec1, 9999, 11), full2), (full1, _trimmed(rec2, 9999, 12))):
        got, ref = _device_and_reference(a, b)
        assert len(a[2]) + len(b[2]) == 19999 and ref == [] and got == []


def test_a_sample_of_a_few_dozen_records_gives_no_rows():
    """A sample of 49 or 50 records against a full one, either way round: no rows, no fault, on both sides.  This is NOT a check
    of rule 4's 50: a sample below 50 tested pixels is below 10 000 as well, so the rules as written give the 50 no effect
    of its own, and no input can tell a caller with it from one without."""
    rng = np.random.default_rng(6)
    big, _ = dr.synth_pair(60, 60, density=0.9, nloops=2, seed=2)
    for k in (49, 50):
        flat = rng.choice(60 * 60 - 1, size=k - 1, replace=False)
        few = (np.concatenate([flat // 60, [59]]), np.concatenate([flat % 60, [59]]), np.exp(rng.normal(0.0, 0.5, k)))
        for a, b in ((few, big), (big, few)):
            got, ref = _device_and_reference(a, b)
            assert ref == [] and got == []


def test_an_empty_or_constant_sample_gives_no_rows():
    from mustache_amd.diff_trans import call_diff_trans_coo
    x, y, v = tr.synth_trans(80, 60, density=0.3, nloops=2, seed=1)
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    flat = (x, y, np.full(len(v), 3.0))
    for other in (none, flat):
        assert call_diff_trans_coo((x, y, v), other, [1.6, 3.2], 0.88, 0.2, 0.1) == []
        assert call_diff_trans_coo(other, (x, y, v), [1.6, 3.2], 0.88, 0.2, 0.1) == []


# ---- the command line -----------------------------------------------------------------------------------------------------
SUFFIXES = (".loop1", ".diffloop1", ".loop2", ".diffloop2")


def _read_tsv(path):
    with open(path) as fh:
        lines = fh.read().splitlines()
    return lines[0], [ln.split("\t") for ln in lines[1:]]


def _sample_files(tmp_path, res=10000):
    """two `.hic` samples: chr1 x chr2 and chr2 x chr3 trans records from synth_pair (float32 counts), chr1 intra records"""
    from mustache_amd.synth import synth_coo
    p12 = dr.synth_pair(400, 300, density=0.3, nloops=14, seed=21, added=5)
    p23 = dr.synth_pair(300, 350, density=0.3, nloops=14, seed=22, added=5)
    chroms = [("All", 1000), ("1", 600 * res), ("2", 400 * res), ("3", 350 * res)]
    paths = []
    for s in (0, 1):
        xi, yi, vi = synth_coo(600, 150, depth=300.0, seed=5 + s, nloops=20)
        (x12, y12, v12), (x23, y23, v23) = p12[s], p23[s]
        # the file keys (1, 2) as stored: chr2 x chr1 records are written transposed
        mats = {(1, 1): {res: (xi, yi, vi)}, (1, 2): {res: (y12, x12, v12)}, (2, 3): {res: (x23, y23, v23)}}
        paths.append(str(tmp_path / ("s%d.hic" % (s + 1))))
        write_hic_pairs(paths[-1], chroms, mats, version=8)
    return paths


def test_cli_writes_the_restatements_rows_into_the_four_files(tmp_path):
    from mustache_amd.diff_mustache import main
    from mustache_amd.trans import read_hic_trans
    f1, f2 = _sample_files(tmp_path)
    out = str(tmp_path / "d")
    main(["-f1", f1, "-f2", f2, "-ch", "2", "-ch2", "1", "-r", "10kb", "-norm", "NONE", "-o", out])
    recs = []
    for f in (f1, f2):
        x, y, v = read_hic_trans(f, "NONE", "2", "1", 10000)
        recs.append(_device_normalized((x.cpu().numpy().astype(np.int64), y.cpu().numpy().astype(np.int64), v)))
    ref = dr.rows_by_tag(dr.diff_trans_rows_normalized(recs[0], recs[1], 0.88, 0.2, 0.1, [1.6, 3.2]))
    assert len(ref[1]) > 0 and len(ref[3]) > 0 and len(ref[2]) + len(ref[4]) > 0
    for tag, suf in enumerate(SUFFIXES, start=1):
        header, rows = _read_tsv(out + suf)
        assert header.startswith("BIN1_CHR") and len(rows) == len(ref[tag]), suf
        for r, (a, b, q, s) in zip(rows, ref[tag]):
            assert r[0] == "2" and r[3] == "1"
            assert (int(r[1]), int(r[2]), int(r[4]), int(r[5])) == (a * 10000, (a + 1) * 10000, b * 10000, (b + 1) * 10000)
            assert float(r[7]) == float(s) and abs(float(r[6]) - q) <= FDR_BOUND


def test_mixed_run_writes_cis_rows_then_trans_rows(tmp_path):
    from mustache_amd.diff_mustache import main
    f1, f2 = _sample_files(tmp_path)
    common = ["-f1", f1, "-f2", f2, "-r", "10kb", "-norm", "NONE"]
    cis, mixed, trans = (str(tmp_path / n) for n in ("cis", "mixed", "trans"))
    main(common + ["-ch", "1", "-o", cis])
    main(common + ["-ch", "2", "1", "-ch2", "3", "1", "-o", mixed])            # the trans pair first on the command line
    main(common + ["-ch", "2", "-ch2", "3", "-o", trans])
    n_cis = n_trans = 0
    for suf in SUFFIXES:
        cis_text, mixed_text, trans_text = (open(p + suf).read() for p in (cis, mixed, trans))
        n_cis += len(cis_text.splitlines()) - 1
        n_trans += len(trans_text.splitlines()) - 1
        assert mixed_text.startswith(cis_text), suf
        assert mixed_text[len(cis_text):] == "".join(ln + "\n" for ln in trans_text.splitlines()[1:]), suf
    assert n_cis > 0 and n_trans > 0
