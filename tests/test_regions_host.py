"""``compare --regions / --stratify`` without a GPU: the library's sequential restatement (``msim_dbg_cmp_counts_regions``) against
``region_twin`` on every case, the invariants of a restriction, ``msim_bed_scan`` against a Python split, and ``bed.py``'s
normalisation against a brute-force mask.  All comparisons are exact integers and bytes.
"""
from __future__ import annotations

import gzip
import re
from pathlib import Path

import numpy as np
import pytest

import region_twin as rt
from mutation_simulator_amd import _ffi, bed

PASS = _ffi.CMP_PASS
CASES = rt.cases(PASS)
EXPECTED = {}


def expected(name):
    if name not in EXPECTED:
        EXPECTED[name] = rt.expected(CASES[name])
    return EXPECTED[name]


def host(case, fa, fb, mask):
    (a, pa, _), (b, pb, _) = rt.tables_of(case)
    return _ffi.cmp_counts_regions_host(case["bases"], a, pa, fa, b, pb, fb, 2 if case["kind"] == "haploid" else 3, case["sets"], mask,
                                        case["exact"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_restatement_equals_the_twin(name):
    case = CASES[name]
    ma, mb, by_mask, plain, fa, fb = expected(name)
    (a, _, _), (b, _, _) = rt.tables_of(case)
    for mask, (counts, outside) in by_mask.items():
        got = host(case, fa, fb, mask)
        assert got[0].dtype == counts.dtype and got[0].shape == counts.shape
        assert np.array_equal(got[0], counts), (name, mask, np.flatnonzero((got[0] != counts).reshape(-1))[:8].tolist())
        assert got[1].tolist() == outside.tolist(), (name, mask)
        assert np.array_equal(got[2], ma) and np.array_equal(got[3], mb), (name, mask, got[2][:16].tolist(), ma[:16].tolist())
        # inside plus outside are the tables; truth matched == calls matched in every cell (a blocks pass pairs no one with one)
        half = counts.shape[-1] // 2
        assert int(got[0][..., :half].sum()) + int(got[1][0]) == len(a) and int(got[0][..., half:].sum()) + int(got[1][1]) == len(b)
        if case["kind"] != "blocks":
            assert np.array_equal(got[0][..., 0], got[0][..., half])
        if case["kind"] == "diploid":
            assert np.array_equal(got[0][..., 1], got[0][..., half + 1])
    got = host(case, fa, fb, 0)
    assert np.array_equal(got[0], plain) and got[1].tolist() == [0, 0]


def test_the_named_shapes():
    ma, mb, by_mask, *_ = expected("half_open")
    assert ma.tolist() == [0, 1, 1, 0] and mb.tolist() == [0, 1, 1, 0]
    ma, mb, *_ = expected("anchor_outside")
    assert ma.tolist() == [0] and mb.tolist() == [0, 1]                    # both DEs anchor at 20; the SN at 27 is inside
    ma, mb, *_ = expected("anchor_outside_exact")
    assert ma.tolist() == [1] and mb.tolist() == [0, 1]                    # the DE at 27 is inside, the one at 22 is not
    for name in ("pair_across_edge", "pair_across_edge_ins"):
        ma, mb, by_mask, _, fa, fb = expected(name)
        assert fa.tolist() == [1] and fb.tolist() == [1] and ma.tolist() == [2] and mb.tolist() == [2]
        assert by_mask[1][1].tolist() == [1, 1] and by_mask[2][1].tolist() == [0, 0]
    ma, mb, by_mask, _, fa, fb = expected("window_edge")
    assert ma.tolist() == [0b110, 0b110] and mb.tolist() == [0b101, 0b110]   # anchors exactly W; the SN at W - 1
    ma, mb, by_mask, plain, *_ = expected("whole_contig")
    assert np.array_equal(by_mask[1][0], plain) and by_mask[1][1].tolist() == [0, 0]
    ma, mb, by_mask, *_ = expected("empty_set")
    assert not ma.any() and not mb.any() and not by_mask[1][0].any()
    ma, mb, *_ = expected("pass_edges")
    for k in (PASS, 2 * PASS):
        assert ma[k - 1:k + 2].tolist() == [1, 0, 1]
    ma, mb, by_mask, _, fa, fb = expected("dip_gt_mismatch_across_edge")
    assert 2 in fa.tolist() and 2 in fb.tolist()
    ma, mb, by_mask, _, fa, fb = expected("blocks_part_of_block")
    assert fa.tolist() == [2, 2] and fb.tolist() == [2, 2] and ma.tolist() == [0b011, 0b010] and mb.tolist() == [0b011, 0b110]


def test_host_refusals():
    case = CASES["half_open"]
    _, _, _, _, fa, fb = expected("half_open")
    (a, pa, _), (b, pb, _) = rt.tables_of(case)
    L = len(case["bases"])

    def call(sets, mask=1, outcomes=2, truth=a):
        return _ffi.cmp_counts_regions_host(case["bases"], truth, pa, fa, b, pb, fb, outcomes, sets, mask)
    for sets in ([rt.one((10, 10))], [rt.one((12, 10))], [rt.one((0, L + 1))], [rt.one((0, 5), (5, 9))], [rt.one((4, 9), (2, 3))],
                 [rt.one()] * 9):
        with pytest.raises(_ffi.MsimError) as e:
            call(sets)
        assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="not resident"):
        call([rt.one((0, 5))], mask=2)
    with pytest.raises(_ffi.MsimError, match="outcomes"):
        call([rt.one((0, 5))], outcomes=4)
    bad = a.copy()
    bad["type"][1] = 9
    with pytest.raises(_ffi.MsimError, match="truth record 1: unknown type"):
        call([rt.one((0, 5))], truth=bad)
    call([rt.one((0, L))])                                                 # (the whole contig is in normal form)


def test_header_constants_and_a_host_only_context():
    text = (Path(__file__).resolve().parents[1] / "include" / "msim.h").read_text()
    defines = dict(re.findall(r"^#define (MSIM_\w+)\s+(\S+)", text, re.M))
    assert int(defines["MSIM_CMP_REGION_SETS"]) == _ffi.CMP_REGION_SETS == rt.SETS == 8
    assert int(defines["MSIM_CMP_DIPLOID"].rstrip("u")) == _ffi.CMP_DIPLOID == 2 and _ffi.CMP_DIPLOID & _ffi.CMP_EXACT == 0
    for name in ("msim_cmp_regions_set", "msim_cmp_regions_drop", "msim_cmp_regions_mark", "msim_cmp_counts_regions", "msim_cmp_fetch_regions",
                 "msim_cmp_regions_timing", "msim_dbg_cmp_counts_regions", "msim_bed_scan"):
        assert re.search(rf"^int {name}\(", text, re.M) and hasattr(_ffi.load(), name), name
    e = _ffi.Engine(-1)
    try:
        for call in (lambda: e.cmp_regions_set(0, 0, [1], [2]), lambda: e.cmp_regions_drop(), lambda: e.cmp_regions_mark(0),
                     lambda: e.cmp_counts_regions(0, 1), lambda: e.cmp_fetch_regions(0), lambda: e.cmp_regions_timing()):
            with pytest.raises(_ffi.MsimError, match="host-only context") as ei:
                call()
            assert ei.value.code == _ffi.ERR_HIP
    finally:
        e.close()


def test_usage_errors(tmp_path, capsys):
    from mutation_simulator_amd import argument_parser as ap
    (tmp_path / "g.fa").write_text(">c\nACGT\n")
    for name in ("t.vcf", "a.bed", "b.bed"):
        (tmp_path / name).write_text("")
    base = [str(tmp_path / "g.fa"), "compare", str(tmp_path / "t.vcf"), str(tmp_path / "t.vcf")]
    bed_a, bed_b = str(tmp_path / "a.bed"), str(tmp_path / "b.bed")

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            ap.get_args(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err
    refused(["--diploid", "--phased", "--regions", bed_a], "--phased", "genome-wide")
    refused(["--diploid", "--phased", "--stratify", f"a={bed_a}"], "--phased", "genome-wide")
    for bad in (f"={bed_a}", f"a b={bed_a}", f"a#={bed_a}", f"a\tb={bed_a}", "noequals", "a="):
        refused(["--stratify", bad], "--stratify takes NAME=FILE")
    refused(["--stratify", f"a={bed_a}", "--stratify", f"a={bed_b}"], "distinct")
    args = ap.get_args(base + ["--regions", bed_a, "--stratify", f"x={bed_a}", "--stratify", f"y=z={bed_b}", "--diploid", "--exact", "--per-contig",
                               "--list"])
    assert args.regions == tmp_path / "a.bed" and args.stratify == [("x", tmp_path / "a.bed"), ("y", Path(f"z={bed_b}"))]
    args = ap.get_args(base + ["--blocks"])
    assert args.regions is None and args.stratify == []


# ------------------------------------------------------------------------------ msim_bed_scan
BED = (b"# a comment\n"
       b"track name=x\n"
       b"browser position chr1:1-100\n"
       b"\n"
       b"chr1\t10\t20\n"
       b"chr1 30   40\textra\tcolumns 7\n"
       b"chr2\t5\t5\n"                    # start == end: valid and dropped
       b"chr2\t0\t4294967295\r\n"
       b"chr1\t1\t2\n"                    # a scattered run of chr1
       b"\r\n"
       b"chrUn\t7\t9\n"
       b"chrUn\t1\t3")                    # the last line without a newline


def split_scan(text: bytes):
    """The scan by a Python split: (name, start, end, line) per kept interval."""
    out = []
    for n, line in enumerate(text.split(b"\n"), 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith((b"#", b"track", b"browser")):
            continue
        f = line.replace(b"\t", b" ").split()
        if int(f[1]) != int(f[2]):
            out.append((f[0], int(f[1]), int(f[2]), n))
    return out


def test_bed_scan_equals_a_python_split():
    starts, ends, lines, name_off, name_len, first, count = _ffi.bed_scan(BED)
    want = split_scan(BED)
    assert [w[1] for w in want] == starts.tolist() and [w[2] for w in want] == ends.tolist() and [w[3] for w in want] == lines.tolist()
    assert lines.tolist() == [5, 6, 8, 9, 11, 12] and starts.dtype == ends.dtype == np.uint32
    names = [BED[int(o):int(o) + int(n)] for o, n in zip(name_off, name_len)]
    assert names == [b"chr1", b"chr2", b"chr1", b"chrUn"] and first.tolist() == [0, 2, 3, 4] and count.tolist() == [2, 1, 1, 2]
    for k in range(len(first)):
        assert all(want[j][0] == names[k] for j in range(int(first[k]), int(first[k]) + int(count[k])))
    for empty in (b"", b"\n\n# nothing\n", b"chr1\t3\t3\n"):
        assert all(len(x) == 0 for x in _ffi.bed_scan(empty))


@pytest.mark.parametrize("text,why", [
    (b"chr1\t1\t2\nchr1\t5\n", "BED line 2: fewer than three fields"),
    (b"#c\n\nchr1\n", "BED line 3: fewer than three fields"),
    (b"chr1\t1\t2\nchr1\t-1\t5\n", "BED line 2: start is no number"),
    (b"chr1\t1e3\t5000\n", "BED line 1: start is no number"),
    (b"chr1\t4294967296\t4294967297\n", "BED line 1: start is no number"),
    (b"track\nchr1\t1\t2x\n", "BED line 2: end is no number"),
    (b"chr1\t1\t4294967296\n", "BED line 1: end is no number"),
    (b"chr1\t1\t2\r", "BED line 1: end is no number"),
    (b"chr1\t1\t2\n\nchr1\t9\t8\nchr1\tx\ty\n", "BED line 3: end in front of start"),
])
def test_bed_scan_refusals_name_the_line(text, why):
    with pytest.raises(_ffi.MsimError) as e:
        _ffi.bed_scan(text)
    assert e.value.code == _ffi.ERR_VALUE and str(e.value).endswith(why)


# ------------------------------------------------------------------------------ bed.py
@pytest.mark.parametrize("seed", range(6))
def test_normalise_equals_the_brute_force_mask(seed):
    rs = np.random.RandomState(seed)
    L = 300
    fixed = [(10, 20), (15, 30), (30, 35), (40, 60), (45, 50), (59, 61), (5, 6), (100, 101), (101, 102), (0, 1)]   # overlapping, abutting, nested, unsorted
    n = int(rs.randint(0, 40))
    s = rs.randint(0, L, n)
    pairs = fixed[:seed * 2] + [(int(a), int(a + rs.randint(1, 12))) for a in s if a + 12 <= L]
    rs.shuffle(pairs)
    starts, ends = bed.normalise([p[0] for p in pairs], [p[1] for p in pairs])
    assert starts.dtype == ends.dtype == np.uint32
    want = rt.member(L, [p[0] for p in pairs], [p[1] for p in pairs])
    assert np.array_equal(rt.member(L, starts, ends), want)
    assert (starts < ends).all() and (starts[1:] > ends[:-1]).all()        # normal form: merged, abutting ones too
    edges = np.flatnonzero(np.diff(np.concatenate([[False], want, [False]]).astype(np.int8)))
    assert starts.tolist() == edges[0::2].tolist() and ends.tolist() == edges[1::2].tolist()


def test_regions_of_a_file(tmp_path):
    text = (b"chr2\t50\t60\nchrM\t1\t5\nchrM\t9\t12\nchr1\t10\t20\nchr2\t10\t55\n# c\nchr1\t15\t30\nchr1\t30\t31\nchrUn_x\t0\t9\nchr1\t0\t1\n")
    (tmp_path / "r.bed").write_bytes(text)
    r = bed.Regions(tmp_path / "r.bed", ["chr1", "chr2", "chr3"], [31, 60, 5])
    assert [(s.tolist(), e.tolist()) for s, e in r.sets] == [([0, 10], [1, 31]), ([10], [60]), ([], [])]
    assert r.foreign_lines == 3 and r.n_intervals == 3 and r.bases == 22 + 50 and r.scan_s >= 0
    with gzip.open(tmp_path / "r.bed.gz", "wb") as f:
        f.write(text)
    z = bed.Regions(tmp_path / "r.bed.gz", ["chr1", "chr2", "chr3"], [31, 60, 5])
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(r.sets, z.sets))
    # the end beyond the contig: the line of the file, not the interval's index
    with pytest.raises(bed.BedError, match=r"r\.bed: BED line 8: end beyond the contig's last base"):
        bed.Regions(tmp_path / "r.bed", ["chr1", "chr2"], [30, 60])
    with pytest.raises(bed.BedError, match=r"r\.bed: BED line 1: end beyond the contig's last base"):
        bed.Regions(tmp_path / "r.bed", ["chr1", "chr2"], [31, 59])
    (tmp_path / "bad.bed").write_bytes(b"chr1\t1\t2\nchr1\t3\n")
    with pytest.raises(bed.BedError, match=r"bad\.bed: BED line 2: fewer than three fields"):
        bed.Regions(tmp_path / "bad.bed", ["chr1"], [10])
