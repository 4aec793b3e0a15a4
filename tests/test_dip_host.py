"""``compare --diploid`` without a GPU: the library's sequential restatements (``msim_dbg_cmp_join``,
``msim_dbg_cmp_counts_diploid``) against ``dip_twin`` on every shape the GPU tier runs, the haploid restatement as the diploid
one with equal dosages, the file writer with the ``GT`` column, and the command line's names and usage errors.  All comparisons
are exact integers and bytes."""
from __future__ import annotations

import contextlib
import ctypes as C
import io
from pathlib import Path

import numpy as np
import pytest

import cmp_twin as tw
import dip_twin as dt
from mutation_simulator_amd import _ffi, argument_parser as ap, compare

PASS, TILE = _ffi.CMP_PASS, _ffi.CMP_JOIN_TILE
CASES = dt.small_cases(PASS, TILE)


def joined(side):
    """One side's diploid table by the twin, held against the library's merge: (U, pool, gt)."""
    want = dt.join(*side)
    got = _ffi.cmp_join_host(*side)
    for name, g, w in zip(("records", "pool", "genotypes"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    return got


def check_host(case):
    bases, truth, calls, exact = case
    (a, pa, ga), (b, pb, gb) = joined(truth), joined(calls)
    for u, gt, (h1, _, h2, _) in ((a, ga, truth), (b, gb, calls)):
        assert (np.diff(u["pos"].astype(np.int64)) >= 0).all() and ((gt >= 1) & (gt <= 3)).all()
        assert len(u) == len(h1) + len(h2) - int((gt == 3).sum())
        assert int((gt & 1 != 0).sum()) == len(h1) and int((gt & 2 != 0).sum()) == len(h2)
    want = dt.score(bases, a, pa, ga, b, pb, gb, exact)
    got = _ffi.cmp_counts_diploid_host(bases, a, pa, ga, b, pb, gb, exact)
    assert got[0].dtype == np.uint64 and got[0].shape == (8, _ffi.CMP_BINS, 6) and got[1].shape == (2,)
    for name, g, w in zip(("counts", "tallies", "truth flags", "calls flags"), got, want):
        assert np.array_equal(g, w), (name, g.tolist(), w.tolist())
    invariants(got[0], len(a), len(b))
    # the sides change places: the halves of the counts do
    swapped = _ffi.cmp_counts_diploid_host(bases, b, pb, gb, a, pa, ga, exact)[0]
    assert np.array_equal(swapped[..., :3], got[0][..., 3:]) and np.array_equal(swapped[..., 3:], got[0][..., :3])
    return (a, pa, ga), (b, pb, gb), got


def invariants(counts, n_truth, n_calls):
    assert np.array_equal(counts[..., 0], counts[..., 3]) and np.array_equal(counts[..., 1], counts[..., 4])
    assert int(counts[..., :3].sum()) == n_truth and int(counts[..., 3:].sum()) == n_calls


def totals(counts):
    """(TP, GT, truth missed, calls extra)"""
    return tuple(int(counts[..., k].sum()) for k in (0, 1, 2, 5))


# ------------------------------------------------------------------------------ 1. the join and the counts
def test_constants_are_the_headers():
    header = (Path(__file__).resolve().parent.parent / "include" / "msim.h").read_text()
    assert f"#define MSIM_CMP_JOIN_TILE {TILE}\n" in header and TILE % 64 == 0
    assert f"#define MSIM_CMP_TRUTH {_ffi.CMP_TRUTH}\n" in header and f"#define MSIM_CMP_CALLS {_ffi.CMP_CALLS}\n" in header
    assert (_ffi.CMP_TRUTH, _ffi.CMP_CALLS) == (0, 1) and "#define MSIM_ABI_VERSION 8\n" in header


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_restatements_equal_the_twin(case):
    check_host(CASES[case])


HAPLOID_CASES = tw.small_cases(PASS)
HAPLOID_OF_DIPLOID = (0, 2, 3, 5)          # truth matched, missed, calls matched, extra among the six values of a diploid cell


@pytest.mark.parametrize("exact", (False, True), ids=("normalised", "exact"))
@pytest.mark.parametrize("case", sorted(HAPLOID_CASES))
def test_a_haploid_comparison_is_the_diploid_one_with_every_dosage_equal(case, exact):
    """Both restatements run one loop (csrc/compare.hip: ``dbg_counts``): with every genotype byte 3 on both sides no pair can
    differ in dosage, and the diploid counts are the haploid ones with two empty columns.  The diploid entry point refuses what
    the haploid one counts as nothing (an unknown type, an unsorted table); none of the haploid cases is such a table, so no
    case is left out and a refusal fails the test."""
    bases, a, pa, b, pb, _ = HAPLOID_CASES[case]
    hom = lambda t: np.full(len(t), 3, dtype=np.uint8)                                     # noqa: E731
    want = _ffi.cmp_counts_host(bases, a, pa, b, pb, exact)
    got = _ffi.cmp_counts_diploid_host(bases, a, pa, hom(a), b, pb, hom(b), exact)
    assert np.array_equal(got[0][..., HAPLOID_OF_DIPLOID], want[0]) and not got[0][..., (1, 4)].any()
    for name, g, w in zip(("tallies", "truth flags", "calls flags"), got[1:], want[1:]):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


def test_what_the_named_cases_are_about():
    """The twin and the library agree on every case (above); here the cases' own claims, in plain numbers."""
    for case, want in {"both_empty": (0, 0, 0, 0), "het_het_other_phase": (1, 0, 0, 0), "het_het_same_phase": (1, 0, 0, 0),
                       "het_hom": (0, 2, 0, 0), "hom_het": (0, 1, 0, 0), "multi_allelic_1_2_vs_2_1": (2, 0, 0, 0),
                       "shifted_equal_dosage": (1, 0, 0, 0), "shifted_equal_dosage_exact": (0, 0, 1, 1),
                       "shifted_unequal_dosage": (0, 1, 0, 0), "shifted_ins_unequal_dosage": (0, 1, 0, 0),
                       "rank_mixed_dosages": (2, 0, 1, 0), "rank_mixed_dosages_crossed": (0, 2, 1, 0),
                       "shifted_across_haplotypes": (0, 1, 1, 0), "every_type": (0, 7, 0, 0), "equal": (0, 5, 0, 0),
                       "disjoint": (9, 0, 0, 0)}.items():
        assert totals(check_host(CASES[case])[2][0]) == want, case
    (a, pa, ga), _, _ = check_host(CASES["equal"])
    assert ga.tolist() == [3] * 5 and len(a) == 5
    (a, pa, ga), _, _ = check_host(CASES["same_pos_other_sn_base"])
    assert a["pos"].tolist() == [9, 9, 30] and ga.tolist() == [1, 2, 3] and a["aux"].tolist() == [0, 2, 1]
    (a, pa, ga), _, _ = check_host(CASES["same_pos_other_ins_bytes"])
    assert a["pos"].tolist() == [12, 12, 50] and ga.tolist() == [1, 2, 3]
    assert [tw.insert_of(r, pa) for r in a] == [b"GT", b"GA", b"AC"]
    # pool offsets: the merged insert keeps H1's offset, H2's own insert reads its bytes through the rebased offset
    (a, pa, ga), _, _ = check_host(CASES["ins_pool_offsets"])
    assert ga.tolist() == [1, 3, 2] and a["extra"].tolist() == [0, 2, 5 + 3] and pa.tobytes() == b"GTACGACGTTA"
    assert [tw.insert_of(r, pa) for r in a] == [b"GT", b"ACG", b"TTA"]
    # the duplicates at a scan tile's edge: H2's records TILE - 1 and TILE
    _, truth, _, _ = CASES["dup_at_tile_edge"]
    h1, _, h2, _ = truth
    assert len(h2) == TILE + 4 and [int(np.flatnonzero(h2["pos"] == p)[0]) for p in h1["pos"][1:]] == [7, TILE - 1, TILE]
    (a, _, ga), _, _ = check_host(CASES["dup_at_tile_edge"])
    assert int((ga == 3).sum()) == 3 and int((ga == 1).sum()) == 1 and len(a) == TILE + 5
    h1, _, h2, _ = CASES["h2_all_duplicates"][1]
    (a, _, ga), _, _ = check_host(CASES["h2_all_duplicates"])
    assert len(h1) > len(h2) > TILE - 30 and len(a) == len(h1) and int((ga == 3).sum()) == len(h2) and not (ga == 2).any()
    for n2 in (PASS - 1, PASS, PASS + 1, TILE - 1, TILE, TILE + 1):
        assert len(CASES[f"sn_pair_{n2}"][1][2]) == n2


def test_refusals_of_the_restatements_and_of_a_host_only_context():
    bases, truth, calls, _ = CASES["disjoint"]
    h1, p1, h2, p2 = truth
    bad = h1.copy()
    bad["type"][1] = 9
    with pytest.raises(_ffi.MsimError, match="haplotype 1 record 1: unknown type") as e:
        _ffi.cmp_join_host(bad, p1, h2, p2)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="haplotype 2 record 1: unknown type"):
        _ffi.cmp_join_host(h2, p2, bad, p1)
    with pytest.raises(_ffi.MsimError, match="haplotype 1 record 1: the table is not sorted by pos"):
        _ffi.cmp_join_host(h1[[1, 0]], p1, h2, p2)
    a, pa, ga = _ffi.cmp_join_host(h1, p1, h2, p2)
    b, pb, gb = _ffi.cmp_join_host(*calls)
    with pytest.raises(_ffi.MsimError, match="truth record 1: unknown type") as e:
        _ffi.cmp_counts_diploid_host(bases, bad, p1, np.ones(len(bad), np.uint8), b, pb, gb)
    assert e.value.code == _ffi.ERR_ARG
    for wrong in (0, 4, 255):
        gt = gb.copy()
        gt[2] = wrong
        with pytest.raises(_ffi.MsimError, match="calls record 2: genotype byte outside 1..3") as e:
            _ffi.cmp_counts_diploid_host(bases, a, pa, ga, b, pb, gt)
        assert e.value.code == _ffi.ERR_ARG
    # a NULL table with a count
    lib = _ffi.load()
    n = C.c_uint64()
    out, gt, pool = np.zeros(8, _ffi.RECORD_DTYPE), np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    assert lib.msim_dbg_cmp_join(None, 3, None, 0, None, 0, None, 0, _ffi._ptr(out), _ffi._ptr(pool), _ffi._ptr(gt), C.byref(n)) == _ffi.ERR_ARG
    assert lib.msim_dbg_cmp_join(None, 0, None, 2, None, 0, None, 0, _ffi._ptr(out), _ffi._ptr(pool), _ffi._ptr(gt), C.byref(n)) == _ffi.ERR_ARG
    counts, tallies = np.zeros((8, _ffi.CMP_BINS, 6), np.uint64), np.zeros(2, np.uint64)
    assert lib.msim_dbg_cmp_counts_diploid(None, 0, None, 2, None, 0, None, None, 0, None, 0, None, 0, _ffi._ptr(counts),
                                           _ffi._ptr(tallies), None, None) == _ffi.ERR_ARG
    assert lib.msim_dbg_cmp_counts_diploid(None, 0, _ffi._ptr(out), 2, None, 0, None, None, 0, None, 0, None, 0, _ffi._ptr(counts),
                                           _ffi._ptr(tallies), None, None) == _ffi.ERR_ARG          # records without genotypes
    # the join's size refusals need no table that large: the sizes are judged first
    rc = lib.msim_dbg_cmp_join(_ffi._ptr(out), 1 << 30, None, 0, _ffi._ptr(out), 1 << 30, None, 0, _ffi._ptr(out), _ffi._ptr(pool),
                               _ffi._ptr(gt), C.byref(n))
    assert rc == _ffi.ERR_UNSUPPORTED and "2^31 records" in lib.msim_last_error(None).decode()
    rc = lib.msim_dbg_cmp_join(None, 0, _ffi._ptr(pool), 1 << 31, None, 0, _ffi._ptr(pool), 1 << 31, _ffi._ptr(out), _ffi._ptr(pool),
                               _ffi._ptr(gt), C.byref(n))
    assert rc == _ffi.ERR_UNSUPPORTED and "4 GiB" in lib.msim_last_error(None).decode()
    with _ffi.Engine(-1) as eng:
        cid = eng.add_contig(bases)
        eng.set_records(cid, h1, p1)
        for call in (lambda: eng.cmp_join(cid, _ffi.CMP_TRUTH), lambda: eng.cmp_counts_diploid(cid),
                     lambda: eng.cmp_fetch_diploid(cid, _ffi.CMP_TRUTH)):
            with pytest.raises(_ffi.MsimError, match="needs the GPU") as e:
                call()
            assert e.value.code == _ffi.ERR_HIP
        assert eng.cmp_join_timing() == 0.0


# ------------------------------------------------------------------------------ 2. the file
def test_rendering_with_the_gt_column_and_na_cells():
    counts = np.zeros((2, 8, _ffi.CMP_BINS, 6), dtype=np.uint64)
    counts[0, tw.SN, 0] = (80, 10, 10, 80, 10, 30)
    counts[1, tw.SN, 0] = (10, 0, 0, 10, 0, 0)
    counts[0, tw.DE, 1] = (0, 0, 4, 0, 0, 0)               # truth only: precision has no denominator
    counts[1, tw.IN, 4] = (0, 0, 0, 0, 0, 2)               # calls only: recall has none
    counts[1, tw.IN, 0] = (0, 3, 0, 0, 3, 0)               # found, every one with the wrong genotype
    text = compare.render(["a note", "another"], counts, ["chr1", "chr 2"])
    lines = text.splitlines()
    assert compare.HEADER_DIPLOID == ("type", "length", "truth", "calls", "TP", "FN", "FP", "GT", "recall", "precision")
    assert lines[:2] == ["# a note", "# another"] and lines[2] == "\t".join(compare.HEADER_DIPLOID)
    assert text.endswith("\n") and len(lines) == 2 + 3 * 17 + 2
    rows = {tuple(l.split("\t")[:2]): l.split("\t")[2:] for l in lines[3:19]}
    assert [l.split("\t")[:2] for l in lines[3:19]] == (
        [["SN", "."]] + [["IN", b] for b in compare.BIN_NAMES] + [["DE", b] for b in compare.BIN_NAMES] +
        [["DU", "."], ["IV", "."], ["TL", "."], ["TLI", "."], ["ALL", "."]])
    assert rows[("SN", ".")] == ["110", "130", "90", "20", "40", "10", "0.818182", "0.692308"]       # FN and FP include GT
    assert rows[("DE", "2-5")] == ["4", "0", "0", "4", "0", "0", "0.000000", "NA"]
    assert rows[("IN", "51+")] == ["0", "2", "0", "0", "2", "0", "NA", "0.000000"]
    assert rows[("IN", "1")] == ["3", "3", "0", "3", "3", "3", "0.000000", "0.000000"]
    assert rows[("DU", ".")] == ["0", "0", "0", "0", "0", "0", "NA", "NA"]
    assert rows[("ALL", ".")] == ["117", "135", "90", "27", "45", "13", "0.769231", "0.666667"]
    assert lines[19] == "# contig chr1" and lines[37] == "# contig chr 2"
    assert lines[21].split("\t") == ["SN", ".", "100", "120", "80", "20", "40", "10", "0.800000", "0.666667"]
    assert lines[39].split("\t") == ["SN", ".", "10", "10", "10", "0", "0", "0", "1.000000", "1.000000"]
    assert compare.render([], counts).count("\n") == 17
    # the haploid renderers are what they were
    assert compare.HEADER == ("type", "length", "truth", "calls", "TP", "FN", "FP", "recall", "precision")
    assert compare.render([], np.zeros((1, 8, _ffi.CMP_BINS, 4), np.uint64)).splitlines()[0] == "\t".join(compare.HEADER)


def test_record_rows():
    # the truth carries five records on both haplotypes and a DU and a TLI that differ between them; the calls are haplotype 2's
    # records, every one het: the five are found with the wrong genotype, haplotype 1's DU and TLI are missed
    (a, pa, ga), (b, pb, gb), got = check_host(CASES["every_type_changed_exact"])
    rows = compare.record_rows_diploid("chr1", a, ga, got[2], b, gb, got[3])
    assert rows == ["GT\tchr1\t6\tSN\t1\t1/1\t0/1", "GT\tchr1\t11\tIN\t2\t1/1\t0/1", "GT\tchr1\t21\tDE\t3\t1/1\t0/1",
                    "FN\tchr1\t31\tDU\t4\t0/1\t.", "GT\tchr1\t41\tIV\t5\t1/1\t0/1", "GT\tchr1\t51\tTL\t5\t1/1\t0/1",
                    "FN\tchr1\t61\tTLI\t-5\t0/1\t."]
    kinds = set()
    for name in sorted(CASES):
        (a, pa, ga), (b, pb, gb), got = check_host(CASES[name])
        rows = compare.record_rows_diploid("chr1", a, ga, got[2], b, gb, got[3])
        want = [f"{k}\tchr1\t{p + 1}\t{compare.TYPE_NAMES[t]}\t{n}\t{x}\t{y}" for k, p, t, n, x, y in dt.listed(a, ga, got[2], b, gb, got[3])]
        assert rows == want, name
        kinds |= {r.split("\t")[0] for r in rows}
    assert kinds == {"FN", "GT", "FP"}
    (a, pa, ga), (b, pb, gb), got = check_host(CASES["hom_het"])
    assert compare.record_rows_diploid("c", a, ga, got[2], b, gb, got[3]) == ["GT\tc\t21\tIN\t2\t1/1\t0/1"]
    (a, pa, ga), (b, pb, gb), got = check_host(CASES["shifted_across_haplotypes"])
    assert compare.record_rows_diploid("c", a, ga, got[2], b, gb, got[3]) == ["GT\tc\t3\tDE\t1\t0/1\t1/1", "FN\tc\t8\tDE\t1\t0/1\t."]


# ------------------------------------------------------------------------------ 3. the command line
def test_diploid_is_in_the_compare_namespace_only():
    a = ap.get_args(["-o", "out", "genome.fa", "compare", "truth.vcf", "calls.vcf"])
    assert a.diploid is False
    a = ap.get_args(["genome.fa", "compare", "t.vcf", "c.vcf", "--diploid", "--truth-sample", "T", "--sample", "S", "--exact",
                     "--per-contig", "--list"])
    assert (a.diploid, a.truth_sample, a.sample, a.truth_haplotype, a.haplotype, a.exact, a.per_contig, a.list_records) == (
        True, "T", "S", None, None, True, True, True)
    assert ap.compare_refusal(a) is None
    for argv in (["genome.fa", "vcf", "x.vcf"], ["genome.fa", "vcf", "x.vcf", "--consensus"], ["genome.fa", "args", "-sn", "0.1"],
                 ["genome.fa", "rmt", "x.rmt"], ["genome.fa", "it", "0.1"], ["genome.fa", "profile", "x.vcf"]):
        assert not hasattr(ap.get_args(argv), "diploid"), argv


@pytest.mark.parametrize("argv", [
    ["genome.fa", "compare", "t.vcf", "c.vcf", "--diploid", "--haplotype", "1"],
    ["genome.fa", "compare", "t.vcf", "c.vcf", "--diploid", "--truth-haplotype", "2"],
    ["genome.fa", "vcf", "x.vcf", "--diploid"],
    ["genome.fa", "profile", "x.vcf", "--diploid"],
    ["genome.fa", "args", "-sn", "0.1", "--diploid"],
])
def test_usage_errors(argv):
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
        ap.get_args(argv)
    assert ei.value.code == 2 and "usage:" in err.getvalue()
    if argv[1] == "compare":
        assert "--haplotype and --truth-haplotype do not apply" in err.getvalue()
