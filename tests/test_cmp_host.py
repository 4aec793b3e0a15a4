"""The ``compare`` mode without a GPU: the library's sequential restatement (``msim_dbg_cmp_counts``) against ``cmp_twin`` on
every shape the GPU tier runs, the twin's stepwise rules against its brute-force oracle (``apply_ref.apply`` of one record, no
shifting code), the file writer, and the command line's names, refusals and usage errors.  All comparisons are exact integers."""
from __future__ import annotations

import contextlib
import io
from pathlib import Path

import numpy as np
import pytest

import cmp_twin as tw
from mutation_simulator_amd import _ffi, argument_parser as ap, compare

PASS = _ffi.CMP_PASS
CASES = tw.small_cases(PASS)
NEW_NAMES = ("truthfile", "callsfile", "truth_sample", "truth_haplotype", "exact", "list_records", "outcompare", "outcompare_records")


def check_host(case):
    bases, a, pa, b, pb, exact = case
    want = tw.compare(bases, a, pa, b, pb, exact)
    got = _ffi.cmp_counts_host(bases, a, pa, b, pb, exact)
    assert got[0].dtype == np.uint64 and got[0].shape == (8, _ffi.CMP_BINS, 4) and got[1].shape == (2,)
    for name, g, w in zip(("counts", "tallies", "truth flags", "calls flags"), got, want):
        assert np.array_equal(g, w), (name, g.tolist(), w.tolist())
    counts = got[0]
    assert np.array_equal(counts[..., 0], counts[..., 2])                      # truth matched == calls matched, every cell
    assert int(counts[..., :2].sum()) == len(a) and int(counts[..., 2:].sum()) == len(b)
    assert int(got[2].sum()) == int(got[3].sum()) == int(counts[..., 0].sum())
    return got


# ------------------------------------------------------------------------------ 1. the counts
def test_constants_are_the_headers():
    header = (Path(__file__).resolve().parent.parent / "include" / "msim.h").read_text()
    assert f"#define MSIM_CMP_PASS   {PASS}\n" in header and PASS % 64 == 0
    assert "#define MSIM_CMP_WINDOW 65536\n" in header and "#define MSIM_CMP_BINS   5\n" in header
    assert "#define MSIM_CMP_EXACT  1u\n" in header and "#define MSIM_ABI_VERSION 8\n" in header
    assert (_ffi.CMP_WINDOW, _ffi.CMP_BINS, _ffi.CMP_EXACT) == (1 << tw.WINDOW_SHIFT, tw.BINS, 1)


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_restatement_equals_the_twin(case):
    check_host(CASES[case])


def matched(case):
    counts = check_host(CASES[case])[0]
    return int(counts[..., 0].sum()), int(counts[..., 1].sum()), int(counts[..., 3].sum())


def test_what_the_named_cases_are_about():
    """The twin and the library agree on every case (above); here the cases' own claims, in plain numbers (TP, FN, FP)."""
    for case, want in {"homopolymer_ends": (1, 0, 0), "homopolymer_ends_exact": (0, 1, 1), "homopolymer_lengths": (0, 1, 1),
                       "repeat_rotated": (1, 0, 0), "repeat_other_bytes": (0, 1, 1), "repeat3_shift_2": (1, 0, 0),
                       "repeat_negative_shift": (1, 0, 0), "repeat3_wrong_rotation": (0, 1, 1), "end_pos0": (1, 0, 0),
                       "end_last_base": (1, 0, 0), "end_ins_last_base": (1, 0, 0), "stop_N": (0, 1, 1), "window_edge": (0, 1, 1),
                       "window_same_side": (1, 0, 0), "rank_2v1": (1, 1, 0), "rank_1v2": (1, 0, 1), "rank_3v2": (2, 1, 0),
                       "rank_3v2_truth_at_pass": (2, PASS, 0), "rank_3v2_calls_at_pass": (2, 1, PASS - 1),
                       "every_type": (7, 0, 0), "every_type_changed": (5, 2, 2), "sn_aux_differs": (1, 1, 1)}.items():
        assert matched(case) == want, case
    for case, tallies in {"stop_N": [0, 1], "stop_N_run": [0, 1], "window_edge": [1, 0], "window_edge_ins": [1, 0], "end_pos0": [0, 0],
                          "homopolymer_ends_exact": [0, 0]}.items():
        assert check_host(CASES[case])[1].tolist() == tallies, case
    a = CASES["rank_3v2_truth_at_pass"][1]
    assert a["type"][PASS - 1:].tolist() == [tw.DE] * 3 and len(a) == PASS + 2      # indices PASS - 1, PASS, PASS + 1
    b = CASES["rank_3v2_calls_at_pass"][3]
    assert b["type"][PASS - 1:].tolist() == [tw.DE] * 2
    # the rank rule: the first two of the truth's three are the matched ones
    assert check_host(CASES["rank_3v2"])[2].tolist() == [1, 1, 0]


def test_bin_edges_fall_into_their_bins():
    counts = check_host(CASES["bin_edges"])[0]
    for t in (tw.IN, tw.DE):
        assert (counts[t, :, 0] + counts[t, :, 1]).tolist() == [1, 2, 2, 2, 1]         # 1 | 2, 5 | 6, 20 | 21, 50 | 51
    assert [tw.length_bin(n) for n in (1, 2, 5, 6, 20, 21, 50, 51, 10 ** 6)] == [0, 1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("seed", range(6))
def test_stepwise_rules_equal_the_brute_force_oracle(seed):
    """On a random 200-base contig over two letters: two same-type, same-length indels are one variant by the stepwise twin
    (the other's pos inside the interval, an insert's bytes what the moves make of them) iff applying each alone gives the
    same bytes -- for every position of a deletion, and for the placements and a sample of foreign inserts."""
    rs = np.random.RandomState(seed)
    g = np.frombuffer(b"AC", dtype=np.uint8)[rs.randint(0, 2, 200)].copy()
    L = len(g)
    for n in (1, 2, 3, 5):
        for pos in rs.randint(0, L - n, 6).tolist():
            pl, stops = tw.placements(g, tw.DE, pos, n)
            assert stops == 0 and sorted(pl) == list(range(min(pl), max(pl) + 1))
            same = [q for q in range(L - n + 1) if tw.brute_same(g, tw.DE, n, pos, b"", q, b"")]
            assert same == sorted(pl), (n, pos)
            S = bytes(b"AC"[int(x)] for x in rs.randint(0, 2, n))
            pl, stops = tw.placements(g, tw.IN, pos, n, S)
            assert stops == 0
            for q in range(max(0, min(pl) - 3), min(L - 1, max(pl) + 3) + 1):
                for T in {pl[q][3] if q in pl else S, S, S[1:] + S[:1]}:
                    assert tw.brute_same(g, tw.IN, n, pos, S, q, T) == (q in pl and pl[q][3] == T), (n, pos, S, q, T)
            # ... and the rule of msim.h: S_b[i] == S_a[(i + d) mod n]
            for q, (_, _, _, T) in pl.items():
                assert all(T[i] == S[(i + q - pos) % n] for i in range(n))


def test_refusals_of_the_restatement_and_of_a_host_only_context():
    bases, a, pa, b, pb, _ = CASES["identical"]
    bad = a.copy()
    bad["type"][1] = 9
    with pytest.raises(_ffi.MsimError, match="truth record 1: unknown type") as e:
        _ffi.cmp_counts_host(bases, bad, pa, b, pb)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="calls record 1: unknown type"):
        _ffi.cmp_counts_host(bases, a, pa, bad, pb)
    with _ffi.Engine(-1) as eng:
        cid = eng.add_contig(bases)
        eng.set_records(cid, a, pa)
        for call in (lambda: eng.cmp_hold(cid), lambda: eng.cmp_counts(cid), lambda: eng.cmp_fetch(cid)):
            with pytest.raises(_ffi.MsimError, match="needs the GPU") as e:
                call()
            assert e.value.code == _ffi.ERR_HIP
        eng.cmp_release()
        assert eng.cmp_timing() == 0.0


# ------------------------------------------------------------------------------ 2. the file
def test_rendering_with_na_cells():
    counts = np.zeros((2, 8, _ffi.CMP_BINS, 4), dtype=np.uint64)
    counts[0, tw.SN, 0] = (90, 10, 90, 30)
    counts[1, tw.SN, 0] = (10, 0, 10, 0)
    counts[0, tw.DE, 1] = (0, 4, 0, 0)                     # truth only: precision has no denominator
    counts[1, tw.IN, 4] = (0, 0, 0, 2)                     # calls only: recall has none
    text = compare.render(["a note", "another"], counts, ["chr1", "chr 2"])
    lines = text.splitlines()
    assert lines[:2] == ["# a note", "# another"] and lines[2] == "\t".join(compare.HEADER)
    assert text.endswith("\n") and len(lines) == 2 + 3 * 17 + 2
    rows = {tuple(l.split("\t")[:2]): l.split("\t")[2:] for l in lines[3:19]}
    assert [l.split("\t")[:2] for l in lines[3:19]] == (
        [["SN", "."]] + [["IN", b] for b in compare.BIN_NAMES] + [["DE", b] for b in compare.BIN_NAMES] +
        [["DU", "."], ["IV", "."], ["TL", "."], ["TLI", "."], ["ALL", "."]])
    assert rows[("SN", ".")] == ["110", "130", "100", "10", "30", "0.909091", "0.769231"]
    assert rows[("DE", "2-5")] == ["4", "0", "0", "4", "0", "0.000000", "NA"]
    assert rows[("IN", "51+")] == ["0", "2", "0", "0", "2", "NA", "0.000000"]
    assert rows[("DU", ".")] == ["0", "0", "0", "0", "0", "NA", "NA"]
    assert rows[("ALL", ".")] == ["114", "132", "100", "14", "32", "0.877193", "0.757576"]
    assert lines[19] == "# contig chr1" and lines[37] == "# contig chr 2"
    assert lines[21].split("\t") == ["SN", ".", "100", "120", "90", "10", "30", "0.900000", "0.750000"]
    assert lines[39].split("\t") == ["SN", ".", "10", "10", "10", "0", "0", "1.000000", "1.000000"]
    assert compare.render([], counts).count("\n") == 17    # no per-contig blocks without names


def test_record_rows():
    _, a, _, b, _, _ = CASES["every_type_changed"]
    got = _ffi.cmp_counts_host(*CASES["every_type_changed"][:5])
    rows = compare.record_rows("FN", "chr1", a, got[2]) + compare.record_rows("FP", "chr1", b, got[3])
    assert rows == ["FN\tchr1\t31\tDU\t4", "FN\tchr1\t61\tTLI\t-5", "FP\tchr1\t31\tDU\t5", "FP\tchr1\t61\tTLI\t-5"]
    want = [(k, p + 1, compare.TYPE_NAMES[t], n) for k, p, t, n in tw.unmatched(a, got[2], b, got[3])]
    assert [(r.split("\t")[0], int(r.split("\t")[2]), r.split("\t")[3], int(r.split("\t")[4])) for r in rows] == want


# ------------------------------------------------------------------------------ 3. the command line
def test_compare_namespace():
    a = ap.get_args(["-o", "out", "genome.fa", "compare", "truth.vcf", "calls.vcf.gz"])
    assert a.mode == "compare" and str(a.truthfile) == "truth.vcf" and str(a.callsfile) == "calls.vcf.gz"
    assert str(a.outcompare) == "out_ms.compare.tsv" and str(a.outcompare_records) == "out_ms.compare.records.tsv"
    assert (a.truth_sample, a.truth_haplotype, a.sample, a.haplotype, a.exact, a.per_contig, a.list_records) == (
        None, None, None, None, False, False, False)
    assert ap.compare_refusal(a) is None
    a = ap.get_args(["genome.fa", "compare", "t.vcf", "c.vcf", "--truth-sample", "T", "--truth-haplotype", "2", "--sample", "S1",
                     "--haplotype", "3", "--exact", "--per-contig", "--list"])
    assert (a.truth_sample, a.truth_haplotype, a.sample, a.haplotype, a.exact, a.per_contig, a.list_records) == (
        "T", 2, "S1", 3, True, True, True)
    assert str(a.outcompare) == "genome_ms.compare.tsv"


@pytest.mark.parametrize("argv", [["genome.fa", "vcf", "x.vcf"], ["genome.fa", "vcf", "x.vcf", "--consensus"],
                                  ["genome.fa", "args", "-sn", "0.1"], ["genome.fa", "rmt", "x.rmt"], ["genome.fa", "it", "0.1"],
                                  ["genome.fa", "profile", "x.vcf"]])
def test_the_other_modes_namespaces_carry_none_of_the_new_names(argv):
    other = ap.get_args(argv)
    assert not [name for name in NEW_NAMES if hasattr(other, name)]
    assert ap.compare_refusal(other) is None


@pytest.mark.parametrize("argv", [
    ["genome.fa", "compare", "t.vcf", "c.vcf", "--haplotype", "0"],
    ["genome.fa", "compare", "t.vcf", "c.vcf", "--truth-haplotype", "0"],
    ["genome.fa", "compare", "t.vcf", "c.vcf", "--truth-haplotype", "-1"],
    ["genome.fa", "compare", "t.vcf"],
    ["genome.fa", "compare"],
    ["genome.fa", "compare", "t.vcf", "c.vcf", "--consensus"],
    ["genome.fa", "vcf", "x.vcf", "--exact"],
    ["genome.fa", "profile", "x.vcf", "--list"],
    ["genome.fa", "args", "-sn", "0.1", "--truth-sample", "T"],
])
def test_usage_errors(argv):
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
        ap.get_args(argv)
    assert ei.value.code == 2 and "usage:" in err.getvalue()
    if argv[-1] in ("0", "-1"):
        assert "--haplotype and --truth-haplotype count from 1" in err.getvalue()


def _refused(monkeypatch, argv, message):
    """main(argv) exits with the message as an error, before a device or an output file is opened."""
    import mutation_simulator_amd.__main__ as msa_main

    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(_ffi, "warm_up_async", no_device)
    monkeypatch.setattr(_ffi, "Engine", no_device)
    err = io.StringIO()
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(SystemExit) as e:
            msa_main.main(argv)
    assert e.value.code == 1
    assert any(line.startswith("ERROR:") and message in line for line in err.getvalue().splitlines()), err.getvalue()


@pytest.mark.parametrize("front,message", [
    (["--ploidy", "2"], "--ploidy 2 does not apply to the compare mode"),
    (["--chain"], "--chain does not apply to the compare mode"),
    (["--bgzip"], "--bgzip does not apply to the compare mode"),
    (["--gpus", "2"], "the compare mode needs a single-GPU run (--gpus 1)"),
])
def test_refused_combinations(monkeypatch, tmp_path, front, message):
    _refused(monkeypatch, ["-c", *front, "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "compare", str(tmp_path / "t.vcf"),
                           str(tmp_path / "c.vcf")], message)
    assert not list(tmp_path.glob("out*"))
