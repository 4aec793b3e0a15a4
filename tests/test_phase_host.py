"""``compare --diploid --phased`` without a GPU: the grammar of a line's phase word (``msim_dbg_vcf_phase_word``) on hand-written
lines, the library's sequential restatement of the pass (``msim_dbg_cmp_phase``) against ``phase_twin`` on every shape the GPU tier
runs, the switch / flip decomposition in closed form, the file writer, the header's constants and the command line's names and
usage errors.  All comparisons are exact integers and bytes."""
from __future__ import annotations

import contextlib
import io
import re
from pathlib import Path

import numpy as np
import pytest

import phase_twin as pt
from mutation_simulator_amd import _ffi, argument_parser as ap, compare

TILE, PASS = _ffi.CMP_PHASE_TILE, _ffi.CMP_PASS
CASES = pt.small_cases(TILE, PASS)
CONTIG = _ffi.PHASE_CONTIG
NAMES = ("truth.het.phased", "calls.het.phased", "pairs", "blocks", "singletons", "assessed", "switch.raw", "switches", "flips", "hamming",
         "pairs in blocks of two or more")


def named(out):
    return dict(zip(NAMES, (int(x) for x in out)))


def check_host(case):
    """The restatement against the twin; returns (the named counts, the truth's state bytes)."""
    bases, (a, pa, ga, wa), (b, pb, gb, wb), exact = pt.tables_of(case)
    got = _ffi.cmp_phase_host(bases, a, pa, ga, wa, b, pb, gb, wb, exact)
    want = pt.tally(bases, a, pa, ga, wa, b, pb, gb, wb, exact)
    assert got[0].dtype == np.uint64 and got[0].shape == (_ffi.CMP_PHASE_COUNTS,) and got[1].shape == (len(a),)
    assert named(got[0]) == named(want[0])
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:8]
    n = named(got[0])
    assert n["assessed"] == n["pairs"] - n["blocks"] and n["switches"] + 2 * n["flips"] == n["switch.raw"] <= n["assessed"]
    assert n["pairs in blocks of two or more"] == n["pairs"] - n["singletons"] and n["hamming"] <= n["pairs"] // 2
    assert n["pairs"] == int((got[1] != 0).sum()) <= min(n["truth.het.phased"], n["calls.het.phased"])
    assert n["switch.raw"] == int((got[1] & 2 != 0).sum())
    return n, got[1]


# ------------------------------------------------------------------------------ 1. the grammar
def line(fmt: str, *samples: str) -> bytes:
    f = ["c", "10", ".", "A", "C", ".", "PASS", "."] + ([fmt, *samples] if fmt else [])
    return "\t".join(f).encode()


@pytest.mark.parametrize("text, nf0, sample, want", [
    (line("GT", "0|1"), 10, 0, (CONTIG, False)),
    (line("GT", "1|0"), 10, 0, (CONTIG, False)),
    (line("GT", "0/1"), 10, 0, (0, False)),
    (line("GT", "1"), 10, 0, (0, False)),
    (line("GT", "1|2"), 10, 0, (CONTIG, False)),
    (line("GT", ".|1"), 10, 0, (CONTIG, False)),
    (line("GT", "0|1/1"), 10, 0, (0, False)),
    (line("GT:PS", "0|1:77"), 10, 0, (77, False)),
    (line("GT:PS", "0|1:."), 10, 0, (CONTIG, False)),
    (line("GT:PS", "0|1:"), 10, 0, (CONTIG, False)),
    (line("GT:PS", "0|1"), 10, 0, (CONTIG, False)),
    (line("GT:PS", "0/1:77"), 10, 0, (0, False)),
    (line("GT:DP:GQ:PS", "1|0:30:99:1234567"), 10, 0, (1234567, False)),
    (line("GT:DP:GQ:PS", "1|0:30"), 10, 0, (CONTIG, False)),
    (line("GT:PSX:PS", "1|0:5:6"), 10, 0, (6, False)),
    (line("GT:XPS:PS", "1|0:5:6"), 10, 0, (6, False)),
    (line("GT:PSX", "1|0:5"), 10, 0, (CONTIG, False)),
    (line("GT:XPS", "1|0:5"), 10, 0, (CONTIG, False)),
    (line("GT:PS:PS", "1|0:5:6"), 10, 0, (5, False)),
    (line("GT:PS", "0|1:0"), 10, 0, (0, True)),
    (line("GT:PS", "0|1:-1"), 10, 0, (0, True)),
    (line("GT:PS", "0|1:+1"), 10, 0, (0, True)),
    (line("GT:PS", "0|1:7a"), 10, 0, (0, True)),
    (line("GT:PS", "0|1:4294967295"), 10, 0, (0, True)),
    (line("GT:PS", "0|1:4294967294"), 10, 0, (4294967294, False)),
    (line("GT:PS", "0|1:0000000012"), 10, 0, (12, False)),
    (line("GT:PS", "0|1:12345678901"), 10, 0, (0, True)),
    (line("GT:PS", "0|1:9999999999"), 10, 0, (0, True)),
    (line("GT:PS", "0|1:3", "0/1:4", "1|0:5"), 12, 0, (3, False)),
    (line("GT:PS", "0|1:3", "0/1:4", "1|0:5"), 12, 1, (0, False)),
    (line("GT:PS", "0|1:3", "0/1:4", "1|0:5"), 12, 2, (5, False)),
    (line("GT:PS", "0|1:3", "0/1:4", "1|0:5"), 12, 3, (0, False)),      # no such sample column
    (line("GT:PS", "0|1:3", "0/1:4", "1|0:5"), 10, 0, (0, False)),      # not the file's field count
    (line(""), 8, 0, (0, False)),
    (line("DP:GT", "30:0|1"), 10, 0, (0, False)),
    (b"", 10, 0, (0, False)),
])
def test_phase_word(text, nf0, sample, want):
    assert _ffi.vcf_phase_word(text, nf0, sample) == want
    assert pt.phase_word(text, nf0, sample) == want


def test_phase_word_reads_its_line_only():
    """The same buffer cut shorter: the bytes behind the line's end would change the answer if they were read."""
    body = line("GT:PS", "0|1:42")
    assert _ffi.vcf_phase_word(body, 10) == (42, False)
    assert _ffi.vcf_phase_word(body[:-1], 10) == (4, False) and _ffi.vcf_phase_word(body[:-3], 10) == (CONTIG, False)


# ------------------------------------------------------------------------------ 2. the pass
@pytest.mark.parametrize("case", sorted(CASES))
def test_small_shapes(case):
    n, state = check_host(CASES[case])
    want = {
        "no_pair": (2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), "no_records": (0,) * 11, "truth_empty": (0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0),
        "one_pair": (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0), "one_pair_swapped": (1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0),
        "two_pairs_one_block": (2, 2, 2, 1, 0, 1, 1, 1, 0, 1, 2), "two_pairs_two_blocks": (2, 2, 2, 2, 2, 0, 0, 0, 0, 0, 0),
        "key_change_truth": (5, 5, 5, 2, 0, 3, 2, 2, 0, 2, 5), "key_change_calls": (5, 5, 5, 2, 0, 3, 1, 1, 0, 1, 5),
        "key_change_both": (6, 6, 6, 2, 0, 4, 4, 0, 2, 2, 6), "key_returns": (6, 6, 6, 3, 0, 3, 0, 0, 0, 0, 6),
        "genotype_mismatch_between": (4, 3, 3, 1, 0, 2, 1, 1, 0, 1, 3), "two_at_one_pos": (5, 5, 5, 1, 0, 4, 2, 2, 0, 2, 5),
        "shifted_indel": (4, 4, 4, 1, 0, 3, 2, 0, 1, 1, 4), "shifted_indel_exact": (4, 4, 3, 1, 0, 2, 0, 0, 0, 0, 3),
        "shifted_insert": (3, 3, 3, 3, 3, 0, 0, 0, 0, 0, 0), "all_swapped": (9, 9, 9, 1, 0, 8, 0, 0, 0, 0, 9),
    }.get(case)
    if want:
        assert tuple(n.values()) == want, n
    if case == "transparent_between":
        # o = 0 1 1 0 with a hom, an unphased het and a genotype mismatch behind every pair: one block, two lone switch bits
        assert (n["pairs"], n["blocks"], n["switch.raw"], n["switches"], n["flips"], n["hamming"]) == (4, 1, 2, 2, 0, 2)
        assert state.tolist()[::4] == [1, 7, 5, 3] and not state.reshape(-1, 4)[:, 1:].any()
    if case == "long_gap":
        assert (n["pairs"], n["blocks"], n["switch.raw"]) == (2, 1, 1) and np.flatnonzero(state).tolist() == [0, 2 * TILE + 4]
    if case.startswith("records_"):
        assert n["pairs"] == int(case.split("_")[1]) and n["blocks"] == 1


@pytest.mark.parametrize("r, switches, flips", [(1, 1, 0), (2, 0, 1), (3, 1, 1), (4, 0, 2), (5, 1, 2)])
def test_a_run_of_raw_switch_bits(r, switches, flips):
    n, state = check_host(CASES[f"run_of_{r}"])
    assert (n["switch.raw"], n["switches"], n["flips"], n["blocks"], n["pairs"]) == (r, switches, flips, 1, r + 4)
    assert (state & 2 != 0).tolist() == [False, False] + [True] * r + [False, False]


def test_both_haplotypes_swapped_over_a_block():
    n, state = check_host(CASES["all_swapped"])
    assert (n["switch.raw"], n["switches"], n["flips"], n["hamming"], n["blocks"]) == (0, 0, 0, 0, 1) and (state == 5).all()


def test_the_tile_edges_are_in_the_cases():
    n, state = check_host(CASES["tile_edge_run_and_block"])
    dense = np.flatnonzero(state)
    assert len(dense) == TILE + 5 and (state[dense] & 2 != 0).nonzero()[0].tolist() == [TILE - 2, TILE - 1, TILE, TILE + 1]
    assert (n["blocks"], n["flips"], n["switches"]) == (2, 2, 0)
    for at in (TILE - 1, TILE, TILE + 1):
        n, state = check_host(CASES[f"run_ends_at_{at}"])
        assert (n["switch.raw"], n["flips"], n["switches"]) == (at, at // 2, at % 2)
        n, state = check_host(CASES[f"block_starts_at_{at}"])
        assert n["blocks"] == 2 and n["pairs in blocks of two or more"] == n["pairs"] == at + 4
    n, _ = check_host(CASES["random_three_tiles"])
    assert n["pairs"] == 3 * TILE + 5 and n["blocks"] > 10 and n["flips"] > 10 and n["switches"] > 10


def test_refusals():
    bases, (a, pa, ga, wa), (b, pb, gb, wb), _ = pt.tables_of(CASES["two_pairs_one_block"])
    for bad in (0, 4):
        g = ga.copy()
        g[0] = bad
        with pytest.raises(_ffi.MsimError, match="genotype byte outside 1..3"):
            _ffi.cmp_phase_host(bases, a, pa, g, wa, b, pb, gb, wb)
    with pytest.raises(_ffi.MsimError, match="not sorted by pos"):
        _ffi.cmp_phase_host(bases, a[::-1], pa, ga, wa, b, pb, gb, wb)
    r = a.copy()
    r["type"][0] = 9
    with pytest.raises(_ffi.MsimError, match="unknown type"):
        _ffi.cmp_phase_host(bases, r, pa, ga, wa, b, pb, gb, wb)


# ------------------------------------------------------------------------------ 3. the file and the header
def test_rendered_table():
    outs = np.array([[10, 9, 8, 2, 1, 6, 3, 1, 1, 2, 7], [4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint64)
    text = compare.render_phase(["a note"], outs, ["ctgA", "ctgB"])
    assert text == "# a note\n" + pt.table_text(outs, ["ctgA", "ctgB"])
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    assert rows[0] == list(pt.HEADER) == list(compare.PHASE_HEADER)
    assert rows[1] == ["ALL", "14", "13", "8", "2", "1", "6", "3", "0.500000", "1", "1", "0.333333", "2", "0.285714"]
    assert rows[3] == ["ctgB", "4", "4", "0", "0", "0", "0", "0", "NA", "0", "0", "NA", "0", "NA"]
    assert compare.render_phase([], outs) == pt.table_text(outs)
    bases, (a, pa, ga, wa), (b, pb, gb, wb), _ = pt.tables_of(CASES["two_at_one_pos"])
    state = _ffi.cmp_phase_host(bases, a, pa, ga, wa, b, pb, gb, wb)[1]
    assert compare.switch_rows("c", a, ga, state) == pt.switch_lines("c", a, ga, state) == [
        "SW\tc\t13\tSN\t1\t1|0\t0|1", "SW\tc\t20\tSN\t1\t1|0\t1|0"]


def test_header_constants():
    text = (Path(__file__).resolve().parents[1] / "include" / "msim.h").read_text()
    defines = dict(re.findall(r"^#define (MSIM_\w+)\s+(\S+)", text, re.M))
    assert defines["MSIM_ABI_VERSION"] == "8" and _ffi.load().msim_abi_version() == 8
    assert int(defines["MSIM_PHASE_CONTIG"].rstrip("u"), 16) == _ffi.PHASE_CONTIG == pt.CONTIG == 0xFFFFFFFF
    assert int(defines["MSIM_CMP_PHASE_TILE"]) == _ffi.CMP_PHASE_TILE
    assert int(defines["MSIM_CMP_PHASE_COUNTS"]) == _ffi.CMP_PHASE_COUNTS == pt.N_COUNTS == len(NAMES)
    for name in ("msim_cmp_phase_mark", "msim_cmp_phase_join", "msim_cmp_phase_set", "msim_cmp_phase_counts", "msim_cmp_fetch_phase",
                 "msim_cmp_phase_timing", "msim_dbg_cmp_phase", "msim_dbg_vcf_phase_word"):
        assert re.search(rf"^int {name}\(", text, re.M) and hasattr(_ffi.load(), name), name


def test_device_entries_on_a_host_only_context():
    e = _ffi.Engine(-1)
    try:
        for call in (lambda: e.cmp_phase_mark(0, 0, 1), lambda: e.cmp_phase_join(0, 0), lambda: e.cmp_phase_set(0, 0, np.zeros(1, np.uint32)),
                     lambda: e.cmp_phase_counts(0)):
            with pytest.raises(_ffi.MsimError, match="host-only context") as ei:
                call()
            assert ei.value.code == _ffi.ERR_HIP
        assert e.cmp_phase_timing() == 0.0
    finally:
        e.close()


# ------------------------------------------------------------------------------ 4. the command line
def test_names():
    args = ap.get_args(["-o", "out/base", "genome.fa", "compare", "t.vcf", "c.vcf", "--diploid", "--phased", "--per-contig"])
    assert args.phased and args.diploid and args.outcompare_phase == Path("out/base_ms.compare.phase.tsv")
    assert not ap.get_args(["genome.fa", "compare", "t.vcf", "c.vcf", "--diploid"]).phased


@pytest.mark.parametrize("argv, message", [
    (["genome.fa", "compare", "t.vcf", "c.vcf", "--phased"], "--phased needs --diploid"),
    (["genome.fa", "compare", "t.vcf", "c.vcf", "--phased", "--blocks"], "--phased compares the phasing of a diploid comparison: it cannot be combined with --blocks"),
    (["genome.fa", "compare", "t.vcf", "c.vcf", "--phased", "--haplotype", "2"], "--phased needs --diploid"),
])
def test_usage_errors(argv, message):
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
        ap.get_args(argv)
    assert ei.value.code == 2 and "usage:" in err.getvalue() and message in err.getvalue()
