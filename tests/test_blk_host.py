"""``compare --blocks`` without a GPU: the library's sequential restatement (``msim_dbg_cmp_counts_blocks``, built from
csrc/cmp_blocks.h) against ``blk_twin`` -- the rule in Python, its replay literally ``apply_ref.apply`` -- on every case the GPU tier
runs, the cases' own claims in plain numbers, the file writer and the command line's usage errors.  All comparisons are exact
integers."""
from __future__ import annotations

import contextlib
import io
from pathlib import Path

import numpy as np
import pytest

import blk_twin as bt
import cmp_twin as tw
from mutation_simulator_amd import _ffi, argument_parser as ap, compare

PASS = _ffi.CMP_PASS
CASES = bt.cases(PASS)
NAMES = ("counts", "tallies", "block tallies", "truth flags", "calls flags")


def check_host(name):
    bases, a, pa, b, pb, exact, gap = bt.random_case(name) if isinstance(name, int) else CASES[name]
    want = bt.expected(name, PASS)
    got = _ffi.cmp_counts_blocks_host(bases, a, pa, b, pb, exact, gap)
    assert got[0].dtype == np.uint64 and got[0].shape == (8, _ffi.CMP_BINS, 6) and got[1].shape == (2,) and got[2].shape == (5,)
    for what, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), (name, what, g.tolist(), w.tolist())
    counts, _, blocks, fa, fb = got
    assert int(counts[..., :3].sum()) == len(a) and int(counts[..., 3:].sum()) == len(b)
    assert np.array_equal(counts[..., 0], counts[..., 3])                      # matched one to one, block-matched not
    assert int(blocks[0]) == int(blocks[1]) + int(blocks[3]) + int(blocks[4]) and blocks[2] <= blocks[1]
    # the pass only rescues: what the match paired stays paired, and its flags are the haploid call's wherever they are not 2
    plain = _ffi.cmp_counts_host(bases, a, pa, b, pb, exact)
    assert np.array_equal(np.where(fa == 2, 0, fa), plain[2]) and np.array_equal(np.where(fb == 2, 0, fb), plain[3])
    assert np.array_equal(got[1], plain[1])
    return got


def totals(counts):
    """(TP, BLK, FN, TP.calls, BLK.calls, FP): TP and TP.calls hold the block-matched records."""
    s = [int(counts[..., k].sum()) for k in range(6)]
    return s[0] + s[1], s[1], s[2], s[3] + s[4], s[4], s[5]


# ------------------------------------------------------------------------------ 1. the library against the twin
def test_constants_are_the_headers():
    header = (Path(__file__).resolve().parent.parent / "include" / "msim.h").read_text()
    for name, value in (("MSIM_CMP_BLOCK_GAP    ", bt.GAP), ("MSIM_CMP_BLOCK_RECORDS", bt.MAX_RECORDS), ("MSIM_CMP_BLOCK_SPAN   ", bt.MAX_SPAN)):
        assert f"#define {name} {value}\n" in header
    assert (_ffi.CMP_BLOCK_GAP, _ffi.CMP_BLOCK_RECORDS, _ffi.CMP_BLOCK_SPAN) == (bt.GAP, bt.MAX_RECORDS, bt.MAX_SPAN)


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_restatement_equals_the_twin(case):
    check_host(case)


def test_what_the_named_cases_are_about():
    """The twin and the library agree on every case (above); here the cases' own claims: (TP, BLK, FN, TP.calls, BLK.calls, FP) and
    (candidates, replayed, equal, over a limit, holding a translocation)."""
    for case, want, blocks in (
            ("mnp_vs_snps", (2, 2, 0, 2, 2, 0), [1, 1, 1, 0, 0]), ("snps_vs_mnp", (2, 2, 0, 2, 2, 0), [1, 1, 1, 0, 0]),
            ("du_vs_in_at_start", (1, 1, 0, 1, 1, 0), [1, 1, 1, 0, 0]), ("du_vs_in_behind", (1, 1, 0, 1, 1, 0), [1, 1, 1, 0, 0]),
            ("in_vs_du", (1, 1, 0, 1, 1, 0), [1, 1, 1, 0, 0]), ("du_vs_other_in", (0, 0, 1, 0, 0, 1), [1, 1, 0, 0, 0]),
            ("iv_vs_transitions", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]), ("iv_palindrome_vs_nothing", (1, 1, 0, 0, 0, 0), [1, 1, 1, 0, 0]),
            ("nothing_vs_iv_palindrome", (0, 0, 0, 1, 1, 0), [1, 1, 1, 0, 0]),
            ("gap0_distance1", (0, 0, 2, 0, 0, 0), [2, 2, 0, 0, 0]), ("gap1_distance1", (2, 2, 0, 0, 0, 0), [1, 1, 1, 0, 0]),
            ("gap1_distance2", (0, 0, 2, 0, 0, 0), [2, 2, 0, 0, 0]), ("gap50_distance50", (2, 2, 0, 0, 0, 0), [1, 1, 1, 0, 0]),
            ("gap50_distance51", (0, 0, 2, 0, 0, 0), [2, 2, 0, 0, 0]),
            ("gap0_du_in_distance0", (1, 1, 0, 1, 1, 0), [1, 1, 1, 0, 0]), ("gap0_du_in_distance1", (0, 0, 1, 0, 0, 1), [2, 2, 0, 0, 0]),
            ("gap1_du_in_distance1", (1, 1, 0, 1, 1, 0), [1, 1, 1, 0, 0]),
            ("shifted_de_exact", (1, 1, 0, 1, 1, 0), [1, 1, 1, 0, 0]), ("shifted_de_normalised", (1, 0, 0, 1, 0, 0), [0, 0, 0, 0, 0]),
            ("records_64", (33, 3, 0, 31, 1, 0), [1, 1, 1, 0, 0]), ("records_65", (30, 0, 4, 30, 0, 1), [1, 0, 0, 1, 0]),
            ("span_4096", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]), ("span_4097", (0, 0, 1, 0, 0, 2), [1, 0, 0, 1, 0]),
            ("tl_in_block", (0, 0, 3, 0, 0, 0), [2, 0, 0, 0, 2]), ("tli_in_block", (0, 0, 3, 0, 0, 0), [2, 0, 0, 0, 2]),
            ("tl_is_record_65", (0, 0, 65, 0, 0, 0), [1, 0, 0, 0, 1]), ("de_is_record_65", (0, 0, 65, 0, 0, 0), [1, 0, 0, 1, 0]),
            ("block_at_pos0", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]), ("block_at_last_base", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]),
            ("whole_contig_one_block", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]),
            ("prefix_at_contig_end", (0, 0, 1, 0, 0, 1), [1, 1, 0, 0, 0]), ("prefix_inside", (0, 0, 1, 0, 0, 1), [1, 1, 0, 0, 0]),
            ("sn_on_R", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]), ("sn_on_N", (1, 1, 0, 0, 0, 0), [1, 1, 1, 0, 0]),
            ("sn_on_N_transversion", (1, 1, 0, 0, 0, 0), [1, 1, 1, 0, 0]), ("sn_on_lower_case", (1, 1, 0, 0, 0, 0), [1, 1, 1, 0, 0]),
            ("sn_key_error", (0, 0, 1, 0, 0, 0), [1, 1, 0, 0, 0]), ("iv_on_R", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]),
            ("iv_on_R_and_lower_case", (1, 1, 0, 2, 2, 0), [1, 1, 1, 0, 0]),
            ("one_unmatched_snp", (2, 0, 1, 2, 0, 0), [1, 1, 0, 0, 0]), ("shifted_pair_around_a_snp", (2, 0, 0, 2, 0, 0), [0, 0, 0, 0, 0])):
        counts, _, got_blocks, _, _ = check_host(case)
        assert totals(counts) == want, (case, totals(counts))
        assert got_blocks.tolist() == blocks, (case, got_blocks.tolist())


def test_grid_blocks_lie_across_a_pass():
    bases, a, pa, b, pb, exact, gap = CASES["grid"]
    assert len(a) == len(b) == 3 * PASS + 1
    counts, _, blocks, fa, fb = check_host("grid")
    for recs in (a, b):                                    # records PASS - 1 .. PASS + 1 and 2 PASS - 1 .. 2 PASS + 1: one block each
        for k in (PASS, 2 * PASS):
            d = np.diff(recs["pos"][k - 2:k + 3].astype(np.int64))
            assert d.tolist() == [gap + 3, 3, 3, gap + 3]
    for k in (PASS, 2 * PASS):
        assert fa[k - 1:k + 2].tolist() == [2, 2, 2] and fb[k - 1:k + 2].tolist() == [2, 2, 2]
    assert int(blocks[1]) > 128 and int(blocks[2]) > 64 and blocks[2] < blocks[1]          # more descriptors than two waves hold
    assert int(blocks[0]) == int(blocks[1]) < 3 * PASS + 1 - 4                             # (matched SN pairs are no candidates)


def test_random_rerepresentations():
    """200 random truth tables against calls made of them by re-representation: the library equals the twin on every one, and the
    set rescues and fails often enough to say something about both."""
    equal = unequal = 0
    for seed in bt.RANDOM_SEEDS:
        _, _, blocks, _, _ = check_host(seed)
        equal += int(blocks[2]) > 0
        unequal += int(blocks[1]) > int(blocks[2])
    n = len(bt.RANDOM_SEEDS)
    assert equal * 4 >= n and unequal * 4 >= n, (equal, unequal, n)


def test_refusals():
    bases, a, pa, b, pb, _, _ = CASES["mnp_vs_snps"]
    with pytest.raises(_ffi.MsimError, match="block gap") as e:
        _ffi.cmp_counts_blocks_host(bases, a, pa, b, pb, False, bt.MAX_SPAN + 1)
    assert e.value.code == _ffi.ERR_ARG
    _ffi.cmp_counts_blocks_host(bases, a, pa, b, pb, False, bt.MAX_SPAN)
    with pytest.raises(_ffi.MsimError, match="not sorted"):
        _ffi.cmp_counts_blocks_host(bases, a[::-1], pa, b, pb)
    none = a[:0]
    got = _ffi.cmp_counts_blocks_host(bases, none, tw.NO_POOL, none, tw.NO_POOL)
    assert not got[0].any() and not got[1].any() and not got[2].any() and len(got[3]) == len(got[4]) == 0
    with _ffi.Engine(-1) as eng:                           # a host-only context refuses the device calls
        with pytest.raises(_ffi.MsimError, match="needs the GPU"):
            eng.cmp_counts_blocks(0)
        assert eng.cmp_blocks_timing() == 0.0


# ------------------------------------------------------------------------------ 2. the file
def test_rendering_the_block_columns():
    counts = np.zeros((1, 8, _ffi.CMP_BINS, 6), dtype=np.uint64)
    counts[0, tw.SN, 0] = (90, 6, 4, 90, 10, 20)
    counts[0, tw.DE, 1] = (0, 2, 2, 0, 0, 0)
    counts[0, tw.IN, 1] = (0, 0, 0, 0, 1, 0)
    lines = compare.render(["a note"], counts, blocks=True).splitlines()
    assert lines[1].split("\t") == ["type", "length", "truth", "calls", "TP", "FN", "FP", "TP.calls", "BLK", "BLK.calls", "recall", "precision"]
    assert lines[1] == "\t".join(compare.HEADER_BLOCKS) and len(lines) == 1 + 17
    rows = {tuple(l.split("\t")[:2]): l.split("\t")[2:] for l in lines[2:]}
    assert rows[("SN", ".")] == ["100", "120", "96", "4", "20", "100", "6", "10", "0.960000", "0.833333"]
    assert rows[("DE", "2-5")] == ["4", "0", "2", "2", "0", "0", "2", "0", "0.500000", "NA"]
    assert rows[("IN", "2-5")] == ["0", "1", "0", "0", "0", "1", "0", "1", "NA", "1.000000"]
    assert rows[("ALL", ".")] == ["104", "121", "98", "6", "20", "101", "8", "11", "0.942308", "0.834711"]
    # six values without `blocks` are a diploid comparison's, as before
    assert compare.render([], counts).splitlines()[0] == "\t".join(compare.HEADER_DIPLOID)


def test_record_rows_name_the_side_of_a_block_match():
    bases, a, pa, b, pb, exact, gap = CASES["iv_vs_transitions"]
    _, _, _, fa, fb = check_host("iv_vs_transitions")
    assert compare.record_rows("FN", "c", a, fa) == [] and compare.record_rows("FP", "c", b, fb) == []
    assert compare.record_rows("BLK", "c", a, fa, 2, "truth") == ["BLK\tc\t5\tIV\t2\ttruth"]
    assert compare.record_rows("BLK", "c", b, fb, 2, "calls") == ["BLK\tc\t5\tSN\t1\tcalls", "BLK\tc\t6\tSN\t1\tcalls"]


# ------------------------------------------------------------------------------ 3. the command line
def test_compare_namespace():
    a = ap.get_args(["genome.fa", "compare", "t.vcf", "c.vcf"])
    assert (a.blocks, a.block_gap) == (False, None)
    a = ap.get_args(["genome.fa", "compare", "t.vcf", "c.vcf", "--blocks"])
    assert (a.blocks, a.block_gap) == (True, None) and ap.compare_refusal(a) is None
    a = ap.get_args(["genome.fa", "compare", "t.vcf", "c.vcf", "--blocks", "--block-gap", "0", "--exact", "--list"])
    assert (a.blocks, a.block_gap, a.exact, a.list_records) == (True, 0, True, True)
    for argv in (["genome.fa", "vcf", "x.vcf"], ["genome.fa", "profile", "x.vcf"], ["genome.fa", "args", "-sn", "0.1"]):
        other = ap.get_args(argv)
        assert not hasattr(other, "blocks") and not hasattr(other, "block_gap")


@pytest.mark.parametrize("argv,message", [
    (["genome.fa", "compare", "t.vcf", "c.vcf", "--block-gap", "10"], "--block-gap needs --blocks"),
    (["genome.fa", "compare", "t.vcf", "c.vcf", "--blocks", "--diploid"], "cannot be combined with --diploid"),
    (["genome.fa", "compare", "t.vcf", "c.vcf", "--blocks", "--block-gap", "4097"], "--block-gap must lie in 0..4096"),
    (["genome.fa", "compare", "t.vcf", "c.vcf", "--blocks", "--block-gap", "-1"], "--block-gap must lie in 0..4096"),
])
def test_usage_errors(argv, message):
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
        ap.get_args(argv)
    assert ei.value.code == 2 and "usage:" in err.getvalue() and message in err.getvalue()
