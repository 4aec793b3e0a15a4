"""``compare --blocks`` on the device: ``msim_cmp_counts_blocks`` (csrc/cmp_blocks.hip: ``k_blk_scan``, ``k_blk_replay``, behind
``k_cmp_match`` and in front of ``k_cmp_tally``) on the cases of ``blk_twin`` -- hand-built tables installed with ``set_records`` and
``cmp_hold`` --, held against the twin (the rule in Python, its replay ``apply_ref.apply``) and against the library's sequential
restatement; and the command line on an MNP line against two SNP lines.  All comparisons are exact integers and bytes.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import blk_twin as bt
import cmp_twin as tw
from mutation_simulator_amd import _ffi, compare
from test_gpu_spectrum import run_cli

pytestmark = pytest.mark.gpu

PASS = _ffi.CMP_PASS
CASES = bt.cases(PASS)
NAMES = ("counts", "tallies", "block tallies", "truth flags", "calls flags")


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def install(eng, case):
    """A fresh contig with the case's truth held and its calls current."""
    bases, a, pa, b, pb, _, _ = case
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, a, pa)
    eng.cmp_hold(cid)
    eng.set_records(cid, b, pb)
    return cid


def run_device(eng, case, cid=None):
    """The device's (counts, tallies, block tallies, truth flags, calls flags) of a case."""
    bases, a, pa, b, pb, exact, gap = case
    cid = install(eng, case) if cid is None else cid
    counts, tallies, blocks = eng.cmp_counts_blocks(cid, exact, gap)
    held, held_pool, fa, fb = eng.cmp_fetch(cid)
    assert held.tobytes() == np.ascontiguousarray(a).tobytes() and held_pool.tobytes() == np.ascontiguousarray(pa).tobytes()
    return counts, tallies, blocks, fa, fb


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, g.reshape(-1)[:16].tolist(), w.reshape(-1)[:16].tolist(),
                                      np.flatnonzero((g != w).reshape(-1))[:8].tolist())


def check(eng, name):
    case = bt.random_case(name) if isinstance(name, int) else CASES[name]
    got = run_device(eng, case)
    same(got, bt.expected(name, PASS), (name, "twin"))
    same(got, _ffi.cmp_counts_blocks_host(*case), (name, "host restatement"))
    counts, _, blocks, _, _ = got
    assert int(counts[..., :3].sum()) == len(case[1]) and int(counts[..., 3:].sum()) == len(case[3])
    assert int(blocks[0]) == int(blocks[1]) + int(blocks[3]) + int(blocks[4])
    return got


def totals(counts):
    s = [int(counts[..., k].sum()) for k in range(6)]
    return s[0] + s[1], s[1], s[2], s[3] + s[4], s[4], s[5]         # TP, BLK, FN, TP.calls, BLK.calls, FP


# ------------------------------------------------------------------------------ 1. the cases
@pytest.mark.parametrize("case", sorted(CASES))
def test_cases_equal_the_twin(eng, case):
    counts, _, blocks, fa, fb = check(eng, case)
    if case in ("mnp_vs_snps", "snps_vs_mnp"):
        assert totals(counts) == (2, 2, 0, 2, 2, 0) and blocks.tolist() == [1, 1, 1, 0, 0]
    if case == "iv_palindrome_vs_nothing":
        assert totals(counts) == (1, 1, 0, 0, 0, 0) and len(fb) == 0
    if case == "records_64":
        assert blocks.tolist() == [1, 1, 1, 0, 0] and int((fa == 2).sum()) == 3 and int((fb == 2).sum()) == 1
    if case == "records_65":
        assert blocks.tolist() == [1, 0, 0, 1, 0] and not (fa == 2).any() and not (fb == 2).any()
    if case == "span_4096":
        assert blocks.tolist() == [1, 1, 1, 0, 0]
    if case == "span_4097":
        assert blocks.tolist() == [1, 0, 0, 1, 0]
    if case == "tl_is_record_65":
        assert blocks.tolist() == [1, 0, 0, 0, 1]
    if case == "grid":
        for k in (PASS, 2 * PASS):                         # the blocks across the edge of a pass, on both sides
            assert fa[k - 1:k + 2].tolist() == [2, 2, 2] and fb[k - 1:k + 2].tolist() == [2, 2, 2]
        assert int(blocks[1]) > 128                        # more descriptors than two waves append
    eng.clear()


def test_flags_are_the_plain_calls_where_nothing_is_rescued(eng):
    """The pass only rescues: on the same tables ``cmp_counts`` and ``cmp_counts_blocks`` agree wherever a flag is not 2, and the
    plain call after the block call gives its own flags again (0 and 1)."""
    case = CASES["grid"]
    bases, a, pa, b, pb, exact, gap = case
    cid = install(eng, case)
    _, _, _, fa, fb = run_device(eng, case, cid)
    counts, tallies = eng.cmp_counts(cid, exact)
    _, _, pa_flags, pb_flags = eng.cmp_fetch(cid)
    assert set(np.unique(pa_flags)) <= {0, 1} and set(np.unique(pb_flags)) <= {0, 1}
    assert np.array_equal(np.where(fa == 2, 0, fa), pa_flags) and np.array_equal(np.where(fb == 2, 0, fb), pb_flags)
    want = tw.compare(bases, a, pa, b, pb, exact)
    assert np.array_equal(counts, want[0]) and np.array_equal(tallies, want[1])
    eng.clear()


def test_refusals_and_timing(eng):
    eng.clear()
    eng.reset_stats()
    assert eng.cmp_blocks_timing() == 0.0
    bases, a, pa, b, pb, _, _ = CASES["mnp_vs_snps"]
    cid = eng.add_contig(bases)
    with pytest.raises(_ffi.MsimError, match="contig has not been planned"):
        eng.cmp_counts_blocks(cid)
    eng.set_records(cid, a, pa)
    with pytest.raises(_ffi.MsimError, match="no held table"):
        eng.cmp_counts_blocks(cid)
    eng.cmp_hold(cid)
    eng.set_records(cid, b, pb)
    with pytest.raises(_ffi.MsimError, match="block gap") as e:
        eng.cmp_counts_blocks(cid, False, _ffi.CMP_BLOCK_SPAN + 1)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="call it first"):
        eng.cmp_fetch(cid)
    counts, _, blocks = eng.cmp_counts_blocks(cid, False, _ffi.CMP_BLOCK_SPAN)
    assert totals(counts) == (2, 2, 0, 2, 2, 0) and blocks.tolist() == [1, 1, 1, 0, 0]
    assert 0 < eng.cmp_blocks_timing() < 1000 and 0 < eng.cmp_timing() < 1000
    eng.reset_stats()
    assert eng.cmp_blocks_timing() == 0.0
    # two empty tables: zeros, nothing launched
    none = a[:0]
    eng.set_records(cid, none, tw.NO_POOL)
    eng.cmp_hold(cid)
    counts, tallies, blocks = eng.cmp_counts_blocks(cid)
    assert not counts.any() and not tallies.any() and not blocks.any() and eng.cmp_blocks_timing() == 0.0
    eng.clear()


# ------------------------------------------------------------------------------ 2. random re-representations
@pytest.mark.parametrize("first", range(0, 200, 50))
def test_random_rerepresentations(eng, first):
    for seed in range(first, first + 50):
        check(eng, seed)
    eng.clear()


# ------------------------------------------------------------------------------ 3. the command line
HEAD = "##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tcaller\n"
MNP = HEAD + "ctg\t5\t.\tAC\tGT\t.\tPASS\t.\tGT\t1\n"                                     # bases 4 and 5 of the contig: "AC"
SNPS = HEAD + "ctg\t5\t.\tA\tG\t.\tPASS\t.\tGT\t1\n" + "ctg\t6\t.\tC\tT\t.\tPASS\t.\tGT\t1\n"

NOTES = """# compare: calls snps.vcf against truth mnp.vcf on g.fa (1 contigs)
# truth: sample (first) haplotype 1
# calls: sample (first) haplotype 1
# matching: normalised (an indel matches any placement inside its repeat)
# truth indels whose placements end at a window edge: 0
# truth indels whose placements end at a base outside ACGT: 0
"""
# what the run without --blocks wrote before the option existed: written out here, not rendered by the code under test
PLAIN_ROWS = {("SN", "."): "0\t2\t0\t0\t2\tNA\t0.000000", ("IN", "2-5"): "1\t0\t0\t1\t0\t0.000000\tNA",
              ("DE", "2-5"): "1\t0\t0\t1\t0\t0.000000\tNA", ("ALL", "."): "2\t2\t0\t2\t2\t0.000000\t0.000000"}
ROW_KEYS = ([("SN", ".")] + [("IN", b) for b in ("1", "2-5", "6-20", "21-50", "51+")] + [("DE", b) for b in ("1", "2-5", "6-20", "21-50", "51+")] +
            [("DU", "."), ("IV", "."), ("TL", "."), ("TLI", "."), ("ALL", ".")])
PLAIN_TABLE = NOTES + "type\tlength\ttruth\tcalls\tTP\tFN\tFP\trecall\tprecision\n" + "".join(
    f"{t}\t{b}\t" + PLAIN_ROWS.get((t, b), "0\t0\t0\t0\t0\tNA\tNA") + "\n" for t, b in ROW_KEYS)
PLAIN_RECORDS = "FN\tctg\t5\tDE\t2\nFN\tctg\t7\tIN\t2\nFP\tctg\t5\tSN\t1\nFP\tctg\t6\tSN\t1\n"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("blocks")
    (d / "g.fa").write_text(">ctg\n" + "".join(bt.G[k:k + 60] + "\n" for k in range(0, len(bt.G), 60)))
    (d / "mnp.vcf").write_text(MNP)
    (d / "snps.vcf").write_text(SNPS)
    return d


def rows_of(path):
    lines = path.read_text().splitlines()
    body = [l.split("\t") for l in lines if not l.startswith("#")]
    return [l for l in lines if l.startswith("#")], body[0], {(r[0], r[1]): r[2:] for r in body[1:]}


def test_cli_without_blocks_writes_what_it_wrote(files, tmp_path):
    run_cli(["-o", tmp_path / "p", files / "g.fa", "compare", files / "mnp.vcf", files / "snps.vcf", "--list"])
    assert (tmp_path / "p_ms.compare.tsv").read_text() == PLAIN_TABLE                       # FN 2 (DE + IN), FP 2
    assert (tmp_path / "p_ms.compare.records.tsv").read_text() == PLAIN_RECORDS
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, "-o", tmp_path / "q", files / "g.fa", "compare", files / "mnp.vcf", files / "snps.vcf"])
    assert (tmp_path / "q_ms.compare.tsv").read_text() == PLAIN_TABLE and not (tmp_path / "q_ms.compare.records.tsv").exists()
    assert "cmp_block_kernel_ms" not in json.loads(stats.read_text())


def test_cli_blocks_rescues_the_mnp(files, tmp_path):
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, "-o", tmp_path / "b", files / "g.fa", "compare", files / "mnp.vcf", files / "snps.vcf", "--blocks",
             "--list"])
    notes, header, rows = rows_of(tmp_path / "b_ms.compare.tsv")
    assert header == list(compare.HEADER_BLOCKS)
    assert header == ["type", "length", "truth", "calls", "TP", "FN", "FP", "TP.calls", "BLK", "BLK.calls", "recall", "precision"]
    assert rows[("ALL", ".")] == ["2", "2", "2", "0", "0", "2", "2", "2", "1.000000", "1.000000"]          # BLK 2, BLK.calls 2, FN 0, FP 0
    assert rows[("SN", ".")] == ["0", "2", "0", "0", "0", "2", "0", "2", "NA", "1.000000"]
    assert rows[("DE", "2-5")] == rows[("IN", "2-5")] == ["1", "0", "1", "0", "0", "0", "1", "0", "1.000000", "NA"]
    assert notes[:6] == NOTES.splitlines()
    assert notes[6:] == ["# blocks: gap 50; 1 candidates, 1 replayed, 1 equal, 0 over a limit (64 records, 4096 bases), 0 holding a translocation"]
    assert (tmp_path / "b_ms.compare.records.tsv").read_text() == (
        "BLK\tctg\t5\tDE\t2\ttruth\nBLK\tctg\t7\tIN\t2\ttruth\nBLK\tctg\t5\tSN\t1\tcalls\nBLK\tctg\t6\tSN\t1\tcalls\n")
    bench = json.loads(stats.read_text())
    assert bench["cmp_block_kernel_ms"] > 0 and bench["cmp_kernel_ms"] > 0
    # the other way round, and a gap of 1: the insertion stands one base behind the deletion's footprint, still one block
    run_cli(["-o", tmp_path / "m", files / "g.fa", "compare", files / "snps.vcf", files / "mnp.vcf", "--blocks", "--block-gap", 1])
    notes, _, rows = rows_of(tmp_path / "m_ms.compare.tsv")
    assert rows[("ALL", ".")] == ["2", "2", "2", "0", "0", "2", "2", "2", "1.000000", "1.000000"]
    assert notes[6].startswith("# blocks: gap 1; 1 candidates, 1 replayed, 1 equal")
