"""``compare --regions / --stratify`` on the device: ``msim_cmp_regions_mark`` and ``msim_cmp_counts_regions`` (csrc/cmp_regions.hip:
``k_region_mark``, ``k_region_tally``) on the cases of ``region_twin`` -- hand-built tables installed with ``set_records``,
``cmp_hold`` and ``cmp_join`` --, held against the twin (the rule in Python, membership by a brute-force mask) and against the
library's sequential restatement; a stride case held against ``np.searchsorted``; the stale-state refusals; and the command line.
All comparisons are exact integers and bytes.
"""
from __future__ import annotations

import gzip
import json

import numpy as np
import pytest

import blk_twin as bt
import cmp_twin as tw
import dip_twin as dt
import region_twin as rt
from mutation_simulator_amd import _ffi, compare
from mutation_simulator_amd.vcf_replay import plan_all
from test_gpu_spectrum import data_lines, run_cli

pytestmark = pytest.mark.gpu

PASS = _ffi.CMP_PASS
CASES = rt.cases(PASS)
TRUTH, CALLS = _ffi.CMP_TRUTH, _ffi.CMP_CALLS


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def install(eng, case):
    """A fresh contig with the case's tables: the truth held and the calls current, or both sides' diploid tables joined."""
    eng.clear()
    cid = eng.add_contig(case["bases"])
    if case["kind"] == "diploid":
        for side, (h1, p1, h2, p2) in ((TRUTH, case["truth"]), (CALLS, case["calls"])):
            eng.set_records(cid, h1, p1)
            eng.cmp_hold(cid)
            eng.set_records(cid, h2, p2)
            eng.cmp_join(cid, side)
    else:
        eng.set_records(cid, *case["truth"])
        eng.cmp_hold(cid)
        eng.set_records(cid, *case["calls"])
    return cid


def count(eng, cid, case):
    """The count call of the case's kind: its counts."""
    if case["kind"] == "diploid":
        return eng.cmp_counts_diploid(cid, case["exact"])[0]
    if case["kind"] == "blocks":
        return eng.cmp_counts_blocks(cid, case["exact"], case["gap"])[0]
    return eng.cmp_counts(cid, case["exact"])[0]


def flags_of(eng, cid, case):
    if case["kind"] == "diploid":
        return eng.cmp_fetch_diploid(cid, TRUTH)[3], eng.cmp_fetch_diploid(cid, CALLS)[3]
    return eng.cmp_fetch(cid)[2:]


def equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, got.reshape(-1)[:16].tolist(), want.reshape(-1)[:16].tolist(),
                                       np.flatnonzero((got != want).reshape(-1))[:8].tolist())


# ------------------------------------------------------------------------------ 1. the cases
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_twin_and_the_host(eng, name):
    case = CASES[name]
    diploid = case["kind"] == "diploid"
    ma, mb, by_mask, plain, fa, fb = rt.expected(case)
    (a, pa, _), (b, pb, _) = rt.tables_of(case)
    cid = install(eng, case)
    equal(count(eng, cid, case), plain, (name, "the count call"))
    got_fa, got_fb = flags_of(eng, cid, case)
    equal(got_fa, fa, (name, "truth flags"))
    equal(got_fb, fb, (name, "calls flags"))
    for s, (starts, ends) in enumerate(case["sets"]):
        eng.cmp_regions_set(cid, s, starts, ends)
    eng.cmp_regions_mark(cid, case["exact"], diploid)
    got_ma, got_mb = eng.cmp_fetch_regions(cid, case["exact"], diploid)
    equal(got_ma, ma, (name, "truth marks"))
    equal(got_mb, mb, (name, "calls marks"))
    width = plain.shape[-1]
    for mask, (counts, outside) in by_mask.items():
        got = eng.cmp_counts_regions(cid, mask, case["exact"], diploid, width)
        host = _ffi.cmp_counts_regions_host(case["bases"], a, pa, fa, b, pb, fb, width // 2, case["sets"], mask, case["exact"])
        equal(got[0], counts, (name, mask, "counts against the twin"))
        equal(got[1], outside, (name, mask, "outside against the twin"))
        equal(got[0], host[0], (name, mask, "counts against the host restatement"))
        equal(got[1], host[1], (name, mask, "outside against the host restatement"))
        equal(got_ma, host[2], (name, mask, "truth marks against the host restatement"))
        equal(got_mb, host[3], (name, mask, "calls marks against the host restatement"))
        half = width // 2
        assert int(got[0][..., :half].sum()) + int(got[1][0]) == len(a) and int(got[0][..., half:].sum()) + int(got[1][1]) == len(b)
        if case["kind"] != "blocks":
            assert np.array_equal(got[0][..., 0], got[0][..., half])
    got = eng.cmp_counts_regions(cid, 0, case["exact"], diploid, width)
    equal(got[0], plain, (name, "mask 0"))
    assert got[1].tolist() == [0, 0]
    eng.clear()


# ------------------------------------------------------------------------------ 2. more passes than the grid has workgroups
def test_stride_case_equals_searchsorted(eng):
    n = 2048 * PASS + 300
    rs = np.random.RandomState(5)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, 2 * n + 2)]
    k = np.arange(n)
    truth = np.zeros(n, dtype=_ffi.RECORD_DTYPE)
    truth["pos"] = truth["stop"] = 2 * k
    truth["type"] = tw.SN
    truth["aux"] = k % 3
    calls = truth.copy()
    moved = k % 7 == 0                                     # every seventh call stands one base further: unmatched on both sides
    calls["pos"] = calls["stop"] = 2 * k + moved
    cuts = np.unique(rs.randint(0, 2 * n + 2, 4000))
    cuts = cuts[:len(cuts) // 2 * 2]
    sets = [(cuts[0::2].astype(np.uint32), cuts[1::2].astype(np.uint32)), rt.one((1000, 2 * n - 999))]
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, truth, tw.NO_POOL)
    eng.cmp_hold(cid)
    eng.set_records(cid, calls, tw.NO_POOL)
    counts, _ = eng.cmp_counts(cid)
    assert int(counts[tw.SN, 0, 0]) == n - int(moved.sum())
    for s, (starts, ends) in enumerate(sets):
        eng.cmp_regions_set(cid, s, starts, ends)
    eng.cmp_regions_mark(cid)

    def inside(pos, starts, ends):
        at = np.searchsorted(starts, pos, side="right") - 1
        return (at >= 0) & (pos < ends[np.maximum(at, 0)])
    want = [sum(inside(t["pos"], *sets[s]).astype(np.uint8) << s for s in range(2)) for t in (truth, calls)]
    got = eng.cmp_fetch_regions(cid)
    equal(got[0], want[0].astype(np.uint8), "truth marks")
    equal(got[1], want[1].astype(np.uint8), "calls marks")
    for mask in (1, 2, 3):
        counts, outside = eng.cmp_counts_regions(cid, mask)
        ia, ib = (want[0] & mask) == mask, (want[1] & mask) == mask
        row = [int((ia & ~moved).sum()), int((ia & moved).sum()), int((ib & ~moved).sum()), int((ib & moved).sum())]
        assert counts[tw.SN, 0].tolist() == row and int(counts.sum()) == sum(row), mask
        assert outside.tolist() == [n - int(ia.sum()), n - int(ib.sum())], mask
    eng.clear()


# ------------------------------------------------------------------------------ 3. refusals and timing
def test_stale_state_is_refused(eng):
    case = CASES["pair_across_edge"]
    sets = case["sets"]
    eng.clear()
    cid = eng.add_contig(case["bases"])
    L = len(case["bases"])
    for bad in (rt.one((5, 5)), rt.one((0, L + 1)), rt.one((0, 5), (5, 9)), rt.one((6, 9), (1, 3))):
        with pytest.raises(_ffi.MsimError, match="normal form") as e:
            eng.cmp_regions_set(cid, 0, *bad)
        assert e.value.code == _ffi.ERR_ARG
    for index in (-1, _ffi.CMP_REGION_SETS):
        with pytest.raises(_ffi.MsimError, match="set index") as e:
            eng.cmp_regions_set(cid, index, *sets[0])
        assert e.value.code == _ffi.ERR_ARG
    eng.cmp_regions_set(cid, 0, *sets[0])
    with pytest.raises(_ffi.MsimError, match="contig has not been planned"):   # no tables at all
        eng.cmp_regions_mark(cid)
    with pytest.raises(_ffi.MsimError, match="no diploid table of both sides"):
        eng.cmp_regions_mark(cid, diploid=True)
    eng.set_records(cid, *case["truth"])
    with pytest.raises(_ffi.MsimError, match="no held table"):
        eng.cmp_regions_mark(cid)
    eng.cmp_hold(cid)
    eng.set_records(cid, *case["calls"])
    eng.cmp_regions_mark(cid)
    with pytest.raises(_ffi.MsimError, match="call it first") as e:         # no count
        eng.cmp_counts_regions(cid, 1)
    assert e.value.code == _ffi.ERR_ARG
    eng.cmp_counts(cid)
    assert eng.cmp_counts_regions(cid, 1)[1].tolist() == [1, 1]
    with pytest.raises(_ffi.MsimError, match="not resident") as e:          # a mask bit without a set
        eng.cmp_counts_regions(cid, 3)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="MSIM_CMP_EXACT") as e:        # another exact bit than the count's and the mark's
        eng.cmp_counts_regions(cid, 1, exact=True)
    assert e.value.code == _ffi.ERR_ARG
    eng.cmp_counts(cid, True)                              # ... the count's exact bit follows, the mark's does not
    with pytest.raises(_ffi.MsimError, match="MSIM_CMP_EXACT"):
        eng.cmp_counts_regions(cid, 1, exact=True)
    with pytest.raises(_ffi.MsimError, match="MSIM_CMP_EXACT"):
        eng.cmp_counts_regions(cid, 1)
    eng.cmp_counts(cid)
    eng.cmp_regions_set(cid, 1, *sets[1])                  # a set changed after the mark
    with pytest.raises(_ffi.MsimError, match="cmp_regions_mark") as e:
        eng.cmp_counts_regions(cid, 1)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="cmp_regions_mark"):
        eng.cmp_fetch_regions(cid)
    eng.cmp_regions_mark(cid)
    assert eng.cmp_counts_regions(cid, 2)[1].tolist() == [0, 0]
    eng.cmp_regions_drop(cid, 1)                           # ... and a set dropped
    with pytest.raises(_ffi.MsimError, match="cmp_regions_mark"):
        eng.cmp_counts_regions(cid, 1)
    eng.cmp_regions_mark(cid)
    eng.set_records(cid, *case["calls"])                   # a new current table since the mark and the count
    with pytest.raises(_ffi.MsimError, match="call it first"):
        eng.cmp_counts_regions(cid, 1)
    eng.cmp_counts(cid)
    with pytest.raises(_ffi.MsimError, match="changed since"):
        eng.cmp_counts_regions(cid, 1)
    eng.cmp_regions_mark(cid)
    assert eng.cmp_counts_regions(cid, 1)[1].tolist() == [1, 1]
    eng.cmp_hold(cid)                                      # a new hold
    with pytest.raises(_ffi.MsimError) as e:
        eng.cmp_counts_regions(cid, 1)
    assert e.value.code == _ffi.ERR_ARG
    eng.cmp_release(cid)                                   # the sets go with the held tables
    eng.set_records(cid, *case["truth"])
    eng.cmp_hold(cid)
    eng.cmp_counts(cid)
    eng.cmp_regions_mark(cid)
    with pytest.raises(_ffi.MsimError, match="not resident"):
        eng.cmp_counts_regions(cid, 1)
    eng.clear()


def test_timing_and_empty_tables(eng):
    case = CASES["half_open"]
    eng.clear()
    eng.reset_stats()
    assert eng.cmp_regions_timing() == 0.0
    cid = eng.add_contig(case["bases"])
    none = case["truth"][0][:0]
    eng.set_records(cid, none, tw.NO_POOL)
    eng.cmp_hold(cid)
    eng.cmp_regions_set(cid, 0, *case["sets"][0])
    eng.cmp_regions_set(cid, 7, *rt.one())
    eng.cmp_counts(cid)
    eng.cmp_regions_mark(cid)                              # two empty tables: nothing launched
    counts, outside = eng.cmp_counts_regions(cid, 0b10000001)
    assert not counts.any() and outside.tolist() == [0, 0] and eng.cmp_regions_timing() == 0.0
    eng.set_records(cid, *case["calls"])
    eng.cmp_counts(cid)
    eng.cmp_regions_mark(cid)
    assert 0 < eng.cmp_regions_timing() < 1000
    assert eng.cmp_counts_regions(cid, 1)[1].tolist() == [0, 2] and eng.cmp_counts_regions(cid, 0b10000001)[1].tolist() == [0, 4]
    eng.reset_stats()
    assert eng.cmp_regions_timing() == 0.0
    eng.clear()


# ------------------------------------------------------------------------------ 4. the command line
NAMES = ("ctgA", "ctgB")
BPL = 60


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """Two small contigs of runs of A, C, G and T, a simulator run as the truth (haploid and diploid), the truth without every
    third line and another run as calls; a BED of whole contigs, one of the first half of each, one of the second."""
    d = tmp_path_factory.mktemp("regions")
    rs = np.random.RandomState(78)
    seqs = []
    for n_runs in (800, 500):
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, n_runs)]
        seqs.append(np.repeat(letters, rs.randint(1, 10, n_runs)))
    (d / "g.fa").write_bytes(b"".join(b">" + name.encode() + b"\n" + b"".join(s.tobytes()[k:k + BPL] + b"\n" for k in range(0, len(s), BPL))
                                      for name, s in zip(NAMES, seqs)))
    rates = ["args", "-sn", 0.01, "-in", 0.01, "-de", 0.01, "-inmax", 4, "-demax", 4]
    run_cli(["--seed", 11, "-o", d / "t", d / "g.fa", *rates])
    run_cli(["--seed", 12, "-o", d / "o", d / "g.fa", *rates])
    run_cli(["--seed", 13, "--ploidy", 2, "-o", d / "d", d / "g.fa", *rates])
    run_cli(["--seed", 14, "--ploidy", 2, "-o", d / "e", d / "g.fa", *rates])
    head, body = data_lines((d / "t_ms.vcf").read_bytes())
    lines = body.splitlines(keepends=True)
    (d / "sub.vcf").write_bytes(head + b"\n" + b"".join(l for k, l in enumerate(lines) if k % 3))
    halves = [len(s) // 2 for s in seqs]
    (d / "whole.bed").write_text("".join(f"{n}\t0\t{len(s)}\n" for n, s in zip(NAMES, seqs)))
    # scattered, unsorted, overlapping lines and a name the genome does not have: the first half of every contig
    (d / "first.bed").write_text("# first halves\n" + f"ctgB\t10\t{halves[1]}\nchrUn\t0\t99\nctgA\t100\t{halves[0]}\nctgB 0 40\nctgA\t0\t100\n")
    (d / "second.bed").write_text("".join(f"{n}\t{h}\t{len(s)}\n" for n, s, h in zip(NAMES, seqs, halves)))
    with gzip.open(d / "first.bed.gz", "wb") as f:
        f.write((d / "first.bed").read_bytes())
    return d, seqs, halves


def tables_of(seqs, vcf_path, haplotype=1):
    """The record tables the consensus parser makes of a VCF, per contig: [(records, pool)]."""
    e = _ffi.Engine(0)
    try:
        cids = [e.add_contig(s) for s in seqs]
        plan_all(e, np.fromfile(vcf_path, dtype=np.uint8), list(NAMES), cids, (None, haplotype))
        return [e.fetch_records(c) for c in cids]
    finally:
        e.close()


def blocks_of(path):
    """(comment lines, [the table blocks: lists of lines without the header]) of a compare table."""
    notes, blocks = [], []
    for line in path.read_text().splitlines():
        if line.startswith("#"):
            notes.append(line)
        elif line.startswith("type\t"):
            blocks.append([])
        else:
            blocks[-1].append(line)
    return notes, blocks


def twin_block(kind, seqs, truth, calls, sets_per_contig, mask, listed=None):
    """The rows (without the header) of the genome-wide block the twin gives, and its outside counts.  ``truth`` / ``calls``: per
    contig (records, pool) or (H1, pool, H2, pool); ``listed``: a list that gets, per contig, (truth records, flags, marks, calls
    records, flags, marks)."""
    total, outside = None, np.zeros(2, dtype=np.uint64)
    for g, t, c, sets in zip(seqs, truth, calls, sets_per_contig):
        case = {"kind": kind, "bases": g, "truth": t, "calls": c, "exact": False, "gap": bt.GAP, "sets": sets, "masks": [mask]}
        ma, mb, by_mask, _, fa, fb = rt.expected(case)
        total = by_mask[mask][0] if total is None else total + by_mask[mask][0]
        outside += by_mask[mask][1]
        if listed is not None:
            listed.append((rt.tables_of(case)[0][0], fa, ma, rt.tables_of(case)[1][0], fb, mb))
    return compare.render_block(total, kind == "blocks")[1:], outside.tolist()


def test_cli_regions_list_and_strata(genome, tmp_path):
    d, seqs, halves = genome
    truth, calls = d / "t_ms.vcf", d / "sub.vcf"
    cmp = lambda out, *extra: run_cli(["-o", tmp_path / out, d / "g.fa", "compare", truth, calls, *extra])    # noqa: E731
    cmp("plain", "--list")
    plain_notes, plain = blocks_of(tmp_path / "plain_ms.compare.tsv")
    # a BED of whole contigs: the rows of the run without it, nothing outside
    cmp("whole", "--regions", d / "whole.bed", "--per-contig")
    notes, blocks = blocks_of(tmp_path / "whole_ms.compare.tsv")
    assert blocks[0] == plain[0] and len(blocks) == 3
    n_bases = sum(len(s) for s in seqs)
    assert notes[:len(plain_notes)] == plain_notes
    assert notes[len(plain_notes)] == (f"# regions: whole.bed: 2 intervals, {n_bases} bases (0 lines on names the genome does not have); "
                                       "outside and not scored: 0 truth records, 0 calls records")
    # the first halves, listed; the strata partition the genome
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, "-o", tmp_path / "half", d / "g.fa", "compare", truth, calls, "--regions", d / "first.bed", "--list",
             "--stratify", f"first={d / 'first.bed'}", "--stratify", f"second={d / 'second.bed'}"])
    bench = json.loads(stats.read_text())
    assert bench["cmp_region_kernel_ms"] > 0 and bench["bed_scan_s"] >= 0
    notes, blocks = blocks_of(tmp_path / "half_ms.compare.tsv")
    ta, tb = tables_of(seqs, truth), tables_of(seqs, calls)
    first = [[rt.one((0, h))] for h in halves]
    listed = []
    want, outside = twin_block("haploid", seqs, ta, tb, first, 1, listed)
    assert blocks[0] == want and outside[0] > 20 and outside[1] > 20
    assert notes[len(plain_notes)] == (f"# regions: first.bed: 2 intervals, {sum(halves)} bases (1 lines on names the genome does not have); "
                                       f"outside and not scored: {outside[0]} truth records, {outside[1]} calls records")
    both = [[rt.one((0, h)), rt.one((h, len(s)))] for h, s in zip(halves, seqs)]
    assert blocks[1] == want                               # the stratum "first" inside --regions first.bed: the main table again
    empty, out_second = twin_block("haploid", seqs, ta, tb, both, 3)
    assert blocks[2] == empty and all(r.split("\t")[2:4] == ["0", "0"] for r in empty)
    assert notes[-2] == f"# stratum first: first.bed: 2 intervals, {sum(halves)} bases; outside: {outside[0]} truth, {outside[1]} calls"
    assert notes[-1] == (f"# stratum second: second.bed: 2 intervals, {n_bases - sum(halves)} bases; outside: {out_second[0]} truth, "
                         f"{out_second[1]} calls")
    # --list: the inside records only
    rows = []
    for name, (a, fa, ma, b, fb, mb) in zip(NAMES, listed):
        rows += compare.record_rows("FN", name, a[(ma & 1) != 0], fa[(ma & 1) != 0]) + compare.record_rows("FP", name, b[(mb & 1) != 0], fb[(mb & 1) != 0])
    got = (tmp_path / "half_ms.compare.records.tsv").read_text().splitlines()
    assert got == rows and 0 < len(got) < len((tmp_path / "plain_ms.compare.records.tsv").read_text().splitlines())
    # the .bed.gz gives the same file
    cmp("gz", "--regions", d / "first.bed.gz")
    assert (tmp_path / "gz_ms.compare.tsv").read_text().replace("first.bed.gz", "first.bed") == "\n".join(
        notes[:len(plain_notes) + 1] + ["\t".join(compare.HEADER)] + blocks[0]) + "\n"


def test_cli_two_strata_that_partition_the_genome_sum_to_the_main_table(genome, tmp_path):
    d, seqs, halves = genome
    run_cli(["-o", tmp_path / "s", d / "g.fa", "compare", d / "t_ms.vcf", d / "o_ms.vcf", "--stratify", f"a={d / 'first.bed'}",
             "--stratify", f"b={d / 'second.bed'}"])
    notes, blocks = blocks_of(tmp_path / "s_ms.compare.tsv")
    assert len(blocks) == 3 and not any(n.startswith("# regions:") for n in notes)
    for main, a, b in zip(*blocks):
        m, x, y = main.split("\t"), a.split("\t"), b.split("\t")
        assert m[:2] == x[:2] == y[:2] and [int(v) for v in m[2:7]] == [int(p) + int(q) for p, q in zip(x[2:7], y[2:7])]
    assert int(blocks[0][-1].split("\t")[2]) > 100 and int(blocks[1][-1].split("\t")[2]) > 30 and int(blocks[2][-1].split("\t")[2]) > 30
    ta, tb = tables_of(seqs, d / "t_ms.vcf"), tables_of(seqs, d / "o_ms.vcf")
    both = [[rt.one((0, h)), rt.one((h, len(s)))] for h, s in zip(halves, seqs)]
    assert blocks[1] == twin_block("haploid", seqs, ta, tb, both, 1)[0] and blocks[2] == twin_block("haploid", seqs, ta, tb, both, 2)[0]


def test_cli_diploid_and_blocks_with_regions(genome, tmp_path):
    d, seqs, halves = genome
    first = [[rt.one((0, h))] for h in halves]
    run_cli(["-o", tmp_path / "dip", d / "g.fa", "compare", d / "d_ms.vcf", d / "e_ms.vcf", "--diploid", "--regions", d / "first.bed"])
    sides = [[h1 + h2 for h1, h2 in zip(tables_of(seqs, d / f"{x}_ms.vcf", 1), tables_of(seqs, d / f"{x}_ms.vcf", 2))] for x in "de"]
    want, outside = twin_block("diploid", seqs, sides[0], sides[1], first, 1)
    notes, blocks = blocks_of(tmp_path / "dip_ms.compare.tsv")
    assert blocks == [want] and f"outside and not scored: {outside[0]} truth records, {outside[1]} calls records" in notes[-1]
    assert outside[0] > 20 and int(want[-1].split("\t")[2]) > 20
    run_cli(["-o", tmp_path / "blk", d / "g.fa", "compare", d / "t_ms.vcf", d / "sub.vcf", "--blocks", "--regions", d / "first.bed"])
    want, outside = twin_block("blocks", seqs, tables_of(seqs, d / "t_ms.vcf"), tables_of(seqs, d / "sub.vcf"), first, 1)
    notes, blocks = blocks_of(tmp_path / "blk_ms.compare.tsv")
    assert blocks == [want] and f"outside and not scored: {outside[0]} truth records, {outside[1]} calls records" in notes[-1]
    assert notes[-2].startswith("# blocks: gap 50;")


def test_cli_usage_errors(genome, tmp_path):
    d, _, _ = genome
    base = ["-o", tmp_path / "u", d / "g.fa", "compare", d / "d_ms.vcf", d / "d_ms.vcf"]
    err = run_cli(base + ["--diploid", "--phased", "--regions", d / "first.bed"], expect=2)
    assert "--phased" in err and "genome-wide" in err
    err = run_cli(base + ["--diploid", "--phased", "--stratify", f"a={d / 'first.bed'}"], expect=2)
    assert "--phased" in err
    for bad in ("=x.bed", "a b=x.bed", "a#=x.bed", "a\tb=x.bed", "noequals", "a="):
        assert "--stratify takes NAME=FILE" in run_cli(base + ["--stratify", bad], expect=2)
    err = run_cli(base + ["--stratify", f"a={d / 'first.bed'}", "--stratify", f"a={d / 'second.bed'}"], expect=2)
    assert "distinct" in err
    (tmp_path / "beyond.bed").write_text("ctgA\t0\t5\nctgB\t0\t999999\n")
    err = run_cli(base[:4] + [d / "t_ms.vcf", d / "t_ms.vcf", "--regions", tmp_path / "beyond.bed"], expect=1)
    assert "beyond.bed: BED line 2: end beyond the contig's last base" in err
    assert not list(tmp_path.glob("u_ms*"))


def test_cli_whole_contigs_and_no_options_write_the_existing_path(genome, tmp_path):
    """The run without --regions / --stratify against a file rendered by the code path that existed before them -- the twin's
    plain counts through ``compare.render`` --, and the run with a BED of whole contigs: the same file with one more comment."""
    d, seqs, _ = genome
    run_cli(["-o", tmp_path / "p", d / "g.fa", "compare", d / "t_ms.vcf", d / "sub.vcf", "--per-contig"])
    run_cli(["-o", tmp_path / "w", d / "g.fa", "compare", d / "t_ms.vcf", d / "sub.vcf", "--per-contig", "--regions", d / "whole.bed"])
    got = (tmp_path / "p_ms.compare.tsv").read_text()
    assert [l for l in (tmp_path / "w_ms.compare.tsv").read_text().splitlines(keepends=True) if not l.startswith("# regions:")] == \
        got.splitlines(keepends=True)
    ta, tb = tables_of(seqs, d / "t_ms.vcf"), tables_of(seqs, d / "sub.vcf")
    counts, tallies = [], np.zeros(2, dtype=np.uint64)
    for g, (a, pa), (b, pb) in zip(seqs, ta, tb):
        c, t, _, _ = tw.compare(g, a, pa, b, pb)
        counts.append(c)
        tallies += t
    notes = ["compare: calls sub.vcf against truth t_ms.vcf on g.fa (2 contigs)", "truth: sample (first) haplotype 1",
             "calls: sample (first) haplotype 1", "matching: normalised (an indel matches any placement inside its repeat)",
             f"truth indels whose placements end at a window edge: {int(tallies[0])}",
             f"truth indels whose placements end at a base outside ACGT: {int(tallies[1])}"]
    assert got == compare.render(notes, np.stack(counts), list(NAMES))
