"""``compare --diploid --phased`` on the device (csrc/cmp_phase.hip): ``msim_cmp_phase_counts`` (``k_phase_pairs``,
``k_phase_compact``, ``k_phase_reduce``, ``k_phase_tilescan``, ``k_phase_tally``) on hand-built diploid tables with words set by
``msim_cmp_phase_set``; ``msim_cmp_phase_mark`` / ``msim_cmp_phase_join`` (``k_cons_phase``, ``k_phase_join``) on VCF text; and the
command line.  Every result is held against ``phase_twin`` (the rules in Python) AND against the library's sequential restatement
(``_ffi.cmp_phase_host``); all comparisons are exact.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import cmp_twin as tw
import dip_twin as dt
import phase_twin as pt
from mutation_simulator_amd import _ffi, compare
from mutation_simulator_amd.vcf_replay import plan_all, plan_loaded
from test_gpu_compare import NAMES, args_run, genome  # noqa: F401  (genome: the module's fixture, shared)
from test_gpu_compare_diploid import haplotype_tables, join_side
from test_gpu_spectrum import data_lines, run_cli

pytestmark = pytest.mark.gpu

TILE, PASS = _ffi.CMP_PHASE_TILE, _ffi.CMP_PASS
CASES = pt.small_cases(TILE, PASS)
TRUTH, CALLS = _ffi.CMP_TRUTH, _ffi.CMP_CALLS
CONTIG = _ffi.PHASE_CONTIG


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def install(eng, case):
    """A fresh contig with both sides joined and their words set; (contig id, tables as ``phase_twin.tables_of`` gives them)."""
    bases, truth, calls, wa, wb, exact = case
    eng.clear()
    cid = eng.add_contig(bases)
    join_side(eng, cid, TRUTH, *truth)
    join_side(eng, cid, CALLS, *calls)
    eng.cmp_phase_set(cid, TRUTH, wa)
    eng.cmp_phase_set(cid, CALLS, wb)
    return cid, pt.tables_of(case)


def check(eng, case):
    """The device's counts, words and state bytes against the host restatement and the twin, and the diploid comparison's own
    counts and flag bytes before and behind the phase pass.  Returns (counts, state bytes)."""
    cid, (bases, (a, pa, ga, wa), (b, pb, gb, wb), exact) = install(eng, case)
    before = eng.cmp_counts_diploid(cid, exact)
    flags = [eng.cmp_fetch_diploid(cid, side) for side in (TRUTH, CALLS)]
    assert flags[0][0].tobytes() == a.tobytes() and flags[1][0].tobytes() == b.tobytes()          # (the twin's join is the device's)
    out = eng.cmp_phase_counts(cid, exact)
    words_a, state = eng.cmp_fetch_phase(cid, TRUTH)
    words_b, none = eng.cmp_fetch_phase(cid, CALLS, state=False)
    assert none is None and np.array_equal(words_a, wa) and np.array_equal(words_b, wb)
    for what, want in (("host restatement", _ffi.cmp_phase_host(bases, a, pa, ga, wa, b, pb, gb, wb, exact)),
                       ("twin", pt.tally(bases, a, pa, ga, wa, b, pb, gb, wb, exact))):
        assert out.dtype == want[0].dtype and out.tolist() == want[0].tolist(), (what, out.tolist(), want[0].tolist())
        assert state.dtype == want[1].dtype and np.array_equal(state, want[1]), (what, np.flatnonzero(state != want[1])[:8])
    # no side effects: the flag bytes are what they were, a second pass gives the same, the comparison's counts too
    for side, (_, _, _, fl) in zip((TRUTH, CALLS), flags):
        assert np.array_equal(eng.cmp_fetch_diploid(cid, side)[3], fl)
    assert eng.cmp_phase_counts(cid, exact).tolist() == out.tolist() and np.array_equal(eng.cmp_fetch_phase(cid, TRUTH)[1], state)
    after = eng.cmp_counts_diploid(cid, exact)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    return out, state


# ------------------------------------------------------------------------------ 1. the small shapes
@pytest.mark.parametrize("case", sorted(CASES))
def test_small_shapes(eng, case):
    out, state = check(eng, CASES[case])
    pairs, blocks, raw, switches, flips = (int(out[k]) for k in (2, 3, 6, 7, 8))
    if case == "no_pair":
        assert pairs == 0 and not state.any() and out[:2].tolist() == [2, 1]
    if case.startswith("run_of_"):
        r = int(case[-1])
        assert (raw, switches, flips, blocks) == (r, r % 2, r // 2, 1)
    if case == "all_swapped":
        assert out[2:].tolist() == [9, 1, 0, 8, 0, 0, 0, 0, 9]
    if case == "tile_edge_run_and_block":
        dense = np.flatnonzero(state)
        assert len(dense) == TILE + 5 and np.flatnonzero(state[dense] & 2).tolist() == [TILE - 2, TILE - 1, TILE, TILE + 1]
        assert (blocks, flips, switches) == (2, 2, 0)
    if case.startswith("run_ends_at_"):
        at = int(case.rsplit("_", 1)[1])
        assert (raw, flips, switches) == (at, at // 2, at % 2)
    if case.startswith("block_starts_at_"):
        assert blocks == 2 and int(out[10]) == pairs == int(case.rsplit("_", 1)[1]) + 4
    if case == "long_gap":
        assert (pairs, blocks, raw) == (2, 1, 1) and np.flatnonzero(state).tolist() == [0, 2 * TILE + 4]
    if case.startswith("records_"):
        assert pairs == int(case.split("_")[1]) == len(state) and blocks == 1
    if case == "shifted_indel":
        assert (pairs, raw, flips) == (4, 2, 1)
    eng.clear()


# ------------------------------------------------------------------------------ 2. the calls' lifetime and the refusals
HEAD = "##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\n"


def tiny_vcf(s, genotypes):
    """An SNP line every tenth base of ``s``, one per entry of ``genotypes`` (FORMAT, sample), as text bytes."""
    other = {b: [x for x in "ACGT" if x != b][0] for b in "ACGT"}
    lines = [f"c\t{10 * k + 5}\t.\t{s[10 * k + 4]}\t{other[s[10 * k + 4]]}\t.\tPASS\t.\t{fmt}\t{smp}\n" for k, (fmt, smp) in enumerate(genotypes)]
    return np.frombuffer((HEAD + "".join(lines)).encode(), dtype=np.uint8)


def refused(call, match):
    with pytest.raises(_ffi.MsimError, match=match) as e:
        call()
    assert e.value.code == _ffi.ERR_ARG


def test_lifetime_and_refusals(eng):
    eng.clear()
    eng.reset_stats()
    assert eng.cmp_phase_timing() == 0.0
    s = tw.RANDOM_200
    text = tiny_vcf(s, [("GT", "1|0"), ("GT:PS", "0|1:7"), ("GT", "1/1"), ("GT:PS", "1|0:x"), ("GT:PS", "1|1:7")])
    cid = eng.add_contig(tw.as_bases(s))
    empty = eng.add_contig(tw.as_bases(s))
    behind = "directly behind a consensus-grammar msim_vcf_plan_contig"
    refused(lambda: eng.cmp_phase_mark(cid, TRUTH, 1), behind)                   # nothing loaded
    bases, truth, calls, wa, wb, _ = CASES["two_pairs_one_block"]
    eng.set_records(cid, truth[0], truth[1])
    refused(lambda: eng.cmp_phase_mark(cid, TRUTH, 1), behind)                   # a table, but no plan from text
    marks = []
    plan_all(eng, text, ["c", "none"], [cid, empty], (None, 1), lambda c: marks.append((c, eng.cmp_phase_mark(c, TRUTH, 1).tolist())))
    # haplotype 1 holds lines 1, 3, 4 and 5: 1|0 phased, 1/1 not, the unreadable PS, 1|1 phased; the contig without lines: empty marks
    assert marks == [(cid, [2, 1, 1]), (empty, [0, 0, 0])]
    refused(lambda: eng.cmp_phase_mark(cid, TRUTH, 1), behind)                   # the last plan was another contig's
    eng.vcf_plan_contig(cid, 0)
    eng.set_records(cid, *eng.fetch_records(cid))
    refused(lambda: eng.cmp_phase_mark(cid, TRUTH, 1), behind)                   # the same records, but no longer the parser's table
    eng.vcf_plan_contig(cid, 0)
    for side in (2, -1):
        refused(lambda: eng.cmp_phase_mark(cid, side, 1), "unknown side")
    for hap in (0, 3):
        refused(lambda: eng.cmp_phase_mark(cid, TRUTH, hap), "unknown haplotype")
    assert eng.cmp_phase_mark(cid, TRUTH, 1).tolist() == [2, 1, 1]
    refused(lambda: eng.cmp_phase_join(cid, TRUTH), "no diploid table of that side")
    eng.cmp_hold(cid)
    eng.vcf_select(1, 0, 2)
    refused(lambda: eng.cmp_phase_mark(cid, TRUTH, 2), behind)                   # selected, not planned
    eng.vcf_plan_contig(cid, 0)
    eng.cmp_join(cid, TRUTH)
    refused(lambda: eng.cmp_phase_join(cid, TRUTH), "no marks of both haplotypes")
    assert eng.cmp_phase_mark(cid, TRUTH, 2).tolist() == [2, 1, 0]               # lines 2, 3 and 5
    eng.vcf_release()
    refused(lambda: eng.cmp_phase_mark(cid, TRUTH, 2), behind)                   # the text is gone
    eng.cmp_phase_join(cid, TRUTH)
    refused(lambda: eng.cmp_phase_join(cid, TRUTH), "no marks of both haplotypes")     # consumed
    refused(lambda: eng.cmp_phase_counts(cid), "no diploid table of both sides")
    # the calls: the same table by hand, words set
    text2 = tiny_vcf(s, [("GT", "1|0"), ("GT", "0|1"), ("GT", "1|1"), ("GT", "1|0"), ("GT", "1|1")])
    plan_all(eng, text2, ["c", "none"], [cid, empty], (None, 1))
    eng.cmp_hold(cid)
    plan_loaded(eng, text2, ["c", "none"], [cid, empty], (None, 2))
    eng.cmp_join(cid, CALLS)
    eng.vcf_release()
    refused(lambda: eng.cmp_phase_counts(cid), "behind msim_cmp_counts_diploid")
    eng.cmp_counts_diploid(cid)
    refused(lambda: eng.cmp_phase_counts(cid), "no phase words of both sides")
    refused(lambda: eng.cmp_fetch_phase(cid, CALLS, state=False), "no phase words of that side")
    refused(lambda: eng.cmp_phase_set(cid, CALLS, np.zeros(4, dtype=np.uint32)), "4 words for a diploid table of 5 records")
    refused(lambda: eng.cmp_phase_set(empty, CALLS, np.zeros(0, dtype=np.uint32)), "no diploid table of that side")
    eng.cmp_phase_set(cid, CALLS, np.full(5, CONTIG, dtype=np.uint32))
    refused(lambda: eng.cmp_phase_counts(cid, exact=True), "with the same flags")
    refused(lambda: eng.cmp_fetch_phase(cid, TRUTH), "call it first")
    words = eng.cmp_fetch_phase(cid, TRUTH, state=False)[0]
    assert words.tolist() == [CONTIG, 7, 0, 0, 7]                               # (1|0, 0|1 in set 7, 1/1, the unreadable PS, 1|1 in set 7)
    out = eng.cmp_phase_counts(cid)
    assert out.tolist() == [2, 3, 2, 2, 2, 0, 0, 0, 0, 0, 0] and eng.cmp_fetch_phase(cid, TRUTH)[1].tolist() == [1, 1, 0, 0, 0]
    with pytest.raises(_ffi.MsimError, match="the state bytes are the truth's"):
        eng.cmp_fetch_phase(cid, CALLS)
    assert 0 < eng.cmp_phase_timing() < 1000
    # a new join of a side consumes that side's words; msim_cmp_release and msim_clear everything
    eng.set_records(cid, truth[0], truth[1])
    eng.cmp_hold(cid)
    eng.cmp_join(cid, CALLS)
    eng.cmp_counts_diploid(cid)
    refused(lambda: eng.cmp_phase_counts(cid), "no phase words of both sides")
    assert eng.cmp_fetch_phase(cid, TRUTH, state=False)[0].tolist() == words.tolist()
    eng.cmp_release(cid)
    refused(lambda: eng.cmp_phase_counts(cid), "no diploid table of both sides")
    cid2, _ = install(eng, CASES["two_pairs_one_block"])
    eng.cmp_counts_diploid(cid2)
    assert eng.cmp_phase_counts(cid2)[2] == 2
    eng.clear()
    cid = eng.add_contig(bases)
    refused(lambda: eng.cmp_phase_counts(cid), "no diploid table of both sides")
    eng.reset_stats()
    assert eng.cmp_phase_timing() == 0.0
    eng.clear()


# ------------------------------------------------------------------------------ 3. through the text
def genotype_of(line: bytes):
    return line.split(b"\t")[9].split(b":")[0]


def twin_words(vcf: bytes, seqs, tables):
    """Per contig the words of the side's diploid table as the twin's parser gives them, and the side's (phased, unphased,
    unreadable) records over both haplotype tables.  The simulator's dialect: a line is one record, so haplotype h's k-th record
    is the k-th line of the contig whose h-th genotype entry names an allele."""
    lines = data_lines(vcf)[1].splitlines()
    tally = [0, 0, 0]
    out = []
    for name, (h1, p1, h2, p2) in zip(NAMES, tables):
        own = [l for l in lines if l.split(b"\t")[0] == name.encode()]
        by_pos = []
        for h, recs in ((0, h1), (1, h2)):
            words = [pt.phase_word(l, 10) for l in own if genotype_of(l).replace(b"/", b"|").split(b"|")[h] not in (b"0", b".")]
            assert len(words) == len(recs)
            for w, bad in words:
                tally[2 if bad else 0 if w else 1] += 1
            by_pos.append(dict(zip(recs["pos"].tolist(), (w for w, _ in words))))
        u, _, gt = dt.join(h1, p1, h2, p2)
        out.append(np.array([by_pos[0 if g & 1 else 1][int(p)] for p, g in zip(u["pos"], gt)], dtype=np.uint32))
    return out, tally


def rewritten(vcf: bytes, change) -> bytes:
    """The VCF with every data line's FORMAT and sample replaced by ``change(contig, line number within it, genotype)``."""
    out, k, last = [], 0, None
    for line in vcf.split(b"\n"):
        if line and not line.startswith(b"#"):
            f = line.split(b"\t")
            k = k + 1 if f[0] == last else 0
            last = f[0]
            f[8], f[9] = change(f[0].decode(), k, f[9])
            line = b"\t".join(f)
        out.append(line)
    return b"\n".join(out)


SWAP = {b"1|0": b"0|1", b"0|1": b"1|0", b"1|1": b"1|1"}


def test_text_and_cli(genome, tmp_path):  # noqa: F811
    d, seqs = genome
    fa = d / "g.fa"
    run_cli(args_run(d, tmp_path / "d", "--ploidy", "2"))
    truth = tmp_path / "d_ms.vcf"
    raw = truth.read_bytes()
    n_a = sum(1 for l in data_lines(raw)[1].splitlines() if l.startswith(b"ctgA\t"))
    assert n_a > 600

    def change(contig, k, g):
        """ctgA: three phase sets, both haplotypes swapped from line 200 on; ctgB: no PS, one het flipped; every 11th line unphased,
        one PS unreadable."""
        if contig == "ctgA":
            g = SWAP[g] if k >= 200 else g
            ps = b"x7" if k == 50 else str(1 + 1000 * (3 * k // n_a)).encode()
            return b"GT:DP:PS", (g.replace(b"|", b"/") if k % 11 == 0 else g) + b":30:" + ps
        if k == flip_at:
            g = SWAP[g]
        return b"GT", g.replace(b"|", b"/") if k % 11 == 5 else g
    b_lines = [l for l in data_lines(raw)[1].splitlines() if l.startswith(b"ctgB\t")]
    flip_at = next(k for k, l in enumerate(b_lines) if k > 40 and k % 11 != 5 and genotype_of(l) != b"1|1")
    calls = tmp_path / "calls.vcf"
    calls.write_bytes(rewritten(raw, change))

    # 1. msim_cmp_phase_mark + msim_cmp_phase_join give the words the twin's parser gives
    tables = {"truth": haplotype_tables(seqs, truth), "calls": haplotype_tables(seqs, calls)}
    want = {"truth": twin_words(raw, seqs, tables["truth"]), "calls": twin_words(calls.read_bytes(), seqs, tables["calls"])}
    assert want["truth"][1][1:] == [0, 0] and want["calls"][1][2] in (1, 2) and want["calls"][1][1] > 100
    e = _ffi.Engine(0)
    try:
        cids = [e.add_contig(s) for s in seqs]
        for side, path, key in ((TRUTH, truth, "truth"), (CALLS, calls, "calls")):
            tally = np.zeros(3, dtype=np.uint64)

            def mark(haplotype):
                def hook(cid):
                    tally[:] += e.cmp_phase_mark(cid, side, haplotype)
                return hook
            text = np.fromfile(path, dtype=np.uint8)
            plan_all(e, text, list(NAMES), cids, (None, 1), mark(1))
            for c in cids:
                e.cmp_hold(c)
            plan_loaded(e, text, list(NAMES), cids, (None, 2), mark(2))
            for c in cids:
                e.cmp_join(c, side)
                e.cmp_phase_join(c, side)
            assert tally.tolist() == want[key][1], key
            e.vcf_release()
        for side, key in ((TRUTH, "truth"), (CALLS, "calls")):
            for c, words in zip(cids, want[key][0]):
                assert np.array_equal(e.cmp_fetch_phase(c, side, state=False)[0], words), (key, c)
        outs, states, listed, plain = [], [], [], []
        for name, c, g, t, k in zip(NAMES, cids, seqs, tables["truth"], tables["calls"]):
            counts = e.cmp_counts_diploid(c)
            a, pa, ga, fl_a = e.cmp_fetch_diploid(c, TRUTH)
            b, pb, gb, fl_b = e.cmp_fetch_diploid(c, CALLS)
            out = e.cmp_phase_counts(c)
            wa, state = e.cmp_fetch_phase(c, TRUTH)
            wb = e.cmp_fetch_phase(c, CALLS, state=False)[0]
            host, twin = _ffi.cmp_phase_host(g, a, pa, ga, wa, b, pb, gb, wb), pt.tally(g, a, pa, ga, wa, b, pb, gb, wb)
            assert out.tolist() == host[0].tolist() == twin[0].tolist() and np.array_equal(state, host[1]) and np.array_equal(state, twin[1])
            outs.append(out)
            plain.append((counts, compare.record_rows_diploid(name, a, ga, fl_a, b, gb, fl_b)))
            listed.append(pt.switch_lines(name, a, ga, state))
    finally:
        e.close()
    # ctgA: one switch at line 200, and a block boundary wherever the calls' set changes; ctgB: one flip
    assert int(outs[0][3]) == 3 and (int(outs[0][7]), int(outs[0][8])) == (1, 0) and int(outs[0][9]) > 0
    assert int(outs[1][3]) == 1 and (int(outs[1][6]), int(outs[1][7]), int(outs[1][8]), int(outs[1][9])) == (2, 0, 1, 1)

    # 2. the command line: the phase table, the SW lines, the note, the time
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, "-o", tmp_path / "p", fa, "compare", truth, calls, "--diploid", "--phased", "--list", "--per-contig"])
    text = (tmp_path / "p_ms.compare.phase.tsv").read_text()
    notes = [l for l in text.splitlines() if l.startswith("#")]
    assert "".join(l + "\n" for l in text.splitlines() if not l.startswith("#")) == pt.table_text(outs, NAMES)
    t_tally, c_tally = want["truth"][1], want["calls"][1]
    assert notes[0] == "# compare --phased: calls calls.vcf against truth d_ms.vcf on g.fa (2 contigs)"
    assert notes[1] == f"# truth: sample (first); records of both haplotype tables: {t_tally[0]} phased, 0 unphased, 0 with an unreadable PS"
    assert notes[2] == (f"# calls: sample (first); records of both haplotype tables: {c_tally[0]} phased, {c_tally[1]} unphased, "
                        f"{c_tally[2]} with an unreadable PS")
    records = (tmp_path / "p_ms.compare.records.tsv").read_text().splitlines()
    assert [l for l in records if l.startswith("SW\t")] == listed[0] + listed[1] and len(listed[0]) == 1 and len(listed[1]) == 2
    total = np.sum(outs, axis=0)
    table = (tmp_path / "p_ms.compare.tsv").read_text().splitlines()
    assert table[4] == f"# phasing: {int(total[2])} pairs in {int(total[3])} blocks, {int(total[6])} raw switches (see p_ms.compare.phase.tsv)"
    assert json.loads(stats.read_text())["cmp_phase_kernel_ms"] > 0
    run_cli(["-o", tmp_path / "q", fa, "compare", truth, calls, "--diploid", "--phased"])
    assert (tmp_path / "q_ms.compare.phase.tsv").read_text().splitlines()[len(notes):] == pt.table_text(outs).splitlines()

    # 3. without --phased every file is what the existing code path writes, and no phase table
    run_cli(["--bench-json", stats, "-o", tmp_path / "u", fa, "compare", truth, calls, "--diploid", "--list", "--per-contig"])
    assert sorted(p.name for p in tmp_path.glob("u_ms*")) == ["u_ms.compare.records.tsv", "u_ms.compare.tsv"]
    assert "cmp_phase_kernel_ms" not in json.loads(stats.read_text())
    tallies = sum(t for (_, t), _ in plain)
    plain_notes = ["compare: calls calls.vcf against truth d_ms.vcf on g.fa (2 contigs)", "truth: sample (first) both haplotypes",
                   "calls: sample (first) both haplotypes", "genotypes: diploid, unphased (dosage compared; a haploid 1 counts as 1/1)",
                   "matching: normalised (an indel matches any placement inside its repeat)",
                   f"truth indels whose placements end at a window edge: {int(tallies[0])}",
                   f"truth indels whose placements end at a base outside ACGT: {int(tallies[1])}"]
    assert (tmp_path / "u_ms.compare.tsv").read_text() == compare.render(plain_notes, np.stack([c for (c, _), _ in plain]), list(NAMES))
    assert (tmp_path / "u_ms.compare.records.tsv").read_text() == "".join(r + "\n" for _, rows in plain for r in rows)
    assert (tmp_path / "u_ms.compare.tsv").read_text().splitlines() == table[:4] + table[5:]
    per_contig = []                                        # the records file of the phased run: each contig's rows, then its SW lines
    for (_, rows), sw in zip(plain, listed):
        per_contig += rows + sw
    assert records == per_contig
