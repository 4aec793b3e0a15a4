"""The ``compare`` mode on the device: ``msim_cmp_hold`` / ``msim_cmp_counts`` / ``msim_cmp_fetch`` (csrc/compare.hip:
``k_cmp_match``, ``k_cmp_tally``) on hand-built and planned record tables, and the command line.  Every case is held against
``cmp_twin`` (the rules in Python) AND against the library's sequential restatement (``_ffi.cmp_counts_host``); all comparisons
are exact integers.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import apply_ref
import cmp_twin as tw
from mutation_simulator_amd import _ffi, compare
from mutation_simulator_amd.vcf_replay import plan_all
from test_gpu_sampler import _params, _sv_range
from test_gpu_spectrum import data_lines, run_cli

pytestmark = pytest.mark.gpu

PASS = _ffi.CMP_PASS
CASES = tw.small_cases(PASS)
KEY = 0xC0DE_C0FFEE


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def same(got, want, what):
    for name, g, w in zip(("counts", "tallies", "truth flags", "calls flags"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(-1))[:8])


def install(eng, bases, a, pa, b, pb):
    """A fresh contig with ``a`` held (the truth) and ``b`` current (the calls)."""
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, a, pa)
    eng.cmp_hold(cid)
    eng.set_records(cid, b, pb)
    return cid


def check(eng, cid, bases, a, pa, b, pb, exact=False, twin=None):
    """The device's counts, tallies and flags of contig ``cid`` against the twin and the host restatement."""
    counts, tallies = eng.cmp_counts(cid, exact)
    held, held_pool, fa, fb = eng.cmp_fetch(cid)
    assert held.tobytes() == np.ascontiguousarray(a).tobytes() and held_pool.tobytes() == np.ascontiguousarray(pa).tobytes()
    got = (counts, tallies, fa, fb)
    same(got, twin if twin is not None else tw.compare(bases, a, pa, b, pb, exact), "twin")
    same(got, _ffi.cmp_counts_host(bases, a, pa, b, pb, exact), "host restatement")
    assert np.array_equal(counts[..., 0], counts[..., 2])                      # truth matched == calls matched, every cell
    assert int(counts[..., :2].sum()) == len(a) and int(counts[..., 2:].sum()) == len(b)
    return got


def totals(counts):
    return int(counts[..., 0].sum()), int(counts[..., 1].sum()), int(counts[..., 3].sum())      # TP, FN, FP


# ------------------------------------------------------------------------------ 1. the small shapes
@pytest.mark.parametrize("case", sorted(CASES))
def test_small_shapes(eng, case):
    bases, a, pa, b, pb, exact = CASES[case]
    cid = install(eng, bases, a, pa, b, pb)
    counts, tallies, fa, fb = check(eng, cid, bases, a, pa, b, pb, exact)
    if case.startswith("identical"):
        assert totals(counts) == (len(a), 0, 0) and fa.all() and fb.all()
    if case == "disjoint":
        assert totals(counts) == (0, len(a), len(b))
    if case in ("homopolymer_ends", "repeat_rotated", "repeat_negative_shift", "repeat3_shift_2", "repeat3_shift_4", "end_pos0",
                "end_last_base", "end_ins_last_base", "window_same_side"):
        assert totals(counts) == (1, 0, 0)
    if case in ("homopolymer_ends_exact", "homopolymer_lengths", "repeat_rotated_exact", "repeat_other_bytes",
                "repeat3_wrong_rotation", "stop_N", "stop_N_ins", "window_edge", "window_edge_ins"):
        assert totals(counts) == (0, 1, 1)
    if case.startswith("stop_"):
        assert tallies.tolist() == [0, 1]
    if case.startswith("window_"):
        assert tallies.tolist() == [1, 0]
    if case.startswith("rank_3v2"):
        assert int(counts[tw.DE if "ins" not in case else tw.IN, 0 if "ins" not in case else 1, 0]) == 2
    # the other way round: the truth and the calls change places, matched stays matched
    cid = install(eng, bases, b, pb, a, pa)
    swapped = check(eng, cid, bases, b, pb, a, pa, exact)[0]
    assert np.array_equal(swapped[..., 0], counts[..., 0]) and np.array_equal(swapped[..., 1], counts[..., 3])
    eng.clear()


def test_rank_classes_straddle_a_pass(eng):
    for side, k in (("truth", 1), ("calls", 3)):
        recs = CASES[f"rank_3v2_{side}_at_pass"][k]
        assert recs["type"][PASS - 1:].tolist() == [tw.DE] * (3 if side == "truth" else 2)     # indices PASS - 1, PASS, ...
        assert (recs["type"][:PASS - 1] == tw.SN).all()


# ------------------------------------------------------------------------------ 2. the calls' lifetime and the refusals
def test_empty_tables_and_refusals(eng):
    eng.clear()
    eng.reset_stats()
    assert eng.cmp_timing() == 0.0
    bases, a, pa, b, pb, _ = CASES["identical"]
    none = a[:0]
    cid = eng.add_contig(bases)
    with pytest.raises(_ffi.MsimError, match="contig has not been planned") as e:
        eng.cmp_hold(cid)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="contig has not been planned") as e:
        eng.cmp_counts(cid)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="no such contig"):
        eng.cmp_counts(cid + 1)
    eng.set_records(cid, a, pa)
    with pytest.raises(_ffi.MsimError, match="no held table") as e:
        eng.cmp_counts(cid)
    assert e.value.code == _ffi.ERR_ARG
    # two empty tables: zeros, nothing launched
    eng.set_records(cid, none, tw.NO_POOL)
    eng.cmp_hold(cid)
    counts, tallies = eng.cmp_counts(cid)
    assert not counts.any() and not tallies.any() and eng.cmp_timing() == 0.0
    assert [len(x) for x in eng.cmp_fetch(cid)] == [0, 0, 0, 0]
    # the held table survives a new plan and a release of the contig; a released contig is unplanned
    eng.set_records(cid, a, pa)
    eng.cmp_hold(cid)
    with pytest.raises(_ffi.MsimError, match="call it first"):
        eng.cmp_fetch(cid)                                 # (no counts since the hold)
    eng.set_records(cid, b, pb)
    check(eng, cid, bases, a, pa, b, pb)
    assert 0 < eng.cmp_timing() < 1000
    eng.release_result(cid)
    with pytest.raises(_ffi.MsimError, match="contig has not been planned") as e:
        eng.cmp_counts(cid)
    assert e.value.code == _ffi.ERR_ARG
    eng.set_records(cid, none, tw.NO_POOL)
    assert totals(check(eng, cid, bases, a, pa, none, tw.NO_POOL)[0]) == (0, len(a), 0)
    assert eng.cmp_fetch(cid, flags=False)[0].tobytes() == a.tobytes()
    # ... and goes with msim_cmp_release and with msim_clear
    eng.cmp_release(cid)
    with pytest.raises(_ffi.MsimError, match="no held table"):
        eng.cmp_counts(cid)
    eng.cmp_hold(cid)
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, a, pa)
    with pytest.raises(_ffi.MsimError, match="no held table"):
        eng.cmp_counts(cid)
    eng.reset_stats()
    assert eng.cmp_timing() == 0.0
    eng.clear()


def test_held_table_is_the_selected_haplotypes(eng):
    bases, a, pa, _, _, _ = CASES["bin_edges"]
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, a, pa)
    gt = (np.arange(len(a)) % 3 + 1).astype(np.uint8)
    eng.set_genotypes(cid, gt)
    eng.select_haplotype(cid, 2)
    eng.cmp_hold(cid)
    eng.select_haplotype(cid, 1)
    h1, h2 = a[(gt & 1) != 0], a[(gt & 2) != 0]
    counts = check(eng, cid, bases, h2, pa, h1, pa)[0]
    assert totals(counts) == (int((gt == 3).sum()), int((gt == 2).sum()), int((gt == 1).sum()))
    eng.clear()


# ------------------------------------------------------------------------------ 3. a planned table, shifted
BIG_N = (1 << 17) + 1


@pytest.fixture(scope="module")
def big():
    """2^17 + 1 records of an SV mix the counter-based engine planned on runs of A and C, and the calls made of them: every indel
    at a random placement of its interval, every tenth record dropped, the dropped SNPs back with another base (foreign)."""
    rs = np.random.RandomState(23)
    runs = rs.randint(1, 7, 1_200_000)
    bases = np.repeat(np.frombuffer(b"AC", dtype=np.uint8)[np.arange(len(runs)) & 1], runs)
    L = len(bases)
    e = _ffi.Engine(0, _ffi.RNG_FAST)
    try:
        e.set_params(_params(titv=2.0))
        e.set_fast_key(KEY)
        cid = e.add_contig(bases)
        e.plan_contig(cid, [_sv_range(0, L - 1, BIG_N + 6000, {1: 0.4, 2: 0.25, 3: 0.25, 4: 0.05, 5: 0.05},
                                      {2: (1, 7), 3: (1, 7), 4: (2, 6), 5: (2, 6)})])
        a, pa = e.fetch_records(cid)
    finally:
        e.close()
    assert len(a) >= BIG_N
    a = a[:BIG_N].copy()
    keep = np.arange(BIG_N) % 10 != 3
    calls = tw.shifted(bases, a, pa, lambda ok: ok[int(rs.randint(0, len(ok)))], keep=keep)
    foreign = a[~keep & (a["type"] == tw.SN)]
    for r in foreign:
        calls.sn(int(r["pos"]), (int(r["aux"]) + 1) % 3)
    b, pb = calls.build()
    return bases, a, pa, b, pb, keep, len(foreign)


def test_shifted_table_of_2_17_plus_1_records(eng, big):
    bases, a, pa, b, pb, keep, n_foreign = big
    assert len(a) == BIG_N and len(b) == int(keep.sum()) + n_foreign and n_foreign > 1000
    indel = (a["type"] == tw.IN) | (a["type"] == tw.DE)
    kept = a[keep]
    moved = int((kept["pos"][indel[keep]] != b["pos"][np.isin(b["type"], (tw.IN, tw.DE))]).sum())
    assert int(indel.sum()) > 50_000 and moved > 10_000                        # shifts are the rule
    cid = install(eng, bases, a, pa, b, pb)
    counts, tallies, fa, fb = check(eng, cid, bases, a, pa, b, pb)
    # the construction: what was kept is found, wherever it stands; what was dropped is missed; the foreign records are extra
    assert totals(counts) == (int(keep.sum()), BIG_N - int(keep.sum()), n_foreign)
    assert int(fa.sum()) == int(fb.sum()) == int(keep.sum())                   # (inside a class the FIRST records match: the rank rule)
    for t in range(1, 8):
        assert int(counts[t, :, 1].sum()) == int((a["type"][~keep] == t).sum())
    assert int(counts[tw.SN, 0, 3]) == n_foreign and not tallies.any()
    # the literal comparison loses a moved indel twice: once as missed, once as extra
    tp, fn, fp = totals(check(eng, cid, bases, a, pa, b, pb, exact=True)[0])
    lost = int(keep.sum()) - tp
    assert moved // 2 < lost <= moved and (fn, fp) == (BIG_N - int(keep.sum()) + lost, n_foreign + lost)
    eng.clear()


# ------------------------------------------------------------------------------ 3b. more passes than the grid has workgroups
GRID = 2048                  # csrc/compare.hip: CMP_MAX_BLOCKS -- beyond that many passes a workgroup takes more than one


@pytest.mark.parametrize("n", [GRID * PASS, GRID * PASS + 1], ids=["grid_full", "grid_strides"])
def test_sn_table_at_and_past_the_grid_cap(eng, n):
    """An SN record on every base of a contig of ``n`` bases, and the calls: the same table with every 1000th record's
    alternative base changed.  At ``GRID * PASS`` records every workgroup takes one pass; with one record more the grid
    strides, workgroup 0 takes two, and the slot of the result a workgroup adds to follows its number, not its pass.  Held
    against the host restatement (linear in SN records) and the closed form: 524 changed records, each missed once and extra
    once."""
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(5).randint(0, 4, n)]
    a = np.zeros(n, dtype=_ffi.RECORD_DTYPE)
    a["pos"] = a["stop"] = np.arange(n, dtype=np.uint32)
    a["type"] = tw.SN
    a["aux"] = np.arange(n) % 3
    changed = np.arange(999, n, 1000)
    assert len(changed) == 524
    b = a.copy()
    b["aux"][changed] = (b["aux"][changed] + 1) % 3
    cid = install(eng, bases, a, tw.NO_POOL, b, tw.NO_POOL)
    counts, tallies = eng.cmp_counts(cid)
    held, _, fa, fb = eng.cmp_fetch(cid)
    assert held.tobytes() == a.tobytes()
    same((counts, tallies, fa, fb), _ffi.cmp_counts_host(bases, a, tw.NO_POOL, b, tw.NO_POOL), "host restatement")
    assert counts[tw.SN, 0].tolist() == [n - 524, 524, n - 524, 524] and int(counts.sum()) == 2 * n and not tallies.any()
    want = np.ones(n, dtype=np.uint8)
    want[changed] = 0
    assert np.array_equal(fa, want) and np.array_equal(fb, want)
    eng.clear()


# ------------------------------------------------------------------------------ 4. the command line
NAMES = ("ctgA", "ctgB")
BPL = 60


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """Two contigs of runs of A, C, G and T, 1 to 9 bases a run: most indels stand inside a repeat."""
    d = tmp_path_factory.mktemp("compare")
    rs = np.random.RandomState(77)
    seqs = []
    for n_runs in (9000, 5000):
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, n_runs)]
        seqs.append(np.repeat(letters, rs.randint(1, 10, n_runs)))
    out = []
    for name, seq in zip(NAMES, seqs):
        raw = seq.tobytes()
        out.append(b">" + name.encode() + b"\n" + b"".join(raw[k:k + BPL] + b"\n" for k in range(0, len(raw), BPL)))
    (d / "g.fa").write_bytes(b"".join(out))
    return d, seqs


def args_run(d, out, *extra):
    return ["--seed", 11, *extra, "-o", out, d / "g.fa", "args", "-sn", 0.01, "-in", 0.01, "-de", 0.01, "-inmax", 4, "-demax", 4]


def tables_of(seqs, vcf_path, haplotype=1):
    """The record tables the consensus parser makes of a VCF, per contig: [(records, pool)]."""
    e = _ffi.Engine(0)
    try:
        cids = [e.add_contig(s) for s in seqs]
        plan_all(e, np.fromfile(vcf_path, dtype=np.uint8), list(NAMES), cids, (None, haplotype))
        return [e.fetch_records(c) for c in cids]
    finally:
        e.close()


ALT_OF = {(ref, aux): (chr(apply_ref.TRANSITIONS[ord(ref)]) if aux == 0 else apply_ref.TRANSVERSIONS[ref][aux - 1])
          for ref in "ACGT" for aux in range(3)}


def vcf_text(seqs, tables) -> bytes:
    """A plain VCF of the tables: one line a record, the anchor base in front (behind, at a contig's first base)."""
    lines = [b"##fileformat=VCFv4.3", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tcaller"]
    for name, g, (recs, pool) in zip(NAMES, seqs, tables):
        s = g.tobytes().decode()
        for r in recs:
            p, q, typ = int(r["pos"]), int(r["stop"]), int(r["type"])
            if typ == tw.SN:
                pos, ref, alt = p + 1, s[p], ALT_OF[s[p], int(r["aux"])]
            elif typ == tw.DE:
                pos, ref, alt = (p, s[p - 1:q + 1], s[p - 1]) if p else (1, s[:q + 2], s[q + 1])
            else:
                ins = tw.insert_of(r, pool).decode()
                pos, ref, alt = (p, s[p - 1], s[p - 1] + ins) if p else (1, s[0], ins + s[0])
            lines.append(f"{name}\t{pos}\t.\t{ref}\t{alt}\t.\tPASS\t.\tGT\t1".encode())
    return b"\n".join(lines) + b"\n"


def table_rows(path):
    """(comment lines, {(type, length): [truth, calls, TP, FN, FP, recall, precision]} of the genome-wide block)."""
    lines = path.read_text().splitlines()
    notes = [l for l in lines if l.startswith("#")]
    body = [l.split("\t") for l in lines if not l.startswith("#")]
    assert body[0] == list(compare.HEADER)
    return notes, {(r[0], r[1]): r[2:] for r in body[1:1 + len(compare.ROWS) + 1]}


def all_ones(rows):
    assert all(r[5] in ("1.000000", "NA") and r[6] in ("1.000000", "NA") and r[3] == r[4] == "0" for r in rows.values()), rows
    for key in (("SN", "."), ("IN", "1"), ("IN", "2-5"), ("DE", "1"), ("DE", "2-5"), ("ALL", ".")):
        assert rows[key][5] == rows[key][6] == "1.000000" and int(rows[key][0]) > 20, key


def test_cli_a_run_against_itself_and_left_aligned(genome, tmp_path):
    d, seqs = genome
    run_cli(args_run(d, tmp_path / "o"))
    run_cli(args_run(d, tmp_path / "z", "--bgzip"))
    truth = tmp_path / "o_ms.vcf"
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, "-o", tmp_path / "self", d / "g.fa", "compare", truth, tmp_path / "z_ms.vcf.gz", "--list"])
    assert sorted(p.name for p in tmp_path.glob("self*")) == ["self_ms.compare.records.tsv", "self_ms.compare.tsv"]
    notes, rows = table_rows(tmp_path / "self_ms.compare.tsv")
    all_ones(rows)
    n_lines = len(data_lines(truth.read_bytes())[1].splitlines())
    assert int(rows[("ALL", ".")][0]) == int(rows[("ALL", ".")][1]) == n_lines
    assert (tmp_path / "self_ms.compare.records.tsv").read_text() == ""
    assert notes[0] == "# compare: calls z_ms.vcf.gz against truth o_ms.vcf on g.fa (2 contigs)"
    assert "# matching: normalised (an indel matches any placement inside its repeat)" in notes
    bench = json.loads(stats.read_text())
    assert bench["truth_vcf_bytes"] == truth.stat().st_size == bench["calls_vcf_bytes"] and bench["cmp_kernel_ms"] > 0
    assert bench["vcf_load_kernel_ms"] > 0 and bench["vcf_plan_kernel_ms"] > 0 and set(bench["cli_s"]) == {"load_index", "compare"}

    # the same variants as a caller reports them: every indel as far left as its repeat (and its neighbours) let it stand
    tables = tables_of(seqs, truth)
    left = [tw.shifted(g, recs, pool, lambda ok: ok[0], gap=1).build() for g, (recs, pool) in zip(seqs, tables)]
    (tmp_path / "left.vcf").write_bytes(vcf_text(seqs, left))
    calls = tables_of(seqs, tmp_path / "left.vcf")
    twin = [tw.compare(g, a, pa, b, pb) for g, (a, pa), (b, pb) in zip(seqs, tables, calls)]
    twin_exact = [tw.compare(g, a, pa, b, pb, True) for g, (a, pa), (b, pb) in zip(seqs, tables, calls)]
    assert all(fa.all() and fb.all() for _, _, fa, fb in twin)
    lost = sum(int((fa == 0).sum()) for _, _, fa, _ in twin_exact)
    assert lost > 50                                       # the genome makes it certain: most indels stood to the right of their repeat's start
    run_cli(["-o", tmp_path / "norm", d / "g.fa", "compare", truth, tmp_path / "left.vcf", "--per-contig"])
    notes, rows = table_rows(tmp_path / "norm_ms.compare.tsv")
    all_ones(rows)
    text = (tmp_path / "norm_ms.compare.tsv").read_text().splitlines()
    assert [l for l in text if l.startswith("# contig ")] == ["# contig ctgA", "# contig ctgB"]
    per = [l.split("\t") for l in text if l.startswith("ALL\t")]
    assert len(per) == 3 and int(per[0][2]) == int(per[1][2]) + int(per[2][2]) == n_lines
    run_cli(["-o", tmp_path / "lit", d / "g.fa", "compare", truth, tmp_path / "left.vcf", "--exact", "--list"])
    notes, rows = table_rows(tmp_path / "lit_ms.compare.tsv")
    assert "# matching: exact (positions compared literally)" in notes
    indel_rows = [rows[(t, b)] for t in ("IN", "DE") for b in compare.BIN_NAMES if int(rows[(t, b)][0])]
    assert any(float(r[5]) < 1 and float(r[6]) < 1 for r in indel_rows)
    assert rows[("SN", ".")][5] == rows[("SN", ".")][6] == "1.000000"
    assert int(rows[("ALL", ".")][3]) == int(rows[("ALL", ".")][4]) == lost
    want = []
    for name, (a, _), (b, _), (_, _, fa, fb) in zip(NAMES, tables, calls, twin_exact):
        want += [f"{k}\t{name}\t{p + 1}\t{compare.TYPE_NAMES[t]}\t{n}" for k, p, t, n in tw.unmatched(a, fa, b, fb)]
    assert (tmp_path / "lit_ms.compare.records.tsv").read_text().splitlines() == want and len(want) == 2 * lost


def test_cli_one_haplotype_of_a_diploid_truth(genome, tmp_path):
    d, seqs = genome
    run_cli(args_run(d, tmp_path / "d", "--ploidy", "2"))
    truth = tmp_path / "d_ms.vcf"
    lines = data_lines(truth.read_bytes())[1].splitlines()
    on2 = sum(1 for l in lines if l.split(b"\t")[9] in (b"0|1", b"1|1"))
    on1 = sum(1 for l in lines if l.split(b"\t")[9] in (b"1|0", b"1|1"))
    assert 0 < on2 < len(lines) and on1 != on2
    run_cli(["-o", tmp_path / "h2", d / "g.fa", "compare", truth, truth, "--truth-haplotype", 2, "--haplotype", 2])
    notes, rows = table_rows(tmp_path / "h2_ms.compare.tsv")
    all_ones(rows)
    assert int(rows[("ALL", ".")][0]) == on2
    assert "# truth: sample (first) haplotype 2" in notes and "# calls: sample (first) haplotype 2" in notes
    # haplotype 1 against haplotype 2: what both carry is found, the rest is missed or extra
    run_cli(["-o", tmp_path / "h12", d / "g.fa", "compare", truth, truth, "--haplotype", 2])
    _, rows = table_rows(tmp_path / "h12_ms.compare.tsv")
    both = sum(1 for l in lines if l.split(b"\t")[9] == b"1|1")
    assert int(rows[("ALL", ".")][0]) == on1 and int(rows[("ALL", ".")][1]) == on2 and int(rows[("ALL", ".")][2]) >= both
    assert int(rows[("ALL", ".")][3]) > 0 and int(rows[("ALL", ".")][4]) > 0


def test_cli_refused_lines_name_their_file(genome, tmp_path):
    d, seqs = genome
    run_cli(args_run(d, tmp_path / "o"))
    good = tmp_path / "o_ms.vcf"
    raw = good.read_bytes().split(b"\n")
    k = next(i for i, l in enumerate(raw) if l and not l.startswith(b"#")) + 5
    fields = raw[k].split(b"\t")
    fields[3] = b"N" + fields[3][1:]                       # REF is not the genome's
    raw[k] = b"\t".join(fields)
    (tmp_path / "bad.vcf").write_bytes(b"\n".join(raw))
    err = run_cli(["-o", tmp_path / "p", d / "g.fa", "compare", tmp_path / "bad.vcf", good], expect=1)
    assert f"truth VCF line {k + 1}: " in err
    err = run_cli(["-o", tmp_path / "p", d / "g.fa", "compare", good, tmp_path / "bad.vcf", "--list"], expect=1)
    assert f"calls VCF line {k + 1}: " in err
    err = run_cli(["-o", tmp_path / "p", d / "g.fa", "compare", good, good, "--sample", "nobody"], expect=1)
    assert "calls VCF: the VCF has no sample column 'nobody'" in err
    assert not list(tmp_path.glob("p_ms*"))
