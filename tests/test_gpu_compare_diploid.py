"""``compare --diploid`` on the device: ``msim_cmp_join`` (csrc/compare.hip: ``k_join_flag``, ``k_join_put2``, ``k_join_put1``) and
``msim_cmp_counts_diploid`` (``k_cmp_match<3>``, ``k_cmp_tally<3>``) on hand-built and planned record tables, and the command line.
Every result is held against ``dip_twin`` (the rules in Python) AND against the library's sequential restatements
(``_ffi.cmp_join_host``, ``_ffi.cmp_counts_diploid_host``) through ``cmp_fetch_diploid``; all comparisons are exact.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import cmp_twin as tw
import dip_twin as dt
from mutation_simulator_amd import _ffi, compare
from mutation_simulator_amd.vcf_replay import plan_all, plan_loaded
from test_gpu_compare import ALT_OF, KEY, NAMES, args_run, genome  # noqa: F401  (genome: the module's fixture, shared)
from test_gpu_sampler import _params, _sv_range
from test_gpu_spectrum import data_lines, run_cli

pytestmark = pytest.mark.gpu

PASS, TILE = _ffi.CMP_PASS, _ffi.CMP_JOIN_TILE
CASES = dt.small_cases(PASS, TILE)
TRUTH, CALLS = _ffi.CMP_TRUTH, _ffi.CMP_CALLS


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def same(got, want, names, what):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, np.flatnonzero(g.view(np.uint8) != w.view(np.uint8))[:8])


def join_side(eng, cid, side, h1, p1, h2, p2):
    """H1 installed and held, H2 installed, the two joined into the contig's diploid table of ``side``."""
    eng.set_records(cid, h1, p1)
    eng.cmp_hold(cid)
    eng.set_records(cid, h2, p2)
    eng.cmp_join(cid, side)


def invariants(counts, n_truth, n_calls):
    assert np.array_equal(counts[..., 0], counts[..., 3]) and np.array_equal(counts[..., 1], counts[..., 4])
    assert int(counts[..., :3].sum()) == n_truth and int(counts[..., 3:].sum()) == n_calls


def check(eng, bases, truth, calls, exact=False, twin=True):
    """A fresh contig, both sides joined and counted: the device's tables, counts, tallies and flags against the twin and the
    host restatements.  Returns ((U, pool, gt) of the truth, ... of the calls, (counts, tallies, flags, flags))."""
    eng.clear()
    cid = eng.add_contig(bases)
    join_side(eng, cid, TRUTH, *truth)
    join_side(eng, cid, CALLS, *calls)
    counts, tallies = eng.cmp_counts_diploid(cid, exact)
    sides = []
    for side, tables in ((TRUTH, truth), (CALLS, calls)):
        u, pool, gt, flags = eng.cmp_fetch_diploid(cid, side)
        if twin:
            same((u, pool, gt), dt.join(*tables), ("records", "pool", "genotypes"), "twin join")
        same((u, pool, gt), _ffi.cmp_join_host(*tables), ("records", "pool", "genotypes"), "host join")
        sides.append((u, pool, gt, flags))
    (a, pa, ga, fa), (b, pb, gb, fb) = sides
    got = (counts, tallies, fa, fb)
    names = ("counts", "tallies", "truth flags", "calls flags")
    if twin:
        same(got, dt.score(bases, a, pa, ga, b, pb, gb, exact), names, "twin")
    same(got, _ffi.cmp_counts_diploid_host(bases, a, pa, ga, b, pb, gb, exact), names, "host restatement")
    invariants(counts, len(a), len(b))
    return (a, pa, ga), (b, pb, gb), got


def totals(counts):
    """(TP, GT, truth missed, calls extra)"""
    return tuple(int(counts[..., k].sum()) for k in (0, 1, 2, 5))


# ------------------------------------------------------------------------------ 1. the small shapes
@pytest.mark.parametrize("case", sorted(CASES))
def test_small_shapes(eng, case):
    bases, truth, calls, exact = CASES[case]
    (a, pa, ga), (b, pb, gb), (counts, tallies, fa, fb) = check(eng, bases, truth, calls, exact)
    if case == "both_empty":
        assert len(a) == len(b) == 0 and not counts.any() and fa.shape == fb.shape == (0,)
    if case == "equal":
        assert ga.tolist() == [3] * len(truth[0]) and len(a) == len(truth[0])
    if case == "same_pos_other_sn_base":
        assert a["pos"].tolist() == [9, 9, 30] and ga.tolist() == [1, 2, 3]
    if case == "ins_pool_offsets":
        assert ga.tolist() == [1, 3, 2] and [tw.insert_of(r, pa) for r in a] == [b"GT", b"ACG", b"TTA"]
    if case == "h2_all_duplicates":
        assert len(a) == len(truth[0]) > len(truth[2]) and int((ga == 3).sum()) == len(truth[2])
    want = {"het_het_other_phase": (1, 0, 0, 0), "het_hom": (0, 2, 0, 0), "multi_allelic_1_2_vs_2_1": (2, 0, 0, 0),
            "shifted_equal_dosage": (1, 0, 0, 0), "shifted_equal_dosage_exact": (0, 0, 1, 1), "shifted_unequal_dosage": (0, 1, 0, 0),
            "rank_mixed_dosages": (2, 0, 1, 0), "rank_mixed_dosages_crossed": (0, 2, 1, 0), "every_type": (0, 7, 0, 0)}.get(case)
    if want:
        assert totals(counts) == want
    # the sides change places: the halves of the counts do
    swapped = check(eng, bases, calls, truth, exact)[2][0]
    assert np.array_equal(swapped[..., :3], counts[..., 3:]) and np.array_equal(swapped[..., 3:], counts[..., :3])
    eng.clear()


# ------------------------------------------------------------------------------ 2. the calls' lifetime and the refusals
def test_lifetime_and_refusals(eng):
    eng.clear()
    eng.reset_stats()
    assert eng.cmp_join_timing() == 0.0
    bases, truth, calls, _ = CASES["disjoint"]
    h1, p1, h2, p2 = truth
    cid = eng.add_contig(bases)
    with pytest.raises(_ffi.MsimError, match="contig has not been planned") as e:
        eng.cmp_join(cid, TRUTH)
    assert e.value.code == _ffi.ERR_ARG
    eng.set_records(cid, h1, p1)
    with pytest.raises(_ffi.MsimError, match="no held table") as e:
        eng.cmp_join(cid, TRUTH)
    assert e.value.code == _ffi.ERR_ARG
    eng.cmp_hold(cid)
    for side in (2, -1):
        with pytest.raises(_ffi.MsimError, match="unknown side") as e:
            eng.cmp_join(cid, side)
        assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError, match="no diploid table of both sides") as e:
        eng.cmp_counts_diploid(cid)
    assert e.value.code == _ffi.ERR_ARG
    # two empty inputs: an empty diploid table, nothing launched
    none = h1[:0]
    join_side(eng, cid, TRUTH, none, tw.NO_POOL, none, tw.NO_POOL)
    assert eng.cmp_join_timing() == 0.0
    with pytest.raises(_ffi.MsimError, match="no diploid table of both sides"):
        eng.cmp_counts_diploid(cid)                        # (one side only)
    with pytest.raises(_ffi.MsimError, match="no diploid table of both sides"):
        eng.cmp_fetch_diploid(cid, TRUTH)
    join_side(eng, cid, CALLS, none, tw.NO_POOL, none, tw.NO_POOL)
    counts, tallies = eng.cmp_counts_diploid(cid)
    assert not counts.any() and not tallies.any() and eng.cmp_join_timing() == 0.0 and eng.cmp_timing() == 0.0
    # the join consumes the held table; a new join replaces the side's table
    with pytest.raises(_ffi.MsimError, match="no held table"):
        eng.cmp_join(cid, TRUTH)
    join_side(eng, cid, TRUTH, *truth)
    join_side(eng, cid, CALLS, *calls)
    assert 0 < eng.cmp_join_timing() < 1000
    with pytest.raises(_ffi.MsimError, match="call it first"):
        eng.cmp_fetch_diploid(cid, TRUTH)                  # (no counts since the joins)
    assert eng.cmp_fetch_diploid(cid, TRUTH, flags=False)[0].tobytes() == dt.join(*truth)[0].tobytes()
    want = eng.cmp_counts_diploid(cid)
    assert totals(want[0]) == (9, 0, 0, 0)
    # the diploid tables survive a new plan of the contig and its release, and msim_cmp_counts beside them is what it was
    bb, a, pa, b, pb, _ = tw.small_cases(PASS)["disjoint"]
    assert bb.tobytes() == bases.tobytes()
    eng.set_records(cid, a, pa)
    eng.cmp_hold(cid)
    eng.set_records(cid, b, pb)
    haploid = eng.cmp_counts(cid)
    for g, w in zip(haploid + eng.cmp_fetch(cid)[2:], _ffi.cmp_counts_host(bases, a, pa, b, pb)):
        assert np.array_equal(g, w)
    eng.release_result(cid)
    again = eng.cmp_counts_diploid(cid)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    # ... and go with msim_cmp_release and with msim_clear
    eng.cmp_release(cid)
    with pytest.raises(_ffi.MsimError, match="no diploid table of both sides"):
        eng.cmp_counts_diploid(cid)
    join_side(eng, cid, TRUTH, *truth)
    join_side(eng, cid, CALLS, *calls)
    eng.cmp_counts_diploid(cid)
    eng.clear()
    cid = eng.add_contig(bases)
    with pytest.raises(_ffi.MsimError, match="no diploid table of both sides"):
        eng.cmp_counts_diploid(cid)
    eng.reset_stats()
    assert eng.cmp_join_timing() == 0.0
    eng.clear()


# ------------------------------------------------------------------------------ 3. a planned table with drawn genotypes
BIG_N = (1 << 17) + 1


def test_planned_table_of_2_17_plus_1_records(eng):
    """The shape of ``test_gpu_compare``'s ``big``: an SV mix the counter-based engine planned on runs of A and C, genotypes
    from ``msim_genotype_contig``; each side's haplotypes are the library's own selections.  The calls are the same records
    with every indel at a random placement of its interval and every tenth het made hom: those are found with the wrong
    genotype, everything else is found."""
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
    a = a[:BIG_N].copy()
    assert len(a) == BIG_N
    b, pb = tw.shifted(bases, a, pa, lambda ok: ok[int(rs.randint(0, len(ok)))]).build()
    assert len(b) == BIG_N and int((a["pos"] != b["pos"]).sum()) > 10_000
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, a, pa)
    eng.genotype_contig(cid, KEY, 0, 1 << 52)              # half of the records heterozygous
    gt = eng.fetch_genotypes(cid, BIG_N)
    hets = np.flatnonzero(gt != 3)
    changed = hets[::10]
    assert len(hets) > 50_000 and int((gt == 1).sum()) > 20_000 and int((gt == 2).sum()) > 20_000
    gt_calls = gt.copy()
    gt_calls[changed] = 3
    sides = []
    both = ((TRUTH, a, pa, gt), (CALLS, b, pb, gt_calls))
    for side, recs, pool, g in both:
        eng.set_records(cid, recs, pool)
        eng.set_genotypes(cid, g)
        eng.select_haplotype(cid, 1)
        eng.cmp_hold(cid)
        eng.select_haplotype(cid, 2)
        eng.cmp_join(cid, side)
    for side, recs, pool, g in both:
        u, upool, ugt, _ = eng.cmp_fetch_diploid(cid, side, flags=False)
        # the join puts the two selections together again: the table, its genotypes, the pool twice
        assert np.array_equal(ugt, g) and upool.tobytes() == pool.tobytes() * 2
        want = recs.copy()
        only2 = (g == 2) & (recs["type"] == tw.IN)
        want["extra"][only2] += len(pool)
        assert u.tobytes() == want.tobytes()
        h1, h2 = recs[(g & 1) != 0], recs[(g & 2) != 0]
        same((u, upool, ugt), _ffi.cmp_join_host(h1, pool, h2, pool), ("records", "pool", "genotypes"), "host join")
        sides.append((u, upool, ugt))
    (ua, upa, uga), (ub, upb, ugb) = sides
    counts, tallies = eng.cmp_counts_diploid(cid)
    fa, fb = eng.cmp_fetch_diploid(cid, TRUTH)[3], eng.cmp_fetch_diploid(cid, CALLS)[3]
    names = ("counts", "tallies", "truth flags", "calls flags")
    same((counts, tallies, fa, fb), dt.score(bases, ua, upa, uga, ub, upb, ugb), names, "twin")
    same((counts, tallies, fa, fb), _ffi.cmp_counts_diploid_host(bases, ua, upa, uga, ub, upb, ugb), names, "host restatement")
    invariants(counts, BIG_N, BIG_N)
    assert totals(counts) == (BIG_N - len(changed), len(changed), 0, 0) and not tallies.any()
    assert np.array_equal(np.flatnonzero(fa == 2), changed) and np.array_equal(fa, fb)
    # the haploid counts of the same context are what they are without a diploid run beside them
    eng.set_records(cid, a, pa)
    eng.cmp_hold(cid)
    eng.set_records(cid, b, pb)
    haploid = eng.cmp_counts(cid)
    assert int(haploid[0][..., 0].sum()) == BIG_N and not haploid[0][..., 1].any() and not haploid[0][..., 3].any()
    eng.clear()


# ------------------------------------------------------------------------------ 4. one scoring path for both comparisons
HAPLOID_CASES = tw.small_cases(PASS)
HAPLOID_OF_DIPLOID = (0, 2, 3, 5)          # truth matched, missed, calls matched, extra among the six values of a diploid cell


def check_haploid_is_diploid(eng, bases, a, pa, b, pb, exact=False):
    """``cmp_counts`` of ``a`` against ``b``, then each table joined with itself -- installed, held, left current, joined: every
    record of haplotype 2 is haplotype 1's again -- and ``cmp_counts_diploid``: the same records with every genotype byte 3 and
    the pool twice, the haploid counts with two empty columns, the same tallies and flags.  Returns the haploid result."""
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, a, pa)
    eng.cmp_hold(cid)
    eng.set_records(cid, b, pb)
    want = eng.cmp_counts(cid, exact) + eng.cmp_fetch(cid)[2:]
    for side, recs, pool in ((TRUTH, a, pa), (CALLS, b, pb)):
        eng.set_records(cid, recs, pool)
        eng.cmp_hold(cid)
        eng.cmp_join(cid, side)
    counts, tallies = eng.cmp_counts_diploid(cid, exact)
    flags = []
    for side, recs, pool in ((TRUTH, a, pa), (CALLS, b, pb)):
        u, upool, gt, fl = eng.cmp_fetch_diploid(cid, side)
        assert u.tobytes() == np.ascontiguousarray(recs).tobytes() and upool.tobytes() == np.ascontiguousarray(pool).tobytes() * 2
        assert gt.shape == (len(recs),) and (gt == 3).all()
        flags.append(fl)
    assert np.array_equal(counts[..., HAPLOID_OF_DIPLOID], want[0]) and not counts[..., (1, 4)].any()
    same((tallies, *flags), want[1:], ("tallies", "truth flags", "calls flags"), "haploid")
    eng.clear()
    return want


@pytest.mark.parametrize("case", sorted(HAPLOID_CASES))
def test_haploid_small_shapes_as_diploid(eng, case):
    check_haploid_is_diploid(eng, *HAPLOID_CASES[case])


def test_sn_table_past_the_grid_cap_as_diploid(eng):
    """``2048 * PASS + 1`` SN records a side (``test_gpu_compare``'s table past the grid cap): the first size at which a workgroup
    of the diploid instantiation takes a second pass.  The closed form: 524 changed records, each missed once and extra once."""
    n = 2048 * PASS + 1
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(5).randint(0, 4, n)]
    a = np.zeros(n, dtype=_ffi.RECORD_DTYPE)
    a["pos"] = a["stop"] = np.arange(n, dtype=np.uint32)
    a["type"] = tw.SN
    a["aux"] = np.arange(n) % 3
    changed = np.arange(999, n, 1000)
    b = a.copy()
    b["aux"][changed] = (b["aux"][changed] + 1) % 3
    counts, tallies, fa, fb = check_haploid_is_diploid(eng, bases, a, tw.NO_POOL, b, tw.NO_POOL)
    assert len(changed) == 524 and counts[tw.SN, 0].tolist() == [n - 524, 524, n - 524, 524] and not tallies.any()
    assert np.array_equal(np.flatnonzero(fa == 0), changed) and np.array_equal(fa, fb)


# ------------------------------------------------------------------------------ 5. the command line
def haplotype_tables(seqs, vcf_path, names=NAMES):
    """The two record tables the consensus parser makes of a VCF's first sample, per contig: [(H1, pool, H2, pool)]."""
    e = _ffi.Engine(0)
    try:
        cids = [e.add_contig(s) for s in seqs]
        text = np.fromfile(vcf_path, dtype=np.uint8)
        plan_all(e, text, list(names), cids, (None, 1))
        first = [e.fetch_records(c) for c in cids]
        plan_loaded(e, text, list(names), cids, (None, 2))
        return [h1 + e.fetch_records(c) for h1, c in zip(first, cids)]
    finally:
        e.close()


def twin_of(seqs, truth_tables, calls_tables, exact=False):
    """Per contig: (the truth's U, pool, gt), (the calls'), the twin's (counts, tallies, flags, flags)."""
    out = []
    for g, t, c in zip(seqs, truth_tables, calls_tables):
        a, b = dt.join(*t), dt.join(*c)
        out.append((a, b, dt.score(g, *a, *b, exact)))
    return out


def table_rows(path):
    """(comment lines, {(type, length): [truth, calls, TP, FN, FP, GT, recall, precision]} of the genome-wide block)."""
    lines = path.read_text().splitlines()
    notes = [l for l in lines if l.startswith("#")]
    body = [l.split("\t") for l in lines if not l.startswith("#")]
    assert body[0] == list(compare.HEADER_DIPLOID)
    return notes, {(r[0], r[1]): r[2:] for r in body[1:1 + len(compare.ROWS) + 1]}


def body_of(path):
    return [l for l in path.read_text().splitlines() if not l.startswith("#")]


def all_ones(rows):
    assert all(r[6] in ("1.000000", "NA") and r[7] in ("1.000000", "NA") and r[3] == r[4] == r[5] == "0" for r in rows.values()), rows
    for key in (("SN", "."), ("IN", "1"), ("IN", "2-5"), ("DE", "1"), ("DE", "2-5"), ("ALL", ".")):
        assert rows[key][6] == rows[key][7] == "1.000000" and int(rows[key][0]) > 20, key


def rewritten(vcf: bytes, genotype) -> bytes:
    """The VCF with every data line's genotype field replaced by ``genotype(data line number, old field)``."""
    out, k = [], 0
    for line in vcf.split(b"\n"):
        if line and not line.startswith(b"#"):
            f = line.split(b"\t")
            f[9] = genotype(k, f[9])
            line = b"\t".join(f)
            k += 1
        out.append(line)
    return b"\n".join(out)


UNPHASED = {b"1|0": b"0/1", b"0|1": b"1/0", b"1|1": b"1/1"}        # every het's phase swapped, written with '/'
FLIPPED = {b"1|0": b"1/1", b"0|1": b"1/1", b"1|1": b"0/1"}


def diploid_vcf_text(seqs, tables) -> bytes:
    """``test_gpu_compare.vcf_text`` with a genotype column: one line a record of (U, pool, gt), unphased."""
    lines = [b"##fileformat=VCFv4.3", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tcaller"]
    for name, g, (recs, pool, gt) in zip(NAMES, seqs, tables):
        s = g.tobytes().decode()
        for r, d in zip(recs, dt.dosage(gt)):
            p, q, typ = int(r["pos"]), int(r["stop"]), int(r["type"])
            if typ == tw.SN:
                pos, ref, alt = p + 1, s[p], ALT_OF[s[p], int(r["aux"])]
            elif typ == tw.DE:
                pos, ref, alt = (p, s[p - 1:q + 1], s[p - 1]) if p else (1, s[:q + 2], s[q + 1])
            else:
                ins = tw.insert_of(r, pool).decode()
                pos, ref, alt = (p, s[p - 1], s[p - 1] + ins) if p else (1, s[0], ins + s[0])
            lines.append(f"{name}\t{pos}\t.\t{ref}\t{alt}\t.\tPASS\t.\tGT\t{'0/1' if d == 1 else '1/1'}".encode())
    return b"\n".join(lines) + b"\n"


def test_cli_diploid(genome, tmp_path):  # noqa: F811
    d, seqs = genome
    fa = d / "g.fa"
    run_cli(args_run(d, tmp_path / "d", "--ploidy", "2"))
    truth = tmp_path / "d_ms.vcf"
    raw = truth.read_bytes()
    lines = data_lines(raw)[1].splitlines()
    n_lines = len(lines)
    genotypes = [l.split(b"\t")[9] for l in lines]
    assert set(genotypes) == set(UNPHASED) and n_lines > 500

    # 1. the truth against itself
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, "-o", tmp_path / "self", fa, "compare", truth, truth, "--diploid", "--list"])
    notes, rows = table_rows(tmp_path / "self_ms.compare.tsv")
    all_ones(rows)
    assert int(rows[("ALL", ".")][0]) == int(rows[("ALL", ".")][1]) == n_lines         # not one haplotype's count
    assert (tmp_path / "self_ms.compare.records.tsv").read_text() == ""
    assert notes[:4] == ["# compare: calls d_ms.vcf against truth d_ms.vcf on g.fa (2 contigs)",
                         "# truth: sample (first) both haplotypes", "# calls: sample (first) both haplotypes",
                         "# genotypes: diploid, unphased (dosage compared; a haploid 1 counts as 1/1)"]
    bench = json.loads(stats.read_text())
    assert bench["cmp_join_kernel_ms"] > 0 and bench["cmp_kernel_ms"] > 0 and bench["vcf_plan_kernel_ms"] > 0
    first = body_of(tmp_path / "self_ms.compare.tsv")

    # 2. the calls as a caller writes them: unphased, every het's phase swapped -- no choice of --haplotype scores these
    (tmp_path / "unphased.vcf").write_bytes(rewritten(raw, lambda k, g: UNPHASED[g]))
    run_cli(["-o", tmp_path / "un", fa, "compare", truth, tmp_path / "unphased.vcf", "--diploid", "--per-contig"])
    text = body_of(tmp_path / "un_ms.compare.tsv")
    assert text[:len(first)] == first
    per = [l.split("\t") for l in text if l.startswith("ALL\t")]
    assert len(per) == 3 and all(int(per[0][k]) == int(per[1][k]) + int(per[2][k]) for k in range(2, 8)) and int(per[1][2]) > 0 < int(per[2][2])
    assert [l for l in (tmp_path / "un_ms.compare.tsv").read_text().splitlines() if l.startswith("# contig ")] == ["# contig ctgA", "# contig ctgB"]

    # 3. ... with every seventh line's genotype flipped het to hom or hom to het
    flipped = list(range(0, n_lines, 7))
    (tmp_path / "flip.vcf").write_bytes(rewritten(raw, lambda k, g: FLIPPED[g] if k % 7 == 0 else UNPHASED[g]))
    run_cli(["-o", tmp_path / "flip", fa, "compare", truth, tmp_path / "flip.vcf", "--diploid", "--list"])
    _, rows = table_rows(tmp_path / "flip_ms.compare.tsv")
    assert rows[("ALL", ".")][:6] == [str(n_lines), str(n_lines), str(n_lines - len(flipped)), str(len(flipped)), str(len(flipped)),
                                      str(len(flipped))]
    listed = (tmp_path / "flip_ms.compare.records.tsv").read_text().splitlines()
    truth_tables = haplotype_tables(seqs, truth)
    twin = twin_of(seqs, truth_tables, haplotype_tables(seqs, tmp_path / "flip.vcf"))
    want = []
    for name, ((a, _, ga), (b, _, gb), (_, _, fa_, fb_)) in zip(NAMES, twin):
        want += [f"{k}\t{name}\t{p + 1}\t{compare.TYPE_NAMES[t]}\t{n}\t{x}\t{y}" for k, p, t, n, x, y in dt.listed(a, ga, fa_, b, gb, fb_)]
    assert listed == want and len(listed) == len(flipped) and all(l.startswith("GT\t") for l in listed)
    was_hom = [genotypes[k] == b"1|1" for k in flipped]                                # (the lines are in table order)
    assert [l.split("\t")[5:] for l in listed] == [["1/1", "0/1"] if hom else ["0/1", "1/1"] for hom in was_hom]

    # 4. ... with every indel left-aligned
    left = [tw.shifted(g, a, pa, lambda ok: ok[0], gap=1).build() + (ga,) for g, ((a, pa, ga), _, _) in zip(seqs, twin)]
    (tmp_path / "left.vcf").write_bytes(diploid_vcf_text(seqs, left))
    left_tables = haplotype_tables(seqs, tmp_path / "left.vcf")
    twin_exact = twin_of(seqs, truth_tables, left_tables, exact=True)
    assert all((fa_ == 1).all() and (fb_ == 1).all() for _, _, (_, _, fa_, fb_) in twin_of(seqs, truth_tables, left_tables))
    tp, gt_pairs = (sum(int((fa_ == f).sum()) for _, _, (_, _, fa_, _) in twin_exact) for f in (1, 2))
    lost = n_lines - tp - gt_pairs                         # the moved indels: each missed once and extra once
    assert lost > 50 and lost == sum(int((fb_ == 0).sum()) for _, _, (_, _, _, fb_) in twin_exact)
    run_cli(["-o", tmp_path / "norm", fa, "compare", truth, tmp_path / "left.vcf", "--diploid"])
    assert body_of(tmp_path / "norm_ms.compare.tsv") == first
    run_cli(["-o", tmp_path / "lit", fa, "compare", truth, tmp_path / "left.vcf", "--diploid", "--exact"])
    notes, rows = table_rows(tmp_path / "lit_ms.compare.tsv")
    assert "# matching: exact (positions compared literally)" in notes
    assert rows[("ALL", ".")][:6] == [str(n_lines), str(n_lines), str(tp), str(lost + gt_pairs), str(lost + gt_pairs), str(gt_pairs)]
    assert gt_pairs < lost // 10                           # (a moved indel may land on another record of its class: rare)
    assert rows[("SN", ".")][6] == rows[("SN", ".")][7] == "1.000000"

    # 6. without --diploid the files are what they were: the existing renderers over the device's haploid counts
    run_cli(["-o", tmp_path / "hap", fa, "compare", truth, tmp_path / "flip.vcf", "--list", "--per-contig"])
    e = _ffi.Engine(0)
    try:
        cids = [e.add_contig(s) for s in seqs]
        plan_all(e, np.fromfile(truth, dtype=np.uint8), list(NAMES), cids, (None, 1))
        for c in cids:
            e.cmp_hold(c)
        plan_all(e, np.fromfile(tmp_path / "flip.vcf", dtype=np.uint8), list(NAMES), cids, (None, 1))
        got = [e.cmp_counts(c) for c in cids]
        rows = []
        for name, c in zip(NAMES, cids):
            held, _, fa_, fb_ = e.cmp_fetch(c)
            rows += compare.record_rows("FN", name, held, fa_) + compare.record_rows("FP", name, e.fetch_records(c)[0], fb_)
    finally:
        e.close()
    tallies = sum(t for _, t in got)
    notes = ["compare: calls flip.vcf against truth d_ms.vcf on g.fa (2 contigs)", "truth: sample (first) haplotype 1",
             "calls: sample (first) haplotype 1", "matching: normalised (an indel matches any placement inside its repeat)",
             f"truth indels whose placements end at a window edge: {int(tallies[0])}",
             f"truth indels whose placements end at a base outside ACGT: {int(tallies[1])}"]
    assert (tmp_path / "hap_ms.compare.tsv").read_text() == compare.render(notes, np.stack([c for c, _ in got]), list(NAMES))
    assert (tmp_path / "hap_ms.compare.records.tsv").read_text() == "".join(r + "\n" for r in rows) and rows


def test_cli_multi_allelic_and_overlapping_haplotypes(tmp_path):
    """A hand-written pair: a ``1|2`` SNP, and a deletion on one haplotype that overlaps an SNP on the other -- one table could
    not hold the two, a haplotype's table can."""
    s = tw.RANDOM_200
    (tmp_path / "g.fa").write_text(">c\n" + s + "\n")
    other = {b: [x for x in "ACGT" if x != b] for b in "ACGT"}
    head = "##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\n"

    def line(pos, ref, alt, gt):
        return f"c\t{pos}\t.\t{ref}\t{alt}\t.\tPASS\t.\tGT\t{gt}\n"
    x, y = other[s[9]][:2]
    (tmp_path / "t.vcf").write_text(head + line(10, s[9], f"{x},{y}", "1|2") + line(20, s[19:23], s[19], "1|0") +
                                    line(22, s[21], other[s[21]][0], "0|1") + line(40, s[39], other[s[39]][2], "1|1"))
    (tmp_path / "c.vcf").write_text(head + line(10, s[9], f"{y},{x}", "2/1") + line(20, s[19:23], s[19], "1|0") +
                                    line(22, s[21], other[s[21]][0], "0|1") + line(40, s[39], other[s[39]][2], "0/1"))
    seqs = [tw.as_bases(s)]
    run_cli(["-o", tmp_path / "o", tmp_path / "g.fa", "compare", tmp_path / "t.vcf", tmp_path / "c.vcf", "--diploid", "--list"])
    truth, calls = haplotype_tables(seqs, tmp_path / "t.vcf", ("c",)), haplotype_tables(seqs, tmp_path / "c.vcf", ("c",))
    assert [len(t) for t in truth[0][::2]] == [3, 3]       # each haplotype: its allele of the 1|2, the deletion or the SNP, the 1|1
    (a, _, ga), (b, _, gb), (counts, _, fa_, fb_) = twin_of(seqs, truth, calls)[0]
    assert a["pos"].tolist() == [9, 9, 20, 21, 39] and ga.tolist() == [1, 2, 1, 2, 3]
    assert body_of(tmp_path / "o_ms.compare.tsv") == compare.render_block(counts)
    _, rows = table_rows(tmp_path / "o_ms.compare.tsv")
    assert rows[("SN", ".")][:6] == ["4", "4", "3", "1", "1", "1"] and rows[("DE", "2-5")][:6] == ["1", "1", "1", "0", "0", "0"]
    assert (tmp_path / "o_ms.compare.records.tsv").read_text() == "GT\tc\t40\tSN\t1\t1/1\t0/1\n"
    # together on one haplotype the deletion and the SNP are refused, with the file and the line named
    (tmp_path / "bad.vcf").write_text(head + line(20, s[19:23], s[19], "0/1") + line(22, s[21], other[s[21]][0], "0/1"))
    err = run_cli(["-o", tmp_path / "p", tmp_path / "g.fa", "compare", tmp_path / "t.vcf", tmp_path / "bad.vcf", "--diploid"], expect=1)
    assert "calls VCF line 4: " in err and not list(tmp_path.glob("p_ms*"))
