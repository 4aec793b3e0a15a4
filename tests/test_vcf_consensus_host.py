"""CPU tier of ``vcf --consensus``: libmsim's host parser (host-only context, csrc/vcf_parse.hip: plan_host_cons) and the
reference rewrite (tests/apply_ref.py) against the mode's plain restatement (tests/consensus_ref.py), plus the command line.

The hand-written cases and refusals below are also what tests/test_gpu_vcf_consensus.py holds the device parser against.
"""
from __future__ import annotations

import contextlib
import io
import random
from pathlib import Path

import numpy as np
import pytest

import apply_ref
import consensus_ref as cref
import mutation_simulator_amd as msa
import vcf_replay_ref
from helpers import CASES, case_input_bytes, case_meta, parse_fasta_bytes
from mutation_simulator_amd import _ffi, vcf_replay

#          1234567890123456789012345678901 2
C1, C2 = b"ACGTACGTAGCTAGCTNNACGTRYACGTACGT", b"TTGACCA"
GENOME = [{"name": "c1", "bases": np.frombuffer(C1, dtype=np.uint8)}, {"name": "c2", "bases": np.frombuffer(C2, dtype=np.uint8)}]


def header(samples=("x",)):
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + ("\tFORMAT\t" + "\t".join(samples) if samples else "")
    return ("##fileformat=VCFv4.3\n" + cols + "\n").encode()                  # lines 1-2: the first data line is line 3


def ln(chrom, pos, ref, alt, gts=("1",), fmt="GT", info=".", ident="."):
    tail = "" if gts is None else f"\t{fmt}\t" + "\t".join(gts)
    return f"{chrom}\t{pos}\t{ident}\t{ref}\t{alt}\t.\tPASS\t{info}{tail}\n".encode()


def case(lines, samples=("x",), sample=None, hap=1):
    return header(samples) + b"".join(lines), sample, hap


ACCEPTED = {
    "snv_lut_transition": case([ln("c1", 2, "C", "T")]),
    "snv_lut_transversions": case([ln("c1", 2, "C", "A"), ln("c1", 4, "T", "A")]),
    "snv_n_to_a": case([ln("c1", 17, "N", "A")]),
    "snv_a_to_n": case([ln("c1", 5, "A", "N")]),
    "snv_alt_is_genome_base": case([ln("c1", 5, "A", "A"), ln("c1", 6, "C", "G")]),
    "snv_iupac_raw_reachable": case([ln("c1", 23, "R", "G")]),
    "snv_iupac_converted_reachable": case([ln("c1", 23, "A", "G")]),
    "snv_iupac_raw_unreachable": case([ln("c1", 23, "R", "A")]),
    "snv_iupac_converted_unreachable": case([ln("c1", 24, "C", "C")]),
    "mnp": case([ln("c1", 2, "CGT", "TAC")]),
    "ins_leading": case([ln("c1", 5, "A", "ATT")]),
    "ins_trailing": case([ln("c1", 5, "A", "TTA")]),
    "ins_no_anchor": case([ln("c1", 5, "A", "TT")]),
    "del_leading": case([ln("c1", 5, "ACG", "A")]),
    "del_trailing": case([ln("c1", 5, "ACG", "G")]),
    "del_no_anchor": case([ln("c1", 5, "ACG", "T")]),
    "complex_leading": case([ln("c1", 5, "ACG", "ATT")]),
    "complex_trailing": case([ln("c1", 5, "ACG", "TTG")]),
    "complex_no_anchor": case([ln("c1", 5, "ACG", "TT")]),
    "same_ref_alt": case([ln("c1", 5, "ACG", "ACG"), ln("c1", 10, "G", "g")]),
    "leading_anchor_on_iupac_del": case([ln("c1", 23, "AC", "A")]),
    "leading_anchor_on_iupac_ins": case([ln("c1", 23, "R", "RGG")]),
    "deletion_to_last_base": case([ln("c2", 5, "CCA", "C")]),
    "insertion_before_base_0": case([ln("c1", 1, "A", "GGA")]),
    "lead_would_hit_end_uses_trailing": case([ln("c2", 7, "A", "AA")]),
    "lower_case": case([ln("c1", 5, "acg", "a"), ln("c1", 10, "g", "gtt")]),
    "eight_fields": case([ln("c1", 2, "C", "T", gts=None), ln("c2", 3, "G", "GAA,T", gts=None)], samples=()),
    "three_samples_by_name": case([ln("c1", 2, "C", "T", ("0", "1", "0")), ln("c1", 5, "A", "ATT", ("1", "0", "1"))],
                                  samples=("s1", "s2", "s3"), sample="s2"),
    "three_samples_last": case([ln("c1", 2, "C", "T", ("0", "1", "0")), ln("c1", 5, "A", "ATT", ("1", "0", "1"))],
                               samples=("s1", "s2", "s3"), sample="s3"),
    "het_0_1_hap1": case([ln("c1", 2, "C", "T", ("0|1",))], hap=1),
    "het_0_1_hap2": case([ln("c1", 2, "C", "T", ("0|1",))], hap=2),
    "three_alts_1_2_hap1": case([ln("c1", 2, "C", "T,G,CAA", ("1/2",))], hap=1),
    "three_alts_1_2_hap2": case([ln("c1", 2, "C", "T,G,CAA", ("1/2",))], hap=2),
    "three_alts_third": case([ln("c1", 2, "C", "T,G,CAA", ("3",))]),
    "haploid_under_hap2": case([ln("c1", 2, "C", "T", ("1",))], hap=2),
    "skipped_genotypes": case([ln("c1", 2, "G", "T", (".",)), ln("c1", 99, "C", "<X>", ("./.",)), ln("c1", "x", "", "", ("0",)),
                               ln("c1", 6, "C", "T")]),
    "star_allele": case([ln("c1", 2, "C", "*,T", ("1",)), ln("c1", 6, "C", "*,T", ("2",)), ln("c1", 8, "G", "*")]),
    "other_alt_symbolic": case([ln("c1", 2, "C", "T,<DEL>", ("1",))]),
    "long_info_and_id": case([ln("c1", 2, "C", "T", info="AC=" + "1," * 150, ident="rs" + "7" * 300)]),
    "gt_with_subfields": case([ln("c1", 2, "C", "T", ("1:30:99",), fmt="GT:DP:GQ"), ln("c1", 6, "C", "T", ("0/1:3:9",), fmt="GT:DP:GQ")]),
    "two_contigs_mixed": case([ln("c1", 1, "A", "GGA"), ln("c1", 3, "GT", "G"), ln("c1", 7, "GTA", "CC"), ln("c1", 12, "T", "A"),
                               ln("c1", 30, "CGT", "C"), ln("c2", 1, "T", "C"), ln("c2", 3, "GA", "TTT"), ln("c2", 7, "A", "AA")]),
    "no_chrom_line": (b"##fileformat=VCFv4.3\n" + ln("c1", 2, "C", "T", ("0", "1")) + ln("c1", 6, "C", "T", ("1", "0")), None, 1),
    "last_line_open": (header() + ln("c1", 2, "C", "T") + ln("c1", 5, "ACG", "A")[:-1], None, 1),
    "header_only": (header(), None, 1),
}

LONG_ALT = "A" * 4096
REFUSALS = {
    # name: (case, offending line, reason)
    "end_no_anchor": (case([ln("c2", 7, "A", "AG")]), 3, cref.END),
    "end_unreachable_snv": (case([ln("c2", 7, "A", "N")]), 3, cref.END),
    "end_mnp": (case([ln("c1", 2, "C", "T"), ln("c2", 6, "CA", "TG")]), 4, cref.END),
    "allele_index_beyond": (case([ln("c1", 2, "C", "T", ("2",))]), 3, cref.ALLELE),
    "symbolic_del": (case([ln("c1", 4, "T", "<DEL>")]), 3, cref.ALLELE),
    "breakend": (case([ln("c1", 4, "T", "T[c2:3[")]), 3, cref.ALLELE),
    "alt_not_a_letter": (case([ln("c1", 2, "C", "CA7T")]), 3, cref.INSERT),
    "alt_star_inside": (case([ln("c1", 2, "C", "C*")]), 3, cref.INSERT),
    "ref_mismatch": (case([ln("c1", 2, "G", "A")]), 3, cref.REF),
    "ref_mismatch_inside": (case([ln("c1", 5, "ACT", "A")]), 3, cref.REF),
    "ref_past_contig": (case([ln("c2", 6, "CATT", "C")]), 3, cref.REF),
    "overlap": (case([ln("c1", 4, "TACG", "T"), ln("c1", 6, "C", "T")]), 4, cref.ORDER),
    "line_at_insertion_anchor_plus_1": (case([ln("c1", 5, "A", "ATT"), ln("c1", 6, "C", "T")]), 4, cref.ORDER),
    "positions_equal": (case([ln("c1", 2, "C", "T"), ln("c1", 2, "C", "G")]), 4, cref.ORDER),
    "field_count_differs": (case([ln("c1", 2, "C", "T"), ln("c1", 6, "C", "T", ("1", "1"))]), 4, cref.FIELDS),
    "nine_fields": (case([b"c1\t2\t.\tC\tT\t.\t.\t.\tGT\n"]), 3, cref.FIELDS),
    "format_not_gt_first": (case([ln("c1", 2, "C", "T", ("3:1",), fmt="DP:GT")]), 3, cref.SAMPLE),
    "format_gtx": (case([ln("c1", 2, "C", "T", fmt="GTX")]), 3, cref.SAMPLE),
    "genotype_letter": (case([ln("c1", 2, "C", "T", ("x",))]), 3, cref.SAMPLE),
    "genotype_empty_entry": (case([ln("c1", 2, "C", "T", ("1/",))], hap=2), 3, cref.SAMPLE),
    "genotype_haplotype_beyond": (case([ln("c1", 2, "C", "T", ("0/1",))], hap=3), 3, cref.SAMPLE),
    "pos_beyond_contig": (case([ln("c1", 33, "A", "G")]), 3, cref.POS),
    "pos_and_genotype_bad": (case([ln("c1", 0, "A", "G", ("?",))]), 3, cref.POS),
    "comma_in_long_alt": (case([ln("c1", 1, "A", LONG_ALT + ",T")]), 3, cref.ALLELE),
    "comma_in_long_alt_second": (case([ln("c1", 1, "A", "T," + LONG_ALT, ("2",))]), 3, cref.ALLELE),
    "two_bad_lines_earlier_wins": (case([ln("c1", 2, "C", "T"), ln("c1", 5, "A", "A7"), ln("c1", 9, "C", "T")]), 4, cref.INSERT),
    "two_reasons_ref_and_letter": (case([ln("c1", 2, "G", "C7")]), 3, cref.REF),
    "two_reasons_allele_and_ref": (case([ln("c1", 2, "G", "<DEL>")]), 3, cref.ALLELE),
    "two_reasons_ref_and_end": (case([ln("c2", 7, "G", "GT")]), 3, cref.REF),
    "two_reasons_allele_and_ref_past": (case([ln("c2", 6, "CATT", "C]c1:1]")]), 3, cref.ALLELE),
}


def ref_result(genome, spec):
    vcf, sample, hap = spec
    return cref.consensus([(c["name"], c["bases"].tobytes()) for c in genome], vcf, sample, hap)


def parse(genome, spec, device=-1):
    """[(records, pool)] per contig from the consensus parser of a context on ``device`` (-1: the host parser)."""
    vcf, sample, hap = spec
    eng = _ffi.Engine(device=device)
    try:
        cids = [eng.add_contig(c["bases"]) for c in genome]
        for cid, c in zip(cids, genome):
            eng.vcf_host_bases(cid, c["bases"])
        vcf_replay.plan_all(eng, np.frombuffer(vcf, dtype=np.uint8), [c["name"] for c in genome], cids, (sample, hap))
        return [tuple(a.copy() for a in eng.fetch_records(cid)) for cid in cids]
    finally:
        eng.close()


def refusal(genome, spec, device=-1) -> str:
    with pytest.raises((vcf_replay.VcfReplayError, ValueError)) as ei:
        parse(genome, spec, device)
    return str(ei.value)


def applied(genome, tables):
    out = []
    eng = _ffi.Engine(device=-1)
    try:
        for c, (recs, pool) in zip(genome, tables):
            res = apply_ref.apply(c["bases"], recs, pool)
            assert res.key_error is None
            out.append(res.seq.tobytes())
            eng.set_records(eng.add_contig(c["bases"]), recs, pool)       # check_record_table passes
    finally:
        eng.close()
    return out


# ------------------------------------------------------------------------------ 1. hand-written cases
@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_accepted(name):
    want = ref_result(GENOME, ACCEPTED[name])
    assert isinstance(want, list), want
    assert applied(GENOME, parse(GENOME, ACCEPTED[name])) == want


def test_reference_on_known_answers():
    """The restatement itself, on answers worked out by hand."""
    def one(name):
        return ref_result(GENOME, ACCEPTED[name])
    assert one("snv_lut_transition")[0] == b"ATGT" + C1[4:]
    assert one("ins_leading")[0] == C1[:5] + b"TT" + C1[5:]
    assert one("ins_trailing")[0] == C1[:4] + b"TT" + C1[4:]
    assert one("complex_no_anchor")[0] == C1[:4] + b"TT" + C1[7:]
    assert one("leading_anchor_on_iupac_del")[0] == C1[:23] + C1[24:]          # the R stays an R
    assert one("snv_iupac_raw_unreachable")[0] == C1[:22] + b"A" + C1[23:]
    assert one("deletion_to_last_base")[1] == b"TTGAC"
    assert one("insertion_before_base_0")[0] == b"GG" + C1
    assert one("lead_would_hit_end_uses_trailing")[1] == b"TTGACCAA"
    assert one("het_0_1_hap1")[0] == C1 and one("het_0_1_hap2")[0] == b"ATGT" + C1[4:]
    assert one("three_alts_1_2_hap2")[0] == b"AGGT" + C1[4:] and one("three_alts_third")[0] == b"ACAAGT" + C1[4:]
    assert one("skipped_genotypes")[0] == C1[:5] + b"T" + C1[6:]
    assert one("star_allele")[0] == C1[:5] + b"T" + C1[6:]
    assert one("three_samples_by_name")[0] == b"ATGT" + C1[4:] and one("three_samples_last")[0] == C1[:5] + b"TT" + C1[5:]


def test_record_shapes():
    """What the decomposition emits: an SN record where the LUT reaches ALT, a DE directly followed by an IN for a replacement."""
    SN, IN, DE = 1, 2, 3
    rows = lambda t: [tuple(r)[:5] for r in t[0].tolist()]                  # noqa: E731
    assert rows(parse(GENOME, ACCEPTED["snv_lut_transversions"])[0]) == [(1, 1, 0, SN, 1), (3, 3, 0, SN, 2)]
    recs, pool = parse(GENOME, ACCEPTED["complex_no_anchor"])[0]
    assert rows((recs,)) == [(4, 6, 0, DE, 0), (7, 8, 0, IN, 0)] and pool.tobytes() == b"TT"
    recs, pool = parse(GENOME, ACCEPTED["snv_a_to_n"])[0]
    assert rows((recs,)) == [(4, 4, 0, DE, 0), (5, 5, 0, IN, 0)] and pool.tobytes() == b"N"
    recs, pool = parse(GENOME, ACCEPTED["lower_case"])[0]
    assert rows((recs,)) == [(5, 6, 0, DE, 0), (10, 11, 0, IN, 0)] and pool.tobytes() == b"TT"
    assert [len(r) for r, _ in parse(GENOME, ACCEPTED["snv_alt_is_genome_base"])] == [1, 0]


# ------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(name):
    spec, number, reason = REFUSALS[name]
    assert ref_result(GENOME, spec) == (number, reason)
    assert refusal(GENOME, spec) == cref.message(number, reason)


def test_unknown_sample_is_named():
    with pytest.raises(vcf_replay.VcfReplayError, match="no sample column 'nobody'"):
        parse(GENOME, (ACCEPTED["three_samples_by_name"][0], "nobody", 1))


def test_select_arguments():
    eng = _ffi.Engine(device=-1)
    try:
        with pytest.raises(_ffi.MsimError):
            eng.vcf_select(1, 0, 1)                                        # before vcf_load
        eng.vcf_load(ACCEPTED["three_samples_by_name"][0])
        for bad in ((2, 0, 1), (1, 0, 0), (1, 3, 1), (0, 1, 1)):
            with pytest.raises(_ffi.MsimError):
                eng.vcf_select(*bad)
        eng.vcf_select(1, 2, 2)
        eng.vcf_select(0)
    finally:
        eng.close()


def test_dialect_unchanged_after_load():
    """msim_vcf_load selects the dialect again: a consensus-only VCF is refused as before."""
    eng = _ffi.Engine(device=-1)
    try:
        cid = eng.add_contig(GENOME[0]["bases"])
        eng.vcf_host_bases(cid, GENOME[0]["bases"])
        text = header() + ln("c1", 2, "CGT", "TAC")
        eng.vcf_load(text)
        eng.vcf_select(1, 0, 1)
        eng.vcf_plan_contig(cid, 0)
        eng.vcf_load(text)
        with pytest.raises(ValueError, match="VCF line 3: "):
            eng.vcf_plan_contig(cid, 0)
    finally:
        eng.close()


# ------------------------------------------------------------------------------ 3. the simulator's own VCFs under --consensus
def _plain_goldens():
    names = []
    for d in sorted(CASES.iterdir()):
        if (d / "expected_ms.vcf").is_file() and (d / "expected_ms.fa").is_file():
            bases = b"".join(seq for _, seq, _ in vcf_replay_ref.read_fasta(case_input_bytes(case_meta(d.name))))
            if set(bases) <= set(b"ACGTN"):
                names.append(d.name)
    return names


PLAIN_GOLDENS = _plain_goldens()


def test_enough_goldens_qualify():
    assert len(PLAIN_GOLDENS) >= 4, PLAIN_GOLDENS


@pytest.mark.parametrize("name", PLAIN_GOLDENS)
def test_golden_round_trip(name):
    fasta = case_input_bytes(case_meta(name))
    vcf = (CASES / name / "expected_ms.vcf").read_bytes()
    want = [seq for _, seq, _ in vcf_replay_ref.read_fasta((CASES / name / "expected_ms.fa").read_bytes())]
    contigs = parse_fasta_bytes(fasta)
    assert applied(contigs, parse(contigs, (vcf, None, 1))) == want
    assert ref_result(contigs, (vcf, None, 1)) == want


# ------------------------------------------------------------------------------ 4. random property test
N_RANDOM = 200
IUPAC = b"KSYMWRBDHV"


def random_lines(rs: random.Random, name: str, seq: bytes, n_samples: int, fmt: str, max_gap: int = 40):
    """Data lines for the contig ``seq``, acceptable by construction: REF spans at least two bases apart and two bases off the
    contig's end; every shape, 1-3 ALTs, random genotypes, REF bytes raw or de-ambiguated, now and then lower-case."""
    def bases(n):
        return bytes(rs.choice(b"ACGT") for _ in range(n))

    L, lines = len(seq), []
    a = rs.randint(0, 5)
    while True:
        R = rs.choice([1, 1, 1, 2, 3, rs.randint(1, 30)])
        if a + R > L - 2:
            return lines
        ref = bytes(rs.choice([g, cref.conv(g)]) for g in seq[a:a + R])
        alts = []
        for _ in range(rs.randint(1, 3)):
            shape = rs.randrange(6)
            if shape == 0:                                                 # SNV / MNP of the same length, N and the base itself included
                alt = bytes(rs.choice(b"ACGTN" + ref) for _ in range(R))
            elif shape == 1:                                               # leading anchor
                alt = ref[:1] + bases(rs.randint(0, 12))
            elif shape == 2:                                               # trailing anchor
                alt = bases(rs.randint(0, 12)) + ref[-1:]
            elif shape == 3:                                               # whatever the bytes give
                alt = bases(rs.randint(1, 12))
            elif shape == 4:
                alt = b"*"
            else:
                alt = ref[:1] + bases(rs.randint(1, 4)) + ref[-1:]
            alts.append(alt)

        def gt():
            entries = [rs.choice([".", "0"] + [str(k + 1) for k in range(len(alts))] * 3) for _ in range(rs.randint(1, 2))]
            return rs.choice("/|").join(entries) + (":7" if fmt != "GT" else "")
        if rs.random() < 0.2:
            ref, alts = ref.lower(), [x.lower() for x in alts]
        lines.append(ln(name, a + 1, ref.decode(), b",".join(alts).decode(), [gt() for _ in range(n_samples)], fmt=fmt,
                        info=rs.choice([".", "DP=9;AF=0.5"])))
        a += R + rs.randint(2, max_gap)


def random_genome_bytes(rs: random.Random, L: int) -> bytes:
    seq = bytearray(rs.choice(b"ACGT") for _ in range(L))
    for _ in range(rs.randint(0, 3)):
        at = rs.randrange(L)
        end = min(L, at + rs.randint(1, 40))
        seq[at:end] = b"N" * (end - at)
    for _ in range(rs.randint(0, L // 20)):
        seq[rs.randrange(L)] = rs.choice(IUPAC)
    return bytes(seq)


def random_case(rs: random.Random):
    """One or two contigs of 200-3 000 bases with N runs and IUPAC codes, 1-4 samples, a followed sample and a haplotype."""
    genome, lines = [], []
    n_samples = rs.randint(1, 4)
    follow, hap, fmt = rs.randrange(n_samples), rs.randint(1, 2), rs.choice(["GT", "GT:DP"])
    for ci in range(rs.randint(1, 2)):
        seq = random_genome_bytes(rs, rs.randint(200, 3000))
        genome.append({"name": f"r{ci}", "bases": np.frombuffer(seq, dtype=np.uint8)})
        lines += random_lines(rs, f"r{ci}", seq, n_samples, fmt)
    samples = tuple(f"s{k}" for k in range(n_samples))
    return genome, (header(samples) + b"".join(lines), samples[follow], hap)


def test_random_vcfs():
    rs = random.Random(20240607)
    done = changed = 0
    for _ in range(N_RANDOM):
        genome, spec = random_case(rs)
        want = ref_result(genome, spec)
        assert isinstance(want, list), want
        assert applied(genome, parse(genome, spec)) == want
        changed += want != [c["bases"].tobytes() for c in genome]
        done += 1
    assert done == N_RANDOM and changed > N_RANDOM * 3 // 4


# ------------------------------------------------------------------------------ 5. the command line
def test_sample_without_consensus_is_a_usage_error():
    for extra in (["--sample", "x"], ["--haplotype", "2"], ["--consensus", "--haplotype", "0"]):
        with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
            msa.get_args(["genome.fa", "vcf", "t.vcf"] + extra)
        assert ei.value.code == 2 and "usage:" in err.getvalue()


def test_plain_vcf_namespace_is_unchanged():
    args = msa.get_args(["-o", "out/base", "genome.fa", "vcf", "truth.vcf"])
    assert sorted(vars(args)) == sorted(["infile", "outbase", "ignore_warnings", "no_color", "no_progress", "quiet", "seed", "device",
                                         "gpus", "rng", "bgzip", "chain", "bench_json", "mode", "vcffile", "outfasta", "outvcf",
                                         "outfastait", "outbedpe", "outchain"])


def test_consensus_arguments():
    args = msa.get_args(["--chain", "genome.fa", "vcf", "calls.vcf.gz", "--consensus", "--sample", "NA12878", "--haplotype", "2"])
    assert args.consensus and args.sample == "NA12878" and args.haplotype == 2 and args.vcffile == Path("calls.vcf.gz")
    assert args.outfasta == Path("genome_ms.fa") and args.outchain == Path("genome_ms.chain")
    args = msa.get_args(["genome.fa", "vcf", "calls.vcf", "--consensus"])
    assert args.consensus and args.sample is None and args.haplotype is None
