"""CPU tier of the ``vcf`` mode: the semantics (tests/vcf_replay_ref.py) against the real reference's bytes, and libmsim's host
parser (host-only context, csrc/vcf_parse.hip) against the semantics, the renderer and ``check_record_table``.

The refusal "mutated length of 2^32 or more" needs a contig of nearly 4 GiB; it is exercised by
``test_refusal_mutated_length`` on such a contig (8 GiB of host memory for a few seconds).
"""
from __future__ import annotations

import contextlib
import glob
import io
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import apply_ref
import mutation_simulator_amd as msa
import vcf_replay_ref as ref
from helpers import CASES, case_input_bytes, case_meta, parse_fasta_bytes
from mutation_simulator_amd import _ffi, vcf_replay

ROOT = Path(__file__).resolve().parent.parent
GOLDENS = ["blocks_nondefault", "it_rmt_mutations", "readme_mix_no_tl", "readme_mix_tl", "rmt_quiet_none_std", "rmt_small",
           "snp_titv2_2ctg", "svmix_2ctg_200k", "svmix_iupac", "tiny_contigs", "titv0_dense", "tl_heavy", "tl_rmt", "warn_rmt_meta"]
SN, IN, DE, DU, IV, TL, TLI = 1, 2, 3, 4, 5, 6, 7


def _golden(name):
    meta = case_meta(name)
    return case_input_bytes(meta), (CASES / name / "expected_ms.vcf").read_bytes(), (CASES / name / "expected_ms.fa").read_bytes()


def host_parse(contigs, vcf: bytes):
    """[(records, pool)] per contig from the host parser; the engine is returned open (host-only)."""
    eng = _ffi.Engine(device=-1)
    try:
        cids = [eng.add_contig(c["bases"]) for c in contigs]
        for cid, c in zip(cids, contigs):
            eng.vcf_host_bases(cid, c["bases"])
        vcf_replay.plan_all(eng, np.frombuffer(vcf, dtype=np.uint8), [c["name"] for c in contigs], cids)
        return [tuple(a.copy() for a in eng.fetch_records(cid)) for cid in cids]
    finally:
        eng.close()


# ------------------------------------------------------------------------------ 1. the semantics, against the real reference
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_reference_fasta(name):
    fasta, vcf, want = _golden(name)
    assert ref.replay_fasta(fasta, vcf) == want


def test_anchor_rule_matters():
    """Without the anchor rule the IUPAC goldens differ: their VCF holds NON_AMBIGUOUS[base] where the genome holds a code."""
    for name in ("svmix_iupac", "tl_heavy"):
        fasta, vcf, want = _golden(name)
        by = ref.data_lines(vcf)
        plain = lambda seq, lines: ref.replay(seq, [(p, r, a, b".") for p, r, a, _ in lines])      # noqa: E731
        got = [plain(seq, by.get(head.split()[0], [])) for head, seq, _ in ref.read_fasta(fasta)]
        exp = [seq for _, seq, _ in ref.read_fasta(want)]
        assert got != exp, name


# ------------------------------------------------------------------------------ 2. the host parser on the goldens
@pytest.mark.parametrize("name", GOLDENS)
def test_host_parser_reproduces_reference_fasta(name):
    fasta, vcf, want = _golden(name)
    contigs = parse_fasta_bytes(fasta)
    tables = host_parse(contigs, vcf)
    exp = [seq for _, seq, _ in ref.read_fasta(want)]
    n_lines = sum(len(v) for v in ref.data_lines(vcf).values())
    assert sum(len(r) for r, _ in tables) == n_lines                      # one record per line
    eng = _ffi.Engine(device=-1)
    try:
        for c, (recs, pool), e in zip(contigs, tables, exp):
            res = apply_ref.apply(c["bases"], recs, pool)
            assert res.key_error is None and res.seq.tobytes() == e, (name, c["name"])
            eng.set_records(eng.add_contig(c["bases"]), recs, pool)       # check_record_table passes
    finally:
        eng.close()


# ------------------------------------------------------------------------------ 3. inverse of the renderer
def _conv(b):
    return apply_ref.NON_AMBIGUOUS[b]


def canonical(recs, pool, bases):
    """What the parser must give back for the VCF text of this table: suppressed records dropped, TL -> DE, a non-empty TLI ->
    IN with literal bytes; a trailing-anchor line whose first byte equals the anchor reads as a leading-anchor one (the tie
    rule: leading where it gives a valid record), i.e. one position further with the bytes rotated."""
    L = len(bases)
    rows, out_pool = [], bytearray()

    def insert(pos, ins, trailing):
        ins = bytes(ins)
        if trailing and ins[:1] == bytes([_conv(bases[pos])]) and pos + 1 < L:
            pos, ins = pos + 1, ins[1:] + bytes([_conv(bases[pos])])
        rows.append((pos, pos + len(ins) - 1, len(out_pool), IN, 0, 0))
        out_pool.extend(ins)

    for pos, stop, extra, typ, aux in zip(recs["pos"].tolist(), recs["stop"].tolist(), recs["extra"].tolist(), recs["type"].tolist(),
                                          recs["aux"].tolist()):
        if typ == SN:
            r = int(_conv(bases[pos]))
            alt = int(apply_ref.TRANSITIONS[r]) if aux == 0 else ord(apply_ref.TRANSVERSIONS[chr(r)][aux - 1])
            if alt != r:
                rows.append((pos, pos, 0, SN, aux, 0))
        elif typ == IN:
            insert(pos, pool[extra:extra + stop + 1 - pos].tobytes(), trailing=pos == 0)
        elif typ in (DE, TL):
            if pos == 0 and _conv(bases[0]) == _conv(bases[stop + 1]):    # position-0 form that also reads as a leading one
                pos, stop = 1, stop + 1
            rows.append((pos, stop, 0, DE, 0, 0))
        elif typ == IV:
            seg = _conv(bases[pos:stop + 1])
            if seg.tobytes() != apply_ref.COMPLEMENT[seg][::-1].tobytes():
                rows.append((pos, stop, 0, IV, 0, 0))
        elif typ == DU:
            rows.append((pos, stop, 0, DU, 0, 0))
        else:
            seg = _conv(bases[extra:stop + 1])
            if len(seg):
                insert(pos, apply_ref.COMPLEMENT[seg[::-1]] if aux & 1 else seg, trailing=not aux & 2)
    return np.array(rows, dtype=_ffi.RECORD_DTYPE), np.frombuffer(bytes(out_pool), dtype=np.uint8)


def _roundtrip(contigs, tables):
    vcf = b"##fileformat=VCFv4.3\n#CHROM\tPOS\n" + b"".join(
        _ffi.render_vcf(recs, pool, c["bases"], c["name"]) for c, (recs, pool) in zip(contigs, tables))
    got = host_parse(contigs, vcf)
    for c, (recs, pool), (g_recs, g_pool) in zip(contigs, tables, got):
        w_recs, w_pool = canonical(recs, pool, c["bases"])
        assert g_recs.tobytes() == w_recs.tobytes() and g_pool.tobytes() == w_pool.tobytes(), c["name"]
        a, b = apply_ref.apply(c["bases"], recs, pool), apply_ref.apply(c["bases"], g_recs, g_pool)
        if b"N" not in c["bases"].tobytes() and set(c["bases"].tobytes()) <= set(b"ACGT"):
            assert a.seq.tobytes() == b.seq.tobytes()                     # (exact where no suppressed record changes a byte)
    return got


def _table(*rows):
    return np.array([tuple(r) + (0,) * (6 - len(r)) for r in rows], dtype=_ffi.RECORD_DTYPE)


def test_inverse_of_renderer_hand_built():
    bases = np.frombuffer(b"ACGTTGCANNRYACGTAGCTAGGATCCTTAAGCGCGATATCCGGAATTCAGTCAGTC", dtype=np.uint8)
    L = len(bases)
    pool = np.frombuffer(b"GGTTACA", dtype=np.uint8)
    tables = [
        _table((0, 2, 0, IN), (3, 3, 0, SN, 1), (5, 8, 3, IN), (9, 9, 0, SN), (12, 15, 0, IV), (20, 25, 0, DU), (30, 33, 0, DE),
               (40, 41, 0, TL), (44, 41, 40, TLI, 3), (50, L - 1, 0, DE)),                   # position-0 insert, N SNP, clamped deletion
        _table((0, 4, 0, DE), (10, 10, 0, SN, 2), (22, 27, 0, IV), (30, 31, 0, TL), (36, 31, 30, TLI, 0)),   # position-0 deletion
        _table((0, 0, 0, IN), (2, 5, 1, IN)),                                                # insert "A" before "A": reads as leading
    ]
    for t in tables:
        _roundtrip([{"name": "h1", "bases": bases}], [(t, pool)])


@pytest.mark.parametrize("name", ["svmix_iupac", "tl_heavy", "svmix_2ctg_200k", "readme_mix_tl"])
def test_inverse_of_renderer_planner_tables(name):
    from test_apply_ref_host import _plan_host
    meta = case_meta(name)
    contigs = parse_fasta_bytes(case_input_bytes(meta))
    _, tables = _plan_host(meta["argv_tail"], contigs, meta["seed_py"], meta["seed_np"])
    empty = (np.zeros(0, dtype=_ffi.RECORD_DTYPE), np.zeros(0, dtype=np.uint8))
    _roundtrip(contigs, [tables.get(i, empty) for i in range(len(contigs))])


# ------------------------------------------------------------------------------ 4. refusals
GENOME = [{"name": "c1", "bases": np.frombuffer(b"ACGTACGTAGCTAGCTNNACGTRYACGTACGT", dtype=np.uint8)},
          {"name": "c2", "bases": np.frombuffer(b"TTGACCA", dtype=np.uint8)}]
HDR = b"##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tx\n"     # lines 1-2


def line(chrom, pos, ref, alt, info=".", fmt="GT", sample="1", extra=""):
    return f"{chrom}\t{pos}\t.\t{ref}\t{alt}\t.\t.\t{info}\t{fmt}\t{sample}{extra}\n".encode()


def sv(kind, end=1, length=1):
    return f"SVTYPE={kind};END={end};SVLEN={length}"


OK1 = line("c1", 2, "C", "T")
REFUSALS = {
    # name: (lines behind the header, offending line number, text the reason must hold)
    "nine_fields": ([OK1, b"c1\t5\t.\tA\tG\t.\t.\t.\tGT\n"], 4, "other than 10"),
    "eleven_fields": ([OK1, line("c1", 5, "A", "G", extra="\t1")], 4, "other than 10"),
    "stray_tab_in_ref": ([line("c1", 5, "AC\tGT", "A", sv("DEL"))], 3, "other than 10"),
    "empty_line": ([OK1, b"\n"], 4, "no contig"),
    "pos_not_a_number": ([line("c1", "x7", "T", "C")], 3, "POS"),
    "pos_zero": ([line("c1", 0, "A", "G")], 3, "POS"),
    "pos_beyond_contig": ([line("c1", 33, "A", "G")], 3, "POS"),
    "unknown_chrom": ([OK1, line("c9", 1, "A", "G")], 4, "no contig"),
    "not_contiguous": ([OK1, line("c2", 1, "T", "C"), line("c1", 6, "C", "T")], 5, "not contiguous"),
    "positions_decrease": ([line("c1", 6, "C", "T"), line("c1", 2, "C", "T")], 4, "earlier line consumed"),
    "positions_equal": ([OK1, OK1], 4, "earlier line consumed"),
    "inside_a_deletion": ([line("c1", 4, "TACG", "T", sv("DEL")), line("c1", 6, "C", "T")], 4, "earlier line consumed"),
    "snp_ref_mismatch": ([line("c1", 2, "G", "A")], 3, "REF does not match"),
    "del_ref_mismatch": ([line("c1", 4, "TACC", "T", sv("DEL"))], 3, "REF does not match"),
    "del_ref_past_contig": ([line("c2", 6, "CAT", "C", sv("DEL"))], 3, "REF does not match"),
    "inv_ref_mismatch": ([line("c1", 1, "ACGA", "TCGT", sv("INV"))], 3, "REF does not match"),
    "dup_ref_is_raw_input": ([line("c1", 21, "GTAC", "GTACGTAC", sv("DUP"))], 3, "REF does not match"),     # the genome holds GTRY
    "inv_alt_not_revcomp": ([line("c1", 1, "ACGT", "ACGA", sv("INV"))], 3, "ALT is not what"),
    "dup_alt_not_twice": ([line("c1", 1, "ACGT", "ACGTACGA", sv("DUP"))], 3, "ALT is not what"),
    "dup_alt_wrong_length": ([line("c1", 1, "ACGT", "ACGTACG", sv("DUP"))], 3, "ALT is not what"),
    "ins_without_anchor": ([line("c1", 2, "C", "GGG", sv("INS"))], 3, "ALT is not what"),
    "del_without_anchor": ([line("c1", 1, "ACG", "C", sv("DEL"))], 3, "ALT is not what"),
    "snp_two_bases": ([line("c1", 2, "CG", "TA")], 3, "ALT is not what"),
    "multi_allelic": ([line("c1", 2, "C", "T,G")], 3, "multi-allelic"),
    "multi_allelic_long": ([line("c1", 1, "ACGTACGTAGCTAGCTNNAC", "ACGTACGTAG,TAGCTNNACA", sv("DUP"))], 3, "multi-allelic"),
    "symbolic": ([line("c1", 4, "T", "<DEL>", sv("DEL"))], 3, "symbolic"),
    "breakend": ([line("c1", 4, "T", "T[c2:3[", sv("INS"))], 3, "breakend"),
    "svtype_bnd": ([line("c1", 4, "T", "TA", sv("BND"))], 3, "SVTYPE"),
    "svtype_cnv": ([line("c1", 4, "T", "TA", "SVTYPE=CNV")], 3, "SVTYPE"),
    "info_other": ([line("c1", 4, "T", "C", "DP=3")], 3, "SVTYPE"),
    "sample_0": ([line("c1", 2, "C", "T", sample="0")], 3, "GT and 1"),
    "sample_diploid": ([line("c1", 2, "C", "T", sample="0/1")], 3, "GT and 1"),
    "format_other": ([line("c1", 2, "C", "T", fmt="GT:DP", sample="1:3")], 3, "GT and 1"),
    "snp_alt_unreachable": ([line("c1", 2, "C", "N")], 3, "SNP ALT"),
    "snp_alt_equals_ref": ([line("c1", 2, "C", "C")], 3, "SNP ALT"),
    "insert_digit": ([line("c1", 2, "C", "CA7T", sv("INS"))], 3, "no letter"),
    "insert_tab_count": ([line("c1", 2, "C", "CA-T", sv("INS:ME"))], 3, "no letter"),
    "truncated_last_line": ([OK1, b"c1\t9\t.\tA\tG\t."], 4, "other than 10"),
}


def _refusal(lines):
    eng = _ffi.Engine(device=-1)
    try:
        cids = [eng.add_contig(c["bases"]) for c in GENOME]
        for cid, c in zip(cids, GENOME):
            eng.vcf_host_bases(cid, c["bases"])
        with pytest.raises((vcf_replay.VcfReplayError, ValueError)) as ei:
            vcf_replay.plan_all(eng, np.frombuffer(HDR + b"".join(lines), dtype=np.uint8), [c["name"] for c in GENOME], cids)
        # the context is usable afterwards
        vcf_replay.plan_all(eng, np.frombuffer(HDR + OK1, dtype=np.uint8), [c["name"] for c in GENOME], cids)
        assert eng.fetch_records(cids[0])[0]["pos"].tolist() == [1]
        return str(ei.value)
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(name):
    lines, number, reason = REFUSALS[name]
    msg = _refusal(lines)
    assert msg.startswith(f"VCF line {number}: ") and reason in msg, msg


def test_refusal_is_value_error_code():
    eng = _ffi.Engine(device=-1)
    try:
        cid = eng.add_contig(GENOME[0]["bases"])
        eng.vcf_host_bases(cid, GENOME[0]["bases"])
        eng.vcf_load(HDR + line("c1", 2, "G", "A"))
        assert eng.lib.msim_vcf_plan_contig(eng.h, cid, 0) == _ffi.ERR_VALUE
        assert eng.lib.msim_last_error(eng.h).decode() == "VCF line 3: REF does not match the genome"
    finally:
        eng.close()


def test_refusal_mutated_length():
    """A contig of 2^32 - 50 bases and a duplication of 60: 2^32 + 10."""
    L = (1 << 32) - 50
    bases = np.full(L, ord("A"), dtype=np.uint8)
    eng = _ffi.Engine(device=-1)
    try:
        cid = eng.add_contig(bases)
        eng.vcf_host_bases(cid, bases)
        del bases
        eng.vcf_load(HDR + line("big", 5, "A" * 60, "A" * 120, sv("DUP", 64, 60)))
        with pytest.raises(ValueError, match=r"VCF line 3: mutated length of 2\^32 or more"):
            eng.vcf_plan_contig(cid, 0)
    finally:
        eng.close()


def test_accepted_edge_cases():
    """Header only, empty file, a contig without lines, a last line without terminator, both anchor forms."""
    for vcf in (HDR, b""):
        assert [len(r) for r, _ in host_parse(GENOME, vcf)] == [0, 0]
    got = host_parse(GENOME, HDR + line("c2", 1, "T", "GGT", sv("INS", 1, 2)) + line("c2", 3, "G", "GAA", sv("INS", 3, 2))
                     + line("c2", 4, "ACC", "A", sv("DEL", 6, 2))[:-1])
    assert len(got[0][0]) == 0
    recs, pool = got[1]
    assert [tuple(r)[:4] for r in recs.tolist()] == [(0, 1, 0, IN), (3, 4, 2, IN), (4, 5, 0, DE)] and pool.tobytes() == b"GGAA"
    assert apply_ref.apply(GENOME[1]["bases"], recs, pool).seq.tobytes() == b"GGTTGAAAA"


# ------------------------------------------------------------------------------ 5. the command line
def test_argument_parsing():
    args = msa.get_args(["-o", "out/base", "--bgzip", "genome.fa", "vcf", "truth.vcf.gz"])
    assert args.mode == "vcf" and args.vcffile == Path("truth.vcf.gz") and args.infile == Path("genome.fa")
    assert args.outfasta == Path("out/base_ms.fa.gz")
    assert msa.get_args(["genome.fa", "vcf", "t.vcf"]).outfasta == Path("genome_ms.fa")
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        msa.get_args(["genome.fa", "vcf"])


def test_gpus_refused(tmp_path):
    from mutation_simulator_amd import __main__ as cli
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">c1\nACGT\n")
    err = io.StringIO()
    state = (random.getstate(), np.random.get_state()[1].tobytes())
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        cli.main(["-c", "--gpus", "2", str(fa), "vcf", str(tmp_path / "t.vcf")])
    assert ei.value.code not in (0, None) and "single-GPU" in err.getvalue()
    assert not (tmp_path / "g_ms.fa").exists()
    assert (random.getstate(), np.random.get_state()[1].tobytes()) == state


# ------------------------------------------------------------------------------ 6. the host parser under ASan + UBSan
ASAN_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(root)r + "/mutation-simulator_amd", %(root)r + "/tests", %(root)r + "/tests/golden"]
import numpy as np
import test_vcf_replay_host as t
for name in t.GOLDENS:
    fasta, vcf, want = t._golden(name)
    t.host_parse(t.parse_fasta_bytes(fasta), vcf)
for name in sorted(t.REFUSALS):
    t._refusal(t.REFUSALS[name][0])
fasta, vcf, _ = t._golden("svmix_iupac")
contigs = t.parse_fasta_bytes(fasta)
rs = np.random.RandomState(7)
body = vcf[vcf.index(b"\n#CHROM"):]
for cut in rs.randint(1, len(body), 200).tolist():                       # truncated and garbled texts: refused or accepted, never a bad read
    text = bytearray(body[:cut])
    for at in rs.randint(0, cut, 3).tolist():
        text[at] = int(rs.randint(0, 256))
    try:
        t.host_parse(contigs, bytes(text))
    except (t.vcf_replay.VcfReplayError, ValueError):
        pass
print("SANITIZED-OK")
"""


def test_host_parser_under_asan_ubsan():
    r = subprocess.run(["make", "-C", str(ROOT / "mutation-simulator_amd" / "csrc"), "asan"], capture_output=True, text=True)
    lib = ROOT / "mutation-simulator_amd" / "lib_asan" / "libmsim.so"
    assert r.returncode == 0 and lib.exists(), r.stderr[-2000:]
    rts = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so")
    assert rts, "clang ASan runtime not found"
    env = dict(os.environ, MSIM_LIB=str(lib), LD_PRELOAD=rts[0], ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sys.executable, "-c", ASAN_CHILD % {"root": str(ROOT)}], capture_output=True, text=True, env=env,
                       timeout=1200, cwd=str(ROOT))
    assert "SANITIZED-OK" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
