"""``--ploidy 2`` on the CPU tier: the host-only restatements behind ``msim_genotype_contig`` / ``msim_select_haplotype``, the
host VCF renderer with a genotype column (``msim_render_vcf_gt``) and the command line.  All comparisons are exact.

* the genotype draw against the numpy twin (``tests/ploidy_twin.py``: written from the rules over ``fast_twin``'s Philox);
* the haplotype selection against numpy's ``recs[gt & h != 0]``, its chain against ``chain_ref``;
* the phased VCF text against ``msim_render_vcf``'s lines with their tails replaced by record;
* the parser's names and every refusal.
"""
from __future__ import annotations

import contextlib
import io
from pathlib import Path

import numpy as np
import pytest

import chain_ref
import ploidy_twin
from apply_ref import DE, DU, IN, IV, SN, TL, TLI
from helpers import CASES, case_input_bytes, case_meta
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import argument_parser as ap

L = 250_000
N_REC = 5000


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(-1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def table():
    return ploidy_twin.linked_table(N_REC, 11, L)


def install(eng, recs, pool, length=L):
    eng.clear()
    cid = eng.add_contig(np.zeros(length, dtype=np.uint8))
    eng.set_records(cid, recs, pool)
    return cid


def test_symbols_exist():
    lib = _ffi.load()
    for name in ("msim_genotype_contig", "msim_set_genotypes", "msim_fetch_genotypes", "msim_select_haplotype", "msim_render_vcf_gt"):
        assert hasattr(lib, name)
    assert lib.msim_abi_version() == 8


@pytest.mark.parametrize("key,seq,het_thr", ploidy_twin.DRAW_CASES)
def test_genotype_draw_equals_the_twin(eng, table, key, seq, het_thr):
    recs, pool, pairs, unlinked = table
    assert len(recs) == N_REC and len(pairs) >= 40
    cid = install(eng, recs, pool)
    eng.genotype_contig(cid, key, seq, het_thr)
    ploidy_twin.check_draw(eng.fetch_genotypes(cid, len(recs)), recs, pairs, unlinked, key, seq, het_thr)


def test_draw_depends_on_key_and_contig(table):
    recs = table[0]
    thr = ploidy_twin.ceil_scaled(0.5)
    a = ploidy_twin.genotypes(recs, 1, 0, thr)
    assert not np.array_equal(a, ploidy_twin.genotypes(recs, 2, 0, thr))
    assert not np.array_equal(a, ploidy_twin.genotypes(recs, 1, 1, thr))
    assert 0.4 < (a != 3).mean() < 0.6 and 0.4 < (a[a != 3] == 1).mean() < 0.6


def test_genotype_argument_checks(eng, table):
    recs, pool = table[0], table[1]
    cid = install(eng, recs, pool)
    with pytest.raises(_ffi.MsimError):
        eng.fetch_genotypes(cid, len(recs))                 # none yet
    with pytest.raises(_ffi.MsimError):
        eng.select_haplotype(cid, 1)                        # selecting without genotypes
    eng.select_haplotype(cid, 0)                            # (the full table is the full table)
    with pytest.raises(_ffi.MsimError):
        eng.genotype_contig(cid, 1, 0, ploidy_twin.TWO53 + 1)
    for bad in (0, 4, 255):
        gt = np.full(len(recs), 3, dtype=np.uint8)
        gt[len(recs) // 2] = bad
        with pytest.raises(_ffi.MsimError):
            eng.set_genotypes(cid, gt)
    eng.set_genotypes(cid, np.full(len(recs), 2, dtype=np.uint8))
    with pytest.raises(_ffi.MsimError):
        eng.select_haplotype(cid, 3)
    eng.set_records(cid, recs, pool)                        # a new table drops the genotypes
    with pytest.raises(_ffi.MsimError):
        eng.fetch_genotypes(cid, len(recs))


@pytest.mark.parametrize("pattern", ["random", "all3", "all1", "all2", "alternating"])
def test_selection_equals_the_numpy_filter(eng, table, pattern):
    recs, pool = table[0], table[1]
    n = len(recs)
    gt = {"random": np.random.RandomState(3).randint(1, 4, n), "all3": np.full(n, 3), "all1": np.full(n, 1), "all2": np.full(n, 2),
          "alternating": 1 + (np.arange(n) & 1)}[pattern].astype(np.uint8)
    cid = install(eng, recs, pool)
    eng.set_genotypes(cid, gt)
    for hap in (1, 2, 2, 1, 0):
        eng.select_haplotype(cid, hap)
        want = recs[(gt & hap) != 0] if hap else recs
        got, got_pool = eng.fetch_records(cid)
        assert eng.result_sizes(cid, applied=False)[1:] == (len(want), len(pool))
        assert got.tobytes() == want.tobytes() and np.array_equal(got_pool, pool), (pattern, hap)
        assert (got["rsv"] == 0).all()
        assert _ffi.render_chain(got, L, "chrT", "chrT", 5) == chain_ref.render(want, L, "chrT", "chrT", 5)
        assert np.array_equal(eng.fetch_genotypes(cid, n), gt)          # (the full table's, whichever is selected)


def vcf_table():
    """Records of every type with lines of their own, among them records whose line is suppressed: a transversion of N, an
    inversion of a reverse-complement palindrome, a TLI with an empty span."""
    bases = np.frombuffer(b"ACGTTGCAAC" * 40, dtype=np.uint8).copy()
    bases[50:54] = np.frombuffer(b"ACGT", dtype=np.uint8)               # its own reverse complement
    bases[70] = ord("N")
    bases[90] = ord("R")
    rows = [(0, 2, 0, IN, 0, 0), (10, 10, 0, SN, 0, 0), (20, 24, 0, DE, 0, 0), (30, 30, 0, SN, 2, 0), (40, 44, 0, DU, 0, 0),
            (50, 53, 0, IV, 0, 0),                                      # suppressed
            (60, 66, 0, IV, 0, 0), (70, 70, 0, SN, 1, 0),               # N -> N: suppressed
            (80, 80, 0, SN, 1, 0), (90, 90, 0, SN, 0, 0), (100, 109, 0, TL, 0, 0), (120, 109, 100, TLI, 3, 0),
            (130, 99, 100, TLI, 2, 0),                                  # empty span: suppressed
            (140, 143, 3, IN, 0, 0), (150, 150, 0, SN, 0, 0)]
    recs = np.array(rows, dtype=_ffi.RECORD_DTYPE).reshape(-1)
    return bases, recs, np.frombuffer(b"GATTACA", dtype=np.uint8).copy()


def phased_text(recs, gt, pool, bases, name):
    """``msim_render_vcf``'s lines, record by record, each line's tail replaced from the genotype of the record that made it."""
    out, suppressed = [], 0
    for i in range(len(recs)):
        line = _ffi.render_vcf(recs[i:i + 1], pool, bases, name)
        if not line:
            suppressed += 1
            continue
        assert line.endswith(b"\tGT\t1\n") and line.count(b"\n") == 1
        out.append(line[:-2] + b"%d|%d\n" % (gt[i] & 1, (gt[i] >> 1) & 1))
    return b"".join(out), suppressed


def test_phased_vcf_text():
    bases, recs, pool = vcf_table()
    plain = _ffi.render_vcf(recs, pool, bases, "chr1")
    assert _ffi.render_vcf_gt(recs, None, pool, bases, "chr1") == plain
    for seed in range(4):
        gt = np.random.RandomState(seed).randint(1, 4, len(recs)).astype(np.uint8)
        want, suppressed = phased_text(recs, gt, pool, bases, "chr1")
        assert suppressed == 3
        got = _ffi.render_vcf_gt(recs, gt, pool, bases, "chr1")
        assert got == want
        assert len(got) == len(plain) + 2 * plain.count(b"\n")
    gt = np.full(len(recs), 3, dtype=np.uint8)
    gt[4] = 0
    with pytest.raises(_ffi.MsimError) as e:
        _ffi.render_vcf_gt(recs, gt, pool, bases, "chr1")
    assert e.value.code == _ffi.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_names():
    a = ap.get_args(["--ploidy", "2", "genome.fa", "args", "-sn", "0.01"])
    assert a.ploidy == 2 and a.het == 0.5
    assert (a.outfasta_h1, a.outfasta_h2, a.outvcf) == (Path("genome_ms_h1.fa"), Path("genome_ms_h2.fa"), Path("genome_ms.vcf"))
    assert (a.outchain_h1, a.outchain_h2) == (Path("genome_ms_h1.chain"), Path("genome_ms_h2.chain"))
    a = ap.get_args(["--ploidy", "2", "--het", "0.25", "--chain", "-o", "out/base", "asm.fasta", "rmt", "x.rmt"])
    assert a.het == 0.25 and a.chain
    assert (str(a.outfasta_h1), str(a.outfasta_h2), str(a.outvcf)) == ("out/base_ms_h1.fasta", "out/base_ms_h2.fasta", "out/base_ms.vcf")
    assert (str(a.outchain_h1), str(a.outchain_h2)) == ("out/base_ms_h1.chain", "out/base_ms_h2.chain")
    a = ap.get_args(["genome.fa", "args", "-sn", "0.01"])                # the default changes nothing
    assert a.ploidy == 1 and a.het is None and not hasattr(a, "outfasta_h1") and a.outfasta == Path("genome_ms.fa")
    assert ap.ploidy_refusal(a) is None
    for het in ("0", "1"):
        assert ap.get_args(["--ploidy", "2", "--het", het, "genome.fa", "args"]).het == float(het)


@pytest.mark.parametrize("extra", [["--het", "0.5"], ["--ploidy", "1", "--het", "0.5"], ["--ploidy", "2", "--het", "1.5"],
                                   ["--ploidy", "2", "--het", "-0.1"], ["--ploidy", "2", "--het", "nan"], ["--ploidy", "3"]])
def test_usage_errors(extra):
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
        ap.get_args(extra + ["genome.fa", "args", "-sn", "0.01"])
    assert ei.value.code == 2 and "usage:" in err.getvalue()


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


def test_refused_with_it_mode(monkeypatch, tmp_path):
    meta = case_meta("it_only_4ctg")
    infile = tmp_path / meta["infile_name"]
    infile.write_bytes(case_input_bytes(meta))
    _refused(monkeypatch, ["-c", "--ploidy", "2", "-o", str(tmp_path / "out"), str(infile), "it", "0.5"],
             "--ploidy 2 does not apply to the interchromosomal pass (it)")
    assert not list(tmp_path.glob("out*"))


def test_refused_with_it_lines_in_rmt(monkeypatch, tmp_path):
    meta = case_meta("it_rmt_mutations")
    infile = tmp_path / meta["infile_name"]
    infile.write_bytes(case_input_bytes(meta))
    rmt = tmp_path / "case.rmt"
    rmt.write_text((CASES / "it_rmt_mutations" / "case.rmt").read_text())
    _refused(monkeypatch, ["-c", "--ploidy", "2", "-o", str(tmp_path / "out"), str(infile), "rmt", str(rmt)],
             "--ploidy 2 does not apply to the interchromosomal pass (it lines in the RMT)")
    assert not list(tmp_path.glob("out*"))


def test_refused_with_vcf_mode(monkeypatch, tmp_path):
    _refused(monkeypatch, ["-c", "--ploidy", "2", "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "vcf", str(tmp_path / "t.vcf")],
             "--ploidy 2 does not apply to the vcf mode")
    assert not list(tmp_path.glob("out*"))


def test_refused_with_several_gpus(monkeypatch, tmp_path):
    _refused(monkeypatch, ["-c", "--ploidy", "2", "--gpus", "2", "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "args", "-sn", "0.01"],
             "--ploidy 2 needs a single-GPU run (--gpus 1)")
    assert not list(tmp_path.glob("out*"))


def test_refused_with_bgzip(monkeypatch, tmp_path):
    _refused(monkeypatch, ["-c", "--ploidy", "2", "--bgzip", "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "args", "-sn", "0.01"],
             "a third BGZF output channel, which is a follow-up")
    assert not list(tmp_path.glob("out*"))


def test_refusal_messages():
    ns = ap.get_args(["--ploidy", "2", "genome.fa", "args", "-sn", "0.01"])
    assert ap.ploidy_refusal(ns) is None and "it lines in the RMT" in ap.ploidy_refusal(ns, has_it=True)
