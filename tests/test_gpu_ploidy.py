"""``--ploidy 2`` on the device: the genotype draw (``k_gt_draw``), the haplotype selection (``k_hap_count``, ``k_scan_u32``,
``k_hap_compact``), APPLY of the selected tables, the phased VCF text (``k_vcf_lines`` / ``k_vcf_plain`` with a genotype column)
and the command line.  All comparisons are exact.

References: numpy's filter of the record table, ``apply_ref`` (the plain restatement of the reference's rewrite loop) on the
filtered table, ``ploidy_twin`` (the draw's rules over ``fast_twin``'s Philox), ``msim_render_vcf_gt`` (the host renderer),
``msim_render_chain`` and, end to end, what ``vcf --consensus --haplotype h`` makes of the diploid VCF.
"""
from __future__ import annotations

import contextlib
import io
import random

import numpy as np
import pytest

import apply_ref
import ploidy_twin
from helpers import case_input_bytes, case_meta, parse_fasta_bytes
from mutation_simulator_amd import _ffi
from test_gpu_apply_tables import ACGT, Table, make_bases, random_table
from test_ploidy_host import phased_text, vcf_table

pytestmark = pytest.mark.gpu

B = 1024                       # records of a workgroup of k_hap_count / k_hap_compact (haplotype.hip: HAP_BLOCK): 16 runs of 64
COUNTS = [0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1]
PATTERNS = ["all3", "all1", "all2", "alternating", "random", "edges_off_h1", "edges_off_h2"]


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def pattern(name, n, seed=5):
    """all1: haplotype 2 is empty; edges_off_h*: every block's first and last record is missing from haplotype *."""
    idx = np.arange(n)
    if name in ("all1", "all2", "all3"):
        return np.full(n, int(name[-1]), dtype=np.uint8)
    if name == "alternating":
        return (1 + (idx & 1)).astype(np.uint8)
    gt = np.random.RandomState(seed).randint(1, 4, n).astype(np.uint8)
    if name.startswith("edges_off"):
        gt[:] = 3
        gt[(idx % B == 0) | (idx % B == B - 1) | (idx == n - 1)] = 2 if name.endswith("h1") else 1
    return gt


def snp_table(n, seed):
    """n SNP records, one every 3..5 bases."""
    L = 5 * n + 64
    tab = Table(make_bases(L, seed), seed=seed)
    for _ in range(n):
        tab.add(apply_ref.SN, tab.at + 2 + int(tab.rs.randint(0, 3)), aux=int(tab.rs.randint(0, 3)))
    return tab.done()


def test_block_size_is_the_kernels():
    assert _ffi.hap_block() == B


# ------------------------------------------------------------------------------ 1. the selection: the active table
@pytest.mark.parametrize("n", COUNTS)
def test_selected_table_equals_the_numpy_filter(eng, n):
    bases, recs, pool = snp_table(n, 100 + n)
    assert len(recs) == n
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, recs, pool)
    for name in PATTERNS:
        gt = pattern(name, n)
        eng.set_genotypes(cid, gt)
        assert np.array_equal(eng.fetch_genotypes(cid, n), gt)
        for hap in (1, 2):
            eng.select_haplotype(cid, hap)
            want = recs[(gt & hap) != 0]
            got, _ = eng.fetch_records(cid)
            assert eng.result_sizes(cid, applied=False)[1] == len(want), (name, hap)
            assert got.tobytes() == want.tobytes(), (name, hap)
        eng.select_haplotype(cid, 0)
        assert eng.fetch_records(cid)[0].tobytes() == recs.tobytes(), name
    eng.clear()


def test_selection_needs_genotypes(eng):
    bases, recs, pool = snp_table(65, 3)
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, recs, pool)
    with pytest.raises(_ffi.MsimError):
        eng.select_haplotype(cid, 1)
    with pytest.raises(_ffi.MsimError):
        eng.set_genotypes(cid, np.zeros(65, dtype=np.uint8))
    eng.set_genotypes(cid, np.full(65, 3, dtype=np.uint8))
    eng.select_haplotype(cid, 2)
    eng.set_records(cid, recs, pool)                       # a new table: the selection and the genotypes are gone
    assert len(eng.fetch_records(cid)[0]) == 65
    with pytest.raises(_ffi.MsimError):
        eng.select_haplotype(cid, 1)
    eng.clear()


# ------------------------------------------------------------------------------ 2. APPLY of a haplotype, 3. the full table again
@pytest.fixture(scope="module")
def big_tables():
    """A ~200 kb IUPAC contig with about 3 000 records of all seven types, and an SNP-only table; each with the reference's
    result for the full table."""
    sv = random_table(200_000, 21, "large_window")
    snp = random_table(120_000, 22, "snp_only")
    assert set(np.unique(sv[1]["type"]).tolist()) == {1, 2, 3, 4, 5, 6, 7} and 2 * B < len(sv[1]) < 6000
    assert len(snp[1]) > B and (snp[1]["type"] == apply_ref.SN).all()
    return {"sv": (sv, apply_ref.apply(*sv)), "snp": (snp, apply_ref.apply(*snp))}


def applied(eng, cid, want):
    eng.apply_contig(cid)
    assert eng.result_sizes(cid)[0] == want.out_len
    got = eng.fetch_sequence(cid)
    assert np.array_equal(got, want.seq), int(np.flatnonzero(got != want.seq)[0]) if len(got) == len(want.seq) else (len(got), len(want.seq))
    assert eng.key_error(cid) is None


@pytest.mark.parametrize("which", ["sv", "snp"])
@pytest.mark.parametrize("name", PATTERNS)
def test_apply_of_each_haplotype(eng, big_tables, which, name):
    (bases, recs, pool), full = big_tables[which]
    gt = pattern(name, len(recs), seed=9)
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, recs, pool, with_offsets=which == "sv" and name == "random")   # (offsets that came with the full table are no haplotype's)
    eng.set_genotypes(cid, gt)
    for hap in (1, 2):
        eng.select_haplotype(cid, hap)
        sub = recs[(gt & hap) != 0]
        want = full if len(sub) == len(recs) else apply_ref.apply(bases, sub, pool)
        applied(eng, cid, want)
        if len(sub) == 0:
            assert np.array_equal(want.seq, bases)                          # an empty haplotype: the input
        assert eng.fetch_sequence_framed(cid, 60).tobytes().replace(b"\n", b"") == want.seq.tobytes()
        assert eng.render_chain_device(cid, "c", "c", 3).tobytes() == _ffi.render_chain(sub, len(bases), "c", "c", 3)
    eng.select_haplotype(cid, 0)
    assert eng.fetch_records(cid)[0].tobytes() == recs.tobytes()
    applied(eng, cid, full)
    eng.clear()


# ------------------------------------------------------------------------------ the genotype draw
@pytest.fixture(scope="module")
def linked():
    return ploidy_twin.linked_table(5000, 11, 250_000)


@pytest.mark.parametrize("key,seq,het_thr", ploidy_twin.DRAW_CASES)
def test_device_draw_equals_the_twin(eng, linked, key, seq, het_thr):
    recs, pool, pairs, unlinked = linked
    eng.clear()
    cid = eng.add_contig(ACGT[np.arange(250_000) & 3].copy())
    eng.set_records(cid, recs, pool)
    eng.genotype_contig(cid, key, seq, het_thr)
    ploidy_twin.check_draw(eng.fetch_genotypes(cid, len(recs)), recs, pairs, unlinked, key, seq, het_thr)
    eng.clear()


# ------------------------------------------------------------------------------ the VCF text
def test_device_text_of_a_genotyped_contig(eng, big_tables, monkeypatch):
    cases = [vcf_table(), big_tables["sv"][0], big_tables["snp"][0]]
    for k, (bases, recs, pool) in enumerate(cases):
        eng.clear()
        cid = eng.add_contig(bases)
        eng.set_records(cid, recs, pool)
        plain = _ffi.render_vcf(recs, pool, bases, "chrT")
        assert eng.render_vcf_device(cid, "chrT").tobytes() == plain         # no genotypes: today's text
        gt = pattern("random", len(recs), seed=40 + k)
        eng.set_genotypes(cid, gt)
        want = _ffi.render_vcf_gt(recs, gt, pool, bases, "chrT")
        assert want != plain and len(want) == len(plain) + 2 * plain.count(b"\n")
        if k == 0:
            by_record, suppressed = phased_text(recs, gt, pool, bases, "chrT")
            assert want == by_record and suppressed == 3
        assert eng.render_vcf_device(cid, "chrT").tobytes() == want
        eng.select_haplotype(cid, 1)                                         # the text is the full table's, whichever is active
        assert eng.render_vcf_device(cid, "chrT").tobytes() == want
        eng.select_haplotype(cid, 0)
        if k < 2:                                                            # the per-lane path (k_vcf_plain) takes the column too
            monkeypatch.setenv("MSIM_DBG_VCF_PLAIN", "1")
            assert eng.render_vcf_device(cid, "chrT").tobytes() == want
            monkeypatch.delenv("MSIM_DBG_VCF_PLAIN")
        eng.set_records(cid, recs, pool)                                     # a new table: haploid text again
        assert eng.render_vcf_device(cid, "chrT").tobytes() == plain
    eng.clear()


# ------------------------------------------------------------------------------ the command line
SEED = 7
SV = ["-sn", "0.002", "-in", "0.002", "-de", "0.002", "-iv", "0.002", "-du", "0.002"]
CONFIGS = {
    "snp": ([], ["args", "-sn", "0.01"]),
    "all_six": ([], ["args"] + SV + ["-tl", "0.002"]),
    "snp_fast": (["--rng", "fast"], ["args", "-sn", "0.01"]),
    "five_fast": (["--rng", "fast"], ["args"] + SV),
}
LETTERS = np.frombuffer(b"KSYMWRBDHVN", dtype=np.uint8)


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """Three contigs of about 500 kb (line widths 60 / 70 / 61), the second with IUPAC codes and N runs.

    The codes are few on purpose.  ``vcf --consensus`` keeps the one base REF and ALT share as the genome has it (README: the
    mode's anchor rule), the mutation pass writes an inversion's whole span de-ambiguated: where an inversion's first or last
    base is an ambiguity code AND its REF and ALT agree there, the consensus of the simulator's own VCF differs from the
    simulator's Fasta in that one byte -- haploid or diploid alike.  1 000 inversions per contig put about 0.1 % of a contig's
    positions at such a place, so 48 codes leave that to chance at a few percent per seed (``haploid`` asserts that it did not
    happen for SEED); with a code every 13 bases no seed would pass.  N converts to itself and is free of this: the N runs
    (about 6 000 bases) are where transversions are suppressed and the genotype has to be indexed by record, not by line.
    Dense ambiguity codes under every record type are test_apply_of_each_haplotype's."""
    d = tmp_path_factory.mktemp("ploidy")
    rs = np.random.RandomState(99)
    out = []
    for i, (L, bpl) in enumerate([(500_000, 60), (500_009, 70), (499_993, 61)]):
        seq = ACGT[rs.randint(0, 4, L)].copy()
        if i == 1:
            for s in rs.randint(0, L - 300, 40):
                seq[s:s + int(rs.randint(1, 300))] = ord("N")
            at = np.unique(rs.randint(0, L, 48))
            seq[at] = LETTERS[rs.randint(0, len(LETTERS), len(at))]
        raw = seq.tobytes()
        out.append(b">ctg%d part %d\n" % (i + 1, i) + b"".join(raw[k:k + bpl] + b"\n" for k in range(0, L, bpl)))
    (d / "g.fa").write_bytes(b"".join(out))
    return d


def run_cli(argv, expect=0):
    from mutation_simulator_amd import __main__ as msa_main
    err = io.StringIO()
    code = 0
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        try:
            msa_main.main(["-q", "-c"] + [str(a) for a in argv])
        except SystemExit as e:
            code = e.code
    assert code in ((0, None) if expect == 0 else (expect,)), err.getvalue()
    return generator_states()


def generator_states():
    """The states of ``random`` and ``numpy.random`` as what they stand for: the next 1 400 words of each stream.  The tuples of
    ``getstate()`` / ``get_state()`` themselves depend on which PLAN engine handed the state back -- the host planner (the haploid
    run batches these contigs) leaves CPython's block-aligned array and an index, a device engine the 624 words in front of the
    position with index 624 (plan_gpu.hip: gpu_plan_sync_to_host; either is a valid state of the same generator) -- and a diploid
    run goes contig by contig, so it may meet another engine than the haploid run of the same flags."""
    r = random.Random()
    r.setstate(random.getstate())
    rs = np.random.RandomState()
    rs.set_state(np.random.get_state())
    return tuple(r.getrandbits(32) for _ in range(1400)), rs.bytes(4 * 1400)


def haploid_tail(vcf: bytes, gt: bytes = b"1") -> bytes:
    """The VCF with every data line's sample column replaced by ``gt``."""
    out = []
    for line in vcf.split(b"\n"):
        if line and not line.startswith(b"#"):
            head, fmt, _ = line.rsplit(b"\t", 2)
            assert fmt == b"GT"
            line = head + b"\tGT\t" + gt
        out.append(line)
    return b"\n".join(out)


_HAPLOID: dict = {}


def haploid(genome, config):
    """The haploid run of a configuration (once per module): its files, the generators' states behind it -- and, the precondition
    of the consensus check, that ``vcf --consensus`` takes this seed's haploid VCF and gives the haploid Fasta."""
    if config not in _HAPLOID:
        d = genome / config
        d.mkdir(exist_ok=True)
        extra, tail = CONFIGS[config]
        states = run_cli(["--seed", SEED, *extra, "-o", d / "hap", genome / "g.fa", *tail])
        fa, vcf = (d / "hap_ms.fa").read_bytes(), (d / "hap_ms.vcf").read_bytes()
        run_cli(["-o", d / "pre", genome / "g.fa", "vcf", d / "hap_ms.vcf", "--consensus"])
        assert (d / "pre_ms.fa").read_bytes() == fa, "vcf --consensus does not reproduce the HAPLOID run of this seed: choose another"
        _HAPLOID[config] = (fa, vcf, states)
    return _HAPLOID[config]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_cli_het_0_is_the_haploid_run_twice(genome, config, tmp_path):
    fa, vcf, states = haploid(genome, config)
    extra, tail = CONFIGS[config]
    got = run_cli(["--seed", SEED, "--ploidy", "2", "--het", "0", *extra, "-o", tmp_path / "d", genome / "g.fa", *tail])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["d_ms.vcf", "d_ms_h1.fa", "d_ms_h2.fa"]
    assert (tmp_path / "d_ms_h1.fa").read_bytes() == fa and (tmp_path / "d_ms_h2.fa").read_bytes() == fa
    assert (tmp_path / "d_ms.vcf").read_bytes() == haploid_tail(vcf, b"1|1")
    assert got == states                                                   # neither generator noticed


@pytest.mark.parametrize("config", list(CONFIGS))
def test_cli_het_1_has_no_homozygous_line(genome, config, tmp_path):
    _, vcf, states = haploid(genome, config)
    extra, tail = CONFIGS[config]
    got = run_cli(["--seed", SEED, "--ploidy", "2", "--het", "1", *extra, "-o", tmp_path / "d", genome / "g.fa", *tail])
    text = (tmp_path / "d_ms.vcf").read_bytes()
    assert b"1|1" not in text and b"\tGT\t1|0\n" in text and b"\tGT\t0|1\n" in text
    assert haploid_tail(text) == vcf and got == states


@pytest.mark.parametrize("config", list(CONFIGS))
def test_cli_het_half(genome, config, tmp_path, monkeypatch):
    fa, vcf, states = haploid(genome, config)
    extra, tail = CONFIGS[config]
    seen = []
    draw = _ffi.Engine.genotype_contig

    def spy(self, contig, key, seq, het_thr):
        draw(self, contig, key, seq, het_thr)
        recs, pool = self.fetch_records(contig)
        seen.append((self.read_contig(contig), recs, pool, self.fetch_genotypes(contig, len(recs)), key, seq, het_thr))
    monkeypatch.setattr(_ffi.Engine, "genotype_contig", spy)
    got = run_cli(["--seed", SEED, "--ploidy", "2", "--chain", *extra, "-o", tmp_path / "d", genome / "g.fa", *tail])
    monkeypatch.undo()
    assert got == states
    assert sorted(p.name for p in tmp_path.iterdir()) == ["d_ms.vcf", "d_ms_h1.chain", "d_ms_h1.fa", "d_ms_h2.chain", "d_ms_h2.fa"]
    text = (tmp_path / "d_ms.vcf").read_bytes()
    assert haploid_tail(text) == vcf
    assert all(text.count(b"\tGT\t" + g + b"\n") > 100 for g in (b"1|0", b"0|1", b"1|1"))
    assert len(seen) == 3 and [s[5] for s in seen] == [0, 1, 2] and len({s[4] for s in seen}) == 1
    assert all(s[6] == ploidy_twin.ceil_scaled(0.5) for s in seen)
    for bases, recs, pool, gt, key, seq, thr in seen:                       # the run's genotypes are the twin's
        assert np.array_equal(gt, ploidy_twin.genotypes(recs, key, seq, thr))
    names = [b"ctg1", b"ctg2", b"ctg3"]
    for hap in (1, 2):
        out = (tmp_path / f"d_ms_h{hap}.fa").read_bytes()
        contigs = parse_fasta_bytes(out)
        assert len(contigs) == 3
        chains = []
        for k, (bases, recs, pool, gt, *_) in enumerate(seen):
            sub = recs[(gt & hap) != 0]
            want = apply_ref.apply(bases, sub, pool)
            assert contigs[k]["name"].encode() == names[k] and np.array_equal(contigs[k]["bases"], want.seq), (hap, k)
            chain = _ffi.render_chain(sub, len(bases), names[k].decode(), names[k].decode(), k + 1)
            assert int(chain.split(b"\n", 1)[0].split()[8]) == want.out_len        # qSize: the haplotype's contig
            chains.append(chain)
        assert (tmp_path / f"d_ms_h{hap}.chain").read_bytes() == b"".join(chains)
        run_cli(["-o", tmp_path / f"c{hap}", genome / "g.fa", "vcf", tmp_path / "d_ms.vcf", "--consensus", "--haplotype", hap])
        assert (tmp_path / f"c{hap}_ms.fa").read_bytes() == out, hap
    assert (tmp_path / "d_ms_h1.fa").read_bytes() != (tmp_path / "d_ms_h2.fa").read_bytes() != fa


def test_key_error_is_the_haploid_runs(tmp_path):
    meta = case_meta("err_snp_on_U")
    infile = tmp_path / meta["infile_name"]
    infile.write_bytes(case_input_bytes(meta))
    raised = []
    for extra in ([], ["--ploidy", "2"], ["--ploidy", "2", "--het", "1"]):
        random.seed(meta["seed_py"])
        np.random.seed(meta["seed_np"])
        with pytest.raises(KeyError) as e:
            run_cli([*extra, "-o", tmp_path / f"o{len(raised)}", infile, *meta["argv_tail"]])
        raised.append(repr(e.value.args[0]))
    assert raised == [meta["exception"]["repr_args"][0]] * 3
