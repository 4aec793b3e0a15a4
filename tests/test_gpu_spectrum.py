"""``--spectrum`` on the device: the trinucleotide census (``k_ctx_census``), the per-site sampler (``k_spectrum_draw``,
``k_scan_u32``, ``k_spectrum_emit``), APPLY of its tables and the command line.  All comparisons are exact.

References: ``spectrum_twin`` (the engine's rules in numpy over ``fast_twin``'s Philox), ``vcf_ref.snp_text`` (the VCF lines
of an SNP table) and, end to end, what the ``vcf`` mode makes of the files a run wrote.
"""
from __future__ import annotations

import contextlib
import gzip
import io
import random

import numpy as np
import pytest

import spectrum_twin as tw
import vcf_ref
from helpers import parse_fasta_bytes
from mutation_simulator_amd import _ffi

pytestmark = pytest.mark.gpu

T = _ffi.SPECTRUM_TILE
LENGTHS = [0, 1, 2, 3, 15, 16, 17, T - 1, T, T + 1, 2 * T + 1]
KEY = 0xF00DFACE12345678


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fast_eng():
    e = _ffi.Engine(0, _ffi.RNG_FAST)
    yield e
    e.close()


def genome(L, seed):
    return tw.random_genome(np.random.RandomState(seed), L)


def test_tile_is_the_headers():
    header = (__import__("pathlib").Path(__file__).resolve().parent.parent / "include" / "msim.h").read_text()
    assert f"#define MSIM_SPECTRUM_TILE {T}\n" in header and T % 16 == 0


# ------------------------------------------------------------------------------ 1. census
def check_census(eng, bases):
    eng.clear()
    cid = eng.add_contig(bases)
    counts, n_valid = eng.context_counts(cid)
    want, want_n = tw.census(bases)
    assert counts.dtype == np.uint64 and np.array_equal(counts, want), np.flatnonzero(counts != want)
    assert n_valid == want_n
    return cid


@pytest.mark.parametrize("L", LENGTHS)
def test_census_lengths(eng, L):
    check_census(eng, genome(L, 300 + L))
    eng.clear()


@pytest.mark.parametrize("at", [T - 1, T, T + 1])
def test_census_n_at_the_tile_edge(eng, at):
    """An N invalidates the site on either side of it: across the tile edge that is the halo's doing."""
    bases = genome(2 * T + 1, 7)
    clean = tw.census(bases)[1]
    bases[at] = ord("N")
    check_census(eng, bases)
    assert tw.census(bases)[1] == clean - 3
    eng.clear()


def test_census_iupac_rich_and_long(eng):
    rs = np.random.RandomState(8)
    check_census(eng, tw.random_genome(rs, 300_000, n_runs=30, iupac=20_000))
    homopolymer = np.full(5 * T + 3, ord("A"), dtype=np.uint8)         # every lane of every wave adds to one bin
    check_census(eng, homopolymer)
    eng.clear()


def test_census_beyond_one_tile_per_workgroup(eng):
    """The census's grid stops at 2048 workgroups; a longer contig (here 8.4 Mb: one tile more) is strided over."""
    check_census(eng, tw.random_genome(np.random.RandomState(12), 2048 * T + T + 5, n_runs=5, iupac=1000))
    eng.clear()


def test_census_two_contigs_resident(eng):
    eng.clear()
    a, b = genome(T + 5, 1), tw.random_genome(np.random.RandomState(2), 3 * T - 7, n_runs=3, iupac=50)
    ca, cb = eng.add_contig(a), eng.add_contig(b)
    for cid, bases in ((cb, b), (ca, a), (cb, b)):
        counts, n = eng.context_counts(cid)
        want, want_n = tw.census(bases)
        assert np.array_equal(counts, want) and n == want_n
    eng.clear()


# ------------------------------------------------------------------------------ 2. the plan against the twin
def check_plan(eng, bases, thr, key=KEY, seq=0, cid=None):
    if cid is None:
        eng.clear()
        cid = eng.add_contig(bases)
    eng.plan_contig_spectrum(cid, thr, key, seq)
    want = tw.plan(bases, thr, key, seq)
    assert eng.result_sizes(cid, applied=False)[1:] == (len(want), 0)
    recs, pool = eng.fetch_records(cid)
    assert len(pool) == 0
    for field in ("pos", "stop", "extra", "type", "aux", "rsv"):
        assert np.array_equal(recs[field], want[field]), (field, np.flatnonzero(recs[field] != want[field])[:8])
    assert eng.plan_was_empty(cid) == (len(want) == 0)
    return cid, recs


@pytest.mark.parametrize("L", LENGTHS)
def test_every_site_table(eng, L):
    """Maximum density: every wave and tile boundary carries a hit on both sides."""
    bases = genome(L, 500 + L)
    _, recs = check_plan(eng, bases, tw.every_site_table())
    assert len(recs) == max(0, L - 2)
    eng.clear()


@pytest.mark.parametrize("L", [0, 3, T + 1])
def test_all_zero_table_is_an_empty_plan(eng, L):
    cid, recs = check_plan(eng, genome(L, 9), np.zeros(192, dtype=np.uint64))
    assert len(recs) == 0 and eng.plan_was_empty(cid)
    if L:
        eng.apply_contig(cid)                                          # an empty table applies to the input
        assert np.array_equal(eng.fetch_sequence(cid), genome(L, 9))
    eng.clear()


def test_one_hot_context_at_the_tile_edges(eng):
    """CCC occurs exactly at T - 1, T and 2T - 1 of an all-A contig and is the only context that mutates."""
    bases = np.full(2 * T + 1, ord("A"), dtype=np.uint8)
    bases[T - 2:T + 2] = ord("C")
    bases[2 * T - 2:2 * T + 1] = ord("C")
    ccc = 16 + 4 + 1
    pos, ctx = tw.sites(bases)
    assert pos[ctx == ccc].tolist() == [T - 1, T, 2 * T - 1]
    thr = np.zeros((64, 3), dtype=np.uint64)
    thr[ccc] = np.array([1 << 62, 1 << 63, (1 << 64) - 1], dtype=np.uint64)
    _, recs = check_plan(eng, bases, thr.reshape(-1))
    assert recs["pos"].tolist() == [T - 1, T, 2 * T - 1]
    eng.clear()


@pytest.mark.parametrize("density", [1e-4, 1e-2, 0.25])
def test_random_tables(eng, density):
    rs = np.random.RandomState(int(density * 1e4) + 1)
    bases = tw.random_genome(rs, 250_000 + int(rs.randint(0, 4000)), n_runs=10, iupac=100)
    _, recs = check_plan(eng, bases, tw.random_table(rs, density), key=KEY ^ 0x55, seq=12)
    assert 0.4 * density * len(bases) < len(recs) < 1.6 * density * len(bases)
    eng.clear()


def test_contig_number_changes_the_table_and_a_repeat_does_not(eng):
    eng.clear()
    bases = genome(3 * T + 100, 21)
    thr = tw.random_table(np.random.RandomState(3), 0.05)
    ca, cb = eng.add_contig(bases), eng.add_contig(bases)
    _, ra = check_plan(eng, bases, thr, seq=0, cid=ca)
    _, rb = check_plan(eng, bases, thr, seq=1, cid=cb)
    assert ra.tobytes() != rb.tobytes()
    _, again = check_plan(eng, bases, thr, seq=0, cid=ca)
    assert again.tobytes() == ra.tobytes()
    assert eng.fetch_records(cb)[0].tobytes() == rb.tobytes()          # the other contig's table is untouched
    eng.clear()


def test_refusals_and_timing(eng):
    eng.clear()
    eng.reset_stats()
    assert eng.spectrum_timing() == (0.0, 0.0)
    bases = genome(T + 9, 4)
    cid = eng.add_contig(bases)
    bad = tw.every_site_table().copy()
    bad[3 * 6 + 2] = 7
    with pytest.raises(_ffi.MsimError, match="context 6 are not non-decreasing") as e:
        eng.plan_contig_spectrum(cid, bad, KEY, 0)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError):
        eng.plan_contig_spectrum(cid + 1, tw.every_site_table(), KEY, 0)
    eng.context_counts(cid)
    check_plan(eng, bases, tw.every_site_table(), cid=cid)
    census_ms, plan_ms = eng.spectrum_timing()
    assert 0 < census_ms < 1000 and 0 < plan_ms < 1000
    eng.reset_stats()
    assert eng.spectrum_timing() == (0.0, 0.0)
    eng.clear()


# ------------------------------------------------------------------------------ 3. plan + APPLY in the library
@pytest.mark.parametrize("density", [1e-2, 0.25])
@pytest.mark.parametrize("which", ["compat", "fast"])
def test_planned_contig_applies_to_the_twins_bases(eng, fast_eng, which, density):
    e = eng if which == "compat" else fast_eng
    rs = np.random.RandomState(31)
    bases = tw.random_genome(rs, 200_000 + 77, n_runs=8, iupac=60)
    thr = tw.random_table(rs, density)
    cid, recs = check_plan(e, bases, thr, seq=5)
    e.apply_contig(cid)
    assert e.result_sizes(cid)[0] == len(bases)
    want = tw.apply(bases, recs)
    got = e.fetch_sequence(cid)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert (got != bases).sum() == len(recs)                            # every record changes its base
    assert e.key_error(cid) is None
    text = e.render_vcf_device(cid, "c").tobytes()
    assert text == vcf_ref.snp_text(bases, recs, "c")
    assert e.render_chain_device(cid, "c", "c", 1).tobytes() == _ffi.render_chain(recs, len(bases), "c", "c", 1)
    e.clear()


# ------------------------------------------------------------------------------ 4. the command line
SEED = 5
RATE = 0.02
NAMES = [b"ctg1", b"tiny", b"ctg3"]
BPL = [60, 60, 71]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Three contigs: 150 kb with an N run and a few ambiguity codes, one of 2 bases, 90 001 bases; and the skewed spectrum."""
    d = tmp_path_factory.mktemp("spectrum")
    rs = np.random.RandomState(42)
    seqs = [tw.random_genome(rs, 150_000, n_runs=1, iupac=12), np.frombuffer(b"AC", dtype=np.uint8), tw.random_genome(rs, 90_001)]
    seqs[0][70_000:70_500] = ord("N")
    out = []
    for name, seq, bpl in zip(NAMES, seqs, BPL):
        raw = seq.tobytes()
        out.append(b">" + name + b" some description\n" + b"".join(raw[k:k + bpl] + b"\n" for k in range(0, len(raw), bpl)))
    (d / "g.fa").write_bytes(b"".join(out))
    (d / "s.tsv").write_text("Type\tSBSa\tSBSb\n" + "".join(f"{c}\t{w!r}\t0.5\n" for c, w in zip(tw.CHANNELS, tw.skewed_weights())))
    (d / "spike.csv").write_text("".join(f"{c},{1.0 if c == 'A[C>T]G' else 1e-6}\n" for c in tw.CHANNELS))
    return d, seqs


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
    return err.getvalue()


def twin_run(seqs):
    """What the run must write: per contig the twin's table under the run's key (the first 64 bits of ``random.seed(SEED)``) and
    the contig's number, the bases with it applied, its VCF lines."""
    key = random.Random(SEED).getrandbits(64)
    fasta, vcf, tables = [], [], []
    for k, (name, seq, bpl) in enumerate(zip(NAMES, seqs, BPL)):
        counts, _ = tw.census(seq)
        recs = tw.plan(seq, tw.thresholds(counts, tw.skewed_weights(), RATE), key, k)
        raw = tw.apply(seq, recs).tobytes()
        fasta.append(b">" + name + b" some description\n" + b"".join(raw[q:q + bpl] + b"\n" for q in range(0, len(raw), bpl)))
        vcf.append(vcf_ref.snp_text(seq, recs, name))
        tables.append(recs)
    text = b"".join(fasta)
    if len(seqs[-1]) % BPL[-1]:                                         # (the writer ends no partial last line)
        text = text[:-1]
    return text, b"".join(vcf), tables


def data_lines(vcf: bytes):
    lines = vcf.split(b"\n")
    head = [l for l in lines if l.startswith(b"#")]
    return b"\n".join(head), b"".join(l + b"\n" for l in lines if l and not l.startswith(b"#"))


def spectrum_argv(d, out, *extra):
    return ["--seed", SEED, "--rng", "fast", *extra, "-o", out, d / "g.fa", "args", "-sn", RATE, "--spectrum", d / "s.tsv"]


def test_cli_equals_the_twin_and_replays(files, tmp_path):
    d, seqs = files
    want_fa, want_vcf, tables = twin_run(seqs)
    assert len(tables[0]) > 2000 and len(tables[1]) == 0 and len(tables[2]) > 1200
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, *spectrum_argv(d, tmp_path / "o")])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bench.json", "o_ms.fa", "o_ms.vcf"]
    assert (tmp_path / "o_ms.fa").read_bytes() == want_fa
    head, body = data_lines((tmp_path / "o_ms.vcf").read_bytes())
    assert body == want_vcf
    import json
    bench = json.loads(stats.read_text())
    assert bench["census_ms"] > 0 and bench["spectrum_plan_ms"] > 0
    # the header is the one every args run writes, and the vcf mode reads the file back
    run_cli(["--bench-json", stats, "--seed", SEED, "--rng", "fast", "-o", tmp_path / "p", d / "g.fa", "args", "-sn", RATE])
    assert data_lines((tmp_path / "p_ms.vcf").read_bytes())[0] == head
    assert "census_ms" not in json.loads(stats.read_text())
    run_cli(["-o", tmp_path / "r", d / "g.fa", "vcf", tmp_path / "o_ms.vcf"])
    assert (tmp_path / "r_ms.fa").read_bytes() == want_fa
    # --signature picks the other column: constant weights, another table
    run_cli([*spectrum_argv(d, tmp_path / "s"), "--signature", "SBSb"])
    assert (tmp_path / "s_ms.fa").read_bytes() != want_fa


def test_cli_bgzip_decompresses_to_the_same_bytes(files, tmp_path):
    d, seqs = files
    want_fa, want_vcf, _ = twin_run(seqs)
    run_cli(spectrum_argv(d, tmp_path / "z", "--bgzip"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["z_ms.fa.gz", "z_ms.vcf.gz"]
    assert gzip.decompress((tmp_path / "z_ms.fa.gz").read_bytes()) == want_fa
    assert data_lines(gzip.decompress((tmp_path / "z_ms.vcf.gz").read_bytes()))[1] == want_vcf


def test_cli_diploid_with_chains(files, tmp_path):
    d, seqs = files
    _, want_vcf, tables = twin_run(seqs)
    run_cli(spectrum_argv(d, tmp_path / "d", "--ploidy", "2", "--chain"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["d_ms.vcf", "d_ms_h1.chain", "d_ms_h1.fa", "d_ms_h2.chain", "d_ms_h2.fa"]
    text = (tmp_path / "d_ms.vcf").read_bytes()
    plain = b"".join(l.rsplit(b"\t", 1)[0] + b"\t1\n" for l in data_lines(text)[1].splitlines())
    assert plain == want_vcf                                            # the haploid run's lines, phased
    assert all(text.count(b"\tGT\t" + g + b"\n") > 100 for g in (b"1|0", b"0|1", b"1|1"))
    for hap in (1, 2):
        out = (tmp_path / f"d_ms_h{hap}.fa").read_bytes()
        assert [c["name"].encode() for c in parse_fasta_bytes(out)] == NAMES
        assert (tmp_path / f"d_ms_h{hap}.chain").stat().st_size > 0
        run_cli(["-o", tmp_path / f"c{hap}", d / "g.fa", "vcf", tmp_path / "d_ms.vcf", "--consensus", "--haplotype", hap])
        assert (tmp_path / f"c{hap}_ms.fa").read_bytes() == out, hap
    assert (tmp_path / "d_ms_h1.fa").read_bytes() != (tmp_path / "d_ms_h2.fa").read_bytes()


def test_cli_refuses_a_rate_the_contig_cannot_carry(files, tmp_path):
    d, _ = files
    """All the weight on A[C>T]G: at -sn 0.05 the ACG and CGT sites, a thirty-second of the contig, would have to mutate 1.6
    times each."""
    err = run_cli(["--seed", SEED, "--rng", "fast", "-o", tmp_path / "x", d / "g.fa", "args", "-sn", "0.05", "--spectrum", d / "spike.csv"],
                  expect=1)
    assert "ERROR:" in err and "would mutate with probability" in err and ("context ACG" in err or "context CGT" in err)
