"""The ``profile`` mode on the device: ``msim_sbs_counts`` (csrc/spectrum.hip: ``k_sbs_count``) on hand-built and planned
record tables, and the command line.  Every case is held against ``sbs_twin`` (the rules in numpy) AND against the library's
sequential restatement (``_ffi.sbs_counts_host``); all comparisons are exact integers.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import sbs_twin as st
import spectrum_twin as tw
from mutation_simulator_amd import _ffi, spectrum
from test_gpu_sampler import _params, _snp_range
from test_gpu_spectrum import NAMES, RATE, SEED, data_lines, files, run_cli, spectrum_argv, twin_run  # noqa: F401  (files: a fixture)

pytestmark = pytest.mark.gpu

B = _ffi.SBS_PASS
CASES = st.small_cases(B)
KEY = 0x5B5_96_C0FFEE


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def same(got, want, what):
    assert got[0].dtype == np.uint64 and got[0].shape == (96,) and got[1].shape == (8,)
    assert np.array_equal(got[0], want[0]), (what, np.flatnonzero(got[0] != want[0])[:8])
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])


def check_counts(eng, cid, bases, recs):
    """The device's counts of contig ``cid`` against the twin and the host restatement over (bases, recs)."""
    got = eng.sbs_counts(cid)
    same(got, st.counts(bases, recs), "twin")
    same(got, _ffi.sbs_counts_host(bases, recs), "host restatement")
    assert int(got[0].sum()) + int(got[1][0]) == int(got[1][1])
    return got


def check_table(eng, bases, recs, pool=st.NO_POOL):
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, recs, pool)
    return cid, check_counts(eng, cid, bases, recs)


# ------------------------------------------------------------------------------ 1-5. the small shapes
@pytest.mark.parametrize("case", sorted(CASES))
def test_small_shapes(eng, case):
    bases, recs, pool = CASES[case]
    _, (c, t) = check_table(eng, bases, recs, pool)
    if case.startswith("short_"):                                      # only L = 3, p = 1 has a channel
        assert int(c.sum()) == (1 if len(bases) == 3 else 0) and int(t[1]) == len(bases)
    if case.startswith("non_acgt_"):
        assert int(c.sum()) == 0 and t.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    if case.startswith("every_type_"):
        assert (t[1:] > 0).all() and int(c.sum()) > 0
    eng.clear()


def test_every_context_and_every_channel(eng):
    """(ctx, aux) lands in CHANNEL_OF for every pair; the three tables together give each channel exactly 2."""
    bases = st.de_bruijn()
    pos, ctx = tw.sites(bases)
    total = np.zeros(96, dtype=np.uint64)
    for aux in range(3):
        _, (c, t) = check_table(eng, bases, st.every_context()[f"every_context_aux{aux}"][1])
        want = np.bincount([spectrum.CHANNEL_OF[x][aux] for x in ctx.tolist()], minlength=96)
        assert np.array_equal(c, want.astype(np.uint64)) and int(t[0]) == 0
        total += c
    assert (total == 2).all()
    eng.clear()


def test_empty_table_and_refusals(eng):
    eng.clear()
    eng.reset_stats()
    assert eng.sbs_timing() == 0.0
    bases = tw.random_genome(np.random.RandomState(1), 500)
    cid = eng.add_contig(bases)
    with pytest.raises(_ffi.MsimError, match="contig has not been planned") as e:
        eng.sbs_counts(cid)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(_ffi.MsimError):
        eng.sbs_counts(cid + 1)
    eng.set_records(cid, st.snp_table([], 0), st.NO_POOL)
    c, t = eng.sbs_counts(cid)
    assert not c.any() and not t.any() and eng.sbs_timing() == 0.0    # nothing was launched
    eng.set_records(cid, st.snp_table([7, 9], 1), st.NO_POOL)
    check_counts(eng, cid, bases, st.snp_table([7, 9], 1))
    assert 0 < eng.sbs_timing() < 1000
    eng.release_result(cid)
    with pytest.raises(_ffi.MsimError, match="contig has not been planned"):
        eng.sbs_counts(cid)
    eng.reset_stats()
    assert eng.sbs_timing() == 0.0
    eng.clear()


# ------------------------------------------------------------------------------ 6. one-channel and flat tables
def test_one_channel_table(eng):
    """2^20 + 1 records, all of them A[C>T]G: a narrow shared counter or a racy final reduction loses some."""
    bases, recs, pool = st.one_channel()
    _, (c, t) = check_table(eng, bases, recs, pool)
    assert int(c[tw.CHANNELS.index("A[C>T]G")]) == st.ONE_CHANNEL_N == int(c.sum()) and t.tolist()[:2] == [0, st.ONE_CHANNEL_N]
    eng.clear()


def test_flat_table_of_the_same_size(eng):
    eng.clear()
    bases = tw.random_genome(np.random.RandomState(5), st.ONE_CHANNEL_N + 2)
    cid = eng.add_contig(bases)
    eng.plan_contig_spectrum(cid, tw.every_site_table(), KEY, 0)
    recs, _ = eng.fetch_records(cid)
    assert len(recs) == st.ONE_CHANNEL_N
    c, _ = check_counts(eng, cid, bases, recs)
    assert int(c.min()) > 5000
    eng.clear()


# ------------------------------------------------------------------------------ 7. applied contigs and haplotypes
def test_applied_contig_and_selected_haplotypes(eng):
    bases, recs, pool = CASES["every_type_size_mixed_2049"]
    cid, before = check_table(eng, bases, recs, pool)
    eng.apply_contig(cid)
    assert not np.array_equal(eng.fetch_sequence(cid), bases)
    same(check_counts(eng, cid, bases, recs), before, "applied")       # the context is the reference's
    gt = (np.arange(len(recs)) % 3 + 1).astype(np.uint8)
    eng.set_genotypes(cid, gt)
    for hap in (1, 2, 0):
        eng.select_haplotype(cid, hap)
        active, _ = eng.fetch_records(cid)
        want = recs if hap == 0 else recs[(gt & hap) != 0]
        assert active.tobytes() == want.tobytes()
        got = check_counts(eng, cid, bases, active)
        assert int(got[1][1:].sum()) == len(want)
    same(eng.sbs_counts(cid), before, "full table again")
    eng.clear()


# ------------------------------------------------------------------------------ 8. across the planners
def test_tables_of_the_planners():
    rs = np.random.RandomState(17)
    bases = tw.random_genome(rs, 300_000 + 11, n_runs=6, iupac=300)
    L = len(bases)
    for flags, label in ((0, "compat"), (_ffi.RNG_FAST, "fast")):
        eng = _ffi.Engine(0, flags)
        try:
            eng.seed(42, 42)
            eng.set_params(_params(titv=2.0))
            if flags:
                eng.set_fast_key(KEY)
            cid = eng.add_contig(bases)
            eng.plan_contig(cid, [_snp_range(0, L - 1, 3000)])
            recs, _ = eng.fetch_records(cid)
            assert len(recs) == 3000 and (recs["type"] == 1).all(), label
            c, t = check_counts(eng, cid, bases, recs)
            assert int(c.sum()) > 2500 and int(t[0]) > 0, label        # (some fall into the N runs)
            # the same contig planned again by the context-dependent engine
            counts, _ = eng.context_counts(cid)
            eng.plan_contig_spectrum(cid, spectrum.thresholds(counts, tw.skewed_weights(), 0.01), KEY, 0)
            recs, _ = eng.fetch_records(cid)
            c, t = check_counts(eng, cid, bases, recs)
            assert int(t[0]) == 0 and int(c.sum()) == len(recs) > 2000, label      # it draws at eligible sites only
        finally:
            eng.close()


# ------------------------------------------------------------------------------ 9. the command line
def safe_parse(text, name):
    try:
        return spectrum.parse(text, name)
    except spectrum.SpectrumError as e:
        return str(e)


def columns_of(path):
    """{column name: uint64[96], or the parser's refusal for an all-zero column}"""
    text = path.read_text()
    names = [l for l in text.splitlines() if not l.startswith("#")][0].split("\t")[1:]
    out = {}
    for n in names:
        got = safe_parse(text, n)
        out[n] = got if isinstance(got, str) else np.array([int(v) for v in got], dtype=np.uint64)
    return text, out


def test_cli_profile_of_a_spectrum_run(files, tmp_path):  # noqa: F811
    d, seqs = files
    _, _, tables = twin_run(seqs)
    want = [st.counts(seq, recs) for seq, recs in zip(seqs, tables)]
    total = sum(w[0] for w in want)
    run_cli(spectrum_argv(d, tmp_path / "o"))
    stats = tmp_path / "bench.json"
    run_cli(["--bench-json", stats, "-o", tmp_path / "p", d / "g.fa", "profile", tmp_path / "o_ms.vcf", "--per-contig"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bench.json", "o_ms.fa", "o_ms.vcf", "p_ms.sbs96.tsv"]
    text, cols = columns_of(tmp_path / "p_ms.sbs96.tsv")
    assert list(cols) == ["profile"] + [n.decode() for n in NAMES]
    assert np.array_equal(cols["profile"], total) and int(total.sum()) == sum(len(t) for t in tables)
    assert np.array_equal(cols["ctg1"], want[0][0]) and np.array_equal(cols["ctg3"], want[2][0])
    assert "all 96 weights are zero" in cols["tiny"]                   # a contig of two bases holds no SNP
    assert np.array_equal(cols["ctg1"] + cols["ctg3"], cols["profile"])
    # the comment lines: the tallies, and the opportunities of the whole genome
    n_sn = int(total.sum())
    assert f"# records: SN {n_sn}, no context 0, IN 0, DE 0, DU 0, IV 0, TL 0, TLI 0" in text.splitlines()
    census = sum(tw.census(seq)[0] for seq in seqs)
    opp = [l.split(" ")[2:] for l in text.splitlines() if l.startswith("# opportunities ")]
    assert len(opp) == 32
    for name, n in opp:
        ctx = 16 * "ACGT".index(name[0]) + 4 * "ACGT".index(name[1]) + "ACGT".index(name[2])
        assert int(n) == int(census[ctx]) + int(census[tw.rc(ctx)])
    bench = json.loads(stats.read_text())
    assert bench["vcf_bytes"] == (tmp_path / "o_ms.vcf").stat().st_size and bench["sbs_kernel_ms"] > 0 and bench["census_ms"] > 0
    assert {"vcf_load_kernel_ms", "vcf_plan_kernel_ms", "cli_s"} <= set(bench)
    # without --per-contig, under another name: one column
    run_cli(["-o", tmp_path / "q", d / "g.fa", "profile", tmp_path / "o_ms.vcf", "--name", "tumour"])
    _, cols = columns_of(tmp_path / "q_ms.sbs96.tsv")
    assert list(cols) == ["tumour"] and np.array_equal(cols["tumour"], total)
    # the loop closes: the written file is a spectrum --spectrum reads
    run_cli(["--seed", SEED, "--rng", "fast", "-o", tmp_path / "again", d / "g.fa", "args", "-sn", RATE, "--spectrum", tmp_path / "p_ms.sbs96.tsv",
             "--signature", "profile"])
    assert len(data_lines((tmp_path / "again_ms.vcf").read_bytes())[1].splitlines()) > 3000


def test_cli_profile_of_the_bgzip_vcf(files, tmp_path):  # noqa: F811
    d, seqs = files
    _, _, tables = twin_run(seqs)
    total = sum(st.counts(seq, recs)[0] for seq, recs in zip(seqs, tables))
    run_cli(spectrum_argv(d, tmp_path / "z", "--bgzip"))
    run_cli(["-o", tmp_path / "p", d / "g.fa", "profile", tmp_path / "z_ms.vcf.gz"])
    _, cols = columns_of(tmp_path / "p_ms.sbs96.tsv")
    assert list(cols) == ["profile"] and np.array_equal(cols["profile"], total)


def test_cli_profile_of_one_haplotype(files, tmp_path):  # noqa: F811
    """A diploid run's VCF under --consensus --haplotype 2: the records whose genotype holds that haplotype."""
    d, seqs = files
    _, _, tables = twin_run(seqs)
    run_cli(spectrum_argv(d, tmp_path / "d", "--ploidy", "2"))
    lines = data_lines((tmp_path / "d_ms.vcf").read_bytes())[1].splitlines()
    on2 = np.array([l.rsplit(b"\t", 1)[1] in (b"0|1", b"1|1") for l in lines])
    assert len(on2) == sum(len(t) for t in tables) and 0.6 < on2.mean() < 0.9
    total, at = np.zeros(96, dtype=np.uint64), 0
    for seq, recs in zip(seqs, tables):
        total += st.counts(seq, recs[on2[at:at + len(recs)]])[0]
        at += len(recs)
    run_cli(["-o", tmp_path / "h2", d / "g.fa", "profile", tmp_path / "d_ms.vcf", "--consensus", "--haplotype", "2"])
    text, cols = columns_of(tmp_path / "h2_ms.sbs96.tsv")
    assert np.array_equal(cols["profile"], total) and int(total.sum()) == int(on2.sum())
    assert "# consensus: sample (first) haplotype 2" in text.splitlines()


def test_cli_refused_line_ends_the_profile_like_the_replay(files, tmp_path):  # noqa: F811
    d, _ = files
    run_cli(spectrum_argv(d, tmp_path / "o"))
    raw = (tmp_path / "o_ms.vcf").read_bytes().split(b"\n")
    k = next(i for i, l in enumerate(raw) if l and not l.startswith(b"#")) + 40
    f = raw[k].split(b"\t")
    f[3] = b"A" if f[3] != b"A" else b"C"                              # REF no longer matches the genome
    raw[k] = b"\t".join(f)
    (tmp_path / "bad.vcf").write_bytes(b"\n".join(raw))
    replay = run_cli(["-o", tmp_path / "r", d / "g.fa", "vcf", tmp_path / "bad.vcf"], expect=1)
    prof = run_cli(["-o", tmp_path / "p", d / "g.fa", "profile", tmp_path / "bad.vcf"], expect=1)
    assert prof == replay and prof.startswith(f"ERROR: VCF line {k + 1}: ")
    assert not list(tmp_path.glob("p_ms*"))
    err = run_cli(["-o", tmp_path / "p", d / "g.fa", "profile", tmp_path / "o_ms.vcf", "--per-contig", "--name", "ctg3"], expect=1)
    assert "appears twice" in err and not list(tmp_path.glob("p_ms*"))
