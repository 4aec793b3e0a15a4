"""The ``profile`` mode without a GPU: the library's sequential restatement (``msim_dbg_sbs_counts``) against ``sbs_twin`` on
every shape the GPU tier runs, the file writer against the parser ``--spectrum`` reads with, and the command line's names,
refusals and usage errors.  All comparisons are exact integers."""
from __future__ import annotations

import contextlib
import io
from pathlib import Path

import numpy as np
import pytest

import sbs_twin as st
import spectrum_twin as tw
from mutation_simulator_amd import _ffi, argument_parser as ap, spectrum

B = _ffi.SBS_PASS
CASES = st.small_cases(B)


def check_host(bases, recs):
    got_c, got_t = _ffi.sbs_counts_host(bases, recs)
    want_c, want_t = st.counts(bases, recs)
    assert got_c.dtype == np.uint64 and got_c.shape == (96,) and got_t.shape == (8,)
    assert np.array_equal(got_c, want_c), np.flatnonzero(got_c != want_c)
    assert np.array_equal(got_t, want_t), (got_t, want_t)
    assert int(got_c.sum()) + int(got_t[0]) == int(got_t[1])
    return got_c, got_t


# ------------------------------------------------------------------------------ 1. the counts
def test_constants_are_the_headers():
    header = (Path(__file__).resolve().parent.parent / "include" / "msim.h").read_text()
    assert f"#define MSIM_SBS_PASS   {B}\n" in header and B % 64 == 0
    assert "#define MSIM_SBS_CHANNELS 96\n" in header and "#define MSIM_SBS_TALLIES   8\n" in header
    assert (_ffi.SBS_CHANNELS, _ffi.SBS_TALLIES) == (96, 8)


def test_the_twins_channel_table_is_the_packages():
    assert st.INDEX.tolist() == [list(row) for row in spectrum.CHANNEL_OF]


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_restatement_equals_the_twin(case):
    bases, recs, _ = CASES[case]
    check_host(bases, recs)


def test_short_contigs_have_one_channel_in_all():
    total = np.zeros(96, dtype=np.uint64)
    for key, (bases, recs, _) in st.short_contigs().items():
        c, t = check_host(bases, recs)
        assert int(t[1]) == len(bases) and int(c.sum()) == (1 if len(bases) == 3 else 0), key
        total += c
    assert np.flatnonzero(total).tolist() == [tw.CHANNELS.index("G[C>A]A")]       # GCA, aux 1: C>A


def test_every_context_lands_in_its_channel_and_every_channel_gets_two():
    bases = st.de_bruijn()
    pos, ctx = tw.sites(bases)
    assert len(bases) == 66 and sorted(ctx.tolist()) == list(range(64))
    total = np.zeros(96, dtype=np.uint64)
    for aux in range(3):
        recs = st.every_context()[f"every_context_aux{aux}"][1]
        c, t = check_host(bases, recs)
        assert int(t[0]) == 0 and int(t[1]) == 64
        for p, x in zip(pos.tolist(), ctx.tolist()):                   # one record alone: its (ctx, aux) is CHANNEL_OF's
            one, _ = _ffi.sbs_counts_host(bases, recs[recs["pos"] == p])
            assert np.flatnonzero(one).tolist() == [spectrum.CHANNEL_OF[x][aux]]
        total += c
    assert (total == 2).all()


def test_non_acgt_neighbourhoods_are_tallied_not_counted():
    for key, (bases, recs, _) in st.non_acgt().items():
        c, t = check_host(bases, recs)
        assert int(c.sum()) == 0 and t.tolist() == [1, 1, 0, 0, 0, 0, 0, 0], key
    lower = np.frombuffer(b"acgtacgt", dtype=np.uint8)                 # the context holds upper-cased bases: lower case is no base
    assert _ffi.sbs_counts_host(lower, st.snp_table([3], 0))[1].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]


def test_every_type_is_tallied_and_the_snps_among_them_counted():
    for key, (bases, recs, _) in st.every_type().items():
        c, t = check_host(bases, recs)
        assert (t[1:] > 0).all() and int(t[1:].sum()) == len(recs) and int(c.sum()) > 0 and int(t[0]) > 0, key


def test_one_channel_and_flat_tables():
    bases, recs, _ = st.one_channel()
    c, t = check_host(bases, recs)
    assert int(c[tw.CHANNELS.index("A[C>T]G")]) == st.ONE_CHANNEL_N == int(c.sum()) and int(t[0]) == 0
    flat = tw.random_genome(np.random.RandomState(5), st.ONE_CHANNEL_N + 2)
    recs = _ffi.spectrum_plan_host(flat, tw.every_site_table(), 77, 0)
    assert len(recs) == st.ONE_CHANNEL_N
    c, _ = check_host(flat, recs)
    assert int(c.min()) > 5000                                         # spread over all channels


def test_refusals_of_the_restatement_and_of_a_host_only_context():
    bases = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    bad = st.snp_table([3], 0)
    bad["type"] = 9
    with pytest.raises(_ffi.MsimError, match="record 0: unknown type") as e:
        _ffi.sbs_counts_host(bases, bad)
    assert e.value.code == _ffi.ERR_ARG
    with _ffi.Engine(-1) as eng:
        cid = eng.add_contig(bases)
        eng.set_records(cid, st.snp_table([3], 0), st.NO_POOL)
        with pytest.raises(_ffi.MsimError, match="needs the GPU") as e:
            eng.sbs_counts(cid)
        assert e.value.code == _ffi.ERR_HIP
        assert eng.sbs_timing() == 0.0


# ------------------------------------------------------------------------------ 2. the file
def test_render_profile_round_trips_through_parse():
    rs = np.random.RandomState(3)
    cols = [("profile", rs.randint(0, 1 << 40, 96)), ("chr1", rs.randint(0, 50, 96)), ("chr_2|x", np.arange(96) * 7 + 1),
            ("big", np.full(96, (1 << 53) - 1))]
    census = rs.randint(0, 10_000, 64)
    text = spectrum.render_profile(cols, spectrum.opportunities(census), notes=["made by a test", "records: SN 5, no context 1"])
    lines = text.splitlines()
    assert lines[:2] == ["# made by a test", "# records: SN 5, no context 1"]
    opp = [l for l in lines if l.startswith("# opportunities ")]
    assert len(opp) == 32 and lines[2:34] == opp and lines[34] == "Type\tprofile\tchr1\tchr_2|x\tbig"
    for line in opp:
        _, _, name, n = line.split(" ")
        ctx = 16 * "ACGT".index(name[0]) + 4 * "ACGT".index(name[1]) + "ACGT".index(name[2])
        assert name[1] in "CT" and int(n) == int(census[ctx]) + int(census[tw.rc(ctx)])
    assert [l.split("\t")[0] for l in lines[35:]] == tw.CHANNELS and len(lines) == 35 + 96
    for name, values in cols:
        got = spectrum.parse(text, name)
        assert got == [float(v) for v in values] and [int(v) for v in got] == [int(v) for v in values], name
    assert spectrum.parse(text) == [float(v) for v in cols[0][1]]      # the first column is the default
    # rows in any order, as a --signature pick finds them
    shuffled = lines[:35] + [lines[35 + i] for i in rs.permutation(96)]
    assert spectrum.parse("\n".join(shuffled) + "\n", "chr1") == [float(v) for v in cols[1][1]]


def test_an_all_zero_column_is_written_and_refused_by_parse():
    text = spectrum.render_profile([("profile", [0] * 96), ("c", [1] * 96)], notes=["empty"])
    with pytest.raises(spectrum.SpectrumError, match="all 96 weights are zero"):
        spectrum.parse(text, "profile")
    assert spectrum.parse(text, "c") == [1.0] * 96


@pytest.mark.parametrize("names,message", [
    (["profile", "profile"], "appears twice"), (["a b"], "holds a tab, a comma or a blank"), (["a\tb"], "holds a tab"),
    (["a,b"], "a comma"), ([""], "is empty"), ([], "no column")])
def test_render_profile_refuses_names_the_parser_would_split(names, message):
    with pytest.raises(spectrum.SpectrumError, match=message):
        spectrum.render_profile([(n, [1] * 96) for n in names])


# ------------------------------------------------------------------------------ 3. the command line
def test_profile_namespace():
    a = ap.get_args(["-o", "out", "genome.fa", "profile", "calls.vcf"])
    assert a.mode == "profile" and str(a.vcffile) == "calls.vcf" and str(a.outprofile) == "out_ms.sbs96.tsv"
    assert (a.consensus, a.sample, a.haplotype, a.per_contig, a.name) == (False, None, None, False, "profile")
    assert ap.profile_refusal(a) is None
    a = ap.get_args(["genome.fa", "profile", "calls.vcf.gz", "--consensus", "--sample", "S1", "--haplotype", "2", "--per-contig",
                     "--name", "tumour"])
    assert (a.consensus, a.sample, a.haplotype, a.per_contig, a.name) == (True, "S1", 2, True, "tumour")
    assert str(a.outprofile) == "genome_ms.sbs96.tsv"
    for argv in (["genome.fa", "vcf", "x.vcf"], ["genome.fa", "args", "-sn", "0.1"], ["genome.fa", "rmt", "x.rmt"], ["genome.fa", "it", "0.1"]):
        other = ap.get_args(argv)
        assert not hasattr(other, "outprofile") and not hasattr(other, "per_contig") and ap.profile_refusal(other) is None


@pytest.mark.parametrize("argv", [
    ["genome.fa", "profile", "x.vcf", "--sample", "S1"],
    ["genome.fa", "profile", "x.vcf", "--haplotype", "2"],
    ["genome.fa", "profile", "x.vcf", "--consensus", "--haplotype", "0"],
    ["genome.fa", "profile"],
    ["genome.fa", "profile", "x.vcf", "--spectrum", "s.tsv"],
    ["genome.fa", "vcf", "x.vcf", "--per-contig"],
])
def test_usage_errors(argv):
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
        ap.get_args(argv)
    assert ei.value.code == 2 and "usage:" in err.getvalue()
    if "--sample" in argv or argv[-2:] == ["--haplotype", "2"]:
        assert "--sample and --haplotype need --consensus" in err.getvalue()


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


@pytest.mark.parametrize("front,message", [
    (["--ploidy", "2"], "--ploidy 2 does not apply to the profile mode"),
    (["--chain"], "--chain does not apply to the profile mode"),
    (["--bgzip"], "--bgzip does not apply to the profile mode"),
    (["--gpus", "2"], "the profile mode needs a single-GPU run (--gpus 1)"),
])
def test_refused_combinations(monkeypatch, tmp_path, front, message):
    _refused(monkeypatch, ["-c", *front, "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "profile", str(tmp_path / "x.vcf")], message)
    assert not list(tmp_path.glob("out*"))


def test_column_names_are_checked_before_the_gpu(tmp_path):
    from mutation_simulator_amd import profile
    assert profile.column_refusal("profile", ["chr1", "chr2"], True) is None
    assert profile.column_refusal("profile", ["chr 1", "chr1"], False) is None     # (no contig heads a column)
    assert "appears twice" in profile.column_refusal("chr1", ["chr1", "chr2"], True)
    assert "appears twice" in profile.column_refusal("p", ["chr1", "chr1"], True)
    for bad in ("chr 1", "chr\t1", "chr,1"):
        assert "separators" in profile.column_refusal("p", ["ok", bad], True)
        assert "--name" in profile.column_refusal(bad, [], False)

    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError("the engine was used")

    class Rec:
        name = "profile"
    args = ap.get_args(["-o", str(tmp_path / "o"), "genome.fa", "profile", "x.vcf", "--per-contig"])
    with pytest.raises(profile.ProfileError, match="'profile' appears twice"):
        profile.Profile(args, [Rec()], engine=NoEngine()).run()
    assert not list(tmp_path.iterdir())
