"""``--spectrum`` without a GPU: the spectrum file parser, the (context, aux) -> channel mapping, the exact thresholds, the
library's sequential restatements (``msim_dbg_context_counts`` / ``msim_dbg_spectrum_plan``) against ``spectrum_twin``, the
distribution the draw produces, and the command line's refusals.  All comparisons with the twin are exact."""
from __future__ import annotations

import contextlib
import io
import math
from fractions import Fraction

import numpy as np
import pytest

import spectrum_twin as tw
from mutation_simulator_amd import _ffi, argument_parser as ap, spectrum

KEY = 0x0123456789ABCDEF


# ------------------------------------------------------------------------------ 1. the file
def flat(n=96):
    return [1.0 + i for i in range(n)]


def test_cosmic_shaped_file_and_signature_by_name():
    """COSMIC's layout: a header "Type<TAB>SBS1<TAB>SBS2 ...", one row per channel, sorted by substitution then flanks."""
    cols = {"SBS1": [1e-3 * (i + 1) for i in range(96)], "SBS2": [5.5e-7 * (96 - i) for i in range(96)], "SBS5": flat()}
    order = sorted(range(96), key=lambda i: (tw.CHANNELS[i][2:5], tw.CHANNELS[i][0], tw.CHANNELS[i][6]))
    text = "Type\t" + "\t".join(cols) + "\n" + "".join(
        tw.CHANNELS[i] + "\t" + "\t".join(repr(v[i]) for v in cols.values()) + "\n" for i in order)
    assert spectrum.parse(text) == cols["SBS1"]                       # default: the first value column
    for name, want in cols.items():
        assert spectrum.parse(text, name) == want
    with pytest.raises(spectrum.SpectrumError, match=r"line 1: no signature named 'SBS9'; the file has: SBS1, SBS2, SBS5"):
        spectrum.parse(text, "SBS9")


@pytest.mark.parametrize("sep", ["\t", ",", " ", "   "])
def test_two_column_files(sep):
    w = flat()
    assert spectrum.parse(tw.spectrum_text(w, sep=sep, header=None)) == w
    assert spectrum.parse(tw.spectrum_text(w, sep=sep)) == w
    assert spectrum.parse("# a comment\n\n" + tw.spectrum_text(w, sep=sep, shuffle_seed=3).replace("\n", "\n\n# x\n", 5)) == w


def test_channel_order_is_the_twins():
    assert list(spectrum.CHANNELS) == tw.CHANNELS and len(set(tw.CHANNELS)) == 96


def _rows(w=None):
    return tw.spectrum_text(w or flat(), header=None).splitlines()


REFUSED_FILES = [
    ("95 rows", "\n".join(_rows()[:95]), r"line 95: 95 channels, 96 are required \(missing: T\[T>G\]T\)"),
    ("duplicate", "\n".join(_rows()[:40] + [_rows()[1]] + _rows()[40:]), r"line 41: channel A\[C>A\]C appears twice"),
    ("purine", "\n".join(_rows()[:10] + ["A[G>T]C\t1.0"] + _rows()[11:]), r"line 11: 'A\[G>T\]C' is purine-centred"),
    ("negative", "\n".join(_rows()[:5] + ["C[C>A]C\t-0.5"] + _rows()[6:]), r"line 6: weight -0.5 of C\[C>A\]C"),
    ("nan", "\n".join(_rows()[:5] + ["C[C>A]C\tnan"] + _rows()[6:]), r"line 6: weight nan of C\[C>A\]C"),
    ("inf", "\n".join(_rows()[:5] + ["C[C>A]C\tinf"] + _rows()[6:]), r"line 6: weight inf of C\[C>A\]C"),
    ("no number", "\n".join(_rows()[:5] + ["C[C>A]C\tx"] + _rows()[6:]), r"line 6: 'x' is no number"),
    ("all zeros", "\n".join(_rows([0.0] * 96)), r"line 96: all 96 weights are zero"),
    ("same base", "\n".join(_rows()[:5] + ["A[C>C]C\t1"] + _rows()[6:]), r"line 6: 'A\[C>C\]C' is no substitution"),
    ("junk row", "\n".join(_rows()[:5] + ["hello\t1"] + _rows()[6:]), r"line 6: 'hello' is no channel"),
    ("short row", "\n".join(["Type\ta\tb"] + _rows()[:5] + ["C[C>A]C"] + _rows()[6:]), r"line 7: no value in column 2"),
]


@pytest.mark.parametrize("name,text,message", REFUSED_FILES, ids=[c[0].replace(" ", "_") for c in REFUSED_FILES])
def test_refused_files(name, text, message):
    with pytest.raises(spectrum.SpectrumError, match=message):
        spectrum.parse(text + "\n")


def test_signature_without_a_header_and_unreadable_file(tmp_path):
    with pytest.raises(spectrum.SpectrumError, match="line 1: no signature named 'SBS1'; the file has no header line"):
        spectrum.parse(tw.spectrum_text(flat(), header=None), "SBS1")
    with pytest.raises(spectrum.SpectrumError, match="cannot read"):
        spectrum.load(tmp_path / "nothing.tsv")
    f = tmp_path / "s.csv"
    f.write_text(tw.spectrum_text(flat(), sep=","))
    assert spectrum.load(f) == flat()


# ------------------------------------------------------------------------------ 2. channels
def test_every_pair_maps_onto_a_channel_and_each_channel_is_hit_twice():
    seen: dict = {}
    for ctx in range(64):
        for aux in range(3):
            name = spectrum.channel_name(ctx, aux)
            assert name == tw.channel(ctx, aux) and tw.CHANNELS[spectrum.channel_index(ctx, aux)] == name
            seen.setdefault(name, []).append((ctx, aux))
    assert sorted(seen) == sorted(tw.CHANNELS)
    for name, pairs in seen.items():
        assert len(pairs) == 2, name
        (c0, a0), (c1, a1) = pairs
        assert c1 == tw.rc(c0) == spectrum.rc(c0) and c0 != c1


def test_hand_checked_channels():
    ctx = lambda s: 16 * "ACGT".index(s[0]) + 4 * "ACGT".index(s[1]) + "ACGT".index(s[2])   # noqa: E731
    assert spectrum.channel_name(ctx("ACG"), 0) == "A[C>T]G"
    assert spectrum.channel_name(ctx("CGT"), 0) == "A[C>T]G"          # the other strand of the same site
    assert spectrum.channel_name(ctx("ACG"), 1) == "A[C>A]G" and spectrum.channel_name(ctx("ACG"), 2) == "A[C>G]G"
    assert spectrum.channel_name(ctx("TTT"), 0) == "T[T>C]T" and spectrum.channel_name(ctx("AAA"), 0) == "T[T>C]T"
    assert spectrum.channel_name(ctx("GAC"), 1) == "G[T>A]C"          # A>T read from the other strand: GTC, T>A
    assert spectrum.context_name(ctx("GAC")) == "GAC" and spectrum.rc(ctx("GAC")) == ctx("GTC")


# ------------------------------------------------------------------------------ 3. thresholds
def test_thresholds_equal_the_twins():
    rs = np.random.RandomState(4)
    for trial in range(6):
        counts = rs.randint(1000, 5000, 64).astype(np.uint64)
        gone = rs.randint(0, 64, 4)
        counts[gone] = 0                                              # contexts that do not occur: alone, and with their
        counts[[tw.rc(int(c)) for c in gone[:2]]] = 0                  # reverse complement (the channel then contributes nothing)
        w = list(rs.uniform(0, 1, 96))
        w[int(rs.randint(0, 96))] = 0.0
        rate = float(rs.uniform(1e-4, 0.03))
        got = spectrum.thresholds(counts, w, rate)
        want = tw.thresholds(counts, w, rate)
        assert len(got) == 192 and all(isinstance(x, int) for x in got)
        assert np.array_equal(np.array(got, dtype=np.uint64), want)
        for ctx in range(64):
            t = got[3 * ctx:3 * ctx + 3]
            assert t[0] <= t[1] <= t[2]
            if counts[ctx] == 0:
                assert t == [0, 0, 0]
    # the expected number of SNPs is RATE * n_valid where every context and its reverse complement occur
    counts = rs.randint(1, 5000, 64)
    p = spectrum.probabilities(counts, tw.skewed_weights(), 0.02)
    assert sum(int(counts[c]) * sum(p[c]) for c in range(64)) == Fraction(0.02) * int(counts.sum())


def test_probability_above_one_is_refused_by_context_name():
    counts = np.full(64, 1000, dtype=np.uint64)
    counts[6] = counts[tw.rc(6)] = 1                                  # ACG / CGT are rare, the spectrum wants many of them
    w = tw.skewed_weights()
    with pytest.raises(spectrum.SpectrumError, match="context ACG would mutate with probability"):
        spectrum.thresholds(counts, w, 0.02)
    with pytest.raises(tw.Refused) as e:
        tw.thresholds(counts, w, 0.02)
    assert e.value.ctx == 6
    assert len(spectrum.thresholds(counts, w, 1e-5)) == 192            # the same census at a rate it can carry
    # exactly 1 passes and saturates: one context pair, one channel
    counts = np.zeros(64, dtype=np.uint64)
    counts[6] = counts[tw.rc(6)] = 10
    w = [0.0] * 96
    w[tw.CHANNELS.index("A[C>T]G")] = 3.0
    thr = spectrum.thresholds(counts, w, 1.0)
    assert thr[18:21] == [2**64 - 1] * 3 and thr[3 * tw.rc(6):3 * tw.rc(6) + 3] == [2**64 - 1] * 3 and sum(thr) == 6 * (2**64 - 1)


# ------------------------------------------------------------------------------ 4. the library's host restatements
def check_both(bases, thr, key=KEY, seq=3):
    counts, n_valid = _ffi.context_counts_host(bases)
    want_counts, want_n = tw.census(bases)
    assert np.array_equal(counts, want_counts) and n_valid == want_n
    got = _ffi.spectrum_plan_host(bases, thr, key, seq)
    want = tw.plan(bases, thr, key, seq)
    assert got.dtype == _ffi.RECORD_DTYPE and got.tobytes() == want.tobytes(), (len(got), len(want))
    return got


@pytest.mark.parametrize("L", [0, 1, 2, 3, 4, 17])
def test_tiny_contigs(L):
    bases = np.frombuffer(b"ACGTTGCAACGTACGTA"[:L], dtype=np.uint8)
    recs = check_both(bases, tw.every_site_table())
    assert len(recs) == max(0, L - 2)
    assert len(check_both(bases, np.zeros(192, dtype=np.uint64))) == 0


def test_all_n_and_ambiguity_runs():
    rs = np.random.RandomState(11)
    assert len(check_both(np.full(5000, ord("N"), dtype=np.uint8), tw.every_site_table())) == 0
    bases = tw.random_genome(rs, 30_000, n_runs=20, iupac=400)
    recs = check_both(bases, tw.every_site_table())
    pos, _ = tw.sites(bases)
    assert np.array_equal(recs["pos"], pos) and 0 < len(pos) < len(bases) - 2
    assert set(np.unique(recs["aux"]).tolist()) == {0, 1, 2}
    lower = np.frombuffer(bytes(bases).lower(), dtype=np.uint8)        # the context holds upper-cased bases: lower case is no base
    assert _ffi.context_counts_host(lower)[1] == 0


def test_random_genomes_and_tables():
    rs = np.random.RandomState(2024)
    for trial in range(20):
        L = int(rs.randint(3, 50_001))
        bases = tw.random_genome(rs, L, n_runs=int(rs.randint(0, 4)), iupac=int(rs.randint(0, 30)))
        thr = tw.random_table(rs, float(rs.choice([1e-3, 1e-2, 0.25, 0.6])))
        check_both(bases, thr, key=int(rs.randint(0, 2**62)) * 4 + trial, seq=int(rs.randint(0, 70000)))


def test_refusals_of_the_restatements():
    bases = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    thr = tw.every_site_table().copy()
    thr[3 * 6 + 1] = 5                                                 # ACG: 2^64/3, 5, 2^64 - 1
    with pytest.raises(_ffi.MsimError, match="context 6 are not non-decreasing") as e:
        _ffi.spectrum_plan_host(bases, thr, KEY, 0)
    assert e.value.code == _ffi.ERR_ARG
    with pytest.raises(ValueError):
        _ffi.spectrum_plan_host(bases, np.zeros(191, dtype=np.uint64), KEY, 0)
    lib = _ffi.load()
    n = _ffi.C.c_uint64()
    ok = tw.every_site_table()
    small = np.zeros(2, dtype=_ffi.RECORD_DTYPE)
    assert lib.msim_dbg_spectrum_plan(bases.ctypes.data, 8, ok.ctypes.data, KEY, 0, small.ctypes.data, 2, _ffi.C.byref(n)) == _ffi.ERR_ARG
    assert lib.msim_dbg_spectrum_plan(bases.ctypes.data, 8, ok.ctypes.data, KEY, 0, None, 0, _ffi.C.byref(n)) == _ffi.OK and n.value == 6


def test_a_host_only_context_refuses_the_device_calls():
    with _ffi.Engine(-1) as eng:
        cid = eng.add_contig(np.frombuffer(b"ACGTACGT", dtype=np.uint8))
        for call in (lambda: eng.context_counts(cid), lambda: eng.plan_contig_spectrum(cid, tw.every_site_table(), KEY, 0)):
            with pytest.raises(_ffi.MsimError) as e:
                call()
            assert e.value.code == _ffi.ERR_HIP
        assert eng.spectrum_timing() == (0.0, 0.0)


def test_the_draw_depends_on_key_and_contig_number_only_through_philox():
    bases = tw.random_genome(np.random.RandomState(1), 20_000)
    thr = tw.random_table(np.random.RandomState(2), 0.05)
    a = _ffi.spectrum_plan_host(bases, thr, KEY, 0)
    assert a.tobytes() == _ffi.spectrum_plan_host(bases, thr, KEY, 0).tobytes()
    assert a.tobytes() != _ffi.spectrum_plan_host(bases, thr, KEY, 1).tobytes()
    assert a.tobytes() != _ffi.spectrum_plan_host(bases, thr, KEY + 1, 0).tobytes()
    assert (np.diff(a["pos"].astype(np.int64)) > 0).all() and (a["stop"] == a["pos"]).all()
    assert not a["extra"].any() and not a["rsv"].any() and (a["type"] == 1).all() and a["aux"].max() <= 2


# ------------------------------------------------------------------------------ 5. the distribution
def test_channel_counts_follow_the_spectrum():
    """One uniform contig of 1 000 000 bases at RATE 0.02 under the skewed spectrum: every channel's count within 6 sigma of
    RATE * n_valid * w / W (binomial over the pooled sites of its two contexts, which share one probability), the total within
    6 sigma of RATE * n_valid.  The twin is deterministic, so this passes always or never."""
    rate, L = 0.02, 1_000_000
    bases = tw.random_genome(np.random.RandomState(77), L)
    w = tw.skewed_weights()
    W = sum(w)
    cpg = [tw.CHANNELS.index(f"{l}[C>T]G") for l in "ACGT"]
    assert sorted(np.argsort(w)[-4:].tolist()) == cpg and min(w) == 1.0 + 6.0 * 4 / 95.0 and max(w[i] for i in range(96) if i not in cpg) == 7.0
    counts, n_valid = tw.census(bases)
    assert n_valid == L - 2 and counts.min() > 0
    expect = [rate * n_valid * x / W for x in w]
    assert min(expect) >= 50, min(expect)                              # no channel is left out of the check
    thr = tw.thresholds(counts, w, rate)
    assert np.array_equal(np.array(spectrum.thresholds(counts, w, rate), dtype=np.uint64), thr)
    pos, ctx, j = tw.outcomes(bases, thr, KEY, 0)
    hit = j < 3
    observed = np.zeros(96, dtype=np.int64)
    index = np.array([[tw.CHANNELS.index(tw.channel(c, a)) for a in range(3)] for c in range(64)])
    np.add.at(observed, index[ctx[hit], j[hit]], 1)
    for ch in range(96):
        pooled = sum(int(counts[c]) for c in range(64) for a in range(3) if index[c, a] == ch)
        p = expect[ch] / pooled
        assert abs(observed[ch] - expect[ch]) <= 6 * math.sqrt(expect[ch] * (1 - p)), (tw.CHANNELS[ch], int(observed[ch]), expect[ch])
    total = int(hit.sum())
    assert abs(total - rate * n_valid) <= 6 * math.sqrt(rate * n_valid * (1 - rate)), total
    # and the library's restatement draws the same table
    recs = _ffi.spectrum_plan_host(bases, thr, KEY, 0)
    assert len(recs) == total and recs.tobytes() == tw.plan(bases, thr, KEY, 0).tobytes()


# ------------------------------------------------------------------------------ 6. the command line
def test_namespace_carries_spectrum_and_signature():
    a = ap.get_args(["--rng", "fast", "genome.fa", "args", "-sn", "0.01", "--spectrum", "sbs.tsv", "--signature", "SBS1"])
    assert str(a.spectrum) == "sbs.tsv" and a.signature == "SBS1" and ap.spectrum_refusal(a) is None
    a = ap.get_args(["genome.fa", "args", "-sn", "0.01"])
    assert a.spectrum is None and a.signature is None and ap.spectrum_refusal(a) is None
    for mode in (["rmt", "x.rmt"], ["it", "0.1"], ["vcf", "x.vcf"]):
        assert not hasattr(ap.get_args(["genome.fa"] + mode), "spectrum")


@pytest.mark.parametrize("argv", [
    ["genome.fa", "args", "-sn", "0.01", "--signature", "SBS1"],
    ["genome.fa", "rmt", "x.rmt", "--spectrum", "s.tsv"],
    ["genome.fa", "it", "0.1", "--spectrum", "s.tsv"],
    ["genome.fa", "vcf", "x.vcf", "--spectrum", "s.tsv"],
    ["--spectrum", "s.tsv", "genome.fa", "args", "-sn", "0.01"],
])
def test_usage_errors(argv):
    with pytest.raises(SystemExit) as ei, contextlib.redirect_stderr(io.StringIO()) as err:
        ap.get_args(argv)
    assert ei.value.code == 2 and "usage:" in err.getvalue()
    if "--signature" in argv:
        assert "--signature needs --spectrum" in err.getvalue()


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


@pytest.mark.parametrize("front,tail,message", [
    ([], ["-sn", "0.01"], "--spectrum needs --rng fast"),
    (["--rng", "compat"], ["-sn", "0.01"], "--spectrum needs --rng fast"),
    (["--rng", "fast"], ["-sn", "0.01", "-in", "0.001"], "--spectrum draws SNPs only (-in given)"),
    (["--rng", "fast"], ["-sn", "0.01", "-de", "0.001", "-tl", "0.001"], "--spectrum draws SNPs only (-de, -tl given)"),
    (["--rng", "fast"], ["-sn", "0.01", "-iv", "0.001"], "--spectrum draws SNPs only (-iv given)"),
    (["--rng", "fast"], ["-sn", "0.01", "-du", "0.001"], "--spectrum draws SNPs only (-du given)"),
    (["--rng", "fast"], [], "--spectrum needs an SNP rate"),
    (["--rng", "fast", "--gpus", "2"], ["-sn", "0.01"], "--spectrum needs a single-GPU run (--gpus 1)"),
])
def test_refused_combinations(monkeypatch, tmp_path, front, tail, message):
    spec = tmp_path / "s.tsv"
    spec.write_text(tw.spectrum_text(tw.skewed_weights()))
    _refused(monkeypatch, ["-c", *front, "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "args", *tail, "--spectrum", str(spec)], message)
    assert not list(tmp_path.glob("out*"))


def test_a_bad_spectrum_file_ends_the_run_before_anything_is_opened(monkeypatch, tmp_path):
    spec = tmp_path / "s.tsv"
    spec.write_text("\n".join(tw.spectrum_text(flat()).splitlines()[:-1]) + "\n")
    argv = ["-c", "--rng", "fast", "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "args", "-sn", "0.01", "--spectrum", str(spec)]
    _refused(monkeypatch, argv, "s.tsv line 96: 95 channels, 96 are required")
    spec.write_text(tw.spectrum_text(flat()))
    _refused(monkeypatch, argv + ["--signature", "SBS7a"], "s.tsv line 1: no signature named 'SBS7a'; the file has: SBSx")
    assert not list(tmp_path.glob("out*"))
