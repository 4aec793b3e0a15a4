"""The ``reads`` mode on the device: ``k_reads_render`` against the numpy twin (``reads_twin``) on the cases of ``reads_cases``
-- the lane-pair and wave edges of the read length, chunk splits around a workgroup's reads, the top of the read counter, the
contig edges, IUPAC codes and N runs, fragment tables of 1 and 4096 entries --, checks that do not need the twin (a name
reproduces its bases; every base substituted), and the command line with and without ``--bgzip``."""
from __future__ import annotations

import gzip

import numpy as np
import pytest

from mutation_simulator_amd import _ffi
from mutation_simulator_amd import reads as rd
import reads_cases as rc
import reads_twin
from test_gpu_spectrum import run_cli

pytestmark = pytest.mark.gpu
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def setup_case(eng, case):
    eng.clear()
    for b in case.contigs:
        eng.add_contig(b)
    stride, n_elig, P = eng.reads_setup(case.params())
    plan = case.plan()
    assert (stride, n_elig, P) == (plan.stride, len(plan.idx), plan.P)
    return stride


def device_text(eng, name):
    case = rc.cases()[name]
    setup_case(eng, case)
    return [eng.reads_render(m, first, count) for m, first, count in case.ranges]


@pytest.mark.parametrize("name", [f"{kind}_len{n}" for n in rc.LENS for kind in ("se", "pe")])
def test_device_equals_twin_at_length_edges(eng, name):
    for got, want in zip(device_text(eng, name), rc.reference(name)):
        assert got == want


@pytest.mark.parametrize("name", ["stride_even", "stride_odd"])
def test_chunk_invariance(eng, name):
    """[0, N) in one call equals the calls' concatenation when the range is cut at 1, R - 1, R, R + 1 reads and an odd
    remainder: a read does not depend on where its call starts, and the ragged last workgroup writes what a full one does."""
    case = rc.cases()[name]
    stride = setup_case(eng, case)
    assert stride % 2 == (name == "stride_odd")
    R = _ffi.reads_group(stride)
    assert R % 16 == 0 and 2 * R + 8 < case.n_reads
    whole = eng.reads_render(0, 0, case.n_reads)
    assert whole == rc.reference(name)[0]
    cuts, at = [], 0
    for n in (1, R - 1, R, R + 1):
        cuts.append((at, n))
        at += n
    cuts.append((at, case.n_reads - at))
    assert (case.n_reads - at) % 2 == 1 and (case.n_reads - at) % R
    assert b"".join(eng.reads_render(0, first, count) for first, count in cuts) == whole


def test_top_of_the_counter(eng):
    """first = 2^32 - 5, count = 5 under N = 2^32 - 1: the 32-bit counter's last values and the 10-digit index field."""
    case = rc.cases()["top_of_counter"]
    for (mate, first, count), got, want in zip(case.ranges, device_text(eng, "top_of_counter"), rc.reference("top_of_counter")):
        assert got == want
        recs = rc.parse_records(got, case.plan().stride, case.prefix)
        assert [r[0] for r in recs] == list(range(2**32 - 5, 2**32)) and got[2:12] == b"4294967291"


def test_contig_edges(eng):
    """A contig exactly fmax long (one start), shorter ones first, in the middle and last (excluded, the numbering still the
    Fasta's), and reads that end on their contig's last base."""
    case = rc.cases()["contig_edges"]
    texts = device_text(eng, "contig_edges")
    assert tuple(texts) == rc.reference("contig_edges")
    recs = rc.parse_records(texts[0], case.plan().stride, case.prefix)
    assert {r[1] for r in recs} == {2, 4}
    assert all(r[2] == 1 for r in recs if r[1] == 2)                       # the single start of the contig of fmax bases
    assert any(r[2] - 1 + r[3] == len(case.contigs[r[1] - 1]) and r[3] == 306 and r[2] - 1 == len(case.contigs[r[1] - 1]) - 306
               for r in recs)


def test_names_reproduce_bases_without_errors(eng):
    """Independent of the twin: with every error threshold 0 a record's name, parsed back, gives its bases from the genome."""
    case = rc.cases()["err_none"]
    stride = case.plan().stride
    texts = device_text(eng, "err_none")
    for mate, text in enumerate(texts):
        recs = rc.parse_records(text, stride, case.prefix)
        assert [r[0] for r in recs] == list(range(case.n_reads))
        strands = set()
        for i, c, s, f, strand, m, seq, ql in recs:
            assert m == mate + 1 and seq == rc.expected_bases(case.contigs, c, s, f, strand, m, case.length)
            assert ql == bytes(case.qual[mate])
            strands.add(strand)
        assert strands == {"+", "-"}


def test_mates_of_a_read_long_fragment_are_reverse_complements(eng):
    case = rc.cases()["frag_1"]
    zero = rc.Case(case.contigs, case.key, case.n_reads, case.length, True, case.frag_min, case.frag_thr, err=(0.0, 0.0))
    stride = setup_case(eng, zero)
    m1 = rc.parse_records(eng.reads_render(0, 0, zero.n_reads), stride, zero.prefix)
    m2 = rc.parse_records(eng.reads_render(1, 0, zero.n_reads), stride, zero.prefix)
    for a, b in zip(m1, m2):
        assert a[:5] == b[:5] and a[3] == zero.length
        assert b[6] == a[6].translate(rc._COMP)[::-1]
    assert tuple(device_text(eng, "frag_1")) == rc.reference("frag_1")


def test_every_base_substituted_when_the_thresholds_are_full(eng):
    """err_thr all 2^53: no A/C/G/T base equals the genome's, every N stays N with quality '!'."""
    case = rc.cases()["err_all"]
    stride = case.plan().stride
    texts = device_text(eng, "err_all")
    assert tuple(texts) == rc.reference("err_all")
    n_seen = 0
    for mate, text in enumerate(texts):
        for i, c, s, f, strand, m, seq, ql in rc.parse_records(text, stride, case.prefix):
            clean = rc.expected_bases(case.contigs, c, s, f, strand, m, case.length)
            for got, was, q in zip(seq, clean, ql):
                if was == ord("N"):
                    assert got == ord("N") and q == ord("!")
                    n_seen += 1
                else:
                    assert got != was and got in b"ACGT" and q != ord("!")
    assert n_seen > 1000


def test_iupac_codes_and_n_runs(eng):
    case = rc.cases()["iupac"]
    texts = device_text(eng, "iupac")
    assert tuple(texts) == rc.reference("iupac")
    recs = rc.parse_records(texts[0], case.plan().stride, case.prefix)
    only_n = sum(1 for r in recs if set(r[6]) == {ord("N")})
    assert only_n > 0 and all(set(r[6]) <= set(b"ACGTN") for r in recs)
    _, all_n = eng.reads_timing()
    only_n2 = sum(1 for r in rc.parse_records(texts[1], case.plan().stride, case.prefix) if set(r[6]) == {ord("N")})
    assert all_n == (only_n, only_n2)                      # what the log reports


@pytest.mark.parametrize("name", ["frag_4096", "frag_7_all"])
def test_fragment_tables(eng, name):
    case = rc.cases()[name]
    texts = device_text(eng, name)
    assert tuple(texts) == rc.reference(name)
    seen = {r[3] for r in rc.parse_records(texts[0], case.plan().stride, case.prefix)}
    if name == "frag_7_all":                               # 20 000 reads over 7 lengths: every one occurs
        assert seen == set(range(36, 43))
    else:
        assert min(seen) >= 50 and max(seen) <= 50 + 4095 and len(seen) > 1000


# ------------------------------------------------------------------------------------------------------ the command line
N_CLI, SEED = 3000, 7
CLI = ["reads", "-n", str(N_CLI), "-l", "100", "--paired", "--frag-mean", "300", "--frag-sd", "30", "--prefix", "cli."]


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads_cli")
    contigs = rc.genome(21, 5000, 200, 3777, alphabet=b"ACGTACGTACGTN")
    fa = d / "g.fa"
    with open(fa, "wb") as f:
        for k, b in enumerate(contigs):
            f.write(b">c%d\n" % k + b"".join(b.tobytes()[q:q + 60] + b"\n" for q in range(0, len(b), 60)))
    run_cli(["--seed", SEED, "-o", d / "plain", fa] + CLI)
    return d, fa, contigs


def test_cli_paired_files_equal_the_twin(cli_run):
    d, fa, contigs = cli_run
    fmin, thr = rd.fragment_table(100, True, 300, 30)
    err_thr, qual = rd.error_tables(100, 0.001, 0.01)
    for mate in (0, 1):
        want = reads_twin.render(contigs, rd.key_of(SEED), N_CLI, 100, fmin, thr, err_thr, qual, "cli.", mate, 0, N_CLI)
        assert (d / f"plain_ms_{mate + 1}.fq").read_bytes() == want


def test_cli_bgzip_decompresses_to_the_plain_files(cli_run):
    d, fa, _ = cli_run
    run_cli(["--seed", SEED, "--bgzip", "-o", d / "bz", fa] + CLI)
    for mate in (1, 2):
        raw = (d / f"bz_ms_{mate}.fq.gz").read_bytes()
        assert raw.endswith(BGZF_EOF)
        assert gzip.decompress(raw) == (d / f"plain_ms_{mate}.fq").read_bytes()


def test_cli_seed_decides_the_bytes(cli_run):
    d, fa, _ = cli_run
    run_cli(["--seed", SEED, "-o", d / "again", fa] + CLI)
    run_cli(["--seed", SEED + 1, "-o", d / "other", fa] + CLI)
    for mate in (1, 2):
        plain = (d / f"plain_ms_{mate}.fq").read_bytes()
        assert (d / f"again_ms_{mate}.fq").read_bytes() == plain
        other = (d / f"other_ms_{mate}.fq").read_bytes()
        assert len(other) == len(plain) and other != plain
