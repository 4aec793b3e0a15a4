"""The ``reads`` mode without a GPU: the library's sequential restatement of the rule (``msim_dbg_reads_render``) against the
numpy twin on every case of ``reads_cases``, the table builders, and the usage errors the command line refuses."""
from __future__ import annotations

import numpy as np
import pytest

from mutation_simulator_amd import _ffi
from mutation_simulator_amd import reads as rd
from mutation_simulator_amd.argument_parser import get_args, reads_refusal
import reads_cases as rc

ONE53 = 1 << 53


@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_host_restatement_equals_twin(name):
    case = rc.cases()[name]
    plan = case.plan()
    for (mate, first, count), want in zip(case.ranges, rc.reference(name)):
        got, stride, n_elig, P = _ffi.dbg_reads_render(case.params(), case.contigs, mate, first, count)
        assert (stride, n_elig, P) == (plan.stride, len(plan.idx), plan.P)
        assert len(want) == count * stride
        assert got == want


def test_twin_reproduces_bases_from_names():
    """The twin itself against the documentation's reading of a name: without errors every record's bases are its
    fragment's, and the excluded contigs keep their numbers."""
    case = rc.cases()["contig_edges"]
    zero = rc.Case(case.contigs, case.key, case.n_reads, case.length, True, case.frag_min, case.frag_thr, err=(0.0, 0.0), prefix=case.prefix)
    stride = zero.plan().stride
    touched = 0
    for mate in (0, 1):
        for i, c, s, f, strand, m, seq, ql in rc.parse_records(zero.twin(mate, 0, zero.n_reads), stride, zero.prefix):
            assert c in (2, 4) and m == mate + 1
            assert seq == rc.expected_bases(zero.contigs, c, s, f, strand, m, zero.length)
            touched += s - 1 + f == len(zero.contigs[c - 1]) and f == 306
    assert touched > 0                                     # some fragment ends on its contig's last base


def test_seven_lengths_all_occur_in_the_twin():
    case = rc.cases()["frag_7_all"]
    stride = case.plan().stride
    seen = {r[3] for r in rc.parse_records(rc.reference("frag_7_all")[0], stride, case.prefix)}
    assert seen == set(range(36, 43))


# ------------------------------------------------------------------------------------------------------ the table builders
@pytest.mark.parametrize("length,mean,sd", [(150, 400, 50), (100, 100, 0), (512, 300, 511), (1, 1, 1), (150, 100, 20)])
def test_fragment_thresholds_ascend_and_end_at_2_53(length, mean, sd):
    fmin, thr = rd.fragment_table(length, True, mean, sd)
    assert fmin == max(length, mean - 4 * sd) and len(thr) == mean + 4 * sd - fmin + 1
    assert 1 <= len(thr) <= _ffi.READS_MAX_FRAG
    assert np.all(np.diff(thr.astype(object)) >= 0) and int(thr[-1]) == ONE53
    if sd:                                                 # the mode of the (truncated) normal carries the largest mass
        mass = np.diff(np.concatenate([[0], thr.astype(object)]))
        assert abs(int(np.argmax(mass)) + fmin - max(mean, fmin)) <= 1


def test_single_end_table_is_the_read():
    fmin, thr = rd.fragment_table(150, False)
    assert fmin == 150 and thr.tolist() == [ONE53]


def test_error_tables():
    thr, qual = rd.error_tables(150, 0.0, 0.0)
    assert thr.shape == (2, 150) and not thr.any() and set(qual.ravel().tolist()) == {33 + 41}
    thr, qual = rd.error_tables(150, 0.001, 0.01)
    from fractions import Fraction
    import math
    assert int(thr[0, 0]) == math.ceil(Fraction(0.001) * ONE53) and int(thr[0, -1]) == math.ceil(Fraction(0.01) * ONE53)
    assert np.all(np.diff(thr[0].astype(object)) >= 0) and np.array_equal(thr[0], thr[1])
    assert qual[0, 0] == 33 + 30 and qual[0, -1] == 33 + 20
    thr, qual = rd.error_tables(3, 1.0, 1.0)
    assert set(thr.ravel().tolist()) == {ONE53} and set(qual.ravel().tolist()) == {33 + 2}
    thr, _ = rd.error_tables(1, 0.25, 0.75)                # one cycle: the first value
    assert thr.tolist() == [[ONE53 // 4], [ONE53 // 4]]
    assert rd.parse_error_rate("0.5") == (0.5, 0.5) and rd.parse_error_rate("0:1") == (0.0, 1.0)


@pytest.mark.parametrize("call", [
    lambda: rd.fragment_table(150, False, 400, None),       # --frag-* without --paired
    lambda: rd.fragment_table(150, True, 400, None),        # --paired without both
    lambda: rd.fragment_table(150, True, None, 50),
    lambda: rd.fragment_table(150, True, 400, 512),         # SD > 511
    lambda: rd.fragment_table(150, True, 100, 12),          # M + 4 SD < LEN
    lambda: rd.fragment_table(0, False),
    lambda: rd.fragment_table(513, False),
    lambda: rd.parse_error_rate("1.5"),
    lambda: rd.parse_error_rate("0.1:0.2:0.3"),
    lambda: rd.parse_error_rate("x"),
    lambda: rd.read_count(0, None, 1000, 100, 1),
    lambda: rd.read_count(2**32, None, 1000, 100, 1),
    lambda: rd.read_count(None, 0.01, 1000, 100, 1),        # a coverage that gives no read
])
def test_table_builders_refuse_usage_errors(call):
    with pytest.raises(rd.ReadsError):
        call()


def test_read_count_from_coverage():
    assert rd.read_count(None, 30.0, 3_000_000, 150, 2) == 300_000
    assert rd.read_count(None, 0.5, 1001, 100, 1) == 5
    assert rd.eligible_bases([100, 306, 50, 346, 200], 306) == 652
    assert rd.prefix_refusal("ok.A_z-9") is None and rd.prefix_refusal("a b") and rd.prefix_refusal("x" * 33)


# ------------------------------------------------------------------------------------------------------ the command line
def _parse(tmp_path, *argv):
    fa = tmp_path / "g.fa"
    fa.write_text(">a\nACGT\n")
    return get_args([str(fa), *argv])


def test_parser_accepts_and_names_the_outputs(tmp_path):
    a = _parse(tmp_path, "-o", str(tmp_path / "out"), "reads", "-n", "10")
    assert (a.length, a.paired, a.error_rate, a.prefix, a.n_reads) == (150, False, "0.001:0.01", "r", 10)
    assert a.outfastq.name == "out_ms.fq" and reads_refusal(a) is None
    a = _parse(tmp_path, "--bgzip", "reads", "--coverage", "2.5", "--paired", "--frag-mean", "400", "--frag-sd", "50", "-l", "100")
    assert (a.outfastq_1.name, a.outfastq_2.name) == ("g_ms_1.fq.gz", "g_ms_2.fq.gz") and a.coverage == 2.5


@pytest.mark.parametrize("argv", [
    ["reads"],                                                             # neither -n nor --coverage
    ["reads", "-n", "5", "--coverage", "1"],
    ["reads", "-n", "0"],
    ["reads", "-n", str(2**32)],
    ["reads", "-n", "5", "-l", "0"],
    ["reads", "-n", "5", "-l", "513"],
    ["reads", "-n", "5", "--frag-mean", "400"],                            # --frag-* without --paired
    ["reads", "-n", "5", "--frag-sd", "50"],
    ["reads", "-n", "5", "--paired"],                                      # --paired without both
    ["reads", "-n", "5", "--paired", "--frag-mean", "400"],
    ["reads", "-n", "5", "--paired", "--frag-sd", "50"],
    ["reads", "-n", "5", "--paired", "--frag-mean", "400", "--frag-sd", "512"],
    ["reads", "-n", "5", "--paired", "--frag-mean", "100", "--frag-sd", "12"],   # M + 4 SD < LEN
    ["reads", "-n", "5", "--error-rate", "2"],
    ["reads", "-n", "5", "--error-rate", "0.1:0.2:0.3"],
    ["reads", "-n", "5", "--prefix", "a b"],
    ["reads", "-n", "5", "--prefix", "x" * 33],
])
def test_parser_refuses_usage_errors(tmp_path, argv):
    with pytest.raises(SystemExit):
        _parse(tmp_path, *argv)


@pytest.mark.parametrize("front", [["--ploidy", "2"], ["--chain"], ["--gpus", "2"]])
def test_reads_refusals(tmp_path, front):
    a = _parse(tmp_path, *front, "reads", "-n", "5")
    assert reads_refusal(a)


def test_no_eligible_contig_is_refused_before_the_gpu(tmp_path):
    """A genome without a contig of fmax bases ends the run before an engine exists."""
    a = _parse(tmp_path, "reads", "-n", "5", "-l", "10")
    fasta = [np.frombuffer(b"ACGT", dtype=np.uint8)]
    r = rd.Reads(a, fasta, engine=None)
    with pytest.raises(rd.ReadsError, match="no contig"):
        r.run()
    assert r._engine is None


def test_library_refuses_bad_tables():
    case = rc.cases()["frag_1"]
    good = dict(key=1, n_reads=10, length=75, paired=True, frag_min=75, frag_thr=[ONE53], err_thr=case.err_thr, qual=case.qual,
                prefix="r")
    for bad in (dict(frag_thr=[5, 4, ONE53]), dict(frag_thr=[ONE53 - 1]), dict(frag_min=74), dict(prefix="a b"), dict(n_reads=2**32),
                dict(err_thr=np.full((2, 75), ONE53 + 1, dtype=np.uint64))):
        with pytest.raises(_ffi.MsimError):
            _ffi.dbg_reads_render(_ffi.reads_params(**{**good, **bad}), case.contigs, 0, 0, 1)
    with pytest.raises(ValueError):                        # no eligible contig
        _ffi.dbg_reads_render(_ffi.reads_params(**{**good, "frag_min": 4000}), case.contigs, 0, 0, 1)
    with pytest.raises(_ffi.MsimError):                    # mate 2 of a single-end run
        _ffi.dbg_reads_render(_ffi.reads_params(**{**good, "paired": False}), case.contigs, 1, 0, 1)
