"""CPU tier: the restatement of the rewrite loop (tests/apply_ref.py) and the record-table test hook.

``apply_ref`` is the yardstick of tests/test_gpu_apply_tables.py, so it must not owe its correctness to the kernels:

* on the twelve edge cases of tests/golden/apply.json it reproduces the bytes the REAL reference wrote;
* on tables the host planner makes (host-only context) it reproduces the oracle's mutated Fasta for the same seeds -- IUPAC
  letters and N runs, an SV mix, the translocation goldens (whose expected Fasta is the real reference's) -- and the
  oracle's KeyError;
* ``msim_dbg_set_records`` refuses, before anything could be launched, every table the kernels are not written for.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import apply_ref
import mutation_simulator_amd as msa
from helpers import CASES, case_input_bytes, case_meta, load_json, parse_fasta_bytes
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import mutator as mm
from oracle import oracle as orc
from test_host_settings import dump_sim
from test_property_host import _Fasta, _Rec

APPLY = load_json("apply.json")


# ------------------------------------------------------------------------------ against the real reference's bytes
@pytest.mark.parametrize("case", APPLY["cases"], ids=lambda c: c["name"])
def test_restatement_reproduces_reference_goldens(case):
    assert case["exception"] is None
    recs, pool = apply_ref.golden_table(case)
    bases = np.frombuffer(case["sequence"].encode(), dtype=np.uint8)
    res = apply_ref.apply(bases, recs, pool)
    assert res.key_error is None
    assert res.seq.tobytes() == apply_ref.unwrap_fasta(case["fasta"]).tobytes()
    assert res.out_len == len(res.seq)


def test_golden_tables_cover_every_type_the_goldens_have():
    seen = set()
    for case in APPLY["cases"]:
        recs, _ = apply_ref.golden_table(case)
        seen |= set(recs["type"].tolist())
    assert seen == {1, 2, 3, 4, 5}
    # covered_skips: five of its eight entries start inside an earlier span and are never visited
    recs, _ = apply_ref.golden_table(next(c for c in APPLY["cases"] if c["name"] == "covered_skips"))
    assert recs["pos"].tolist() == [2, 12, 21, 26]


# ------------------------------------------------------------------------------ against the oracle, on planner tables
def _plan_host(argv_tail, contigs, seed_py, seed_np):
    """Settings -> host planner (host-only context), contig by contig on chained streams: (dumped settings, tables)."""
    fasta = _Fasta([_Rec(c["name"], c["bases"]) for c in contigs])
    for r, c in zip(fasta.recs, contigs):
        r.long_name = c["long_name"]
    with contextlib.redirect_stderr(io.StringIO()):
        args = msa.get_args(["x.fa"] + list(argv_tail))
        sim = msa.SimulationSettings.from_args(args, fasta, True)
    eng = _ffi.Engine(device=-1)
    eng.seed(seed_py, seed_np)
    eng.set_params(mm.params_descriptor(sim))
    tables = {}
    for chrom in sim.chromosomes:
        cid = eng.add_contig(contigs[chrom.number]["bases"])
        eng.plan_contig(cid, mm.plan_descriptors(chrom))
        recs, pool = eng.fetch_records(cid)
        tables[chrom.number] = (recs.copy(), pool.copy())
    eng.close()
    return dump_sim(sim), tables


def _contig(name, bases, lenc=60):
    return {"name": name, "long_name": name + " synthetic", "lenc": lenc, "bases": bases}


def _check_against_oracle(argv_tail, contigs, seed_py, seed_np):
    sim, tables = _plan_host(argv_tail, contigs, seed_py, seed_np)
    o = orc.Oracle()
    o.seed(seed_py, seed_np)
    fa, _, _, _ = o.run_genome(contigs, sim, "x.fa")
    want = parse_fasta_bytes(fa)
    assert len(want) == len(contigs)
    all_recs = []
    for i, c in enumerate(contigs):
        recs, pool = tables.get(i, (np.zeros(0, dtype=_ffi.RECORD_DTYPE), np.zeros(0, dtype=np.uint8)))
        res = apply_ref.apply(c["bases"], recs, pool)
        assert res.key_error is None
        assert res.seq.tobytes() == want[i]["bases"].tobytes(), (i, c["name"])
        all_recs.append(recs)
    return np.concatenate(all_recs), fa


def _iupac_bases(L, seed):
    """Random ACGT with IUPAC letters sprinkled in and runs of N."""
    rs = np.random.RandomState(seed)
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, L)].copy()
    at = rs.choice(L, L // 7, replace=False)
    b[at] = np.frombuffer(b"KSYMWRBDHVN", dtype=np.uint8)[rs.randint(0, 11, len(at))]
    for s in rs.choice(L - 600, 6, replace=False):
        b[s:s + int(rs.randint(1, 500))] = ord("N")
    return b


def test_planner_tables_iupac_and_n_runs():
    """SNPs, inversions and duplications over IUPAC letters and N runs.  titv is large: every SNP a transition, no KeyError."""
    contigs = [_contig("u1", _iupac_bases(60_000, 1)), _contig("u2", _iupac_bases(9_000, 2), lenc=70)]
    recs, _ = _check_against_oracle(["args", "-sn", "0.02", "-iv", "0.003", "-ivmax", "40", "-du", "0.003", "-dumax", "30", "-in", "0.002",
                                     "-de", "0.002", "-demax", "20", "-titv", "1e12"], contigs, 5, 6)
    assert set(recs["type"].tolist()) == {1, 2, 3, 4, 5} and np.all(recs["aux"][recs["type"] == 1] == 0)


def test_planner_tables_sv_mix():
    from inputs import random_bases
    contigs = [_contig("s1", random_bases(200_000, 3)), _contig("s2", random_bases(1_000, 4))]
    recs, _ = _check_against_oracle(["args", "-sn", "0.005", "-in", "0.001", "-inmax", "50", "-de", "0.001", "-demax", "50", "-du", "0.0005",
                                     "-dumin", "50", "-dumax", "500", "-iv", "0.0005", "-ivmin", "50", "-ivmax", "500", "-titv", "1.0"],
                                    contigs, 42, 43)
    assert set(recs["type"].tolist()) == {1, 2, 3, 4, 5} and set(recs["aux"][recs["type"] == 1].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", ["tl_heavy", "readme_mix_tl"])
def test_planner_tables_translocations(name):
    """The translocation goldens' settings, input and seeds: TL excised, TLI = converted or reverse-complemented copy of the
    linked span.  The oracle's Fasta here IS the real reference's (the stored expected file)."""
    meta = case_meta(name)
    contigs = parse_fasta_bytes(case_input_bytes(meta))
    recs, fa = _check_against_oracle(meta["argv_tail"], contigs, meta["seed_py"], meta["seed_np"])
    assert fa == (CASES / name / "expected_ms.fa").read_bytes()
    tli = recs[recs["type"] == 7]
    assert (recs["type"] == 6).sum() > 100 and len(tli) > 100
    assert (tli["aux"] & 1).any() and (~(tli["aux"] & 1).astype(bool)).any()          # both orientations occur


def test_key_error_base_and_position():
    """err_snp_on_U's settings: every SNP a transversion, the input an RNA.  The reference raises KeyError('U') at the first
    SNP that stands on a U; the walk is sequential, so that is the lowest such position."""
    meta = case_meta("err_snp_on_U")
    contigs = parse_fasta_bytes(case_input_bytes(meta))
    sim, tables = _plan_host(meta["argv_tail"], contigs, meta["seed_py"], meta["seed_np"])
    o = orc.Oracle()
    o.seed(meta["seed_py"], meta["seed_np"])
    with pytest.raises(KeyError) as ei:
        o.run_genome(contigs, sim, "x.fa")
    recs, pool = tables[0]
    res = apply_ref.apply(contigs[0]["bases"], recs, pool)
    on_u = recs["pos"][(recs["type"] == 1) & (recs["aux"] > 0) & (contigs[0]["bases"][recs["pos"]] == ord("U"))]
    assert res.seq is None and res.key_error == (ei.value.args[0], int(on_u.min())) and res.key_error[0] == "U"


# ------------------------------------------------------------------------------ the hook: validation and round trip
def _table(*rows):
    return np.array([tuple(r) + (0,) * (6 - len(r)) for r in rows], dtype=_ffi.RECORD_DTYPE)


L0 = 100
POOL0 = np.frombuffer(b"ACGTACGT", dtype=np.uint8)

REFUSED = {
    "type_0": _table((5, 5, 0, 0)),
    "type_8": _table((5, 5, 0, 8)),
    "stop_below_pos": _table((10, 9, 0, 3)),
    "insert_stop_below_pos": _table((10, 9, 0, 2)),
    "pos_beyond_contig": _table((L0, L0, 0, 1)),
    "stop_beyond_contig_DE": _table((90, L0, 0, 3)),
    "stop_beyond_contig_DU": _table((90, L0, 0, 4)),
    "stop_beyond_contig_IV": _table((90, L0, 0, 5)),
    "stop_beyond_contig_TL": _table((90, L0, 0, 6)),
    "tli_span_beyond_contig": _table((50, L0, 95, 7)),
    "equal_positions": _table((7, 7, 0, 1), (7, 7, 0, 1)),
    "decreasing_positions": _table((9, 9, 0, 1), (7, 7, 0, 1)),
    "record_inside_a_deletion": _table((10, 20, 0, 3), (15, 15, 0, 1)),
    "record_on_a_span_end": _table((10, 20, 0, 5), (20, 20, 0, 1)),
    "insert_beyond_pool": _table((10, 10 + 8, 0, 2)),
    "insert_offset_beyond_pool": _table((10, 10, 9, 2)),
    "insert_range_crosses_pool_end": _table((10, 12, 6, 2)),
    "snp_outcome_3": _table((10, 10, 0, 1, 3)),
    "snp_stop_off": _table((10, 11, 0, 1)),
}


@pytest.mark.parametrize("with_offsets", [False, True])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_hook_refuses(name, with_offsets):
    eng = _ffi.Engine(device=-1)
    cid = eng.add_contig(np.full(L0, ord("A"), dtype=np.uint8))
    with pytest.raises(_ffi.MsimError, match="libmsim error 1: record"):
        eng.set_records(cid, REFUSED[name], POOL0, with_offsets)
    with pytest.raises(_ffi.MsimError):                    # nothing was installed
        eng.fetch_records(cid)
    eng.close()


def test_hook_refuses_a_mutated_length_of_4_gib():
    """Host-only contexts plan from the length alone: a 2 GiB contig costs nothing.  Duplicating all of it gives 2^32 bases."""
    eng = _ffi.Engine(device=-1)
    cid = C.c_int()
    dummy = np.zeros(16, dtype=np.uint8)
    assert eng.lib.msim_add_contig(eng.h, C.c_void_p(dummy.ctypes.data), 1 << 31, C.byref(cid)) == _ffi.OK
    with pytest.raises(_ffi.MsimError, match="mutated length"):
        eng.set_records(cid.value, _table((0, (1 << 31) - 1, 0, 4)), POOL0)
    eng.set_records(cid.value, _table((1, (1 << 31) - 1, 0, 4)), POOL0, True)        # 2^32 - 1: the largest that fits
    assert eng.planned_out_len(cid.value) == ((1 << 32) - 1, True)
    eng.close()


def test_hook_accepts_what_the_planners_emit_and_round_trips():
    bases = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    recs = _table((0, 2, 5, 2), (1, 1, 0, 1, 2), (2, 9, 0, 3), (10, 10, 0, 4), (11, 30, 0, 5), (31, 40, 0, 6),
                  (41, 40, 31, 7, 3),             # TLI linked to the TL in front of it, reversed
                  (50, 0, 50, 7, 2),              # TLI that found no TL: start = pos, stop = 0, an empty span
                  (60, 99, 0, 3))
    want = apply_ref.apply(bases, recs, POOL0)
    for with_offsets in (False, True):
        eng = _ffi.Engine(device=-1)
        cid = eng.add_contig(bases)
        eng.set_records(cid, recs, POOL0, with_offsets)
        got, pool = eng.fetch_records(cid)
        assert got.tobytes() == recs.tobytes() and pool.tobytes() == POOL0.tobytes()
        assert eng.result_sizes(cid, applied=False)[1:] == (len(recs), len(POOL0))
        assert eng.planned_out_len(cid) == ((want.out_len, True) if with_offsets else (0, False))
        assert not eng.plan_was_empty(cid)
        # (the host renderer takes the table; the inversion of ACGT x 5 is its own reverse complement: no line, vcf_writer.py)
        assert _ffi.render_vcf(got, pool, bases, "c").count(b"\n") == len(recs) - 1
        eng.set_records(cid, recs[:0], POOL0[:0], with_offsets)         # an empty table replaces it
        assert eng.result_sizes(cid, applied=False)[1:] == (0, 0) and eng.plan_was_empty(cid)
        eng.close()


def test_whole_contig_deleted_is_a_valid_table():
    eng = _ffi.Engine(device=-1)
    cid = eng.add_contig(np.full(L0, ord("C"), dtype=np.uint8))
    eng.set_records(cid, _table((0, L0 - 1, 0, 3)), POOL0, True)
    assert eng.planned_out_len(cid) == (0, True)
    eng.close()
