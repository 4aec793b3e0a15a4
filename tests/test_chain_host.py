"""CPU tier: the liftover chain of a record table -- ``msim_render_chain`` (csrc/render.cpp) -- and the ``--chain`` option.

* the host renderer writes, byte for byte, what ``tests/chain_ref.py`` reads off the rewrite loop's walk: on hand-built tables
  (every type alone at the contig's edges, merged runs, leading and trailing gaps, contigs without an aligned base, numbers of
  1 to 10 digits) and on tables the host planner makes (SV mix, translocations);
* what a chain SAYS holds on the mutated bytes ``apply_ref.apply`` produces: every block is the same bases on both sides (SNP
  positions apart), the reference bases outside every block are exactly the deleted and the inverted ones, qSize is the
  mutated length;
* the size call and the refusal of a short buffer;
* the parser's ``args.outchain`` and the three refusals of ``__main__``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import apply_ref
import chain_cases
import chain_ref
import mutation_simulator_amd as msa
from chain_cases import DE, IV, SN, TL
from helpers import CASES, case_input_bytes, case_meta, parse_fasta_bytes
from mutation_simulator_amd import _ffi

HAND = chain_cases.hand_cases()
HUGE = chain_cases.huge_cases()


def both(recs, length, name="chr", chain_id=1):
    got = _ffi.render_chain(recs, length, name, name, chain_id)
    want = chain_ref.render(recs, length, name, name, chain_id)
    assert got == want, (got[:400], want[:400])
    return got


# ------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_tables(name):
    recs, _, length = HAND[name]
    text = both(recs, length, name, 3)
    if name.startswith("wholly_deleted"):
        assert text == b""
    if name in ("no_records", "snp_only"):
        assert text == f"chain {length} {name} {length} + 0 {length} {name} {length} + 0 {length} 3\n{length}\n\n".encode()


@pytest.mark.parametrize("name", sorted(HUGE))
def test_numbers_up_to_ten_digits(name):
    recs, _, length = HUGE[name]
    text = both(recs, length)
    assert length == 4294967295 and b" 4294967295 " in text


def test_digit_counts_covered():
    text = both(*[HUGE["ten_digit_blocks"][i] for i in (0, 2)])
    widths = {len(x) for line in text.decode().split("\n")[1:] for x in line.split("\t") if x}
    assert {1, 9, 10} <= widths


def test_empty_contig_and_empty_names():
    none = np.zeros(0, dtype=_ffi.RECORD_DTYPE)
    assert both(none, 0) == b""
    assert both(none, 5, "", 0) == b"chain 5  5 + 0 5  5 + 0 5 0\n5\n\n"
    assert both(none, 5, "a b", 2 ** 40).endswith(b" 1099511627776\n5\n\n")


def test_two_names():
    recs, _, length = HAND["DE_middle"]
    got = _render_raw(recs, length, b"ref", b"mut", 9)
    assert got == chain_ref.render(recs, length, "ref", "mut", 9)


def _render_raw(recs, length, t, q, cid, cap=None):
    lib = _ffi.load()
    recs = np.ascontiguousarray(recs, dtype=_ffi.RECORD_DTYPE)
    need = C.c_uint64()
    assert lib.msim_render_chain(recs.ctypes.data, len(recs), length, t, q, cid, None, 0, C.byref(need)) == _ffi.OK
    out = np.zeros(need.value if cap is None else cap, dtype=np.uint8)
    rc = lib.msim_render_chain(recs.ctypes.data, len(recs), length, t, q, cid, out.ctypes.data, len(out), C.byref(need))
    assert rc == _ffi.OK, rc
    return out[:need.value].tobytes()


def test_size_call_and_short_buffer():
    lib = _ffi.load()
    recs, _, length = HAND["every_type_with_snps_between"]
    want = chain_ref.render(recs, length, "c", "c", 1)
    need = C.c_uint64()
    assert lib.msim_render_chain(recs.ctypes.data, len(recs), length, b"c", b"c", 1, None, 0, C.byref(need)) == _ffi.OK
    assert need.value == len(want)
    out = np.full(len(want) + 8, 0x55, dtype=np.uint8)
    need.value = 0
    assert lib.msim_render_chain(recs.ctypes.data, len(recs), length, b"c", b"c", 1, out.ctypes.data, len(want) - 1,
                                 C.byref(need)) == _ffi.ERR_ARG
    assert need.value == len(want) and (out == 0x55).all()               # refused before a byte was written
    assert lib.msim_render_chain(recs.ctypes.data, len(recs), length, b"c", b"c", 1, out.ctypes.data, len(want),
                                 C.byref(need)) == _ffi.OK
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0x55).all()
    assert _render_raw(recs, length, b"c", b"c", 1, cap=len(want) + 100) == want
    # bad arguments
    assert lib.msim_render_chain(None, 1, length, b"c", b"c", 1, None, 0, C.byref(need)) == _ffi.ERR_ARG
    assert lib.msim_render_chain(recs.ctypes.data, len(recs), length, None, b"c", 1, None, 0, C.byref(need)) == _ffi.ERR_ARG
    assert lib.msim_render_chain(recs.ctypes.data, len(recs), length, b"c", b"c", 1, None, 0, None) == _ffi.ERR_ARG


# ------------------------------------------------------------------------------ what the chain says, on the mutated bytes
def check_semantics(recs, pool_len, length, seed=5):
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    bases, pool = acgt[rs.randint(0, 4, length)], acgt[rs.randint(0, 4, pool_len)]
    res = apply_ref.apply(bases, recs, pool)
    assert res.key_error is None
    text = _ffi.render_chain(recs, length, "s", "s", 1)
    if not text:
        gone = np.zeros(length, dtype=bool)
        for r in recs[np.isin(recs["type"], (DE, TL, IV))]:
            gone[r["pos"]:r["stop"] + 1] = True
        assert gone.all()                                                 # no chain: no base is aligned
        return
    (ch,) = chain_ref.parse(text)
    assert ch["tSize"] == length and ch["qSize"] == res.out_len and ch["score"] == sum(n for _, _, n in ch["blocks"])
    assert 0 <= ch["tStart"] < ch["tEnd"] <= length and 0 <= ch["qStart"] < ch["qEnd"] <= res.out_len
    snp = np.zeros(length, dtype=bool)
    snp[recs["pos"][recs["type"] == SN]] = True
    covered = np.zeros(length, dtype=bool)
    for t, q, n in ch["blocks"]:
        same = bases[t:t + n] == res.seq[q:q + n]
        assert (same | snp[t:t + n]).all(), (t, q, n)
        assert not covered[t:t + n].any()
        covered[t:t + n] = True
    gone = np.zeros(length, dtype=bool)
    for r in recs[np.isin(recs["type"], (DE, TL, IV))]:
        gone[r["pos"]:r["stop"] + 1] = True
    assert (covered == ~gone).all()


@pytest.mark.parametrize("name", sorted(HAND))
def test_semantics_on_hand_built_tables(name):
    check_semantics(*HAND[name])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_semantics_on_random_tables_with_merged_runs(seed):
    check_semantics(*chain_cases.counted(300, snp_every=seed - 1, merge_from=40 * seed, merge_len=25, seed=seed))


# ------------------------------------------------------------------------------ host planner tables
SV_MIX = ["args", "-sn", "0.005", "-in", "0.001", "-inmax", "50", "-de", "0.001", "-demax", "50", "-du", "0.0005", "-dumin", "50",
          "-dumax", "500", "-iv", "0.0005", "-ivmin", "50", "-ivmax", "500", "-titv", "1.0"]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_host_planner_sv_mix(seed):
    from inputs import random_bases
    from test_apply_ref_host import _contig, _plan_host
    contigs = [_contig("s1", random_bases(120_000, seed)), _contig("s2", random_bases(900, seed + 100))]
    _, tables = _plan_host(SV_MIX, contigs, seed, seed + 1)
    seen = set()
    for i, c in enumerate(contigs):
        recs, pool = tables[i]
        both(recs, len(c["bases"]), c["name"], i + 1)
        seen |= set(recs["type"].tolist())
        if i == 1:
            check_semantics(recs, len(pool), len(c["bases"]))
    assert seen == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("name", ["tl_heavy", "readme_mix_tl"])
def test_host_planner_translocations(name):
    from test_apply_ref_host import _plan_host
    meta = case_meta(name)
    contigs = parse_fasta_bytes(case_input_bytes(meta))
    _, tables = _plan_host(meta["argv_tail"], contigs, meta["seed_py"], meta["seed_np"])
    types = set()
    for i, c in enumerate(contigs):
        recs, pool = tables.get(i, (np.zeros(0, dtype=_ffi.RECORD_DTYPE), np.zeros(0, dtype=np.uint8)))
        text = both(recs, len(c["bases"]), c["name"], i + 1)
        (ch,) = chain_ref.parse(text)
        assert ch["qSize"] == apply_ref.apply(c["bases"], recs, pool).out_len
        types |= set(recs["type"].tolist())
    assert {6, 7} <= types


# ------------------------------------------------------------------------------ the option
def _args(argv):
    with contextlib.redirect_stderr(io.StringIO()):
        return msa.get_args(argv)


def test_outchain_names(tmp_path):
    a = _args(["dir/genome.fa", "--chain", "args", "-sn", "0.01"])
    assert a.chain and str(a.outchain) == "genome_ms.chain" and str(a.outvcf) == "genome_ms.vcf"
    a = _args(["dir/genome.fa", "args", "-sn", "0.01"])
    assert not a.chain and str(a.outchain) == "genome_ms.chain"
    a = _args(["genome.fa", "-o", "out/base", "--chain", "--bgzip", "args", "-sn", "0.01"])
    assert str(a.outchain) == "out/base_ms.chain"                       # plain under --bgzip ...
    assert str(a.outfasta) == "out/base_ms.fa.gz" and str(a.outvcf) == "out/base_ms.vcf.gz"     # ... which renames the other two
    a = _args(["genome.fa", "-o", "out/", "--chain", "rmt", "x.rmt"])
    assert str(a.outchain) == "out_ms.chain"
    a = _args(["genome.fasta", "-o", ".", "--chain", "vcf", "t.vcf"])
    assert str(a.outchain) == "genome_ms.chain" and str(a.outfasta) == "genome_ms.fasta"
    # a BGZF input: the .gz of its name is dropped before the names are derived
    from mutation_simulator_amd import bgzf
    gz = tmp_path / "asm.fa.gz"
    gz.write_bytes(bgzf.zlib_bgzf(b">a\nACGT\n"))
    a = _args([str(gz), "--chain", "args", "-sn", "0.01"])
    assert str(a.outchain) == "asm_ms.chain" and str(a.outfasta) == "asm_ms.fa"
    a = _args([str(gz), "--chain", "--bgzip", "args", "-sn", "0.01"])
    assert str(a.outchain) == "asm_ms.chain" and str(a.outfasta) == "asm_ms.fa.gz"


def _refused(monkeypatch, argv, message):
    """main(argv) exits with the message as an error, before a device is opened."""
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


def test_chain_refused_with_it_mode(monkeypatch, tmp_path):
    meta = case_meta("it_only_4ctg")
    infile = tmp_path / meta["infile_name"]
    infile.write_bytes(case_input_bytes(meta))
    _refused(monkeypatch, ["-c", "--chain", "-o", str(tmp_path / "out"), str(infile), "it", "0.5"],
             "--chain does not apply to the interchromosomal pass (it)")
    assert not list(tmp_path.glob("out*"))


def test_chain_refused_with_it_lines_in_rmt(monkeypatch, tmp_path):
    meta = case_meta("it_rmt_mutations")
    infile = tmp_path / meta["infile_name"]
    infile.write_bytes(case_input_bytes(meta))
    rmt = tmp_path / "case.rmt"
    rmt.write_text((CASES / "it_rmt_mutations" / "case.rmt").read_text())
    _refused(monkeypatch, ["-c", "--chain", "-o", str(tmp_path / "out"), str(infile), "rmt", str(rmt)],
             "--chain does not apply to the interchromosomal pass (it lines in the RMT)")
    assert not list(tmp_path.glob("out*"))


def test_chain_refused_with_several_gpus(monkeypatch, tmp_path):
    _refused(monkeypatch, ["-c", "--chain", "--gpus", "2", "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"), "args", "-sn", "0.01"],
             "--chain needs a single-GPU run (--gpus 1)")
    assert not list(tmp_path.glob("out*"))
