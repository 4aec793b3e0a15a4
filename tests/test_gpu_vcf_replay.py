"""GPU tier of the ``vcf`` mode: the device parser (csrc/vcf_parse.hip) against the host parser, record for record and pool
byte for byte, and the closed loop ``args`` -> VCF -> ``vcf`` -> the same Fasta bytes, through the command line.

Every command-line run is a child process with a time limit of its own.  Round trips are exact where no suppressed record
changes a byte (an SNP N -> N, a palindromic inversion, an empty translocation insert), which is always the case on ACGTN
inputs: the size tests use those, the IUPAC ground is covered by the goldens.
"""
from __future__ import annotations

import contextlib
import io
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import apply_ref
import test_vcf_replay_host as host
from helpers import CASES, case_input_bytes, case_meta, parse_fasta_bytes
from mutation_simulator_amd import _ffi, vcf_replay

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
README_FLAGS = ["-sn", "0.01", "-in", "0.01", "-de", "0.01", "-du", "0.01", "-iv", "0.01", "-tl", "0.01"]


def cli(argv, limit=600):
    env = dict(os.environ, PYTHONPATH=str(ROOT / "mutation-simulator_amd"))
    p = subprocess.run([sys.executable, "-m", "mutation_simulator_amd", "-q", "-c"] + [str(a) for a in argv], env=env,
                       capture_output=True, text=True, timeout=limit)
    if p.returncode in (134, 139, 124, 137, -6, -11, -9):          # a child that died on the GPU: nothing more is started on it
        pytest.exit(f"{argv}: child ended with {p.returncode}: {p.stderr[-2000:]}", returncode=3)
    return p


def cli_ok(argv, limit=600):
    p = cli(argv, limit)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-2000:])


def same_file(a: Path, b: Path):
    assert a.stat().st_size == b.stat().st_size, (a, b, a.stat().st_size, b.stat().st_size)
    assert subprocess.run(["cmp", str(a), str(b)], capture_output=True, timeout=600).returncode == 0, (a, b)


def gen_genome(path: Path, lengths, seed: int, bpls=(60,), n_runs: bool = True):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for i, L in enumerate(lengths):
            bpl = bpls[i % len(bpls)]
            f.write(f">ctg{i + 1} synthetic len={L}\n".encode())
            b = lut[rng.integers(0, 4, L, dtype=np.uint8)]
            if n_runs and L > 5000:
                b[L // 3: L // 3 + min(L // 50, 50_000)] = ord("N")
            full = L // bpl
            body = np.empty((full, bpl + 1), dtype=np.uint8)
            body[:, :bpl] = b[:full * bpl].reshape(full, bpl)
            body[:, bpl] = 10
            f.write(body.tobytes())
            if L > full * bpl:
                f.write(b[full * bpl:].tobytes() + b"\n")
    return path


def parse_both(contigs, vcf: bytes):
    """(device tables, host tables, device groups, host groups)."""
    text = np.frombuffer(vcf, dtype=np.uint8)
    out = []
    for device in (0, -1):
        eng = _ffi.Engine(device=device)
        try:
            cids = [eng.add_contig(c["bases"]) for c in contigs]
            for cid, c in zip(cids, contigs):
                eng.vcf_host_bases(cid, c["bases"])
            vcf_replay.plan_all(eng, text, [c["name"] for c in contigs], cids)
            groups = eng.vcf_groups().copy()
            out.append(([tuple(a.copy() for a in eng.fetch_records(cid)) for cid in cids], groups))
        finally:
            eng.close()
    (dev, dev_groups), (hst, hst_groups) = out
    return dev, hst, dev_groups, hst_groups


def assert_twins(contigs, vcf: bytes):
    dev, hst, dg, hg = parse_both(contigs, vcf)
    assert dg.tobytes() == hg.tobytes()
    for c, (dr, dp), (hr, hp) in zip(contigs, dev, hst):
        assert len(dr) == len(hr) and dr.tobytes() == hr.tobytes(), c["name"]
        assert dp.tobytes() == hp.tobytes(), c["name"]
    return dev


# ------------------------------------------------------------------------------ 1. the goldens through the command line
@pytest.mark.parametrize("name", host.GOLDENS)
def test_golden_through_cli(name, tmp_path):
    meta = case_meta(name)
    inp = tmp_path / meta["infile_name"]
    inp.write_bytes(case_input_bytes(meta))
    cli_ok(["-o", tmp_path / "out", inp, "vcf", CASES / name / "expected_ms.vcf"], 300)
    got = tmp_path / ("out_ms" + inp.suffix)
    assert got.read_bytes() == (CASES / name / "expected_ms.fa").read_bytes()
    assert not (tmp_path / "out_ms.vcf").exists()


# ------------------------------------------------------------------------------ 2. device parser == host parser
@pytest.mark.parametrize("name", host.GOLDENS)
def test_device_equals_host_on_goldens(name):
    fasta, vcf, _ = host._golden(name)
    assert_twins(parse_fasta_bytes(fasta), vcf)


@pytest.mark.parametrize("lengths,flags", [([120_000_000], ["-sn", "0.01"]), ([30_000_000], README_FLAGS)], ids=["snp_120mb", "readme_tl_30mb"])
def test_device_equals_host_at_size(lengths, flags, tmp_path):
    inp = gen_genome(tmp_path / "g.fa", lengths, 11)
    cli_ok(["--seed", "5", "-o", tmp_path / "out", inp, "args"] + flags, 900)
    vcf = (tmp_path / "out_ms.vcf").read_bytes()
    contigs = parse_fasta_bytes(inp.read_bytes())
    dev = assert_twins(contigs, vcf)
    assert sum(len(r) for r, _ in dev) > 100_000


# ------------------------------------------------------------------------------ 3. round trip at size
@pytest.mark.parametrize("flags", [["-sn", "0.01", "-titv", "2"], README_FLAGS], ids=["snp", "readme"])
def test_round_trip_at_size(flags, tmp_path):
    inp = gen_genome(tmp_path / "g.fa", [60_000_000, 25_000_000, 15_000_000, 4_000_000, 123_457], 21, bpls=(60, 70, 80))
    cli_ok(["--seed", "9", "-o", tmp_path / "out", inp, "args"] + flags, 900)
    cli_ok(["-o", tmp_path / "back", inp, "vcf", tmp_path / "out_ms.vcf"], 900)
    same_file(tmp_path / "out_ms.fa", tmp_path / "back_ms.fa")


def test_round_trip_compressed_three_ways(tmp_path):
    inp = gen_genome(tmp_path / "g.fa", [3_000_000, 700_000, 90_000], 22, bpls=(60, 50))
    cli_ok(["--seed", "3", "--bgzip", "-o", tmp_path / "z", inp, "args"] + README_FLAGS, 600)
    cli_ok(["--seed", "3", "-o", tmp_path / "p", inp, "args"] + README_FLAGS, 600)
    # a BGZF VCF
    cli_ok(["-o", tmp_path / "a", inp, "vcf", tmp_path / "z_ms.vcf.gz"], 600)
    same_file(tmp_path / "p_ms.fa", tmp_path / "a_ms.fa")
    # BGZF output of the replay
    cli_ok(["--bgzip", "-o", tmp_path / "b", inp, "vcf", tmp_path / "p_ms.vcf"], 600)
    same_file(tmp_path / "z_ms.fa.gz", tmp_path / "b_ms.fa.gz")
    # a BGZF genome as input
    eng = _ffi.Engine(0)
    try:
        (tmp_path / "g.fa.gz").write_bytes(eng.bgzf_compress(inp.read_bytes()))
    finally:
        eng.close()
    cli_ok(["-o", tmp_path / "c", tmp_path / "g.fa.gz", "vcf", tmp_path / "p_ms.vcf"], 600)
    same_file(tmp_path / "p_ms.fa", tmp_path / "c_ms.fa")
    # plain gzip is refused as the Fasta loader refuses it
    import gzip
    (tmp_path / "plain.vcf.gz").write_bytes(gzip.compress((tmp_path / "p_ms.vcf").read_bytes()))
    p = cli(["-o", tmp_path / "d", inp, "vcf", tmp_path / "plain.vcf.gz"], 600)
    assert p.returncode != 0 and "BGZF" in p.stderr and not (tmp_path / "d_ms.fa").exists()


# ------------------------------------------------------------------------------ 4. thousands of contigs
def test_round_trip_many_scaffolds(tmp_path):
    rng = np.random.default_rng(4)
    lengths = [int(x) for x in rng.integers(37, 15_000, 3000)] + [900_000] + [int(x) for x in rng.integers(37, 15_000, 1000)]
    inp = gen_genome(tmp_path / "g.fa", lengths, 23, bpls=(60, 70, 80, 61))
    flags = ["-sn", "0.01", "-in", "0.002", "-de", "0.002", "-du", "0.001", "-iv", "0.001", "-tl", "0.001"]
    cli_ok(["--seed", "8", "-o", tmp_path / "out", inp, "args"] + flags, 900)
    cli_ok(["-o", tmp_path / "back", inp, "vcf", tmp_path / "out_ms.vcf"], 900)
    same_file(tmp_path / "out_ms.fa", tmp_path / "back_ms.fa")


# ------------------------------------------------------------------------------ 5. long lines, every alignment
def _rand_bases(L, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, L, dtype=np.uint8)].copy()


def test_long_lines():
    """One deletion, one inversion and one duplication of several megabases each: no lane's work grows with them."""
    bases = _rand_bases(24_000_000, 31)
    pool = _rand_bases(2_000_000, 32)
    recs = host._table((1000, 1000, 0, 1), (2_000, 5_002_000, 0, host.DE), (6_000_000, 9_100_000, 0, host.IV),
                       (10_000_000, 10_000_000 + len(pool) - 1, 0, host.IN), (11_000_000, 15_000_003, 0, host.DU),
                       (20_000_000, 23_999_999, 0, host.DE))
    contigs = [{"name": "long1", "bases": bases}]
    vcf = b"##x\n" + _ffi.render_vcf(recs, pool, bases, "long1")
    dev = assert_twins(contigs, vcf)
    want = apply_ref.apply(bases, recs, pool).seq
    eng = _ffi.Engine(0)
    try:
        cid = eng.add_contig(bases)
        vcf_replay.plan_all(eng, np.frombuffer(vcf, dtype=np.uint8), ["long1"], [cid])
        eng.apply_contig(cid)
        assert eng.fetch_sequence(cid).tobytes() == want.tobytes()
    finally:
        eng.close()
    assert len(dev[0][0]) == 6
    # one wrong byte deep inside a long part is found, and both parsers say the same
    nl = np.flatnonzero(np.frombuffer(vcf, dtype=np.uint8) == 10)
    for at in (int(nl[1]) + 3_000_000, int(nl[2]) + 4_000_000, int(nl[3]) + 1_000_000, int(nl[4]) + 9_000_000):   # DEL REF, INV ALT, INS, DUP ALT
        bad = bytearray(vcf)
        bad[at] = ord("A") if bad[at] != ord("A") else ord("C")
        msgs = []
        for device in (0, -1):
            eng = _ffi.Engine(device)
            try:
                cid = eng.add_contig(bases)
                eng.vcf_host_bases(cid, bases)
                try:
                    vcf_replay.plan_all(eng, np.frombuffer(bytes(bad), dtype=np.uint8), ["long1"], [cid])
                    msgs.append("accepted")
                except vcf_replay.VcfReplayError as e:
                    msgs.append(str(e))
            finally:
                eng.close()
        assert msgs[0] == msgs[1], msgs
        assert msgs[0].startswith("VCF line ") or at == int(nl[3]) + 1_000_000, msgs      # (another letter in an insert is an insert)


def test_every_alignment():
    """Thousands of short structural lines on contigs with names of every length: REF, ALT and the line end fall on every
    offset mod 16 and across the 16-byte pieces, the scan tiles (2048 items) and the 256-line blocks."""
    rng = np.random.default_rng(41)
    contigs, tables = [], []
    for k in range(17):
        L = 400_000
        bases = _rand_bases(L, 50 + k)
        rows, pool, pos = [], bytearray(), int(rng.integers(1, 40))
        while pos < L - 200:
            typ = int(rng.choice([host.SN, host.IN, host.DE, host.DU, host.IV]))
            n = int(rng.integers(1, 70))
            if typ == host.SN:
                rows.append((pos, pos, 0, typ, int(rng.integers(0, 3))))
            elif typ == host.IN:
                rows.append((pos, pos + n - 1, len(pool), typ))
                pool += bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tolist())
            else:
                rows.append((pos, pos + n - 1, 0, typ))
            pos += (n if typ not in (host.SN, host.IN) else 1) + int(rng.integers(1, 60))
        contigs.append({"name": "s" + "x" * k, "bases": bases})
        tables.append((host._table(*rows), np.frombuffer(bytes(pool), dtype=np.uint8)))
    vcf = b"##h\n" + b"".join(_ffi.render_vcf(r, p, c["bases"], c["name"]) for c, (r, p) in zip(contigs, tables))
    seen_ref, seen_end = set(), set()
    off = 0
    for ln in vcf.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        if len(f) == 10:
            seen_ref.add((off + len(f[0]) + len(f[1]) + len(f[2]) + 3) % 16)
            seen_end.add((off + len(ln)) % 16)
        off += len(ln) + 1
    assert seen_ref == set(range(16)) and seen_end == set(range(16))
    dev = assert_twins(contigs, vcf)
    for c, (recs, pool), (dr, dp) in zip(contigs, tables, dev):
        w_recs, w_pool = host.canonical(recs, pool, c["bases"])
        assert dr.tobytes() == w_recs.tobytes() and dp.tobytes() == w_pool.tobytes(), c["name"]


# ------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("name", sorted(host.REFUSALS))
def test_refusal_same_as_host(name):
    lines, number, reason = host.REFUSALS[name]
    want = host._refusal(lines)
    names = [c["name"] for c in host.GENOME]
    eng = _ffi.Engine(0)
    try:
        cids = [eng.add_contig(c["bases"]) for c in host.GENOME]
        with pytest.raises((vcf_replay.VcfReplayError, ValueError)) as ei:
            vcf_replay.plan_all(eng, np.frombuffer(host.HDR + b"".join(lines), dtype=np.uint8), names, cids)
        assert str(ei.value) == want and str(ei.value).startswith(f"VCF line {number}: ")
        # the context is usable afterwards
        vcf_replay.plan_all(eng, np.frombuffer(host.HDR + host.OK1, dtype=np.uint8), names, cids)
        eng.apply_contig(cids[0])
        assert eng.fetch_sequence(cids[0]).tobytes() == b"ATGTACGTAGCTAGCTNNACGTRYACGTACGT"
    finally:
        eng.close()


def test_refusal_through_cli_writes_nothing(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">c1 x\nACGTACGTAGCTAGCTNNACGTRYACGTACGT\n>c2\nTTGACCA\n")
    (tmp_path / "t.vcf").write_bytes(host.HDR + host.OK1 + host.line("c1", 9, "C", "T"))
    p = cli(["-o", tmp_path / "out", fa, "vcf", tmp_path / "t.vcf"], 300)
    assert p.returncode != 0 and "VCF line 4: REF does not match the genome" in p.stderr
    assert not (tmp_path / "out_ms.fa").exists()
    p = cli(["--gpus", "2", "-o", tmp_path / "out", fa, "vcf", tmp_path / "t.vcf"], 300)
    assert p.returncode != 0 and "single-GPU" in p.stderr


# ------------------------------------------------------------------------------ 7. no draw is taken
def test_generator_states_unchanged(tmp_path):
    from mutation_simulator_amd import __main__ as msa_main
    meta = case_meta("svmix_2ctg_200k")
    inp = tmp_path / meta["infile_name"]
    inp.write_bytes(case_input_bytes(meta))
    random.seed(123)
    np.random.seed(456)
    before = (random.getstate(), np.random.get_state()[1].tobytes(), np.random.get_state()[2])
    with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
        msa_main.main(["-q", "--seed", "77", "--rng", "fast", "-o", str(tmp_path / "out"), str(inp), "vcf",
                       str(CASES / "svmix_2ctg_200k" / "expected_ms.vcf")])
    assert (random.getstate(), np.random.get_state()[1].tobytes(), np.random.get_state()[2]) == before
    assert (tmp_path / "out_ms.fa").read_bytes() == (CASES / "svmix_2ctg_200k" / "expected_ms.fa").read_bytes()


# ------------------------------------------------------------------------------ 8. the FIRST offending line, the length bound
def _verdict(device, contigs, vcf: bytes) -> str:
    eng = _ffi.Engine(device)
    try:
        cids = [eng.add_contig(c["bases"]) for c in contigs]
        for cid, c in zip(cids, contigs):
            eng.vcf_host_bases(cid, c["bases"])
        try:
            vcf_replay.plan_all(eng, np.frombuffer(vcf, dtype=np.uint8), [c["name"] for c in contigs], cids)
            return "accepted"
        except (vcf_replay.VcfReplayError, ValueError) as e:
            return str(e)
    finally:
        eng.close()


_TWO_BASES = _rand_bases(4000, 77)
_TWO_S = _TWO_BASES.tobytes().decode()
_TI = {"A": "G", "G": "A", "C": "T", "T": "C"}


def _snp(pos1, wrong_ref=False):
    ref = _TWO_S[pos1 - 1]
    return host.line("two", pos1, _TI[ref] if wrong_ref else ref, ref if wrong_ref else _TI[ref])


def _flip(s, at):
    return s[:at] + ("A" if s[at] != "A" else "C") + s[at + 1:]


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


_REF40 = _TWO_S[100:140]
# a line whose short fields are fine and whose fault lies in the long part, behind the first 16 bytes of REF or ALT
EARLY = {
    "del_ref": (host.line("two", 101, _flip(_REF40, 30), _REF40[0], host.sv("DEL", 140, 39)), "REF does not match"),
    "inv_ref": (host.line("two", 101, _flip(_REF40, 20), _revcomp(_REF40), host.sv("INV", 140, 40)), "REF does not match"),
    "inv_alt": (host.line("two", 101, _REF40, _flip(_revcomp(_REF40), 22), host.sv("INV", 140, 40)), "ALT is not what"),
    "dup_alt": (host.line("two", 101, _REF40, _flip(_REF40 + _REF40, 61), host.sv("DUP", 140, 40)), "ALT is not what"),
    "ins_digit": (host.line("two", 101, _REF40[0], _REF40[0] + "ACGT" * 5 + "7" + "ACGT" * 5, host.sv("INS", 101, 41)), "no letter"),
    "allele_deep": (host.line("two", 101, _REF40, _REF40 + _REF40[:20] + "," + _REF40[21:], host.sv("DUP", 140, 40)), "multi-allelic"),
}
# a later line that the short-field lane or the neighbour check refuses
LATER = {
    "fields": b"two\t500\t.\tA\tG\t.\t.\t.\tGT\n",
    "snp_ref": _snp(500, wrong_ref=True),
    "order": _snp(250),
    "pos": host.line("two", 5000, "A", "G"),
    "sample": host.line("two", 500, "A", "G", sample="0"),
}


@pytest.mark.parametrize("later", sorted(LATER))
@pytest.mark.parametrize("early", sorted(EARLY))
def test_first_offending_line_of_two(early, later):
    """Line 4 fails in its long part, line 6 in its short fields or its order: both parsers name line 4."""
    bad, reason = EARLY[early]
    vcf = host.HDR + _snp(10) + bad + _snp(300) + LATER[later] + _snp(900)
    contigs = [{"name": "two", "bases": _TWO_BASES}]
    dev, hst = _verdict(0, contigs, vcf), _verdict(-1, contigs, vcf)
    assert dev == hst, (dev, hst)
    assert dev.startswith("VCF line 4: ") and reason in dev, dev


def test_two_reasons_on_one_line():
    """A line that is out of order AND wrong in its long part: the smallest reason code, on both sides."""
    contigs = [{"name": "two", "bases": _TWO_BASES}]
    vcf = host.HDR + _snp(300) + EARLY["del_ref"][0] + _snp(900)
    dev, hst = _verdict(0, contigs, vcf), _verdict(-1, contigs, vcf)
    assert dev == hst == "VCF line 4: REF does not match the genome", (dev, hst)
    # the long-part fault of line 3 in front of an order fault of line 4
    vcf = host.HDR + EARLY["inv_alt"][0] + _snp(120) + _snp(900)
    dev, hst = _verdict(0, contigs, vcf), _verdict(-1, contigs, vcf)
    assert dev == hst and dev.startswith("VCF line 3: ALT is not what"), (dev, hst)


LENGTH_MESSAGE = "VCF line 3: mutated length of 2^32 or more"      # what test_vcf_replay_host.test_refusal_mutated_length pins


def _usable_afterwards(eng):
    cids = [eng.add_contig(c["bases"]) for c in host.GENOME]
    vcf_replay.plan_all(eng, np.frombuffer(host.HDR + host.OK1, dtype=np.uint8), [c["name"] for c in host.GENOME], cids)
    eng.apply_contig(cids[0])
    assert eng.fetch_sequence(cids[0]).tobytes() == b"ATGTACGTAGCTAGCTNNACGTRYACGTACGT"


def test_refusal_mutated_length_on_device():
    """The device twin of the host test: a contig of 2^32 - 50 bases and a duplication of 60."""
    L = (1 << 32) - 50
    bases = np.full(L, ord("A"), dtype=np.uint8)
    eng = _ffi.Engine(0)
    try:
        cid = eng.add_contig(bases)
        del bases
        eng.vcf_load(host.HDR + host.line("big", 5, "A" * 60, "A" * 120, host.sv("DUP", 64, 60)))
        with pytest.raises(ValueError) as ei:
            eng.vcf_plan_contig(cid, 0)
        assert str(ei.value) == LENGTH_MESSAGE
        # one base less than the bound is taken: 2^32 - 50 + 49
        eng.vcf_load(host.HDR + host.line("big", 5, "A" * 49, "A" * 98, host.sv("DUP", 53, 49)))
        eng.vcf_plan_contig(cid, 0)
        recs, pool = eng.fetch_records(cid)
        assert [tuple(r)[:4] for r in recs.tolist()] == [(4, 52, 0, host.DU)] and len(pool) == 0
    finally:
        eng.close()
    eng = _ffi.Engine(0)
    try:
        _usable_afterwards(eng)
    finally:
        eng.close()


def test_refusal_inserts_sum_past_2_32_inside_one_scan_tile():
    """2048 insertions of 2^21 bytes each -- one scan tile of insert lengths -- on a small contig: their sum is 2^32, where
    the 32-bit pool offsets wrap; the 64-bit sum of the growth decides, and no pool byte is written."""
    bases = _rand_bases(4096, 78)
    s = bases.tobytes().decode()
    ins = b"ACGT" * (1 << 19)
    tail = b"\t.\t.\tSVTYPE=INS;END=1;SVLEN=2097152\tGT\t1\n"
    vcf = bytearray(host.HDR)
    for p in range(1, 2049):
        vcf += f"many\t{p}\t.\t{s[p - 1]}\t{s[p - 1]}".encode()
        vcf += ins
        vcf += tail
    eng = _ffi.Engine(0)
    try:
        cid = eng.add_contig(bases)
        eng.vcf_load(np.frombuffer(vcf, dtype=np.uint8))
        del vcf
        with pytest.raises(ValueError) as ei:
            eng.vcf_plan_contig(cid, 0)
        assert str(ei.value) == LENGTH_MESSAGE
        _usable_afterwards(eng)
    finally:
        eng.close()
