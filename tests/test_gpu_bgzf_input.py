"""BGZF-compressed Fasta input on the GPU: the device inflate (csrc/bgzf.hip: k_bgzf_inflate) behind ``Engine.bgzf_inflate``
and the loader / CLI on top of it.  The reference for every check is Python's zlib; equality is exact everywhere.

One deviation from the letter of the plan for the uneven-ISIZE file: a STORED member cannot hold 65 536 bytes (header, the
stored blocks' 5-byte headers and the trailer would push BSIZE past its 16 bits), so that file carries deflated members of
ISIZE 65 536 and stored members of the largest size that fits (65 505 bytes)."""
from __future__ import annotations

import contextlib
import functools
import hashlib
import io
import random
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest

from deflate_build import _Bits
from helpers import CASES, all_case_names, case_input_bytes, case_meta, mask_vcf, sha256
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import __main__ as msa_main
from mutation_simulator_amd import bgzf

pytestmark = pytest.mark.gpu

B = bgzf.BGZF_BLOCK
STRATEGIES = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
              (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)]


@pytest.fixture(scope="module")
def engine():
    eng = _ffi.Engine(0)
    yield eng
    eng.close()


def _fasta_text(n_bases: int, seed: int, n_run: int = 0) -> bytes:
    rng = np.random.default_rng(seed)
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_bases)].copy()
    if n_run:
        a = n_bases // 3
        b[a:a + n_run] = ord("N")
    full = n_bases // 60
    body = np.empty((full, 61), dtype=np.uint8)
    body[:, :60] = b[:full * 60].reshape(full, 60)
    body[:, 60] = 10
    return b">chr1\n" + body.tobytes() + b[full * 60:].tobytes()


def _repeats() -> bytes:
    rng = np.random.default_rng(3)
    parts = []
    for d in (3, 17, 255, 256, 1000, 4096, 20000, 32768):
        chunk = rng.integers(65, 91, d, dtype=np.uint8).tobytes()
        parts.append(chunk * max(2, 40000 // d))
    return b"".join(parts)


def _corpora() -> dict:
    return {
        "fasta": _fasta_text(1_000_000, 1, n_run=100_000),
        "vcf_dense": (CASES / "titv0_dense" / "expected_ms.vcf").read_bytes(),
        "vcf_mix": (CASES / "readme_mix_tl" / "expected_ms.vcf").read_bytes(),
        "n_run": b"N" * (10 << 20),
        "random": np.random.default_rng(7).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes(),
        "repeats": _repeats(),
    }


CORPORA = _corpora()


def _first_btype(payload: bytes) -> int:
    return (payload[0] >> 1) & 3


@functools.lru_cache(maxsize=None)
def _zlib_file(name: str, level: int, strategy: int) -> bytes:
    return bgzf.zlib_bgzf(CORPORA[name], level, strategy)


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_decoder_against_zlib(engine, name):
    for level, strategy in STRATEGIES:
        assert engine.bgzf_inflate(_zlib_file(name, level, strategy)) == CORPORA[name], (name, level, strategy)


def test_zlib_files_hold_every_block_type():
    """Stored, fixed and dynamic blocks all occur in what test_decoder_against_zlib decodes (BTYPE of each member's first
    block)."""
    seen = set()
    for name in sorted(CORPORA):
        for level, strategy in STRATEGIES:
            seen |= {_first_btype(m[4]) for m in bgzf.parse_members(_zlib_file(name, level, strategy)) if m[2]}
    assert seen == {0, 1, 2}, seen


def _multi_block_member(blk: bytes, level: int = 6) -> bytes:
    """One member whose deflate data holds several blocks by construction (a full flush in the middle of its data)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    third = len(blk) // 3
    payload = (c.compress(blk[:third]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(blk[third:2 * third])
               + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(blk[2 * third:]) + c.flush())
    return bgzf.make_member(blk, payload)


def test_several_deflate_blocks_per_member(engine):
    data = CORPORA["fasta"][:5 * B + 123] + CORPORA["vcf_dense"][:2 * B]
    gz = b"".join(_multi_block_member(data[a:a + B]) for a in range(0, len(data), B)) + bgzf.EOF_BLOCK
    assert bgzf.check_file(gz) == data
    for m in bgzf.parse_members(gz)[:-1]:                       # (at least: data block, empty stored block, data block ...)
        d = zlib.decompressobj(-15)
        assert len(d.decompress(m[4])) == m[2] and d.eof
        assert m[4].count(b"\x00\x00\xff\xff") >= 2             # the flush markers: empty stored blocks inside the member
    assert engine.bgzf_inflate(gz) == data


def test_members_of_uneven_size(engine):
    text = CORPORA["fasta"]
    rnd = CORPORA["random"]
    members, want, at = [], [], 0
    for k, n in enumerate([1, 2, 3, 5, 64, 255, 256, 4097, 65279, B, 0, 65536, 17, 65536, 65505, 40000, 65505, 1]):
        if n == 65505:                                          # the largest stored member that fits BSIZE: one final stored block
            blk = rnd[k * 100:k * 100 + n]
            m = bgzf.make_member(blk, b"\x01" + struct.pack("<HH", n, n ^ 0xFFFF) + blk)
            assert zlib.decompress(m[18:-8], -15) == blk
        else:
            blk = text[at:at + n]
            at += n
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            m = bgzf.make_member(blk, c.compress(blk) + c.flush()) if n else bgzf.EOF_BLOCK
        assert len(m) <= 65536
        members.append(m)
        want.append(blk)
    gz = b"".join(members) + bgzf.EOF_BLOCK
    assert [m[2] for m in bgzf.parse_members(gz)].count(65536) == 2
    assert _ffi.bgzf_probe(gz) == (sum(map(len, want)), len(members) + 1)
    assert engine.bgzf_inflate(gz) == b"".join(want)


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_round_trip_of_our_encoder(engine, name):
    data = CORPORA[name]
    gz = engine.bgzf_compress(data)
    out = engine.host_buffer(len(data))
    got, ms = engine.bgzf_inflate(gz, out=out, timed=True)      # (into page-locked memory, as the loader does)
    assert got.tobytes() == data and ms > 0


def test_empty_file(engine):
    assert engine.bgzf_inflate(bgzf.EOF_BLOCK) == b""
    assert engine.bgzf_inflate(bgzf.EOF_BLOCK * 3) == b""


# ------------------------------------------------------------------ corrupted members: input validation
def _distance_before_start() -> bytes:
    """A fixed-Huffman block: literal 'A', then <length 3, distance 5> with one byte produced so far."""
    b = _Bits()
    b.put(1, 1)
    b.put(1, 2)
    b.code(0x30 + ord("A"), 8)
    b.code(1, 7)                                                # length symbol 257: 3
    b.code(4, 5)                                                # distance symbol 4: 5 + 1 extra bit
    b.put(0, 1)
    b.code(0, 7)                                                # end of block
    return bgzf.make_member(b"AAAA", b.bytes())


def _replace_member(gz: bytes, k: int, change) -> tuple:
    members = bgzf.parse_members(gz)
    off, bsize = members[k][0], members[k][1]
    new = change(gz[off:off + bsize + 1])
    return gz[:off] + new + gz[off + bsize + 1:], off


def _with_payload(member: bytes, payload: bytes, crc=None, isize=None) -> bytes:
    old_crc, old_isize = struct.unpack("<II", member[-8:])
    return (member[:16] + struct.pack("<H", len(payload) + 25) + payload
            + struct.pack("<II", old_crc if crc is None else crc, old_isize if isize is None else isize))


def _flip(member: bytes) -> bytes:
    p = bytearray(member[18:-8])
    p[len(p) // 2] ^= 0x10
    return _with_payload(member, bytes(p))


def _btype3(member: bytes) -> bytes:
    p = bytearray(member[18:-8])
    p[0] |= 0x06
    return _with_payload(member, bytes(p))


DEFECTS = {
    "flipped bit in the Huffman data": _flip,
    "BTYPE 3": _btype3,
    "distance before the start of the member": lambda m: _distance_before_start(),
    "trailer CRC32 off by one": lambda m: _with_payload(m, m[18:-8], crc=(struct.unpack("<I", m[-8:-4])[0] + 1) & 0xFFFFFFFF),
    "ISIZE too small": lambda m: _with_payload(m, m[18:-8], isize=struct.unpack("<I", m[-4:])[0] - 1),
    "ISIZE too large": lambda m: _with_payload(m, m[18:-8], isize=struct.unpack("<I", m[-4:])[0] + 1),
    "member cut to half": lambda m: _with_payload(m, m[18:-8][:len(m[18:-8]) // 2]),
}
REASONS = {
    "BTYPE 3": "bad block type",
    "distance before the start of the member": "distance too far back",
    "trailer CRC32 off by one": "CRC32 mismatch",
    "ISIZE too small": "data past ISIZE",
    "ISIZE too large": "ISIZE mismatch",
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_corrupted_member_is_reported(engine, defect):
    data = CORPORA["fasta"][:6 * B + 99]
    sound = bgzf.zlib_bgzf(data, 6)
    broken, off = _replace_member(sound, 3, DEFECTS[defect])
    with pytest.raises((bgzf.BgzfError, zlib.error)):           # the reference rejects the same file
        bgzf.check_file(broken)
    with pytest.raises(_ffi.MsimError) as e:
        engine.bgzf_inflate(broken)
    assert e.value.code == _ffi.ERR_VALUE
    assert f"member at offset {off}:" in str(e.value), str(e.value)
    if defect in REASONS:
        assert REASONS[defect] in str(e.value), str(e.value)
    assert engine.bgzf_inflate(sound) == data                   # the same engine goes on


# ------------------------------------------------------------------ the CLI with a compressed input
def _runnable_non_it():
    out = []
    for n in all_case_names():
        m = case_meta(n)
        if m.get("sim") is None or "it_fasta_len" in m or m["argv_tail"][:1] == ["it"]:
            continue
        if m["exception"] is None and "fasta_len" not in m:
            continue
        out.append(n)
    return out


def _run_case(meta: dict, tmp: Path, gz: bytes | None, extra_argv=()):
    """``pipeline.run_product_case`` with the input written as ``<infile_name>.gz`` holding ``gz`` (None: the plain input
    under its own name)."""
    infile = tmp / (meta["infile_name"] + (".gz" if gz is not None else ""))
    infile.write_bytes(gz if gz is not None else case_input_bytes(meta))
    tail = list(meta["argv_tail"])
    if tail[:1] == ["rmt"]:
        rmt = tmp / "case.rmt"
        rmt.write_text((CASES / meta["name"] / "case.rmt").read_text())
        tail = ["rmt", str(rmt)]
    argv = list(extra_argv) + ["-o", str(tmp / "out"), str(infile)] + tail
    out, err = io.StringIO(), io.StringIO()
    code, exc = None, None
    random.seed(meta["seed_py"])
    np.random.seed(meta["seed_np"])
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            try:
                msa_main.main(argv)
            except SystemExit as e:
                code = e.code
    except BaseException as e:  # noqa: BLE001
        exc = e
    res = {"exit_code": code, "exception": exc, "stderr": err.getvalue(), "fasta": None, "vcf": None,
           "words": [random.getrandbits(32) for _ in range(4)]}
    suffix = Path(meta["infile_name"]).suffix
    for key, name in (("fasta", f"out_ms{suffix}"), ("vcf", "out_ms.vcf")):
        for gzname in (name, name + ".gz"):
            if (tmp / gzname).exists():
                raw = (tmp / gzname).read_bytes()
                res[key] = bgzf.check_file(raw) if gzname.endswith(".gz") else raw
    if res["vcf"] is not None:
        res["vcf"] = mask_vcf(res["vcf"])
    assert not (tmp / (infile.name + ".fai")).exists() or gz is None          # no index next to a compressed input
    return res


def _check_against_goldens(meta: dict, res: dict, tmp: Path):
    name = meta["name"]
    if meta["exception"] is not None:
        assert type(res["exception"]).__name__ == meta["exception"]["type"]
        if meta["exception"]["type"] == "KeyError":
            assert repr(res["exception"].args[0]) == meta["exception"]["repr_args"][0]
        plain = tmp / "plain"
        plain.mkdir()
        ref = _run_case(meta, plain, None)
        assert type(ref["exception"]) is type(res["exception"])
        assert res["fasta"] == ref["fasta"] and res["vcf"] == ref["vcf"]      # the partial files the plain run leaves
        assert res["stderr"] == ref["stderr"]
        return
    assert res["exception"] is None and res["exit_code"] is None, (res["exception"], res["stderr"])
    fa, vcf = res["fasta"], res["vcf"]
    assert len(fa) == meta["fasta_len"] and sha256(fa) == meta["fasta_sha256"]
    assert len(vcf) == meta["vcf_len"] and sha256(vcf) == meta["vcf_sha256"]
    if meta["store"] == "full":
        assert fa == (CASES / name / "expected_ms.fa").read_bytes()
        assert vcf == (CASES / name / "expected_ms.vcf").read_bytes()
    assert res["stderr"] == meta["stderr"]
    assert res["words"] == meta["py_next_words_after"]


@pytest.mark.parametrize("name", _runnable_non_it())
def test_golden_case_with_bgzf_input(name, tmp_path):
    meta = case_meta(name)
    res = _run_case(meta, tmp_path, bgzf.zlib_bgzf(case_input_bytes(meta), 6))
    _check_against_goldens(meta, res, tmp_path)


@pytest.mark.parametrize("name", ["svmix_2ctg_200k", "readme_mix_tl"])
def test_golden_case_with_input_from_our_encoder(engine, name, tmp_path):
    meta = case_meta(name)
    res = _run_case(meta, tmp_path, engine.bgzf_compress(case_input_bytes(meta)))
    _check_against_goldens(meta, res, tmp_path)


@pytest.mark.parametrize("name", ["svmix_2ctg_200k", "titv0_dense"])
def test_golden_case_compressed_in_and_out(name, tmp_path):
    meta = case_meta(name)
    res = _run_case(meta, tmp_path, bgzf.zlib_bgzf(case_input_bytes(meta), 6), extra_argv=("--bgzip",))
    suffix = Path(meta["infile_name"]).suffix
    assert (tmp_path / f"out_ms{suffix}.gz").exists() and not (tmp_path / f"out_ms{suffix}").exists()
    _check_against_goldens(meta, res, tmp_path)


def _cli(tmp: Path, argv, seed=7):
    random.seed(seed)
    np.random.seed(seed)
    with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
        msa_main.main(["-q", "-o", str(tmp / "out")] + list(argv))
    return tmp


def _gen_genome(path: Path, lengths, seed: int):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for i, L in enumerate(lengths):
            f.write(f">chr{i + 1} synthetic\n".encode())
            for a in range(0, L, 60 << 20):
                n = min(60 << 20, L - a)
                b = lut[rng.integers(0, 4, n, dtype=np.uint8)]
                if a == 0:
                    b[: min(n, 100_000)] = ord("N")
                full = n // 60
                body = np.empty((full, 61), dtype=np.uint8)
                body[:, :60] = b[:full * 60].reshape(full, 60)
                body[:, 60] = 10
                f.write(body.tobytes())
                if n > full * 60:
                    f.write(b[full * 60:].tobytes() + b"\n")
    return path


def test_chain_of_two_runs(tmp_path):
    inp = _gen_genome(tmp_path / "g.fa", [400_000, 90_000, 1_500_000], 5)
    r1, r2, r3, mid = tmp_path / "r1", tmp_path / "r2", tmp_path / "r3", tmp_path / "mid"
    for d in (r1, r2, r3, mid):
        d.mkdir()
    _cli(r1, ["--bgzip", str(inp), "args", "-sn", "0.01", "-in", "0.001"])
    second = ["args", "-sn", "0.005", "-de", "0.001"]
    _cli(r2, [str(r1 / "out_ms.fa.gz")] + second, seed=8)       # run 1's compressed Fasta straight back in
    plain = mid / "out_ms.fa"                                   # (the same name without .gz: the VCF headers agree)
    plain.write_bytes(bgzf.check_file((r1 / "out_ms.fa.gz").read_bytes()))
    _cli(r3, [str(plain)] + second, seed=8)
    assert (r2 / "out_ms.fa").read_bytes() == (r3 / "out_ms.fa").read_bytes()
    assert mask_vcf((r2 / "out_ms.vcf").read_bytes()) == mask_vcf((r3 / "out_ms.vcf").read_bytes())
    assert not (r1 / "out_ms.fa.gz.fai").exists()


def _sha_of(path: Path) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        while True:
            b = f.read(64 << 20)
            if not b:
                return h.hexdigest()
            h.update(b)


def test_at_size(tmp_path):
    total = 1_200_000_000
    inp = _gen_genome(tmp_path / "g.fa", [total // 6] * 6, 11)
    with open(inp, "rb") as f, open(tmp_path / "g.fa.gz", "wb") as g:         # zlib level 1: the test's host time
        while True:
            chunk = f.read(512 * B)
            if not chunk:
                break
            g.write(bgzf.zlib_bgzf(chunk, 1)[:-28])
        g.write(bgzf.EOF_BLOCK)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _cli(a, [str(inp), "args", "-sn", "0.01"])
    _cli(b, [str(tmp_path / "g.fa.gz"), "args", "-sn", "0.01"])
    assert _sha_of(b / "out_ms.fa") == _sha_of(a / "out_ms.fa")
    assert hashlib.sha256(mask_vcf((b / "out_ms.vcf").read_bytes())).digest() == \
        hashlib.sha256(mask_vcf((a / "out_ms.vcf").read_bytes())).digest()
