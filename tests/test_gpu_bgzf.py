"""--bgzip on the GPU: the device deflate encoder (csrc/bgzf.hip) and the output channels' BGZF mode (csrc/file_io.hip).
Contract: the .gz files are valid BGZF and inflate to exactly what the same run without --bgzip writes."""
from __future__ import annotations

import contextlib
import hashlib
import io
import random
from pathlib import Path

import numpy as np
import pytest

from helpers import CASES, all_case_names, case_meta, mask_vcf, sha256
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import __main__ as msa_main
from mutation_simulator_amd import bgzf
from mutation_simulator_amd import mutator as msa_mutator
from pipeline import run_product_case

pytestmark = pytest.mark.gpu

B = bgzf.BGZF_BLOCK


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


@pytest.fixture(scope="module")
def engine():
    eng = _ffi.Engine(0)
    yield eng
    eng.close()


def _gz_outputs(tmp: Path, suffix: str):
    fa, vcf = tmp / f"out_ms{suffix}.gz", tmp / "out_ms.vcf.gz"
    return (fa.read_bytes() if fa.exists() else None), (vcf.read_bytes() if vcf.exists() else None)


@pytest.mark.parametrize("name", _runnable_non_it())
def test_golden_case_with_bgzip(name, tmp_path):
    meta = case_meta(name)
    res = run_product_case(meta, tmp_path, extra_argv=("--bgzip",))
    suffix = Path(meta["infile_name"]).suffix
    gz_fa, gz_vcf = _gz_outputs(tmp_path, suffix)
    assert res["fasta"] is None and res["vcf"] is None          # no plain files beside the .gz ones
    fa = bgzf.check_file(gz_fa)
    vcf = mask_vcf(bgzf.check_file(gz_vcf))
    if meta["exception"] is not None:
        assert type(res["exception"]).__name__ == meta["exception"]["type"]
        if meta["exception"]["type"] == "KeyError":
            assert repr(res["exception"].args[0]) == meta["exception"]["repr_args"][0]
        plain = tmp_path / "plain"
        plain.mkdir()
        ref = run_product_case(meta, plain)
        assert type(ref["exception"]) is type(res["exception"])
        assert fa == ref["fasta"] and vcf == ref["vcf"]         # the partial files the plain run leaves
        return
    assert res["exception"] is None and res["exit_code"] is None, (res["exception"], res["stderr"])
    assert len(fa) == meta["fasta_len"] and sha256(fa) == meta["fasta_sha256"]
    assert len(vcf) == meta["vcf_len"] and sha256(vcf) == meta["vcf_sha256"]
    if meta["store"] == "full":
        assert fa == (CASES / name / "expected_ms.fa").read_bytes()
        assert vcf == (CASES / name / "expected_ms.vcf").read_bytes()
    assert res["stderr"] == meta["stderr"]
    assert [random.getrandbits(32) for _ in range(4)] == meta["py_next_words_after"]


def _roundtrip(engine, data: bytes) -> bytes:
    gz = engine.bgzf_compress(data)
    assert bgzf.check_file(gz) == data
    members = bgzf.parse_members(gz)
    assert len(members) == (len(data) + B - 1) // B + 1
    assert all(m[2] == B for m in members[:-2])
    return gz


@pytest.mark.parametrize("n", [0, 1, B, B + 1, 2 * B + 17])
def test_one_shot_sizes(engine, n):
    rng = np.random.default_rng(n)
    data = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    gz = _roundtrip(engine, data)
    if n == 0:
        assert gz == bgzf.EOF_BLOCK


def test_one_shot_random_bytes_are_stored(engine):
    data = np.random.default_rng(7).integers(0, 256, 64 << 20, dtype=np.uint8).tobytes()
    gz = _roundtrip(engine, data)
    assert len(gz) <= len(data) + (len(data) // B + 1) * 31 + 28
    assert max(m[1] + 1 for m in bgzf.parse_members(gz)) <= 65536


def test_one_shot_n_run(engine):
    data = b"N" * (10 << 20)
    gz = _roundtrip(engine, data)
    assert len(data) / len(gz) > 100


def test_one_shot_long_distance_repeats(engine):
    rng = np.random.default_rng(3)
    parts = []
    for d in (3, 17, 255, 256, 1000, 4096, 20000, 32768):
        chunk = rng.integers(65, 91, d, dtype=np.uint8).tobytes()
        parts.append(chunk * max(2, 40000 // d))
    data = b"".join(parts)
    gz = _roundtrip(engine, data)
    assert len(gz) < len(data) // 2


def test_one_shot_is_deterministic(engine):
    data = (CASES / "titv0_dense" / "expected_ms.vcf").read_bytes() * 3
    assert engine.bgzf_compress(data) == engine.bgzf_compress(data)


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


def test_ratio_fasta_at_most_zlib_level1(engine):
    for data in (_fasta_text(5_000_000, 1), _fasta_text(5_000_000, 2, n_run=1_500_000)):
        ours, ref = len(engine.bgzf_compress(data)), len(bgzf.zlib_bgzf(data, 1))
        assert ours <= ref, (ours, ref)


@pytest.mark.parametrize("name", ["titv0_dense", "readme_mix_tl"])
def test_ratio_vcf_within_a_quarter_of_zlib_level1(engine, name):
    data = (CASES / name / "expected_ms.vcf").read_bytes()
    ours, ref = len(engine.bgzf_compress(data)), len(bgzf.zlib_bgzf(data, 1))
    assert ours <= 1.25 * ref, (ours, ref)


def _cli(tmp: Path, argv, seed=7):
    random.seed(seed)
    np.random.seed(seed)
    with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
        msa_main.main(["-q", "-o", str(tmp / "out")] + list(argv))
    return tmp


def _gen_genome(path: Path, lengths, seed: int, n_runs: bool = True):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for i, L in enumerate(lengths):
            f.write(f">chr{i + 1} synthetic\n".encode())
            for a in range(0, L, 60 << 20):
                n = min(60 << 20, L - a)
                b = lut[rng.integers(0, 4, n, dtype=np.uint8)]
                if n_runs and a == 0:
                    b[: min(n, 100_000)] = ord("N")
                full = n // 60
                body = np.empty((full, 61), dtype=np.uint8)
                body[:, :60] = b[:full * 60].reshape(full, 60)
                body[:, 60] = 10
                f.write(body.tobytes())
                if n > full * 60:
                    f.write(b[full * 60:].tobytes() + b"\n")
    return path


def test_deterministic_runs_and_paths(tmp_path, monkeypatch):
    inp = _gen_genome(tmp_path / "g.fa", [150_000, 90_000, 2_000_000, 120_000, 60_000], 5)
    argv = ["--bgzip", str(inp), "args", "-sn", "0.01", "-in", "0.001", "-de", "0.001"]
    runs = []
    for k in range(2):
        d = tmp_path / f"r{k}"
        d.mkdir()
        runs.append(_gz_outputs(_cli(d, argv), ".fa"))
    assert runs[0] == runs[1]
    d = tmp_path / "single"
    d.mkdir()
    monkeypatch.setattr(msa_mutator, "BATCH_MAX_LEN", 0)
    monkeypatch.setattr(msa_mutator, "BATCH_SPARSE_MAX_LEN", 0)
    assert _gz_outputs(_cli(d, argv), ".fa") == runs[0]        # per-contig egress == batched egress, byte for byte
    monkeypatch.setattr(msa_mutator, "NATIVE_FILE_EGRESS", False)
    d = tmp_path / "hostframed"
    d.mkdir()
    assert _gz_outputs(_cli(d, argv), ".fa") == runs[0]        # the host-framed fallbacks
    d = tmp_path / "plain"
    d.mkdir()
    monkeypatch.undo()
    _cli(d, argv[1:])
    fa, vcf = runs[0]
    assert bgzf.check_file(fa) == (d / "out_ms.fa").read_bytes()
    assert mask_vcf(bgzf.check_file(vcf)) == mask_vcf((d / "out_ms.vcf").read_bytes())


def test_fast_rng_deterministic(tmp_path):
    inp = _gen_genome(tmp_path / "g.fa", [3_000_000, 500_000], 9)
    argv = ["--bgzip", "--rng", "fast", str(inp), "args", "-sn", "0.01"]
    outs = []
    for k in range(2):
        d = tmp_path / f"r{k}"
        d.mkdir()
        outs.append(_gz_outputs(_cli(d, argv), ".fa"))
    assert outs[0] == outs[1]
    d = tmp_path / "plain"
    d.mkdir()
    _cli(d, argv[1:])
    assert bgzf.check_file(outs[0][0]) == (d / "out_ms.fa").read_bytes()
    assert mask_vcf(bgzf.check_file(outs[0][1])) == mask_vcf((d / "out_ms.vcf").read_bytes())


def _sha_of_gz(path: Path) -> str:
    h = hashlib.sha256()
    for raw in bgzf.inflate_members(path.read_bytes()):       # (every member checked on the way)
        h.update(raw)
    return h.hexdigest()


def _sha_of(path: Path) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        while True:
            b = f.read(64 << 20)
            if not b:
                return h.hexdigest()
            h.update(b)


@pytest.mark.parametrize("total,argv", [
    (1_200_000_000, ["-sn", "0.01"]),
    (300_000_000, ["-sn", "0.001", "-in", "0.0005", "-de", "0.0005", "-iv", "0.0001", "-du", "0.0001"]),
])
def test_at_size(tmp_path, total, argv):
    inp = _gen_genome(tmp_path / "g.fa", [total // 6] * 6, 11)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _cli(a, [str(inp), "args"] + argv)
    _cli(b, ["--bgzip", str(inp), "args"] + argv)
    assert _sha_of_gz(b / "out_ms.fa.gz") == _sha_of(a / "out_ms.fa")
    (a / "out_ms.fa").unlink()
    assert mask_vcf(bgzf.check_file((b / "out_ms.vcf.gz").read_bytes())) == mask_vcf((a / "out_ms.vcf").read_bytes())
