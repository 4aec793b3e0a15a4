"""BGZF on the device (csrc/bgzf.hip): kernel throughput, compressed size against zlib level 1 at the same 65 280-byte
blocking, and the CLI end to end with and without --bgzip.  Prints one JSON line.

    python tools/bgzf_bench.py [--gb 1.0] [--cli-gb 1.2] [--no-cli]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

from mutation_simulator_amd import _ffi  # noqa: E402
from mutation_simulator_amd import bgzf  # noqa: E402


def fasta_text(n: int, seed: int = 1) -> bytes:
    rng = np.random.default_rng(seed)
    lines = n // 61
    body = np.empty((lines, 61), dtype=np.uint8)
    body[:, :60] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (lines, 60), dtype=np.uint8)]
    body[:, 60] = 10
    return body.tobytes()


def vcf_text(n: int, seed: int = 2) -> bytes:
    rng = np.random.default_rng(seed)
    out, size, pos = [], 0, 0
    bases = "ACGT"
    while size < n:
        step = rng.integers(1, 200, 100_000)
        ref = rng.integers(0, 4, 100_000)
        alt = (ref + rng.integers(1, 4, 100_000)) % 4
        chunk = "".join(f"chr1\t{pos + int(s)}\t.\t{bases[r]}\t{bases[a]}\t.\t.\t.\tGT\t1\n"
                        for s, r, a in zip(np.cumsum(step), ref, alt)).encode()
        pos += int(step.sum())
        out.append(chunk)
        size += len(chunk)
    return b"".join(out)[:n]


def kernel(eng, data: bytes, reps: int = 3):
    eng.bgzf_compress(data[: 1 << 24])                     # (warm-up: workspace, code objects)
    best, gz = None, None
    for _ in range(reps):
        gz, ms = eng.bgzf_compress(data, timed=True)
        best = ms if best is None else min(best, ms)
    sample = data[: 64 << 20]
    ours = len(eng.bgzf_compress(sample))
    z1 = len(bgzf.zlib_bgzf(sample, 1))
    return {"bytes": len(data), "kernel_ms": round(best, 3), "gbps": round(len(data) / best / 1e6, 2),
            "ratio": round(len(data) / len(gz), 3), "sample_bytes": len(sample), "ours_vs_zlib1": round(ours / z1, 4)}


def write_genome(path: Path, total: int, seed: int = 11):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    per = total // 6
    with open(path, "wb") as f:
        for i in range(6):
            f.write(f">chr{i + 1}\n".encode())
            for a in range(0, per, 60 << 20):
                n = min(60 << 20, per - a)
                b = lut[rng.integers(0, 4, n, dtype=np.uint8)]
                full = n // 60
                body = np.empty((full, 61), dtype=np.uint8)
                body[:, :60] = b[:full * 60].reshape(full, 60)
                body[:, 60] = 10
                f.write(body.tobytes())
                if n > full * 60:
                    f.write(b[full * 60:].tobytes() + b"\n")


def cli(tmp: Path, inp: Path, extra):
    cmd = [sys.executable, "-m", "mutation_simulator_amd", "-q", "--seed", "1"] + extra + ["-o", str(tmp / "out"), str(inp),
                                                                                            "args", "-sn", "0.01"]
    env = dict(os.environ, PYTHONPATH=str(HERE.parent))
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, env=env)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--cli-gb", type=float, default=1.2)
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    n = int(a.gb * 1e9)
    res = {}
    with _ffi.Engine(0) as eng:
        res["fasta"] = kernel(eng, fasta_text(n))
        res["vcf"] = kernel(eng, vcf_text(min(n, 200_000_000)))
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as td:
            td = Path(td)
            inp = td / "g.fa"
            write_genome(inp, int(a.cli_gb * 1e9))
            cli(td, inp, [])                                   # (warm: page cache, code objects)
            plain = cli(td, inp, [])
            gz = cli(td, inp, ["--bgzip"])
            sizes = {p.name: p.stat().st_size for p in td.glob("out_ms*")}
            res["cli"] = {"bases": int(a.cli_gb * 1e9), "plain_s": round(plain, 3), "bgzip_s": round(gz, 3),
                          "ratio": round(gz / plain, 3), "sizes": sizes}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
