"""BGZF on the device (csrc/bgzf.hip): kernel throughput, compressed size against zlib level 1 at the same 65 280-byte
blocking, and the CLI end to end with and without --bgzip.  Prints one JSON line.

The inflate leg (``--inflate``, input side: k_bgzf_inflate) adds to the same line: kernel GB/s of uncompressed output for
zlib-level-6 members of Fasta text, for our own encoder's members of the same text and for VCF text; the one-shot call end
to end (upload + kernel + download into page-locked memory); ``zlib.decompress`` of the same members on one host core and
over a 16-thread pool (device and pool alternate, min / median / max); and the CLI end to end on a genome given as ``.fa``,
as ``.fa.gz`` and as ``.fa`` after a timed host inflate to a file.

    python tools/bgzf_bench.py [--gb 1.0] [--cli-gb 1.2] [--no-cli] [--inflate] [--no-compress]
"""
from __future__ import annotations

import argparse
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib
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


def _mmm(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(xs[len(xs) // 2], 4), "max": round(xs[-1], 4)}


def _host_inflate(payloads, pool):
    def one(p):
        return len(zlib.decompress(p, -15))                # (zlib releases the GIL while it inflates)
    t0 = time.perf_counter()
    n = sum(pool.map(one, payloads, chunksize=64)) if pool else sum(map(one, payloads))
    return time.perf_counter() - t0, n


def inflate_kernel(eng, gz: bytes, n: int, reps: int = 3):
    out = eng.host_buffer(n)
    eng.bgzf_inflate(gz, out=out)                          # (warm-up: code objects, first touch of the buffer)
    ms = [eng.bgzf_inflate(gz, out=out, timed=True)[1] for _ in range(reps)]
    return {"bytes": n, "compressed": len(gz), "kernel_ms": _mmm(ms), "gbps": round(n / min(ms) / 1e6, 2)}, out


def inflate_leg(eng, n: int, reps: int = 5):
    text = fasta_text(n)
    res = {}
    z6 = bgzf.zlib_bgzf(text[: min(n, 256_000_000)], 6)    # (level 6 on a host core is slow: a quarter GB of it)
    res["fasta_zlib6"], _ = inflate_kernel(eng, z6, min(n, 256_000_000))
    own = eng.bgzf_compress(text)
    res["fasta_own"], out = inflate_kernel(eng, own, len(text))
    vcf = vcf_text(min(n, 200_000_000))
    res["vcf_zlib6"], _ = inflate_kernel(eng, bgzf.zlib_bgzf(vcf, 6), len(vcf))
    # the one-shot call end to end against the host, same members, alternated in one process
    payloads = [m[4] for m in bgzf.parse_members(own) if m[2]]
    dev, pool16, one = [], [], []
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        _host_inflate(payloads[:2000], pool)
        for k in range(reps):
            t0 = time.perf_counter()
            eng.bgzf_inflate(own, out=out)
            dev.append(time.perf_counter() - t0)
            pool16.append(_host_inflate(payloads, pool)[0])
            if k == 0:
                one.append(_host_inflate(payloads, None)[0])
    res["one_shot"] = {"bytes": len(text), "device_s": _mmm(dev), "zlib_16_threads_s": _mmm(pool16),
                       "zlib_1_core_s": round(one[0], 4), "device_gbps": round(len(text) / min(dev) / 1e9, 2),
                       "pool_gbps": round(len(text) / min(pool16) / 1e9, 2),
                       "device_faster_outside_spread": max(dev) < min(pool16)}
    return res


def inflate_cli(td: Path, total: int, reps: int = 3):
    inp, gz = td / "g.fa", td / "g.fa.gz"
    write_genome(inp, total)
    with open(inp, "rb") as f, open(gz, "wb") as g:
        while True:
            chunk = f.read(512 * bgzf.BGZF_BLOCK)
            if not chunk:
                break
            g.write(bgzf.zlib_bgzf(chunk, 1)[:-28])
        g.write(bgzf.EOF_BLOCK)
    cli(td, inp, [])                                       # (warm: page cache, code objects)
    plain, comp, host = [], [], []
    for _ in range(reps):
        plain.append(cli(td, inp, []))
        comp.append(cli(td, gz, []))
        t0 = time.perf_counter()
        subprocess.run(f"gzip -dc {gz} > {td / 'h.fa'}", shell=True, check=True)
        t1 = time.perf_counter()
        host.append((t1 - t0) + cli(td, td / "h.fa", []))
    return {"bases": total, "fa_s": _mmm(plain), "fa_gz_s": _mmm(comp), "gzip_d_then_fa_s": _mmm(host),
            "gz_bytes": gz.stat().st_size}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--cli-gb", type=float, default=1.2)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--inflate", action="store_true", help="add the inflate (compressed input) leg")
    ap.add_argument("--no-compress", action="store_true", help="skip the compression legs")
    a = ap.parse_args()
    n = int(a.gb * 1e9)
    res = {}
    with _ffi.Engine(0) as eng:
        if not a.no_compress:
            res["fasta"] = kernel(eng, fasta_text(n))
            res["vcf"] = kernel(eng, vcf_text(min(n, 200_000_000)))
        if a.inflate:
            res["inflate"] = inflate_leg(eng, n)
    if a.inflate and not a.no_cli:
        with tempfile.TemporaryDirectory() as td:
            res["inflate_cli"] = inflate_cli(Path(td), int(a.cli_gb * 1e9))
    if not a.no_cli and not a.no_compress:
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
