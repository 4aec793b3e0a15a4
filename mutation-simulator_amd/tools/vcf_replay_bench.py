#!/usr/bin/env python3
"""Measure the ``vcf`` mode: parser kernels (GB/s of VCF text, HIP events), the command line end to end beside the ``args``
run that produced its input (same box, same call), and one host core running the host parser on the same text.

    python tools/vcf_replay_bench.py [--mbases 1200] [--contigs 8] [--repeats 3] [--flags sn|readme] [--dir /dev/shm]

Prints one JSON line per flag set.  Every command-line run is a child process with a time limit.
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
FLAGS = {"sn": ["-sn", "0.01"],
         "readme": ["-sn", "0.01", "-in", "0.01", "-de", "0.01", "-du", "0.01", "-iv", "0.01", "-tl", "0.01"]}


def gen_genome(path: Path, lengths, seed: int):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for i, L in enumerate(lengths):
            f.write(f">chr{i + 1} synthetic\n".encode())
            for a in range(0, L, 60 << 20):
                n = min(60 << 20, L - a)
                b = lut[rng.integers(0, 4, n, dtype=np.uint8)]
                full = n // 60
                body = np.empty((full, 61), dtype=np.uint8)
                body[:, :60] = b[:full * 60].reshape(full, 60)
                body[:, 60] = 10
                f.write(body.tobytes())
                if n > full * 60:
                    f.write(b[full * 60:].tobytes() + b"\n")


def cli(argv, limit):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-m", "mutation_simulator_amd", "-q", "-c"] + [str(a) for a in argv], env=env,
                       capture_output=True, text=True, timeout=limit)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"{argv}: exit {p.returncode}: {p.stderr[-2000:]}")
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=int, default=1200)
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--flags", choices=sorted(FLAGS), nargs="*", default=sorted(FLAGS))
    ap.add_argument("--dir", type=Path, default=Path(tempfile.gettempdir()))
    ap.add_argument("--host-parser", action="store_true", help="also time one host core on the host parser (reads the genome into memory)")
    ap.add_argument("--limit", type=int, default=600, help="seconds per command-line run")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        d = Path(d)
        fa = d / "g.fa"
        per = a.mbases * 1_000_000 // a.contigs
        gen_genome(fa, [per] * a.contigs, 1)
        for name in a.flags:
            args_s, vcf_s, load_gbs, plan_gbs = [], [], [], []
            for r in range(a.repeats):
                args_s.append(cli(["--seed", 42, "-o", d / "out", fa, "args"] + FLAGS[name], a.limit))
                vcf_s.append(cli(["--bench-json", d / "b.json", "-o", d / "back", fa, "vcf", d / "out_ms.vcf"], a.limit))
                st = json.loads((d / "b.json").read_text())
                load_gbs.append(st["vcf_bytes"] / 1e6 / max(st["vcf_load_kernel_ms"], 1e-9))
                plan_gbs.append(st["vcf_bytes"] / 1e6 / max(st["vcf_plan_kernel_ms"], 1e-9))
            same = subprocess.run(["cmp", str(d / "out_ms.fa"), str(d / "back_ms.fa")], capture_output=True).returncode == 0
            out = {"flags": name, "mbases": a.mbases, "vcf_bytes": st["vcf_bytes"], "fasta_identical": same,
                   "args_cli_s": [round(x, 3) for x in args_s], "vcf_cli_s": [round(x, 3) for x in vcf_s],
                   "load_kernels_GBps": [round(x, 1) for x in load_gbs], "plan_kernels_GBps": [round(x, 1) for x in plan_gbs],
                   "parser_kernels_GBps": [round(1 / (1 / x + 1 / y), 1) for x, y in zip(load_gbs, plan_gbs)]}
            if a.host_parser:
                from mutation_simulator_amd import _ffi, load_fasta, vcf_replay
                fasta = load_fasta(fa, 0)
                eng = _ffi.Engine(-1)
                recs = [fasta[i] for i in range(len(fasta))]
                cids = [eng.add_contig(rec.bases) for rec in recs]
                for cid, rec in zip(cids, recs):
                    eng.vcf_host_bases(cid, rec.bases)
                text = np.fromfile(d / "out_ms.vcf", dtype=np.uint8)
                t0 = time.perf_counter()
                vcf_replay.plan_all(eng, text, [rec.name for rec in recs], cids)
                out["host_parser_one_core_s"] = round(time.perf_counter() - t0, 3)
                eng.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
