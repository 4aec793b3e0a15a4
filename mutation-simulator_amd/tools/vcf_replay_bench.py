#!/usr/bin/env python3
"""Measure the ``vcf`` mode: parser kernels (GB/s of VCF text, HIP events), the command line end to end beside the ``args``
run that produced its input (same box, same call), and one host core running the host parser on the same text.

    python tools/vcf_replay_bench.py [--mbases 1200] [--contigs 8] [--repeats 3] [--flags sn|readme] [--dir /dev/shm] [--consensus]

``--consensus``: the same run's VCF is also replayed with ``vcf --consensus`` (the general grammar), and its figures stand beside
the dialect's.  The consensus grammar refuses what it has no record form for -- the simulator's own inversion or duplication line
that ends on a contig's last base without a trailing anchor, say; such a draw is reported as ``consensus_refused`` in the JSON
line and the dialect's figures stand alone.  Prints one JSON line per flag set.  Every command-line run is a child process with a time limit.
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


class Refused(Exception):
    """A child ended with a "VCF line N: reason" refusal."""


def cli(argv, limit, may_refuse=False):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-m", "mutation_simulator_amd", "-q", "-c"] + [str(a) for a in argv], env=env,
                       capture_output=True, text=True, timeout=limit)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        if may_refuse and p.returncode == 1 and "VCF line " in p.stderr:
            raise Refused(p.stderr[p.stderr.index("VCF line "):].splitlines()[0])
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
    ap.add_argument("--consensus", action="store_true", help="also replay the VCF with the consensus grammar")
    ap.add_argument("--limit", type=int, default=600, help="seconds per command-line run")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        d = Path(d)
        fa = d / "g.fa"
        per = a.mbases * 1_000_000 // a.contigs
        gen_genome(fa, [per] * a.contigs, 1)
        for name in a.flags:
            args_s, vcf_s, load_gbs, plan_gbs = [], [], [], []
            cons_s, cons_load, cons_plan, cons_same, cons_refused = [], [], [], True, None
            for r in range(a.repeats):
                args_s.append(cli(["--seed", 42, "-o", d / "out", fa, "args"] + FLAGS[name], a.limit))
                vcf_s.append(cli(["--bench-json", d / "b.json", "-o", d / "back", fa, "vcf", d / "out_ms.vcf"], a.limit))
                st = json.loads((d / "b.json").read_text())
                load_gbs.append(st["vcf_bytes"] / 1e6 / max(st["vcf_load_kernel_ms"], 1e-9))
                plan_gbs.append(st["vcf_bytes"] / 1e6 / max(st["vcf_plan_kernel_ms"], 1e-9))
                if a.consensus and cons_refused is None:
                    try:
                        cons_s.append(cli(["--bench-json", d / "c.json", "-o", d / "cons", fa, "vcf", d / "out_ms.vcf", "--consensus"],
                                          a.limit, may_refuse=True))
                    except Refused as e:
                        cons_refused = str(e)
                        continue
                    ct = json.loads((d / "c.json").read_text())
                    cons_load.append(ct["vcf_bytes"] / 1e6 / max(ct["vcf_load_kernel_ms"], 1e-9))
                    cons_plan.append(ct["vcf_bytes"] / 1e6 / max(ct["vcf_plan_kernel_ms"], 1e-9))
                    cons_same &= subprocess.run(["cmp", str(d / "out_ms.fa"), str(d / "cons_ms.fa")], capture_output=True).returncode == 0
            same = subprocess.run(["cmp", str(d / "out_ms.fa"), str(d / "back_ms.fa")], capture_output=True).returncode == 0
            out = {"flags": name, "mbases": a.mbases, "vcf_bytes": st["vcf_bytes"], "fasta_identical": same,
                   "args_cli_s": [round(x, 3) for x in args_s], "vcf_cli_s": [round(x, 3) for x in vcf_s],
                   "load_kernels_GBps": [round(x, 1) for x in load_gbs], "plan_kernels_GBps": [round(x, 1) for x in plan_gbs],
                   "parser_kernels_GBps": [round(1 / (1 / x + 1 / y), 1) for x, y in zip(load_gbs, plan_gbs)]}
            if a.consensus and cons_refused is not None:
                out["consensus_refused"] = cons_refused
            elif a.consensus:
                out.update({"consensus_fasta_identical": cons_same, "consensus_cli_s": [round(x, 3) for x in cons_s],
                            "consensus_load_kernels_GBps": [round(x, 1) for x in cons_load],
                            "consensus_plan_kernels_GBps": [round(x, 1) for x in cons_plan]})
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
