#!/usr/bin/env python3
"""Measure ``--chain``: the chain kernels' device time (HIP events, ``msim_dbg_chain_ms``) on the README-flags tables of a
synthetic genome, beside the wall time of the VCF rendering call on the same tables, and the command line end to end with
and without ``--chain``.

    python tools/chain_bench.py [--mbases 600] [--contigs 6] [--repeats 3] [--dir /dev/shm] [--no-cli]

Prints one JSON line.  Under ``rocprofv3 --kernel-trace --stats -- python tools/chain_bench.py --no-cli`` the kernel
statistics show k_chain_* next to k_vcf_lines on the same tables.  Every command-line run is a child process with a time limit.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import random
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from vcf_replay_bench import FLAGS, cli, gen_genome  # noqa: E402


def kernels(fa: Path, repeats: int) -> dict:
    import mutation_simulator_amd as msa
    from mutation_simulator_amd import _ffi
    from mutation_simulator_amd import mutator as mm
    from mutation_simulator_amd.fasta_io import put_contig
    args = msa.get_args([str(fa), "args"] + FLAGS["readme"])
    fasta = msa.load_fasta(args.infile, 0)
    sim = msa.SimulationSettings.from_args(args, fasta, True)
    random.seed(42)
    np.random.seed(42)
    eng = _ffi.Engine(0)
    mm.export_python_streams(eng)
    eng.set_params(mm.params_descriptor(sim))
    eng.chain_kernel_ms()                               # switches the measurement on
    need = C.c_uint64()
    out = {"records": 0, "chain_bytes": 0, "vcf_bytes": 0, "chain_kernels_ms": [0.0] * repeats, "chain_call_ms": [0.0] * repeats,
           "vcf_call_ms": [0.0] * repeats}
    for chrom in sim.chromosomes:
        rec = fasta[chrom.number]
        cid = put_contig(eng, rec)
        eng.plan_contig(cid, mm.plan_table(chrom))
        eng.sync()
        out["records"] += eng.result_sizes(cid, applied=False)[1]
        name = rec.name.encode()
        for r in range(repeats):
            t0 = time.perf_counter()
            n_vcf = eng.render_vcf_device_size(cid, rec.name)
            eng.sync()                                  # (the size call leaves the write pass in flight)
            t1 = time.perf_counter()
            eng._check(eng.lib.msim_render_chain_device(eng.h, cid, name, name, chrom.number + 1, None, 0, C.byref(need)))
            t2 = time.perf_counter()
            out["vcf_call_ms"][r] += (t1 - t0) * 1e3
            out["chain_call_ms"][r] += (t2 - t1) * 1e3
            out["chain_kernels_ms"][r] += eng.chain_kernel_ms()
        out["chain_bytes"] += need.value
        out["vcf_bytes"] += n_vcf
        eng.clear()
    eng.close()
    fasta.close()
    for k in ("chain_kernels_ms", "chain_call_ms", "vcf_call_ms"):
        out[k] = [round(x, 3) for x in out[k]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=int, default=600)
    ap.add_argument("--contigs", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", type=Path, default=Path(tempfile.gettempdir()))
    ap.add_argument("--no-cli", action="store_true", help="kernels only (for a profiler run)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per command-line run")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        d = Path(d)
        fa = d / "g.fa"
        gen_genome(fa, [a.mbases * 1_000_000 // a.contigs] * a.contigs, 1)
        out = {"mbases": a.mbases, "contigs": a.contigs}
        out.update(kernels(fa, a.repeats))
        if not a.no_cli:
            plain, chain = [], []
            for _ in range(a.repeats):
                plain.append(cli(["--seed", 42, "-o", d / "out", fa, "args"] + FLAGS["readme"], a.limit))
                chain.append(cli(["--seed", 42, "--chain", "-o", d / "with", fa, "args"] + FLAGS["readme"], a.limit))
            out["cli_s"] = [round(x, 3) for x in plain]
            out["cli_chain_s"] = [round(x, 3) for x in chain]
            out["chain_file_bytes"] = (d / "with_ms.chain").stat().st_size
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
