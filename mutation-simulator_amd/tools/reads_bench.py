"""The reads mode on the bench genome:
    python3 mutation-simulator_amd/tools/reads_bench.py [--pairs N] [--file-pairs N] [--runs K] [--dir TMPFS] [--cli] [--json out.json]
A 3 Gb, 24-contig synthetic genome (msim_add_contig_synthetic, the contigs of bench.py), resident; LEN 150, pairs from fragments
of 400 +- 50, --pairs of them (20 M).  One process; medians over --runs (>= 7) passes after a warm-up, with min and max:
  render_kernel_ms   k_reads_render over both mates of all pairs, in chunks of 256 MiB of text (msim_reads_timing: HIP events),
                     and the FASTQ text's GB/s at that time
  copy_floor_ms      a device-to-device copy of the same number of text bytes, chunk by chunk (msim_dbg_reads_copy_floor): the
                     streaming floor the project quotes everywhere
  file_*             --file-pairs pairs (fewer than --pairs: the files live in --dir, a tmpfs) through the two output channels to
                     files, plain and --bgzip: wall seconds until msim_file_wait, the text's GB/s, and the render kernel's time
                     inside that run -- is the kernel the slowest stage of the pipeline?
  --cli              the command line end to end on a 1.2 Gb Fasta at a coverage that keeps the text under 4 GB, plain and
                     --bgzip, beside gzip -c of 256 MiB of the plain text on one host core (scaled to the whole text)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "mutation-simulator_amd", ROOT / "mutation-simulator_amd" / "tools"):
    sys.path.insert(0, str(p))

import bench  # noqa: E402
from mutation_simulator_amd import _ffi  # noqa: E402
from mutation_simulator_amd import reads as rd  # noqa: E402

LEN, MEAN, SD, KEY = 150, 400, 50, 42


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_part(a, res):
    lengths = bench.contig_lengths(a.bases)
    _ffi.warm_up_async(0, pin=True).join()
    eng = _ffi.Engine(0)
    res["device"] = eng.device_name()
    for i, L in enumerate(lengths):
        eng.add_contig_synthetic(L, 1000 + i)
    fmin, thr = rd.fragment_table(LEN, True, MEAN, SD)
    err_thr, qual = rd.error_tables(LEN, 0.001, 0.01)
    lib = eng.lib
    render = lib.msim_dbg_reads_render_device
    render.restype, render.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64]
    floor = lib.msim_dbg_reads_copy_floor
    floor.restype, floor.argtypes = C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_double)]

    def setup(n_pairs):
        return eng.reads_setup(_ffi.reads_params(KEY, n_pairs, LEN, True, fmin, thr, err_thr, qual, "r"))[0]

    stride = setup(a.pairs)
    per_chunk = rd.CHUNK_BYTES // stride
    chunks = [(first, min(per_chunk, a.pairs - first)) for first in range(0, a.pairs, per_chunk)]
    text_bytes = 2 * a.pairs * stride
    res.update(bases=sum(lengths), contigs=len(lengths), pairs=a.pairs, stride=stride, fastq_bytes=text_bytes, runs=a.runs,
               reads_per_workgroup=_ffi.reads_group(stride))

    def kernel_pass():
        eng.reset_stats()
        for first, count in chunks:
            for mate in (0, 1):
                eng._check(render(eng.h, mate, first, count))
        return eng.reads_timing()[0]

    def copy_pass():
        total = 0.0
        for _, count in chunks:
            for _mate in (0, 1):
                ms = C.c_double()
                eng._check(floor(eng.h, count * stride, C.byref(ms)))
                total += ms.value
        return total

    kernel_pass()
    copy_pass()
    k_ms, c_ms = [], []
    for _ in range(a.runs):
        k_ms.append(kernel_pass())
        c_ms.append(copy_pass())
    res["render_kernel_ms"], res["copy_floor_ms"] = spread(k_ms), spread(c_ms)
    res["render_GBps"] = text_bytes / 1e9 / (res["render_kernel_ms"]["median"] * 1e-3)
    res["copy_floor_GBps"] = text_bytes / 1e9 / (res["copy_floor_ms"]["median"] * 1e-3)
    res["floor_fraction"] = res["copy_floor_ms"]["median"] / res["render_kernel_ms"]["median"]

    # through the channels to files on a tmpfs
    stride_f = setup(a.file_pairs)
    bytes_f = 2 * a.file_pairs * stride_f
    per_chunk = rd.CHUNK_BYTES // stride_f
    for label, bgzip in (("file_plain", False), ("file_bgzip", True)):
        walls, kernels, sizes = [], [], 0
        for _ in range(max(1, a.file_runs) + 1):           # (the first one warms the channels up and is dropped)
            with tempfile.TemporaryDirectory(dir=a.dir) as td:
                files = [open(Path(td) / f"m{m}.fq", "wb") for m in (0, 1)]
                eng.reset_stats()
                t0 = time.perf_counter()
                if bgzip:
                    for m, f in enumerate(files):
                        eng.bgzf_open(m, f.fileno())
                for first in range(0, a.file_pairs, per_chunk):
                    count = min(per_chunk, a.file_pairs - first)
                    for m, f in enumerate(files):
                        eng.reads_render_to_file(m, first, count, f.fileno(), first * stride_f)
                if bgzip:
                    for m in (0, 1):
                        eng.bgzf_close(m)
                eng.file_wait()
                walls.append(time.perf_counter() - t0)
                kernels.append(eng.reads_timing()[0])
                for f in files:
                    f.close()
                sizes = sum(os.path.getsize(f.name) for f in files)
        walls, kernels = walls[1:], kernels[1:]
        res[label] = {"pairs": a.file_pairs, "text_bytes": bytes_f, "file_bytes": sizes, "wall_s": spread(walls),
                      "text_GBps": bytes_f / 1e9 / statistics.median(walls), "render_kernel_ms": spread(kernels),
                      "kernel_share_of_wall": statistics.median(kernels) * 1e-3 / statistics.median(walls)}
    eng.reads_release()
    eng.close()


def cli_part(a, res):
    import cli_profile
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        td = Path(td)
        fa = td / "g.fa"
        cli_profile.write_fasta(fa, 1200, 24)
        out = {}
        for label, extra in (("plain", []), ("bgzip", ["--bgzip"])):
            bj = td / f"{label}.json"
            t0 = time.perf_counter()
            subprocess.run([sys.executable, "-m", "mutation_simulator_amd", "--seed", "42", "-q", "--bench-json", str(bj), "-o",
                            str(td / label), *extra, str(fa), "reads", "--coverage", "1.4", "--paired", "--frag-mean", str(MEAN),
                            "--frag-sd", str(SD)], check=True, timeout=600,
                           env={**os.environ, "PYTHONPATH": str(ROOT / "mutation-simulator_amd")})
            out[label] = {"wall_s": time.perf_counter() - t0, **json.loads(bj.read_text()),
                          "file_bytes": sum(p.stat().st_size for p in td.glob(f"{label}_ms_*"))}
        sample = td / "sample.fq"
        with open(td / "plain_ms_1.fq", "rb") as f:
            sample.write_bytes(f.read(256 << 20))
        t0 = time.perf_counter()
        with open(td / "sample.gz", "wb") as g:
            subprocess.run(["gzip", "-c", str(sample)], stdout=g, check=True, timeout=600)
        dt = time.perf_counter() - t0
        out["gzip_one_core"] = {"sample_bytes": sample.stat().st_size, "sample_s": dt,
                                "scaled_to_text_s": dt * out["plain"]["fastq_bytes"] / sample.stat().st_size,
                                "sample_gz_bytes": (td / "sample.gz").stat().st_size}
        res["cli_1200Mb"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--file-pairs", type=int, default=4_000_000, dest="file_pairs")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--file-runs", type=int, default=3, dest="file_runs")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--no-device", action="store_true", dest="no_device")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    a.bases, a.runs = int(a.bases), max(7, a.runs)
    res = {"command": " ".join(sys.argv), "date": time.strftime("%Y-%m-%d")}
    if not a.no_device:
        device_part(a, res)
    if a.cli:
        cli_part(a, res)
    print(json.dumps(res, indent=1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
