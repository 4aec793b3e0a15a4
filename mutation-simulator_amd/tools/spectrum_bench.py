"""The context-dependent SNP engine (--spectrum) on the bench genome, beside the --rng fast step it sits next to:
    python3 mutation-simulator_amd/tools/spectrum_bench.py [runs] [total bases] [out.json]
A 3 Gb, 24-contig synthetic genome (msim_add_contig_synthetic, the contigs of bench.py), RATE 0.01, the skewed spectrum of
the tests (a 1-to-7 ramp over the channels, N[C>T]G times 20).  Per genome, medians over `runs` (>= 5) after a warm-up:
  census_ms / spectrum_plan_ms   the kernels' time on the device (msim_spectrum_timing: HIP events), and bases/s for each
  draw_only_ms                   the plan with an all-zero table: draw + scan, nothing emitted (the Philox work alone)
  spectrum step                  wall time of census + thresholds + plan (+ APPLY) over the genome, synchronised
  fast c2 step                   the same genome through --rng fast -sn 0.01 (tools/fast_steps.py's loop): plan only, plan + apply
The census's share of the HBM read roofline is bases / census time over 6.3 TB/s (MI355X, measured float4 copy)."""
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "mutation-simulator_amd", ROOT / "tests", ROOT / "tests" / "golden"):
    sys.path.insert(0, str(p))

import bench  # noqa: E402
import spectrum_twin  # noqa: E402
from mutation_simulator_amd import _ffi, spectrum  # noqa: E402
from mutation_simulator_amd import mutator as mm  # noqa: E402

HBM_READ_BYTES_PER_S = 6.3e12
RATE = 0.01
KEY = 42


def main():
    runs = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    total = int(float(sys.argv[2])) if len(sys.argv) > 2 else 3_000_000_000
    out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else None
    lengths = bench.contig_lengths(total)
    weights = spectrum_twin.skewed_weights()
    _ffi.warm_up_async(0, pin=True).join()
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    cids = [eng.add_contig_synthetic(L, 1000 + i) for i, L in enumerate(lengths)]
    sim = bench.build_settings("c2", lengths)
    tables = [mm.plan_table(ch) for ch in sim.chromosomes]
    eng.set_params(mm.params_descriptor(sim))
    zero = [0] * 192

    def spectrum_step(apply, table=None):
        """-> (wall s, census ms, plan ms, host threshold s, records)"""
        eng.reset_stats()
        t0 = time.perf_counter()
        host = 0.0
        records = 0
        for seq, cid in enumerate(cids):
            counts, _ = eng.context_counts(cid)
            h0 = time.perf_counter()
            thr = table if table is not None else spectrum.thresholds(counts, weights, RATE)
            host += time.perf_counter() - h0
            eng.plan_contig_spectrum(cid, thr, KEY, seq)
            records += eng.result_sizes(cid, applied=False)[1]
            if apply:
                eng.apply_contig(cid)
        eng.sync()
        wall = time.perf_counter() - t0
        census_ms, plan_ms = eng.spectrum_timing()
        return wall, census_ms, plan_ms, host, records

    def fast_step(apply):
        eng.set_fast_key(KEY)
        t0 = time.perf_counter()
        for ch, t in zip(sim.chromosomes, tables):
            eng.plan_contig(cids[ch.number], t)
            if apply:
                eng.apply_contig(cids[ch.number])
        eng.sync()
        return time.perf_counter() - t0

    med = statistics.median
    res = {"device": eng.device_name(), "bases": sum(lengths), "contigs": len(lengths), "rate": RATE, "runs": runs}
    for _ in range(2):
        spectrum_step(True)
        fast_step(True)
    rows = [spectrum_step(False) for _ in range(runs)]
    res["census_ms"] = med(r[1] for r in rows)
    res["census_ms_min_max"] = [min(r[1] for r in rows), max(r[1] for r in rows)]
    res["spectrum_plan_ms"] = med(r[2] for r in rows)
    res["spectrum_plan_ms_min_max"] = [min(r[2] for r in rows), max(r[2] for r in rows)]
    res["thresholds_host_ms"] = med(r[3] for r in rows) * 1e3
    res["spectrum_plan_only_step_ms"] = med(r[0] for r in rows) * 1e3
    res["records"] = rows[0][4]
    rows = [spectrum_step(False, zero) for _ in range(runs)]
    res["draw_only_ms"] = med(r[2] for r in rows)
    rows = [spectrum_step(True) for _ in range(runs)]
    res["spectrum_step_ms"] = med(r[0] for r in rows) * 1e3
    res["fast_c2_plan_only_step_ms"] = med(fast_step(False) for _ in range(runs)) * 1e3
    res["fast_c2_step_ms"] = med(fast_step(True) for _ in range(runs)) * 1e3
    n = res["bases"]
    res["census_bases_per_s"] = n / (res["census_ms"] * 1e-3)
    res["census_share_of_hbm_read"] = res["census_bases_per_s"] / HBM_READ_BYTES_PER_S
    res["plan_bases_per_s"] = n / (res["spectrum_plan_ms"] * 1e-3)
    res["philox_calls_per_s"] = n / 2 / (res["draw_only_ms"] * 1e-3)
    eng.close()
    for k, v in res.items():
        print(f"{k}: {v:.4g}" if isinstance(v, float) else f"{k}: {v}")
    if out_path:
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
