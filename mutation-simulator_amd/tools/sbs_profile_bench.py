"""The profile kernel (msim_sbs_counts: k_sbs_count) on the bench genome:
    python3 mutation-simulator_amd/tools/sbs_profile_bench.py [runs] [total bases] [out.json]
A 3 Gb, 24-contig synthetic genome (msim_add_contig_synthetic, the contigs of bench.py), resident; its record tables planned by
msim_plan_contig_spectrum at RATE 0.01, once under the skewed spectrum of the tests (a 1-to-7 ramp over the channels, N[C>T]G
times 20) and once with all the weight on one channel (A[C>T]G: every record adds to the same bin).  Per genome -- the sum
over the 24 contigs -- medians over `runs` (>= 7) after a warm-up, with min and max, the two tables' runs alternating:
  sbs_kernel_ms     the kernel's time on the device (msim_sbs_timing: HIP events)
  copy_floor_ms     a device-to-device copy of the same record-table bytes, in the same process (msim_dbg_sbs_copy_floor): the
                    streaming floor of 16 B a record
  census_ms         the census of the same genome (msim_spectrum_timing), for scale
The one claim checked is data independence: the one-channel table's min-max overlaps the skewed table's."""
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "mutation-simulator_amd", ROOT / "tests", ROOT / "tests" / "golden"):
    sys.path.insert(0, str(p))

import bench  # noqa: E402
import spectrum_twin  # noqa: E402
from mutation_simulator_amd import _ffi, spectrum  # noqa: E402

RATE = 0.01
KEY = 42


def main():
    runs = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    total = int(float(sys.argv[2])) if len(sys.argv) > 2 else 3_000_000_000
    out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else None
    lengths = bench.contig_lengths(total)
    one_hot = [0.0] * 96
    one_hot[spectrum.CHANNELS.index("A[C>T]G")] = 1.0
    weights = {"skewed": spectrum_twin.skewed_weights(), "one_channel": one_hot}
    _ffi.warm_up_async(0, pin=True).join()
    engines, cids, records = {}, {}, {}
    copy_floor = _ffi.load().msim_dbg_sbs_copy_floor
    copy_floor.restype, copy_floor.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    res = {"bases": sum(lengths), "contigs": len(lengths), "rate": RATE, "runs": runs}
    for name, w in weights.items():                    # one context per table: both stay resident and planned
        eng = engines[name] = _ffi.Engine(0, _ffi.RNG_FAST)
        res["device"] = eng.device_name()
        cids[name] = [eng.add_contig_synthetic(L, 1000 + i) for i, L in enumerate(lengths)]
        eng.reset_stats()
        records[name] = 0
        for seq, cid in enumerate(cids[name]):
            counts, _ = eng.context_counts(cid)
            eng.plan_contig_spectrum(cid, spectrum.thresholds(counts, w, RATE), KEY, seq)
            records[name] += eng.result_sizes(cid, applied=False)[1]
        res["census_ms"] = eng.spectrum_timing()[0]
        res[f"{name}_records"] = records[name]

    def kernel_pass(name):
        eng = engines[name]
        eng.reset_stats()
        got = [eng.sbs_counts(cid) for cid in cids[name]]
        channels = sum(int(c.sum()) for c, _ in got)
        assert channels + sum(int(t[0]) for _, t in got) == records[name]
        return eng.sbs_timing(), channels

    def copy_pass(name):
        eng, total_ms = engines[name], 0.0
        for cid in cids[name]:
            ms = C.c_double()
            eng._check(copy_floor(eng.h, cid, C.byref(ms)), cid)
            total_ms += ms.value
        return total_ms

    for name in weights:                               # warm-up: code objects, the scratch of the copy
        kernel_pass(name)
        copy_pass(name)
    rows = {name: [] for name in weights}
    floors = {name: [] for name in weights}
    for _ in range(runs):                              # alternating: both tables see the same neighbours on the machine
        for name in weights:
            rows[name].append(kernel_pass(name)[0])
            floors[name].append(copy_pass(name))
    med = statistics.median
    for name in weights:
        res[f"{name}_sbs_kernel_ms"] = med(rows[name])
        res[f"{name}_sbs_kernel_ms_min_max"] = [min(rows[name]), max(rows[name])]
        res[f"{name}_copy_floor_ms"] = med(floors[name])
        res[f"{name}_copy_floor_ms_min_max"] = [min(floors[name]), max(floors[name])]
        res[f"{name}_floor_fraction"] = med(floors[name]) / med(rows[name])
        res[f"{name}_records_per_s"] = records[name] / (med(rows[name]) * 1e-3)
        res[f"{name}_table_bytes"] = 16 * records[name]
    a, b = res["skewed_sbs_kernel_ms_min_max"], res["one_channel_sbs_kernel_ms_min_max"]
    res["ranges_overlap"] = bool(a[0] <= b[1] and b[0] <= a[1])
    for eng in engines.values():
        eng.close()
    for k, v in res.items():
        print(f"{k}: {v:.4g}" if isinstance(v, float) else f"{k}: {v}")
    if out_path:
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
