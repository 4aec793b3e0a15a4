"""The compare kernels (msim_cmp_counts: k_cmp_match, k_cmp_tally) on the bench genome:
    python3 mutation-simulator_amd/tools/compare_bench.py [runs] [total bases] [out.json]
A 3 Gb, 24-contig synthetic genome (msim_add_contig_synthetic, the contigs of bench.py), resident; two record tables per contig
planned by the counter-based engine with an SV mix (SN 0.01, IN / DE 0.001 of 1-50 bases, DU / IV 0.0005 of 50-500: 39 M candidates, about 30 M
records a table), the first under one key and HELD, the second under another.  Per genome -- the sum over the 24 contigs --
medians over `runs` (>= 7) after a warm-up, with min and max:
  cmp_kernel_ms     both kernels' time on the device (msim_cmp_timing: HIP events)
  copy_floor_ms     a device-to-device copy of both tables' record bytes, in the same process (msim_dbg_cmp_copy_floor): the
                    streaming floor of 16 B a record
Two tables from different keys share next to nothing: nearly every record walks, searches and misses -- the kernels' whole path.

With --diploid (anywhere on the line) the same two tables get genotypes (msim_genotype_contig, half of the records heterozygous)
and each side goes the way of `compare --diploid`: haplotype 1 selected and held, haplotype 2 selected, the two joined
(msim_cmp_join), the truth's diploid table scored against the calls' (msim_cmp_counts_diploid).  Reported beside the haploid figures
above, which are taken first in the same process on the same full tables (the join's held table replaces the haploid run's):
  cmp_join_kernel_ms        the join of the calls' two haplotype tables (msim_cmp_join_timing: its kernels and two pool copies)
  join_copy_floor_ms        a device-to-device copy of the bytes that join reads and writes (msim_dbg_cmp_join_copy_floor)
  cmp_diploid_kernel_ms     k_cmp_match<3> + k_cmp_tally<3>, to hold against cmp_kernel_ms"""
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "mutation-simulator_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import bench  # noqa: E402
from mutation_simulator_amd import _ffi  # noqa: E402
from mutation_simulator_amd import mutator as mm  # noqa: E402

SV_MIX = ["-in", "0.001", "-inmin", "1", "-inmax", "50", "-de", "0.001", "-demin", "1", "-demax", "50",
          "-du", "0.0005", "-dumin", "50", "-dumax", "500", "-iv", "0.0005", "-ivmin", "50", "-ivmax", "500"]
KEYS = (42, 43)


HET_THR = 1 << 52           # msim_genotype_contig: half of the records heterozygous


def join_pass_one(eng, cid, side, before_join=None):
    """One contig's genotyped table as `compare --diploid` takes it: haplotype 1 held, haplotype 2 current, joined."""
    eng.select_haplotype(cid, 1)
    eng.cmp_hold(cid)
    eng.select_haplotype(cid, 2)
    if before_join:
        before_join()
    eng.cmp_join(cid, side)


def main():
    diploid = "--diploid" in sys.argv
    if diploid:
        sys.argv.remove("--diploid")
    runs = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    total = int(float(sys.argv[2])) if len(sys.argv) > 2 else 3_000_000_000
    out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else None
    lengths = bench.contig_lengths(total)
    sim = bench.workload_settings(lengths, snp=0.01, titv=1.0, extra=SV_MIX)
    _ffi.warm_up_async(0, pin=True).join()
    copy_floor = _ffi.load().msim_dbg_cmp_copy_floor
    copy_floor.restype, copy_floor.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    join_floor = _ffi.load().msim_dbg_cmp_join_copy_floor
    join_floor.restype, join_floor.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    res = {"bases": sum(lengths), "contigs": len(lengths), "runs": runs, "device": eng.device_name()}
    try:
        cids = [eng.add_contig_synthetic(L, 1000 + i) for i, L in enumerate(lengths)]
        eng.set_params(mm.params_descriptor(sim))
        records = []
        for key in KEYS:
            eng.set_fast_key(key)
            for ch in sim.chromosomes:
                eng.plan_contig(cids[ch.number], mm.plan_table(ch))
            records.append(sum(eng.result_sizes(cid, applied=False)[1] for cid in cids))
            if diploid:
                for i, cid in enumerate(cids):
                    eng.genotype_contig(cid, key, i, HET_THR)
            if key == KEYS[0]:
                for cid in cids:
                    if diploid:                        # the truth's diploid tables, then the full table held for the haploid runs
                        join_pass_one(eng, cid, _ffi.CMP_TRUTH)
                        eng.select_haplotype(cid, 0)
                    eng.cmp_hold(cid)
        res["truth_records"], res["calls_records"] = records

        def kernel_pass():
            eng.reset_stats()
            got = [eng.cmp_counts(cid) for cid in cids]
            counts = sum(c for c, _ in got)
            assert int(counts[..., :2].sum()) == records[0] and int(counts[..., 2:].sum()) == records[1]
            assert (counts[..., 0] == counts[..., 2]).all()
            return eng.cmp_timing(), counts, sum(t for _, t in got)

        def copy_pass():
            total_ms = 0.0
            for cid in cids:
                ms = C.c_double()
                eng._check(copy_floor(eng.h, cid, C.byref(ms)), cid)
                total_ms += ms.value
            return total_ms

        def join_pass():
            """The calls' join, contig by contig: (join ms, copy floor ms of the bytes it moves)."""
            eng.reset_stats()
            floor_ms = 0.0
            for cid in cids:
                ms = C.c_double()
                join_pass_one(eng, cid, _ffi.CMP_CALLS, lambda: eng._check(join_floor(eng.h, cid, C.byref(ms)), cid))
                floor_ms += ms.value
            return eng.cmp_join_timing(), floor_ms

        def diploid_pass():
            eng.reset_stats()
            counts = sum(eng.cmp_counts_diploid(cid)[0] for cid in cids)
            assert int(counts[..., :3].sum()) == records[0] and int(counts[..., 3:].sum()) == records[1]
            assert (counts[..., 0] == counts[..., 3]).all() and (counts[..., 1] == counts[..., 4]).all()
            return eng.cmp_timing(), counts

        _, counts, tallies = kernel_pass()             # warm-up: code objects, the scratch of the copy
        copy_pass()
        res["matched"] = int(counts[..., 0].sum())
        res["window_stops"], res["base_stops"] = int(tallies[0]), int(tallies[1])
        rows, floors = [], []
        for _ in range(runs):
            rows.append(kernel_pass()[0])
            floors.append(copy_pass())
        if diploid:                                    # (behind the haploid runs: the joins' held tables replace theirs)
            join_pass()
            _, dcounts = diploid_pass()
            res["diploid_matched"], res["diploid_gt_mismatched"] = int(dcounts[..., 0].sum()), int(dcounts[..., 1].sum())
            joins, join_floors, dips = [], [], []
            for _ in range(runs):
                j, f = join_pass()
                joins.append(j)
                join_floors.append(f)
                dips.append(diploid_pass()[0])
    finally:
        eng.close()
    med = statistics.median
    res["cmp_kernel_ms"] = med(rows)
    res["cmp_kernel_ms_min_max"] = [min(rows), max(rows)]
    res["copy_floor_ms"] = med(floors)
    res["copy_floor_ms_min_max"] = [min(floors), max(floors)]
    res["kernel_over_floor"] = med(rows) / med(floors)
    res["records_per_s"] = sum(records) / (med(rows) * 1e-3)
    res["table_bytes"] = 16 * sum(records)
    if diploid:
        res["cmp_join_kernel_ms"] = med(joins)
        res["cmp_join_kernel_ms_min_max"] = [min(joins), max(joins)]
        res["join_copy_floor_ms"] = med(join_floors)
        res["join_copy_floor_ms_min_max"] = [min(join_floors), max(join_floors)]
        res["join_over_floor"] = med(joins) / med(join_floors)
        res["cmp_diploid_kernel_ms"] = med(dips)
        res["cmp_diploid_kernel_ms_min_max"] = [min(dips), max(dips)]
        res["diploid_over_haploid"] = med(dips) / med(rows)
        res["join_over_diploid_counts"] = med(joins) / med(dips)
    for k, v in res.items():
        print(f"{k}: {v:.4g}" if isinstance(v, float) else f"{k}: {v}")
    if out_path:
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
