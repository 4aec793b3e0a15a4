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
  cmp_diploid_kernel_ms     k_cmp_match<3> + k_cmp_tally<3>, to hold against cmp_kernel_ms

With --blocks (anywhere on the line) the same two tables -- where nearly every block is a candidate: the worst case -- go through
`compare --blocks` (msim_cmp_counts_blocks) as well, and then a second calls table DERIVED from the truth (the realistic case): about
1 % of its records picked and re-represented -- an SN with room behind it as a deletion and an insertion (an MNP line), a deletion of
two bases or more in two pieces, a duplication as the insertion it is; a picked record with no other form (IN, IV, a one-base DE) is
dropped one time in four and kept otherwise -- and installed with msim_dbg_set_records.  Per table pair, medians of `runs` with min and max:
  cmp_block_kernel_ms       k_blk_scan + k_blk_replay (msim_cmp_blocks_timing)
  cmp_kernel_ms_in_blocks   k_cmp_match<2> + k_cmp_tally<3> of the same calls (msim_cmp_timing)
  blk_scan_ms, blk_replay_ms   the two kernels apart, and replay_lane_use: the bytes the replay's lanes compared over 64 x the
                            longest lane of every wave -- what blocks of different lengths leave of a wave (msim_dbg_cmp_blocks_split)
the derived pair's figures under derived_*, with its own cmp_kernel_ms (no blocks) and copy floor.

With --phased (with --diploid) a third section follows: the calls become the truth's own tables again (the truth's key planned and
genotyped once more) with 1 % of the heterozygous records on the other haplotype, joined; the truth's words are one phase set per
contig, the calls' sets of 4096 records (msim_cmp_phase_set).  Every record then has a partner and half of them are pairs.  Per
genome, medians of `runs` with min and max, all from this process:
  cmp_phase_kernel_ms           msim_cmp_phase_counts (msim_cmp_phase_timing: its six kernels)
  phased_cmp_diploid_kernel_ms  k_cmp_match<3> + k_cmp_tally<3> on the same tables (msim_cmp_counts_diploid, which the pass follows)
  phase_copy_floor_ms           a device-to-device copy of the bytes the phase pass reads and writes (msim_dbg_cmp_phase_copy_floor)

With --regions (anywhere on the line) the same two tables are marked and tallied again inside region sets, behind the plain runs and in
the same process: `dense` sets of 1000 bases in every 2000 (about 1.5 M intervals a set over the genome) and `sparse` sets of 100 in
every 100 000, one resident set and eight different ones (set s shifted by s / 8 of the period).  Per configuration
regions_<dense|sparse>_<1|8>_*, medians of `runs` with min and max:
  mark_ms             k_region_mark over the 24 contigs, both tables (msim_cmp_regions_timing around msim_cmp_regions_mark)
  tally_ms            one k_region_tally<2> pass over them, mask = set 0 (msim_cmp_counts_regions)
  mark_over_match     mark_ms over cmp_kernel_ms of the plain comparison; mark_over_floor: over copy_floor_ms"""
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "mutation-simulator_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

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


def snp_alt_table():
    """alt[aux, base]: the byte an SN writes (tests/apply_ref.py's tables; 0: the reference has none)."""
    import apply_ref
    conv = apply_ref.NON_AMBIGUOUS
    alt = np.zeros((3, 256), dtype=np.uint8)
    alt[0] = apply_ref.TRANSITIONS[conv]
    for x in range(256):
        pair = apply_ref.TRANSVERSIONS.get(chr(int(conv[x])))
        if pair:
            alt[1, x], alt[2, x] = ord(pair[0]), ord(pair[1])
    return alt


def derived_calls(eng, cid, share=0.01):
    """The contig's held table with `share` of its records picked and re-represented (see above): (records, pool)."""
    a, pa, _, _ = eng.cmp_fetch(cid, flags=False)
    g = eng.read_contig(cid)
    n = len(a)
    rs = np.random.RandomState(cid)
    pick = rs.random_sample(n) < share
    pos = a["pos"].astype(np.int64)
    length = a["stop"].astype(np.int64) - pos + 1
    nxt = np.append(pos[1:], len(g))
    alt = snp_alt_table()[a["aux"] % 3, g[pos]]
    as_mnp = pick & (a["type"] == 1) & (pos + 3 <= nxt) & (alt != 0)       # an SN as a DE and an IN behind it
    split = pick & (a["type"] == 3) & (length >= 2)                        # a DE in two pieces
    to_in = pick & (a["type"] == 4)                                        # a DU as the IN it is
    drop = pick & ~as_mnp & ~split & ~to_in & (rs.random_sample(n) < 0.25)
    reps = np.ones(n, dtype=np.int64)
    reps[split | as_mnp] = 2
    reps[drop] = 0
    b = np.repeat(a, reps)
    first = np.cumsum(reps) - reps
    i1 = first[split]
    b["stop"][i1] = b["pos"][i1]
    b["pos"][i1 + 1] += 1
    j1 = first[as_mnp]
    b["type"][j1], b["aux"][j1] = 3, 0
    b["type"][j1 + 1], b["aux"][j1 + 1] = 2, 0
    b["pos"][j1 + 1] += 1
    b["stop"][j1 + 1] = b["pos"][j1 + 1]
    b["extra"][j1 + 1] = len(pa) + np.arange(len(j1))
    inserts, off = [pa, alt[as_mnp]], len(pa) + len(j1)
    for k in np.flatnonzero(to_in):
        b["type"][first[k]] = 2
        b["extra"][first[k]] = off
        inserts.append(g[pos[k]:pos[k] + length[k]])
        off += int(length[k])
    return b, np.concatenate(inserts)


def main():
    diploid = "--diploid" in sys.argv
    if diploid:
        sys.argv.remove("--diploid")
    blocks = "--blocks" in sys.argv
    if blocks:
        sys.argv.remove("--blocks")
    if blocks and diploid:
        sys.exit("--blocks replaces the calls' tables: run it without --diploid")
    phased = "--phased" in sys.argv
    if phased:
        sys.argv.remove("--phased")
    if phased and not diploid:
        sys.exit("--phased measures the pass behind the diploid comparison: run it with --diploid")
    regions = "--regions" in sys.argv
    if regions:
        sys.argv.remove("--regions")
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
    phase_floor = _ffi.load().msim_dbg_cmp_phase_copy_floor
    phase_floor.restype, phase_floor.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    split = _ffi.load().msim_dbg_cmp_blocks_split
    split.restype, split.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
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

        def blocks_pass():
            eng.reset_stats()
            got = [eng.cmp_counts_blocks(cid) for cid in cids]
            counts, tallies = sum(g[0] for g in got), sum(g[2] for g in got)
            assert int(counts[..., :3].sum()) == records[0] and int(counts[..., 3:].sum()) == records[1]
            assert int(tallies[0]) == int(tallies[1]) + int(tallies[3]) + int(tallies[4])
            ms, steps = (C.c_double * 2)(), (C.c_uint64 * 2)()
            eng._check(split(eng.h, ms, steps))
            return eng.cmp_blocks_timing(), eng.cmp_timing(), counts, tallies, ms[0], ms[1], steps[0] / max(1, steps[1])

        def blocks_runs(prefix):
            _, _, counts, tallies, *_ = blocks_pass()      # warm-up: code objects, the descriptors' allocation
            res[prefix + "block_matched"] = [int(counts[..., 1].sum()), int(counts[..., 4].sum())]
            res[prefix + "block_tallies"] = [int(t) for t in tallies]
            got = [blocks_pass() for _ in range(runs)]
            res[prefix + "replay_lane_use"] = got[0][6]
            for name, col in (("cmp_block_kernel_ms", 0), ("cmp_kernel_ms_in_blocks", 1), ("blk_scan_ms", 4), ("blk_replay_ms", 5)):
                res[prefix + name] = statistics.median(g[col] for g in got)
                res[prefix + name + "_min_max"] = [min(g[col] for g in got), max(g[col] for g in got)]

        def region_sets(L, period, width, n_sets):
            """n_sets different sets of a contig: `width` bases in every `period`, set s shifted by s * period / 8."""
            out = []
            for s in range(n_sets):
                starts = np.arange(s * (period // 8), L - width, period, dtype=np.int64)
                out.append((starts.astype(np.uint32), (starts + width).astype(np.uint32)))
            return out

        def regions_pass(mask):
            """(k_region_mark ms over the contigs, one k_region_tally<2> pass ms over them, records inside a side, outside a side)"""
            eng.reset_stats()
            for cid in cids:
                eng.cmp_regions_mark(cid)
            mark_ms = eng.cmp_regions_timing()
            got = [eng.cmp_counts_regions(cid, mask) for cid in cids]
            tally_ms = eng.cmp_regions_timing() - mark_ms
            counts, outside = sum(g[0] for g in got), sum(g[1] for g in got)
            assert int(counts[..., :2].sum()) + int(outside[0]) == records[0] and int(counts[..., 2:].sum()) + int(outside[1]) == records[1]
            assert (counts[..., 0] == counts[..., 2]).all()
            return mark_ms, tally_ms, [int(counts[..., :2].sum()), int(counts[..., 2:].sum())], [int(x) for x in outside]

        if regions:                                    # (behind the plain runs: their flag bytes are the ones tallied again)
            for tag, period, width in (("dense", 2000, 1000), ("sparse", 100_000, 100)):
                for n_sets in (1, 8):
                    eng.cmp_regions_drop()
                    n_iv = 0
                    for cid, L in zip(cids, lengths):
                        for s, (starts, ends) in enumerate(region_sets(L, period, width, n_sets)):
                            eng.cmp_regions_set(cid, s, starts, ends)
                            n_iv += len(starts) if s == 0 else 0
                    name = f"regions_{tag}_{n_sets}"
                    _, _, inside, outside = regions_pass(1)        # warm-up: code objects, the mark bytes' allocation
                    res[name + "_intervals_a_set"], res[name + "_inside"], res[name + "_outside"] = n_iv, inside, outside
                    got = [regions_pass(1)[:2] for _ in range(runs)]
                    for what, col in (("mark_ms", 0), ("tally_ms", 1)):
                        res[f"{name}_{what}"] = statistics.median(g[col] for g in got)
                        res[f"{name}_{what}_min_max"] = [min(g[col] for g in got), max(g[col] for g in got)]
                    res[name + "_mark_over_match"] = res[name + "_mark_ms"] / statistics.median(rows)
                    res[name + "_mark_over_floor"] = res[name + "_mark_ms"] / statistics.median(floors)
            eng.cmp_regions_drop()
        if blocks:                                     # (in front of the joins: they consume the held tables)
            blocks_runs("")
            for cid in cids:
                eng.set_records(cid, *derived_calls(eng, cid))
            records[1] = sum(eng.result_sizes(cid, applied=False)[1] for cid in cids)
            res["derived_calls_records"] = records[1]
            _, counts, _ = kernel_pass()
            res["derived_matched"] = int(counts[..., 0].sum())
            plain, plain_floor = [], []
            for _ in range(runs):
                plain.append(kernel_pass()[0])
                plain_floor.append(copy_pass())
            res["derived_cmp_kernel_ms"] = statistics.median(plain)
            res["derived_cmp_kernel_ms_min_max"] = [min(plain), max(plain)]
            res["derived_copy_floor_ms"] = statistics.median(plain_floor)
            res["derived_copy_floor_ms_min_max"] = [min(plain_floor), max(plain_floor)]
            blocks_runs("derived_")
            records[1] = res["calls_records"]              # (the figures below are the independent pair's)
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
        if phased:                                     # (last: the calls' tables are replaced)
            rs = np.random.RandomState(7)
            eng.set_fast_key(KEYS[0])
            swapped = 0
            for i, (cid, ch) in enumerate(zip(cids, sim.chromosomes)):
                eng.plan_contig(cid, mm.plan_table(ch))
                eng.genotype_contig(cid, KEYS[0], i, HET_THR)
                gt = eng.fetch_genotypes(cid, eng.result_sizes(cid, applied=False)[1])
                flip = (gt != 3) & (rs.random_sample(len(gt)) < 0.01)
                gt[flip] = 3 - gt[flip]
                swapped += int(flip.sum())
                eng.set_genotypes(cid, gt)
                join_pass_one(eng, cid, _ffi.CMP_CALLS)
                for side in (_ffi.CMP_TRUTH, _ffi.CMP_CALLS):
                    n = C.c_uint64()
                    eng._check(eng.lib.msim_cmp_fetch_diploid(eng.h, cid, side, C.byref(n), None, None, None, None, None), cid)
                    words = np.ones(n.value, dtype=np.uint32) if side == _ffi.CMP_TRUTH else 1 + (np.arange(n.value, dtype=np.uint32) >> 12)
                    eng.cmp_phase_set(cid, side, words)
            res["phased_swapped_hets"] = swapped

            def phased_pass():
                """(phase ms, the diploid comparison's ms on the same tables, copy floor ms, the summed counts)"""
                eng.reset_stats()
                out, floor_ms = np.zeros(_ffi.CMP_PHASE_COUNTS, dtype=np.uint64), 0.0
                for cid in cids:
                    eng.cmp_counts_diploid(cid)
                    out += eng.cmp_phase_counts(cid)
                dip_ms, phase_ms = eng.cmp_timing(), eng.cmp_phase_timing()
                for cid in cids:
                    ms = C.c_double()
                    eng._check(phase_floor(eng.h, cid, C.byref(ms)), cid)
                    floor_ms += ms.value
                return phase_ms, dip_ms, floor_ms, out

            out = phased_pass()[3]                         # warm-up: code objects, the pass's scratch
            res["phase_counts"] = [int(x) for x in out]
            phases = [phased_pass()[:3] for _ in range(runs)]
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
    if phased:
        for name, col in (("cmp_phase_kernel_ms", 0), ("phased_cmp_diploid_kernel_ms", 1), ("phase_copy_floor_ms", 2)):
            res[name] = med(p[col] for p in phases)
            res[name + "_min_max"] = [min(p[col] for p in phases), max(p[col] for p in phases)]
        res["phase_over_floor"] = res["cmp_phase_kernel_ms"] / res["phase_copy_floor_ms"]
        res["phase_over_diploid_counts"] = res["cmp_phase_kernel_ms"] / res["phased_cmp_diploid_kernel_ms"]
    for k, v in res.items():
        print(f"{k}: {v:.4g}" if isinstance(v, float) else f"{k}: {v}")
    if out_path:
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
