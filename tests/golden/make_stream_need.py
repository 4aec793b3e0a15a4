"""Record ``stream_need.json``: what the stream-window arithmetic of the device PLAN engines (csrc/plan_windows.h) gave at the
commit BEFORE it got a header of its own -- the expected values of tests/test_stream_need_host.py.

The table is NOT made from the code under test.  ``stream_need_parent_export.patch`` adds the test export
``msim_dbg_stream_need`` to the parent commit, with that commit's expressions copied verbatim out of ``gpu_plan_make_room``,
``enqueue_sample_chain``, ``plan_contig_gpu_hostsample`` and ``plan_contig_gpu_mixed``:

    git worktree add /tmp/parent b754764abd8b20d00cff209baa198cc47dd5f343
    git -C /tmp/parent apply tests/golden/stream_need_parent_export.patch      (path of this checkout's patch)
    make -C /tmp/parent/mutation-simulator_amd/csrc
    python tests/golden/make_stream_need.py --lib /tmp/parent/mutation-simulator_amd/lib/libmsim.so            # rewrites the JSON
    python tests/golden/make_stream_need.py --lib ... --check                                                   # compares, bit for bit

A case is a msim_params, a few type tables (``settings``) and rows ``[setting, start, stop, k, setsize]``; the test rebuilds the
msim_range table from them, so the JSON is all it reads.
"""
from __future__ import annotations

import ctypes as C
import json
import random
import sys
from math import ceil, log
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1] / "mutation-simulator_amd"))
from mutation_simulator_amd._ffi import Params, Range  # noqa: E402

OUT = HERE / "stream_need.json"
PARENT = "b754764abd8b20d00cff209baa198cc47dd5f343"
FIELDS = ("py", "np", "bad", "big_window", "small_e", "small_v", "acc_min")
SN, IN, DE, DU, IV, TL, TLI = range(1, 8)
ONE = 1 << 53


def setsize(k):
    """CPython's random.sample: the population size up to which it takes the pool path."""
    return 21 + (4 ** ceil(log(k * 3, 4)) if k > 5 else 0)


def setting(types, cdf, lens=None):
    """cdf: cumulative thresholds as fractions of 2^53 (ints are taken as they are)."""
    thr = [t if isinstance(t, int) else int(t * ONE) for t in cdf]
    lo, hi = [0] * 8, [0] * 8
    for t, (a, b) in (lens or {}).items():
        lo[t], hi[t] = a, b
    return {"types": list(types), "cdf_thr": thr, "min_len": lo, "max_len": hi}


SN_ONLY = setting([SN], [ONE])
SV = setting([SN, IN, DE, DU, IV], [0.8, 0.85, 0.9, 0.95, ONE], {IN: (1, 50), DE: (1, 1025), DU: (5, 68), IV: (2, 9)})
INS = setting([IN, SN], [0.25, ONE], {IN: (10, 4000)})
TLS = setting([SN, TL, TLI], [0.9, 0.95, ONE], {TL: (100, 611)})
TLI_ONLY = setting([SN, TLI], [0.5, ONE])
# entries 0 and 1 cannot be drawn (threshold 0), entry 3 starts at or beyond 2^53: only the SNP is drawable
EDGES = setting([IN, DE, SN, DU], [0, 0, ONE + 5, 1 << 54], {IN: (1, 3), DE: (1, 3), DU: (1, 3)})
# ... and the same with a drawable entry in front, the SNP ending beyond 2^53
EDGES2 = setting([DE, IN, SN, IV], [0, 0.5, ONE + 1, ONE + 2], {DE: (1, 7), IN: (1, 1), IV: (1, 100)})
# widths outside 1 .. 2^32 - 1 (never past an engine's eligibility): skipped by the least acceptance
ODD_W = setting([SN, IV, DE, DU], [0.4, 0.6, 0.8, ONE], {IV: (10, 5), DE: (1, 1 << 32), DU: (1, 3)})


def row(s, start, n, k, d=1, ss=None):
    """A range of population n at sampling distance d: stop = start + n + (k - 1) d."""
    return [s, start, start + n + (k - 1) * d, k, setsize(k) if ss is None else ss]


def big_table():
    """2,000 ranges mixing three settings: SNP-only gene blocks, an SV `std` line between them, pool-path hot spots; some draw nothing."""
    rng = random.Random(20261019)
    rows, at = [], 1000
    for i in range(2000):
        kind = rng.randrange(10)
        if kind < 5:
            k = rng.randrange(1, 400); n = rng.randrange(40 * k + 2000, 200 * k + 4000); s = 0
        elif kind < 8:
            k = rng.randrange(1, 3000); n = rng.randrange(20 * k + 2000, 60 * k + 4000); s = 1
        elif kind < 9:
            k = rng.randrange(6, 300); n = rng.randrange(k, setsize(k) + 1); s = 2            # hot spot: pool path
        else:
            k = 0; n = rng.randrange(100, 5000); s = 0
        if i == 700:
            k, n, s = 250000, 30000000, 1                                                    # one range with a window of its own
        r = row(s, at, n, k) if k else [s, at, at + n, 0, 21]
        rows.append(r)
        at = r[2] + rng.randrange(1, 500)
    return rows


def cases():
    B1 = [0] + [1] * 7
    out = []

    def add(name, settings, rows, block=B1, ti_lim=ONE // 3 + 1):
        out.append({"name": name, "block": list(block), "ti_lim": ti_lim, "settings": settings, "ranges": rows})

    add("pool_k100", [SN_ONLY], [row(0, 10, 1000, 100)])
    add("pool_k100_n_eq_setsize", [SN_ONLY], [row(0, 10, setsize(100), 100)])
    add("small_set_k100", [SN_ONLY], [row(0, 0, 100000, 100)])
    add("small_set_k100_just_above_setsize", [SN_ONLY], [row(0, 0, setsize(100) + 1, 100)])
    add("small_set_k4095", [SN_ONLY], [row(0, 0, 3000000, 4095)])
    add("big_k4096", [SN_ONLY], [row(0, 0, 1000000, 4096)])
    add("big_k1e6", [SN_ONLY], [row(0, 5, 100000000, 1000000)])
    add("big_k1e6_sv", [SV], [row(0, 5, 250000000, 1000000)])
    add("big_n_2m_plus_1", [SN_ONLY], [row(0, 0, (1 << 20) + 1, 5000)])
    add("big_n_2m_minus_1", [SN_ONLY], [row(0, 0, (1 << 20) - 1, 5000)])
    add("big_n_2m", [SN_ONLY], [row(0, 0, 1 << 20, 5000)])
    add("small_n_2m_plus_1", [SN_ONLY], [row(0, 0, (1 << 16) + 1, 200)])
    add("small_n_2m_minus_1", [SN_ONLY], [row(0, 0, (1 << 16) - 1, 200)])
    add("big_n_2p31_plus_1", [SN_ONLY], [row(0, 0, (1 << 31) + 1, 100000)])
    add("big_n_2p32_minus_1", [SN_ONLY], [row(0, 0, (1 << 32) - 1, 100000)])
    add("small_k_close_to_n", [SN_ONLY], [row(0, 0, 1003, 1000, ss=21)])
    add("big_k_close_to_n", [SN_ONLY], [row(0, 0, 5010, 5000, ss=21)])
    add("small_k_eq_n_guard", [SN_ONLY], [row(0, 0, 500, 500, ss=21)])
    add("big_k_eq_n_guard", [SN_ONLY], [row(0, 0, 6000, 6000, ss=21)])
    add("n_lt_k_small", [SN_ONLY], [row(0, 0, 500, 600, ss=21)])
    add("n_lt_k_pool", [SN_ONLY], [row(0, 0, 500, 600)])
    add("n_lt_k_second_range", [SN_ONLY], [row(0, 0, 100000, 100), row(0, 200000, 50, 70, ss=21)])
    add("n_2p32", [SN_ONLY], [row(0, 0, 1 << 32, 10000)])
    add("n_beyond_2p33", [SV], [row(0, 0, (1 << 33) + 5, 100)])
    add("n_2p32_pool", [SN_ONLY], [row(0, 0, 1 << 32, 10000, ss=1 << 33)])
    add("k0_between", [SN_ONLY, SV], [row(0, 0, 100000, 100), [1, 200000, 300000, 0, 21], row(1, 400000, 2000000, 5000)])
    add("negative_k_skipped", [SN_ONLY], [row(0, 0, 100000, 100), [0, 200000, 300000, -5, 21]])
    add("thresholds_0_and_2p53", [EDGES], [row(0, 0, 400000, 2000)])
    add("thresholds_0_and_2p53_drawable", [EDGES2], [row(0, 0, 400000, 8000)])
    add("draws_inserts_small", [INS], [row(0, 0, 400000, 2000)])
    add("draws_inserts_big", [INS, SV], [row(0, 0, 40000000, 200000), row(1, 50000000, 600000, 3000)])
    add("draws_tl", [TLS], [row(0, 0, 9000000, 50000)])
    add("draws_tli_only", [TLI_ONLY], [row(0, 0, 90000, 500)])
    add("sn_tl_then_sn_only", [TLS, SN_ONLY], [row(0, 0, 90000, 500), row(1, 100000, 90000, 700)])
    add("odd_widths", [ODD_W], [row(0, 0, 900000, 4500)])
    add("sn_block_above_d", [SN_ONLY, SV], [row(0, 0, 100000, 100), row(1, 200000, 3000000, 9000)], block=[0, 5, 1, 1, 1, 1, 1, 1])
    add("d3_all", [SV], [row(0, 7, 1000000, 4096, d=3), row(0, 3000000, 2000, 100, d=3)], block=[0] + [3] * 7)
    add("d2_sn_block_4", [SN_ONLY], [row(0, 0, 70000, 3000, d=2)], block=[0, 4, 2, 9, 2, 7, 3, 2])
    add("d1_min_is_last", [SV], [row(0, 0, 70000, 3000)], block=[0, 9, 8, 7, 6, 5, 4, 1])
    add("table_2000_three_settings", [SN_ONLY, SV, INS], big_table())
    return out


def range_table(case):
    rs = (Range * len(case["ranges"]))()
    for r, (s, start, stop, k, ss) in zip(rs, case["ranges"]):
        st = case["settings"][s]
        r.start, r.stop, r.k, r.setsize, r.n_types = start, stop, k, ss, len(st["types"])
        for j, (t, thr) in enumerate(zip(st["types"], st["cdf_thr"])):
            r.types[j], r.cdf_thr[j] = t, thr
        for t in range(8):
            r.min_len[t], r.max_len[t] = st["min_len"][t], st["max_len"][t]
    return rs


def stream_need(lib, case):
    """The seven doubles of msim_dbg_stream_need as a dict (``bad`` as a bool)."""
    fn = lib.msim_dbg_stream_need
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(Params), C.POINTER(Range), C.c_int, C.POINTER(C.c_double)]
    p = Params()
    p.block[:] = case["block"]
    p.ti_lim = case["ti_lim"]
    rs = range_table(case)
    out = (C.c_double * 7)()
    rc = fn(C.byref(p), rs, len(rs), out)
    assert rc == 0, (case["name"], rc)
    d = dict(zip(FIELDS, out))
    d["bad"] = bool(d["bad"])
    return d


def main(argv):
    lib = C.CDLL(argv[argv.index("--lib") + 1])
    cs = cases()
    for c in cs:
        c["expect"] = stream_need(lib, c)
    doc = {"parent": PARENT,
           "recorded_from": "the parent commit + stream_need_parent_export.patch (its own expressions, verbatim); see make_stream_need.py",
           "fields": list(FIELDS), "cases": cs}
    lines = ["{", f' "parent": {json.dumps(doc["parent"])},', f' "recorded_from": {json.dumps(doc["recorded_from"])},',
             f' "fields": {json.dumps(doc["fields"])},', ' "cases": [']
    lines += ["  " + json.dumps(c, separators=(",", ":")) + ("," if i + 1 < len(cs) else "") for i, c in enumerate(cs)]
    text = "\n".join(lines + [" ]", "}"]) + "\n"
    if "--check" in argv:
        assert OUT.read_text() == text, "stream_need.json differs from what this library gives"
        print("stream_need.json: identical")
    else:
        OUT.write_text(text)
        print(f"wrote {OUT} ({len(cs)} cases, {len(text)} bytes)")


if __name__ == "__main__":
    main(sys.argv)
