"""Python restatement of ``compare --regions / --stratify`` (``msim_cmp_regions_mark``, ``msim_cmp_counts_regions``;
include/msim.h), written from its rule on top of ``cmp_twin`` -- test infrastructure shared by the CPU and the GPU tier.  The
device kernels and the library's sequential restatement (``msim_dbg_cmp_counts_regions``) must agree with it exactly.

* ``anchor``: an IN / DE record's leftmost placement (``cmp_twin.interval``'s lo); with ``exact``, and for every other type, its pos.
* membership: where the library binary-searches the starts, this paints every interval onto a boolean mask over the contig and
  reads the anchor's base (``member``, ``marks``).
* ``tally``: the records whose mark holds every bit of the mask, counted by their flag bytes as the count call counts them; every
  other record in ``outside``.  The flag bytes come from ``cmp_twin.compare``, ``dip_twin.score`` and ``blk_twin.compare``.

A case is a dict: ``kind`` (haploid, diploid, blocks), ``bases``, ``truth`` / ``calls`` -- (records, pool), or for a diploid case the
side's two haplotype tables (H1, pool, H2, pool) --, ``exact``, ``gap`` (blocks), ``sets`` -- up to eight (starts, ends) in normal
form -- and the ``masks`` to tally.  ``cases(PASS)`` holds the smallest shapes at which the kernels can still go wrong.
"""
from __future__ import annotations

import numpy as np

import blk_twin as bt
import cmp_twin as tw
import dip_twin as dt
from cmp_twin import DE, IN, Table

SETS = 8                     # msim.h: MSIM_CMP_REGION_SETS
W = 1 << tw.WINDOW_SHIFT


def anchor(bases, rec, pool, exact: bool = False) -> int:
    return tw.interval(bases, rec, pool, exact)[0]


def member(L: int, starts, ends) -> np.ndarray:
    """The set as a boolean per base of the contig."""
    m = np.zeros(L, dtype=bool)
    for s, e in zip(np.asarray(starts).tolist(), np.asarray(ends).tolist()):
        m[s:e] = True
    return m


def marks(bases, recs, pool, exact, sets) -> np.ndarray:
    """A mark byte per record: bit s set iff its anchor lies inside set s."""
    bases = tw.as_bases(bases)
    masks = [member(len(bases), s, e) for s, e in sets]
    out = np.zeros(len(recs), dtype=np.uint8)
    for k in range(len(recs)):
        typ = int(recs[k]["type"])
        at = anchor(bases, recs[k], pool, exact) if typ in (IN, DE) else int(recs[k]["pos"])
        out[k] = sum(1 << s for s, m in enumerate(masks) if m[at])
    return out


def tally(truth, fa, ma, calls, fb, mb, mask: int, width: int):
    """(counts uint64[8, BINS, width], outside uint64[2]): width 4 -- matched, missed a side -- or 6 -- flag 1, flag 2, flag 0."""
    half = width // 2
    counts = np.zeros((8, tw.BINS, width), dtype=np.uint64)
    outside = np.zeros(2, dtype=np.uint64)
    for side, (recs, flags, mk) in enumerate(((truth, fa, ma), (calls, fb, mb))):
        inside = (mk & mask) == mask
        outside[side] = int((~inside).sum())
        r, fl = recs[inside], flags[inside].astype(np.int64)
        n = r["stop"].astype(np.int64) - r["pos"].astype(np.int64) + 1
        typ = r["type"].astype(np.int64)
        bins = np.where((typ == IN) | (typ == DE), np.digitize(n, [2, 6, 21, 51]), 0)
        col = (fl == 0).astype(np.int64) if half == 2 else np.array([2, 0, 1])[fl]
        np.add.at(counts, (typ, bins, side * half + col), 1)
    return counts, outside


def tables_of(case):
    """The two tables the marks and flags are of: (truth records, pool, genotype bytes or None), the calls' likewise."""
    if case["kind"] == "diploid":
        return dt.join(*case["truth"]), dt.join(*case["calls"])
    return case["truth"] + (None,), case["calls"] + (None,)


def plain(case):
    """The count call's own (counts, truth flags, calls flags) and its width."""
    (a, pa, ga), (b, pb, gb) = tables_of(case)
    if case["kind"] == "diploid":
        counts, _, fa, fb = dt.score(case["bases"], a, pa, ga, b, pb, gb, case["exact"])
    elif case["kind"] == "blocks":
        counts, _, _, fa, fb = bt.compare(case["bases"], a, pa, b, pb, case["exact"], case["gap"])
    else:
        counts, _, fa, fb = tw.compare(case["bases"], a, pa, b, pb, case["exact"])
    return counts, fa, fb


def expected(case):
    """(truth marks, calls marks, {mask: (counts, outside)}, the count call's own counts, truth flags, calls flags)."""
    (a, pa, _), (b, pb, _) = tables_of(case)
    counts, fa, fb = plain(case)
    ma = marks(case["bases"], a, pa, case["exact"], case["sets"])
    mb = marks(case["bases"], b, pb, case["exact"], case["sets"])
    return ma, mb, {m: tally(a, fa, ma, b, fb, mb, m, counts.shape[-1]) for m in case["masks"]}, counts, fa, fb


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def u32(values) -> np.ndarray:
    return np.asarray(list(values), dtype=np.uint32)


def one(*intervals):
    """A set of the given (start, end) pairs."""
    return u32(s for s, _ in intervals), u32(e for _, e in intervals)


def default_masks(n_sets: int):
    return [0] + [1 << s for s in range(n_sets)] + ([(1 << n_sets) - 1] if n_sets > 1 else [])


def make(kind, bases, truth, calls, sets, exact=False, gap=bt.GAP, masks=None):
    assert len(sets) <= SETS
    build = (lambda side: side[0].build() + side[1].build()) if kind == "diploid" else (lambda t: t.build())
    return {"kind": kind, "bases": tw.as_bases(bases), "truth": build(truth), "calls": build(calls), "exact": exact, "gap": gap,
            "sets": list(sets), "masks": default_masks(len(sets)) if masks is None else masks}


def of_twin(kind, c, sets, masks=None):
    """A case of cmp_twin / blk_twin (bases, truth, pool, calls, pool, exact[, gap]) with region sets."""
    return {"kind": kind, "bases": tw.as_bases(c[0]), "truth": (c[1], c[2]), "calls": (c[3], c[4]), "exact": c[5],
            "gap": c[6] if len(c) > 6 else bt.GAP, "sets": list(sets), "masks": default_masks(len(sets)) if masks is None else masks}


HOMO = tw.RANDOM_200[:20] + "A" * 10 + "C" + tw.RANDOM_200[:19]          # a homopolymer at [20, 30)
REPEAT = "T" + "AC" * 10 + "T"                                            # a tandem repeat at [1, 21)


def random_set(rs, L: int):
    """A seeded random set in normal form on a contig of L bases (possibly empty)."""
    cuts = np.unique(rs.randint(0, L + 1, 2 * int(rs.randint(0, 9))))
    cuts = cuts[:len(cuts) // 2 * 2]
    return u32(cuts[0::2]), u32(cuts[1::2])                # (strictly increasing cuts: start < end < the next start)


def search_case(n: int):
    """n intervals [4k, 4k + 2), k = 1 .. n, and SNPs on every base of a stretch in front of the first, across several, and behind
    the last."""
    L = 4 * n + 16
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[np.arange(L) % 4]
    sets = [(u32(4 * k for k in range(1, n + 1)), u32(4 * k + 2 for k in range(1, n + 1)))]
    at = sorted(set(range(0, min(14, L))) | set(range(max(0, 2 * n - 6), min(L, 2 * n + 7))) | set(range(max(0, 4 * n - 6), L)))
    t, c = Table(), Table()
    for k, p in enumerate(at):
        t.sn(p, 1)
        if k % 3:
            c.sn(p, 1)
    return make("haploid", g, t, c, sets)


def pass_case(PASS: int):
    """3 * PASS + 1 records; the records PASS - 1, PASS, PASS + 1 and the same around 2 * PASS alternate inside and outside."""
    n = 3 * PASS + 1
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[np.arange(2 * n + 2) % 4]
    t, c = Table(), Table()
    for k in range(n):
        t.sn(2 * k, k % 3)
        if k % 5:
            c.sn(2 * k, k % 3)
        else:
            c.sn(2 * k + 1, 0)                             # (the calls table is as long: its pass edges are the truth's)
    inside = [PASS - 1, PASS + 1, 2 * PASS - 1, 2 * PASS + 1]
    return make("haploid", g, t, c, [one(*[(2 * k, 2 * k + 2) for k in inside])])


def cases(PASS: int):
    out = {}
    g = tw.RANDOM_200
    sn4 = lambda: Table().sn(9, 1).sn(10, 1).sn(13, 2).sn(14, 0)                             # noqa: E731
    out["half_open"] = make("haploid", g, sn4(), sn4(), [one((10, 14))])
    # a 1-base DE at 27 has its anchor at 20: outside [25, 40); an SN at 27 is inside; exact: the DE is inside
    for exact in (False, True):
        out["anchor_outside" + ("_exact" if exact else "")] = make("haploid", HOMO, Table().de(27), Table().de(22).sn(27, 1), [one((25, 40))], exact)
    out["pair_across_edge"] = make("haploid", HOMO, Table().de(29), Table().de(20), [one((25, 40)), one((20, 22))])
    out["pair_across_edge_ins"] = make("haploid", REPEAT, Table().ins(15, "AC"), Table().ins(2, "CA"), [one((10, 18)), one((1, 2))])
    # the left walk stops at the window edge: the anchor is exactly W; one set ends at that base, one starts at it
    edge = "A" * (W + 40)
    out["window_edge"] = make("haploid", edge, Table().de(W + 9).ins(W + 20, "AA"), Table().de(W + 30).sn(W - 1, 1),
                              [one((W - 6, W)), one((W, W + 4)), one((10, W + 1))])
    r = tw.random_tables(3)
    out["empty_set"] = of_twin("haploid", r, [one()])
    out["whole_contig"] = of_twin("haploid", r, [one((0, len(r[0])))])
    for n in (1, 2, 3, 1023, 1024, 1025):
        out[f"search_edges_{n}"] = search_case(n)
    out["pass_edges"] = pass_case(PASS)
    rs = np.random.RandomState(8)
    r = tw.random_shifted(22)
    eight = [random_set(rs, len(r[0])) for _ in range(5)] + [one((0, len(r[0]))), one(), one((7, 60), (61, 150))]
    out["eight_sets"] = of_twin("haploid", r, eight, [0] + [1 << s for s in range(8)] + [0b11, 0b10100000, 0b10100101, 0xff])
    # diploid: two records at one position; a genotype-mismatch pair (flag 2) across an edge
    two = lambda: (Table().sn(10, 1).sn(30, 0), Table().sn(10, 2).sn(40, 1))                 # noqa: E731
    out["dip_two_at_one_pos"] = make("diploid", g, two(), two(), [one((10, 11)), one((11, 35))])
    out["dip_gt_mismatch_across_edge"] = make("diploid", HOMO, (Table().de(29).sn(5, 1), Table().de(29)), (Table().de(20), Table().sn(5, 1)),
                                              [one((25, 40)), one((20, 22)), one((0, 21))])
    # blocks: the MNP line against two SNPs, the set holding only part of the block
    out["blocks_part_of_block"] = of_twin("blocks", bt.mnp_cases()["mnp_vs_snps"], [one((4, 5)), one((4, 7)), one((5, 6))])
    for k, (name, c) in enumerate(sorted(tw.random_cases().items())):
        rs = np.random.RandomState(1000 + k)
        out[name] = of_twin("haploid", c, [random_set(rs, len(c[0])), random_set(rs, len(c[0]))])
    return out
