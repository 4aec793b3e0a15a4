"""Python restatement of ``compare --blocks`` (``msim_cmp_counts_blocks``; include/msim.h), written from its rule -- test
infrastructure shared by the CPU and the GPU tier.  The device kernels (csrc/cmp_blocks.hip) and the library's sequential
restatement (``msim_dbg_cmp_counts_blocks``) must agree with it exactly.

* ``segments``: both tables merged by position (the truth's record first at equal pos); a record starts a block when it stands
  more than ``gap`` bases behind the largest footprint end in front of it.
* ``stop_rule``: a block walked in merged order -- the first TL / TLI, the 65th record, the first footprint end more than 4096
  bases behind the block's first pos.
* the replay is literally ``apply_ref.apply(bases, the block's records of one side)`` on the whole contig, the two results compared
  whole: in front of the block and behind it both are the contig's own bytes, so this is the comparison of the block's stretch.
  A side whose rewrite raises the reference's KeyError equals nothing.
* ``compare``: flags (it starts from ``cmp_twin.compare``'s), counts ``[8, BINS, 6]`` and the five block tallies.

Nothing here knows a cursor, a descriptor or a binary search.  The cases at the end are shared by both tiers.
"""
from __future__ import annotations

import functools

import numpy as np

import apply_ref
import cmp_twin as tw
from cmp_twin import DE, DU, IN, IV, SN, TL, TLI, Table

GAP = 50                     # msim.h: MSIM_CMP_BLOCK_GAP
MAX_RECORDS = 64             # msim.h: MSIM_CMP_BLOCK_RECORDS
MAX_SPAN = 4096              # msim.h: MSIM_CMP_BLOCK_SPAN


def foot_end(rec) -> int:
    pos, stop, _, typ, _ = rec
    return stop if typ in (DE, DU, IV, TL) else pos


def segments(truth, calls, gap: int):
    """The blocks, in order: lists of (side, index, record) with side 0 = truth, 1 = calls."""
    merged = [(r[0], 0, i, r) for i, r in enumerate(tw.fields(truth))] + [(r[0], 1, j, r) for j, r in enumerate(tw.fields(calls))]
    merged.sort(key=lambda m: (m[0], m[1]))
    out, end = [], None
    for pos, side, k, rec in merged:
        if end is None or pos - end > gap:
            out.append([])
            end = foot_end(rec)
        end = max(end, foot_end(rec))
        out[-1].append((side, k, rec))
    return out


def stop_rule(block):
    """None, "limit" or "translocation": what the first record that ends the walk early says."""
    lo = block[0][2][0]
    for n, (_, _, rec) in enumerate(block, 1):
        if rec[3] in (TL, TLI):
            return "translocation"
        if n > MAX_RECORDS or foot_end(rec) - lo > MAX_SPAN:
            return "limit"
    return None


def replayed(bases, recs, pool, picked):
    """The whole contig rewritten with the picked records alone; None for the reference's KeyError."""
    res = apply_ref.apply(bases, recs[np.asarray(picked, dtype=np.int64)], pool)
    return None if res.key_error is not None else res.seq.tobytes()


def compare(bases, truth, truth_pool, calls, calls_pool, exact: bool = False, gap: int = GAP):
    """(counts uint64[8, BINS, 6], tallies uint64[2], block tallies uint64[5], truth flags uint8, calls flags uint8)."""
    bases = tw.as_bases(bases)
    _, tallies, fa, fb = tw.compare(bases, truth, truth_pool, calls, calls_pool, exact)
    flags = (fa, fb)
    blocks = np.zeros(5, dtype=np.uint64)                  # candidates, replayed, equal, over a limit, holding a translocation
    for block in segments(truth, calls, gap):
        if all(flags[side][k] for side, k, _ in block):
            continue
        blocks[0] += 1
        why = stop_rule(block)
        if why is not None:
            blocks[3 if why == "limit" else 4] += 1
            continue
        blocks[1] += 1
        a = replayed(bases, truth, truth_pool, [k for side, k, _ in block if side == 0])
        b = replayed(bases, calls, calls_pool, [k for side, k, _ in block if side == 1])
        if a is None or b is None or a != b:
            continue
        blocks[2] += 1
        for side, k, _ in block:
            if flags[side][k] == 0:
                flags[side][k] = 2
    counts = np.zeros((8, tw.BINS, 6), dtype=np.uint64)
    for recs, fl, col in ((truth, fa, 0), (calls, fb, 3)):
        n = recs["stop"].astype(np.int64) - recs["pos"].astype(np.int64) + 1
        typ = recs["type"].astype(np.int64)
        bins = np.where((typ == IN) | (typ == DE), np.digitize(n, [2, 6, 21, 51]), 0)
        np.add.at(counts, (typ, bins, col + np.where(fl == 1, 0, np.where(fl == 2, 1, 2))), 1)
    return counts, tallies, blocks, fa, fb


# ---- the cases: {id: (bases, truth, truth pool, calls, calls pool, exact, gap)} ------------------------------------------------
def case(bases, truth: Table, calls: Table, exact=False, gap=GAP):
    return tw.case(bases, truth, calls, exact) + (gap,)


def mirror(c):
    bases, a, pa, b, pb, exact, gap = c
    return bases, b, pb, a, pa, exact, gap


G = tw.RANDOM_200            # GATTACAGGC ...: "AT" at 1, "AC" at 4


def mnp_cases():
    p = 4                                                  # "AC" -> "GT": one MNP line (DE + IN) against two transitions
    mnp = case(G, Table().de(p, 2).ins(p + 2, "GT"), Table().sn(p, 0).sn(p + 1, 0))
    return {"mnp_vs_snps": mnp, "snps_vs_mnp": mirror(mnp)}


def cross_type_cases():
    p, s = 10, 15
    span = G[p:s + 1]
    out = {"du_vs_in_at_start": case(G, Table().raw(p, s, DU), Table().ins(p, span)),
           "du_vs_in_behind": case(G, Table().raw(p, s, DU), Table().ins(s + 1, span))}
    out["in_vs_du"] = mirror(out["du_vs_in_at_start"])
    out["du_vs_other_in"] = case(G, Table().raw(p, s, DU), Table().ins(p, span[:-1] + ("A" if span[-1] != "A" else "C")))
    return out


def inversion_cases():
    return {"iv_vs_transitions": case(G, Table().raw(4, 5, IV), Table().sn(4, 0).sn(5, 0)),
            "iv_palindrome_vs_nothing": case(G, Table().raw(1, 2, IV), Table()),
            "nothing_vs_iv_palindrome": case(G, Table(), Table().raw(1, 2, IV))}


def gap_edge_cases():
    """A DE of the first A of a run and an IN of an A behind the run write the contig's own bytes: equal against an empty table
    when one block, two unequal blocks when not.  Inside one table the next record stands at least one base behind a footprint
    end, so at gap 0 only the far side exists there; the near side at gap 0 is a DU against the IN it is, at distance 0 and 1."""
    out = {}
    for gap in (0, 1, 50):
        for d in (gap, gap + 1):
            if d == 0:
                continue
            g = "C" + "A" * d + "GTCA"
            out[f"gap{gap}_distance{d}"] = case(g, Table().de(1).ins(1 + d, "A"), Table(), gap=gap)
    g = "GGTCAGG"
    for gap in (0, 1):
        out[f"gap{gap}_du_in_distance0"] = case(g, Table().raw(3, 3, DU), Table().ins(3, "C"), gap=gap)
        out[f"gap{gap}_du_in_distance1"] = case(g, Table().raw(3, 3, DU), Table().ins(4, "C"), gap=gap)
    return out


def exact_cases():
    g = "GTCAAAAGTC"
    return {"shifted_de_exact": case(g, Table().de(3), Table().de(5), exact=True),
            "shifted_de_normalised": case(g, Table().de(3), Table().de(5))}


def random_bases(n, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(seed).randint(0, 4, n)].copy()


def limit_cases():
    """Blocks at the two limits, built to be EQUAL where the limit lets them be replayed: palindromes' inversions (they write the
    contig's own bytes) and a DU against its IN, chained by matched SN pairs two bases apart."""
    out = {}
    for n_pal, total in ((2, 64), (3, 65)):
        g = "GG" + "ATGG" * n_pal + "C" + "GG" + "AC" * 40
        t, c = Table(), Table()
        for k in range(n_pal):
            t.raw(2 + 4 * k, 3 + 4 * k, IV)
        du = 2 + 4 * n_pal
        t.raw(du, du, DU)
        c.ins(du, "C")
        n_pairs = (64 - 2 - 2) // 2                        # 30 matched SN pairs: 64 records with two palindromes
        for k in range(n_pairs):
            t.sn(du + 3 + 2 * k, k % 3)
            c.sn(du + 3 + 2 * k, k % 3)
        assert len(t.rows) + len(c.rows) == total
        out[f"records_{total}"] = case(g, t, c)
    for span in (4096, 4097):                              # one deletion against the same bases deleted in two pieces
        g = random_bases(4300, 9)
        lo = 100
        out[f"span_{span}"] = case(g, Table().de(lo, span + 1), Table().de(lo, 4096).de(lo + 4096, span + 1 - 4096))
    g = G
    out["tl_in_block"] = case(g, Table().sn(20, 1).raw(30, 34, TL).raw(100, 34, TLI, aux=0, extra=30), Table())
    out["tli_in_block"] = case(g, Table().raw(30, 34, TL).sn(95, 1).raw(100, 34, TLI, aux=1, extra=30), Table(), gap=10)
    t = Table()
    for k in range(64):
        t.sn(2 * k, k % 3)
    out["tl_is_record_65"] = case(g, t.raw(130, 133, TL), Table())
    out["de_is_record_65"] = case(g, t_copy(t.rows[:-1]).de(130, 4), Table())
    return out


def t_copy(rows):
    t = Table()
    t.rows = list(rows)
    return t


def edge_cases():
    g = "ACGGTTGGAC"
    L = len(g)
    out = {"block_at_pos0": case(g, Table().raw(0, 1, IV), Table().sn(0, 0).sn(1, 0)),
           "block_at_last_base": case(g, Table().raw(L - 2, L - 1, IV), Table().sn(L - 2, 0).sn(L - 1, 0)),
           "whole_contig_one_block": case("AC", Table().raw(0, 1, IV), Table().sn(0, 0).sn(1, 0)),
           "prefix_at_contig_end": case(g, Table().de(L - 2, 2), Table().de(L - 2, 1)),
           "prefix_inside": case("GGTAGG", Table().ins(3, "AA"), Table().ins(3, "A"))}
    h = "GGRCGGNGGaGGRaGG"
    out["sn_on_R"] = case(h, Table().sn(2, 0), Table().de(2).ins(3, "G"))            # R -> A, its transition: G
    out["sn_on_N"] = case(h, Table().sn(6, 0), Table())                             # N stays N: the contig's own byte
    out["sn_on_N_transversion"] = case(h, Table().sn(6, 2), Table())
    out["sn_on_lower_case"] = case(h, Table().sn(9, 0), Table())                    # a stays a
    out["sn_key_error"] = case(h, Table().sn(9, 1), Table())                        # no outcome: equals nothing
    out["iv_on_R"] = case(h, Table().raw(2, 3, IV), Table().sn(2, 0).sn(3, 0))      # "RC" reversed and complemented: "GT"
    out["iv_on_R_and_lower_case"] = case(h, Table().raw(12, 13, IV), Table().de(12, 2).ins(14, "aT"))
    return out


def non_rescue_cases():
    g = "GGCAAAAAAGGTTCC"
    return {"one_unmatched_snp": case(G, Table().sn(20, 0).sn(24, 1).sn(28, 2), Table().sn(20, 0).sn(28, 2)),
            "shifted_pair_around_a_snp": case(g, Table().de(4).sn(6, 1), Table().sn(6, 1).de(8))}


def grid_case(PASS: int, gap: int = 5):
    """3 x PASS + 1 records a side, one a unit: a DU of one base in the truth against its IN in the calls (equal), every third
    unit with another inserted base (unequal), every fifth a matched SN pair (no candidate).  Units stand gap + 3 bases apart --
    a block each -- but records PASS - 1 .. PASS + 1 and 2 PASS - 1 .. 2 PASS + 1, which stand 3 apart: a block across the edge
    of a pass, on both sides, rescuable."""
    n = 3 * PASS + 1
    near = {PASS, PASS + 1, 2 * PASS, 2 * PASS + 1}
    pos, at = [], 2
    for k in range(n):
        at += 3 if k in near else gap + 3
        pos.append(at)
    rs = np.random.RandomState(3)
    g = random_bases(at + 8, 4)
    t, c = Table(), Table()
    for k, p in enumerate(pos):
        base = bytes([int(g[p])])
        if k % 5 == 4 and k not in near and k + 1 not in near:
            t.sn(p, k % 3)
            c.sn(p, k % 3)
        elif k % 3 == 2 and k not in near and k + 1 not in near:
            t.raw(p, p, DU)
            c.ins(p, b"A" if base != b"A" else b"C")
        else:
            t.raw(p, p, DU)
            c.ins(p, base)
    del rs
    return case(g, t, c, gap=gap)


def rerepresented(seed: int):
    """A random truth table (``cmp_twin.random_tables``; some of its deletions turned into duplications) and calls made of it by
    re-representation -- an SN as a deletion and an insertion, a deletion in two pieces, a DU as the IN it is --, a record dropped
    now and then, an SNP added now and then: blocks that are rescued and blocks that are not."""
    g, a, pa, _, _, _ = tw.random_tables(seed, letters=b"ACGT", n=16)
    rs = np.random.RandomState(1000 + seed)
    L = len(g)
    rows = tw.fields(a)
    t, c = Table(), Table()
    for k, (pos, stop, extra, typ, aux) in enumerate(rows):
        nxt = rows[k + 1][0] if k + 1 < len(rows) else L
        n = stop - pos + 1
        what = int(rs.randint(0, 8))
        if typ == DE and rs.randint(0, 3) == 0:
            typ = DU
        if typ == SN:
            t.sn(pos, aux)
            alt = bytes([apply_ref.apply(g, a[k:k + 1], pa).seq[pos]])
            if what < 3 and pos + 3 <= nxt and pos + 1 < L:
                c.de(pos).ins(pos + 1, alt)
            elif what < 7:
                c.sn(pos, aux)
        elif typ == DE:
            t.de(pos, n)
            if what < 3 and n >= 2:
                c.de(pos, 1).de(pos + 1, n - 1)
            elif what < 7:
                c.de(pos, n)
        elif typ == DU:
            t.raw(pos, stop, DU)
            if what < 4:
                c.ins(pos, bytes(g[pos:stop + 1]))
            elif what < 7:
                c.raw(pos, stop, DU)
        else:
            S = bytes(pa[extra:extra + n])
            t.ins(pos, S)
            if what < 7:
                c.ins(pos, S)
        free = tw.consumed_to(typ, pos, stop) + 3
        if rs.randint(0, 12) == 0 and free + 3 <= nxt:
            c.sn(free, int(rs.randint(0, 3)))
    return case(g, t, c, exact=bool(seed % 7 == 0), gap=(0, 2, 5, 50)[seed % 4])


RANDOM_SEEDS = range(200)


@functools.lru_cache(maxsize=None)
def cases(PASS: int):
    out = {}
    for part in (mnp_cases(), cross_type_cases(), inversion_cases(), gap_edge_cases(), exact_cases(), limit_cases(), edge_cases(),
                 non_rescue_cases()):
        out.update(part)
    out["grid"] = grid_case(PASS)
    for name, c in tw.small_cases(PASS).items():           # the match's own shapes: every type, ranks, windows, long chains of SNs
        out[f"cmp_{name}"] = c + (GAP,)
    return out


@functools.lru_cache(maxsize=None)
def random_case(seed: int):
    return rerepresented(seed)


@functools.lru_cache(maxsize=None)
def expected(name, PASS: int):
    """The twin's result of a case, computed once for whoever asks."""
    return compare(*(random_case(name) if isinstance(name, int) else cases(PASS)[name]))
