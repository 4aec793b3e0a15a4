"""Hand-built record tables for the liftover-chain tests (tests/test_chain_host.py, tests/test_gpu_chain.py).

``layout`` places records left to right from (type, span, gap) triples, so a case reads as what it is about: ``gap`` untouched
bases in front of the record, ``span`` its length (insert length for IN, linked-span length for TLI).  Every table passes
``check_record_table`` (msim_api.hip): positions strictly increasing, no record inside the input an earlier one consumed.
"""
from __future__ import annotations

import numpy as np

from mutation_simulator_amd._ffi import RECORD_DTYPE

SN, IN, DE, DU, IV, TL, TLI = 1, 2, 3, 4, 5, 6, 7


def layout(items, tail=7, linked=(0, None)):
    """(recs, pool length, contig length).  A TLI copies ``span`` bases from ``linked[0]`` on (anywhere in the contig: the
    chain only needs the length); span 0 is the planner's TLI that found no TL (extra > stop)."""
    rows, pool, at = [], 0, 0
    for typ, span, gap in items:
        p = at + gap
        if typ == SN:
            rows.append((p, p, 0, SN, 0, 0))
            at = p + 1
        elif typ == IN:
            rows.append((p, p + span - 1, pool, IN, 0, 0))
            pool += span
            at = p + 1
        elif typ == TLI:
            start = linked[0]
            rows.append((p, start + span - 1, start, TLI, 2 if p else 0, 0) if span else (p, 0, 1, TLI, 0, 0))
            at = p + 1
        else:
            rows.append((p, p + span - 1, 0, typ, 0, 0))
            at = p + span
    recs = np.array(rows, dtype=RECORD_DTYPE).reshape(-1) if rows else np.zeros(0, dtype=RECORD_DTYPE)
    return recs, pool, at + tail


def _alone(typ, span):
    """The type alone: at position 0, in the middle, at (ending on) the last base."""
    uses = 1 if typ in (SN, IN, TLI) else span
    return {"at_0": layout([(typ, span, 0)], tail=90), "middle": layout([(typ, span, 50)], tail=40),
            "last_base": layout([(typ, span, 100 - uses)], tail=0)}


def hand_cases():
    """name -> (recs, pool length, contig length)"""
    c = {}
    for name, typ, span in (("SN", SN, 1), ("IN", IN, 5), ("DE", DE, 6), ("TL", TL, 6), ("DU", DU, 7), ("IV", IV, 8), ("TLI", TLI, 9),
                            ("DE1", DE, 1), ("DU1", DU, 1), ("IV1", IV, 1)):
        for where, tab in _alone(typ, span).items():
            c[f"{name}_{where}"] = tab
    c["DE_through_the_last_base"] = layout([(SN, 1, 3), (DE, 30, 10)], tail=0)
    c["IN_at_0_then_blocks"] = layout([(IN, 12, 0), (SN, 1, 4), (DE, 3, 5)])
    c["DE_DE_DE_back_to_back"] = layout([(DE, 10, 10), (DE, 10, 0), (DE, 10, 0)], tail=20)
    c["DU_then_IN_at_stop_plus_1"] = layout([(DU, 10, 10), (IN, 4, 0)], tail=20)
    c["IV_next_to_DE"] = layout([(IV, 10, 10), (DE, 10, 0)], tail=20)
    c["DE_next_to_IV"] = layout([(DE, 10, 10), (IV, 10, 0), (DU, 5, 0), (IN, 2, 0)], tail=20)
    c["TL_then_TLI"] = layout([(TL, 10, 10), (SN, 1, 5), (TLI, 10, 14)], tail=20, linked=(10, None))
    c["TLI_then_TL"] = layout([(TLI, 10, 5), (TL, 10, 24)], tail=20, linked=(30, None))
    c["TLI_next_to_TL"] = layout([(DU, 3, 4), (TLI, 4, 0), (TL, 4, 0)], tail=9, linked=(8, None))
    c["TLI_without_a_span"] = layout([(SN, 1, 2), (TLI, 0, 5), (DE, 2, 5)])
    c["wholly_deleted"] = layout([(DE, 100, 0)], tail=0)
    c["wholly_deleted_in_pieces"] = layout([(DE, 40, 0), (TL, 30, 0), (DE, 30, 0)], tail=0)
    c["all_but_one_base_deleted"] = layout([(DE, 40, 0), (DE, 59, 1)], tail=0)
    c["wholly_inverted"] = layout([(IV, 100, 0)], tail=0)
    c["no_records"] = layout([], tail=100)
    c["one_base_no_records"] = layout([], tail=1)
    c["snp_only"] = layout([(SN, 1, g) for g in (0, 0, 3, 17, 0, 50)], tail=5)
    c["snp_on_every_base"] = layout([(SN, 1, 0)] * 40, tail=0)
    c["leading_gaps_merge"] = layout([(DE, 10, 0), (IN, 6, 0), (SN, 1, 3), (DU, 4, 2)], tail=11)
    c["trailing_gaps_merge"] = layout([(IN, 2, 30), (DU, 5, 9), (DE, 5, 0)], tail=0)
    c["trailing_DU"] = layout([(DE, 3, 8), (DU, 10, 20)], tail=0)
    c["leading_and_trailing"] = layout([(IV, 4, 0), (DE, 3, 0), (SN, 1, 6), (DU, 2, 1), (IV, 3, 0)], tail=0)
    c["every_type_with_snps_between"] = layout([(SN, 1, 1), (IN, 3, 2), (SN, 1, 0), (DE, 4, 3), (SN, 1, 0), (DU, 5, 1), (SN, 1, 0),
                                                (IV, 6, 2), (SN, 1, 1), (TL, 7, 2), (SN, 1, 3), (TLI, 7, 1), (SN, 1, 0)],
                                               tail=13, linked=(33, None))
    return c


def huge_cases():
    """Numbers of 1, 9 and 10 digits: a contig of 2^32 - 1 bases given by its length alone (the renderer reads no bases, and no
    device holds such a contig: host renderer only)."""
    L = (1 << 32) - 1
    c = {}
    c["ten_digit_blocks"] = (layout([(IN, 1, 5), (DE, 123_456_789, 1_000_000_000), (IN, 999_999_999, 2_000_000_000)], tail=0)[0:2]
                             + (L,))
    # the last base is L - 1 = 4294967294: records on it and ending on it
    rows = [(7, 7 + 1_234_567_890 - 1, 0, IN, 0, 0), (100_000_000, 1_099_999_999, 0, DU, 0, 0), (L - 11, L - 2, 0, IV, 0, 0),
            (L - 1, L - 1, 0, DE, 0, 0)]
    c["records_at_the_last_base"] = (np.array(rows, dtype=RECORD_DTYPE), 1_234_567_890, L)
    rows = [(0, L - 2, 0, DE, 0, 0), (L - 1, L - 1 + 0, 0, SN, 0, 0)]
    c["one_aligned_base_at_the_end"] = (np.array(rows, dtype=RECORD_DTYPE), 0, L)
    rows = [(L - 1, L - 1, 0, DU, 0, 0)]
    c["DU_of_the_last_base"] = (np.array(rows, dtype=RECORD_DTYPE), 0, L)
    return c


def counted(n_struct, snp_every=0, merge_from=None, merge_len=0, seed=1):
    """``n_struct`` structural records of all six types in random order, 1-3 untouched bases between neighbours, ``snp_every``
    > 0: that many SNPs in front of every structural record (so that the structural ones are spread over many tiles of the
    table).  ``merge_from`` / ``merge_len``: structural records merge_from .. merge_from + merge_len - 1 are deletions back to
    back -- one chain line however many tiles of gaps they cover."""
    rs = np.random.RandomState(seed)
    types = rs.choice([IN, DE, DU, IV, TL, TLI], size=n_struct)
    spans = rs.randint(1, 12, n_struct)
    gaps = rs.randint(1, 4, n_struct)
    items = []
    for k in range(n_struct):
        in_run = merge_from is not None and merge_from <= k < merge_from + merge_len
        for _ in range(0 if in_run and k > merge_from else snp_every):
            items.append((SN, 1, 0))
        if in_run:
            items.append((DE, int(spans[k]), 0 if k > merge_from else 2))
        else:
            items.append((int(types[k]), int(spans[k]), int(gaps[k])))
    return layout(items, tail=5, linked=(0, None))
