"""Python restatement of the compare mode (``msim_cmp_counts``; include/msim.h), written from its rules -- test infrastructure
shared by the CPU and the GPU tier.  The device kernels and the library's sequential restatement (``msim_dbg_cmp_counts``) must
agree with it exactly.  Two parts:

* a brute-force ORACLE that knows no shifting at all: on a contig of A/C/G/T shorter than one window two same-type, same-length
  indels are one variant iff ``apply_ref.apply`` of each record alone gives the same bytes (``brute_same``);
* a STEPWISE twin of the rules: the one-base moves (``step_left`` / ``step_right``: each returns the moved placement, with an insert's
  rotated bytes), the walk with its stop rules (``interval``), the class of a record (``class_of``: type, length, interval, an
  insert's bytes as they stand at the interval's start) and the one-to-one matching -- inside one class the i-th record of the
  truth by position matches the i-th of the calls (``compare``).  Where the kernel scans and binary-searches, this groups by key.

Stop rules, in the order a step checks them: the contig's end; the genome byte the step brings in (g[p-1] to the left, g[q+1] /
g[p] to the right) outside A, C, G, T (STOP_BASE); the comparison; the window of the record's own pos, ``pos >> 16`` (STOP_WINDOW).

The shapes at the end are the smallest at which the kernels can still go wrong; both tiers run them.
"""
from __future__ import annotations

import numpy as np

import apply_ref
from mutation_simulator_amd._ffi import RECORD_DTYPE

SN, IN, DE, DU, IV, TL, TLI = 1, 2, 3, 4, 5, 6, 7
BINS = 5
WINDOW_SHIFT = 16
STOP_WINDOW, STOP_BASE = 1, 2
ACGT = frozenset(b"ACGT")
NO_POOL = np.zeros(0, dtype=np.uint8)


def as_bases(text) -> np.ndarray:
    if isinstance(text, np.ndarray):
        return text.astype(np.uint8)
    return np.frombuffer(text.encode() if isinstance(text, str) else bytes(text), dtype=np.uint8).copy()


def length_bin(n: int) -> int:
    return 0 if n <= 1 else 1 if n <= 5 else 2 if n <= 20 else 3 if n <= 50 else 4


def insert_of(rec, pool) -> bytes:
    n = int(rec["stop"]) - int(rec["pos"]) + 1
    return bytes(pool[int(rec["extra"]):int(rec["extra"]) + n])


# ---- the oracle: no shifting code --------------------------------------------------------------------------------------------
def one_record(typ: int, pos: int, n: int, ins: bytes = b""):
    rec = np.zeros(1, dtype=RECORD_DTYPE)
    rec["pos"], rec["stop"], rec["type"] = pos, pos + n - 1, typ
    return rec, np.frombuffer(ins, dtype=np.uint8)


def brute_same(bases, typ: int, n: int, pos_a: int, ins_a: bytes, pos_b: int, ins_b: bytes) -> bool:
    ra, pa = one_record(typ, pos_a, n, ins_a)
    rb, pb = one_record(typ, pos_b, n, ins_b)
    return apply_ref.apply(bases, ra, pa).seq.tobytes() == apply_ref.apply(bases, rb, pb).seq.tobytes()


# ---- the stepwise twin ---------------------------------------------------------------------------------------------------------
# a placement: (type, p, n, S) -- a deletion of g[p .. p + n - 1] (S = b"") or an insertion of S in front of base p
def step_left(g, L, typ, p, n, S):
    """(why not, or None; the placement one base to the left)."""
    if p == 0:
        return "end", None
    if int(g[p - 1]) not in ACGT:
        return "base", None
    if typ == DE:
        if g[p - 1] != g[p + n - 1]:
            return "differs", None
        return None, (typ, p - 1, n, S)
    if g[p - 1] != S[n - 1]:
        return "differs", None
    return None, (typ, p - 1, n, S[n - 1:] + S[:n - 1])


def step_right(g, L, typ, p, n, S):
    if typ == DE:
        q = p + n - 1
        if q + 1 >= L:
            return "end", None
        if int(g[q + 1]) not in ACGT:
            return "base", None
        if g[q + 1] != g[p]:
            return "differs", None
        return None, (typ, p + 1, n, S)
    if p + 1 > L - 1:
        return "end", None
    if int(g[p]) not in ACGT:
        return "base", None
    if g[p] != S[0]:
        return "differs", None
    return None, (typ, p + 1, n, S[1:] + bytes([int(g[p])]))


def placements(bases, typ: int, pos: int, n: int, S: bytes = b"", exact: bool = False):
    """Every placement of the indel inside the window of ``pos``, by position, and the stop flags of its two walks."""
    g, L = bases, len(bases)
    here = (typ, pos, n, S)
    out, stops = {pos: here}, 0
    if exact:
        return out, stops
    for step in (step_left, step_right):
        at = here
        while True:
            why, nxt = step(g, L, *at)
            if why == "base":
                stops |= STOP_BASE
            if why is None and (nxt[1] >> WINDOW_SHIFT) != (pos >> WINDOW_SHIFT):
                stops |= STOP_WINDOW
                why = "window"
            if why is not None:
                break
            at = nxt
            out[at[1]] = at
    return out, stops


def fields(recs):
    """The table as plain tuples (pos, stop, extra, type, aux): a structured array is slow to read record by record."""
    return list(zip(recs["pos"].tolist(), recs["stop"].tolist(), recs["extra"].tolist(), recs["type"].tolist(), recs["aux"].tolist()))


def class_of(bases, rec, pool, exact: bool = False):
    """(the class of the record (pos, stop, extra, type, aux), the stop flags of its walks).  For an indel the class is its
    type, length, interval [lo, hi] and the insert's bytes as they stand at lo."""
    pos, stop, extra, typ, aux = rec
    if typ == SN:
        return (typ, pos, aux), 0
    if typ in (DU, IV, TL):
        return (typ, pos, stop, aux), 0
    if typ == TLI:
        return (typ, pos, stop, aux, extra), 0
    n = stop - pos + 1
    pl, stops = placements(bases, typ, pos, n, bytes(pool[extra:extra + n]) if typ == IN else b"", exact)
    lo, hi = min(pl), max(pl)
    return (typ, n, lo, hi, pl[lo][3]), stops


def interval(bases, rec, pool, exact: bool = False):
    """(lo, hi, stop flags) of one record of a table; lo = hi = pos for everything but IN and DE."""
    key, stops = class_of(bases, fields(np.atleast_1d(rec))[0], pool, exact)
    return (key[2], key[3], stops) if key[0] in (IN, DE) else (key[1], key[1], 0)


def compare(bases, truth, truth_pool, calls, calls_pool, exact: bool = False):
    """(counts uint64[8, BINS, 4], tallies uint64[2], truth flags uint8, calls flags uint8)."""
    bases = as_bases(bases)
    counts = np.zeros((8, BINS, 4), dtype=np.uint64)
    tallies = np.zeros(2, dtype=np.uint64)
    fa, fb = np.zeros(len(truth), dtype=np.uint8), np.zeros(len(calls), dtype=np.uint8)
    classes: dict = {}
    for i, rec in enumerate(fields(truth)):
        key, stops = class_of(bases, rec, truth_pool, exact)
        classes.setdefault(key, ([], []))[0].append(i)
        tallies[0] += 1 if stops & STOP_WINDOW else 0
        tallies[1] += 1 if stops & STOP_BASE else 0
    for j, rec in enumerate(fields(calls)):
        classes.setdefault(class_of(bases, rec, calls_pool, exact)[0], ([], []))[1].append(j)
    for ia, ib in classes.values():                        # (both in table order: by position)
        for i, j in zip(ia, ib):
            fa[i] = fb[j] = 1
    for recs, flags, col in ((truth, fa, 0), (calls, fb, 2)):
        n = recs["stop"].astype(np.int64) - recs["pos"].astype(np.int64) + 1
        typ = recs["type"].astype(np.int64)
        bins = np.where((typ == IN) | (typ == DE), np.digitize(n, [2, 6, 21, 51]), 0)
        np.add.at(counts, (typ, bins, col + (flags == 0)), 1)
    return counts, tallies, fa, fb


def unmatched(truth, fa, calls, fb):
    """The rows of ``--list``: (FN | FP, 0-based pos, type, length) of every unmatched record, truth first."""
    rows = [("FN", int(r["pos"]), int(r["type"]), int(r["stop"]) - int(r["pos"]) + 1) for r, f in zip(truth, fa) if not f]
    rows += [("FP", int(r["pos"]), int(r["type"]), int(r["stop"]) - int(r["pos"]) + 1) for r, f in zip(calls, fb) if not f]
    return rows


# ---- building tables -------------------------------------------------------------------------------------------------------------
class Table:
    """A record table under construction: rows in any order, ``build()`` sorts them and lays the pool out."""

    def __init__(self):
        self.rows = []

    def sn(self, pos, aux=0):
        self.rows.append((pos, pos, b"", SN, aux, None))
        return self

    def de(self, pos, n=1):
        self.rows.append((pos, pos + n - 1, b"", DE, 0, None))
        return self

    def ins(self, pos, S):
        S = S.encode() if isinstance(S, str) else bytes(S)
        self.rows.append((pos, pos + len(S) - 1, S, IN, 0, None))
        return self

    def raw(self, pos, stop, typ, aux=0, extra=0):
        self.rows.append((pos, stop, b"", typ, aux, extra))
        return self

    def place(self, placement):
        typ, p, n, S = placement
        return self.ins(p, S) if typ == IN else self.de(p, n)

    def build(self):
        rows = sorted(self.rows, key=lambda r: r[0])
        recs = np.zeros(len(rows), dtype=RECORD_DTYPE)
        pool = bytearray()
        for k, (pos, stop, S, typ, aux, extra) in enumerate(rows):
            recs[k] = (pos, stop, len(pool) if typ == IN else (extra or 0), typ, aux, 0)
            pool += S
        return recs, np.frombuffer(bytes(pool), dtype=np.uint8).copy()


def consumed_to(typ: int, pos: int, stop: int) -> int:
    """The last input base a record consumes (SN / IN / TLI their own, the others pos..stop): the next record starts behind it."""
    return pos if typ in (SN, IN, TLI) else stop


def shifted(bases, recs, pool, choose, keep=None, gap: int = 0):
    """A copy of the table with every IN / DE moved to another placement of its interval: ``choose(candidates)`` picks among
    the positions that leave the table one the library takes -- behind what the (moved) predecessor consumed, in front of the
    successor's original pos, with ``gap`` untouched bases on either side (1: the anchor base of a VCF line stays free; where
    the record's own pos does not leave that much, it stays).  ``keep`` (bool per record): the records to copy at all.
    Returns a ``Table``."""
    bases = as_bases(bases)
    out, free = Table(), 0
    for k in range(len(recs)):
        r = recs[k]
        typ, pos, stop = int(r["type"]), int(r["pos"]), int(r["stop"])
        if keep is not None and not keep[k]:               # (left out, but nothing moves onto it: it may come back changed)
            free = consumed_to(typ, pos, stop) + 1
            continue
        if typ not in (IN, DE):
            out.raw(pos, stop, typ, int(r["aux"]), int(r["extra"]))
            free = consumed_to(typ, pos, stop) + 1
            continue
        n = stop - pos + 1
        limit = int(recs[k + 1]["pos"]) if k + 1 < len(recs) else len(bases)
        pl, _ = placements(bases, typ, pos, n, insert_of(r, pool) if typ == IN else b"")
        ok = sorted(p for p in pl if p >= free + gap and consumed_to(typ, p, p + n - 1) + gap < limit) or [pos]
        at = pl[choose(ok)]
        out.place(at)
        free = consumed_to(typ, at[1], at[1] + n - 1) + 1
    return out


def case(bases, truth: Table, calls: Table, exact=False):
    a, pa = truth.build()
    b, pb = calls.build()
    return as_bases(bases), a, pa, b, pb, exact


# ---- shared shapes: {case id: (bases, truth, truth pool, calls, calls pool, exact)} -------------------------------------------
RANDOM_200 = "GATTACAGGCTTAACCGTTGACCATGCATGGCAATCGGATCCTTAGCAAGT" * 4


def basic_cases():
    g = RANDOM_200
    some = lambda: Table().sn(3, 1).de(10, 2).ins(20, "GT").sn(40, 2).de(60, 7)          # noqa: E731
    other = lambda: Table().sn(5, 0).de(14, 3).ins(26, "CCA").sn(44, 1)                   # noqa: E731
    return {"identical": case(g, some(), some()), "identical_exact": case(g, some(), some(), True),
            "disjoint": case(g, some(), other()), "truth_empty": case(g, Table(), some()),
            "calls_empty": case(g, some(), Table()), "both_empty": case(g, Table(), Table()),
            "sn_aux_differs": case(g, Table().sn(9, 0).sn(12, 1), Table().sn(9, 1).sn(12, 1))}


def homopolymer_cases():
    g = "A" * 12
    return {"homopolymer_ends": case(g, Table().de(11), Table().de(0)),
            "homopolymer_ends_exact": case(g, Table().de(11), Table().de(0), True),
            "homopolymer_lengths": case(g, Table().de(9, 2), Table().de(0, 3)),
            "homopolymer_ins": case(g, Table().ins(11, "AA"), Table().ins(0, "AA")),
            "homopolymer_ins_other_base": case(g, Table().ins(11, "A"), Table().ins(0, "C"))}


def repeat_cases():
    g, h = "AC" * 8, "ACG" * 6
    return {"repeat_rotated": case(g, Table().ins(2, "AC"), Table().ins(3, "CA")),
            "repeat_rotated_exact": case(g, Table().ins(2, "AC"), Table().ins(3, "CA"), True),
            "repeat_other_bytes": case(g, Table().ins(2, "AC"), Table().ins(3, "CC")),
            "repeat_same_pos_other_bytes": case(g, Table().ins(2, "AC"), Table().ins(2, "AG")),
            "repeat_negative_shift": case(g, Table().ins(9, "CA"), Table().ins(4, "AC")),
            "repeat3_shift_2": case(h, Table().ins(3, "ACG"), Table().ins(5, "GAC")),
            "repeat3_shift_4": case(h, Table().ins(3, "ACG"), Table().ins(7, "CGA")),
            "repeat3_shift_minus_5": case(h, Table().ins(9, "ACG"), Table().ins(4, "CGA")),
            "repeat3_wrong_rotation": case(h, Table().ins(3, "ACG"), Table().ins(5, "CGA")),
            "repeat_de_2": case(g, Table().de(10, 2), Table().de(1, 2)),
            "repeat_de_2_vs_3": case(g, Table().de(10, 2), Table().de(1, 3))}


def walk_end_cases():
    out = {"end_pos0": case("AAAC", Table().de(2), Table().de(0)),
           "end_last_base": case("CAAA", Table().de(1), Table().de(3)),
           "end_last_base_2": case("CAAAA", Table().de(1, 2), Table().de(3, 2)),
           "end_ins_last_base": case("CAAA", Table().ins(1, "A"), Table().ins(3, "A")),
           "end_ins_pos0": case("AAAC", Table().ins(2, "A"), Table().ins(0, "A")),
           "stop_N": case("AAAANAAAA", Table().de(1), Table().de(6)),
           "stop_N_ins": case("AAAANAAAA", Table().ins(1, "A"), Table().ins(6, "A")),
           "stop_N_run": case("CNNNNC", Table().de(1, 2), Table().de(3, 2)),
           "stop_iupac": case("AAAARAAAA", Table().de(6), Table().de(1))}
    edge = "A" * ((1 << WINDOW_SHIFT) + 40)
    w = 1 << WINDOW_SHIFT
    out["window_edge"] = case(edge, Table().de(w - 6), Table().de(w + 4))
    out["window_edge_ins"] = case(edge, Table().ins(w + 9, "AA"), Table().ins(w - 1, "AA"))
    out["window_same_side"] = case(edge, Table().de(w + 30), Table().de(w))
    out["window_last_of_first"] = case(edge, Table().de(w - 1), Table().de(7))
    return out


def rank_block(offset, n_truth, n_calls, gap=13):
    """n_truth against n_calls one-base deletions in one class: a run of A's at ``offset`` wide enough for all of them, every
    second base (records consume disjoint input), truth and calls interleaved from opposite ends."""
    truth = [offset + 1 + 2 * k for k in range(n_truth)]
    calls = [offset + gap - 1 - 2 * k for k in range(n_calls)]
    return truth, calls


def rank_cases(PASS: int):
    out = {}
    run = "C" + "A" * 13 + "G"
    for n_truth, n_calls in ((2, 1), (1, 2), (3, 2)):
        tag = f"{n_truth}v{n_calls}"
        tp, cp = rank_block(0, n_truth, n_calls)
        t, c = Table(), Table()
        for p in tp:
            t.de(p)
        for p in cp:
            c.de(p)
        out[f"rank_{tag}"] = case(run, t, c)
        # the same class behind PASS - 1 filler SNs, in the truth (its records at indices PASS - 1, PASS, PASS + 1) or the calls
        filler = "CG" * (PASS - 1)
        g = filler + run
        tp, cp = rank_block(len(filler), 3, 2) if tag == "3v2" else rank_block(len(filler), n_truth, n_calls)
        for side in ("truth", "calls"):
            t, c = Table(), Table()
            for k in range(PASS - 1):
                (t if side == "truth" else c).sn(2 * k, k % 3)
            for p in (tp if side == "truth" else cp):
                t.de(p) if side == "truth" else c.de(p)
            for p in (cp if side == "truth" else tp):
                c.de(p) if side == "truth" else t.de(p)
            out[f"rank_{tag}_{side}_at_pass"] = case(g, t, c)
    # one insert class, three against two, rotation and rank together
    g = "T" + "AC" * 10 + "T"
    out["rank_ins_3v2"] = case(g, Table().ins(1, "AC").ins(4, "CA").ins(9, "AC"), Table().ins(6, "CA").ins(15, "AC"))
    return out


def type_cases():
    g = RANDOM_200
    every = lambda: (Table().sn(5, 1).ins(10, "GT").de(20, 3).raw(30, 33, DU).raw(40, 44, IV).raw(50, 54, TL)     # noqa: E731
                     .raw(60, 54, TLI, aux=1, extra=50))
    out = {"every_type": case(g, every(), every())}
    changed = (Table().sn(5, 1).ins(10, "GT").de(20, 3).raw(30, 34, DU).raw(40, 44, IV, aux=0).raw(50, 54, TL)
               .raw(60, 54, TLI, aux=1, extra=51))
    out["every_type_changed"] = case(g, every(), changed)
    out["type_differs"] = case(g, Table().raw(30, 33, DU).de(40, 2), Table().raw(30, 33, IV).raw(40, 41, TL))
    g = (RANDOM_200 * 3)
    lengths = (1, 2, 5, 6, 20, 21, 50, 51)
    t, c = Table(), Table()
    at = 1
    for k, n in enumerate(lengths):
        t.de(at, n)
        if k % 2 == 0:
            c.de(at, n)
        at += n + 3
        S = bytes(b"ACGT"[(k + i * i) & 3] for i in range(n))
        t.ins(at, S)
        if k % 2 == 1:
            c.ins(at, S)
        at += 3
    assert at < len(g)
    out["bin_edges"] = case(g, t, c)
    return out


def random_tables(seed: int, L: int = 200, letters: bytes = b"AC", n: int = 24):
    """Two random tables of SNs and short indels on a low-complexity contig: shifts are the rule."""
    rs = np.random.RandomState(seed)
    g = np.frombuffer(letters, dtype=np.uint8)[rs.randint(0, len(letters), L)].copy()
    tables = []
    for _ in range(2):
        t, at = Table(), int(rs.randint(0, 4))
        while at < L - 8 and len(t.rows) < n:
            kind = int(rs.randint(0, 3))
            k = int(rs.randint(1, 4))
            if kind == 0:
                t.sn(at, int(rs.randint(0, 3)))
                at += 1
            elif kind == 1:
                t.de(at, k)
                at += k
            else:
                t.ins(at, bytes(letters[int(x)] for x in rs.randint(0, len(letters), k)))
                at += 2                                    # (a record may not start directly behind an insertion's anchor)
            at += int(rs.randint(0, 6))
        tables.append(t)
    return case(g, tables[0], tables[1])


def random_shifted(seed: int, letters: bytes = b"AC", exact: bool = False):
    """A random table against itself with every indel at a random placement of its interval and a quarter of the records left out."""
    g, a, pa, _, _, _ = random_tables(seed, letters=letters)
    rs = np.random.RandomState(seed + 7)
    calls = shifted(g, a, pa, lambda ok: ok[int(rs.randint(0, len(ok)))], keep=rs.randint(0, 4, len(a)) > 0)
    b, pb = calls.build()
    return g, a, pa, b, pb, exact


def random_cases():
    out = {f"random_{seed}": random_tables(seed) for seed in range(8)}
    out.update({f"random_shifted_{seed}": random_shifted(seed) for seed in range(20, 28)})
    out["random_shifted_exact"] = random_shifted(20, exact=True)
    out["random_shifted_one_letter"] = random_shifted(30, letters=b"A")
    out["random_shifted_with_N"] = random_shifted(31, letters=b"AAACCN")
    out["random_with_N"] = random_tables(100, letters=b"AAACCN")
    out["random_one_letter"] = random_tables(101, letters=b"A")
    return out


def small_cases(PASS: int):
    out = {}
    for part in (basic_cases(), homopolymer_cases(), repeat_cases(), walk_end_cases(), rank_cases(PASS), type_cases(), random_cases()):
        out.update(part)
    return out
