"""A plain restatement of the reference's rewrite loop, ``Mutator.__mutate_sequence`` (mutator.py:318-426), over a FINISHED
record table: what the generators decide while the reference walks (the SNP outcome, the insert's bases) comes with the
records (``aux`` / the insert pool), everything else is the reference's loop, one record after the other, on bytes.

Written from the reference's lines, not from the kernels: the three translation tables are the reference's strings
(mutator.py:75-77), the transversions its dict (mutator.py:449-455).  Nothing here knows about tiles, groups, windows or the
library's LUT.  ``tests/test_apply_ref_host.py`` holds it against bytes the real reference produced.

Record fields (include/msim.h): pos = Mutation.start, stop = Mutation.stop (IN: pos + insert length - 1), extra = insert
pool offset (IN) / start of the linked TL span (TLI, whose stop is that span's stop), aux = SNP outcome (0 transition,
1 / 2 the transversion dict's column) / TLI bit 0 = trans_reverse.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

SN, IN, DE, DU, IV, TL, TLI = 1, 2, 3, 4, 5, 6, 7


def _table(src: str, dst: str) -> np.ndarray:
    t = np.arange(256, dtype=np.uint8)
    for a, b in zip(src, dst):
        t[ord(a)] = ord(b)
    return t


NON_AMBIGUOUS = _table("KSYMWRBDHV-", "GCCAAACAAAN")          # mutator.py:75
COMPLEMENT = _table("ACGTUMRWSYKVHDB", "TGCAAKYWSRMBDHV")     # mutator.py:76
TRANSITIONS = _table("AGTC", "GACT")                          # mutator.py:77
TRANSVERSIONS = {"A": "TC", "G": "CT", "T": "GA", "C": "AG", "N": "NN"}   # mutator.py:449-455

Result = namedtuple("Result", "seq offsets out_len key_error")


def apply(bases: np.ndarray, recs: np.ndarray, pool: np.ndarray) -> Result:
    """The mutated sequence, every record's output offset (where its first output byte lands; for a record that writes
    nothing, where the next byte lands), the mutated length, and -- instead of a sequence -- the KeyError of the first
    transversion the walk meets on a base outside AGTCN as (base, position)."""
    bases = np.asarray(bases, dtype=np.uint8)
    pool = np.asarray(pool, dtype=np.uint8)
    one = [np.array([b], dtype=np.uint8) for b in range(256)]
    out, offsets = [], np.zeros(len(recs), dtype=np.int64)
    at = 0              # the reference's `pos`: next input base to look at
    o = 0               # bytes written so far

    def write(chunk):
        nonlocal o
        if len(chunk):
            out.append(chunk)
            o += len(chunk)

    fields = zip(recs["pos"].tolist(), recs["stop"].tolist(), recs["extra"].tolist(), recs["type"].tolist(), recs["aux"].tolist())
    for i, (p, stop, extra, typ, aux) in enumerate(fields):
        assert at <= p < len(bases), f"record {i} at {p} is not visited (walk stands at {at})"
        write(bases[at:p])                                            # mutator.py:422-423
        offsets[i] = o
        if typ == SN:                                                 # :334-341
            ref = int(NON_AMBIGUOUS[bases[p]])
            if aux == 0:
                alt = int(TRANSITIONS[ref])
            else:
                pair = TRANSVERSIONS.get(chr(ref))
                if pair is None:
                    return Result(None, offsets[:i + 1], None, (chr(ref), p))
                alt = ord(pair[aux - 1])
            write(one[alt])
            at = p + 1
        elif typ == IN:                                               # :343-358
            write(pool[extra:extra + stop + 1 - p])
            write(bases[p:p + 1])
            at = p + 1
        elif typ in (DE, TL):                                         # :360-377
            at = stop + 1
        elif typ == IV:                                               # :379-387
            write(COMPLEMENT[NON_AMBIGUOUS[bases[p:stop + 1]]][::-1])
            at = stop + 1
        elif typ == DU:                                               # :389-399
            write(bases[p:stop + 1])
            write(bases[p:stop + 1])
            at = stop + 1
        elif typ == TLI:                                              # :401-421
            insert = NON_AMBIGUOUS[bases[extra:stop + 1]]
            if aux & 1:
                insert = COMPLEMENT[insert[::-1]]
            write(insert)
            write(bases[p:p + 1])
            at = p + 1
        else:
            raise AssertionError(f"record {i}: type {typ}")
    write(bases[at:])
    seq = np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)
    assert len(seq) == o
    return Result(seq, offsets, o, None)


def visited(muts):
    """The entries of a position-keyed mutation list that __mutate_sequence visits: the walk jumps to ``stop`` behind a DE, TL,
    IV or DU (mutator.py:376,386,398), so whatever starts inside such a span is never looked at."""
    keep, at = [], 0
    for name, start, stop in sorted(muts, key=lambda m: m[1]):
        if start < at:
            continue
        keep.append((name, start, stop))
        at = stop + 1 if name in ("DE", "TL", "IV", "DU") else start + 1
    return keep


def golden_table(case: dict):
    """Record table + insert pool of one ``tests/golden/apply.json`` case: its mutation list filtered by the visit rule, the
    SNP outcomes and insert bases read from the VCF body the real reference wrote (REF / ALT).  A visited mutation without a
    line is one the VCF writer suppressed because REF == ALT (an SNP on N, a palindrome's inversion): it changes no byte."""
    from mutation_simulator_amd._ffi import RECORD_DTYPE
    type_id = {"SN": SN, "IN": IN, "DE": DE, "DU": DU, "IV": IV}
    svtype = {"IN": "INS", "DE": "DEL", "DU": "DUP", "IV": "INV"}
    seq_len = len(case["sequence"])
    lines = [l.split("\t") for l in case["vcf_body"]]
    rows, pool, k = [], bytearray(), 0
    for name, start, stop in visited(case["muts"]):
        if start >= seq_len:
            continue                                                  # (the walk ends at the sequence's end)
        if name in ("DE", "DU", "IV"):
            stop = min(stop, seq_len - 1)                             # (the reference's slices end with the sequence)
        vpos = start + 1 if name in ("SN", "IV", "DU") or start == 0 else start
        kind = "." if name == "SN" else "SVTYPE=" + svtype[name] + ";"
        hit = k < len(lines) and int(lines[k][1]) == vpos and (lines[k][7] == "." if name == "SN" else lines[k][7].startswith(kind))
        aux = extra = 0
        if hit:
            ref, alt = lines[k][3], lines[k][4]
            k += 1
            if name == "SN":
                aux = 0 if alt == chr(TRANSITIONS[ord(ref)]) else 1 + TRANSVERSIONS[ref].index(alt)
            elif name == "IN":
                insert = alt[1:] if start > 0 else alt[:-1]
                assert len(insert) == stop + 1 - start
                extra = len(pool)
                pool += insert.encode()
        else:
            assert name in ("SN", "IV"), (case["name"], name, start)
        rows.append((start, stop, extra, type_id[name], aux, 0))
    assert k == len(lines), (case["name"], "VCF lines left over")
    return np.array(rows, dtype=RECORD_DTYPE), np.frombuffer(bytes(pool), dtype=np.uint8).copy()


def unwrap_fasta(text: str) -> np.ndarray:
    """The bases of a one-record Fasta text."""
    body = "".join(text.split("\n")[1:])
    return np.frombuffer(body.encode(), dtype=np.uint8).copy()
