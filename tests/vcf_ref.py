"""A plain restatement of the reference's VCF record lines: what ``Mutator.__mutate_sequence`` (mutator.py:334-421) puts into a
``VcfRecord`` for every mutation type and how ``VcfWriter.write`` (vcf_writer.py:44-52,118-126) prints it, over a FINISHED
record table -- the SNP outcome and the insert's bases come with the records (``aux`` / the insert pool), as in
``tests/apply_ref.py``, whose translation tables (the reference's own strings) are used here.

Written from the reference's lines with Python's own slices (which clamp at the sequence's end exactly as the reference's do),
not from ``render.cpp`` or the kernels.  Nothing here knows about stages, gaps, units or lanes.
``tests/test_vcf_ref_host.py`` holds it against bytes the real reference produced.

Record fields (include/msim.h): pos = Mutation.start, stop = Mutation.stop (IN: pos + insert length - 1), extra = insert pool
offset (IN) / Mutation.start of a TLI (the linked TL span's start; its stop is that span's stop; an unlinked TLI keeps
start = pos, stop = 0), aux = SNP outcome (0 transition, 1 / 2 the transversion dict's column) / TLI bit 0 = trans_reverse,
bit 1 = trans_insert_pos > 0.  ``gt``: one genotype byte per record (bit 0: on haplotype 1, bit 1: on haplotype 2), the sample
column becomes ``a|b`` as ``msim_render_vcf_gt`` words it; None: the reference's haploid ``1``.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from apply_ref import COMPLEMENT, DE, DU, IN, IV, NON_AMBIGUOUS, SN, TL, TLI, TRANSITIONS, TRANSVERSIONS

CONV = NON_AMBIGUOUS.tobytes()          # str.translate tables as bytes.translate tables
COMP = COMPLEMENT.tobytes()
TRANS = TRANSITIONS.tobytes()

RAW, CONVERTED, REVCOMP = "raw", "converted", "reverse-complemented"
# the REF / ALT copies of a line: kind -> how its bytes follow from the source
COPY_MODE = {"IN": RAW, "DE_REF": CONVERTED, "TL_REF": CONVERTED, "IV_REF": CONVERTED, "IV_ALT": REVCOMP,
             "DU_REF": RAW, "DU_ALT1": RAW, "DU_ALT2": RAW, "TLI_FWD": CONVERTED, "TLI_REV": REVCOMP}

Copy = namedtuple("Copy", "record kind length offset source")


def _name(name) -> bytes:
    return name if isinstance(name, bytes) else name.encode("utf-8", "replace")


def _record(seq: bytes, ins: bytes, p: int, stop: int, extra: int, typ: int, aux: int):
    """(svtype, start, end, len, ref, alt) of one mutation -- the reference's VcfRecord."""
    if typ == SN:                                                         # mutator.py:334-341
        ref = seq[p:p + 1].translate(CONV)
        alt = ref.translate(TRANS) if aux == 0 else TRANSVERSIONS[ref.decode()][aux - 1].encode()
        return "sn", p + 1, 0, 0, ref, alt
    if typ == IN:                                                         # :343-358
        insert = ins[extra:extra + stop + 1 - p]
        if p > 0:
            ref = seq[p - 1:p].translate(CONV)
            return "INS", p, p, len(insert), ref, ref + insert
        ref = seq[0:1].translate(CONV)
        return "INS", p + 1, p + 1, len(insert), ref, insert + ref
    if typ in (DE, TL):                                                   # :360-377
        svtype = "DEL" if typ == DE else "DEL:ME"
        start, end = p, stop + 1
        if p > 0:
            ref = seq[p - 1:end].translate(CONV)
            alt = ref[0:1]
        else:
            start, end = start + 1, end + 1
            ref = seq[0:end].translate(CONV)
            alt = ref[-1:]
        return svtype, start, end, stop - p + 1, ref, alt
    if typ == IV:                                                         # :379-387
        end = stop + 1
        ref = seq[p:end].translate(CONV)
        return "INV", p + 1, end, 0, ref, ref[::-1].translate(COMP)
    if typ == DU:                                                         # :389-399 (REF is not converted)
        dupe = seq[p:stop + 1]
        return "DUP", p + 1, p + len(dupe), len(dupe), dupe, dupe * 2
    if typ == TLI:                                                        # :401-421
        insert = seq[extra:stop + 1].translate(CONV)
        if aux & 1:
            insert = insert[::-1].translate(COMP)
        start = p
        if aux & 2:                                                       # trans_insert_pos > 0
            ref = seq[p - 1:p].translate(CONV)
            alt = ref + insert
        else:
            start += 1
            ref = seq[p:p + 1].translate(CONV)
            alt = insert + ref
        return "INS:ME", start, start, len(insert), ref, alt
    raise AssertionError(f"type {typ}")


def _fields(bases, recs, pool):
    seq = np.asarray(bases, dtype=np.uint8).tobytes()
    ins = np.asarray(pool, dtype=np.uint8).tobytes()
    cols = zip(recs["pos"].tolist(), recs["stop"].tolist(), recs["extra"].tolist(), recs["type"].tolist(), recs["aux"].tolist())
    return seq, ins, cols


def lines(bases, recs, pool, name, gt=None) -> list:
    """One entry per record: its VCF line, ``b""`` where the writer suppresses it (REF == ALT, vcf_writer.py:123)."""
    name = _name(name)
    seq, ins, cols = _fields(bases, recs, pool)
    out = []
    for i, (p, stop, extra, typ, aux) in enumerate(cols):
        svtype, start, end, length, ref, alt = _record(seq, ins, p, stop, extra, typ, aux)
        if ref == alt:
            out.append(b"")
            continue
        info = b"." if svtype == "sn" else b"SVTYPE=%s;END=%d;SVLEN=%d" % (svtype.encode(), end, length)     # vcf_writer.py:44-52
        g = int(gt[i]) if gt is not None else 0
        sample = b"%d|%d" % (g & 1, (g >> 1) & 1) if g else b"1"
        out.append(b"%s\t%d\t.\t%s\t%s\t.\t.\t%s\tGT\t%s\n" % (name, start, ref, alt, info, sample))         # vcf_writer.py:125
    return out


def rename(body: list, old, new) -> list:
    """The lines of ``lines(..., old)`` under another sequence name (every line starts with it)."""
    old, new = _name(old), _name(new)
    return [new + l[len(old):] if l else l for l in body]


def copies(bases, recs, pool, name, gt=None, body=None) -> list:
    """Where every REF / ALT copy of every line lands: Copy(record, kind, length, offset, source) -- ``offset``: the text
    offset of the copy's first byte in the joined text, read off the joined text's own tabs; ``source``: the index of the
    source byte that gives the copy's first byte (pool offset of an insert; for a reverse-complemented copy the LAST base of
    the span).  The single anchor bases and an SNP's REF / ALT are no copies."""
    name = _name(name)
    body = lines(bases, recs, pool, name, gt) if body is None else body
    text = b"".join(body)
    out, at = [], 0
    cols = zip(recs["pos"].tolist(), recs["stop"].tolist(), recs["extra"].tolist(), recs["type"].tolist(), recs["aux"].tolist())
    for i, (p, stop, extra, typ, aux) in enumerate(cols):
        line = body[i]
        if not line:
            continue
        t1 = text.index(b"\t", at + len(name) + 1)                        # behind POS
        ref_at = t1 + 3                                                   # "\t.\t"
        ref_end = text.index(b"\t", ref_at)
        alt_at = ref_end + 1
        alt_end = text.index(b"\t", alt_at)
        n_ref, n_alt = ref_end - ref_at, alt_end - alt_at
        if typ == IN:
            out.append(Copy(i, "IN", n_alt - 1, alt_at + (1 if p > 0 else 0), extra))
        elif typ in (DE, TL):
            out.append(Copy(i, "DE_REF" if typ == DE else "TL_REF", n_ref, ref_at, p - 1 if p > 0 else 0))
        elif typ == IV:
            out.append(Copy(i, "IV_REF", n_ref, ref_at, p))
            out.append(Copy(i, "IV_ALT", n_alt, alt_at, p + n_ref - 1))
        elif typ == DU:
            out.append(Copy(i, "DU_REF", n_ref, ref_at, p))
            out.append(Copy(i, "DU_ALT1", n_ref, alt_at, p))
            out.append(Copy(i, "DU_ALT2", n_ref, alt_at + n_ref, p))
            assert n_alt == 2 * n_ref
        elif typ == TLI:
            first = alt_at + (1 if aux & 2 else 0)
            out.append(Copy(i, "TLI_REV", n_alt - 1, first, extra + n_alt - 2) if aux & 1 else Copy(i, "TLI_FWD", n_alt - 1, first, extra))
        at += len(line)
    assert at == len(text)
    return out


def snp_text(bases, recs, name, gt=None) -> bytes:
    """``b"".join(lines(...))`` of a table of SNP records only, built with numpy (millions of records): the same rule -- REF is
    the converted base, ALT its transition or the transversion dict's column, equal ones are suppressed -- column by column.
    POS ascends, so lines of one digit count are adjacent and have one length."""
    assert np.all(recs["type"] == SN)
    name = np.frombuffer(_name(name), dtype=np.uint8)
    bases = np.asarray(bases, dtype=np.uint8)
    pos = recs["pos"].astype(np.int64)
    ref = NON_AMBIGUOUS[bases[pos]]
    tv = np.zeros((3, 256), dtype=np.uint8)
    tv[0] = TRANSITIONS
    for k, pair in TRANSVERSIONS.items():
        tv[1][ord(k)], tv[2][ord(k)] = ord(pair[0]), ord(pair[1])
    alt = tv[recs["aux"].astype(np.int64), ref]
    assert alt.all(), "a transversion on a base the dict does not know (KeyError in the reference)"
    keep = ref != alt
    start = pos + 1
    g = np.asarray(gt, dtype=np.uint8) if gt is not None else None
    out = []
    digits = np.searchsorted(np.array([10 ** k for k in range(1, 12)], dtype=np.int64), start, side="right") + 1
    for d in np.unique(digits):
        m = keep & (digits == d)
        n = int(m.sum())
        if not n:
            continue
        tail = b"\t.\tR\tA\t.\t.\t.\tGT\t" + (b"1\n" if g is None else b"a|b\n")
        w = len(name) + 1 + int(d) + len(tail)
        a = np.empty((n, w), dtype=np.uint8)
        a[:, :len(name)] = name
        a[:, len(name)] = 9
        v = start[m]
        for q in range(int(d) - 1, -1, -1):
            a[:, len(name) + 1 + q] = 48 + v % 10
            v = v // 10
        t0 = len(name) + 1 + int(d)
        a[:, t0:] = np.frombuffer(tail, dtype=np.uint8)
        a[:, t0 + 3] = ref[m]
        a[:, t0 + 5] = alt[m]
        if g is not None:
            a[:, w - 4] = 48 + (g[m] & 1)
            a[:, w - 2] = 48 + ((g[m] >> 1) & 1)
        out.append(a.tobytes())
    return b"".join(out)
