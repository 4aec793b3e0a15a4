"""A plain restatement of ``vcf --consensus``: apply one haplotype of one sample of any VCF, by string slicing.

Written from the mode's statement, not from the parsers.  For every data line, in file order: the selected sample's genotype
names one of the ALTs (``.`` / ``0`` / a ``*`` allele: the line is skipped unread); REF and that ALT are upper-cased, REF must
match the genome (each byte as the genome has it, or de-ambiguated), ALT must be letters; one base they share -- their first
bytes, unless that would leave an insertion behind the contig's last base, else their last bytes -- stays as the genome has
it, and what is left of REF is replaced by what is left of ALT.  A line must start behind everything an earlier line used, where
an insertion uses the base it stands in front of.  Nothing here knows records, pools or kernels.

``consensus`` returns the mutated sequences, or ``(line number, reason code)`` of the first offending line: the smallest
line number, and on that line the smallest code.
"""
from __future__ import annotations

import re

FIELDS, POS, SAMPLE, ALLELE, REF, INSERT, ORDER, LENGTH, END = 1, 3, 4, 6, 8, 10, 11, 12, 13
REASON_TEXT = {
    FIELDS: "neither 8 nor 10 or more tab-separated fields, or not as many as the first data line",
    POS: "POS is no number, 0, or beyond the contig",
    SAMPLE: "FORMAT does not start with GT, or a genotype entry that is neither a number nor .",
    ALLELE: "allele index beyond the ALTs, symbolic allele, breakend, or multi-allelic ALT longer than 4096 bytes",
    REF: "REF does not match the genome",
    INSERT: "ALT byte that is no letter",
    ORDER: "not behind the input an earlier line consumed (positions increasing, no overlap)",
    LENGTH: "mutated length of 2^32 or more",
    END: "replacement or insertion that reaches behind the contig's last base",
}
MULTI_ALLELIC_CAP = 4096
NON_AMBIGUOUS = dict(zip(b"KSYMWRBDHV-", b"GCCAAACAAAN"))      # mutator.py:75


def conv(g: int) -> int:
    return NON_AMBIGUOUS.get(g, g)


def message(line: int, reason: int) -> str:
    return f"VCF line {line}: {REASON_TEXT[reason]}"


def sample_index(vcf: bytes, sample) -> int:
    """0-based sample column of ``sample`` (None: the first) by the last ``#CHROM`` line in front of the first data line."""
    names = None
    for line in vcf.split(b"\n"):
        if not (len(line) > 0 and line.startswith(b"#")):
            break
        if line.startswith(b"#CHROM"):
            names = line.split(b"\t")[9:]
    if sample is None:
        return 0
    return names.index(sample.encode())


def _is_letters(s: bytes) -> bool:
    return all(65 <= c <= 90 or 97 <= c <= 122 for c in s)


def _line(seq: bytes, free: int, f, nf0: int, s_idx: int, hap: int):
    """One data line against the contig ``seq`` with everything in front of ``free`` used: None (skipped / no change),
    an int (the reason it is refused for), or (at, deleted, inserted, next free)."""
    L = len(seq)
    if len(f) != nf0 or not (nf0 == 8 or nf0 >= 10):
        return FIELDS
    pos_ok = f[1].isdigit() and len(f[1]) <= 10 and 1 <= int(f[1]) <= L
    k = 1
    if nf0 >= 10:
        bad_gt = not (f[8] == b"GT" or f[8].startswith(b"GT:"))
        if not bad_gt:
            entries = re.split(rb"[/|]", f[9 + s_idx].split(b":")[0])
            want = 1 if len(entries) == 1 else hap
            entry = entries[want - 1] if want <= len(entries) else b""
            if entry == b".":
                k = 0
            elif entry.isdigit() and len(entry) <= 9:
                k = int(entry)
            else:
                bad_gt = True
        if bad_gt:
            return SAMPLE if pos_ok else POS
    if k == 0:
        return None
    if not pos_ok:
        return POS
    ref, alt_field = f[3], f[4]
    if len(alt_field) <= MULTI_ALLELIC_CAP:
        alts = alt_field.split(b",")
        if k > len(alts):
            return ALLELE
        alt = alts[k - 1]
    else:
        if b"," in alt_field or k != 1:
            return ALLELE
        alt = alt_field
    if alt == b"":
        return ALLELE
    if alt == b"*":
        return None
    reasons = []
    if any(c in b"<>[]" for c in alt):
        reasons.append(ALLELE)
    if not _is_letters(alt):
        reasons.append(INSERT)
    ref, alt = ref.upper(), alt.upper()
    a, R, A = int(f[1]) - 1, len(ref), len(alt)
    if R == 0 or a + R > L:
        reasons.append(REF)
        return min(reasons)
    if any(c != g and c != conv(g) for c, g in zip(ref, seq[a:a + R])):
        reasons.append(REF)
    if R == 1 and A == 1:
        # The mode's statement treats one changed base in two ways, and the difference is visible from outside: where ALT is a
        # transition or transversion of the (de-ambiguated) base the line uses base a alone; otherwise it is "delete [a, a] and
        # insert ALT", and an insertion uses the base it stands in front of -- so the next line may start at a + 2 at the
        # earliest, and on a contig's last base there is nothing to stand in front of (END).  The bytes written are the same.
        g, c = seq[a], conv(seq[a])
        if alt[0] == g:
            return min(reasons) if reasons else None
        at, dele, ins = a, seq[a:a + 1], alt
        if c in b"ACGT" and alt[0] in b"ACGT" and alt[0] != c:    # a transition or transversion of the base: one byte changes
            if a < free:
                reasons.append(ORDER)
            return min(reasons) if reasons else (a, dele, ins, a + 1)
    elif ref[0] == alt[0] and not (A > 1 and a + R == L):
        at, dele, ins = a + 1, ref[1:], alt[1:]
    elif ref[-1] == alt[-1]:
        at, dele, ins = a, ref[:-1], alt[:-1]
    else:
        at, dele, ins = a, ref, alt
    if ins and at + len(dele) == L:
        reasons.append(END)                                       # (no record form: the order rule is not asked)
    elif at < free:
        reasons.append(ORDER)
    if reasons:
        return min(reasons)
    return at, dele, ins, at + len(dele) + (1 if ins else 0)


def consensus(contigs, vcf: bytes, sample=None, haplotype: int = 1):
    """``contigs``: [(name, upper-cased bases)].  The mutated bases per contig, or (line, reason)."""
    s_idx = sample_index(vcf, sample)
    by_name = {name.encode(): i for i, (name, _) in enumerate(contigs)}
    out = [[] for _ in contigs]
    cur = [0] * len(contigs)                  # next input base not yet written
    free = [0] * len(contigs)
    lines = vcf.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    nf0, in_header = None, True
    for number, line in enumerate(lines, 1):
        if in_header and len(line) > 0 and line.startswith(b"#"):
            continue
        in_header = False
        f = line.split(b"\t")
        if nf0 is None:
            nf0 = len(f)
        i = by_name[f[0]]
        seq = contigs[i][1]
        got = _line(seq, free[i], f, nf0, s_idx, haplotype)
        if got is None:
            continue
        if isinstance(got, int):
            return number, got
        at, dele, ins, nxt = got
        out[i].append(seq[cur[i]:at])
        out[i].append(ins)
        cur[i] = at + len(dele)
        free[i] = nxt
    return [b"".join(o) + contigs[i][1][cur[i]:] for i, o in enumerate(out)]


def frame(seq: bytes, bpl: int) -> bytes:
    """Body text as FastaWriter leaves it: a newline after every ``bpl`` bases, none after a partial last line."""
    return b"\n".join(seq[i:i + bpl] for i in range(0, len(seq), bpl)) + (b"\n" if seq and len(seq) % bpl == 0 else b"")


def consensus_fasta(records, vcf: bytes, sample=None, haplotype: int = 1):
    """``records``: [(defline without '>', upper-cased bases, bases per line)] (``vcf_replay_ref.read_fasta``).  The whole mutated
    Fasta file, or (line, reason)."""
    got = consensus([(head.split()[0] if head.split() else "", seq) for head, seq, _ in records], vcf, sample, haplotype)
    if isinstance(got, tuple):
        return got
    out, partial = [], False
    for (head, _, bpl), seq in zip(records, got):
        out.append((b"\n" if partial else b"") + b">" + head.encode() + b"\n" + frame(seq, bpl))
        partial = bool(seq) and len(seq) % bpl != 0
    return b"".join(out)
