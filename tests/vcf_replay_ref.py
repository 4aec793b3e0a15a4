"""A plain restatement of the ``vcf`` mode's semantics: replace REF at POS by ALT, line after line, with the anchor rule.

Written from the VCF's meaning, not from the parsers: every data line replaces ``REF`` at ``POS`` by ``ALT``; the one base an
``INS`` / ``INS:ME`` / ``DEL`` / ``DEL:ME`` line shares between REF and ALT -- leading when ``ALT[0] == REF`` (insertions) or
``ALT == REF[0]`` (deletions), trailing otherwise -- is left as the genome has it, because the VCF holds
``NON_AMBIGUOUS[base]`` there and the genome may hold an IUPAC code.  Nothing here knows records, pools or kernels.
``tests/test_vcf_replay_host.py`` holds it against the bytes the real reference wrote.
"""
from __future__ import annotations


def read_fasta(text: bytes):
    """[(defline without '>', upper-cased bases, bases of the first line)] of a Fasta text."""
    out = []
    for block in text.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        lines = body.split(b"\n")
        out.append((head.decode(), b"".join(lines).upper(), len(lines[0]) if lines else 0))
    return out


def data_lines(vcf: bytes):
    """CHROM -> [(POS, REF, ALT, INFO)] in file order."""
    by = {}
    for line in vcf.split(b"\n"):
        if not line or line.startswith(b"#"):
            continue
        f = line.split(b"\t")
        by.setdefault(f[0].decode(), []).append((int(f[1]), f[3], f[4], f[7]))
    return by


def replay(seq: bytes, lines) -> bytes:
    out, at = [], 0                       # at: next input base not yet written
    for pos, ref, alt, info in lines:
        a = pos - 1
        kind = info.split(b";")[0]
        if kind in (b"SVTYPE=INS", b"SVTYPE=INS:ME", b"SVTYPE=DEL", b"SVTYPE=DEL:ME"):
            short, long_ = (ref, alt) if kind.startswith(b"SVTYPE=INS") else (alt, ref)
            assert len(short) == 1 and len(long_) >= 2
            if long_[:1] == short:        # leading anchor: stays as the genome has it
                a, ref, alt = a + 1, ref[1:], alt[1:]
            else:                         # trailing anchor
                assert long_[-1:] == short
                ref, alt = ref[:-1], alt[:-1]
        assert a >= at, f"line at POS {pos} overlaps its predecessor"
        out.append(seq[at:a])
        out.append(alt)
        at = a + len(ref)
    out.append(seq[at:])
    return b"".join(out)


def frame(seq: bytes, bpl: int) -> bytes:
    """Body text as FastaWriter leaves it: a newline after every ``bpl`` bases, none after a partial last line."""
    return b"\n".join(seq[i:i + bpl] for i in range(0, len(seq), bpl)) + (b"\n" if seq and len(seq) % bpl == 0 else b"")


def replay_fasta(fasta: bytes, vcf: bytes) -> bytes:
    """The whole mutated Fasta file."""
    by = data_lines(vcf)
    out, partial = [], False
    for head, seq, bpl in read_fasta(fasta):
        got = replay(seq, by.get(head.split()[0] if head.split() else "", []))
        out.append((b"\n" if partial else b"") + b">" + head.encode() + b"\n" + frame(got, bpl))
        partial = bool(got) and len(got) % bpl != 0
    return b"".join(out)
