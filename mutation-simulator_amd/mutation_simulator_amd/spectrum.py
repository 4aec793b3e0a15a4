"""``--spectrum FILE [--signature NAME]``: SNPs drawn per trinucleotide context from a 96-channel mutational spectrum -- the
pyrimidine-centred ``N[X>Y]N`` table COSMIC's SBS signatures are published in.

This module holds the host side: the file parser, the mapping from (context, alternative base) to channel, and the exact
per-contig probabilities as the 192 64-bit thresholds ``msim_plan_contig_spectrum`` compares its draws with
(include/msim.h; csrc/spectrum.hip draws).

Census (``Engine.context_counts``): ``code(A, C, G, T) = 0..3``, any other byte is invalid; site ``p`` is eligible iff
``1 <= p <= L - 2`` and its three bases are valid; ``ctx = 16 code(b[p-1]) + 4 code(b[p]) + code(b[p+1])``.

Probabilities, per contig, in exact rational arithmetic over the doubles as parsed::

    p(ctx, aux) = RATE * n_valid * w[channel(ctx, aux)] / W / (counts[ctx] + counts[rc(ctx)])        W = sum of the 96 weights

so that the expected number of SNPs of the contig is ``RATE * n_valid``, spread over the channels in the file's proportions
(a channel is reached from a context and from its reverse complement: the two share its weight by their counts).  A channel
whose contexts do not occur in the contig contributes nothing -- the contig then gets fewer SNPs than ``RATE * n_valid``.
``thr[3 ctx + j] = min(2**64 - 1, floor(2**64 * (p(ctx, 0) + ... + p(ctx, j))))``; a context that occurs and whose three
probabilities sum to more than 1 is refused, nothing is clamped.
"""
from __future__ import annotations

import functools
import math
import re
from fractions import Fraction
from pathlib import Path

BASES = "ACGT"
SUBSTITUTIONS = ("C>A", "C>G", "C>T", "T>A", "T>C", "T>G")
# the 96 channels in the order the weights are kept in: substitution-major, then the 5' base, then the 3' base
CHANNELS = tuple(f"{l}[{s}]{r}" for s in SUBSTITUTIONS for l in BASES for r in BASES)
_INDEX = {name: i for i, name in enumerate(CHANNELS)}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
# the alternative base of an SN record's aux (csrc/vcf_parse.h: vcf_ti, vcf_tv(0, .), vcf_tv(1, .))
_ALT = ({"A": "G", "G": "A", "T": "C", "C": "T"},
        {"A": "T", "G": "C", "T": "G", "C": "A"},
        {"A": "C", "G": "T", "T": "A", "C": "G"})
_TWO64 = 1 << 64
_ROW = re.compile(r"^[A-Za-z]\[[A-Za-z]>[A-Za-z]\][A-Za-z]$")
_SPLIT = re.compile(r"[\t,]| +")


class SpectrumError(Exception):
    """A spectrum file that cannot be used, or a spectrum and a rate that ask a context for a probability above 1."""


def context_name(ctx: int) -> str:
    return BASES[ctx >> 4] + BASES[(ctx >> 2) & 3] + BASES[ctx & 3]


def rc(ctx: int) -> int:
    """The reverse-complement context."""
    return ((3 - (ctx & 3)) << 4) | ((3 - ((ctx >> 2) & 3)) << 2) | (3 - (ctx >> 4))


def channel_name(ctx: int, aux: int) -> str:
    l, ref, r = context_name(ctx)
    alt = _ALT[aux][ref]
    if ref in "CT":
        return f"{l}[{ref}>{alt}]{r}"
    return f"{_COMP[r]}[{_COMP[ref]}>{_COMP[alt]}]{_COMP[l]}"


def channel_index(ctx: int, aux: int) -> int:
    return _INDEX[channel_name(ctx, aux)]


CHANNEL_OF = tuple(tuple(channel_index(ctx, aux) for aux in range(3)) for ctx in range(64))


def probabilities(counts, weights, rate) -> list:
    """``p(ctx, aux)`` as 64 triples of ``Fraction``; 0 where the context does not occur."""
    counts = [int(x) for x in counts]
    w = [Fraction(float(x)) for x in weights]
    assert len(counts) == 64 and len(w) == 96
    total = sum(w)
    scale = Fraction(float(rate)) * sum(counts) / total
    out = []
    for ctx in range(64):
        if counts[ctx] == 0:
            out.append((Fraction(0),) * 3)
            continue
        pooled = counts[ctx] + counts[rc(ctx)]
        out.append(tuple(scale * w[CHANNEL_OF[ctx][aux]] / pooled for aux in range(3)))
    return out


@functools.lru_cache(maxsize=8)
def _integer_weights(weights: tuple):
    """The 96 doubles as integers over their common denominator (a power of two), and the integers' sum."""
    fr = [Fraction(x) for x in weights]
    den = max(f.denominator for f in fr)
    a = tuple(f.numerator * (den // f.denominator) for f in fr)
    return a, sum(a)


def thresholds(counts, weights, rate) -> list:
    """The 192 thresholds of one contig (Python ints below 2**64) from its census, the 96 weights (``CHANNELS`` order) and the
    SNP rate.  ``SpectrumError`` names the first context whose probabilities sum to more than 1.  ``probabilities`` in integers
    over one denominator per context (a run evaluates this once per contig): floor(2**64 * sum p) exactly."""
    counts = [int(x) for x in counts]
    assert len(counts) == 64 and len(weights) == 96
    a, total = _integer_weights(tuple(float(x) for x in weights))
    r = Fraction(float(rate))
    num = r.numerator * sum(counts)
    thr = []
    for ctx in range(64):
        if counts[ctx] == 0:
            thr += [0, 0, 0]
            continue
        den = r.denominator * total * (counts[ctx] + counts[rc(ctx)])
        cum = [0, 0, 0]
        acc = 0
        for aux in range(3):
            acc += num * a[CHANNEL_OF[ctx][aux]]
            cum[aux] = acc
        if acc > den:
            raise SpectrumError(f"--spectrum: context {context_name(ctx)} would mutate with probability {acc / den:.6g} > 1 at this "
                                f"SNP rate (it holds {counts[ctx]} of the contig's {sum(counts)} eligible sites): "
                                "lower -sn or use a flatter spectrum")
        thr += [min(_TWO64 - 1, (c << 64) // den) for c in cum]
    return thr


def parse(text: str, signature: str | None = None, where: str = "spectrum") -> list:
    """The 96 weights (``CHANNELS`` order) of one column of a spectrum table.  Text; ``#`` lines and blank lines are skipped; fields
    are split on tab, comma or runs of blanks; the first field is ``N[X>Y]N`` with X in {C, T}.  A first line whose first field
    is not of that form is a header naming the columns: ``signature`` picks one by name (default: the first value column)."""
    weights: dict = {}
    col, names, first = 1, None, True
    last = 0
    for no, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        last = no
        fields = _SPLIT.split(line)
        if first:
            first = False
            if not _ROW.match(fields[0]):
                names = fields[1:]
                if signature is not None:
                    if signature not in names:
                        raise SpectrumError(f"{where} line {no}: no signature named {signature!r}; the file has: {', '.join(names) or '(none)'}")
                    col = 1 + names.index(signature)
                elif not names:
                    raise SpectrumError(f"{where} line {no}: the header names no value column")
                continue
            if signature is not None:
                raise SpectrumError(f"{where} line {no}: no signature named {signature!r}; the file has no header line")
        if not _ROW.match(fields[0]):
            raise SpectrumError(f"{where} line {no}: {fields[0]!r} is no channel of the form N[X>Y]N")
        name = fields[0].upper()
        l, x, y, r = name[0], name[2], name[4], name[6]
        if any(b not in BASES for b in (l, x, y, r)) or x == y:
            raise SpectrumError(f"{where} line {no}: {fields[0]!r} is no substitution between A, C, G and T")
        if x not in "CT":
            raise SpectrumError(f"{where} line {no}: {fields[0]!r} is purine-centred; channels are pyrimidine-centred (X in C, T): "
                                "give its reverse complement")
        if name in weights:
            raise SpectrumError(f"{where} line {no}: channel {name} appears twice")
        if len(fields) <= col:
            raise SpectrumError(f"{where} line {no}: no value in column {col + 1}")
        try:
            value = float(fields[col])
        except ValueError:
            raise SpectrumError(f"{where} line {no}: {fields[col]!r} is no number") from None
        if not math.isfinite(value) or value < 0:
            raise SpectrumError(f"{where} line {no}: weight {fields[col]} of {name} is not a finite, non-negative number")
        weights[name] = value
    if len(weights) != 96:
        missing = [c for c in CHANNELS if c not in weights]
        raise SpectrumError(f"{where} line {last}: {len(weights)} channels, 96 are required (missing: {', '.join(missing[:4])}"
                            f"{' ...' if len(missing) > 4 else ''})")
    out = [weights[c] for c in CHANNELS]
    if not sum(Fraction(v) for v in out) > 0:
        raise SpectrumError(f"{where} line {last}: all 96 weights are zero")
    return out


def column_name_refusal(names):
    """Why ``names`` cannot head the columns of a table ``parse`` reads back, or None: tab, comma and blank are its
    separators, and ``--signature`` picks the first column of a name."""
    seen = set()
    for name in names:
        if not name or any(ch in name for ch in "\t, \n\r"):
            return f"column name {name!r} is empty or holds a tab, a comma or a blank (the spectrum table's separators)"
        if name in seen:
            return f"column name {name!r} appears twice"
        seen.add(name)
    return None


def opportunities(counts) -> list:
    """The 32 pyrimidine-centred contexts with the eligible sites a channel of theirs can be reached from,
    ``counts[ctx] + counts[rc(ctx)]`` (a census, ``Engine.context_counts``): the denominator that turns counts into rates."""
    counts = [int(x) for x in counts]
    assert len(counts) == 64
    return [(context_name(ctx), counts[ctx] + counts[rc(ctx)]) for ctx in range(64) if context_name(ctx)[1] in "CT"]


def render_profile(columns, opportunities=None, notes=()) -> str:
    """The text of a spectrum table holding counts (``profile`` mode): ``#`` comment lines first -- ``notes``, then one
    ``# opportunities XYZ n`` line per pair of ``opportunities`` -- a header ``Type<TAB>name...``, and the 96 rows in ``CHANNELS``
    order with integer counts.  ``columns``: (name, 96 counts) pairs.  ``parse(text, name)`` returns exactly those counts, as
    floats, for every column (counts are below 2**53)."""
    columns = [(str(name), [int(x) for x in values]) for name, values in columns]
    refusal = "no column" if not columns else column_name_refusal([name for name, _ in columns])
    if refusal:
        raise SpectrumError(f"profile: {refusal}")
    if any(len(values) != 96 or min(values) < 0 or max(values) >= 1 << 53 for _, values in columns):
        raise SpectrumError("profile: a column holds 96 counts in [0, 2**53)")
    lines = [f"# {note}" for note in notes]
    lines += [f"# opportunities {name} {int(n)}" for name, n in (opportunities or ())]
    lines.append("\t".join(["Type"] + [name for name, _ in columns]))
    for i, channel in enumerate(CHANNELS):
        lines.append("\t".join([channel] + [str(values[i]) for _, values in columns]))
    return "\n".join(lines) + "\n"


def load(path, signature: str | None = None) -> list:
    path = Path(path)
    try:
        text = path.read_text()
    except OSError as e:
        raise SpectrumError(f"--spectrum: cannot read {path}: {e.strerror or e}") from None
    except UnicodeDecodeError:
        raise SpectrumError(f"--spectrum: {path} is no text file") from None
    return parse(text, signature, path.name)
