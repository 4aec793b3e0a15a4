"""``mutation-simulator genome.fa profile calls.vcf``: the SBS-96 spectrum of a VCF's SNPs against the reference, counted on
the GPU -- the inverse of ``args --spectrum FILE``, and a file that option reads as it stands.

The VCF goes through the ``vcf`` mode's loader and parsers (``vcf_replay.load_vcf_text`` / ``plan_all``: both grammars, BGZF
input, the same "VCF line N: reason" refusals), so a profile counts exactly the SNPs a replay would apply.  Per contig
``msim_sbs_counts`` walks the record table against the resident reference bases (csrc/spectrum.hip: k_sbs_count) and
``msim_context_counts`` takes the census the opportunities come from.  Nothing is applied, no Fasta is written, no generator
is touched.

Rules (include/msim.h): an SN record at ``p`` has a channel iff ``p`` is an eligible site of the census -- ``1 <= p <= L - 2``
and its three reference bases are A, C, G or T; the channel is ``spectrum.CHANNEL_OF[ctx][aux]``.  The context is always the
reference's: neighbouring SNPs do not see each other.  SN records without a channel and every other record are tallied in
the file's comment lines, never dropped silently.
"""
from __future__ import annotations

import numpy as np

from . import _ffi, spectrum
from .vcf_replay import load_vcf_text, plan_all, resident_genome

TALLY_NAMES = ("no context", "SN", "IN", "DE", "DU", "IV", "TL", "TLI")   # msim_sbs_counts: tallies[0..7]


class ProfileError(Exception):
    """The profile cannot be written as asked (the message says why)."""


def column_refusal(name: str, contig_names, per_contig: bool):
    """Why the file's columns cannot be named so, or None: the genome-wide column's name and, with ``--per-contig``, the
    contigs' names head the columns of a table whose separators are tab, comma and blank."""
    names = [name] + (list(contig_names) if per_contig else [])
    refusal = spectrum.column_name_refusal(names)
    if refusal is None:
        return None
    if per_contig:
        return f"profile --per-contig: {refusal}; --name and the contigs' names head the file's columns"
    return f"profile --name: {refusal}"


class Profile:
    """Counts the profile of one VCF on the GPU and writes ``*_ms.sbs96.tsv``."""

    def __init__(self, args, fasta, engine=None):
        self._args = args
        self._fasta = fasta
        self._device = getattr(args, "device", 0) or 0
        self._engine = engine
        self._own_engine = engine is None
        self.stats: dict = {}
        self.channels = None         # uint64[contigs, 96] of the last run
        self.tallies = None          # uint64[contigs, 8]
        self.census = None           # uint64[contigs, 64]

    def run(self):
        fa, args = self._fasta, self._args
        per_contig = bool(getattr(args, "per_contig", False))
        refusal = column_refusal(args.name, [fa[i].name for i in range(len(fa))], per_contig)
        if refusal:                                    # (before anything reaches the GPU)
            raise ProfileError(refusal)
        if self._engine is None:
            self._engine = _ffi.Engine(self._device)
        eng = self._engine
        text = load_vcf_text(args.vcffile, eng)
        _, names, cids = resident_genome(eng, fa, "profile")
        consensus = None
        if getattr(args, "consensus", False):
            consensus = (getattr(args, "sample", None), getattr(args, "haplotype", None) or 1)
        plan_all(eng, text, names, cids, consensus)
        # every line is accepted: count, contig by contig
        sbs0, census0 = eng.sbs_timing(), eng.spectrum_timing()[0]     # (a caller's engine may have counted before)
        n = len(cids)
        self.channels = np.zeros((n, _ffi.SBS_CHANNELS), dtype=np.uint64)
        self.tallies = np.zeros((n, _ffi.SBS_TALLIES), dtype=np.uint64)
        self.census = np.zeros((n, 64), dtype=np.uint64)
        for i, cid in enumerate(cids):
            self.channels[i], self.tallies[i] = eng.sbs_counts(cid)
            self.census[i], _ = eng.context_counts(cid)
        load_ms, plan_ms = eng.vcf_timing()
        self.stats = {"vcf_bytes": int(text.shape[0]), "vcf_load_kernel_ms": load_ms, "vcf_plan_kernel_ms": plan_ms,
                      "sbs_kernel_ms": round(eng.sbs_timing() - sbs0, 4), "census_ms": round(eng.spectrum_timing()[0] - census0, 4)}
        eng.vcf_release()
        args.outprofile.write_text(self.render(names, per_contig))

    def render(self, names, per_contig: bool) -> str:
        args = self._args
        total = self.channels.sum(axis=0, dtype=np.uint64)
        tallies = self.tallies.sum(axis=0, dtype=np.uint64)
        columns = [(args.name, total)]
        if per_contig:
            columns += [(name, self.channels[i]) for i, name in enumerate(names)]
        notes = [f"SBS-96 profile of {args.vcffile.name} against {getattr(args, 'genome_name', args.infile.name)} "
                 f"({len(names)} contigs): SNPs per pyrimidine-centred channel, reference context"]
        if getattr(args, "consensus", False):
            sample = getattr(args, "sample", None)
            notes.append(f"consensus: sample {sample if sample is not None else '(first)'} haplotype {getattr(args, 'haplotype', None) or 1}")
        order = (1, 0, 2, 3, 4, 5, 6, 7)               # SN, no context, IN .. TLI
        notes.append("records: " + ", ".join(f"{TALLY_NAMES[t]} {int(tallies[t])}" for t in order))
        notes.append("opportunities: eligible sites of the reference per context, with its reverse complement's")
        return spectrum.render_profile(columns, spectrum.opportunities(self.census.sum(axis=0, dtype=np.uint64)), notes)

    def close(self):
        eng = self._engine
        self._engine = None
        if eng is not None and self._own_engine:
            eng.close()
