"""``mutation-simulator genome.fa vcf truth.vcf``: the mutated Fasta again, from the reference and the VCF of a run; with
``--consensus [--sample NAME] [--haplotype N]`` from any VCF, one haplotype of one sample (``msim_vcf_select``).

Every data line replaces REF at POS by ALT; libmsim parses the text into the record tables the mutation pass would have
planned (``msim_vcf_*``, csrc/vcf_parse.hip), the unchanged rewrite produces the bytes, and ``FastaWriter`` with the
output channels writes them -- ``--bgzip`` included; ``--chain`` adds the tables' liftover chains (``chain_writer.py``).  No generator is touched: there is nothing random about a replay.

The whole genome is resident while the VCF is checked, because nothing is rewritten before every line has been accepted.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from . import _ffi
from .chain_writer import ChainWriter
from .fasta_io import UnsupportedCompressionFormat, put_contig
from .fasta_writer import FastaWriter

MAX_CONTIGS = 65536          # contigs one context holds (csrc/ctx.h)


class VcfReplayError(Exception):
    """The VCF cannot be replayed onto this Fasta (the message names the line)."""


def load_vcf_text(path, engine) -> np.ndarray:
    """The VCF's text as a uint8 array; a BGZF ``.vcf.gz`` (by content) is inflated on the device, plain gzip refused as
    the Fasta loader refuses it."""
    path = Path(path)
    if not path.is_file():
        raise FileNotFoundError(f"Cannot read VCF from file {path}")
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.shape[0] >= 2 and raw[0] == 0x1F and raw[1] == 0x8B:
        try:
            total, _ = _ffi.bgzf_probe(raw)
        except _ffi.MsimError as e:
            if getattr(e, "code", None) != _ffi.ERR_VALUE:
                raise
            raise UnsupportedCompressionFormat(
                f"Compressed VCF is only supported in BGZF format. Use the samtools bgzip utility (instead of gzip) to "
                f"compress {path} ({str(e).split(': ', 1)[-1]})") from None
        if total == 0:
            return np.zeros(0, np.uint8)
        try:
            return engine.bgzf_inflate(raw, out=np.empty(total, dtype=np.uint8))
        except _ffi.MsimError as e:
            if getattr(e, "code", None) != _ffi.ERR_VALUE:
                raise
            raise VcfReplayError(f"Compressed VCF {path} is damaged: {str(e).split(': ', 1)[-1]}") from None
    return raw


def sample_column(text: np.ndarray, groups, sample) -> int:
    """The 0-based sample column called ``sample`` (None: the first), from the ``#CHROM`` header line: the last line that
    starts so among the bytes in front of the first data line."""
    head = text[:int(groups["name_off"][0])] if len(groups) else text
    names = None
    for line in head.tobytes().split(b"\n"):
        if line.startswith(b"#CHROM"):
            names = line.rstrip(b"\r").split(b"\t")[9:]
    if sample is None:
        return 0
    want = sample.encode("utf-8", "replace")
    if names is None or want not in names:
        raise VcfReplayError(f"the VCF has no sample column {sample!r}")
    return names.index(want)


def resident_genome(engine, fasta, mode_name: str):
    """Every record of ``fasta`` as a contig of ``engine``, for the modes that keep the whole genome resident (``vcf``,
    ``profile``, ``compare``): (records, their names, their contig ids).  A genome of more contigs than a context holds is
    refused before anything is uploaded."""
    if len(fasta) > MAX_CONTIGS:
        raise _ffi.MsimUnsupported(f"{mode_name} mode keeps the genome resident: more than {MAX_CONTIGS} contigs")
    recs = [fasta[i] for i in range(len(fasta))]
    return recs, [r.name for r in recs], [put_contig(engine, r) for r in recs]


def plan_all(engine, text: np.ndarray, names, contig_ids, consensus=None, after_plan=None) -> None:
    """Load ``text`` and plan every contig (``contig_ids[i]`` is the context's id of the contig called ``names[i]``) from the
    lines that name it, in FILE order, so that the first offending line of the file is the one reported (ValueError /
    VcfReplayError, "VCF line N: ...").  Contigs without lines get an empty table.  Nothing has been rewritten when this raises.
    ``consensus``: None for the simulator's dialect, or (sample name or None, haplotype) for the general grammar.
    ``after_plan``: None, or a hook called as ``after_plan(contig id)`` directly behind each contig's plan."""
    engine.vcf_load(text)
    plan_loaded(engine, text, names, contig_ids, consensus, after_plan)


def plan_loaded(engine, text: np.ndarray, names, contig_ids, consensus=None, after_plan=None) -> None:
    """``plan_all`` behind its ``vcf_load``: plan every contig from the text the context already holds, under the grammar and
    haplotype selected here -- so one loaded file can be planned once per haplotype (``compare --diploid``)."""
    groups = engine.vcf_groups()
    if consensus is not None:
        sample, haplotype = consensus
        try:
            engine.vcf_select(1, sample_column(text, groups, sample), haplotype)
        except _ffi.MsimError as e:                    # (the #CHROM line names more samples than the data lines hold)
            if getattr(e, "code", None) != _ffi.ERR_ARG:
                raise
            raise VcfReplayError(str(e).split(": ", 1)[-1]) from None
    by_name = {}
    for i, name in enumerate(names):
        by_name.setdefault(name.encode("utf-8", "replace"), i)
    seen = set()
    for k in range(len(groups)):
        off, nlen, line = int(groups["name_off"][k]), int(groups["name_len"][k]), int(groups["first_line"][k]) + 1
        chrom = text[off:off + nlen].tobytes()
        i = by_name.get(chrom) if nlen <= 255 else None
        if i is None:
            raise VcfReplayError(f"VCF line {line}: CHROM {chrom[:64].decode('utf-8', 'replace')!r} is no contig of the Fasta")
        if i in seen:
            raise VcfReplayError(f"VCF line {line}: the lines of contig {names[i]!r} are not contiguous in the file")
        seen.add(i)
        try:
            engine.vcf_plan_contig(contig_ids[i], k)
        except ValueError as e:
            raise VcfReplayError(str(e)) from None
        if after_plan is not None:
            after_plan(contig_ids[i])
    for i, cid in enumerate(contig_ids):
        if i not in seen:
            engine.vcf_plan_contig(cid, -1)
            if after_plan is not None:
                after_plan(cid)


class VcfReplay:
    """Runs the replay of one genome on the GPU and writes ``*_ms.fa``."""

    def __init__(self, args, fasta, engine=None):
        self._args = args
        self._fasta = fasta
        self._bgzip = bool(getattr(args, "bgzip", False))
        self._device = getattr(args, "device", 0) or 0
        self._engine = engine
        self._own_engine = engine is None
        self._writer = None
        self._chain_writer = None
        self.stats: dict = {}

    def run(self):
        fa = self._fasta
        if self._engine is None:
            self._engine = _ffi.Engine(self._device)
        eng = self._engine
        text = load_vcf_text(self._args.vcffile, eng)
        recs, names, cids = resident_genome(eng, fa, "vcf")
        consensus = None
        if getattr(self._args, "consensus", False):
            consensus = (getattr(self._args, "sample", None), getattr(self._args, "haplotype", None) or 1)
        plan_all(eng, text, names, cids, consensus)
        # every line is accepted: rewrite and write, contig by contig
        if getattr(self._args, "chain", False):        # the one extra file of this mode: the chains of the replayed tables
            self._chain_writer = ChainWriter(self._args.outchain)      # (first: if it cannot be written, no Fasta is left)
        self._writer = FastaWriter(self._args.outfasta, bgzip=self._bgzip, device=self._device)
        self._writer.attach(eng)
        for number, (rec, cid) in enumerate(zip(recs, cids)):
            bpl = fa.faidx.index[rec.name].lenc
            self._writer.set_bpl(bpl)
            self._writer.write_header(rec.long_name)
            eng.apply_contig(cid)
            if bpl > 0:
                out_len = eng.result_sizes(cid)[0]
                try:
                    fd, pos = self._writer.native_span()
                    n_done = eng.fetch_sequence_framed_to_file(cid, bpl, fd, pos)
                    self._writer.commit_native(pos, n_done, out_len)
                except _ffi.MsimUnsupported:           # no regular file: through a mapping made here
                    region = self._writer.map_region(out_len + out_len // bpl)
                    try:
                        eng.fetch_sequence_framed_into(cid, bpl, region.view)
                    finally:
                        self._writer.commit_region(region, out_len)
            else:
                self._writer.write_array(eng.fetch_sequence(cid))
            if self._chain_writer is not None:
                self._chain_writer.write_contig(eng, cid, rec.name, number)
            eng.release_result(cid)
        eng.file_wait()
        load_ms, plan_ms = eng.vcf_timing()
        self.stats = {"vcf_bytes": int(text.shape[0]), "vcf_load_kernel_ms": load_ms, "vcf_plan_kernel_ms": plan_ms}
        eng.vcf_release()

    def close(self):
        pending = None
        eng = self._engine
        if getattr(eng, "h", None):
            try:
                eng.file_wait()
            except _ffi.MsimError as e:
                pending = e
        try:
            if self._writer is not None:
                self._writer.close()                   # (BGZF: tail and EOF marker go out through the engine)
            if self._chain_writer is not None:
                self._chain_writer.close()
        finally:
            self._engine = None
            if eng is not None and self._own_engine:
                eng.close()
        if pending is not None:
            raise pending
