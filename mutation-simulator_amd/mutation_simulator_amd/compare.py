"""``mutation-simulator genome.fa compare truth.vcf calls.vcf``: a calls VCF scored against a truth VCF on the GPU -- the step
behind simulating a genome with a known truth set.

Both files go through the ``vcf`` mode's loader and the consensus grammar (``vcf_replay.load_vcf_text`` / ``plan_all``: any VCF,
BGZF input, one sample and one haplotype a side, the same "VCF line N: reason" refusals, here with ``truth`` or ``calls`` in
front).  The truth's record tables are planned first and HELD (``msim_cmp_hold``), the calls' tables are planned over them, and
``msim_cmp_counts`` joins the two per contig against the resident reference bases (csrc/compare.hip: k_cmp_match, k_cmp_tally).
Nothing is applied, no Fasta is written, no generator is touched.

Rules (include/msim.h): an SNP matches at the same position with the same alternative base; an insertion or deletion matches a
record of the same type and length that is a shifted placement of it -- anywhere inside the homopolymer or tandem repeat it
stands in, an insertion's bytes rotating with it -- as long as both lie in the same window of 65 536 bases and no base outside
A, C, G, T is stepped over; ``--exact`` compares positions literally.  Inside one class of equivalent records the i-th of the
truth matches the i-th of the calls.  Counts come per record type and, for insertions and deletions, per length bin.

``--diploid`` scores genotypes: per side haplotype 1 is planned and held, haplotype 2 is planned from the same loaded text, and
``msim_cmp_join`` joins the two tables per contig into one table of distinct variants with a dosage each (``0/1`` or ``1/1``; phase
is ignored, a haploid ``1`` counts as ``1/1``).  ``msim_cmp_counts_diploid`` matches the truth's table against the calls' by the
same rules and compares the dosages: the table gains a ``GT`` column -- pairs found with the wrong genotype, which count in ``FN``
and in ``FP`` as hap.py reports them.  One renderer writes both tables: the counts' last axis (4 or 6) says which.

``--blocks [--block-gap N]`` (haploid only) rescues records the match leaves unmatched although both files describe the same
sequence: ``msim_cmp_counts_blocks`` cuts both tables into blocks of neighbouring records, replays every block that holds an
unmatched record -- the bytes the rewrite writes with the truth's records of the block alone against the bytes it writes with the
calls' alone (csrc/cmp_blocks.hip) -- and marks the unmatched records of an equal block as matched as part of a block.  The table
gains ``TP.calls``, ``BLK`` and ``BLK.calls``, the comment lines a ``blocks:`` line, the records file ``BLK`` lines.

``--diploid --phased`` compares the phasing as well: behind each haplotype's plan ``msim_cmp_phase_mark`` reads every record's
phase word off its line (``GT`` written with ``|``, ``PS``), behind each join ``msim_cmp_phase_join`` hands the words to the
diploid table, and behind each contig's counts ``msim_cmp_phase_counts`` takes the matched hets that are phased on both sides in
position order (csrc/cmp_phase.hip): blocks, raw switch bits, switches and flips, Hamming distance.  ``*_ms.compare.phase.tsv``
holds them, the comment lines of the table a ``phasing:`` line, the records file ``SW`` lines.

``--regions FILE`` and ``--stratify NAME=FILE`` (repeatable) score inside BED intervals (``bed.py``; csrc/cmp_regions.hip).  A record
is judged by its ANCHOR alone -- an insertion's or deletion's leftmost placement, the left end of the interval the match gives it;
with ``--exact`` and for every other type its position --, so both records of a matched pair fall on the same side of every region
edge and ``TP == TP.calls`` holds in every table.  Per contig, behind the count call, the sets go onto the contig (set 0: the
confident regions; the strata on the free bits, seven a batch with ``--regions``, eight without), ``msim_cmp_regions_mark`` gives
every record of both tables a mark byte once per batch, and ``msim_cmp_counts_regions`` tallies the count call's flag bytes again
under a mask: the main table holds the records inside ``--regions`` only (``--per-contig`` as before), a ``regions:`` comment line
says how many records lay outside and were not scored, ``--list`` lists inside records only, and behind the table comes one
genome-wide block per stratum -- the records inside the stratum and inside ``--regions``.  Limits: only the anchor counts (a long
deletion that reaches out of an interval is inside if its anchor is); strata are genome-wide, not per contig; not with
``--phased``, whose phase table would silently stay genome-wide.
"""
from __future__ import annotations

import contextlib

import numpy as np

from . import _ffi
from .bed import BedError, Regions
from .vcf_replay import VcfReplayError, load_vcf_text, plan_all, plan_loaded, resident_genome

TYPE_NAMES = (None, "SN", "IN", "DE", "DU", "IV", "TL", "TLI")            # msim.h: MSIM_SN .. MSIM_TLI
BIN_NAMES = ("1", "2-5", "6-20", "21-50", "51+")                          # msim_cmp_counts: the length bins of IN and DE
ROWS = [(t, b) for t in range(1, 8) for b in (range(_ffi.CMP_BINS) if t in (2, 3) else (0,))]
HEADER = ("type", "length", "truth", "calls", "TP", "FN", "FP", "recall", "precision")
HEADER_DIPLOID = HEADER[:7] + ("GT",) + HEADER[7:]                        # --diploid: counts[..., 6]
HEADER_BLOCKS = HEADER[:7] + ("TP.calls", "BLK", "BLK.calls") + HEADER[7:]  # --blocks: counts[..., 6], the middle outcome block-matched


class CompareError(Exception):
    """The comparison cannot be made as asked (the message says why)."""


@contextlib.contextmanager
def refusals_of(side: str):
    """What the loader's grammar refuses inside the block, raised as a CompareError that names the side (``truth``, ``calls``)."""
    try:
        yield
    except (VcfReplayError, ValueError) as e:
        msg = str(e)
        raise CompareError(f"{side} {msg}" if msg.startswith("VCF line") else f"{side} VCF: {msg}") from None


def ratio(n: int, d: int) -> str:
    return "NA" if d == 0 else f"{n / d:.6f}"


def row_cells(kind: str, length: str, v) -> list:
    """One row of the table from a cell's values: (truth matched, truth missed, calls matched, calls extra) or, with genotypes,
    (truth matched, genotype-mismatched, missed, calls matched, genotype-mismatched, extra) -- a genotype mismatch counts in FN
    and in FP, and once in the ``GT`` column."""
    v = [int(x) for x in v]
    half = len(v) // 2
    tm, cm = v[0], v[half]
    fn, fp = sum(v[1:half]), sum(v[half + 1:])
    gt = [str(v[1])] if half == 3 else []
    return [kind, length, str(tm + fn), str(cm + fp), str(tm), str(fn), str(fp)] + gt + [ratio(tm, tm + fn), ratio(cm, cm + fp)]


def row_cells_blocks(kind: str, length: str, v) -> list:
    """One row of the ``--blocks`` table from (truth matched, block-matched, missed, calls matched, block-matched, extra): a
    block-matched record is a true positive on its side -- ``TP`` and ``TP.calls`` hold both kinds, ``BLK`` and ``BLK.calls`` the
    block-matched part (a block pairs records, not one with one: the two sides' counts differ)."""
    tm, tb, fn, cm, cb, fp = (int(x) for x in v)
    return [kind, length, str(tm + tb + fn), str(cm + cb + fp), str(tm + tb), str(fn), str(fp), str(cm + cb), str(tb), str(cb),
            ratio(tm + tb, tm + tb + fn), ratio(cm + cb, cm + cb + fp)]


def render_block(counts, blocks: bool = False) -> list:
    """The rows of one ``counts[8][CMP_BINS][4]`` (``[6]``: with the ``GT`` column or, with ``blocks``, the ``BLK`` columns): a row
    per type and length bin, then ALL."""
    counts = np.asarray(counts, dtype=np.uint64)
    width = counts.shape[-1]
    cells = row_cells_blocks if blocks else row_cells
    lines = ["\t".join(HEADER_BLOCKS if blocks else HEADER_DIPLOID if width == 6 else HEADER)]
    for t, b in ROWS:
        lines.append("\t".join(cells(TYPE_NAMES[t], BIN_NAMES[b] if t in (2, 3) else ".", counts[t, b])))
    lines.append("\t".join(cells("ALL", ".", counts.reshape(-1, width).sum(axis=0, dtype=np.uint64))))
    return lines


def render(notes, counts, names=None, blocks: bool = False) -> str:
    """The text of ``*_ms.compare.tsv``: ``#`` comment lines (``notes``), the genome-wide block (the sum of ``counts`` over
    its first axis, the contigs) and, with ``names``, a ``# contig NAME`` line and a block per contig."""
    counts = np.asarray(counts, dtype=np.uint64)
    lines = [f"# {note}" for note in notes]
    lines += render_block(counts.sum(axis=0, dtype=np.uint64), blocks)
    for i, name in enumerate(names or ()):
        lines.append(f"# contig {name}")
        lines += render_block(counts[i], blocks)
    return "\n".join(lines) + "\n"


# ---- --diploid --phased: the phase table and the SW lines of --list -----------------------------------------------------------
PHASE_HEADER = ("contig", "truth.het.phased", "calls.het.phased", "pairs", "blocks", "singletons", "assessed", "switch.raw", "switch.rate",
                "switches", "flips", "switchflip.rate", "hamming", "hamming.rate")
PHASED_GT = {1: "1|0", 2: "0|1"}                                          # a het's genotype byte, phased


def phase_row(label: str, out) -> str:
    """One row of ``*_ms.compare.phase.tsv`` from the values of ``msim_cmp_phase_counts``: ``switch.rate`` = raw switch bits /
    assessed adjacencies, ``switchflip.rate`` = (switches + flips) / assessed, ``hamming.rate`` = Hamming / pairs in blocks of two
    or more."""
    th, ch, pairs, blocks, single, assessed, raw, sw, fl, ham, blocked = (int(x) for x in out)
    return "\t".join([label, str(th), str(ch), str(pairs), str(blocks), str(single), str(assessed), str(raw), ratio(raw, assessed),
                      str(sw), str(fl), ratio(sw + fl, assessed), str(ham), ratio(ham, blocked)])


def render_phase(notes, phase, names=None) -> str:
    """The text of ``*_ms.compare.phase.tsv``: ``#`` comment lines, the header, the ``ALL`` row (the sum of ``phase`` over the
    contigs) and, with ``names``, a row per contig."""
    phase = np.asarray(phase, dtype=np.uint64).reshape(-1, _ffi.CMP_PHASE_COUNTS)
    lines = [f"# {note}" for note in notes] + ["\t".join(PHASE_HEADER), phase_row("ALL", phase.sum(axis=0, dtype=np.uint64))]
    lines += [phase_row(name, phase[i]) for i, name in enumerate(names or ())]
    return "\n".join(lines) + "\n"


def switch_rows(contig: str, truth, truth_gt, state) -> list:
    """The ``SW`` lines of ``--list`` for one contig: every pair with a raw switch bit -- kind, contig, 1-based position, type,
    length, the truth's and the calls' genotype as ``1|0`` / ``0|1`` (state bit 2: the calls' is the other one)."""
    out = []
    for k in np.flatnonzero(np.asarray(state) & 2):
        r, g = truth[k], int(truth_gt[k])
        out.append("\t".join(["SW", contig, str(int(r["pos"]) + 1), TYPE_NAMES[int(r["type"])], str(int(r["stop"]) - int(r["pos"]) + 1),
                              PHASED_GT[g], PHASED_GT[3 - g if int(state[k]) & 4 else g]]))
    return out


def record_rows(kind: str, contig: str, recs, flags, flag: int = 0, side=None) -> list:
    """The lines of ``--list`` for one table: every record whose flag byte is ``flag`` (0: unmatched; 2, with ``--blocks``:
    matched as part of a block -- ``BLK`` lines, which name their ``side``, ``truth`` or ``calls``, in a sixth field)."""
    out = []
    for r in recs[np.asarray(flags) == flag]:
        out.append("\t".join([kind, contig, str(int(r["pos"]) + 1), TYPE_NAMES[int(r["type"])],
                              str(int(r["stop"]) - int(r["pos"]) + 1)] + ([side] if side else [])))
    return out


# ---- --diploid: --list names genotypes ---------------------------------------------------------------------------------------
GT_NAMES = (".", "0/1", "1/1")                                            # by dosage


def dosage(gt) -> int:
    return (int(gt) & 1) + ((int(gt) >> 1) & 1)


def record_rows_diploid(contig: str, truth, truth_gt, truth_flags, calls, calls_gt, calls_flags) -> list:
    """The lines of ``--list`` for one contig's two diploid tables: kind, contig, 1-based position, type, length, truth genotype,
    calls genotype (``.`` where that side has no record).  The truth's records in table order -- ``FN`` where the flag byte is 0,
    ``GT`` where it is 2, written once, at the truth record's position: its partner's dosage is the other one --, then the calls'
    ``FP`` (flag byte 0)."""
    def line(kind, r, a, b):
        return "\t".join([kind, contig, str(int(r["pos"]) + 1), TYPE_NAMES[int(r["type"])], str(int(r["stop"]) - int(r["pos"]) + 1),
                          GT_NAMES[a], GT_NAMES[b]])
    out = []
    for k in np.flatnonzero(np.asarray(truth_flags) != 1):
        d = dosage(truth_gt[k])
        out.append(line("FN", truth[k], d, 0) if truth_flags[k] == 0 else line("GT", truth[k], d, 3 - d))
    for k in np.flatnonzero(np.asarray(calls_flags) == 0):
        out.append(line("FP", calls[k], 0, dosage(calls_gt[k])))
    return out


class Compare:
    """Scores one calls VCF against one truth VCF on the GPU and writes ``*_ms.compare.tsv``."""

    def __init__(self, args, fasta, engine=None):
        self._args = args
        self._fasta = fasta
        self._device = getattr(args, "device", 0) or 0
        self._engine = engine
        self._own_engine = engine is None
        self.stats: dict = {}
        self.counts = None           # uint64[contigs, 8, CMP_BINS, 4] of the last run ([..., 6] with --diploid)
        self.tallies = None          # uint64[contigs, 2]
        self.block_tallies = None    # uint64[contigs, 5] (--blocks)
        self.phase = None            # uint64[contigs, CMP_PHASE_COUNTS] (--phased)
        self.phase_marks = None      # uint64[2, 3] (--phased): per side the phased, unphased, unreadable-PS records
        self.regions = None          # bed.Regions of --regions
        self.outside = None          # uint64[contigs, 2] (--regions): the truth's and the calls' records outside, not scored
        self.strata = []             # (name, bed.Regions) per --stratify, in command-line order
        self.strata_counts = None    # uint64[strata, contigs, 8, CMP_BINS, 4 or 6]: the records inside the stratum (and --regions)
        self.strata_outside = None   # uint64[strata, contigs, 2]

    def _plan(self, eng, side: str, path, names, cids, sample, haplotype):
        """One file's tables onto the contigs; (bytes of its text, load kernel ms, plan kernel ms)."""
        text = load_vcf_text(path, eng)
        with refusals_of(side):
            plan_all(eng, text, names, cids, (sample, haplotype or 1))
        load_ms, plan_ms = eng.vcf_timing()
        return int(text.shape[0]), load_ms, plan_ms

    def _plan_diploid(self, eng, side: str, side_id: int, path, names, cids, sample):
        """One file's two haplotypes onto the contigs, joined into the side's diploid tables: haplotype 1 planned and held,
        haplotype 2 planned from the same loaded text, every contig joined."""
        text = load_vcf_text(path, eng)
        phased = bool(getattr(self._args, "phased", False))

        def marker(haplotype):
            def mark(cid):
                self.phase_marks[side_id] += eng.cmp_phase_mark(cid, side_id, haplotype)
            return mark if phased else None
        with refusals_of(side):
            plan_all(eng, text, names, cids, (sample, 1), marker(1))
            for cid in cids:
                eng.cmp_hold(cid)
            plan_loaded(eng, text, names, cids, (sample, 2), marker(2))
        for cid in cids:
            eng.cmp_join(cid, side_id)
            if phased:
                eng.cmp_phase_join(cid, side_id)
        load_ms, plan_ms = eng.vcf_timing()
        eng.vcf_release()
        return int(text.shape[0]), load_ms, plan_ms

    def _load_beds(self, names, lengths):
        """The BED files of ``--regions`` and ``--stratify`` on this genome; the seconds their scans took."""
        args = self._args
        try:
            path = getattr(args, "regions", None)
            self.regions = Regions(path, names, lengths) if path is not None else None
            self.strata = [(name, Regions(p, names, lengths)) for name, p in (getattr(args, "stratify", None) or ())]
        except BedError as e:
            raise CompareError(str(e)) from None
        return sum(r.scan_s for r in ([self.regions] if self.regions else []) + [r for _, r in self.strata])

    def _score_regions(self, eng, i, cid, exact, diploid, width):
        """Contig i behind its count call: the main counts restricted to ``--regions`` and every stratum's counts.  Returns the two
        tables' mark bytes of the batch that holds set 0 (None without ``--regions``)."""
        base = 1 if self.regions else 0                    # bit 0: the confident set; the strata take the free bits, batch by batch
        room = _ffi.CMP_REGION_SETS - base
        if self.regions:
            eng.cmp_regions_set(cid, 0, *self.regions.sets[i])
        marks = None
        for first in range(0, max(len(self.strata), 1), room):
            batch = self.strata[first:first + room]
            for j, (_, r) in enumerate(batch):
                eng.cmp_regions_set(cid, base + j, *r.sets[i])
            for j in range(len(batch), room if first else 0):
                eng.cmp_regions_drop(cid, base + j)        # (a set of the batch before: not searched again)
            eng.cmp_regions_mark(cid, exact, diploid)
            if self.regions and first == 0:
                self.counts[i], self.outside[i] = eng.cmp_counts_regions(cid, 1, exact, diploid, width)
                marks = eng.cmp_fetch_regions(cid, exact, diploid)
            for j in range(len(batch)):
                self.strata_counts[first + j, i], self.strata_outside[first + j, i] = eng.cmp_counts_regions(
                    cid, (1 << (base + j)) | base, exact, diploid, width)
        return marks

    def run(self):
        fa, args = self._fasta, self._args
        if self._engine is None:
            self._engine = _ffi.Engine(self._device)
        eng = self._engine
        recs, names, cids = resident_genome(eng, fa, "compare")
        diploid, listing = bool(getattr(args, "diploid", False)), bool(getattr(args, "list_records", False))
        blocks = bool(getattr(args, "blocks", False))
        phased = bool(getattr(args, "phased", False))
        gap = getattr(args, "block_gap", None)
        gap = _ffi.CMP_BLOCK_GAP if gap is None else int(gap)
        if blocks and diploid:
            raise CompareError("--blocks compares one haplotype against one: it cannot be combined with --diploid")
        if phased and not diploid:
            raise CompareError("--phased needs --diploid")
        restricted = getattr(args, "regions", None) is not None or bool(getattr(args, "stratify", None))
        if restricted and phased:
            raise CompareError("--regions and --stratify restrict the counts table only: they cannot be combined with --phased")
        bed_scan_s = self._load_beds(names, [len(r) for r in recs]) if restricted else 0.0
        self.phase_marks = np.zeros((2, 3), dtype=np.uint64)
        truth_sample, sample = getattr(args, "truth_sample", None), getattr(args, "sample", None)
        if diploid:
            join0 = eng.cmp_join_timing()
            truth = self._plan_diploid(eng, "truth", _ffi.CMP_TRUTH, args.truthfile, names, cids, truth_sample)
            calls = self._plan_diploid(eng, "calls", _ffi.CMP_CALLS, args.callsfile, names, cids, sample)
        else:
            truth = self._plan(eng, "truth", args.truthfile, names, cids, truth_sample, getattr(args, "truth_haplotype", None))
            for cid in cids:
                eng.cmp_hold(cid)
            eng.vcf_release()
            calls = self._plan(eng, "calls", args.callsfile, names, cids, sample, getattr(args, "haplotype", None))
        # every line of both files is accepted: count, contig by contig
        exact = bool(getattr(args, "exact", False))
        cmp0 = eng.cmp_timing()                        # (a caller's engine may have compared before)
        blk0 = eng.cmp_blocks_timing() if blocks else 0.0
        phase0 = eng.cmp_phase_timing() if phased else 0.0
        region0 = eng.cmp_regions_timing() if restricted else 0.0
        n = len(cids)
        self.counts = np.zeros((n, 8, _ffi.CMP_BINS, 6 if diploid or blocks else 4), dtype=np.uint64)
        self.tallies = np.zeros((n, 2), dtype=np.uint64)
        self.block_tallies = np.zeros((n, 5), dtype=np.uint64)
        self.phase = np.zeros((n, _ffi.CMP_PHASE_COUNTS), dtype=np.uint64)
        self.outside = np.zeros((n, 2), dtype=np.uint64)
        self.strata_counts = np.zeros((len(self.strata), n) + self.counts.shape[1:], dtype=np.uint64)
        self.strata_outside = np.zeros((len(self.strata), n, 2), dtype=np.uint64)
        listed = []
        for i, cid in enumerate(cids):
            if blocks:
                self.counts[i], self.tallies[i], self.block_tallies[i] = eng.cmp_counts_blocks(cid, exact, gap)
            else:
                self.counts[i], self.tallies[i] = eng.cmp_counts_diploid(cid, exact) if diploid else eng.cmp_counts(cid, exact)
            if phased:
                self.phase[i] = eng.cmp_phase_counts(cid, exact)
            marks = self._score_regions(eng, i, cid, exact, diploid, self.counts.shape[-1]) if restricted else None
            ia, ib = (slice(None), slice(None)) if marks is None else ((marks[0] & 1) != 0, (marks[1] & 1) != 0)   # --list: inside only
            if listing and diploid:
                a, _, ga, fa_flags = eng.cmp_fetch_diploid(cid, _ffi.CMP_TRUTH)
                b, _, gb, fb_flags = eng.cmp_fetch_diploid(cid, _ffi.CMP_CALLS)
                a, ga, fa_flags, b, gb, fb_flags = a[ia], ga[ia], fa_flags[ia], b[ib], gb[ib], fb_flags[ib]
                listed += record_rows_diploid(names[i], a, ga, fa_flags, b, gb, fb_flags)
                if phased:
                    listed += switch_rows(names[i], a, ga, eng.cmp_fetch_phase(cid, _ffi.CMP_TRUTH)[1])
            elif listing:
                held, _, fa_flags, fb_flags = eng.cmp_fetch(cid)
                current = eng.fetch_records(cid)[0]
                held, fa_flags, current, fb_flags = held[ia], fa_flags[ia], current[ib], fb_flags[ib]
                listed += record_rows("FN", names[i], held, fa_flags)
                listed += record_rows("FP", names[i], current, fb_flags)
                if blocks:
                    listed += record_rows("BLK", names[i], held, fa_flags, 2, "truth")
                    listed += record_rows("BLK", names[i], current, fb_flags, 2, "calls")
        self.stats = {"truth_vcf_bytes": truth[0], "calls_vcf_bytes": calls[0], "vcf_load_kernel_ms": truth[1] + calls[1],
                      "vcf_plan_kernel_ms": truth[2] + calls[2], "cmp_kernel_ms": round(eng.cmp_timing() - cmp0, 4)}
        if blocks:
            self.stats["cmp_block_kernel_ms"] = round(eng.cmp_blocks_timing() - blk0, 4)
        if diploid:
            self.stats["cmp_join_kernel_ms"] = round(eng.cmp_join_timing() - join0, 4)
        else:
            eng.vcf_release()                          # (a diploid side released its text behind its joins)
        if phased:
            self.stats["cmp_phase_kernel_ms"] = round(eng.cmp_phase_timing() - phase0, 4)
        if restricted:
            self.stats["cmp_region_kernel_ms"] = round(eng.cmp_regions_timing() - region0, 4)
            self.stats["bed_scan_s"] = round(bed_scan_s, 6)
        eng.cmp_release()
        args.outcompare.write_text(self.render(names))
        if phased:
            args.outcompare_phase.write_text(self.render_phase(names))
        if listing:
            args.outcompare_records.write_text("".join(line + "\n" for line in listed))

    def render(self, names) -> str:
        args = self._args
        tallies = self.tallies.sum(axis=0, dtype=np.uint64)

        diploid = bool(getattr(args, "diploid", False))

        def followed(sample, haplotype):
            return f"sample {sample if sample is not None else '(first)'} " + ("both haplotypes" if diploid else f"haplotype {haplotype or 1}")
        notes = [f"compare: calls {args.callsfile.name} against truth {args.truthfile.name} on "
                 f"{getattr(args, 'genome_name', args.infile.name)} ({len(names)} contigs)",
                 f"truth: {followed(getattr(args, 'truth_sample', None), getattr(args, 'truth_haplotype', None))}",
                 f"calls: {followed(getattr(args, 'sample', None), getattr(args, 'haplotype', None))}",
                 "matching: " + ("exact (positions compared literally)" if getattr(args, "exact", False)
                                 else "normalised (an indel matches any placement inside its repeat)"),
                 f"truth indels whose placements end at a window edge: {int(tallies[0])}",
                 f"truth indels whose placements end at a base outside ACGT: {int(tallies[1])}"]
        if diploid:
            notes.insert(3, "genotypes: diploid, unphased (dosage compared; a haploid 1 counts as 1/1)")
        if diploid and getattr(args, "phased", False):
            total = self.phase.sum(axis=0, dtype=np.uint64)
            notes.insert(4, f"phasing: {int(total[2])} pairs in {int(total[3])} blocks, {int(total[6])} raw switches (see {args.outcompare_phase.name})")
        blocks = bool(getattr(args, "blocks", False))
        if blocks:
            gap = getattr(args, "block_gap", None)
            t = [int(x) for x in self.block_tallies.sum(axis=0, dtype=np.uint64)]
            notes.append(f"blocks: gap {_ffi.CMP_BLOCK_GAP if gap is None else int(gap)}; {t[0]} candidates, {t[1]} replayed, {t[2]} equal, "
                         f"{t[3]} over a limit ({_ffi.CMP_BLOCK_RECORDS} records, {_ffi.CMP_BLOCK_SPAN} bases), {t[4]} holding a translocation")
        if self.regions:
            r, out = self.regions, [int(x) for x in self.outside.sum(axis=0, dtype=np.uint64)]
            notes.append(f"regions: {r.path.name}: {r.n_intervals} intervals, {r.bases} bases ({r.foreign_lines} lines on names the genome "
                         f"does not have); outside and not scored: {out[0]} truth records, {out[1]} calls records")
        text = render(notes, self.counts, names if getattr(args, "per_contig", False) else None, blocks)
        lines = []
        for k, (name, r) in enumerate(self.strata):        # genome-wide only: no per-contig blocks per stratum
            out = [int(x) for x in self.strata_outside[k].sum(axis=0, dtype=np.uint64)]
            lines.append(f"# stratum {name}: {r.path.name}: {r.n_intervals} intervals, {r.bases} bases; outside: {out[0]} truth, {out[1]} calls")
            lines += render_block(self.strata_counts[k].sum(axis=0, dtype=np.uint64), blocks)
        return text + "".join(line + "\n" for line in lines)

    def render_phase(self, names) -> str:
        """The text of ``*_ms.compare.phase.tsv``."""
        args = self._args

        def side(k, sample):
            p, u, bad = (int(x) for x in self.phase_marks[k])
            return (f"sample {sample if sample is not None else '(first)'}; records of both haplotype tables: {p} phased, {u} unphased, "
                    f"{bad} with an unreadable PS")
        notes = [f"compare --phased: calls {args.callsfile.name} against truth {args.truthfile.name} on "
                 f"{getattr(args, 'genome_name', args.infile.name)} ({len(names)} contigs)",
                 f"truth: {side(_ffi.CMP_TRUTH, getattr(args, 'truth_sample', None))}",
                 f"calls: {side(_ffi.CMP_CALLS, getattr(args, 'sample', None))}",
                 "pairs: matched heterozygous variants phased on both sides; blocks: runs of pairs in one truth and one calls phase set",
                 "switch.rate = switch.raw / assessed; switchflip.rate = (switches + flips) / assessed; "
                 "hamming.rate = hamming / pairs in blocks of two or more"]
        return render_phase(notes, self.phase, names if getattr(args, "per_contig", False) else None)

    def close(self):
        eng = self._engine
        self._engine = None
        if eng is not None and self._own_engine:
            eng.close()
