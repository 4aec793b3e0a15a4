"""BED files for ``compare --regions / --stratify``: the text is scanned by the library in one sequential pass
(``msim_bed_scan``, csrc/bed.cpp), everything behind it is numpy over whole arrays -- a stratification BED holds 1.5 M lines.

A BED is plain text (a name ending in ``.gz`` or ``.bgz`` is read through ``gzip``, which reads BGZF too).  The scan gives the
intervals and the RUNS of consecutive lines with one name; runs are matched to the genome's contig names -- runs on names the
genome does not have are ignored and counted (a GIAB BED names chromosomes a test genome lacks), runs of one contig may be
scattered and unsorted.  Per contig the intervals are brought into the normal form the region calls take (include/msim.h): a
stable sort by start, the running maximum of the ends, an interval's head wherever ``start > max end so far`` -- overlapping,
abutting and nested intervals merge.
"""
from __future__ import annotations

import gzip
import time
from pathlib import Path

import numpy as np

from . import _ffi


class BedError(Exception):
    """The BED cannot be used as asked (the message says why; ``BED line N: reason`` for a line of the file)."""


def read_text(path) -> bytes:
    path = Path(path)
    if path.name.endswith((".gz", ".bgz")):
        with gzip.open(path, "rb") as f:
            return f.read()
    return path.read_bytes()


def normalise(starts, ends) -> tuple:
    """Half-open intervals in any order, overlapping or not, in normal form: (starts uint32, ends uint32), sorted, with
    ``start[i] > end[i - 1]``."""
    starts, ends = np.asarray(starts, dtype=np.uint32), np.asarray(ends, dtype=np.uint32)
    if not len(starts):
        return starts.copy(), ends.copy()
    order = np.argsort(starts, kind="stable")
    s, e = starts[order], ends[order]
    reach = np.maximum.accumulate(e)                       # the largest end up to and including each interval
    head = np.ones(len(s), dtype=bool)
    head[1:] = s[1:] > reach[:-1]
    first = np.flatnonzero(head)
    last = np.append(first[1:], len(s)) - 1                # a merged interval ends at the reach of its last member
    return s[first].copy(), reach[last].copy()


class Regions:
    """One BED file on one genome: ``sets[i]`` -- (starts, ends) in normal form of contig i --, the interval count and the bases
    covered after merging, the lines on names the genome does not have, the seconds the scan took."""

    def __init__(self, path, names, lengths):
        self.path = Path(path)
        text = np.frombuffer(read_text(self.path), dtype=np.uint8)
        t0 = time.perf_counter()
        try:
            starts, ends, lines, name_off, name_len, first, count = _ffi.bed_scan(text)
        except _ffi.MsimError as e:
            if getattr(e, "code", None) != _ffi.ERR_VALUE:
                raise
            raise BedError(f"{self.path.name}: " + str(e).split(": ", 1)[-1]) from None
        self.scan_s = time.perf_counter() - t0
        by_name = {}
        for i, name in enumerate(names):
            by_name.setdefault(name.encode("utf-8", "replace"), i)
        owner = np.full(len(starts), -1, dtype=np.int64)   # the contig of every interval (-1: a name the genome does not have)
        self.foreign_lines = 0
        for k in range(len(first)):
            off, f, n = int(name_off[k]), int(first[k]), int(count[k])
            i = by_name.get(text[off:off + int(name_len[k])].tobytes())
            if i is None:
                self.foreign_lines += n
            else:
                owner[f:f + n] = i
        known = owner >= 0
        beyond = known & (ends.astype(np.int64) > np.asarray(lengths, dtype=np.int64)[np.where(known, owner, 0)])
        if beyond.any():
            raise BedError(f"{self.path.name}: BED line {int(lines[np.flatnonzero(beyond)[0]])}: end beyond the contig's last base")
        order = np.argsort(owner, kind="stable")           # (file order is kept inside a contig)
        bounds = np.searchsorted(owner[order], np.arange(len(names) + 1))
        self.sets = []
        for i in range(len(names)):
            pick = order[bounds[i]:bounds[i + 1]]
            self.sets.append(normalise(starts[pick], ends[pick]))
        self.n_intervals = sum(len(s) for s, _ in self.sets)
        self.bases = sum(int((e.astype(np.int64) - s.astype(np.int64)).sum()) for s, e in self.sets)
