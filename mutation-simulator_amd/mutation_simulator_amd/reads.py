"""``mutation-simulator genome.fa reads (-n N | --coverage X) ...``: FASTQ reads drawn from the genome on the GPU -- the step
between a mutated genome with its truth VCF (``args`` / ``rmt``) and the scoring of a caller's VCF (``compare``).

The genome is resident (``vcf_replay.resident_genome``); a read (pair) is a pure function of (key, read index) through
Philox (include/msim.h states the rule, csrc/reads.hip renders it).  This module builds the integer tables the rule starts
from -- fragment-length thresholds, per-cycle error thresholds and quality bytes -- in Python's own arithmetic, and streams the
text through the two output channels in chunks: channel 0 writes mate 1, channel 1 mate 2, ``--bgzip`` included.

Every record of a run is ``stride`` bytes long, so read ``i`` lies at byte ``i * stride`` of its (uncompressed) file.

Limits of the rule, on purpose: a fragment always fits its contig because the start is drawn among the first
``len - fmax + 1`` positions, fmax the longest fragment of the table -- the last ``fmax - f`` starts of a contig are never drawn
for a fragment of length f < fmax; contigs shorter than fmax take no reads; the three alternative bases of a substitution come
out 683 : 683 : 682 of 2048; reads from assembly gaps come out as ``N``s (the log says how many hold nothing else).
"""
from __future__ import annotations

import math
import random
from fractions import Fraction

import numpy as np

from . import _ffi
from .vcf_replay import resident_genome

ONE53 = 1 << 53
MAX_LEN, MAX_FRAG, MAX_PREFIX, MAX_SD = _ffi.READS_MAX_LEN, _ffi.READS_MAX_FRAG, _ffi.READS_MAX_PREFIX, 511
CHUNK_BYTES = 256 << 20           # text of one render call at most
PREFIX_CHARS = frozenset("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789._-")


class ReadsError(Exception):
    """The reads cannot be drawn as asked (the message says why)."""


def key_of(seed) -> int:
    """The run's 64-bit Philox key: ``--seed S`` itself (mod 2^64), else 64 bits of Python's generator."""
    return int(seed) & (2**64 - 1) if seed is not None else random.getrandbits(64)


def fragment_table(length: int, paired: bool, mean=None, sd=None):
    """(frag_min, frag_thr): fragment length ``frag_min + k`` is drawn when the 53-bit sample lies in
    [frag_thr[k - 1], frag_thr[k]).  Single-end: the read itself.  Paired: the lengths max(LEN, M - 4 SD) .. M + 4 SD with the
    normal's mass per integer length (``math.erf``), renormalised; ``thr[k] = floor(cum_k * 2^53)``, the last one 2^53."""
    if not 1 <= length <= MAX_LEN:
        raise ReadsError(f"-l must lie in 1..{MAX_LEN}")
    if not paired:
        if mean is not None or sd is not None:
            raise ReadsError("--frag-mean and --frag-sd need --paired")
        return length, np.array([ONE53], dtype=np.uint64)
    if mean is None or sd is None:
        raise ReadsError("--paired needs --frag-mean and --frag-sd")
    mean, sd = int(mean), int(sd)
    if sd < 0 or sd > MAX_SD:
        raise ReadsError(f"--frag-sd must lie in 0..{MAX_SD}")
    if mean + 4 * sd < length:
        raise ReadsError("--frag-mean + 4 --frag-sd lies below the read length: no fragment holds a read")
    lo, hi = max(length, mean - 4 * sd), mean + 4 * sd

    def cdf(x):
        return 0.5 * (1.0 + math.erf((x - mean) / (sd * math.sqrt(2.0))))
    if sd == 0:
        mass = [1.0]
    else:
        mass = [cdf(k + 0.5) - cdf(k - 0.5) for k in range(lo, hi + 1)]
    total = math.fsum(mass)
    thr = np.zeros(len(mass), dtype=np.uint64)
    for k in range(len(mass)):
        thr[k] = min(ONE53, int(math.floor(math.fsum(mass[:k + 1]) / total * ONE53)))
    thr[-1] = ONE53
    thr = np.maximum.accumulate(thr)
    return lo, thr


def parse_error_rate(text: str):
    """``A[:B]`` -> (A, B); a single value is a flat rate.  Each lies in 0..1."""
    parts = str(text).split(":")
    if len(parts) not in (1, 2):
        raise ReadsError("--error-rate takes A or A:B")
    try:
        vals = [float(p) for p in parts]
    except ValueError:
        raise ReadsError("--error-rate takes A or A:B, two numbers") from None
    if any(not 0.0 <= v <= 1.0 for v in vals):            # (NaN fails both comparisons)
        raise ReadsError("--error-rate values lie in 0..1")
    return vals[0], vals[-1]


def error_tables(length: int, a: float, b: float):
    """(err_thr uint64[2, LEN], qual uint8[2, LEN]): the substitution probability runs linearly from ``a`` at cycle 0 to ``b`` at
    the last cycle; ``err_thr = ceil(p * 2^53)`` exactly (the double's own value), ``qual = '!' + clamp(round(-10 log10 p), 2, 41)``,
    Q41 where p is 0.  Both mates get the same ramp."""
    if not 1 <= length <= MAX_LEN:
        raise ReadsError(f"-l must lie in 1..{MAX_LEN}")
    if not (0.0 <= a <= 1.0 and 0.0 <= b <= 1.0):
        raise ReadsError("--error-rate values lie in 0..1")
    thr = np.zeros(length, dtype=np.uint64)
    qual = np.zeros(length, dtype=np.uint8)
    for j in range(length):
        p = a if length == 1 else a + (b - a) * j / (length - 1)
        p = min(1.0, max(0.0, p))
        thr[j] = min(ONE53, math.ceil(Fraction(p) * ONE53))
        q = 41 if p == 0.0 else min(41, max(2, round(-10.0 * math.log10(p))))
        qual[j] = 33 + q
    return np.stack([thr, thr]), np.stack([qual, qual])


def prefix_refusal(prefix: str):
    if len(prefix.encode("utf-8", "replace")) > MAX_PREFIX:
        return f"--prefix is at most {MAX_PREFIX} bytes long"
    if any(ch not in PREFIX_CHARS for ch in prefix):
        return "--prefix takes letters, digits and ._- only"
    return None


def eligible_bases(lengths, fmax: int) -> int:
    """G: the bases of the contigs that can hold the longest fragment."""
    return sum(int(n) for n in lengths if int(n) >= fmax)


def read_count(n, coverage, G: int, length: int, mates: int) -> int:
    """N of a run: ``-n N`` itself, or floor(X * G / (LEN * mates)) for ``--coverage X``; 1 <= N < 2^32."""
    if n is None:
        N = int(math.floor(Fraction(coverage) * G / (length * mates)))
    else:
        N = int(n)
    if not 1 <= N < 2**32:
        raise ReadsError(f"the number of reads ({N}) must lie in 1..2^32 - 1")
    return N


def tables_of(args):
    """(frag_min, frag_thr, err_thr, qual) of a parsed command line (ReadsError: a usage error)."""
    refusal = prefix_refusal(args.prefix)
    if refusal:
        raise ReadsError(refusal)
    frag_min, frag_thr = fragment_table(args.length, bool(args.paired), args.frag_mean, args.frag_sd)
    a, b = parse_error_rate(args.error_rate)
    err_thr, qual = error_tables(args.length, a, b)
    return frag_min, frag_thr, err_thr, qual


class Reads:
    """Draws the reads of one genome on the GPU and writes ``*_ms.fq`` (``*_ms_1.fq`` / ``*_ms_2.fq`` for pairs)."""

    def __init__(self, args, fasta, engine=None):
        self._args = args
        self._fasta = fasta
        self._device = getattr(args, "device", 0) or 0
        self._engine = engine
        self._own_engine = engine is None
        self.stats: dict = {}
        self.key = None
        self.n_reads = None

    def run(self):
        fa, args = self._fasta, self._args
        paired = bool(args.paired)
        mates = 2 if paired else 1
        frag_min, frag_thr, err_thr, qual = tables_of(args)                # (before anything reaches the GPU)
        fmax = frag_min + len(frag_thr) - 1
        G = eligible_bases([len(fa[i]) for i in range(len(fa))], fmax)
        if G == 0:
            raise ReadsError(f"no contig is as long as the longest fragment ({fmax} bases)")
        N = read_count(args.n_reads, args.coverage, G, args.length, mates)
        self.n_reads = N
        self.key = key_of(args.seed)
        if self._engine is None:
            self._engine = _ffi.Engine(self._device)
        eng = self._engine
        resident_genome(eng, fa, "reads")
        params = _ffi.reads_params(self.key, N, args.length, paired, frag_min, frag_thr, err_thr, qual, args.prefix)
        stride, n_eligible, _ = eng.reads_setup(params)
        ms0 = eng.reads_timing()[0]                        # (a caller's engine may have rendered before)
        outs = [args.outfastq_1, args.outfastq_2][:mates] if paired else [args.outfastq]
        files = [open(path, "wb") for path in outs]
        per_chunk = max(1, CHUNK_BYTES // stride)
        try:
            if args.bgzip:
                for m, f in enumerate(files):
                    eng.bgzf_open(m, f.fileno())
            try:
                for first in range(0, N, per_chunk):       # the mates alternate: each channel copies and writes while the other's chunk renders
                    count = min(per_chunk, N - first)
                    for m, f in enumerate(files):
                        eng.reads_render_to_file(m, first, count, f.fileno(), first * stride)
            finally:
                if args.bgzip:
                    for m in range(mates):
                        eng.bgzf_close(m)
            eng.file_wait()
        finally:
            for f in files:
                f.close()
        kernel_ms, all_n = eng.reads_timing()
        eng.reads_release()
        self.stats = {"reads": N * mates, "fastq_bytes": N * stride * mates, "reads_kernel_ms": round(kernel_ms - ms0, 4),
                      "stride": stride, "eligible_contigs": n_eligible, "all_n_reads": sum(all_n)}
        if sum(all_n) and not getattr(args, "quiet", False):
            print(f"reads: {sum(all_n)} of {N * mates} reads hold only N (drawn from gaps of the assembly)")

    def close(self):
        eng = self._engine
        self._engine = None
        if eng is not None and self._own_engine:
            eng.close()
