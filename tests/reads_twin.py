"""numpy restatement of the ``reads`` mode's rule, written from its description in ``include/msim.h`` -- the placement draw,
the fragment and contig searches, the orientation of the two mates, the per-cycle error draw, the fixed-stride record -- on top
of ``fast_twin``'s Philox.  Test infrastructure: the device (``tests/test_gpu_reads.py``) and the library's own sequential
restatement (``msim_dbg_reads_render``, ``tests/test_reads_host.py``) must reproduce it byte for byte.

Integer arithmetic only; the tables (fragment thresholds, error thresholds, quality bytes) are inputs."""
from __future__ import annotations

import numpy as np

from fast_twin import U64, draw4, hi64, lo64, mulhi64

TAG_READ, TAG_RERR = 22, 23
ONE53 = 1 << 53
_CODE = np.full(256, 4, dtype=np.int64)
for _k, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _k
_LETTER = np.frombuffer(b"ACGT", dtype=np.uint8)


def digits(v: int) -> int:
    return len(str(int(v)))


class Plan:
    """What the contig lengths and the tables' sizes fix: the eligible contigs, their weights' prefix sums, the widths."""

    def __init__(self, lengths, frag_min: int, n_frag: int, n_reads: int, length: int, prefix: str):
        self.fmax = frag_min + n_frag - 1
        self.idx = [k for k, L in enumerate(lengths) if L >= self.fmax]
        if not self.idx:
            raise ValueError("no eligible contig")
        w = [lengths[k] - self.fmax + 1 for k in self.idx]
        self.prefix_w = np.array([sum(w[:k]) for k in range(len(w))], dtype=np.uint64)
        self.P = sum(w)
        self.widths = (digits(n_reads - 1), digits(self.idx[-1] + 1), digits(max(lengths[k] for k in self.idx)), digits(self.fmax))
        self.prefix = prefix.encode()
        self.name = 1 + len(self.prefix) + sum(self.widths) + 4 + 4          # '@' prefix i _ c _ s _ f _ strand / mate '\n'
        self.stride = self.name + 2 * length + 4


def place(plan: Plan, key: int, i, frag_min: int, frag_thr):
    """(eligible ordinal, 0-based start, fragment length, strand) of the reads ``i`` (uint64 array)."""
    v = draw4(key, 0, i & U64(0xFFFFFFFF), 0, TAG_READ)
    p = mulhi64(lo64(v), U64(plan.P))
    c = np.searchsorted(plan.prefix_w, p, side="right") - 1                # the last one with prefix_w[c] <= p
    s = p - plan.prefix_w[c]
    h = hi64(v)
    k = np.searchsorted(np.asarray(frag_thr, dtype=np.uint64), h >> U64(11), side="right")   # the first k with u < thr[k]
    return c.astype(np.int64), s.astype(np.int64), (frag_min + k).astype(np.int64), (h & U64(1)).astype(np.int64)


def render(contigs, key: int, n_reads: int, length: int, frag_min: int, frag_thr, err_thr, qual, prefix: str, mate: int,
           first: int, count: int) -> bytes:
    """Records [first, first + count) of ``mate`` (0, 1) over ``contigs`` (uint8 arrays, upper case) as bytes."""
    frag_thr = np.asarray(frag_thr, dtype=np.uint64)
    err_thr = np.asarray(err_thr, dtype=np.uint64).reshape(2, length)
    qual = np.asarray(qual, dtype=np.uint8).reshape(2, length)
    plan = Plan([len(x) for x in contigs], frag_min, len(frag_thr), n_reads, length, prefix)
    if count == 0:
        return b""
    i = np.arange(first, first + count, dtype=np.uint64)
    c, s, f, strand = place(plan, key, i, frag_min, frag_thr)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in contigs])]).astype(np.int64)
    genome = np.concatenate([np.asarray(x, dtype=np.uint8) for x in contigs])
    base0 = starts[np.array(plan.idx, dtype=np.int64)[c]]
    j = np.arange(length, dtype=np.int64)
    comp = (strand != mate)[:, None]
    off = np.where(comp, (s + f - 1)[:, None] - j[None, :], s[:, None] + j[None, :])
    code = _CODE[genome[base0[:, None] + off]]
    valid = code < 4
    b = np.where(comp, 3 - code, code) & 3
    # one call per two cycles: y = mate << 16 | j >> 1
    half = np.arange((length + 1) // 2, dtype=np.uint64)
    w = draw4(key, 0, (i & U64(0xFFFFFFFF))[:, None], (U64(mate) << U64(16)) | half[None, :], TAG_RERR)
    lo, hi = lo64(w), hi64(w)
    word = np.empty((count, 2 * len(half)), dtype=np.uint64)
    word[:, 0::2], word[:, 1::2] = lo, hi
    word = word[:, :length]
    sub = (word >> U64(11)) < err_thr[mate][None, :]
    alt = (b + 1 + (((word & U64(0x7FF)) * U64(3)) >> U64(11)).astype(np.int64)) & 3
    final = np.where(sub, alt, b)
    seq = np.where(valid, _LETTER[final], np.uint8(ord("N"))).astype(np.uint8)
    ql = np.where(valid, qual[mate][None, :], np.uint8(ord("!"))).astype(np.uint8)
    # the records
    rec = np.empty((count, plan.stride), dtype=np.uint8)
    at = 0
    rec[:, at] = ord("@")
    at += 1
    rec[:, at:at + len(plan.prefix)] = np.frombuffer(plan.prefix, dtype=np.uint8)
    at += len(plan.prefix)
    cnum = np.array(plan.idx, dtype=np.int64)[c] + 1
    for v, wd in zip((i.astype(np.int64), cnum, s + 1, f), plan.widths):
        pw = 10 ** np.arange(wd - 1, -1, -1, dtype=np.int64)
        rec[:, at:at + wd] = (v[:, None] // pw[None, :]) % 10 + 48
        at += wd
        rec[:, at] = ord("_")
        at += 1
    rec[:, at] = np.where(strand == 1, ord("-"), ord("+"))
    rec[:, at + 1] = ord("/")
    rec[:, at + 2] = ord("1") + mate
    rec[:, at + 3] = 10
    at += 4
    assert at == plan.name
    rec[:, at:at + length] = seq
    at += length
    rec[:, at:at + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    at += 3
    rec[:, at:at + length] = ql
    rec[:, at + length] = 10
    assert at + length + 1 == plan.stride
    return rec.tobytes()
