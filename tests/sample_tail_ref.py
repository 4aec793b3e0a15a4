"""The contract of ``k_sample_tail`` (plan_kernels.h) restated in numpy / plain Python, independent of libmsim: given the words
of a sample's window, the list of its accepted draws, the accepted draws per 2048-word block (or their prefix sums), a bitmap
that already holds the first draws and the number of duplicates among them,

* the tail ROUNDS: round r consumes as many further accepted draws as round r - 1 found duplicates; a draw whose bit is set
  already is a duplicate, the first occurrence of a value wins (``random.sample``'s set path: every duplicate costs one more
  accepted draw) -- until a round finds none;
* the CUT: A accepted draws were consumed in all; the stream position is one past the window word that holds the A-th of them,
  found through the block table (the last block with fewer than A accepted draws in front of it, then the rank inside it);
* the FLAGS: bit 0 when the window does not hold the draws a round asks for (nothing else is written then), or when the cut
  lies beyond ``pos_limit`` (it is clamped to it).

``tests/test_sample_tail_ref_host.py`` holds this against ``tests/stream_ref.py`` (itself held against ``random.sample``);
``tests/test_gpu_sample_tail_tables.py`` holds the kernel against this, through ``Engine.sample_tail``.

The engine is handed RAW generator words and tempers them itself, so ``untemper`` is here too: the tables are built from the
TEMPERED words (what ``getrandbits(32)`` returns) and the engine gets ``untemper`` of them."""
from __future__ import annotations

import numpy as np

ACC_BLOCK = 2048              # plan_kernels.h ACC_BLOCK: window words per count block
TAIL_LDS_OFFS = 8192          # plan_kernels.h TAIL_LDS_OFFS: the most count blocks the kernel takes as raw counts
FLAG_SAMPLE_OVERFLOW = 1      # plan_kernels.h FLAG_SAMPLE_OVERFLOW


def temper(y):
    """MT19937's output transform of the state words ``y`` (uint32 array)."""
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def untemper(t):
    """The inverse of ``temper``: the raw words whose outputs are ``t``."""
    y = np.asarray(t, dtype=np.uint32).copy()
    y ^= y >> np.uint32(18)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    x = y.copy()
    for _ in range(5):                                   # 7 bits settle per pass
        x = y ^ ((x << np.uint32(7)) & np.uint32(0x9D2C5680))
    y = x
    x = y.copy()
    for _ in range(3):                                   # 11 bits settle per pass
        x = y ^ (x >> np.uint32(11))
    return x


def shift_of(n: int) -> int:
    """``getrandbits(n.bit_length())`` of a 32-bit word: the word shifted right by this."""
    return 32 - int(n).bit_length()


def window_tables(tempered, p0: int, W: int, n: int):
    """(acc, counts, offs) of the window words[p0, p0 + W): every accepted draw's value in order, the accepted draws per block
    of ACC_BLOCK words, and their exclusive prefix sums (len(counts) + 1 entries, the last the total)."""
    v = np.asarray(tempered[p0:p0 + W], dtype=np.uint32) >> np.uint32(shift_of(n))
    ok = v < n
    nb = (W + ACC_BLOCK - 1) // ACC_BLOCK
    padded = np.zeros(nb * ACC_BLOCK, dtype=np.uint32)
    padded[:W] = ok
    counts = padded.reshape(nb, ACC_BLOCK).sum(axis=1).astype(np.uint32)
    offs = np.zeros(nb + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(counts)
    return v[ok].astype(np.uint32), counts, offs


def bitmap_of(values, n: int):
    """(bitmap of ceil(n / 32) uint32 with the bits of ``values``, duplicates among them) -- what the first-k insert leaves."""
    bm = np.zeros((n + 31) // 32, dtype=np.uint32)
    vals = np.asarray(values, dtype=np.int64)
    np.bitwise_or.at(bm, vals >> 5, (np.uint32(1) << (vals & 31).astype(np.uint32)))
    return bm, int(len(vals) - len(np.unique(vals)))


def bitmap_values(bm):
    """The set bits of a uint32 bitmap, ascending."""
    bits = np.unpackbits(np.ascontiguousarray(bm, dtype="<u4").view(np.uint8), bitorder="little")
    return np.flatnonzero(bits)


def sample_tail(tempered, acc, offs, W: int, n: int, k: int, bitmap, state: dict, win=None, pos_limit: int = 2 ** 64 - 1):
    """The kernel's contract.  ``acc``: ALL accepted draws of the window (accepted index 0 on); ``offs``: the blocks' exclusive
    prefix sums; ``state``: pos, snp_base, flags, dups, accepted_used; ``win`` = (pos, need0, d1), the anchored form: the window
    starts at win[0] instead of state['pos'], need0 more draws are consumed already and d1 duplicates are left to replace.
    Returns (state, bitmap), both new."""
    st = {f: int(state.get(f, 0)) for f in ("pos", "snp_base", "flags", "dups", "accepted_used")}
    bm = np.array(bitmap, dtype=np.uint32, copy=True)
    offs = [int(x) for x in offs]
    total = offs[-1]
    p0 = st["pos"] if win is None else int(win[0])
    pos = k if win is None else k + int(win[1])
    need = st["dups"] if win is None else int(win[2])
    if total < pos:
        st["flags"] |= FLAG_SAMPLE_OVERFLOW
        return st, bm
    while need:
        if pos + need > total:
            st["flags"] |= FLAG_SAMPLE_OVERFLOW
            return st, bm
        d = 0
        for v in acc[pos:pos + need]:
            w, b = int(v) >> 5, np.uint32(1 << (int(v) & 31))
            if bm[w] & b:
                d += 1
            bm[w] |= b
        pos, need = pos + need, d
    A = pos
    nb = len(offs) - 1
    below = [b for b in range(nb) if offs[b] < A]
    if not below:                                        # A = 0: no draw to cut behind
        return st, bm
    b = below[-1]
    want = A - offs[b]                                   # 1-based rank inside block b
    lo, hi = b * ACC_BLOCK, min((b + 1) * ACC_BLOCK, W)
    v = np.asarray(tempered[p0 + lo:p0 + hi], dtype=np.uint32) >> np.uint32(shift_of(n))
    hits = np.flatnonzero(v < n)
    if want > len(hits):                                 # (a table that disagrees with the words: nothing is written)
        return st, bm
    cut = p0 + lo + int(hits[want - 1]) + 1
    if cut > pos_limit:
        cut = pos_limit
        st["flags"] |= FLAG_SAMPLE_OVERFLOW
    st["pos"] = st["snp_base"] = cut
    st["accepted_used"] = A
    return st, bm
