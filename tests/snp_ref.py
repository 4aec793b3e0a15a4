"""A literal restatement of the SNP ti/tv transducer (plan_kernels.h section 5), independent of libmsim: tempering and its
inverse, the three masks per word, the 3-state walk, the maps per lane and per block from each start state, the outcomes by
rank and the end position.  Plain Python over lists; numpy only for tempering whole arrays.

The draws of one SNP (mutator.py:436-446): ``random()`` takes two words, a below-``ti_lim`` sample is a transition (outcome 0);
otherwise ``randint(0, 1)`` = ``_randbelow(2)`` takes 2-bit draws -- one word each -- until one is < 2, outcome 1 + that draw.
As a transducer over TEMPERED words:

    state 0  expects the first word of random()                               -> state 1
    state 1  expects the second: A (the pair's sample < ti_lim) emits 0      -> state 0, else -> state 2
    state 2  inside randbelow(2): B (top bit clear) emits 1 + T (bit 30)      -> state 0, else stays

``tests/test_snp_ref_host.py`` holds this file against CPython's own generator; ``stream_ref.snp_draws`` is the same walk written
SNP by SNP."""
from __future__ import annotations

import numpy as np

BLOCK = 8192                  # plan_kernels.h SNP_BLOCK2
LANE = 32                     # plan_kernels.h SNP_ITEMS2
LANES = BLOCK // LANE         # plan_kernels.h SNP_THREADS
FLAG_SNP_OVERFLOW = 2         # plan_kernels.h
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ tempering
def temper(y):
    """MT19937's output tempering of raw state words (numpy uint32 array or int)."""
    y = np.asarray(y, dtype=np.uint64)
    y = y ^ (y >> 11)
    y = y ^ ((y << 7) & 0x9D2C5680)
    y = y ^ ((y << 15) & 0xEFC60000)
    y = y ^ (y >> 18)
    return (y & M32).astype(np.uint32)


def _undo_right(y, s):
    x = y
    for _ in range(32 // s + 1):
        x = y ^ (x >> s)
    return x


def _undo_left(y, s, mask):
    x = y
    for _ in range(32 // s + 1):
        x = y ^ ((x << s) & mask)
    return x


def untemper(t):
    """The raw state words whose tempered values are ``t``: how a test hands the engine words it chose."""
    y = np.asarray(t, dtype=np.uint64)
    y = _undo_right(y, 18)
    y = _undo_left(y, 15, 0xEFC60000)
    y = _undo_left(y, 7, 0x9D2C5680)
    y = _undo_right(y, 11)
    return (y & M32).astype(np.uint32)


def pair_words(u: int, low_a: int = 0, low_b: int = 0):
    """Two tempered words whose ``random()`` sample is ``u`` (53 bits): u = (a >> 5) * 2**26 + (b >> 6)."""
    assert 0 <= u < (1 << 53)
    return ((u >> 26) << 5) | (low_a & 31), ((u & ((1 << 26) - 1)) << 6) | (low_b & 63)


# ------------------------------------------------------------------------------------------------ masks
def word_bits(t, ti_lim: int):
    """Per tempered word i: A[i] (words i - 1, i as a sample are below ti_lim; 0 stands in front of word 0), B[i] (top bit
    clear), T[i] (bit 30) -- lists of 0 / 1."""
    t = [int(x) for x in t]
    A, B, T = [], [], []
    prev = 0
    for w in t:
        u = ((prev >> 5) << 26) | (w >> 6)
        A.append(1 if u < ti_lim else 0)
        B.append(1 - (w >> 31))
        T.append((w >> 30) & 1)
        prev = w
    return A, B, T


def lane_masks(bits, lane_first: int):
    """The 32-bit mask of one lane (words lane_first .. lane_first + 31) of a 0 / 1 list."""
    m = 0
    for i in range(LANE):
        m |= bits[lane_first + i] << i
    return m


# ------------------------------------------------------------------------------------------------ the walk
def walk(A, B, T, lo: int, hi: int, state: int):
    """Words [lo, hi) from ``state``: (emits, end state); emits = [(word, outcome)] in order."""
    out = []
    s = state
    for i in range(lo, hi):
        if s == 0:
            s = 1
        elif s == 1:
            if A[i]:
                out.append((i, 0))
                s = 0
            else:
                s = 2
        else:
            if B[i]:
                out.append((i, 1 + T[i]))
                s = 0
    return out, s


def span_map(A, B, T, lo: int, hi: int):
    """(c0, c1, c2, e) of words [lo, hi): emitted counts from the three start states, end states two bits each."""
    c, e = [], 0
    for s in range(3):
        out, end = walk(A, B, T, lo, hi, s)
        c.append(len(out))
        e |= end << (2 * s)
    return c[0], c[1], c[2], e


def pack_lane_map(m):
    """SnpLane.pm: three 6-bit counts and the 6 bits of end states (plan_kernels.h snp_pack_map)."""
    return (m[0] & 63) | ((m[1] & 63) << 6) | ((m[2] & 63) << 12) | ((m[3] & 63) << 18)


def block_tables(t, ti_lim: int):
    """What the map pass leaves behind for the whole blocks of ``t``: lanes (blocks, 256, 4) uint32 = A, B, T masks and packed
    map per lane, maps (blocks, 4) uint32 per block."""
    A, B, T = word_bits(t, ti_lim)
    nb = len(t) // BLOCK
    lanes = np.zeros((nb, LANES, 4), dtype=np.uint32)
    maps = np.zeros((nb, 4), dtype=np.uint32)
    for b in range(nb):
        for l in range(LANES):
            f = b * BLOCK + l * LANE
            lanes[b, l] = (lane_masks(A, f), lane_masks(B, f), lane_masks(T, f), pack_lane_map(span_map(A, B, T, f, f + LANE)))
        maps[b] = span_map(A, B, T, b * BLOCK, (b + 1) * BLOCK)
    return lanes, maps


def draws(t, ti_lim: int, start: int, K: int):
    """K SNPs' draws from word ``start`` of the whole blocks of ``t``, state 0: (outcomes as bytes, end position, flags).  Fewer
    than K complete: every outcome there is, end position = start (untouched), FLAG_SNP_OVERFLOW."""
    A, B, T = word_bits(t, ti_lim)
    out, _ = walk(A, B, T, start, (len(t) // BLOCK) * BLOCK, 0)
    if len(out) < K:
        return bytes(o for _, o in out), start, FLAG_SNP_OVERFLOW
    return bytes(o for _, o in out[:K]), out[K - 1][0] + 1, 0


def completions(t, ti_lim: int, start: int):
    """The word every SNP drawn from ``start`` completes on (state 0, to the end of the whole blocks)."""
    A, B, T = word_bits(t, ti_lim)
    return [i for i, _ in walk(A, B, T, start, (len(t) // BLOCK) * BLOCK, 0)[0]]
