"""Hand-built blocks for the device deflate encoder (csrc/bgzf.hip: k_bgzf_deflate), each with the reason it exists.

``cases()`` is a list of (name, bytes, edge).  ``edge(s, t)`` is a predicate over what came out: ``s`` is
``deflate_build.scan`` of one member's deflate data (one block) and ``t`` is ``deflate_twin.encode`` on the tokens read back
from it (literal-only tokens where the block is stored).  It states what the case is for -- the repair ran, a distance symbol
was reached -- and a case whose predicate is false on the device's output fails: the input no longer tests what it was built
to test.  A case of more than one block (family A's largest) must satisfy its predicate on every member.

The kernel's parse, for reading the constructions below: thread t owns bytes [255 t, 255 t + 255) ("span") and no match
crosses a span's end; sources are found through a hash table of 4-byte prefixes that holds, per bucket, the last position
of the 256-position tiles already walked, so a source must lie in an earlier tile than its copy and must not have been
overwritten in its bucket; the last two positions of a span are never entered under their own hash; distance 1 is tried
besides.  Shuffles and phrase letters are drawn from fixed seeds; a seed is named where it was picked so that no planted
source is overwritten in its bucket."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

from deflate_build import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, length_symbol
import deflate_twin as tw

B = 65280
SPAN, TILE = 255, 256


def _blk(s):
    (b,) = s["blocks"]
    return b


def stored(s, t):
    return _blk(s)["type"] == "stored"


def dynamic(s, t):
    return _blk(s)["type"] == "dynamic"


def stored_n_plus_5(s, t):
    return stored(s, t) and (s["end_bit"] + 7) // 8 == t["n"] + 5 and _blk(s)["stored_len"] == t["n"]


# ----------------------------------------------------------------------------------------------------------- A: sizes
A_SIZES = [1, 2, 3, 4, 5, 254, 255, 256, 257, 509, 510, 511, B - 1, B, B + 1, 2 * B - 1]


def skewed_text(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGTN\n", dtype=np.uint8)[rng.choice(6, n, p=[0.4, 0.3, 0.15, 0.1, 0.04, 0.01])].tobytes()


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _a_cases():
    out = []
    for n in A_SIZES:
        # text: a last member of 1 byte (n = B + 1) is stored like any block of at most 5 bytes
        out.append((f"a_text_{n}", skewed_text(n, 1000 + n), lambda s, t: stored(s, t) if t["n"] <= 5 else dynamic(s, t)))
        out.append((f"a_random_{n}", random_bytes(n, 2000 + n), stored_n_plus_5))
    return out


# -------------------------------------------------------------------------------------------------- B: tiny alphabets
def one_value_edge(s, t):
    """Two distance codes of one bit each and every copy at distance 1.  The tables are the twin's on the block's tokens: for
    a dynamic block the test holds the device's tables equal to them; a block of two bytes is stored (13 bytes of dynamic block
    against 7) and there they are the tables the kernel weighed against storing.  From 255 bytes on there must be a copy."""
    b = _blk(s)
    if t["hdist"] != 2 or t["d_lengths"] != [1, 1]:
        return False
    if t["n"] >= 255 and not (b["type"] == "dynamic" and b["matches"] and b["n_dist_codes"] == 2):
        return False
    return all(d == 1 for _, d, _ in b.get("matches", ()))


def period_edge(period):
    def edge(s, t):
        b = _blk(s)
        return (b["type"] == "dynamic" and len(b["matches"]) >= 255 and all(d % period == 0 for _, d, _ in b["matches"])
                and b["n_lit"] >= TILE)                        # (the first tile has no source yet)
    return edge


def _b_cases():
    out = [(f"b_one_value_{n}", b"\xa7" * n, one_value_edge) for n in (2, 255, 256, B)]
    for period, letters in ((2, b"RY"), (3, b"acg"), (4, b"\x00\xff\x80\x7f")):
        out.append((f"b_period_{period}", (letters * (B // period + 1))[:B], period_edge(period)))
    out.append(("b_two_different_bytes", b"\x00\xff", lambda s, t: stored(s, t) and t["hdist"] == 2 and t["lfreq"][0] == t["lfreq"][255] == 1))
    return out


# ------------------------------------------------------------------------------------------------ C: the 15-bit limit
C_RARE_1 = bytes(range(0x61, 0x71))                              # 16 byte values, once each: a balanced bottom of the tree
C_CHAIN_1 = [40, 70, 132, 203, 338, 545, 889, 1445, 2352, 3826, 6225, 10128, 16477]
C_RARE_2 = bytes(range(0x80, 0xA0))                              # 32 byte values, once each


def chain_counts(first, second, count, base):
    """Counts whose Huffman tree is a chain: each is ``base`` plus the sum of all before it but the previous one -- then the
    subtree below and the previous count are the two smallest -- widened by 2 % and 30 against the few length symbols and
    the lost literals of chance matches."""
    c = [first, second]
    while len(c) < count:
        c.append(int((base + sum(c[:-1])) * 1.02 + 30))
    return c


assert chain_counts(40, 70, 13, 60) == C_CHAIN_1
C_CHAIN_2 = chain_counts(50, 90, 12, 76)


def histogram_block(rare: bytes, chain_values: bytes, chain, seed: int) -> bytes:
    a = np.concatenate([np.frombuffer(rare, dtype=np.uint8)] + [np.full(c, v, dtype=np.uint8) for v, c in zip(chain_values, chain)])
    return np.random.default_rng(seed).permutation(a).tobytes()


def limit_15_edge(s, t):
    return dynamic(s, t) and t["ll_depth"] >= 16 and t["ll_steps"] > 0 and max(_blk(s)["ll_lengths"]) == 15


def _c_cases():
    out = []
    for seed in (1, 2):
        out.append((f"c_chain13_rare16_shuffle{seed}", histogram_block(C_RARE_1, b"RSYWBDHVNTGCA", C_CHAIN_1, 30 + seed), limit_15_edge))
        out.append((f"c_chain12_rare32_shuffle{seed}", histogram_block(C_RARE_2, bytes(range(0x30, 0x3C)), C_CHAIN_2, 40 + seed), limit_15_edge))
    return out


# ------------------------------------------------------------------------------------- D, G: tables from dyadic counts
def dyadic_block(lengths_of: dict, scale: int, seed: int, top: int) -> bytes:
    """Byte value v occurs scale x 2^(top - lengths_of[v]) times, shuffled: with the end-of-block symbol on the longest length
    and a Kraft sum of exactly 1 the Huffman lengths are ``lengths_of`` whatever the order."""
    a = np.concatenate([np.full(scale << (top - l), v, dtype=np.uint8) for v, l in sorted(lengths_of.items())])
    return np.random.default_rng(seed).permutation(a).tobytes()


D_CLFREQ = {18: 1, 0: 2, 1: 2, 16: 5, 17: 8, 8: 15, 7: 20, 6: 39, 9: 71}
D_COUNTS = {6: 39, 7: 20, 8: 15, 9: 89}                          # (+ end of block on 9 bits: Kraft's sum is exactly 1)


@functools.lru_cache(maxsize=None)
def d_layouts(seed: int = 20240607, count: int = 2):
    """``count`` layouts {byte value: code length} of D_COUNTS over 0..255 whose header spells with exactly D_CLFREQ: a
    code-length histogram 1, 2, 2, 5, 8, 15, 20, 39, 71 -- a chain of depth 8, one repair step down to 7 bits.  Random
    search, deterministic: nine-bit runs of 4..7 (one repeat symbol each) and of 1..3 alternate with groups of the other
    lengths and of the gaps (67, eight of 3, two of 1 zeros); a candidate counts if its spelling has the wanted histogram."""
    rng = np.random.default_rng(seed)
    found = []
    while len(found) < count:
        long_runs = [int(x) for x in rng.integers(4, 8, 5)]
        rest = 90 - sum(long_runs)
        nines = list(long_runs)
        while rest:
            k = min(rest, int(rng.integers(1, 4)))
            nines.append(k)
            rest -= k
        last = nines.pop(int(rng.integers(0, len(nines))))     # the run that ends in the end-of-block symbol
        rng.shuffle(nines)
        nines.append(last)
        others = [6] * 39 + [7] * 20 + [8] * 15 + [-67] + [-3] * 8 + [-1] * 2
        rng.shuffle(others)
        cuts = np.sort(rng.choice(np.arange(1, len(others)), len(nines) - 1, replace=False))
        seq = []
        for g, k in zip(np.split(np.array(others), cuts), nines):      # a group of the others, a run of nines, and so on
            seq += list(g) + [9] * k
        ll = []
        for v in seq:
            ll += [0] * -v if v < 0 else [int(v)]
        if len(ll) != 257 or ll[256] != 9:
            continue
        freq = {}
        for sym, _ in tw.spell(ll, [1, 1]):
            freq[sym] = freq.get(sym, 0) + 1
        if freq != D_CLFREQ:
            continue
        lay = {v: l for v, l in enumerate(ll[:256]) if l}
        if lay not in found:
            found.append(lay)
    return found


def layout_hash(layouts) -> str:
    return hashlib.sha256(repr([sorted(l.items()) for l in layouts]).encode()).hexdigest()


def limit_7_edge(s, t):
    return dynamic(s, t) and t["cl_depth"] >= 8 and t["cl_steps"] > 0 and max(_blk(s)["cl_lengths"]) == 7


def _d_cases():
    first, second = d_layouts()
    return [("d_layout1_shuffle1", dyadic_block(first, 4, 51, 9), limit_7_edge),
            ("d_layout1_shuffle2", dyadic_block(first, 4, 52, 9), limit_7_edge),
            ("d_layout2_shuffle1", dyadic_block(second, 4, 53, 9), limit_7_edge)]


# ------------------------------------------------------------------------------------------------------- E: distances
def _filler(n=B) -> bytearray:
    return bytearray((b"ACGT" * (n // 4 + 1))[:n])


def _phrase(rng, n) -> bytes:
    """n lower-case letters, no two neighbours equal."""
    out = [int(rng.integers(0, 26))]
    while len(out) < n:
        c = int(rng.integers(0, 26))
        if c != out[-1]:
            out.append(c)
    return bytes(97 + c for c in out)


class _Planter:
    """Writes phrases into the filler, refusing to touch a byte twice."""

    def __init__(self, seed):
        self.buf, self.rng, self.used = _filler(), np.random.default_rng(seed), np.zeros(B, dtype=bool)

    def free(self, at, n, margin=4):
        return 0 <= at and at + n <= B and not self.used[max(at - margin, 0):at + n + margin].any()

    def put(self, at, data, margin=4):
        assert self.free(at, len(data), margin), at
        self.buf[at:at + len(data)] = data
        self.used[at:at + len(data)] = True

    def put_twice(self, src, at, data):
        """``data`` at ``src`` and at ``at``, behind two different bytes: a 4-byte window that begins in the filler and ends
        in the phrase is then found nowhere else, and the copy begins at ``at``, not up to three bytes before it."""
        self.put(src, data)
        self.put(at, data, margin=0)
        for p, mark in ((src - 1, b"("), (at - 1, b"[")):
            if p >= 0 and not self.used[p]:
                self.put(p, mark, margin=0)


def _hashable(p):                                                # the last two positions of a span are not entered
    return p % SPAN < SPAN - 2


E1_DISTANCES = [DIST_BASE[s] + ev for s in range(15, 30) for ev in (0, (1 << DIST_EXTRA[s]) - 1)]      # 193, 256, 257 ... 32768
E2_DISTANCES = sorted({DIST_BASE[s] + ev for s in range(1, 16) for ev in (0, (1 << DIST_EXTRA[s]) - 1)})  # 2, 3, 4 ... 193, 256


@functools.lru_cache(maxsize=None)
def e_far(seed: int = 3):
    """(block, copies, trap): for every distance d of E1_DISTANCES a phrase of 16 letters at b - d and at b, b at or near a
    span start, the source in an earlier tile and under its own hash; and one phrase 32 769 bytes before its twin."""
    pl = _Planter(seed)
    trap_b = 255 * SPAN
    trap = (trap_b - 32769, trap_b)
    ph = _phrase(pl.rng, 16)
    pl.put(trap[0], ph)
    pl.put(trap[1], ph)
    copies = []
    k = 254
    for d in sorted(E1_DISTANCES, reverse=True):
        while True:
            b = k * SPAN
            if not _hashable(b - d):
                b += 7
            ok = b - d >= 0 and (b - d) // TILE < b // TILE and _hashable(b - d) and pl.free(b, 16) and pl.free(b - d, 16)
            k -= 1
            if ok:
                break
            assert k > 0
        ph = _phrase(pl.rng, 16)
        pl.put_twice(b - d, b, ph)
        copies.append((b, d))
    return bytes(pl.buf), copies, trap


def e_far_edge(s, t):
    b = _blk(s)
    _, copies, trap = e_far()
    want = {(sym, ev) for sym in range(15, 30) for ev in (0, (1 << DIST_EXTRA[sym]) - 1)}
    at = {(pos, d) for _, d, pos in b["matches"]}
    covered = np.zeros(B, dtype=bool)
    for length, _, pos in b["matches"]:
        covered[pos:pos + length] = True
    return (b["type"] == "dynamic" and want <= b["dist_syms"] and set(copies) <= at
            and any(d == 32768 for _, d, _ in b["matches"])
            and not any(pos - d == trap[0] for _, d, pos in b["matches"])
            and not covered[trap[1]:trap[1] + 4].any())          # (its second occurrence begins with literals)


@functools.lru_cache(maxsize=None)
def e_near(seed: int = 4):
    """(block, copies): for every distance d of E2_DISTANCES the second occurrence at a tile start b = 256 k (k <= 239: 16
    bytes of the span are left), the first at b - d in the tile before; below 16 the phrase is a pattern of period d.  A run of
    one letter adds distance 1."""
    pl = _Planter(seed)
    copies = []
    k = 2
    for d in E2_DISTANCES:
        while True:
            b = k * TILE
            k += 2
            if _hashable(b - d):
                break
        assert k <= 240
        if d < 16:
            unit = bytes(97 + int(c) for c in pl.rng.permutation(26)[:d])
            pl.put(b - d, (unit * 16)[:d + 16])
        else:
            ph = _phrase(pl.rng, 16)
            pl.put_twice(b - d, b, ph)
        copies.append((b, d))
    pl.put(250 * SPAN, b"n" * 24)
    return bytes(pl.buf), copies


def e_near_edge(s, t):
    b = _blk(s)
    _, copies = e_near()
    want = {(sym, ev) for sym in range(1, 16) for ev in (0, (1 << DIST_EXTRA[sym]) - 1)} | {(0, 0)}
    return (b["type"] == "dynamic" and want <= b["dist_syms"] and set(copies) <= {(pos, d) for _, d, pos in b["matches"]}
            and (23, 1, 250 * SPAN + 1) in b["matches"])


# --------------------------------------------------------------------------------------------------------- F: lengths
F_LENGTHS = sorted({LEN_BASE[k] + ev for k in range(27) for ev in (0, (1 << LEN_EXTRA[k]) - 1)} | {227, 254, 255})


@functools.lru_cache(maxsize=None)
def f_lengths(seed: int = 1):
    """(block, copies): a phrase of every length of F_LENGTHS two spans before a span start and again at it, each followed by
    its own closing byte; length 3 cannot be found by its 4-byte prefix and is a run of four that begins one byte earlier."""
    pl = _Planter(seed)
    copies = []
    for j, length in enumerate(F_LENGTHS):
        b = (4 * j + 4) * SPAN
        if length == 3:
            pl.put(b - 1, b"qqqq>")
            copies.append((3, 1, b))
            continue
        ph = _phrase(pl.rng, length)
        pl.put(b - 2 * SPAN, ph + b"<")
        pl.put(b, ph + b">")
        copies.append((length, 2 * SPAN, b))
    return bytes(pl.buf), copies


def f_lengths_edge(s, t):
    b = _blk(s)
    _, copies = f_lengths()
    want = {length_symbol(length)[:2] for length in F_LENGTHS}
    assert {sym for sym, _ in want} == set(range(257, 285))
    return b["type"] == "dynamic" and want <= b["len_syms"] and set(copies) <= set(b["matches"])


# ------------------------------------------------------------------------------------------------- G: header spelling
def _g_layout(with_255: bool):
    """16 byte values on 5 bits, 31 on 6, one on 7 beside the end-of-block symbol: with or without literal 255."""
    values = list(range(0x40, 0x6F)) + [0xFF if with_255 else 0xFE]
    return {v: (5 if i < 16 else 6 if i < 47 else 7) for i, v in enumerate(values)}


@functools.lru_cache(maxsize=None)
def g_cross_block(seed: int = 77, first: int = 1, last: int = 49, p_run: float = 0.4) -> bytes:
    """Spans ``first`` .. ``last`` behind a run: span k begins with k bytes of one phrase -- a copy from the span before, in
    distance symbol 15 -- and from its tile start 256 k on it is a run (distance 1) or a pattern of period 2 (distance 2) of
    255 - k bytes: length symbols 283 and 284, the last two of the table.  With the right mix the four code lengths on either
    side of HLIT are equal and the header spells them as one length and a repeat; the seed was picked for that."""
    rng = np.random.default_rng(seed)
    phrase = _phrase(rng, 80)
    buf = bytearray(b"Z" * (SPAN * first))
    for k in range(first, last + 1):
        seeds = (b"AB", b"BA")[int(rng.integers(0, 2))][:1 if rng.random() < p_run else 2]
        pre = (phrase[:max(k - len(seeds), 0)] + seeds)[-k:]
        buf += pre + (seeds * SPAN)[:SPAN - len(pre)]
    return bytes(buf)


G_DEEP = [1, 2, 4, 7, 12, 20, 33, 54, 88, 143, 232, 376, 609, 986, 1596]      # c[k] = c[k-1] + c[k-2] + 1: a chain of depth 15


def _g_cases():
    deep = np.concatenate([np.full(c, 0x41 + i, dtype=np.uint8) for i, c in enumerate(G_DEEP)])
    return [
        # (also the table that does not use literal 255 and goes on behind 256: HLIT above 257 needs a copy)
        ("g_run_crosses_hlit", g_cross_block(),
         lambda s, t: dynamic(s, t) and _blk(s)["cross"] == [16] and _blk(s)["hlit"] == 285 and _blk(s)["ll_lengths"][255] == 0),
        # the only run of equal lengths that can pass from a match-free literal/length table into the distance table (two
        # codes of 1 bit) is of 1s: literal 255 and the end-of-block symbol alone.  The kernel stores such a block; its
        # dynamic form is the twin's (CPU tier), on the device this is one more stored block.
        ("g_one_byte_255", b"\xff", lambda s, t: stored(s, t) and (16, 0) in t["cl_syms"] and t["ll_lengths"][255:] == [1, 1]),
        ("g_literal_255_used", dyadic_block(_g_layout(True), 4, 61, 7),
         lambda s, t: dynamic(s, t) and _blk(s)["hlit"] == 257 and _blk(s)["ll_lengths"][255] == 7),
        ("g_literal_255_unused", dyadic_block(_g_layout(False), 4, 62, 7),
         lambda s, t: dynamic(s, t) and _blk(s)["hlit"] == 257 and _blk(s)["ll_lengths"][254:256] == [7, 0]),
        ("g_hclen_19", np.random.default_rng(63).permutation(deep).tobytes(),
         lambda s, t: dynamic(s, t) and _blk(s)["hclen"] == 19 and t["ll_depth"] == 15 and t["ll_steps"] == 0),
        # without a copy the distance table is two codes of 1 bit, and length 1 is the 18th in the header's order
        ("g_hclen_18", dyadic_block(_g_layout(True), 4, 64, 7),
         lambda s, t: dynamic(s, t) and _blk(s)["hclen"] == 18 and not _blk(s)["matches"] and _blk(s)["cl_lengths"][15] == 0),
    ]


def match_free_names():
    """The cases whose edges the twin reaches on literal-only tokens: C, D and G but for the block of copies."""
    return [name for name, _, _ in cases() if name[:2] in ("c_", "d_", "g_") and name != "g_run_crosses_hlit"]


@functools.lru_cache(maxsize=None)
def cases():
    out = _a_cases() + _b_cases() + _c_cases() + _d_cases()
    out += [("e_distances_256_and_above", e_far()[0], e_far_edge), ("e_distances_below_256", e_near()[0], e_near_edge),
            ("f_lengths", f_lengths()[0], f_lengths_edge)]
    out += _g_cases()
    assert len({name for name, _, _ in out}) == len(out)
    return out
