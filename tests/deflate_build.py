"""A bit-exact DEFLATE (RFC 1951) writer, an independent scanner and the zlib reference, for tests of the device inflate
(csrc/bgzf.hip: k_bgzf_inflate).

* ``Deflate`` writes stored, fixed and dynamic blocks from tokens and caller-stated code lengths.  Nothing is optimised
  and nothing is validated: an over-subscribed set, a symbol without a code's neighbour, a run of the code-length alphabet
  placed across the HLIT boundary all come out as asked.
* ``scan`` parses a stream again and reports which constructs it holds.  It shares the RFC's tables with the writer and
  nothing else (its own bit reader, its own code assignment), so tests take their coverage from what a stream contains,
  never from what the writer was asked to do.
* ``zlib_verdict`` is the reference: what zlib's inflater makes of a stream, refusals in the project's wording.
* ``replay`` expands tokens to bytes (LZ77), to hold zlib and the writer against each other.
"""
from __future__ import annotations

import zlib

# ---------------------------------------------------------------------------------------------- RFC 1951 section 3.2.5/7
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_DEFAULT = [4] * 13 + [5] * 6            # a complete code over all 19 code-length symbols (13/16 + 6/32 = 1)


class _Bits:
    def __init__(self):
        self.done, self.acc, self.n = bytearray(), 0, 0         # whole bytes; the bits behind them; bits in all

    def put(self, v, nb):                                       # LSB first (header fields, extra bits)
        self.acc |= v << (self.n - 8 * len(self.done))
        self.n += nb
        k = self.n // 8 - len(self.done)
        if k >= 8:
            self.done += (self.acc & ((1 << 8 * k) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k

    def put_bytes(self, data):                                  # (at a byte boundary)
        assert self.n % 8 == 0
        self.done += self.acc.to_bytes(self.n // 8 - len(self.done), "little") + bytes(data)
        self.acc, self.n = 0, 8 * len(self.done)

    def code(self, c, nb):                                      # a Huffman code: most significant bit first
        for k in range(nb - 1, -1, -1):
            self.put((c >> k) & 1, 1)

    def bytes(self):
        return bytes(self.done) + self.acc.to_bytes((self.n + 7) // 8 - len(self.done), "little")


def canonical_codes(lengths):
    """RFC 1951 section 3.2.2, step by step: bl_count, next_code, then codes in symbol order (None: no code)."""
    max_bits = max(lengths, default=0)
    bl_count = [0] * (max_bits + 1)
    for l in lengths:
        bl_count[l] += 1
    bl_count[0] = 0
    code, next_code = 0, [0] * (max_bits + 2)
    for bits in range(1, max_bits + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = []
    for l in lengths:
        if l:
            out.append(next_code[l])
            next_code[l] += 1
        else:
            out.append(None)
    return out


def length_symbol(length: int):
    """(symbol, extra bits' value, number of extra bits) of a match length, 258 as symbol 285."""
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k], LEN_EXTRA[k]


def distance_symbol(dist: int):
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, dist - DIST_BASE[k], DIST_EXTRA[k]


class Deflate:
    """One deflate stream, block by block.  Tokens:
      ('lit', b)                       a literal byte
      ('match', length, dist)          a back-reference; ('match', 258, dist, 284) codes length 258 as 284 + 31
      ('sym', 'l' | 'd', symbol)       the bare code of a symbol of the literal/length or distance alphabet (for illegal ones)
      ('code', value, nbits)           raw bits, most significant first (a code no symbol owns)
      ('bits', value, nbits)           raw bits, least significant first
    ``spans`` records (kind, first bit, bit after the last) of what was written, ``ops`` what ``replay`` expands."""

    def __init__(self):
        self.w = _Bits()
        self.spans = []
        self.ops = []

    def _span(self, kind, a):
        self.spans.append((kind, a, self.w.n))

    def span(self, kind, k=0):
        return [s for s in self.spans if s[0] == kind][k][1:]

    def payload(self) -> bytes:
        return self.w.bytes()

    def stored(self, data: bytes, final: bool = False, len_=None, nlen=None):
        w, a = self.w, self.w.n
        w.put(1 if final else 0, 1)
        w.put(0, 2)
        self._span("header", a)
        w.put(0, -w.n % 8)
        a = w.n
        n = len(data) if len_ is None else len_
        w.put(n, 16)
        w.put(n ^ 0xFFFF if nlen is None else nlen, 16)
        self._span("lennlen", a)
        a = w.n
        w.put_bytes(data)
        self._span("stored_data", a)
        self.ops.append(("stored", bytes(data)))
        return self

    def _tokens(self, tokens, lcodes, llens, dcodes, dlens, eob):
        w = self.w
        for t in tokens:
            a = w.n
            if t[0] == "lit":
                w.code(lcodes[t[1]], llens[t[1]])
            elif t[0] == "match":
                s, ev, eb = length_symbol(t[1]) if len(t) < 4 else (t[3], t[1] - LEN_BASE[t[3] - 257], LEN_EXTRA[t[3] - 257])
                w.code(lcodes[s], llens[s])
                b = w.n
                w.put(ev, eb)
                self._span("len_extra", b)
                s, ev, eb = distance_symbol(t[2])
                w.code(dcodes[s], dlens[s])
                b = w.n
                w.put(ev, eb)
                self._span("dist_extra", b)
            elif t[0] == "sym":
                codes, lens = (lcodes, llens) if t[1] == "l" else (dcodes, dlens)
                w.code(codes[t[2]], lens[t[2]])
            elif t[0] == "code":
                w.code(t[1], t[2])
            elif t[0] == "bits":
                w.put(t[1], t[2])
            else:
                raise ValueError(t)
            self._span("token", a)
        if eob:
            a = w.n
            w.code(lcodes[256], llens[256])
            self._span("eob", a)
        self.ops.append(("tokens", list(tokens)))

    def fixed(self, tokens, final: bool = False, eob: bool = True):
        a = self.w.n
        self.w.put(1 if final else 0, 1)
        self.w.put(1, 2)
        self._span("header", a)
        self._tokens(tokens, canonical_codes(FIXED_LITLEN), FIXED_LITLEN, canonical_codes(FIXED_DIST), FIXED_DIST, eob)
        return self

    def dynamic(self, tokens, litlen_lengths, dist_lengths, cl_symbols=None, hclen=None, final: bool = False,
                cl_lengths=None, eob: bool = True):
        """``litlen_lengths`` (HLIT of them) and ``dist_lengths`` (HDIST of them) are sent as they stand.  ``cl_symbols``
        spells them in the code-length alphabet: an int 0..15 is that length, (16 | 17 | 18, repeat) a run; by default
        one symbol per length.  ``cl_lengths``: the 19 code lengths of that alphabet (default: a complete 4/5-bit code);
        ``hclen``: how many of them are sent (default: up to the last non-zero one in the RFC's order, at least 4)."""
        w, a = self.w, self.w.n
        cl_lengths = list(CL_DEFAULT if cl_lengths is None else cl_lengths)
        if cl_symbols is None:
            cl_symbols = list(litlen_lengths) + list(dist_lengths)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lengths[s]])
        w.put(1 if final else 0, 1)
        w.put(2, 2)
        w.put(len(litlen_lengths) - 257, 5)
        w.put(len(dist_lengths) - 1, 5)
        w.put(hclen - 4, 4)
        self._span("header", a)
        a = w.n
        for s in CL_ORDER[:hclen]:
            w.put(cl_lengths[s], 3)
        self._span("hclen_lens", a)
        a = w.n
        ccodes = canonical_codes(cl_lengths)
        for c in cl_symbols:
            s, rep = (c, 0) if isinstance(c, int) else c
            w.code(ccodes[s], cl_lengths[s])
            if s == 16:
                w.put(rep - 3, 2)
            elif s == 17:
                w.put(rep - 3, 3)
            elif s == 18:
                w.put(rep - 11, 7)
        self._span("code_lens", a)
        self._tokens(tokens, canonical_codes(litlen_lengths), litlen_lengths, canonical_codes(dist_lengths), dist_lengths, eob)
        return self


def replay(ops) -> bytes:
    """The bytes a stream's stored blocks and tokens describe: the LZ77 replay, byte by byte."""
    out = bytearray()
    for kind, arg in ops:
        if kind == "stored":
            out += arg
            continue
        for t in arg:
            if t[0] == "lit":
                out.append(t[1])
            elif t[0] == "match":
                for _ in range(t[1]):
                    out.append(out[-t[2]])
            else:
                raise ValueError(f"no replay of {t!r}")
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------- the scanner
class ScanError(Exception):
    """``kind``: the project's reason for refusing such a stream."""

    def __init__(self, kind, what):
        super().__init__(what)
        self.kind = kind


class _Reader:
    def __init__(self, data):
        self.data, self.p = data, 0

    def bit(self):
        if self.p >= 8 * len(self.data):
            raise ScanError("truncated", f"out of data at bit {self.p}")
        b = (self.data[self.p >> 3] >> (self.p & 7)) & 1
        self.p += 1
        return b

    def field(self, n):                                         # an n-bit number, least significant bit first
        return sum(self.bit() << i for i in range(n))


def _code_table(lengths):
    """{(length, code): symbol}: symbols ordered by (length, symbol) get consecutive codes, shifted left whenever the length
    grows (the definition of a canonical code, not the RFC's next_code procedure)."""
    table, code, last = {}, 0, 0
    for l, s in sorted((l, s) for s, l in enumerate(lengths) if l):
        code <<= l - last
        last = l
        table[(l, code)] = s
        code += 1
    return table


def _symbol(r, table, what):
    data, p, code = r.data, r.p, 0
    for l in range(1, min(15, 8 * len(data) - p) + 1):          # (r.bit() written out: this loop is the scanner's time)
        code = code << 1 | (data[p >> 3] >> (p & 7)) & 1
        p += 1
        s = table.get((l, code))
        if s is not None:
            r.p = p
            return s, l
    if p - r.p < 15:
        r.p = p
        r.bit()
    raise ScanError("invalid code lengths" if what == "code-length" else "invalid code", f"no {what} code at bit {r.p}")


def _check_set(lengths, what, one_code_ok):
    """Kraft's sum in units of 2^-15: above 1 the set is over-subscribed, below 1 incomplete -- refused, as zlib does, unless
    it is empty or (literal/length and distance sets) a single code of one bit."""
    total = sum(1 << (15 - l) for l in lengths if l)
    if total > 1 << 15:
        raise ScanError("invalid code lengths", f"over-subscribed {what} set")
    if 0 < total < 1 << 15 and not (one_code_ok and total == 1 << 14 and sum(1 for l in lengths if l) == 1):
        raise ScanError("invalid code lengths", f"incomplete {what} set")


def _advance(r, state, n):
    state["pos"] += n
    if state["pos"] > state["limit"] and state["past_bit"] is None:
        state["past_bit"] = r.p


def _scan_block(r, blk, state):
    blk["phase"] = r.p % 8
    state["stage"] = "block header"
    blk["final"] = bool(r.bit())
    bt = blk["type"] = ("stored", "fixed", "dynamic", "reserved")[r.field(2)]
    if bt == "reserved":
        raise ScanError("bad block type", "block type 3")
    if bt == "stored":
        r.p += -r.p % 8
        state["stage"] = "LEN / NLEN"
        n, c = r.field(16), r.field(16)
        state["stage"] = "stored data"
        if n ^ c != 0xFFFF:
            raise ScanError("invalid stored block lengths", "LEN / NLEN")
        if r.p + 8 * n > 8 * len(r.data):
            raise ScanError("truncated", "stored data run out")
        blk["stored_len"] = n
        _advance(r, state, n)
        r.p += 8 * n
        return
    if bt == "fixed":
        ll, dl = FIXED_LITLEN, FIXED_DIST
    else:
        hlit, hdist, hclen = r.field(5) + 257, r.field(5) + 1, r.field(4) + 4
        blk.update(hlit=hlit, hdist=hdist, hclen=hclen)
        if hlit > 286 or hdist > 30:
            raise ScanError("invalid code lengths", "HLIT / HDIST")
        cl = [0] * 19
        state["stage"] = "HCLEN lengths"
        for s in CL_ORDER[:hclen]:
            cl[s] = r.field(3)
        _check_set(cl, "code-length", False)
        ctab = _code_table(cl)
        blk["cl_defined"], blk["cl_used"] = sorted({l for l in cl if l}), set()
        blk["cl_lengths"], blk["cl_syms"] = list(cl), []
        blk["cross"], blk["ends_on_boundary"], blk["starts_on_boundary"], blk["rep_after_zero_run"] = [], [], [], []
        lens, before = [], None
        state["stage"] = "code lengths"
        while len(lens) < hlit + hdist:
            s, l = _symbol(r, ctab, "code-length")
            blk["cl_used"].add(l)
            at = len(lens)
            if s < 16:
                lens.append(s)
                blk["cl_syms"].append((s, 0))
            else:
                if s == 16:
                    if not lens:
                        raise ScanError("invalid code lengths", "repeat without a length before it")
                    if before in (17, 18):
                        blk["rep_after_zero_run"].append(before)
                    ext = r.field(2)
                    lens += [lens[-1]] * (3 + ext)
                else:
                    ext = r.field(3) if s == 17 else r.field(7)
                    lens += [0] * (3 + ext if s == 17 else 11 + ext)
                blk["cl_syms"].append((s, ext))
                if at < hlit < len(lens):
                    blk["cross"].append(s)
                if len(lens) == hlit:
                    blk["ends_on_boundary"].append(s)
                if at == hlit:
                    blk["starts_on_boundary"].append(s)
            before = s
        if len(lens) > hlit + hdist:
            raise ScanError("invalid code lengths", "a run passes HLIT + HDIST")
        ll, dl = lens[:hlit], lens[hlit:]
        blk["ll_lengths"], blk["d_lengths"] = list(ll), list(dl)
        if not ll[256]:
            raise ScanError("invalid code lengths", "no end-of-block code")
        _check_set(ll, "literal/length", True)
        _check_set(dl, "distance", True)
    ltab, dtab = _code_table(ll), _code_table(dl)
    blk["ll_defined"], blk["d_defined"] = sorted({l for l in ll if l}), sorted({l for l in dl if l})
    blk["n_dist_codes"] = sum(1 for l in dl if l)
    blk["ll_used"], blk["d_used"], blk["n_lit"] = set(), set(), 0
    blk["matches"], blk["len_syms"], blk["dist_syms"], blk["len258_as"] = [], set(), set(), set()
    while True:
        state["stage"] = "symbols"
        s, l = _symbol(r, ltab, "literal/length")
        blk["ll_used"].add(l)
        if s == 256:
            blk["eob_end"] = r.p
            return
        if s < 256:
            blk["n_lit"] += 1
            _advance(r, state, 1)
            continue
        if s > 285:
            raise ScanError("invalid code", f"length symbol {s}")
        state["stage"] = "length extra bits"
        ev = r.field(LEN_EXTRA[s - 257])
        state["stage"] = "symbols"
        length = LEN_BASE[s - 257] + ev
        blk["len_syms"].add((s, ev))
        if length == 258:
            blk["len258_as"].add(s)
        ds, l = _symbol(r, dtab, "distance")
        blk["d_used"].add(l)
        if ds > 29:
            raise ScanError("invalid code", f"distance symbol {ds}")
        state["stage"] = "distance extra bits"
        ev = r.field(DIST_EXTRA[ds])
        dist = DIST_BASE[ds] + ev
        blk["dist_syms"].add((ds, ev))
        if dist > state["pos"]:
            raise ScanError("distance too far back", f"distance {dist} with {state['pos']} bytes produced")
        blk["matches"].append((length, dist, state["pos"]))     # (pos: bytes produced before this match)
        _advance(r, state, length)


def scan(payload: bytes, strict: bool = True, limit: int = 1 << 30) -> dict:
    """What a deflate stream holds: {'blocks': [per-block dicts], 'out_len', 'end_bit', 'trailing_bytes', 'error', 'past_bit'}.
    Per block: type, bit phase of its header, final; stored_len; hlit / hdist / hclen; of a dynamic block the three tables as
    sent (ll_lengths, d_lengths, cl_lengths) and their spelling, cl_syms: [(code-length symbol, extra value)]; the code lengths defined and used per
    alphabet (cl_ / ll_ / d_ + defined / used); the run symbols that cross the HLIT boundary, end on it or start on it;
    which zero run (17 / 18) a 16 directly followed; n_dist_codes; the matches as (length, distance, bytes produced before);
    the (symbol, extra value) pairs of both alphabets; the symbols length 258 was coded with; the bit after the
    end-of-block code.  ``strict=False``: a stream that does not parse gives what was read, the project's reason for the
    refusal as 'error', the bit it was found at as 'error_bit' and what was being read as 'stage'.  'past_bit': the bit behind the symbol (or stored block's
    lengths) that took the output past ``limit`` bytes."""
    r, state = _Reader(payload), {"pos": 0, "limit": limit, "past_bit": None, "stage": None}
    res = {"blocks": [], "error": None}
    try:
        while True:
            blk = {}
            res["blocks"].append(blk)
            _scan_block(r, blk, state)
            if blk["final"]:
                break
    except ScanError as e:
        if strict:
            raise
        res["error"], res["error_bit"], res["error_text"], res["stage"] = e.kind, r.p, str(e), state["stage"]
    res["out_len"], res["end_bit"], res["past_bit"] = state["pos"], r.p, state["past_bit"]
    res["trailing_bytes"] = len(payload) - (r.p + 7) // 8
    return res


# ----------------------------------------------------------------------------------------------------------- the reference
ZLIB_REASONS = {
    "invalid block type": "bad block type",
    "invalid stored block lengths": "invalid stored block lengths",
    "too many length or distance symbols": "invalid code lengths",
    "invalid code lengths set": "invalid code lengths",
    "invalid bit length repeat": "invalid code lengths",
    "invalid literal/lengths set": "invalid code lengths",
    "invalid distances set": "invalid code lengths",
    "invalid code -- missing end-of-block": "invalid code lengths",
    "invalid literal/length code": "invalid code",
    "invalid distance code": "invalid code",
    "invalid distance too far back": "distance too far back",
}


def zlib_verdict(payload: bytes, isize: int):
    """('ok', bytes) or ('refused', reason in the project's wording): zlib's inflater on a raw deflate stream whose member
    declares ``isize`` bytes."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error as e:
        msg = str(e).split(": ", 1)[-1]
        return "refused", ZLIB_REASONS[msg]
    if not d.eof:
        return "refused", "truncated"
    if len(out) > isize:
        return "refused", "data past ISIZE"
    if len(out) < isize:
        return "refused", "ISIZE mismatch"
    return "ok", out
