"""The device deflate encoder's contract from the tokens onward (csrc/bgzf.hip: k_bgzf_deflate), in integers only.

What the kernel does with a block once its parse has chosen the tokens is a pure function of those tokens: the two
histograms, the ranking, the code lengths (Moffat-Katajainen, limited by the Kraft repair), the canonical codes, the
run-length spelling of the tables, the code-length code, the choice between a dynamic and a stored block and every bit of
the payload.  This module restates all of it in plain Python.  Which matches the kernel takes is NOT restated: that choice
rests on ``__log2f`` costs, so tests read the device's own tokens back from its output (``tokens_of``) and hold everything
behind them to this twin, exactly.

A token is an int (a literal byte) or a pair (length, distance)."""
from __future__ import annotations

import heapq

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def len_sym(length: int):
    """length 3..258 -> (symbol 257..285, extra bits, extra value)."""
    if length <= 10:
        return 254 + length, 0, 0
    if length == 258:
        return 285, 0, 0
    x = length - 3
    nb = x.bit_length() - 1
    e = nb - 2
    return 265 + 4 * (nb - 3) + ((x >> e) & 3), e, x & ((1 << e) - 1)


def dist_sym(dist: int):
    """distance 1..32768 -> (symbol 0..29, extra bits, extra value)."""
    if dist <= 4:
        return dist - 1, 0, 0
    x = dist - 1
    nb = x.bit_length() - 1
    e = nb - 1
    return 2 * nb + ((x >> e) & 1), e, x & ((1 << e) - 1)


def histograms(tokens):
    """(lfreq[286], dfreq[30]): the end-of-block symbol counted once, two distance codes at least."""
    lfreq, dfreq = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, int):
            lfreq[t] += 1
        else:
            lfreq[len_sym(t[0])[0]] += 1
            dfreq[dist_sym(t[1])[0]] += 1
    lfreq[256] = 1
    if sum(1 for f in dfreq if f) < 2:
        dfreq[0] = dfreq[0] or 1
        dfreq[1] = dfreq[1] or 1
    return lfreq, dfreq


def rank(freq):
    """The symbols with a count, ascending (count, symbol)."""
    return [s for _, s in sorted((f, s) for s, f in enumerate(freq) if f)]


def huff_lengths(freq, srt, maxlen):
    """Code lengths of the symbols ``srt`` (ascending count; two at least) limited to ``maxlen`` bits, as a list indexed by
    symbol; also the depth of the unlimited tree and the number of steps the Kraft repair took."""
    m = len(srt)
    assert m >= 2
    a = [freq[s] for s in srt]
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= m or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, m - 2, m - 1
    while avbl > 0:
        while root >= 0 and a[root] == dpth:
            used += 1
            root -= 1
        while avbl > used:
            a[nxt] = dpth
            nxt -= 1
            avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    depth = a[0]                                               # (lengths do not increase along srt)
    num = [0] * 33
    for v in a:
        num[min(v, 32)] += 1
    for i in range(maxlen + 1, 33):
        num[maxlen] += num[i]
        num[i] = 0
    total = sum(num[i] << (maxlen - i) for i in range(1, maxlen + 1))
    steps = 0
    while total != 1 << maxlen:
        num[maxlen] -= 1
        for i in range(maxlen - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
        steps += 1
    lens = [0] * len(freq)
    j = m
    for l in range(1, maxlen + 1):
        for _ in range(num[l]):
            j -= 1
            lens[srt[j]] = l
    return lens, depth, steps


def canonical(lengths):
    """RFC 1951 section 3.2.2: the code of every symbol with a length (others None)."""
    cnt = [0] * 17
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    nxt, c = [0] * 17, 0
    for b in range(1, 16):
        c = (c + cnt[b - 1]) << 1
        nxt[b] = c
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lengths) -> tuple:
    """The Kraft sum of a set of code lengths as (numerator, denominator 2^15)."""
    return sum(1 << (15 - l) for l in lengths if l), 1 << 15


def huffman_cost(freq) -> int:
    """sum(count x length) of an unlimited minimum-redundancy code, built with a heap: what any Huffman code costs."""
    h = [f for f in freq if f]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        s = heapq.heappop(h) + heapq.heappop(h)
        cost += s
        heapq.heappush(h, s)
    return cost


def spell(ll, dl):
    """The run-length spelling of the HLIT + HDIST lengths as [(code-length symbol, extra value)]; runs pass from the
    literal/length table into the distance table."""
    seq = list(ll) + list(dl)
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, nb):                                      # least significant bit first
        self.acc |= v << self.n
        self.n += nb

    def code(self, c, nb):                                     # a Huffman code: most significant bit first
        self.put(int(format(c, f"0{nb}b")[::-1], 2) if nb else 0, nb)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def encode(tokens, n: int, data: bytes | None = None) -> dict:
    """What the kernel writes for a block of ``n`` bytes parsed into ``tokens``.  Keys: lfreq, dfreq; ll_lengths (HLIT of
    them), d_lengths (HDIST), cl_lengths (19); hlit, hdist, hclen; cl_syms; per table the unlimited depth and the repair's
    steps (ll_depth, ll_steps, d_..., cl_...); clfreq; header_bits, total_bits, dyn_bytes, stored; dyn_payload (always) and
    payload (the stored block instead if ``stored``: needs ``data``)."""
    lfreq, dfreq = histograms(tokens)
    ll, ll_depth, ll_steps = huff_lengths(lfreq, rank(lfreq), 15)
    dl, d_depth, d_steps = huff_lengths(dfreq, rank(dfreq), 15)
    hlit, hdist = 286, 30
    while hlit > 257 and not ll[hlit - 1]:
        hlit -= 1
    while hdist > 1 and not dl[hdist - 1]:
        hdist -= 1
    cl_syms = spell(ll[:hlit], dl[:hdist])
    clfreq = [0] * 19
    for s, _ in cl_syms:
        clfreq[s] += 1
    if sum(1 for f in clfreq if f) < 2:
        if not clfreq[0]:
            clfreq[0] = 1
        else:
            clfreq[1] = 1
    cl, cl_depth, cl_steps = huff_lengths(clfreq, rank(clfreq), 7)
    hclen = 19
    while hclen > 4 and not cl[CL_ORDER[hclen - 1]]:
        hclen -= 1
    header_bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl[s] + CL_EXTRA.get(s, 0) for s, _ in cl_syms)
    body = 0
    for t in tokens:
        if isinstance(t, int):
            body += ll[t]
        else:
            s, eb, _ = len_sym(t[0])
            body += ll[s] + eb
            s, eb, _ = dist_sym(t[1])
            body += dl[s] + eb
    total_bits = header_bits + body + ll[256]
    dyn_bytes = (total_bits + 7) // 8
    stored = dyn_bytes >= n + 5

    w = _Bits()
    w.put(1, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.put(cl[s], 3)
    cc = canonical(cl)
    for s, ext in cl_syms:
        w.code(cc[s], cl[s])
        if s >= 16:
            w.put(ext, CL_EXTRA[s])
    assert w.n == header_bits
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if isinstance(t, int):
            w.code(lc[t], ll[t])
        else:
            s, eb, ev = len_sym(t[0])
            w.code(lc[s], ll[s])
            w.put(ev, eb)
            s, eb, ev = dist_sym(t[1])
            w.code(dc[s], dl[s])
            w.put(ev, eb)
    w.code(lc[256], ll[256])
    assert w.n == total_bits
    res = dict(n=n, lfreq=lfreq, dfreq=dfreq, clfreq=clfreq, ll_lengths=ll[:hlit], d_lengths=dl[:hdist], cl_lengths=cl,
               hlit=hlit, hdist=hdist, hclen=hclen, cl_syms=cl_syms, ll_depth=ll_depth, ll_steps=ll_steps, d_depth=d_depth,
               d_steps=d_steps, cl_depth=cl_depth, cl_steps=cl_steps, header_bits=header_bits, total_bits=total_bits,
               dyn_bytes=dyn_bytes, stored=stored, dyn_payload=w.bytes())
    if not stored:
        res["payload"] = res["dyn_payload"]
    elif data is not None:
        assert len(data) == n
        res["payload"] = bytes([1, n & 0xFF, n >> 8, ~n & 0xFF, (~n >> 8) & 0xFF]) + bytes(data)
    return res


def literal_tokens(data: bytes):
    return list(data)


def tokens_of(block: dict, data: bytes):
    """The tokens of one dynamic (or fixed) block that produced all of ``data``, from ``deflate_build.scan``'s record of the
    block: its matches as (length, distance, bytes produced before), literals everywhere else."""
    out, p = [], 0
    for length, dist, pos in block["matches"]:
        assert p <= pos and 1 <= dist <= pos
        out += data[p:pos]
        out.append((length, dist))
        p = pos + length
    assert p <= len(data)
    out += data[p:]
    assert len(out) == block["n_lit"] + len(block["matches"])
    return out
