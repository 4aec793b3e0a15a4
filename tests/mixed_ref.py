"""Plain references for the device half of the SV-mix and host-chain PLAN engines (csrc/plan_kernels.h section 6), in Python
and numpy only: nothing here calls libmsim or reads its sources' tables.  Every rule cites the line of the reference program
(mutation_simulator/mutator.py, util.py) or of CPython / NumPy it restates.

All functions take TEMPERED MT19937 words -- what ``getrandbits(32)`` / ``RandomState.randint(2**32)`` return.  The device
hooks take the RAW state words (the kernels temper); ``untemper`` converts, so a test can place a tempered value exactly.

Mutation type ids as in include/msim.h: SN 1, IN 2, DE 3, DU 4, IV 5, TL 6, TLI 7."""
from __future__ import annotations

import numpy as np

SN, IN, DE, DU, IV, TL, TLI = 1, 2, 3, 4, 5, 6, 7
DROPPED = 0xFFFFFFFF                 # a chain candidate that is blocked / dropped (no Mutation.stop)
TOMBSTONE = 0x80                     # ch_aux: deleted by __fix_tl_amount -- it blocked, but is no record
REACH = 63                           # words a table entry looks ahead (acceptance >= 1/2: the host walk treats 0 as "window over")
RECORD_DTYPE = np.dtype([("pos", "<u4"), ("stop", "<u4"), ("extra", "<u4"), ("type", "u1"), ("aux", "u1"), ("rsv", "<u2")])
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------- MT19937 tempering (Matsumoto & Nishimura 1998, genrand_int32)
def temper(y):
    """y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680; y ^= (y << 15) & 0xefc60000; y ^= y >> 18.  int or uint32 array."""
    y = np.asarray(y, dtype=np.uint64) & np.uint64(M32)
    y = y ^ (y >> np.uint64(11))
    y = y ^ ((y << np.uint64(7)) & np.uint64(0x9D2C5680))
    y = y ^ ((y << np.uint64(15)) & np.uint64(0xEFC60000))
    y = y ^ (y >> np.uint64(18))
    y = (y & np.uint64(M32)).astype(np.uint32)
    return int(y) if y.ndim == 0 else y


def untemper(x):
    """The inverse of ``temper``, step by step backwards; each xorshift is undone by repeating it until the shifted-in bits run out."""
    y = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    y = y ^ (y >> np.uint64(18))                                         # 18 >= 16: once
    y = y ^ ((y << np.uint64(15)) & np.uint64(0xEFC60000))               # 15 * 2 >= 32 under the mask's zeros: once
    t = y
    for _ in range(4):                                                   # 7 bits recovered per round
        t = y ^ ((t << np.uint64(7)) & np.uint64(0x9D2C5680))
    y = t & np.uint64(M32)
    t = y
    for _ in range(2):                                                   # 11 bits per round
        t = y ^ (t >> np.uint64(11))
    y = (t & np.uint64(M32)).astype(np.uint32)
    return int(y) if y.ndim == 0 else y


# ---------------------------------------------------------------------- candidate front
def sample53(words) -> np.ndarray:
    """The integer m of NumPy's legacy random_sample, u = m / 2^53: (a >> 5) * 2^26 + (b >> 6) of words 2j, 2j+1 (randomkit.c: rk_double)."""
    w = np.asarray(words, dtype=np.uint64)
    n = len(w) // 2
    return ((w[0:2 * n:2] >> np.uint64(5)) << np.uint64(26)) | (w[1:2 * n:2] >> np.uint64(6))


def types_of(words, thresholds, types) -> np.ndarray:
    """numpy.random.choice(keys, p=chances, size=k) (mutator.py:170-174): idx = cdf.searchsorted(u, side='right'), u the 53-bit
    samples.  thresholds[j] = ceil(cdf[j] * 2^53), so cdf[j] <= u  <=>  thresholds[j] <= m, m integer."""
    thr = [int(t) for t in thresholds]
    out = np.empty(len(words) // 2, dtype=np.uint8)
    for j, m in enumerate(sample53(words).tolist()):
        idx = 0
        while idx < len(thr) and thr[idx] <= m:
            idx += 1
        out[j] = types[min(idx, len(thr) - 1)]                           # (cdf[-1] == 1.0 > u: the clamp is never needed on a real cdf)
    return out


def positions_of(bitmap, start: int, d: int) -> np.ndarray:
    """sample_with_minimum_distance (util.py:104-109): the sorted sample values s (set bits of the bitmap, offsets from
    ``start``) become start + s + d * rank."""
    v = np.flatnonzero(np.unpackbits(np.asarray(bitmap, dtype=np.uint64).view(np.uint8), bitorder="little")).astype(np.int64)
    return (start + v + d * np.arange(len(v), dtype=np.int64)).astype(np.uint32)


def compaction(cand_pos, cand_type, all_: bool = False):
    """The chain's candidates: every non-SNP (all_: every candidate), in order -- (pos, type, rank)."""
    t = np.asarray(cand_type, dtype=np.uint8)
    rank = np.arange(len(t), dtype=np.uint32) if all_ else np.flatnonzero(t != SN).astype(np.uint32)
    pos = None if cand_pos is None else np.asarray(cand_pos, dtype=np.uint32)[rank]
    return pos, t[rank], rank


# ---------------------------------------------------------------------- accept tables
def lg_rows_of(n_classes: int) -> int:
    return 0 if n_classes <= 1 else 1 if n_classes == 2 else 2 if n_classes <= 4 else 3


def class_of(width: int):
    """(shift, width) of randint(a, a + width - 1): _randbelow_with_getrandbits(width) draws getrandbits(width.bit_length())
    = word >> (32 - bits) until the value is below width (Lib/random.py)."""
    return 32 - int(width).bit_length(), int(width)


def accept_table(tempered, classes) -> np.ndarray:
    """For every start position i = 0..n of the window and every class the literal retry loop: read words i, i+1, ... until
    ``w >> shift < width``; give up after REACH words or at the window's end.  Entry = (words read << lg_rows) << vbits | value,
    0 where the loop gave up; vbits = 24 up to four classes, 23 beyond.  Shape (n + 1, 1 << lg_rows), unused rows zero."""
    w = [int(x) for x in np.asarray(tempered, dtype=np.uint32)]
    n, lg = len(w), lg_rows_of(len(classes))
    vbits = 24 if lg <= 2 else 23
    T = np.zeros((n + 1, 1 << lg), dtype=np.uint32)
    for k, (sh, width) in enumerate(classes):
        for i in range(n + 1):
            q = i
            while q < n and q - i < REACH:
                v = w[q] >> sh
                q += 1
                if v < width:
                    T[i, k] = (((q - i) << lg) << vbits) | v
                    break
    return T


def rejection_run(n_rejected: int, tail: int = 3) -> np.ndarray:
    """TEMPERED words: ``n_rejected`` words every randint class rejects (all value bits set: >= any width below 2^bits), one
    every class with at most 26 value bits accepts as value 0, then ``tail`` more of those."""
    return np.array([0xFFFFFFFF] * n_rejected + [0x2A] * (1 + tail), dtype=np.uint32)


def words_of_m(m, seed: int = 0) -> np.ndarray:
    """TEMPERED word pairs whose 53-bit sample is m: a = m >> 26 in the top 27 bits, b = m's low 26 bits in the top 26; the bits
    random_sample discards (5 of a, 6 of b) are filled at random."""
    m = np.asarray(m, dtype=np.uint64)
    rs = np.random.RandomState(seed)
    w = np.empty(2 * len(m), dtype=np.uint32)
    w[0::2] = ((m >> np.uint64(26)) << np.uint64(5)).astype(np.uint32) | rs.randint(0, 32, size=len(m)).astype(np.uint32)
    w[1::2] = ((m & np.uint64((1 << 26) - 1)) << np.uint64(6)).astype(np.uint32) | rs.randint(0, 64, size=len(m)).astype(np.uint32)
    return w


# ---------------------------------------------------------------------- boundary pass -> visit rule -> records
def boundary_and_emit(L: int, block: dict, ranges: list, np_words, sn_chained: bool = False, link: dict | None = None,
                      has_tl: bool | None = None) -> dict:
    """The reference's own sequence of steps on candidates whose positions, types and LENGTHS are given (nothing is drawn here
    but the insert bases):

    1. per drawing range, in order, the boundary pass of __get_mutations (mutator.py:184-213): ``last_mut_range = range(0)`` at
       the start of every range; a candidate inside it is deleted; otherwise it gets its stop (__get_stop_position,
       mutator.py:238-265: SN stop = start; a length of None is the IV that does not fit, :243-244; DU / DE / TL clamped to
       L - 1, :257-264; TLI falls through every branch, stop stays 0) and opens range(start, start + 1 + block) for SN / IN,
       range(start, stop + 1 + block) otherwise (:204-209) -- for a TLI that is the absolute range(start, 1 + block).
    2. __link_tls (mutator.py:267-304) with the random decisions given in ``link``: ``tombstones`` (positions __fix_tl_amount
       deletes: they blocked in step 1 but are gone now), ``pairs`` = [(tl_pos, tli_pos, coin)] in tlis order; the TLI becomes
       Mutation(TLI, tl_pos, muts[tl_pos].stop, reverse, tli_pos), reverse = not (coin == 0 or length < 2) (:313).  Without
       any TL nothing is linked (:130): a TLI keeps start = its position, stop = 0.  ``link`` may be a function
       (tls, tlis) -> that dict, called with the lists step 1 leaves.
    3. the walk of __mutate_sequence (mutator.py:332-424): positions ascending; after a DE / TL (:376), IV (:386) or DU (:398)
       ``pos = stop``, so mutations inside the span are never visited.
    4. per visited mutation a record (pos, stop, extra, type, aux): IN extra = offset of its bases in the insert pool, TLI
       extra = source start, aux = reverse | (insert_pos > 0) << 1; the record's offset in the mutated sequence = pos + the
       length change of all records before it (IN / DU + len, DE / TL - len, TLI + copied span, IV / SN 0); SNP ordinals;
       insert bases ``"ATGC"[w & 3]``, one NumPy word per base in position order (__get_insert, mutator.py:465-471:
       choice(4 letters, n) draws randint(0, 4, n), a masked 32-bit word each).

    ranges: [{"clip": range stop + 1, "pos": [...], "type": [...], "length": [...]}], positions ascending over the contig;
    "length" may be a function (type, pos) -> length, asked once per candidate that reaches __get_stop_position's randint.
    Returns the records and what the device kernels take as INPUT, derived from the same run: ch_rank / ch_stop / ch_extra /
    ch_aux (the chain's verdicts), rt rows (rec_base, clip) and visit_from per range -- by its definition, the smallest
    position of the range that the walk of step 3 can still visit given the EARLIER ranges' records (ctx.h:256-258)."""
    b = {t: int(block.get(t, 1)) for t in range(1, 8)}
    cand_pos, cand_type, stops, rng_of = [], [], [], []
    muts, tls, tlis = {}, [], []                                           # mutator.py:112-114
    rt = []
    for ri, r in enumerate(ranges):
        rt.append((len(cand_pos), int(r["clip"])))
        last = range(0)                                                    # mutator.py:184
        lengths = r["length"]
        for i, (p, t) in enumerate(zip(r["pos"], r["type"])):
            p, t = int(p), int(t)
            cand_pos.append(p); cand_type.append(t); rng_of.append(ri)
            if p in last:                                                  # :190-192
                stops.append(DROPPED)
                continue
            if t == SN:
                stop = p                                                   # :239
            elif t == TLI:
                stop = 0                                                   # (no branch: Mutation's default)
            else:
                ln = lengths(t, p) if callable(lengths) else lengths[i]    # (a callable is asked exactly where the reference draws)
                if ln is None:
                    stops.append(DROPPED)                                  # :243-244, :199-201
                    continue
                stop = p + int(ln) - 1                                     # randint(start + min - 1, start + max - 1): the draw is the input
                if t in (DU, TL, DE) and stop > L - 1:
                    stop = L - 1                                           # :257-258, :263-264
            stops.append(stop)
            muts[p] = [t, p, stop, False, 0]                               # type, start, stop, trans_reverse, trans_insert_pos
            if t in (SN, IN):
                last = range(p, p + 1 + b[t])                              # :205-206
            else:
                last = range(p, stop + 1 + b[t])                           # :208-209
                if t == TL:
                    tls.append(p)
                if t == TLI:
                    tlis.append(p)
    k = len(cand_pos)
    assert all(cand_pos[i] < cand_pos[i + 1] for i in range(k - 1)), "positions ascend over the contig"
    if has_tl is None:
        has_tl = link is not None or any(t in (TL, TLI) for t in cand_type)
    extra_of, aux_of, stop_of = {}, {}, {}
    if tls:                                                                # mutator.py:130-131
        link = (link(list(tls), list(tlis)) if callable(link) else link) or {}
        for p in link.get("tombstones", ()):                               # __fix_tl_amount, :296-303
            longer = tlis if len(tls) < len(tlis) else tls
            assert len(tls) != len(tlis) and p in longer, "only surplus entries of the longer list are deleted"
            longer.remove(p)
            del muts[p]
            aux_of[p] = TOMBSTONE
        assert len(tls) == len(tlis), "the tombstones given do not even the lists out"
        pairs = link.get("pairs", [])
        assert [q for _, q, _ in pairs] == tlis and sorted(q for q, _, _ in pairs) == sorted(tls), "pairs: every TL once, in tlis order"
        for tl_pos, tli_pos, coin in pairs:                                # :280-284
            tl_stop = muts[tl_pos][2]
            rev = not (coin == 0 or tl_stop + 1 - muts[tl_pos][1] < 2)     # :313
            muts[tli_pos] = [TLI, tl_pos, tl_stop, rev, tli_pos]
            extra_of[tli_pos], stop_of[tli_pos] = tl_pos, tl_stop
            aux_of[tli_pos] = (1 if rev else 0) | (2 if tli_pos > 0 else 0)
    else:
        for p in tlis:
            extra_of[p] = p                                                # Mutation(type=TLI, start=pos): stop 0
    # ---- the walk (mutator.py:332-424)
    np_words = np.asarray(np_words, dtype=np.uint32)
    recs, rec_off, sn_index, pool = [], [], [], []
    visit_from = [0] * len(ranges)
    at, shift, seen_range = 0, 0, -1
    for j in range(k):
        p = cand_pos[j]
        while seen_range < rng_of[j]:                                      # entering a range: what earlier ranges' spans still cover
            seen_range += 1
            visit_from[seen_range] = at
        if p not in muts or p < at:
            continue
        t, start, stop, rev, ins_pos = muts[p]
        rec = [p, stop, 0, t, 0]
        delta = 0
        if t == SN:
            sn_index.append(len(recs))
        elif t == IN:
            n = stop + 1 - p                                               # :344
            rec[2] = len(pool)
            pool.extend(b"ATGC"[int(w) & 3] for w in np_words[len(pool):len(pool) + n])
            assert len(pool) == rec[2] + n, "not enough words for the insert pool"
            delta = n
        elif t in (DE, TL):
            delta, at = -(stop - p + 1), stop + 1                          # :376 (pos = stop; pos += 1)
        elif t == IV:
            at = stop + 1                                                  # :386
        elif t == DU:
            delta, at = stop + 1 - p, stop + 1                             # :391-398
        elif t == TLI:
            rec[2], rec[4] = start, (1 if rev else 0) | (2 if ins_pos > 0 else 0)
            delta = max(0, stop + 1 - start)                               # len(sequence[start:stop + 1]), :403-404
        rec_off.append(p + shift)
        shift += delta
        recs.append(tuple(rec))
    while seen_range < len(ranges) - 1:
        seen_range += 1
        visit_from[seen_range] = at
    out_recs = np.zeros(len(recs), dtype=RECORD_DTYPE)
    for i, (p, stop, extra, t, aux) in enumerate(recs):
        out_recs[i] = (p, stop, extra, t, aux, 0)
    # ---- the kernels' inputs
    on_chain = [j for j in range(k) if sn_chained or cand_type[j] != SN]
    ch_stop = [stop_of.get(cand_pos[j], stops[j]) for j in on_chain]
    return {
        "recs": out_recs, "rec_off": np.array(rec_off, dtype=np.uint32), "sn_index": np.array(sn_index, dtype=np.uint32),
        "pool": np.array(pool, dtype=np.uint8), "n_rec": len(recs), "n_sn": len(sn_index), "pool_len": len(pool), "len_delta": shift,
        "cand_pos": np.array(cand_pos, dtype=np.uint32), "cand_type": np.array(cand_type, dtype=np.uint8),
        "ch_rank": np.array(on_chain, dtype=np.uint32), "ch_stop": np.array(ch_stop, dtype=np.uint32),
        "ch_extra": np.array([extra_of.get(cand_pos[j], 0) for j in on_chain], dtype=np.uint32) if has_tl else None,
        "ch_aux": np.array([aux_of.get(cand_pos[j], 0) for j in on_chain], dtype=np.uint8) if has_tl else None,
        "rt": rt, "visit_from": np.array(visit_from, dtype=np.uint32), "sn_chained": sn_chained,
    }
