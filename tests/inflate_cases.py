"""The hand-built deflate streams the device inflate (csrc/bgzf.hip: k_bgzf_inflate) is held to: constructs that are legal
(or illegal) by RFC 1951 but that neither zlib's encoder nor the project's own ever writes.  ``accepted()`` and ``refused()``
give the case tables; tests/test_deflate_build_host.py holds every stream to zlib and asserts from ``deflate_build.scan``
that each holds the construct it is named for, tests/test_gpu_inflate_streams.py runs them through the kernel.

Where a defect sits in a block's header no sound stream can follow it; such cases (and all others of k..m, o, p) are
followed by at least 16 bytes -- sound symbols where the code still exists, filler bits where it does not -- so that the
refusal is never the kernel's catch-all "truncated"."""
from __future__ import annotations

import functools
import random
import zlib

from deflate_build import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, Deflate, replay
from mutation_simulator_amd.bgzf import make_member

SEED = 20
N_RANDOM = 300


def rnd(n: int, seed: int) -> bytes:
    return random.Random(seed).randbytes(n)


def complete(symbols) -> dict:
    """A Kraft-complete flat code over ``symbols``: lengths m - 1 and m, 2^m >= len(symbols) (one symbol: length 1)."""
    k = len(symbols)
    if k == 1:
        return {symbols[0]: 1}
    m = (k - 1).bit_length()
    short = (1 << m) - k
    return {s: (m - 1 if i < short else m) for i, s in enumerate(symbols)}


def table(n: int, assign: dict) -> list:
    out = [0] * n
    for s, l in assign.items():
        out[s] = l
    return out


def spell(lengths, rng=None, runs=None, allowed=(16, 17, 18)):
    """``lengths`` in the code-length alphabet.  ``runs`` {index: (symbol, repeat)}: those runs and one symbol per length
    elsewhere.  Otherwise runs wherever they fit: the longest (18, 17, 16 in that order) without ``rng``, a random choice of
    symbol and repeat count with it."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v = lengths[i]
        if runs is not None:
            if i in runs:
                s, rep = runs[i]
                assert all(x == (lengths[i - 1] if s == 16 else 0) for x in lengths[i:i + rep]) and i + rep <= n, (i, s, rep)
                out.append((s, rep))
                i += rep
            else:
                out.append(v)
                i += 1
            continue
        run = 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        opts = []
        if v == 0 and run >= 11 and 18 in allowed:
            opts.append((18, 11, min(run, 138)))
        if v == 0 and run >= 3 and 17 in allowed:
            opts.append((17, 3, min(run, 10)))
        if i > 0 and lengths[i - 1] == v and run >= 3 and 16 in allowed:
            opts.append((16, 3, min(run, 6)))
        if not opts or (rng is not None and rng.random() < 0.2):
            out.append(v)
            i += 1
            continue
        s, lo, hi = opts[0] if rng is None else rng.choice(opts)
        rep = hi if rng is None else rng.randint(lo, hi)
        out.append((s, rep))
        i += rep
    return out


def lits(text: bytes):
    return [("lit", b) for b in text]


LL5 = complete([97, 98, 99, 100, 256])      # 'a'..'d' and end-of-block: 2, 2, 2, 3, 3
LL8 = complete([97, 98, 99, 100, 256, 257, 258, 259])           # and lengths 3, 4, 5: eight codes of 3 bits


# ------------------------------------------------------------------------------------------------------------- accepted
def _a_cases(out):
    # 18-run over lit/len 260..285 and distance 0..5
    ll, dl = table(286, LL8), [0, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    toks = lits(b"abcdabcdabcdd") + [("match", 4, 9), ("match", 5, 13), ("match", 3, 12), ("match", 5, 16)]
    out["a_run18_across_boundary"] = Deflate().dynamic(toks, ll, dl, spell(ll + dl, runs={260: (18, 32)}), final=True)
    out["a_run_ends_on_and_run_starts_on_boundary"] = Deflate().dynamic(
        toks, ll, dl, spell(ll + dl, runs={260: (18, 26), 286: (17, 6)}), final=True)
    # 17-run over lit/len 260..262 and distance 0..3
    ll, dl = table(263, LL8), [0, 0, 0, 0, 1, 1]
    toks = lits(b"abcdabcd") + [("match", 3, 5), ("match", 4, 6), ("match", 5, 7), ("match", 3, 8)]
    out["a_run17_across_boundary"] = Deflate().dynamic(toks, ll, dl, spell(ll + dl, runs={260: (17, 7)}), final=True)
    # 16-run copying length 3 of lit/len 255 into 256, 257 and distance 0..2
    ll, dl = table(258, {s: 3 for s in (97, 98, 99, 100, 101, 255, 256, 257)}), [3] * 8
    toks = lits(b"abcde\xffedcba\xffabcdea") + [("match", 3, d) for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16)]
    out["a_run16_across_boundary"] = Deflate().dynamic(toks, ll, dl, spell(ll + dl, runs={256: (16, 5)}), final=True)


def _b_cases(out):
    ll, dl = table(258, complete([97, 98, 99, 100, 256, 257])), [1, 1]
    toks = lits(b"abcdabcd") + [("match", 3, 1), ("match", 3, 2)]
    for name, runs in (("b_16_after_18", {101: (18, 138), 239: (16, 6), 245: (18, 11)}),
                       ("b_16_after_17", {101: (17, 10), 111: (16, 6), 117: (18, 138)})):
        out[name] = Deflate().dynamic(toks, ll, dl, spell(ll + dl, runs=runs), final=True)


COMB = list(range(1, 16)) + [15]            # 1, 2, ..., 14, 15, 15: a complete code over 16 symbols


def _c_cases(out):
    syms = list(range(65, 75)) + [256, 257, 264, 265, 284, 285]
    toks = lits(bytes(range(65, 75))) + [("match", 3, 1), ("match", 10, 2), ("match", 12, 1), ("match", 257, 2), ("match", 258, 1)]
    for name, lens in (("c_litlen_comb_long_codes_on_low_symbols", COMB[::-1]), ("c_litlen_comb_long_codes_on_high_symbols", COMB)):
        ll = table(286, dict(zip(syms, lens)))
        out[name] = Deflate().dynamic(toks, ll, [1, 1], spell(ll + [1, 1]), final=True)
    ll = table(258, {0: 1, 256: 2, 257: 2})
    for name, dsyms, lens in (("c_dist_comb_long_codes_on_low_symbols", range(16), COMB[::-1]),
                              ("c_dist_comb_long_codes_on_high_symbols", range(14, 30), COMB)):
        dl = table(max(dsyms) + 1, dict(zip(dsyms, lens)))
        toks = [("lit", 0)] + [("match", 3, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1) for s in dsyms]
        out[name] = Deflate().stored(rnd(32768, 31)).dynamic(toks, ll, dl, spell(ll + dl), final=True)
    # a code-length code of the full 7 bits, every one of its eight codes used
    cl = table(19, dict(zip((0, 18, 4, 2, 3, 17, 16, 1), COMB[:6] + [7, 7])))
    ll = table(260, {97: 1, 98: 2, 99: 3, 256: 4, 259: 4})
    runs = {0: (18, 97), 100: (18, 138), 238: (17, 8), 246: (16, 3), 249: (16, 6)}
    out["c_code_length_code_of_7_bits"] = Deflate().dynamic(lits(b"abcabc") + [("match", 5, 1), ("match", 5, 2)], ll, [1, 1],
                                                            spell(ll + [1, 1], runs=runs), cl_lengths=cl, final=True)
    ll, dl = [8] * 226 + [9] * 60, [4, 4] + [5] * 28
    toks = lits(bytes(range(0, 256, 5))) + [("match", LEN_BASE[k], 7 * k + 1) for k in range(29)] + \
        [("match", 3, DIST_BASE[s]) for s in range(18)]
    out["c_hlit_286_hdist_30_hclen_19"] = Deflate().stored(rnd(300, 32)).dynamic(toks, ll, dl, final=True)
    # the smallest HCLEN of a valid block: 16, 17, 18, 0 alone cannot give symbol 256 a length, 8 is the fifth
    cl = table(19, {16: 2, 18: 2, 0: 2, 8: 2})
    ll = table(257, {s: 8 for s in list(range(255)) + [256]})
    out["c_smallest_hclen"] = Deflate().dynamic(lits(bytes(range(255))), ll, [0], spell(ll + [0], allowed=(16, 18)),
                                                cl_lengths=cl, final=True)


def _d_cases(out):
    ll = table(258, complete([97, 98, 256, 257]))
    out["d_one_distance_code"] = Deflate().dynamic(lits(b"ab") + [("match", 3, 1), ("lit", 97), ("match", 3, 1)], ll, [1], final=True)
    out["d_no_distance_code"] = Deflate().dynamic(lits(b"abba"), ll, [0], final=True)
    out["d_two_distance_codes"] = Deflate().dynamic(lits(b"ab") + [("match", 3, 1), ("match", 3, 2)], ll, [1, 1], final=True)
    out["d_fixed_distance_symbols_0_and_29"] = Deflate().stored(rnd(32768, 41)).fixed(
        [("match", 3, 1), ("match", 3, 32768), ("match", 4, 24577)], final=True)


def _e_cases(out):
    toks = []
    for k in range(29):
        for ev in sorted({0, (1 << LEN_EXTRA[k]) - 1}):
            length = LEN_BASE[k] + ev
            toks.append(("match", length, 40 + 9 * len(toks)) + ((284,) if (k, length) == (27, 258) else ()))
    out["e_every_length_symbol"] = Deflate().stored(rnd(600, 51)).fixed(toks, final=True)
    toks = [("match", 3, 32768)]                                # (32 768 bytes produced so far: reaches byte 0)
    for s in range(30):
        for ev in sorted({0, (1 << DIST_EXTRA[s]) - 1}):
            toks.append(("match", 3 + s % 4, DIST_BASE[s] + ev))
    toks += [("match", 3, 32507), ("match", 258, 32767), ("match", 258, 32768, 284)]
    out["e_every_distance_symbol"] = Deflate().stored(rnd(32768, 52)).fixed(toks, final=True)
    out["e_distance_reaches_byte_0"] = Deflate().fixed(lits(b"xyz") + [("match", 3, 3), ("match", 258, 6), ("match", 4, 264)], final=True)


F_DISTS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 259, 319, 320, 321]
F_LENS = [3, 4, 63, 64, 65, 66, 127, 128, 129, 257, 258]


def _f_cases(out):
    # before the matches of one distance: that many fresh random bytes, so what they copy has no shorter period
    d = Deflate().stored(rnd(400, 60))
    for k, dist in enumerate(F_DISTS):
        d.stored(rnd(dist, 61 + k))
        d.fixed([("match", length, dist) for length in F_LENS], final=dist == F_DISTS[-1])
    out["f_copy_forms"] = d


G_SIZES = [0, 1, 63, 64, 65, 4097]


def _g_cases(out):
    for phase in range(8):
        head = lits(bytes(200 + i for i in range((phase - 2) % 8))) + lits(b"GATTACA")   # 9-bit literals move the phase
        for n in G_SIZES:
            out[f"g_stored_{n}_at_phase_{phase}"] = Deflate().fixed(head).stored(rnd(n, 70 + n)).fixed(
                [("match", 6, n + 3), ("match", 258, n + 9)], final=True)
    out["g_two_stored_blocks_in_a_row"] = Deflate().fixed(lits(b"GATTACA")).stored(rnd(5, 81)).stored(rnd(7, 82)).fixed(
        [("match", 15, 17)], final=True)
    out["g_stored_first_and_final"] = Deflate().stored(rnd(10, 83)).fixed([("match", 4, 10)]).stored(rnd(3, 84), final=True)


def _h_cases(out):
    for nine in range(8):                                       # bits: 10 + 9 * nine + 8 * eight
        for eight in range(1, 5):
            out[f"h_tail_{nine}_{eight}"] = Deflate().fixed(lits(bytes(200 + i for i in range(nine))) + lits(b"ACGT"[:eight]), final=True)


def _i_cases(out):
    d = Deflate()
    for _ in range(64):
        d.fixed([])
    out["i_64_empty_fixed_blocks"] = d.fixed(lits(b"after the empty blocks"), final=True)
    out["i_empty_dynamic_block"] = Deflate().fixed(lits(b"before")).dynamic([], table(257, {97: 1, 256: 1}), [0]).fixed(
        lits(b"behind") + [("match", 6, 12)], final=True)
    out["i_empty_dynamic_block_of_one_code"] = Deflate().fixed(lits(b"before")).dynamic([], table(257, {256: 1}), [0]).fixed(
        lits(b"behind") + [("match", 6, 12)], final=True)
    out["i_isize_1"] = Deflate().fixed(lits(b"N"), final=True)
    # 65 536 = 1 + 254 * 258 + 3: a literal and 255 matches, 254 of them of 258
    out["i_isize_65536"] = Deflate().fixed(lits(b"N") + [("match", 258, 1)] * 254 + [("match", 3, 1)], final=True)


def random_kraft(rng, n: int, cap: int = 15) -> list:
    """n code lengths of a complete code: leaves of a binary tree grown by splitting random leaves, deep ones more often."""
    if n == 1:
        return [1]
    leaves = [1, 1]
    while len(leaves) < n:
        cand = [i for i, d in enumerate(leaves) if d < cap]
        i = max(rng.sample(cand, min(3, len(cand))), key=leaves.__getitem__) if rng.random() < 0.7 else rng.choice(cand)
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    rng.shuffle(leaves)
    return leaves


def random_member(rng) -> Deflate:
    d, pos = Deflate(), 0
    nblocks = rng.randint(1, 4)
    for b in range(nblocks):
        final = b == nblocks - 1
        kind = rng.choice(("stored", "fixed", "dynamic", "dynamic", "dynamic"))
        if kind == "stored":
            n = 33000 if b == 0 and rng.random() < 0.3 else rng.randint(0, 300)
            d.stored(rng.randbytes(n), final)
            pos += n
            continue
        if kind == "fixed":
            lsyms = rng.sample(range(256), rng.randint(1, 40))
            lsym_l, dsyms = rng.sample(range(257, 286), rng.randint(0, 8)), list(range(30))
        else:
            lsyms = rng.sample(range(256), rng.randint(1, 60))
            lsym_l = rng.sample(range(257, 286), rng.randint(0, 8))
            dsyms = rng.sample(range(30), rng.randint(1, 8)) if lsym_l and rng.random() < 0.9 else []
        toks = []
        for s in lsyms + lsym_l + [rng.choice(lsyms + lsym_l) for _ in range(rng.randint(0, 30))]:
            if s < 256:
                toks.append(("lit", s))
                pos += 1
                continue
            ok = [x for x in dsyms if DIST_BASE[x] <= pos]
            if not ok or pos > 60000:
                continue
            x = rng.choice(ok)
            dist = min(pos, DIST_BASE[x] + rng.randrange(1 << DIST_EXTRA[x]))
            ev = rng.choice((0, (1 << LEN_EXTRA[s - 257]) - 1, rng.randrange(1 << LEN_EXTRA[s - 257])))
            length = LEN_BASE[s - 257] + ev
            toks.append(("match", length, dist) + ((284,) if s == 284 and length == 258 else ()))
            pos += length
        if kind == "fixed":
            d.fixed(toks, final)
            continue
        coded = sorted(lsyms + lsym_l + [256])
        ll = table(rng.randint(max(coded[-1] + 1, 257), 286), dict(zip(coded, random_kraft(rng, len(coded)))))
        dl = table(rng.randint(max(dsyms, default=0) + 1, 30), dict(zip(sorted(dsyms), random_kraft(rng, len(dsyms))))) if dsyms \
            else [0] * rng.randint(1, 4)
        d.dynamic(toks, ll, dl, spell(ll + dl, rng=rng), final=final)
    return d


def _j_cases(out):
    rng = random.Random(SEED)
    for k in range(N_RANDOM):
        out[f"j_random_{k:03d}"] = random_member(rng)


@functools.lru_cache(maxsize=None)
def accepted() -> dict:
    """{name: (deflate payload, the bytes its tokens describe)}; the last one carries bytes behind its final block."""
    built = {}
    for f in (_a_cases, _b_cases, _c_cases, _d_cases, _e_cases, _f_cases, _g_cases, _h_cases, _i_cases, _j_cases):
        f(built)
    out = {name: (d.payload(), replay(d.ops)) for name, d in built.items()}
    d = Deflate().fixed(lits(b"final block, then bytes that belong to nothing"), final=True)
    out["r_bytes_behind_the_final_block"] = (d.payload() + b"\x00\xff\x55", replay(d.ops))
    return out


# -------------------------------------------------------------------------------------------------------------- refused
FILLER = [("bits", 0xA5, 8)] * 20
TAIL = lits(b"sound symbols follow")


def _k_cases(out):
    def dyn(ll, dl, isize=8, toks=FILLER, **kw):
        return Deflate().dynamic(toks, ll, dl, final=True, eob=False, **kw).payload(), isize, "invalid code lengths"
    ok_ll = table(257, LL5)
    out["k_litlen_oversubscribed"] = dyn(table(257, {97: 1, 98: 1, 256: 1}), [1, 1])
    out["k_litlen_incomplete"] = dyn(table(257, {97: 2, 256: 2}), [1, 1])
    out["k_dist_incomplete_two_2bit_codes"] = dyn(ok_ll, [2, 2])
    out["k_dist_single_code_of_length_2"] = dyn(ok_ll, [2])
    zeros = [0] * 259
    out["k_code_length_set_incomplete"] = dyn(ok_ll, [1, 1], cl_symbols=zeros, cl_lengths=table(19, {0: 2, 2: 2, 18: 2}))
    out["k_code_length_set_of_one_code"] = dyn(ok_ll, [1, 1], cl_symbols=zeros, cl_lengths=table(19, {0: 1}))
    out["k_16_as_first_symbol"] = dyn(ok_ll, [1, 1], cl_symbols=[(16, 3)] + spell((ok_ll + [1, 1])[3:]))
    ll = table(270, LL5)
    out["k_run_passes_hlit_hdist_by_one"] = dyn(ll, [1, 1, 0, 0, 0], cl_symbols=spell(ll + [1, 1]) + [(17, 4)])
    out["k_no_code_for_256"] = dyn(table(257, {97: 1, 98: 1}), [1, 1])
    out["k_hlit_287"] = dyn(table(287, LL5), [1, 1])
    out["k_hlit_288"] = dyn(table(288, LL5), [1, 1])
    out["k_hdist_31"] = dyn(ok_ll, [1, 1] + [0] * 29)
    out["k_hdist_32"] = dyn(ok_ll, [1, 1] + [0] * 30)
    out["k_hclen_4_leaves_256_without_a_code"] = dyn([0] * 257, [0], cl_symbols=[(18, 138), (18, 120)],
                                                     cl_lengths=table(19, {0: 1, 18: 1}), hclen=4)


def _l_cases(out):
    for s in (286, 287):
        out[f"l_fixed_litlen_symbol_{s}"] = Deflate().fixed(lits(b"ab") + [("sym", "l", s)] + TAIL, final=True).payload(), 40, "invalid code"
    for s in (30, 31):
        out[f"l_fixed_distance_symbol_{s}"] = Deflate().fixed(lits(b"ab") + [("sym", "l", 257), ("sym", "d", s)] + TAIL,
                                                              final=True).payload(), 40, "invalid code"
    ll = table(258, complete([97, 98] + sorted(set(b"sound symbols follow") - {97, 98}) + [256, 257]))
    out["l_unassigned_code_of_a_single_code_distance_set"] = Deflate().dynamic(
        lits(b"ab") + [("match", 3, 1), ("sym", "l", 257), ("code", 1, 1)] + TAIL + TAIL, ll, [1], final=True).payload(), 60, "invalid code"
    out["l_match_in_a_block_without_distance_codes"] = Deflate().dynamic(
        lits(b"ab") + [("sym", "l", 257)] + TAIL + TAIL, ll, [0], final=True).payload(), 60, "invalid code"


def _m_cases(out):
    for nine in (0, 3):
        head = lits(bytes(200 + i for i in range(nine))) + lits(b"GATTACA")
        d = Deflate().fixed(head).stored(rnd(20, 90), nlen=20 ^ 0xFFFE).fixed(TAIL, final=True)
        out[f"m_len_nlen_mismatch_at_phase_{(2 + nine) % 8}"] = d.payload(), 60, "invalid stored block lengths"


def _cut(build, kind, k=0):
    """``build(pad)`` with the first pad (that many 9-bit literals ahead of the dynamic block) that puts a byte boundary inside span ``kind``
    number k, cut at that boundary: (payload, isize, reason)."""
    for pad in range(8):
        d = build(pad)
        a, b = d.span(kind, k)
        c = a // 8 + 1                                          # the first byte boundary strictly after bit a
        if 8 * c < b:
            return d.payload()[:c], len(replay(d.ops)), "truncated"
    raise AssertionError(kind)


def _n_cases(out):
    ll = table(286, complete(sorted(set(b"GATTACA")) + [256, 284]))
    dl = table(30, {28: 1, 29: 1})

    def build(pad):
        return (Deflate().stored(rnd(20000, 95)).fixed(lits(bytes(200 + i for i in range(pad))))
                .dynamic(lits(b"GATTACA") + [("match", 240, 19000), ("match", 250, 30000 - 10000)] + lits(b"TAGA"), ll, dl)
                .fixed(lits(b"the end"), final=True))
    out["n_cut_in_block_header"] = _cut(build, "header", 2)
    out["n_cut_in_hclen_lengths"] = _cut(build, "hclen_lens")
    out["n_cut_in_code_lengths"] = _cut(build, "code_lens")
    out["n_cut_in_symbols"] = _cut(build, "token", -17)         # (the dynamic block's fourth literal)
    out["n_cut_in_length_extra_bits"] = _cut(build, "len_extra")
    out["n_cut_in_distance_extra_bits"] = _cut(build, "dist_extra")
    out["n_cut_in_len_nlen"] = _cut(build, "lennlen")
    out["n_cut_in_stored_data"] = _cut(build, "stored_data")
    for pad in range(8):                                        # the end-of-block code's last bit alone in the last byte
        d = build(pad)
        if d.w.n % 8 == 1:
            out["n_cut_one_bit_before_the_end_of_block_code_ends"] = d.payload()[:-1], len(replay(d.ops)), "truncated"
    out["n_no_payload_at_all"] = b"", 5, "truncated"


def _o_cases(out):
    out["o_distance_produced_plus_1_in_first_block"] = Deflate().fixed(
        lits(b"GATTA") + [("match", 3, 6)] + TAIL, final=True).payload(), 40, "distance too far back"
    out["o_distance_produced_plus_1_behind_stored_block"] = Deflate().stored(rnd(10, 96)).fixed(
        [("match", 3, 11)] + TAIL, final=True).payload(), 40, "distance too far back"


def _p_cases(out):
    """(payload, the bytes up to ISIZE, reason): these members carry the CRC32 of what they hold up to ISIZE."""
    d = Deflate().fixed(lits(b"GATTACA") + [("lit", 33)] + TAIL, final=True)
    out["p_literal_at_isize"] = d.payload(), replay(d.ops)[:7], "data past ISIZE"
    d = Deflate().fixed(lits(b"GATTACA") + [("match", 5, 7)] + TAIL, final=True)
    out["p_match_ends_one_past_isize"] = d.payload(), replay(d.ops)[:11], "data past ISIZE"
    d = Deflate().fixed(lits(b"GATTACA")).stored(rnd(30, 97), final=True)
    out["p_stored_block_one_byte_too_long"] = d.payload(), replay(d.ops)[:36], "data past ISIZE"


@functools.lru_cache(maxsize=None)
def refused() -> dict:
    """{name: (deflate payload, the ISIZE bytes the member declares, reason)}."""
    out = {}
    for f in (_k_cases, _l_cases, _m_cases, _n_cases, _o_cases, _p_cases):
        f(out)
    return {name: (p, b"\0" * blk if isinstance(blk, int) else blk, why) for name, (p, blk, why) in out.items()}


# ---------------------------------------------------------------------------------------------------------------- files
def sound_member(text: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return make_member(text, c.compress(text) + c.flush())


SOUND_A = b"GATTACA" * 300 + b"a sound member ahead of the broken one\n"
SOUND_B = b">chr1\n" + b"ACGTTGCANN" * 500 + b"\nand one behind it\n"
