"""CPU tier of the hand-built blocks (tests/deflate_cases.py) that tests/test_gpu_deflate_blocks.py puts through the device
deflate encoder, and of the encoder's twin (tests/deflate_twin.py) that the device's output is held to.

The twin is trusted for nothing it cannot show here: every stream it writes is inflated by zlib to the bytes it was given,
parsed by the strict scanner, its three tables are complete codes, and its code lengths cost what a heap-built Huffman code
costs whenever the length limit did not bind.  The inputs of the match-free families reach their edges in the twin alone, so
they are known to be sound before a GPU sees them."""
from __future__ import annotations

import random

import pytest

import deflate_cases as dc
import deflate_twin as tw
from deflate_build import distance_symbol, length_symbol, scan, zlib_verdict

B = dc.B
FULL = 1 << 15
D_LAYOUTS_SHA256 = "6cff80773657478ad61a9a21199baf46f2f549a4d02fbfb5220baa0177440516"
G_LAYOUTS_SHA256 = "d985c0aafd2033c958615d723fe387e5f6cb49292a1739eaf1c5fe0531c7de82"


def greedy_tokens(data: bytes):
    """A trivial chooser, nothing like the kernel's: the last place the next three bytes were seen, or distance 1, whichever
    copies more; 3 bytes at least, 258 at most."""
    last, out, p, n = {}, [], 0, len(data)
    while p < n:
        best = (0, 0)
        for c in (last.get(data[p:p + 3]), p - 1 if p else None):
            if c is not None and p - c <= 32768:
                length = 0
                while length < 258 and p + length < n and data[c + length] == data[p + length]:
                    length += 1
                if length > best[0]:
                    best = (length, p - c)
        step = best[0] if best[0] >= 3 else 1
        out.append(best if best[0] >= 3 else data[p])
        for q in range(p, p + step):
            last[data[q:q + 3]] = q
        p += step
    return out


def blocks_of(data: bytes):
    return [data[a:a + B] for a in range(0, len(data), B)]


def check_stream(t, blk, tokens, name):
    for payload in {t["dyn_payload"], t["payload"]}:
        assert zlib_verdict(payload, len(blk)) == ("ok", blk), name
        s = scan(payload)
        assert s["trailing_bytes"] == 0 and s["out_len"] == len(blk) and len(s["blocks"]) == 1 and s["blocks"][0]["final"], name
    (b,) = scan(t["dyn_payload"])["blocks"]
    assert b["type"] == "dynamic"
    for key in ("ll_lengths", "d_lengths", "cl_lengths", "cl_syms", "hlit", "hdist", "hclen"):
        assert b[key] == t[key], (name, key)
    for key in ("ll_lengths", "d_lengths", "cl_lengths"):
        assert tw.kraft(t[key]) == (FULL, FULL), (name, key)
    assert max(t["ll_lengths"]) <= 15 and max(t["d_lengths"]) <= 15 and max(t["cl_lengths"]) <= 7
    assert tw.tokens_of(b, blk) == tokens, name
    assert len(t["payload"]) == min(len(blk) + 5, len(t["dyn_payload"])), name


def check_cost(freq, lens, depth, steps, limit, what):
    cost, best = sum(f * l for f, l in zip(freq, lens)), tw.huffman_cost(freq)
    assert all(bool(f) == bool(l) for f, l in zip(freq, lens)), what
    assert tw.kraft(lens) == (FULL, FULL) and max(lens) <= limit, what
    assert (steps > 0) == (depth > limit), what
    if steps == 0:
        assert cost == best and max(lens) == depth, what
    else:
        assert cost >= best and max(lens) == limit, what


@pytest.mark.parametrize("name", [c[0] for c in dc.cases()])
def test_twin_streams_of_every_case(name):
    data = {c[0]: c[1] for c in dc.cases()}[name]
    for blk in blocks_of(data):
        for tokens in (tw.literal_tokens(blk), greedy_tokens(blk)):
            t = tw.encode(tokens, len(blk), blk)
            check_stream(t, blk, tokens, name)
            check_cost(t["lfreq"], t["ll_lengths"] + [0] * (286 - t["hlit"]), t["ll_depth"], t["ll_steps"], 15, name)
            check_cost(t["dfreq"], t["d_lengths"] + [0] * (30 - t["hdist"]), t["d_depth"], t["d_steps"], 15, name)
            check_cost(t["clfreq"], t["cl_lengths"], t["cl_depth"], t["cl_steps"], 7, name)


def test_symbols_of_every_length_and_distance():
    for length in range(3, 259):
        s, eb, ev = tw.len_sym(length)
        assert (s, ev, eb) == length_symbol(length)
    for dist in range(1, 32769):
        s, eb, ev = tw.dist_sym(dist)
        assert (s, ev, eb) == distance_symbol(dist)


def test_code_lengths_cost_what_a_heap_built_huffman_code_costs():
    """20 000 seeded histograms at both limits: flat, geometric and Fibonacci-like counts, 2 to 286 (19) symbols."""
    rng = random.Random(19510)
    repaired = {7: 0, 15: 0}
    for k in range(20000):
        limit = 7 if k % 2 else 15
        size = 19 if limit == 7 else 286
        m = rng.randint(2, size)
        kind = rng.randrange(4)
        if kind == 0:
            counts = [rng.randint(1, 1000) for _ in range(m)]
        elif kind == 1:
            counts = [max(1, int(rng.uniform(1.3, 2.2) ** rng.uniform(0, min(m, 24)))) for _ in range(m)]
        elif kind == 2:
            counts, a, b = [], 1, 1
            for _ in range(m):
                counts.append(a + rng.randint(0, 2))
                a, b = b, a + b if b < 1 << 24 else b
        else:
            counts = [rng.choice((1, 1, 1, 2, 3, 65280)) for _ in range(m)]
        freq = [0] * size
        for s, c in zip(rng.sample(range(size), m), counts):
            freq[s] = c
        lens, depth, steps = tw.huff_lengths(freq, tw.rank(freq), limit)
        check_cost(freq, lens, depth, steps, limit, (k, freq))
        repaired[limit] += steps > 0
    assert repaired[7] > 2000 and repaired[15] > 500, repaired


@pytest.mark.parametrize("name", dc.match_free_names())
def test_match_free_cases_reach_their_edges_in_the_twin(name):
    (data, edge), = [(c[1], c[2]) for c in dc.cases() if c[0] == name]
    t = tw.encode(tw.literal_tokens(data), len(data), data)
    assert edge(scan(t["payload"]), t), name


def test_the_run_across_hlit_is_in_the_twins_dynamic_form():
    """The kernel stores this block of one byte; what it weighed against storing spells 1, 1 | 1, 1 as a 1 and a repeat."""
    (data,) = [c[1] for c in dc.cases() if c[0] == "g_one_byte_255"]
    t = tw.encode(tw.literal_tokens(data), 1, data)
    (b,) = scan(t["dyn_payload"])["blocks"]
    assert t["stored"] and b["cross"] == [16] and b["hlit"] == 257 and b["hdist"] == 2


def test_layouts_are_the_pinned_ones():
    layouts = dc.d_layouts()
    assert len(layouts) == 2 and layouts[0] != layouts[1]
    for lay in layouts:
        ll = [lay.get(v, 0) for v in range(256)] + [9]
        assert {l: ll[:256].count(l) for l in (6, 7, 8, 9)} == dc.D_COUNTS
        freq = [0] * 19
        for s, _ in tw.spell(ll, [1, 1]):
            freq[s] += 1
        assert {s: f for s, f in enumerate(freq) if f} == dc.D_CLFREQ
        lens, depth, steps = tw.huff_lengths(freq, tw.rank(freq), 7)
        assert (depth, steps, max(lens)) == (8, 1, 7)
        for s in dc.D_CLFREQ:                                   # the depth holds when any one count moves by one
            for delta in (-1, 1):
                moved = list(freq)
                moved[s] += delta
                if moved[s]:
                    assert tw.huff_lengths(moved, tw.rank(moved), 7)[1] >= 8, (s, delta)
    assert dc.layout_hash(layouts) == D_LAYOUTS_SHA256
    assert dc.layout_hash([dc._g_layout(True), dc._g_layout(False)]) == G_LAYOUTS_SHA256


def test_planted_blocks_are_what_their_edges_assume():
    far, copies, trap = dc.e_far()
    assert len(far) == B and sorted(d for _, d in copies) == sorted(dc.E1_DISTANCES) and 32768 in dc.E1_DISTANCES
    assert trap[1] - trap[0] == 32769 and far[trap[0]:trap[0] + 16] == far[trap[1]:trap[1] + 16]
    for b, d in copies:
        assert far[b - d:b - d + 16] == far[b:b + 16] and far[b:b + 16].islower() and d >= 193
        assert (b - d) // 256 < b // 256 and (b - d) % 255 < 253 and b % 255 in (0, 7)
    near, copies = dc.e_near()
    assert len(near) == B and [d for _, d in copies] == dc.E2_DISTANCES and dc.E2_DISTANCES[0] == 2 and dc.E2_DISTANCES[-1] == 256
    for b, d in copies:
        assert near[b - d:b - d + 16] == near[b:b + 16] and b % 256 == 0 and b // 256 <= 239 and (b - d) % 255 < 253
    block, copies = dc.f_lengths()
    assert len(block) == B and [c[0] for c in copies] == dc.F_LENGTHS and dc.F_LENGTHS[:9] == list(range(3, 12))
    assert dc.F_LENGTHS[-3:] == [227, 254, 255] and len(dc.F_LENGTHS) == 49
    for length, d, b in copies:
        assert block[b - d:b - d + length] == block[b:b + length] and block[b - d + length] != block[b + length] and b % 255 == 0
