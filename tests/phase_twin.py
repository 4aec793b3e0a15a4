"""Python restatement of ``compare --diploid --phased`` (``msim_cmp_phase_*``; include/msim.h), written from its rules on top of
``cmp_twin`` and ``dip_twin`` -- test infrastructure shared by the CPU and the GPU tier.  The device kernels and the library's
sequential restatements (``msim_dbg_cmp_phase``, ``msim_dbg_vcf_phase_word``) must agree with it exactly.

* ``phase_word``: a VCF line's phase word, from the line split into fields and subfields.
* ``partners``: the calls' record every truth record is matched with -- the i-th of a class with the i-th, as ``dip_twin.score``.
* ``tally``: the informative pairs as a list, cut into blocks by key; a block's raw switch bits as a string of 0 and 1 whose runs of
  1 are counted; (out, state bytes) as ``Engine.cmp_phase_counts`` / ``Engine.cmp_fetch_phase`` give them.
* ``table_text``, ``switch_lines``: what the command line writes of them.

A case is ``(bases, (H1, pool, H2, pool) of the truth, ... of the calls, truth words, calls words, exact)``, the words one per record
of the side's diploid table; ``small_cases`` holds the smallest shapes at which the passes' tile (TILE) and the match kernels' pass
(PASS) can still go wrong.
"""
from __future__ import annotations

import itertools
import re

import numpy as np

import cmp_twin as tw
import dip_twin as dt
from cmp_twin import Table

CONTIG = 0xFFFFFFFF
N_COUNTS = 11
HEADER = ("contig", "truth.het.phased", "calls.het.phased", "pairs", "blocks", "singletons", "assessed", "switch.raw", "switch.rate",
          "switches", "flips", "switchflip.rate", "hamming", "hamming.rate")
TYPE_NAMES = (None, "SN", "IN", "DE", "DU", "IV", "TL", "TLI")


# ---- the grammar ----------------------------------------------------------------------------------------------------------------
def phase_word(line: bytes, nf0: int, sample: int = 0):
    """(word, unreadable) of one data line (no terminator) of a file with ``nf0`` fields a line."""
    f = line.split(b"\t")
    if len(f) != nf0 or nf0 < 10 or sample >= nf0 - 9:
        return 0, False
    keys, sub = f[8].split(b":"), f[9 + sample].split(b":")
    if keys[0] != b"GT" or b"|" not in sub[0] or b"/" in sub[0]:
        return 0, False
    if b"PS" not in keys or keys.index(b"PS") >= len(sub) or sub[keys.index(b"PS")] in (b"", b"."):
        return CONTIG, False
    v = sub[keys.index(b"PS")]
    if not re.fullmatch(rb"[0-9]{1,10}", v) or not 1 <= int(v) <= 0xFFFFFFFE:
        return 0, True
    return int(v), False


# ---- the pass -------------------------------------------------------------------------------------------------------------------
def partners(bases, truth, truth_pool, calls, calls_pool, exact: bool = False):
    """Per truth record the index of its calls record, or -1."""
    bases = tw.as_bases(bases)
    classes: dict = {}
    for i, rec in enumerate(tw.fields(truth)):
        classes.setdefault(tw.class_of(bases, rec, truth_pool, exact)[0], ([], []))[0].append(i)
    for j, rec in enumerate(tw.fields(calls)):
        classes.setdefault(tw.class_of(bases, rec, calls_pool, exact)[0], ([], []))[1].append(j)
    out = [-1] * len(truth)
    for ia, ib in classes.values():
        for i, j in zip(ia, ib):
            out[i] = j
    return out


def tally(bases, truth, truth_pool, truth_gt, truth_words, calls, calls_pool, calls_gt, calls_words, exact: bool = False):
    """(out uint64[11], the truth's state bytes uint8)."""
    out = np.zeros(N_COUNTS, dtype=np.uint64)
    state = np.zeros(len(truth), dtype=np.uint8)
    out[0] = sum(1 for g, w in zip(truth_gt, truth_words) if int(g) in (1, 2) and int(w))
    out[1] = sum(1 for g, w in zip(calls_gt, calls_words) if int(g) in (1, 2) and int(w))
    da, db = dt.dosage(truth_gt), dt.dosage(calls_gt)
    pairs = []                                              # (truth record, key, orientation)
    for i, j in enumerate(partners(bases, truth, truth_pool, calls, calls_pool, exact)):
        if j < 0 or da[i] != db[j] or int(truth_gt[i]) not in (1, 2) or not int(truth_words[i]) or not int(calls_words[j]):
            continue
        pairs.append((i, (int(truth_words[i]), int(calls_words[j])), int(int(truth_gt[i]) != int(calls_gt[j]))))
    blocks = [list(g) for _, g in itertools.groupby(pairs, key=lambda p: p[1])]
    for block in blocks:
        o = [p[2] for p in block]
        bits = "0" + "".join("1" if a != b else "0" for a, b in zip(o, o[1:]))
        for (i, _, orient), bit in zip(block, bits):
            state[i] = 1 | (2 if bit == "1" else 0) | (4 if orient else 0)
        runs = [len(r) for r in re.findall("1+", bits)]
        out[6] += sum(runs)
        out[7] += sum(r % 2 for r in runs)
        out[8] += sum(r // 2 for r in runs)
        out[9] += min(sum(o), len(o) - sum(o))
        out[4] += len(block) == 1
        out[10] += len(block) if len(block) >= 2 else 0
    out[2], out[3] = len(pairs), len(blocks)
    out[5] = out[2] - out[3]
    return out, state


# ---- what the command line writes --------------------------------------------------------------------------------------------------
def ratio(n, d):
    return "NA" if int(d) == 0 else f"{int(n) / int(d):.6f}"


def row(label, out):
    v = [int(x) for x in out]
    return [label] + [str(x) for x in v[:7]] + [ratio(v[6], v[5]), str(v[7]), str(v[8]), ratio(v[7] + v[8], v[5]), str(v[9]), ratio(v[9], v[10])]


def table_text(outs, names=None):
    """The table of ``*_ms.compare.phase.tsv`` behind its comment lines: header, ALL, with ``names`` a row per contig."""
    outs = np.asarray(outs, dtype=np.uint64).reshape(-1, N_COUNTS)
    rows = [list(HEADER), row("ALL", outs.sum(axis=0, dtype=np.uint64))] + [row(n, o) for n, o in zip(names or (), outs)]
    return "".join("\t".join(r) + "\n" for r in rows)


def switch_lines(contig, truth, truth_gt, state):
    text = {1: "1|0", 2: "0|1"}
    out = []
    for r, g, s in zip(truth, truth_gt, state):
        if int(s) & 2:
            g = int(g)
            out.append("\t".join(["SW", contig, str(int(r["pos"]) + 1), TYPE_NAMES[int(r["type"])], str(int(r["stop"]) - int(r["pos"]) + 1),
                                  text[g], text[3 - g if int(s) & 4 else g]]))
    return out


# ---- building cases ---------------------------------------------------------------------------------------------------------------
class Sites:
    """Variants site by site, SNs unless said otherwise: ``add(pos, truth genotype, calls genotype, truth word, calls word)``, a
    genotype 0 (absent), 1 (``1|0``), 2 (``0|1``) or 3 (``1|1``).  ``build`` gives a case; every record at a pos gets its site's word."""

    def __init__(self, length: int, seed: int = 1):
        self.bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(seed).randint(0, 4, length)].copy()
        self.t, self.c = (Table(), Table()), (Table(), Table())
        self.tw, self.cw = {}, {}

    def add(self, pos, tg, cg, tword=CONTIG, cword=CONTIG, put=None, cput=None):
        """``put(table)`` / ``cput(table)``: how the truth's / the calls' record is written (default: an SN with aux 0 at pos)."""
        put = put or (lambda t: t.sn(pos, 0))
        cput = cput or put
        for h in (0, 1):
            if tg & (1 << h):
                put(self.t[h])
            if cg & (1 << h):
                cput(self.c[h])
        self.tw[pos], self.cw[pos] = tword, cword
        return self

    def word_at(self, pos, tword, cword):
        self.tw[pos], self.cw[pos] = tword, cword
        return self

    def build(self, exact=False):
        truth, calls = dt.side(*self.t), dt.side(*self.c)
        ua, ub = dt.join(*truth)[0], dt.join(*calls)[0]
        wa = np.array([self.tw[int(p)] for p in ua["pos"]], dtype=np.uint32)
        wb = np.array([self.cw[int(p)] for p in ub["pos"]], dtype=np.uint32)
        return self.bases, truth, calls, wa, wb, exact


def orientations(o, keys=None, between=0, seed=3, every=7):
    """Pairs with the orientations ``o`` (``keys[k]``: the k-th pair's (truth word, calls word)), ``every`` bases apart, and
    ``between`` uninformative records (a hom, an unphased het, a het the calls hold as hom, in turn) behind each pair."""
    s = Sites(every * (len(o) * (between + 1) + 2), seed)
    pos = 3
    for k, x in enumerate(o):
        ta, cb = keys[k] if keys else (CONTIG, CONTIG)
        s.add(pos, 1 + (k & 1), (1 + (k & 1)) if not x else (2 - (k & 1)), ta, cb)
        pos += every
        for q in range(between):
            kind = q % 3
            s.add(pos, (3, 1, 2)[kind], (3, 1, 3)[kind], (CONTIG, 0, CONTIG)[kind], CONTIG)
            pos += every
    return s.build()


def run_of(r: int):
    """The orientations of a lone block with one run of ``r`` raw switch bits: two pairs alike, ``r`` alternations, two alike."""
    o = [0, 0]
    for _ in range(r):
        o.append(1 - o[-1])
    return o + [o[-1]] * 2


def small_cases(TILE: int, PASS: int):
    cases = {}
    cases["no_pair"] = Sites(64).add(5, 3, 3).add(9, 1, 1, 0, CONTIG).add(13, 2, 2, CONTIG, 0).add(20, 1, 3).build()
    cases["no_records"] = Sites(16).build()
    cases["truth_empty"] = Sites(32).add(5, 0, 1).add(9, 0, 2).build()
    cases["one_pair"] = Sites(32).add(5, 1, 1).build()
    cases["one_pair_swapped"] = Sites(32).add(5, 1, 2).build()
    cases["two_pairs_one_block"] = orientations([0, 1])
    cases["two_pairs_two_blocks"] = orientations([0, 1], [(5, 9), (6, 9)])
    cases["key_change_truth"] = orientations([0, 1, 1, 0, 0], [(5, 9)] * 2 + [(6, 9)] * 3)
    cases["key_change_calls"] = orientations([0, 1, 1, 0, 0], [(5, 9)] * 3 + [(5, CONTIG)] * 2)
    cases["key_change_both"] = orientations([0, 1, 0, 1, 0, 1], [(5, 9)] * 3 + [(6, 10)] * 3)
    cases["key_returns"] = orientations([0, 0, 1, 1, 0, 0], [(5, 9)] * 2 + [(6, 9)] * 2 + [(5, 9)] * 2)
    cases["transparent_between"] = orientations([0, 1, 1, 0], between=3)
    # a het the calls hold as a hom between two pairs: flag 2, not assessed
    cases["genotype_mismatch_between"] = Sites(64).add(5, 1, 1).add(12, 1, 3).add(19, 2, 1).add(26, 2, 1).build()
    # 1|2: two records at one pos, haplotype 1's first; the calls hold them as 2|1
    cases["two_at_one_pos"] = (Sites(64).add(5, 1, 1).add(12, 1, 2, put=lambda t: t.sn(12, 0)).add(12, 2, 1, put=lambda t: t.sn(12, 1))
                               .add(19, 1, 1).add(26, 2, 2).build())
    # a deletion inside a homopolymer, the calls' copy left-aligned and on the other haplotype
    s = Sites(96, seed=4)
    s.bases[40:52] = ord("A")
    s.bases[39], s.bases[52] = ord("C"), ord("G")
    cases["shifted_indel"] = (s.add(5, 1, 1).add(47, 1, 2, put=lambda t: t.de(47, 2), cput=lambda t: t.de(40, 2)).word_at(40, CONTIG, CONTIG)
                              .add(60, 1, 1).add(70, 2, 2).build())
    cases["shifted_indel_exact"] = cases["shifted_indel"][:5] + (True,)
    s = Sites(96, seed=5)
    s.bases[30:38] = np.frombuffer(b"ACACACAC", dtype=np.uint8)
    s.bases[29], s.bases[38] = ord("G"), ord("T")
    cases["shifted_insert"] = (s.add(5, 2, 2).add(34, 2, 1, put=lambda t: t.ins(34, "AC"), cput=lambda t: t.ins(31, "CA")).word_at(31, 7, 7)
                               .add(60, 1, 1).build())
    for r in (1, 2, 3, 4, 5):
        cases[f"run_of_{r}"] = orientations(run_of(r))
    cases["all_swapped"] = orientations([1] * 9)
    # the tile's edge in the dense sequence: a switch run over pairs TILE - 2 .. TILE + 1 inside a block that starts at TILE - 4
    o = [0] * (TILE - 2) + [1, 0, 1, 0] + [0] * 3
    cases["tile_edge_run_and_block"] = orientations(o, [(5, 9)] * (TILE - 4) + [(6, 9)] * (len(o) - TILE + 4), between=1)
    for at in (TILE - 1, TILE, TILE + 1):                  # a block that starts and a run that ends at the pair of that index
        o = [0] * (at - 3) + [1, 0, 1] + [1] * 4
        cases[f"block_starts_at_{at}"] = orientations(o, [(5, 9)] * at + [(5, 10)] * (len(o) - at))
        o = [k & 1 for k in range(at + 1)] + [at & 1] * 3
        cases[f"run_ends_at_{at}"] = orientations(o)
    rs = np.random.RandomState(11)
    n = 3 * TILE + 5
    keys, key = [], (5, 9)
    for _ in range(n):
        if rs.randint(0, 40) == 0:
            key = (int(rs.randint(1, 4)), int(rs.choice([CONTIG, 8, 9])))
        keys.append(key)
    cases["random_three_tiles"] = orientations(np.cumsum(rs.randint(0, 4, n) == 0) & 1, keys, between=1)
    # two pairs with more than two tiles of uninformative records between them
    cases["long_gap"] = orientations([0, 1], between=2 * TILE + 3)
    for n in (PASS - 1, PASS, PASS + 1):
        cases[f"records_{n}"] = orientations(rs.randint(0, 2, n))
    return cases


def tables_of(case):
    """(bases, (U, pool, gt, words) of the truth, ... of the calls, exact) of a case."""
    bases, truth, calls, wa, wb, exact = case
    return bases, dt.join(*truth) + (wa,), dt.join(*calls) + (wb,), exact
