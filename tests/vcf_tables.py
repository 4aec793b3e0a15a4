"""Hand-built record tables for the VCF renderers (csrc/text_gpu.hip: k_vcf_lines / k_vcf_plain; csrc/render.cpp), as pure
functions: every generator returns ``{case id: (bases, recs, pool, names, gt)}`` -- the contig, the record table and insert
pool, the sequence names to render it under and the genotype bytes of the genotyped render (1, 2, 3 cycling by record).
``tests/test_vcf_ref_host.py`` (no GPU: host renderer, coverage) and ``tests/test_gpu_vcf_tables.py`` use the same tables; the
expected text of both is ``tests/vcf_ref.py``.

The coverage helpers at the end describe what a table exercises as a function of the EXPECTED text alone (where a copy
lands, which part of it is 16-byte aligned in the text, which lines share 4096 bytes), so they are checked without a GPU.
"""
from __future__ import annotations

import functools

import numpy as np

import vcf_ref
from apply_ref import DE, DU, IN, IV, SN, TL, TLI
from mutation_simulator_amd._ffi import RECORD_DTYPE
from test_gpu_apply_tables import Table

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODES = np.frombuffer(b"KSYMWRBDHVUUN-X", dtype=np.uint8)        # ambiguity codes, U (complement only), N, '-', an untouched byte
INLINE = 25                                                       # text_gpu.hip: VCF_INLINE (copies up to it stay in the stage)
STAGE = 4096                                                      # text_gpu.hip: VCF_STAGE
GRID_LENGTHS = [1, 15, 16, 17, 24, 25, 26, 27, 30, 31, 32, 33, 41, 47, 48, 49, 64, 257]
GRID_KINDS = ["IN", "DE", "TL", "IV", "DU", "TLI_fwd", "TLI_rev"]
NAME_EDGES = [1, 63, 64, 65, 1023, 1024, 1025]                    # lname's 64 bytes; VCF_MAX_NAME: 1024 last staged, 1025 first plain
SIZES = [1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 2047, 2048, 2049]
TYPE_OF = {"SN": SN, "IN": IN, "DE": DE, "DU": DU, "IV": IV, "TL": TL}


def genome(L, seed, codes_every=3):
    """Random ACGT with a code of CODES about every ``codes_every`` bases (0: none): raw, converted and reverse-complemented
    copies of any span of a few bases differ.  Long contigs repeat a block of 1 Mb."""
    rs = np.random.RandomState(seed)
    n = min(L, 1 << 20)
    b = ACGT[rs.randint(0, 4, n)].copy()
    if codes_every and n:
        at = np.unique(rs.randint(0, n, n // codes_every))
        b[at] = CODES[rs.randint(0, len(CODES), len(at))]
    return b if n == L else np.resize(b, L)


def name_of(n):
    return ("chr" + "n" * n)[:n] if n < 3 else ("chr" + "0123456789" * (n // 10 + 1))[:n]


def finish(tab, names):
    bases, recs, pool = tab.done()
    return bases, recs, pool, [name_of(n) if isinstance(n, int) else n for n in names], (np.arange(len(recs)) % 3 + 1).astype(np.uint8)


def add(tab, kind, pos, n=1, sr=None, aux=0):
    """One record of ``kind`` at ``pos`` with a copy source of ``n`` bases; ``sr``: the source's index mod 16 for the kinds
    whose source is not the position (the insert's pool offset, a TLI's span start)."""
    if kind == "SN":
        if tab.bases[pos] not in ACGT:
            tab.bases[pos] = ACGT[pos % 4]                            # (an SNP on N, '-', U or X is a suppressed line)
        return tab.add(SN, pos, aux=aux)
    if kind == "IN":
        return tab.add(IN, pos, n, pool_mod=sr)
    if kind.startswith("TLI"):
        room = (getattr(tab, "span_hi", len(tab.bases)) - n) // 16 - 1
        start = 16 * int(tab.rs.randint(0, max(room, 1))) + (sr if sr is not None else int(tab.rs.randint(0, 16))) if room > 0 else 0
        return tab.add(TLI, pos, span=(start, n), aux=1 if kind == "TLI_rev" else 0)
    return tab.add(TYPE_OF[kind], pos, n)


# ------------------------------------------------------------------------------ a. copy geometry grid
def grid():
    """Every copy kind x GRID_LENGTHS x source residue 0..15, under 16 names of consecutive lengths.  A DE / TL REF holds the
    anchor base, so its copy length n is a span of n - 1 bases and length 1 does not exist.
    A copy of the table's line i moves by (i + 1) x (name length) in the text, through all 16 residues when i is even: an SNP
    behind each source residue's 124 records makes a (kind, length)'s sixteen records alternate between even and odd lines."""
    tab = Table(genome(260_000, 11), seed=5)
    tab.at = tab.span_hi = 4096                                       # (the TLI spans lie in front of the records)
    k = 0
    for sr in range(16):
        for n in GRID_LENGTHS:
            for kind in GRID_KINDS[k % 7:] + GRID_KINDS[:k % 7]:
                k += 1
                pos = tab.at + 9 + k % 5
                if kind in ("DE", "TL"):
                    if n == 1:
                        continue
                    add(tab, kind, pos + (sr + 1 - pos) % 16, n - 1)     # REF = seq[pos - 1 : stop + 1]
                elif kind in ("IV", "DU"):
                    pos += (sr - pos) % 16
                    if kind == "IV":
                        tab.bases[pos + n - 1] = ord("R")                 # (no palindrome, no N at 1 base: every record has a line)
                        tab.bases[pos] = ord("M")
                    add(tab, kind, pos, n)
                else:
                    add(tab, kind, pos, n, sr=sr)
        add(tab, "SN", tab.at + 3, aux=sr % 3)                        # (125 lines per residue: see below)
    tab.bases = tab.bases[:tab.at + 40]
    return {"grid": finish(tab, range(4, 20))}


# ------------------------------------------------------------------------------ b. stage groups
def _solve_wave(x_lo, x_hi, want):
    """(b, e): b short IN / DE records of 1..3 bases, e bases in all, so that 29 b + e (what they add to a wave of SNP lines)
    satisfies ``want``."""
    for b in range(65):
        for e in range(b, 3 * b + 1):
            if x_lo <= 29 * b + e <= x_hi and want(29 * b + e):
                return b, e
    raise AssertionError("no wave")


def _short_wave(tab, b, e, step=8):
    """64 records: b IN / DE of 1..3 bases (e in all) among SNPs."""
    ks = [1] * b
    for i in range(e - b):
        ks[i % b] += 1
    slots = set(tab.rs.permutation(64)[:b].tolist())
    j = 0
    for i in range(64):
        pos = tab.at + step
        if i in slots:
            add(tab, "IN" if j % 2 else "DE", pos, ks[j])
            j += 1
        else:
            add(tab, "SN", pos, aux=i % 3)


def group_limit():
    """Two waves of 64 short records at 7-digit positions: the second one starts at text phase 0..15 and its 64 lines total
    4095, 4096 and 4097 bytes minus the phase -- the stage holds phase + total <= 4096, so the group cut falls on either side.
    An SNP line has name + 26 bytes there, an IN / DE of k bases name + 55 + k."""
    bases = genome(1_003_000, 21, codes_every=0)
    out = {}
    for ph in range(16):
        for d in (-1, 0, 1):
            total = STAGE - ph + d
            n = (total - 64 * 26 - 29 * 24) // 64 - 1                  # name length: leaves about 24 structural records' worth
            x = total - 64 * (n + 26)
            b1, e1 = _solve_wave(x, x, lambda v: True)
            b0, e0 = _solve_wave(0, 4000, lambda v: v % 16 == ph)
            tab = Table(bases, seed=100 + ph)
            tab.at = 1_000_000
            _short_wave(tab, b0, e0)
            _short_wave(tab, b1, e1)
            out[f"limit_phase{ph}_{total}"] = finish(tab, [n])
    return out


def group_limit_snp():
    """The same for the SNP-only kernel, whose wave is staged when phase + total <= 4096 and writes its lines itself when not:
    two waves of 64 SNPs on a contig of 1300 bases; a line has name + 19 + (digits of POS) bytes, so the number of two-digit
    positions among the first wave's three-digit ones sets the phase, the number of three-digit positions among the second
    wave's four-digit ones the total."""
    bases = genome(1300, 26, codes_every=0)
    out = {}
    for ph in range(16):
        for d in (-1, 0, 1):
            total = STAGE - ph + d
            n = -(-total // 64) - 23                                   # 64 lines of name + 23 bytes, minus one per three-digit POS
            m1, m0 = 64 * (n + 23) - total, (16 - ph) % 16
            tab = Table(bases, seed=ph)
            for i in range(64):
                add(tab, "SN", (9 + 2 * i) if i < m0 else 100 + 3 * i, aux=i % 3)
            for i in range(64):
                add(tab, "SN", (600 + 3 * i) if i < m1 else 1000 + 3 * i, aux=i % 3)
            out[f"snplimit_phase{ph}_{total}"] = finish(tab, [n])
    return out


def long_in_wave():
    """One wave of 64 records, 63 SNPs and a DU of 5000 bases (a line of 15 kB) at lane 0, 31, 63 -- and at lane 32 under a
    name that makes the SNP lines 128 bytes, so that lanes 0..31 fill the stage exactly and the DU opens the second group."""
    out = {}
    for key, lane, n in (("lane0", 0, 7), ("lane31", 31, 7), ("lane63", 63, 7), ("second_group", 32, 102)):
        tab = Table(genome(1_020_000, 22), seed=7)
        tab.at = 1_000_000
        for i in range(64):
            if i == lane:
                add(tab, "DU", tab.at + 11, 5000)
            else:
                add(tab, "SN", tab.at + 11, aux=i % 3)
        out[f"long_{key}"] = finish(tab, [n])
    return out


def long_wave():
    """A wave of 64 long records of mixed kinds (and a second wave of 37)."""
    tab = Table(genome(120_000, 23), seed=8)
    for i in range(101):
        add(tab, GRID_KINDS[i % 7], tab.at + 5 + i % 16, 26 + (i * 37) % 680)
    return {"long_wave": finish(tab, [5, 18])}


def fill_mixed(tab, n_rec, step=7, lens=(1, 2, 3, 1, 9, 24, 25, 26, 2, 40, 1, 70)):
    cycle = ["SN", "IN", "DE", "SN", "DU", "IV", "SN", "TL", "TLI_fwd", "SN", "TLI_rev"]
    for i in range(n_rec):
        kind = cycle[i % len(cycle)]
        add(tab, kind, tab.at + step + i % 3, lens[i % len(lens)] if kind != "SN" else 1, aux=i % 3)


def fill_snps(tab, n_rec, step=3):
    for i in range(n_rec):
        add(tab, "SN", tab.at + step + i % 2, aux=i % 3)


def name_edges():
    """A mixed table and an SNP-only table under names of 1, 63, 64, 65 (the workgroup's LDS copy of the name holds 64),
    1023, 1024 (the last name a staged wave takes) and 1025 bytes (the first that goes the plain way)."""
    tab = Table(genome(30_000, 24), seed=9)
    fill_mixed(tab, 200)
    snp = Table(genome(30_000, 25), seed=9)
    fill_snps(snp, 200)
    return {"names_mixed": finish(tab, NAME_EDGES), "names_snp": finish(snp, NAME_EDGES)}


# ------------------------------------------------------------------------------ c. table sizes, suppressed lines
def sizes():
    out = {}
    for n in SIZES:
        tab = Table(genome(40 * n + 2000, 30 + n % 7), seed=n)
        fill_mixed(tab, n)
        out[f"size_mixed_{n}"] = finish(tab, [9])
        tab = Table(genome(5 * n + 100, 40 + n % 7), seed=n)
        fill_snps(tab, n)
        out[f"size_snp_{n}"] = finish(tab, [9])
    return out


SUPPRESS_N = 600                                                      # three workgroups of 256 records: 256, 256, 88
SUPPRESS_PLACES = {"lane0": {0, 64, 320}, "last_lane": {SUPPRESS_N - 1}, "wave": set(range(128, 192)),
                   "workgroup": set(range(256, 512)), "alternating": set(range(0, SUPPRESS_N, 2)),
                   "table": set(range(SUPPRESS_N))}
SUPPRESS_ROUTES = ("snp_on_n", "snp_on_n_mixed", "palindrome_iv", "empty_tli")


def suppressed():
    """{id: (table, the records whose line must be empty)}: an SNP on N (in an SNP-only and in a mixed table), an even-length
    reverse-complement palindrome's inversion, a TLI with an empty span (an unlinked one behind position 0: start = pos,
    stop = 0) at the placements of SUPPRESS_PLACES; every other record has a line."""
    out = {}
    for route in SUPPRESS_ROUTES:
        for place, idx in SUPPRESS_PLACES.items():
            tab = Table(genome(14 * SUPPRESS_N + 500, 50, codes_every=0 if route == "snp_on_n" else 3), seed=12)
            cycle = ["SN"] if route == "snp_on_n" else ["SN", "IN", "DE", "DU", "SN", "TL", "TLI_fwd", "IV"]
            for i in range(SUPPRESS_N):
                pos = tab.at + 5 + i % 4
                if i not in idx:
                    kind = cycle[i % len(cycle)]
                    if kind == "IV":
                        tab.bases[pos:pos + 3] = np.frombuffer(b"AAC", dtype=np.uint8)       # (no palindrome)
                    add(tab, kind, pos, 1 if kind == "SN" else 3, aux=i % 3)
                elif route.startswith("snp_on_n"):
                    tab.bases[pos] = ord("N-"[i % 2]) if route.endswith("mixed") else ord("N")
                    tab.add(SN, pos, aux=i % 3)
                elif route == "palindrome_iv":
                    pal = (b"ACGT", b"GAATTC", b"KC", b"N-")[i % 4]                          # (converted: GC, NN)
                    tab.bases[pos:pos + len(pal)] = np.frombuffer(pal, dtype=np.uint8)
                    tab.add(IV, pos, len(pal))
                else:
                    tab.rows.append((pos, 0, pos, TLI, 0, 0))
                    tab.at = pos + 1
            out[f"suppress_{route}_{place}"] = (finish(tab, [6]), sorted(idx))
    return out


# ------------------------------------------------------------------------------ d. contig edges
def edges():
    """Every type at position 0 and, where it has a span, ending with the contig; DE / TL over the whole contig (END = stop + 2
    clamps; on a contig of ONE base REF == ALT and the reference writes no line); an IV of >= 48 bases at 0, a DU and a
    forward TLI span ending at L - 1, a reversed TLI span at 0; inserts that are the pool's first and last bytes; contigs of
    1, 2, 16 and 17 bases."""
    out = {}
    for L in (1, 2, 16, 17, 4099):
        n = min(L, 60)

        def table(key, *adds):
            tab = Table(genome(L, 60 + L), seed=L)
            for kind, pos, kw in adds:
                if kind == "TLI":
                    tab.add(TLI, pos, **kw)
                else:
                    add(tab, kind, pos, **kw)
            out[f"edge_L{L}_{key}"] = finish(tab, [4, 11])

        heads = [("SN", ("SN", 0, {"aux": 1})), ("IN", ("IN", 0, {"n": n})), ("DE", ("DE", 0, {"n": n})), ("TL", ("TL", 0, {"n": n})),
                 ("DU", ("DU", 0, {"n": n})), ("IV", ("IV", 0, {"n": n})), ("TLI_fwd", ("TLI", 0, {"span": (0, n)})),
                 ("TLI_rev", ("TLI", 0, {"span": (0, n), "aux": 1})), ("TLI_end", ("TLI", 0, {"span": (L - n, n)}))]
        tails = [("SN", ("SN", L - 1, {"aux": 2})), ("IN", ("IN", L - 1, {"n": 33})), ("DE", ("DE", L - n, {"n": n})),
                 ("TL", ("TL", L - n, {"n": n})), ("DU", ("DU", L - n, {"n": n})), ("IV", ("IV", L - n, {"n": n})),
                 ("TLI_fwd", ("TLI", L - 1, {"span": (L - n, n)})), ("TLI_rev", ("TLI", L - 1, {"span": (0, n), "aux": 1}))]
        for key, head in heads:
            table("head_" + key, head)
            if L > 1:
                table("head1_" + key, (head[0], 0, {**head[2], **({"n": 1} if "n" in head[2] else {})}))
        for key, tail in tails:
            if L > 1:
                one = {**tail[2], **({"n": 1} if "n" in tail[2] and key != "IN" else {})}
                table("tail1_" + key, ("IN", 0, {"n": 1}), (tail[0], L - 1, one))      # (pool: first byte; the IN tail: its last bytes)
            if L > 2 * n:
                table("both_" + key, heads[1 + (len(key) + L) % 6][1], ("SN", n + 5, {}), tail)     # (some head of 60 bases with it)
        if L > 1:                                                     # DE / TL from 0 to L - 1 and from 1 to L - 1
            for kind in ("DE", "TL"):
                table("whole_" + kind, (kind, 0, {"n": L}))
                table("rest_" + kind, (kind, 1, {"n": L - 1}))
                table("almost_" + kind, (kind, 0, {"n": L - 1}))      # stop = L - 2: END = L, REF = the whole contig, unclamped
    return out


# ------------------------------------------------------------------------------ e. digit counts
def _digit_flip(tab, B, svlen=True, rev=0):
    """Around B = 10^k: POS B - 1 and B, END B - 1 and B, a line whose END has a digit more than its POS, and (svlen) SVLEN
    B - 1 and B as the copies of two linked spans."""
    tab.add(DU, B - 4, 3)                                             # POS B - 3, END B - 1
    tab.add(DE, B - 1, 1)                                             # POS B - 1, END B
    tab.add(IN, B, 2)                                                 # POS B, END B
    if svlen:
        tab.add(TLI, B + 2, span=(3, B - 1), aux=rev)
        tab.add(TLI, B + 4, span=(5, B))


def digits():
    tab = Table(genome(10_000_016, 70), seed=1)
    for k in range(1, 8):
        _digit_flip(tab, 10 ** k, rev=k % 2)
    out = {"digits_10M": finish(tab, [8])}
    tab = Table(genome(100_000_016, 71), seed=2)
    add(tab, "SN", 5, aux=1)
    add(tab, "IV", 99_999_900, 30)
    add(tab, "SN", 99_999_990, aux=2)
    _digit_flip(tab, 10 ** 8, svlen=False)
    add(tab, "SN", 10 ** 8 + 3)
    add(tab, "TL", 10 ** 8 + 5, 4)
    add(tab, "TLI_rev", 10 ** 8 + 9, 40)
    add(tab, "DU", 10 ** 8 + 11, 5)
    assert len(tab.rows) == 10
    out["digits_100M"] = finish(tab, [8])
    return out


# ------------------------------------------------------------------------------ f. more than 1024 length blocks
BLOCKS_N = 1024 * 2048 + 2049


def many_blocks():
    """SNPs on consecutive bases of a contig of 1024 x 2048 + 2049 bases (the scan of the lengths' block sums takes a second
    round of 1024), with suppressed lines (N) strewn in; ``blocks_de``: the last record a 1-base DE -- the general kernel."""
    bases = genome(BLOCKS_N, 80, codes_every=0)
    bases[::1013] = ord("N")
    recs = np.zeros(BLOCKS_N, dtype=RECORD_DTYPE)
    recs["pos"] = recs["stop"] = np.arange(BLOCKS_N)
    recs["type"] = SN
    recs["aux"] = np.arange(BLOCKS_N) % 3
    pool = np.zeros(0, dtype=np.uint8)
    gt = (np.arange(BLOCKS_N) % 3 + 1).astype(np.uint8)
    de = recs.copy()
    de["type"][-1], de["aux"][-1] = DE, 0
    return {"blocks_snp": (bases, recs, pool, ["chrB"], gt), "blocks_de": (bases, de, pool, ["chrB"], gt)}


@functools.lru_cache(maxsize=None)
def tables_blocks():
    return many_blocks()


def blocks_text(case, name, gt=None):
    """The expected text of a many_blocks table: the SNP records by vcf_ref's vectorised path, a last DE by ``lines``."""
    bases, recs, pool = case[:3]
    n = len(recs) - (recs["type"][-1] != SN)
    text = vcf_ref.snp_text(bases, recs[:n], name, None if gt is None else gt[:n])
    return text + b"".join(vcf_ref.lines(bases, recs[n:], pool, name, None if gt is None else gt[n:]))


PARTS = {"grid": grid, "group_limit": group_limit, "group_limit_snp": group_limit_snp, "long_in_wave": long_in_wave, "long_wave": long_wave, "name_edges": name_edges,
         "sizes": sizes, "suppressed": lambda: {k: v[0] for k, v in suppressed().items()}, "edges": edges, "digits": digits}
PLAIN_PARTS = ("grid", "edges")                                       # g: once more the byte-by-byte way


@functools.lru_cache(maxsize=None)
def tables(part):
    """The tables of one part (built once per process; nobody writes to them)."""
    return PARTS[part]()


@functools.lru_cache(maxsize=None)
def expected(part):
    """id -> (lines, lines of the genotyped render) under the table's FIRST name: vcf_ref, computed once (vcf_ref.rename
    gives the other names)."""
    return {key: (vcf_ref.lines(b, r, p, names[0]), vcf_ref.lines(b, r, p, names[0], gt)) for key, (b, r, p, names, gt) in tables(part).items()}


# ------------------------------------------------------------------------------ coverage: functions of the expected text
def interior(c):
    """The 16-byte-aligned interior [ia, ib) in TEXT coordinates of a copy longer than INLINE, or None: what a stage leaves
    out and the wave copies source -> text."""
    if c.length <= INLINE:
        return None
    ia, ib = (c.offset + 15) & ~15, (c.offset + c.length) & ~15
    return (ia, ib) if ib > ia else None


def stage_groups(body, copies, first_offset=0):
    """The groups of consecutive lanes whose compact text (line minus its copies' interiors) fits STAGE together with the
    phase of the group's first line: [(wave, first lane, one past the last lane)] -- DESIGN.md's statement of the scheme."""
    gaps = np.zeros(len(body), dtype=np.int64)
    for c in copies:
        r = interior(c)
        if r:
            gaps[c.record] += r[1] - r[0]
    lens = np.array([len(l) for l in body], dtype=np.int64)
    offs = first_offset + np.cumsum(lens) - lens
    out = []
    for w0 in range(0, len(body), 64):
        lo, last = w0, min(w0 + 64, len(body))
        while lo < last:
            used, hi = int(offs[lo] % 16), lo
            while hi < last and used + lens[hi] - gaps[hi] <= STAGE:
                used += int(lens[hi] - gaps[hi])
                hi += 1
            hi = max(hi, lo + 1)
            out.append((w0 // 64, lo - w0, hi - w0))
            lo = hi
    return out
