"""The APPLY kernels (csrc/apply.hip) on HAND-BUILT record tables.

Every other GPU test reaches ``k_rewrite_snp``, ``k_rewrite<140>``, ``k_rewrite<1024>`` and their batch variants behind a
planner, so the offsets, alignments and densities the kernels see are whatever the reference's draws give.  Here the tables
are made by construction (``msim_dbg_set_records``) and every result is compared, byte for byte, with ``tests/apply_ref.py``
-- the plain restatement of ``__mutate_sequence`` that tests/test_apply_ref_host.py pins to the real reference's bytes.

Each table goes through three routes: (a) the device offset scan, (b) offsets that came with the table, (c) the same inside
``msim_dbg_apply_batch`` (``k_tile_index_batch`` + ``k_rewrite*_b``).  All comparisons are exact.
"""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import apply_ref
from apply_ref import DE, DU, IN, IV, SN, TL, TLI
from helpers import load_json
from mutation_simulator_amd import _ffi

pytestmark = pytest.mark.gpu

T = 16384                      # output bytes per tile (apply.hip: THREADS * GROUP * ITERS)
WIN_SMALL, WIN_LARGE = 140, 1024
ROUTES = ("scan", "offsets", "batch")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
IUPAC = np.frombuffer(b"KSYMWRBDHV-NUX", dtype=np.uint8)
NAMES = {SN: "SN", IN: "IN", DE: "DE", DU: "DU", IV: "IV", TL: "TL", TLI: "TLI"}


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def make_bases(L, seed, iupac=True):
    """Random ACGT; with ``iupac`` single ambiguity codes every ~11 bases (so that most dwords holding one hold exactly one:
    map4's table path beside its permute path), U, '-', a byte no table touches, and a few N runs."""
    rs = np.random.RandomState(seed)
    b = ACGT[rs.randint(0, 4, L)].copy()
    if iupac and L > 64:
        at = np.unique(rs.randint(0, L, L // 11))
        b[at] = IUPAC[rs.randint(0, len(IUPAC), len(at))]
        for s in rs.randint(0, L - 40, 4):
            b[s:s + int(rs.randint(1, 40))] = ord("N")
    return b


def tv_safe(byte):
    return bytes([apply_ref.NON_AMBIGUOUS[byte]]) in (b"A", b"C", b"G", b"T", b"N")


class Table:
    """A record table made in position order.  ``delta`` = output offset - input position for the next record, so a wanted
    output offset ``o`` is the position ``o - delta``; a DE or IN in front shifts the two against each other."""

    def __init__(self, bases, seed=1):
        self.bases, self.rows, self.pool = bases, [], bytearray()
        self.at, self.delta, self.rs = 0, 0, np.random.RandomState(seed)

    def add(self, typ, pos, length=1, aux=0, span=None, pool_mod=None):
        assert self.at <= pos < len(self.bases), (NAMES[typ], pos, self.at, len(self.bases))
        o = pos + self.delta
        if typ == SN:
            if aux and not tv_safe(self.bases[pos]):
                self.bases[pos] = ord("R")                            # (R converts to A: a transversion the dict knows)
            self.rows.append((pos, pos, 0, SN, aux, 0))
            self.at = pos + 1
        elif typ == IN:
            while pool_mod is not None and len(self.pool) % 16 != pool_mod:
                self.pool.append(ord("T"))
            self.rows.append((pos, pos + length - 1, len(self.pool), IN, 0, 0))
            self.pool += ACGT[self.rs.randint(0, 4, length)].tobytes()
            self.delta += length
            self.at = pos + 1
        elif typ == TLI:
            start, n = span
            assert 0 <= start and start + n <= len(self.bases)
            self.rows.append((pos, start + n - 1, start, TLI, (aux & 1) | (2 if pos else 0), 0))
            self.delta += n
            self.at = pos + 1
        else:
            assert pos + length <= len(self.bases), (NAMES[typ], pos, length)
            self.rows.append((pos, pos + length - 1, 0, typ, 0, 0))
            self.delta += length if typ == DU else 0 if typ == IV else -length
            self.at = pos + length
        return o

    def at_offset(self, typ, o, **kw):
        return self.add(typ, o - self.delta, **kw)

    def shift_mod16(self, want):
        """A short deletion so that (output offset - position) % 16 == want for what follows."""
        k = (self.delta - want) % 16
        if k:
            self.add(DE, self.at + 3, k)

    def done(self):
        recs = np.array(self.rows, dtype=_ffi.RECORD_DTYPE).reshape(-1) if self.rows else np.zeros(0, dtype=_ffi.RECORD_DTYPE)
        return self.bases, recs, np.frombuffer(bytes(self.pool), dtype=np.uint8).copy()


def picks_small_window(n_rec, out_len):
    """apply_contig_device's rule for a table with host-known sizes: the 140-entry window when the mean number of records
    per tile is below 80 % of it."""
    n_tiles = (out_len + T - 1) // T
    return n_rec * 5 + 64 * 4 < n_tiles * WIN_SMALL * 4


def explain(got, want, recs, offsets):
    n = min(len(got), len(want))
    bad = np.nonzero(got[:n] != want[:n])[0]
    if not len(bad):
        return f"lengths differ: {len(got)} != {len(want)}"
    d = int(bad[0])
    j = int(np.searchsorted(offsets, d, side="right")) - 1
    gov = "none (in front of the first record)" if j < 0 else \
        f"#{j} {NAMES[int(recs['type'][j])]} pos={recs['pos'][j]} stop={recs['stop'][j]} extra={recs['extra'][j]} aux={recs['aux'][j]} offset={offsets[j]}"
    return (f"{len(bad)} bytes differ, first at output offset {d} (tile {d // T}, group {(d % T) // 16}, byte {d % 16}): "
            f"got {bytes(got[d:d + 8])!r} want {bytes(want[d:d + 8])!r}; governing record {gov}")


def compare(eng, cid, bases, recs, pool, want, route, text=False):
    if want.key_error is not None:
        assert eng.key_error(cid) == want.key_error, route
        with pytest.raises(KeyError):
            eng.result_sizes(cid)
        return
    assert eng.result_sizes(cid) == (want.out_len, len(recs), len(pool)), route
    got = eng.fetch_sequence(cid)
    assert len(got) == want.out_len and np.array_equal(got, want.seq), f"route {route}: " + explain(got, want.seq, recs, want.offsets)
    assert eng.key_error(cid) is None, route
    if text:
        assert eng.render_vcf_device(cid, "chrT").tobytes() == _ffi.render_vcf(recs, pool, bases, "chrT"), route
        assert eng.fetch_sequence_framed(cid, 60).tobytes().replace(b"\n", b"") == want.seq.tobytes(), route


def run_table(eng, bases, recs, pool, text=False, routes=ROUTES, want=None):
    """One table through the routes; returns the reference's result."""
    want = want or apply_ref.apply(bases, recs, pool)
    for route in routes:
        eng.clear()
        cid = eng.add_contig(bases)
        eng.set_records(cid, recs, pool, with_offsets=route != "scan")
        try:
            if route == "batch":
                eng.apply_batch([cid])
            else:
                eng.apply_contig(cid)
        except KeyError:                                              # (the scan route collects its APPLY at once)
            assert want.key_error is not None and route == "scan"
        compare(eng, cid, bases, recs, pool, want, route, text)
    eng.clear()
    return want


# ------------------------------------------------------------------------------ 1. the reference's goldens through the kernels
APPLY = load_json("apply.json")


@pytest.mark.parametrize("case", APPLY["cases"], ids=lambda c: c["name"])
def test_goldens_through_the_kernels(eng, case):
    recs, pool = apply_ref.golden_table(case)
    bases = np.frombuffer(case["sequence"].encode(), dtype=np.uint8).copy()
    want = run_table(eng, bases, recs, pool, text=True)
    assert want.seq.tobytes() == apply_ref.unwrap_fasta(case["fasta"]).tobytes()      # the real reference's bytes


# ------------------------------------------------------------------------------ 2. edges by construction
KINDS = ["IN", "DE", "DU", "IV", "TL", "TLI_fwd", "TLI_rev"]
EDGE_D = [-17, -16, -15, -1, 0, 1, 15, 16, 17]
EDGE_LEN = [1, 2, 15, 16, 17, 31, 32, 33, 255]


def add_kind(tab, kind, o, length, src_mod=None):
    """One record of ``kind`` whose first output byte lands at ``o``; ``src_mod``: its source's address mod 16 (the insert's
    pool offset, a TLI's span start -- for the others the source is the position itself, fixed by ``shift_mod16``)."""
    if kind == "IN":
        return tab.at_offset(IN, o, length=length, pool_mod=src_mod)
    if kind.startswith("TLI"):
        start = 16 * int(tab.rs.randint(1, 250)) + (src_mod if src_mod is not None else int(tab.rs.randint(0, 16)))
        return tab.at_offset(TLI, o, span=(start, length), aux=1 if kind == "TLI_rev" else 0)
    return tab.at_offset({"DE": DE, "DU": DU, "IV": IV, "TL": TL}[kind], o, length=length)


def seg_len(kind, length):
    return 0 if kind in ("DE", "TL") else length


@pytest.mark.parametrize("length", EDGE_LEN)
@pytest.mark.parametrize("kind", KINDS)
def test_segment_edges_at_tile_edges(eng, kind, length):
    """A segment (or, for DE / TL, the cut) that starts at T + d, and one that ends at T + d, for T = one and two tiles: one
    record at each of the two tile edges of a contig, a short deletion in front shifting source against output."""
    for d in EDGE_D:
        for where in ("start", "end"):
            tab = Table(make_bases(3 * T + 4096, 100 + length), seed=d + 50)
            tab.shift_mod16((length * 7 + d) % 16)
            for edge in (T, 2 * T):
                o = edge + d - (seg_len(kind, length) if where == "end" else 0)
                assert add_kind(tab, kind, o, length) == o
            run_table(eng, *tab.done(), text=(d == 0 and where == "start"))


def test_snps_at_tile_and_group_edges(eng):
    tab = Table(make_bases(3 * T, 7))
    for edge in (T, 2 * T):
        for k, d in enumerate(EDGE_D):
            tab.add(SN, edge + d, aux=k % 3)
    bases, recs, pool = tab.done()
    assert np.all(recs["type"] == SN)
    run_table(eng, bases, recs, pool, text=True)                       # k_rewrite_snp
    tab = Table(make_bases(3 * T, 8))
    tab.add(DE, 40, 5)
    for edge in (T, 2 * T):
        for k, d in enumerate(EDGE_D):
            tab.at_offset(SN, edge + d, aux=k % 3)
    run_table(eng, *tab.done())                                       # pass B2 of k_rewrite


@pytest.mark.parametrize("gap", [400, 32], ids=["sparse", "dense"])
@pytest.mark.parametrize("kind", KINDS)
def test_all_source_and_output_alignments(eng, kind, gap):
    """Length-33 segments at all 16 x 16 pairs of (source address mod 16, output offset mod 16): the two aligned loads + byte
    funnel of piece_load / piece_finish, for the segment and for the copy run behind it.  ``sparse``: records far enough apart
    for the 140-entry window; ``dense``: more than 128 structural records per tile, the 1024-entry window (pass B's loop)."""
    reps = 1 if gap == 400 else 2                                     # (dense: twice, so that a whole tile is that dense)
    L = reps * 2 * 256 * (gap + 120) + 8192
    tab = Table(make_bases(L, 31), seed=3)
    tab.at = 4400                                                     # (the TLI spans lie in front of it)
    for sa, oa in [(q // 16 % 16, q % 16) for q in range(256 * reps)]:
        if True:
            if kind == "IN" or kind.startswith("TLI"):                # source = pool offset / span start; output = oa
                pos = tab.at + gap
                pos += (oa - pos - tab.delta) % 16
                assert add_kind(tab, kind, pos + tab.delta, 33, src_mod=sa) % 16 == oa
            else:                                                     # source = the position
                tab.shift_mod16((oa - sa) % 16)
                pos = tab.at + gap
                pos += (sa - pos) % 16
                assert add_kind(tab, kind, pos + tab.delta, 33) % 16 == oa and pos % 16 == sa
    tab.bases = tab.bases[:tab.at + 100]
    bases, recs, pool = tab.done()
    want = apply_ref.apply(bases, recs, pool)
    assert picks_small_window(len(recs), want.out_len) == (gap == 400)
    per_tile = np.bincount(want.offsets // T)
    assert (per_tile.max() < WIN_SMALL) if gap == 400 else (128 < per_tile[1] < WIN_LARGE)
    run_table(eng, bases, recs, pool, text=True, want=want)


# ------------------------------------------------------------------------------ 3. long pieces, contig ends, tiny contigs
def test_pieces_that_span_many_tiles(eng):
    L = 1_400_000
    tab = Table(make_bases(L, 41), seed=4)
    o = 8 * T + 8191
    for kind, n in (("DU", 50_000), ("IV", 50_000), ("IN", 50_000), ("TLI_fwd", 50_000), ("TLI_rev", 50_000), ("DE", 400_000),
                    ("TL", 400_000)):
        if kind.startswith("TLI"):
            tab.at_offset(TLI, o, span=(1000 + 7 * len(tab.rows), n), aux=1 if kind == "TLI_rev" else 0)
        else:
            add_kind(tab, kind, o, n)
        o = (tab.at + tab.delta) // T * T + 2 * T + 8191 + 3 * len(tab.rows)      # mid-tile, two tiles behind the piece
    bases, recs, pool = tab.done()
    want = run_table(eng, bases, recs, pool, text=True)
    assert np.all((want.offsets % T > 4000) & (want.offsets % T < 12000))


@pytest.mark.parametrize("p", [0, 1, 15, 16, 31])
def test_reversed_sources_at_the_contig_start(eng, p):
    """An inversion at 0..31 and a reversed TLI whose span starts there: the first aligned load of the reversed source lies
    in the pad in front of the contig."""
    tab = Table(make_bases(40_000, 42 + p))
    tab.add(IV, p, 40)
    tab.add(TLI, 3000, span=(p, 45), aux=1)
    tab.add(TLI, 20_000, span=(p, 17), aux=1)
    run_table(eng, *tab.done(), text=p == 0)


@pytest.mark.parametrize("kind", ["DU", "IV", "DE", "TLI_fwd", "IN"])
def test_sources_at_the_contig_end(eng, kind):
    """A forward source that ends with the contig (its last aligned load reaches into the pad behind it); insertions in front
    of the first and of the last base."""
    L = 40_000 + 7
    tab = Table(make_bases(L, 43))
    if kind == "TLI_fwd":
        tab.add(TLI, 100, span=(L - 77, 77))
    elif kind == "IN":
        tab.add(IN, 0, 50)
        tab.add(IN, L - 1, 50_000)
    else:
        tab.add(DE, 50, 3)
        tab.add({"DU": DU, "IV": IV, "DE": DE}[kind], L - 300, 300)
    run_table(eng, *tab.done())


@pytest.mark.parametrize("L", [1, 15, 16, 17, 16383, 16384, 16385])
def test_contig_lengths_around_a_group_and_a_tile(eng, L):
    tables = []

    def table(*adds, seed=0):
        tab = Table(make_bases(L, 44 + L % 7 + seed, iupac=L > 100))
        for a in adds:
            tab.add(a[0], a[1], **a[2])
        tables.append(tab.done())

    table()
    table((SN, 0, {"aux": 1}))
    table((SN, L - 1, {"aux": 2}))
    table((IN, 0, {"length": 3}), *([(IN, L - 1, {"length": 18})] if L > 1 else []))
    table((DU, 0, {"length": L}))
    table((IV, 0, {"length": L}))
    table((DE, 0, {"length": L}))
    table((TL, 0, {"length": L - 1}), seed=1) if L > 1 else None
    table((TLI, 0, {"span": (0, L)}))
    table((TLI, L - 1, {"span": (0, L), "aux": 1}))
    for k, t in enumerate(tables):
        run_table(eng, *t, text=k == 3)


# ------------------------------------------------------------------------------ 4. density
def dense_cluster(tab, o0, n_struct):
    """n_struct structural records (DE of 1, IN of 1, alternating) with an SNP behind each, from output offset o0 on: four
    input bases and four output bytes per pair."""
    pos = o0 - tab.delta
    for k in range(n_struct):
        tab.add(DE if k % 2 == 0 else IN, pos + 2 * k, 1)
        tab.add(SN, pos + 2 * k + 1, aux=k % 3)


def background(tab, step, out_upto=None, in_upto=None):
    """Records of every type, one about every ``step`` bases, an SNP behind each, as long as the next one stays in front of
    the output offset ``out_upto`` / the position ``in_upto``."""
    kinds = ["IN", "DE", "DU", "IV", "TL", "TLI_fwd", "TLI_rev"]
    in_upto = len(tab.bases) if in_upto is None else in_upto
    k = 0
    while tab.at + step + 500 < in_upto and (out_upto is None or tab.at + tab.delta + step + 500 < out_upto):
        pos = tab.at + step + int(tab.rs.randint(0, 32))
        add_kind(tab, kinds[k % 7], pos + tab.delta, 1 + int(tab.rs.randint(0, 60)))
        tab.add(SN, tab.at + 9, aux=k % 3)
        k += 1


def density_table(L, step, tiles, seed):
    """Background records every ``step`` bases; in tile t of ``tiles`` exactly tiles[t] structural records (dense_cluster)."""
    tab = Table(make_bases(L, seed), seed=seed)
    for t in sorted(tiles):
        background(tab, step, out_upto=(t - 1) * T + T // 2)           # (leaves the tile in front of t half empty)
        dense_cluster(tab, t * T + 64, tiles[t])
        tab.add(SN, tab.at + (t + 1) * T + 64 - (tab.at + tab.delta), aux=0)   # the next record: behind tile t
    background(tab, step)
    return tab.done()


def struct_per_tile(want, recs):
    return np.bincount(want.offsets[recs["type"] != SN] // T, minlength=want.out_len // T + 1)


def test_dense_tiles_in_a_sparse_table(eng):
    """The 140-entry window kernel with single tiles that overflow it: rewrite_tile<false, 140>."""
    tiles = {20: 141, 60: 200, 100: 300, 180: 5000}
    bases, recs, pool = density_table(4_000_000, 1500, tiles, 51)
    want = apply_ref.apply(bases, recs, pool)
    assert picks_small_window(len(recs), want.out_len)
    per_tile = struct_per_tile(want, recs)
    for t, n in tiles.items():
        assert per_tile[t] == n
    assert np.sort(per_tile)[-5] < 40                                 # every other tile fits the window with room
    run_table(eng, bases, recs, pool, text=True, want=want)


def test_dense_tiles_in_a_dense_table(eng):
    """The 1024-entry window kernel at its capacity: 1023 structural records + the anchor fit, 1024 and more fall back to
    rewrite_tile<false, 1024>; every tile has more than 128 (pass B's loop)."""
    tiles = {8: 1023, 16: 1024, 24: 1025, 40: 5000}
    bases, recs, pool = density_table(1_000_000, 50, tiles, 52)
    want = apply_ref.apply(bases, recs, pool)
    assert not picks_small_window(len(recs), want.out_len)
    per_tile = struct_per_tile(want, recs)
    for t, n in tiles.items():
        assert per_tile[t] == n
    assert np.median(per_tile) > 128
    run_table(eng, bases, recs, pool, text=True, want=want)


@pytest.mark.parametrize("shape", ["snp_only", "small_window", "large_window"])
def test_snp_hot_spot(eng, shape):
    """More than 1024 SNPs in one tile: k_rewrite_snp's record loop; pass B2's loop beyond a tile's first 256 records."""
    L = 600_000
    tab = Table(make_bases(L, 53), seed=5)
    if shape != "snp_only":
        background(tab, 1500 if shape == "small_window" else 40, out_upto=5 * T)
    tab.add(SN, 6 * T + 100 - tab.delta)
    for k in range(3000):
        tab.add(SN, tab.at + 1 + k % 3, aux=k % 3)
        if shape != "snp_only" and k % 500 == 250:
            tab.add(DE, tab.at + 1, 2)
    if shape != "snp_only":
        background(tab, 1500 if shape == "small_window" else 40)
    bases, recs, pool = tab.done()
    want = apply_ref.apply(bases, recs, pool)
    snps = np.bincount(want.offsets[recs["type"] == SN] // T)
    assert snps[6] > 1024 and np.all(recs["type"] == SN) == (shape == "snp_only")
    if shape != "snp_only":
        assert picks_small_window(len(recs), want.out_len) == (shape == "small_window")
    run_table(eng, bases, recs, pool, text=True, want=want)


# ------------------------------------------------------------------------------ 5. sizes
def test_whole_contig_deleted(eng):
    for L in (1, 5000, 3 * T):
        tab = Table(make_bases(L, 61))
        tab.add(DE, 0, L)
        want = run_table(eng, *tab.done())
        assert want.out_len == 0


@pytest.mark.parametrize("how", ["DE", "IN"])
@pytest.mark.parametrize("out_len", [T - 1, T, T + 1, 2 * T])
def test_mutated_length_at_a_tile_edge(eng, out_len, how):
    if how == "DE":
        tab = Table(make_bases(out_len + 777, 62))
        tab.add(SN, 5, aux=0)
        tab.add(DE, out_len, 777)
    else:
        tab = Table(make_bases(out_len - 37, 63))
        tab.add(SN, 5, aux=0)
        tab.add(IN, out_len - 38, 37)
    want = run_table(eng, *tab.done(), text=True)
    assert want.out_len == out_len


def test_records_with_equal_output_offsets(eng):
    """A record that writes nothing (DE, TL) followed at once by another: both have the same output offset, the later one
    governs (atomicMax).  Once on a group edge, once inside a group, once on a tile edge."""
    tab = Table(make_bases(4 * T, 64))
    tab.add(DE, 0, 10)
    tab.add(IN, 10, 7)                                                # DE at 0, then IN
    for o in (1024, 4096 + 16 * 9 + 5, T, 2 * T + 3):
        p = o - tab.delta
        tab.add(DE, p, 10)
        tab.add(DE, p + 10, 6)                                        # DE, DE
        p = o + 200 - tab.delta
        tab.add(DE, p, 4)
        tab.add(IN, p + 4, 9)                                         # DE, IN
        p = o + 400 - tab.delta
        tab.add(TL, p, 12)
        tab.add(SN, p + 12, aux=1)                                    # TL, SN
        p = o + 600 - tab.delta
        tab.add(TL, p, 3)
        tab.add(DU, p + 3, 20)
    bases, recs, pool = tab.done()
    want = run_table(eng, bases, recs, pool, text=True)
    assert (np.diff(want.offsets) == 0).sum() == 17


# ------------------------------------------------------------------------------ 6. the device offset scan at size
def test_offset_scan_over_a_million_mixed_records(eng):
    """60 Mb, 1.25 M records of all seven types: more than 1024 blocks for k_delta_reduce / k_scan_sums / k_offsets."""
    L, stride = 60_000_000, 48
    rs = np.random.RandomState(71)
    bases = make_bases(L, 72)
    n = (L - 4096) // stride
    recs = np.zeros(n, dtype=_ffi.RECORD_DTYPE)
    pos = (np.arange(n, dtype=np.int64) * stride + rs.randint(0, 8, n)).astype(np.int64)
    typ = rs.choice([SN, IN, DE, DU, IV, TL, TLI], size=n, p=[0.4, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1])
    length = rs.randint(1, 31, n)
    safe = np.isin(apply_ref.NON_AMBIGUOUS[bases[pos]], np.frombuffer(b"ACGTN", dtype=np.uint8))
    recs["pos"], recs["type"] = pos, typ
    recs["stop"] = np.where(typ == SN, pos, pos + length - 1)
    recs["aux"] = np.where(typ == SN, np.where(safe, rs.randint(0, 3, n), 0), np.where(typ == TLI, rs.randint(0, 2, n) | 2, 0))
    ins = np.where(typ == IN, length, 0)
    recs["extra"] = np.cumsum(ins) - ins
    span = rs.randint(0, L - 64, n)
    tli = typ == TLI
    recs["extra"][tli] = span[tli]
    recs["stop"][tli] = span[tli] + length[tli] - 1
    pool = ACGT[rs.randint(0, 4, int(ins.sum()))]
    assert n > 1024 * 1024 and len(set(typ.tolist())) == 7
    want = apply_ref.apply(bases, recs, pool)
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, recs, pool)
    eng.apply_contig(cid)
    assert eng.result_sizes(cid) == (want.out_len, n, len(pool))
    got = eng.fetch_sequence(cid)
    if hashlib.sha256(got.tobytes()).digest() != hashlib.sha256(want.seq.tobytes()).digest():
        raise AssertionError(explain(got, want.seq, recs, want.offsets))
    eng.clear()


# ------------------------------------------------------------------------------ 7. KeyError
def key_error_table(shape, offenders):
    """SNPs with transversions on R and '-' (fine: they convert to A and N) and N (N -> N), plus ``offenders``: (tile, byte in
    tile, base) of transversions on bases the dict does not know."""
    L = 12 * T
    tab = Table(make_bases(L, 81, iupac=False), seed=8)
    marks = {}
    for t, at, base in offenders:
        marks[t * T + at] = base
    events = sorted([(o, b) for o, b in marks.items()] + [(t * T + 5000 + 16 * k + k, b) for t in range(1, 11) for k, b in
                                                          enumerate((ord("R"), ord("-"), ord("N"), ord("N")))])
    if shape == "dense_fallback":
        events = [(o, b) for o, b in events if not 3 * T <= o < 5 * T or o in marks]
    step = {"snp_only": None, "small_window": 1500, "large_window": 40, "dense_fallback": 1500}[shape]
    for o, b in events:
        if shape == "dense_fallback" and o in marks and o // T == 3:
            background(tab, step, out_upto=3 * T - 2000)
            dense_cluster(tab, 3 * T + 64, 400)                       # the offender of tile 3 stands behind 400 pairs
        elif step:
            background(tab, step, out_upto=o - 300)
        pos = o - tab.delta
        if pos < tab.at:
            continue
        tab.bases[pos] = b
        tab.rows.append((pos, pos, 0, SN, 1 + (pos & 1), 0))          # (not Table.add: it would make the base a known one)
        tab.at = pos + 1
    return tab.done()


@pytest.mark.parametrize("shape", ["snp_only", "small_window", "large_window", "dense_fallback"])
def test_key_error_reports_the_lowest_position(eng, shape):
    offenders = [(9, 160, ord("X")), (3, 8000 + 16 * 31, ord("U")), (6, 77, ord("*"))]      # (tile 3's stands on a group's first byte)
    bases, recs, pool = key_error_table(shape, offenders)
    want = apply_ref.apply(bases, recs, pool)
    assert want.key_error is not None and want.key_error[0] == "U" and (recs["type"] == SN).all() == (shape == "snp_only")
    hit = recs["pos"][(recs["type"] == SN) & np.isin(bases[recs["pos"]], [ord("X"), ord("U"), ord("*")])]
    assert len(hit) == 3 and want.key_error[1] == hit.min()
    off = apply_ref.apply(bases, recs[recs["pos"] < hit.min()], pool).out_len - (len(bases) - hit.min())
    assert off // T == 3                                              # not in the first tile launched
    if shape == "dense_fallback":                                     # tile 3: 400 structural records in the small window's kernel
        before = apply_ref.apply(bases, recs[recs["pos"] < hit.min()], pool)
        assert picks_small_window(len(recs), len(bases)) and struct_per_tile(before, recs[recs["pos"] < hit.min()])[3] == 400
    run_table(eng, bases, recs, pool, want=want)


@pytest.mark.parametrize("shape", ["snp_only", "small_window", "large_window"])
def test_transversions_the_dict_knows_are_no_error(eng, shape):
    """R -> A and '-' -> N take the dict's column; N transverses to N: no KeyError, the bytes equal the reference's."""
    bases, recs, pool = key_error_table(shape, [])
    sn = recs[recs["type"] == SN]
    assert {ord("R"), ord("-"), ord("N")} <= set(bases[sn["pos"]].tolist()) and np.all(sn["aux"][np.isin(bases[sn["pos"]], [ord("N")])] > 0)
    want = run_table(eng, bases, recs, pool, text=True)
    assert want.key_error is None
    n_pos = sn["pos"][bases[sn["pos"]] == ord("N")]
    assert np.all(want.seq[want.offsets[np.isin(recs["pos"], n_pos)]] == ord("N"))


# ------------------------------------------------------------------------------ 8. batches
def random_table(L, seed, shape):
    tab = Table(make_bases(L, seed), seed=seed)
    if shape == "snp_only":
        while tab.at + 200 < L:
            tab.add(SN, tab.at + 1 + int(tab.rs.randint(0, 150)), aux=int(tab.rs.randint(0, 3)))
    else:
        background(tab, 1500 if shape == "small_window" else 40)
    return tab.done()


def run_batch(eng, tables):
    eng.clear()
    wants = [apply_ref.apply(*t) for t in tables]
    cids = []
    for bases, recs, pool in tables:
        cids.append(eng.add_contig(bases))
        eng.set_records(cids[-1], recs, pool, with_offsets=True)
    eng.apply_batch(cids)
    for k, (cid, t, want) in enumerate(zip(cids, tables, wants)):
        compare(eng, cid, *t, want, f"batch of {len(tables)}, contig {k}", text=k < 2)
    eng.clear()


def shapes_of(tables):
    out = []
    for bases, recs, pool in tables:
        out_len = apply_ref.apply(bases, recs, pool).out_len
        out.append("snp_only" if np.all(recs["type"] == SN) else "small_window" if picks_small_window(len(recs), out_len) else "large_window")
    return out


def test_batch_of_two(eng):
    tables = [random_table(150_000, 91, "small_window"), random_table(90_000, 92, "snp_only")]
    assert shapes_of(tables) == ["small_window", "snp_only"]
    run_batch(eng, tables)


def test_batch_of_sixteen_mixed(eng):
    kinds = ["snp_only", "small_window", "large_window"]
    tables = [random_table(60_000 + 7001 * k, 100 + k, kinds[k % 3]) for k in range(15)] + [random_table(9_000, 120, "large_window")]
    assert shapes_of(tables) == [kinds[k % 3] for k in range(15)] + ["large_window"] and len(tables[-1][0]) < T
    run_batch(eng, tables)


def test_batch_beyond_one_launch(eng):
    """Seventeen contigs of one kernel variant do not fit one launch (RW_JOBS = 16), thirty-six not one tile-index launch
    (32 jobs): 17 small-window, 17 SNP-only, one large-window table and a contig of a single tile (small window too)."""
    tables = [random_table(50_000 + 3001 * k, 200 + k, "small_window") for k in range(17)] + \
             [random_table(40_000 + 5003 * k, 300 + k, "snp_only") for k in range(17)] + \
             [random_table(120_000, 400, "large_window"), random_table(5_000, 401, "small_window")]
    s = shapes_of(tables)
    assert s.count("small_window") == 18 and s.count("snp_only") == 17 and len(tables) == 36
    run_batch(eng, tables)


def test_batch_in_which_one_contig_offends(eng):
    """Five contigs, the fourth holds the transversions on U / X / *: its KeyError is its own, the others' bytes are right."""
    bad = key_error_table("small_window", [(9, 160, ord("X")), (3, 8000, ord("U")), (6, 77, ord("*"))])
    tables = [random_table(150_000, 501, "small_window"), random_table(90_000, 502, "snp_only"), random_table(80_000, 503, "large_window"),
              bad, key_error_table("small_window", [])]
    eng.clear()
    wants = [apply_ref.apply(*t) for t in tables]
    assert [w.key_error is not None for w in wants] == [False, False, False, True, False]
    cids = []
    for bases, recs, pool in tables:
        cids.append(eng.add_contig(bases))
        eng.set_records(cids[-1], recs, pool, with_offsets=True)
    eng.apply_batch(cids)
    assert [eng.key_error(c) for c in cids] == [w.key_error for w in wants]
    for k, (cid, t, want) in enumerate(zip(cids, tables, wants)):
        if want.key_error is None:
            compare(eng, cid, *t, want, f"contig {k} beside an offender", text=k == 0)
        else:
            with pytest.raises(KeyError):
                eng.fetch_sequence(cid, 0, 16)
    eng.clear()
