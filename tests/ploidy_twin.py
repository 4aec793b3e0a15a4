"""numpy restatement of the genotype draw of a diploid run (``--ploidy 2``; include/msim.h: msim_genotype_contig), written from
its rules over ``fast_twin``'s Philox -- test infrastructure shared by the CPU and the GPU tier:

* counter (x = record index in the contig's full table, y = 0, the contig's number ``seq``, tag 20) under the 64-bit key;
* heterozygous iff ``(lo64 >> 11) < het_thr``; the phase is bit 0 of ``hi64`` (0: haplotype 1, 1: haplotype 2);
* genotype byte: bit 0 "on haplotype 1", bit 1 "on haplotype 2" -- 1, 2 or 3;
* a TLI takes the draw of the TL record whose ``pos`` equals its ``extra`` (binary search over the sorted ``pos``); without such
  a record it keeps its own.
"""
from __future__ import annotations

import numpy as np

import fast_twin
from apply_ref import DE, DU, IN, IV, SN, TL, TLI
from mutation_simulator_amd import _ffi

TAG_GT = 20
TWO53 = 1 << 53
U64 = np.uint64


def ceil_scaled(f: float) -> int:
    """ceil(f * 2**53), exactly."""
    num, den = float(f).as_integer_ratio()
    return -((-num * TWO53) // den)


def draw_source(recs: np.ndarray) -> np.ndarray:
    """Per record the index of the record whose draw it takes: its own, or its TL's for a linked TLI."""
    n = len(recs)
    src = np.arange(n, dtype=np.int64)
    if not n:
        return src
    pos = recs["pos"].astype(np.int64)
    tli = np.flatnonzero(recs["type"] == TLI)
    j = np.searchsorted(pos, recs["extra"][tli].astype(np.int64))
    jc = np.minimum(j, n - 1)
    ok = (j < n) & (pos[jc] == recs["extra"][tli]) & (recs["type"][jc] == TL)
    src[tli[ok]] = j[ok]
    return src


def genotypes(recs: np.ndarray, key: int, seq: int, het_thr: int) -> np.ndarray:
    v = fast_twin.draw4(key, seq, draw_source(recs), 0, TAG_GT)
    het = (fast_twin.lo64(v) >> U64(11)) < U64(het_thr)
    second = (fast_twin.hi64(v) & U64(1)) == U64(1)
    return np.where(het, np.where(second, 2, 1), 3).astype(np.uint8)


def linked_table(n: int, seed: int, L: int):
    """``n`` records of every type in position order on a contig of ``L`` bases, TL / TLI pairs among them (a TLI in front of
    its TL and behind it), one TLI whose ``extra`` is no record's position, one whose ``extra`` is the position of a record that
    is no TL.  Returns (recs, pool, indices of linked (TLI, TL) pairs, indices of the two unlinked TLIs)."""
    rs = np.random.RandomState(seed)
    step = L // (n + 2)
    assert step >= 40
    rows, pool = [], bytearray()
    kinds = [SN, SN, SN, IN, DE, DU, IV, SN, SN]
    pos = [step * (i + 1) + int(rs.randint(0, 8)) for i in range(n)]
    pairs_at = set(range(50, n - 50, 97))                  # record i: a TL, record i + 7 (or i - 7): its TLI
    role = {}
    for q, i in enumerate(sorted(pairs_at)):
        role[i] = ("TL", None)
        role[i + 7 if q % 2 == 0 else i - 7] = ("TLI", i)
    lone, wrong = 20, 30                                   # TLIs without a TL: extra hits nothing / hits an SNP's position
    role[lone] = ("TLI_none", None)
    role[wrong] = ("TLI_wrong", 29)
    for i in range(n):
        p = pos[i]
        kind, link = role.get(i, (None, None))
        if kind == "TL":
            rows.append((p, p + 9, 0, TL, 0, 0))
        elif kind == "TLI":
            rows.append((p, pos[link] + 9, pos[link], TLI, (i & 1) | 2, 0))
        elif kind == "TLI_none":
            rows.append((p, pos[5] + 20, pos[5] + 11, TLI, 2, 0))       # (pos[5] + 11: between two records)
        elif kind == "TLI_wrong":
            rows.append((p, pos[link] + 9, pos[link], TLI, 2, 0))
        else:
            t = SN if i == 29 else kinds[int(rs.randint(0, len(kinds)))]
            if t == SN:
                rows.append((p, p, 0, SN, 0, 0))
            elif t == IN:
                k = 1 + int(rs.randint(0, 12))
                rows.append((p, p + k - 1, len(pool), IN, 0, 0))
                pool += bytes(b"ACGT"[x] for x in rs.randint(0, 4, k))
            else:
                rows.append((p, p + 1 + int(rs.randint(0, 12)), 0, t, 0, 0))
    recs = np.array(rows, dtype=_ffi.RECORD_DTYPE).reshape(-1)
    pairs = [(j, link) for j, (kind, link) in role.items() if kind == "TLI"]
    return recs, np.frombuffer(bytes(pool), dtype=np.uint8).copy(), pairs, (lone, wrong)


DRAW_CASES = [(key, seq, thr) for key in (0x0123456789ABCDEF, 0xF00DFACE12345678) for seq in (0, 7)
              for thr in (0, TWO53, ceil_scaled(0.3))]


def check_draw(got: np.ndarray, recs: np.ndarray, pairs, unlinked, key: int, seq: int, het_thr: int):
    want = genotypes(recs, key, seq, het_thr)
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert got.min() >= 1 and got.max() <= 3
    if het_thr == 0:
        assert (got == 3).all()
    if het_thr == TWO53:
        assert not (got == 3).any()
    for tli, tl in pairs:
        assert got[tli] == got[tl], (tli, tl)
    own = fast_twin.draw4(key, seq, np.array(unlinked), 0, TAG_GT)      # the unlinked TLIs keep their own draw
    het = (fast_twin.lo64(own) >> U64(11)) < U64(het_thr)
    assert np.array_equal(got[list(unlinked)], np.where(het, np.where((fast_twin.hi64(own) & U64(1)) == U64(1), 2, 1), 3))
