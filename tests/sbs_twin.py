"""numpy restatement of the SBS-96 profile (``msim_sbs_counts``; include/msim.h), written from its rules over
``spectrum_twin``'s channel naming -- test infrastructure shared by the CPU and the GPU tier.  The device kernel, the library's
sequential restatement (``msim_dbg_sbs_counts``) and ``mutation_simulator_amd.spectrum.CHANNEL_OF`` must agree with it exactly.

* an SN record at ``p`` of a contig ``b[0..L)`` has a channel iff ``1 <= p <= L - 2`` and ``b[p-1], b[p], b[p+1]`` are each A, C, G
  or T; then ``ctx = 16 code(b[p-1]) + 4 code(b[p]) + code(b[p+1])`` and the channel is the one ``spectrum_twin.channel(ctx, aux)``
  names, indexed in ``CHANNELS`` order.  The context is the reference's: records do not see each other.
* ``tallies[0]``: SN records without a channel; ``tallies[t]``, t = 1..7: records of type t.

The shapes at the end are the smallest at which the kernel can still go wrong; both tiers run them.
"""
from __future__ import annotations

import functools

import numpy as np

import spectrum_twin as tw
from mutation_simulator_amd._ffi import RECORD_DTYPE

SN = 1
INDEX = np.array([[tw.CHANNELS.index(tw.channel(ctx, aux)) for aux in range(3)] for ctx in range(64)], dtype=np.int64)
NON_ACGT = "NRYKMSWBDHVU-"
NO_POOL = np.zeros(0, dtype=np.uint8)


def counts(bases, recs):
    """(channels uint64[96], tallies uint64[8]) of a record table over a contig's bases."""
    b = tw.as_bases(bases)
    L = len(b)
    channels = np.zeros(96, dtype=np.uint64)
    tallies = np.zeros(8, dtype=np.uint64)
    for t in range(1, 8):
        tallies[t] = int((recs["type"] == t).sum())
    sn = recs[recs["type"] == SN]
    p = sn["pos"].astype(np.int64)
    ok = (p >= 1) & (p <= L - 2)
    q, aux = p[ok], sn["aux"][ok].astype(np.int64)
    code = tw._CODE[b]
    l, m, r = code[q - 1], code[q], code[q + 1]
    valid = (l < 4) & (m < 4) & (r < 4)
    ctx = 16 * l[valid] + 4 * m[valid] + r[valid]
    channels += np.bincount(INDEX[ctx, aux[valid]], minlength=96).astype(np.uint64)
    tallies[0] = len(sn) - int(valid.sum())
    return channels, tallies


def snp_table(pos, aux) -> np.ndarray:
    pos = np.asarray(pos, dtype=np.uint32)
    recs = np.zeros(len(pos), dtype=RECORD_DTYPE)
    recs["pos"] = recs["stop"] = pos
    recs["type"] = SN
    recs["aux"] = aux
    return recs


# ---- shared shapes: {case id: (bases, recs, pool)} ----------------------------------------------------------------------
def short_contigs():
    """L = 1, 2, 3 with an SN at every position: only L = 3, p = 1 has a channel (the neighbour reads at both ends)."""
    return {f"short_L{L}": (np.frombuffer(b"GCA"[:L], dtype=np.uint8), snp_table(np.arange(L), np.arange(L) % 3), NO_POOL)
            for L in (1, 2, 3)}


def de_bruijn() -> np.ndarray:
    """A de Bruijn word of order 3 over ACGT, linearised: 66 bases, every trinucleotide exactly once."""
    k, n = 4, 3
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    word = seq + seq[:2]
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.array(word)].copy()


def every_context():
    """Three tables over the de Bruijn word: aux 0, 1 and 2 at every eligible site (1..64)."""
    bases = de_bruijn()
    return {f"every_context_aux{aux}": (bases, snp_table(np.arange(1, 65), aux), NO_POOL) for aux in range(3)}


def non_acgt():
    """N, IUPAC, U or - at p - 1, p and p + 1 of the one record in turn."""
    out = {}
    for ch in NON_ACGT:
        for off in (-1, 0, 1):
            bases = np.frombuffer(b"ACGTTGCATGCA", dtype=np.uint8).copy()
            bases[5 + off] = ord(ch)
            out[f"non_acgt_{'dash' if ch == '-' else ch}_{off + 1}"] = (bases, snp_table([5], (off + 1) % 3), NO_POOL)
    return out


def every_type():
    """A table holding every record type among SN records, on a genome rich in ambiguity codes (tests/vcf_tables.py)."""
    import vcf_tables
    out = {}
    for key in ("size_mixed_257", "size_mixed_2049"):
        bases, recs, pool = vcf_tables.tables("sizes")[key][:3]
        assert set(np.unique(recs["type"]).tolist()) == set(range(1, 8))
        out[f"every_type_{key}"] = (bases, recs, pool)
    return out


def split_counts(B: int):
    return [0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1]


def work_split(B: int):
    """Record counts around the wave (64) and the workgroup's pass (B) on random genomes with N runs and ambiguity codes."""
    out = {}
    for n in split_counts(B):
        rs = np.random.RandomState(9000 + n)
        L = 3 * n + 40
        bases = tw.random_genome(rs, L, n_runs=3, iupac=L // 50)
        pos = np.sort(rs.permutation(L)[:n])                          # (the first and the last base included, now and then)
        out[f"split_{n}"] = (bases, snp_table(pos, rs.randint(0, 3, n)), NO_POOL)
    return out


ONE_CHANNEL_N = (1 << 20) + 1


@functools.lru_cache(maxsize=None)
def one_channel():
    """ACG repeated with an aux 0 record on every C: 2^20 + 1 records, all of them A[C>T]G."""
    bases = np.tile(np.frombuffer(b"ACG", dtype=np.uint8), ONE_CHANNEL_N)
    return bases, snp_table(3 * np.arange(ONE_CHANNEL_N, dtype=np.int64) + 1, 0), NO_POOL


def small_cases(B: int):
    out = {}
    for part in (short_contigs(), every_context(), non_acgt(), every_type(), work_split(B)):
        out.update(part)
    return out
