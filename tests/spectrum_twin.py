"""numpy restatement of the context-dependent SNP engine (``--spectrum``; include/msim.h: msim_context_counts,
msim_plan_contig_spectrum), written from its rules over ``fast_twin``'s Philox -- test infrastructure shared by the CPU and
the GPU tier.  The library (device kernels and host restatements alike) and ``mutation_simulator_amd.spectrum`` must agree
with it bit for bit.

* census: bases as the context holds them; ``code(A, C, G, T) = 0, 1, 2, 3``, every other byte invalid; site ``p`` is eligible iff
  ``1 <= p <= L - 2`` and ``b[p-1], b[p], b[p+1]`` are valid; ``ctx = 16 code(b[p-1]) + 4 code(b[p]) + code(b[p+1])``.
* channel of (ctx, aux): ``ref = b[p]``; ``alt`` = the rewrite's base for aux 0 (transition), 1 / 2 (transversion columns 0 / 1);
  ``l[ref>alt]r`` for a pyrimidine ``ref``, else the reverse complement ``comp(r)[comp(ref)>comp(alt)]comp(l)``.
* ``p(ctx, aux) = RATE * n_valid * w[channel] / W / (counts[ctx] + counts[rc(ctx)])``, 0 where ``counts[ctx] = 0``, in
  ``fractions.Fraction`` over the doubles; ``thr[3 ctx + j] = min(2**64 - 1, floor(2**64 * sum_{i <= j} p(ctx, i)))``; a
  context that occurs with ``sum p > 1`` is refused.
* draw: ``v = draw4(key, seq, x = p >> 1, y = 0, tag 21)``; ``r`` = the high 64 bits for an odd ``p``, the low 64 for an even
  one; ``j = #{i : thr[3 ctx + i] <= r}``; ``j == 3``: nothing; else ``{pos = p, stop = p, extra = 0, SN, aux = j, rsv = 0}``.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import fast_twin
from mutation_simulator_amd import _ffi

TAG_CTX = 21
U64 = np.uint64
SN = 1
ACGT = "ACGT"
TWO64 = 1 << 64
SUBS = ["C>A", "C>G", "C>T", "T>A", "T>C", "T>G"]
CHANNELS = [f"{l}[{s}]{r}" for s in SUBS for l in ACGT for r in ACGT]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
TI = {"A": "G", "G": "A", "T": "C", "C": "T"}                        # aux 0
TV = [{"A": "T", "G": "C", "T": "G", "C": "A"},                      # aux 1: column 0
      {"A": "C", "G": "T", "T": "A", "C": "G"}]                      # aux 2: column 1

_CODE = np.full(256, 4, dtype=np.int64)
for _i, _ch in enumerate(ACGT):
    _CODE[ord(_ch)] = _i
# alt[aux][byte]: the byte an SN record writes over a valid base
ALT = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
for _b in ACGT:
    ALT[0][ord(_b)] = ord(TI[_b])
    ALT[1][ord(_b)] = ord(TV[0][_b])
    ALT[2][ord(_b)] = ord(TV[1][_b])


class Refused(Exception):
    def __init__(self, ctx):
        super().__init__(ctx_name(ctx))
        self.ctx = ctx


def as_bases(x) -> np.ndarray:
    return np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype=np.uint8)


def ctx_name(ctx: int) -> str:
    return ACGT[ctx >> 4] + ACGT[(ctx >> 2) & 3] + ACGT[ctx & 3]


def sites(bases):
    """(positions of the eligible sites, their contexts)."""
    b = as_bases(bases)
    L = len(b)
    if L < 3:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    c = _CODE[b]
    ok = (c[:-2] < 4) & (c[1:-1] < 4) & (c[2:] < 4)
    pos = np.flatnonzero(ok) + 1
    ctx = 16 * c[pos - 1] + 4 * c[pos] + c[pos + 1]
    return pos, ctx


def census(bases):
    _, ctx = sites(bases)
    counts = np.bincount(ctx, minlength=64).astype(np.uint64)
    return counts, int(counts.sum())


def rc(ctx: int) -> int:
    l, m, r = ctx >> 4, (ctx >> 2) & 3, ctx & 3
    return 16 * (3 - r) + 4 * (3 - m) + (3 - l)


def channel(ctx: int, aux: int) -> str:
    l, ref, r = ctx_name(ctx)
    alt = TI[ref] if aux == 0 else TV[aux - 1][ref]
    if ref in "CT":
        return f"{l}[{ref}>{alt}]{r}"
    return f"{COMP[r]}[{COMP[ref]}>{COMP[alt]}]{COMP[l]}"


def probabilities(counts, weights, rate):
    """weights: 96 floats in ``CHANNELS`` order.  64 triples of Fraction."""
    w = {name: Fraction(float(x)) for name, x in zip(CHANNELS, weights)}
    W = sum(w.values())
    counts = [int(x) for x in counts]
    n_valid = sum(counts)
    out = []
    for ctx in range(64):
        if counts[ctx] == 0:
            out.append([Fraction(0)] * 3)
            continue
        pooled = counts[ctx] + counts[rc(ctx)]
        out.append([Fraction(float(rate)) * n_valid * w[channel(ctx, aux)] / W / pooled for aux in range(3)])
    return out


def thresholds(counts, weights, rate) -> np.ndarray:
    thr = []
    for ctx, triple in enumerate(probabilities(counts, weights, rate)):
        if sum(triple) > 1:
            raise Refused(ctx)
        for j in range(3):
            thr.append(min(TWO64 - 1, math.floor(sum(triple[:j + 1]) * TWO64)))
    return np.array(thr, dtype=np.uint64)


def outcomes(bases, thr, key: int, seq: int):
    """(eligible positions, their contexts, j per site: 0..2 = aux, 3 = no mutation)."""
    pos, ctx = sites(bases)
    thr = np.asarray(thr, dtype=np.uint64).reshape(64, 3)
    v = fast_twin.draw4(key, seq, (pos >> 1).astype(np.uint64), 0, TAG_CTX)
    r = np.where((pos & 1) == 1, fast_twin.hi64(v), fast_twin.lo64(v))
    j = (thr[ctx] <= r[:, None]).sum(axis=1)
    return pos, ctx, j


def plan(bases, thr, key: int, seq: int) -> np.ndarray:
    pos, _, j = outcomes(bases, thr, key, seq)
    hit = j < 3
    recs = np.zeros(int(hit.sum()), dtype=_ffi.RECORD_DTYPE)
    recs["pos"] = pos[hit]
    recs["stop"] = pos[hit]
    recs["type"] = SN
    recs["aux"] = j[hit]
    return recs


def apply(bases, recs) -> np.ndarray:
    """The contig with every SN record of a spectrum plan written over it (the sites are A, C, G or T)."""
    out = as_bases(bases).copy()
    p = recs["pos"].astype(np.int64)
    out[p] = ALT[recs["aux"].astype(np.int64), out[p]]
    return out


# ---- shared test material ----------------------------------------------------------------------------------------------
def every_site_table() -> np.ndarray:
    """Each context's last threshold is 2**64 - 1: every eligible site mutates; the aux values split three ways."""
    thr = np.zeros((64, 3), dtype=np.uint64)
    thr[:, 0] = U64(TWO64 // 3)
    thr[:, 1] = U64(2 * (TWO64 // 3))
    thr[:, 2] = U64(TWO64 - 1)
    return thr.reshape(-1)


def random_table(rs, density: float) -> np.ndarray:
    """Random non-decreasing triples; a site mutates with probability around ``density`` (between 0.5 and 1.5 times it)."""
    top = (rs.uniform(0.5, 1.5, 64) * density * TWO64).astype(np.float64)
    cut = np.sort(rs.uniform(0, 1, (64, 2)), axis=1)
    thr = np.zeros((64, 3), dtype=np.uint64)
    for x in range(64):
        t = min(int(top[x]), TWO64 - 1)
        thr[x] = np.array([int(cut[x, 0] * t), int(cut[x, 1] * t), t], dtype=np.uint64)
    return thr.reshape(-1)


def skewed_weights() -> list:
    """A 1-to-7 ramp over the 96 channels, N[C>T]G times 20 (CpG transitions dominate, no channel is 0).  The ramp starts at the
    four N[C>T]G channels and goes on through the others in ``CHANNELS`` order: the boosted channels then add the least to the
    sum, which keeps the rarest channel's share at 1.25 / 467 -- 53 expected SNPs among 20 000 (test_spectrum_host.py)."""
    cpg = [i for i, name in enumerate(CHANNELS) if name[2:5] == "C>T" and name[6] == "G"]
    order = cpg + [i for i in range(96) if i not in cpg]
    w = [0.0] * 96
    for rank, i in enumerate(order):
        w[i] = (1.0 + 6.0 * rank / 95.0) * (20.0 if i in cpg else 1.0)
    return w


def spectrum_text(weights, sep="\t", header=("Type", "SBSx"), shuffle_seed=None) -> str:
    rows = [f"{name}{sep}{w!r}" for name, w in zip(CHANNELS, weights)]
    if shuffle_seed is not None:
        np.random.RandomState(shuffle_seed).shuffle(rows)
    head = [sep.join(header)] if header else []
    return "\n".join(head + rows) + "\n"


def random_genome(rs, L: int, n_runs: int = 0, iupac: int = 0) -> np.ndarray:
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, L)].copy()
    for _ in range(n_runs if L > 8 else 0):
        s = int(rs.randint(0, L - 1))
        b[s:s + int(rs.randint(1, max(2, min(300, L // 4))))] = ord("N")
    if iupac and L:
        at = rs.randint(0, L, iupac)
        b[at] = np.frombuffer(b"KSYMWRBDHVNU-", dtype=np.uint8)[rs.randint(0, 13, iupac)]
    return b
