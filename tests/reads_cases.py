"""The cases of the ``reads`` mode's tests, shared by the host tier (``msim_dbg_reads_render`` against the twin) and the GPU tier
(the device against the twin): small genomes, the tables, the ranges to render.  The twin's text of a case is computed once
(``reference``) and left unchanged."""
from __future__ import annotations

import functools

import numpy as np

from mutation_simulator_amd import reads as rd
import reads_twin

ONE53 = 1 << 53
LENS = (1, 2, 63, 64, 65, 127, 128, 129, 150, 512)       # the lane-pair and wave edges of two cycles a lane


def genome(seed: int, *lengths, alphabet=b"ACGT"):
    rs = np.random.RandomState(seed)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    return [letters[rs.randint(0, len(letters), size=n)].copy() for n in lengths]


def even_table(n: int):
    """n fragment lengths of (nearly) equal mass."""
    thr = np.array([(k + 1) * ONE53 // n for k in range(n)], dtype=np.uint64)
    thr[-1] = ONE53
    return thr


class Case:
    def __init__(self, contigs, key, n_reads, length, paired, frag_min, frag_thr, err=(0.02, 0.3), prefix="r", ranges=None,
                 err_thr=None):
        self.contigs, self.key, self.n_reads, self.length, self.paired = contigs, key, n_reads, length, paired
        self.frag_min, self.frag_thr, self.prefix = frag_min, np.asarray(frag_thr, dtype=np.uint64), prefix
        self.err_thr, self.qual = rd.error_tables(length, *err)
        if err_thr is not None:
            self.err_thr = np.full((2, length), err_thr, dtype=np.uint64)
        mates = (0, 1) if paired else (0,)
        self.ranges = ranges if ranges is not None else [(m, 0, n_reads) for m in mates]

    def params(self):
        from mutation_simulator_amd import _ffi
        return _ffi.reads_params(self.key, self.n_reads, self.length, self.paired, self.frag_min, self.frag_thr, self.err_thr,
                                 self.qual, self.prefix)

    def twin(self, mate, first, count) -> bytes:
        return reads_twin.render(self.contigs, self.key, self.n_reads, self.length, self.frag_min, self.frag_thr, self.err_thr,
                                 self.qual, self.prefix, mate, first, count)

    def plan(self) -> reads_twin.Plan:
        return reads_twin.Plan([len(x) for x in self.contigs], self.frag_min, len(self.frag_thr), self.n_reads, self.length, self.prefix)


IUPAC = b"ACGTACGTACGTNRYKMSWBDHVN"


def _iupac_genome():
    g = genome(41, 3000, 2500, alphabet=IUPAC)
    g[0][700:1400] = ord("N")                          # an assembly gap longer than any fragment: reads of N alone
    g[1][:300] = ord("N")
    g[1][-200:] = ord("N")
    return g


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {}
    for n in LENS:                                     # single-end and paired at every edge length; 700 reads: several workgroups, a ragged last one
        out[f"se_len{n}"] = Case(genome(n, 4000, 2777), 1000 + n, 700, n, False, n, [ONE53], prefix="se.")
        fmin, thr = rd.fragment_table(n, True, n + 60, 15)
        out[f"pe_len{n}"] = Case(genome(100 + n, 3001, 5003), 2000 + n, 700, n, True, fmin, thr, prefix="pe-")
    # the counter's top and the 10-digit index field
    out["top_of_counter"] = Case(genome(7, 2000), 77, 2**32 - 1, 50, True, 60, even_table(5),
                                 ranges=[(0, 2**32 - 5, 5), (1, 2**32 - 5, 5)])
    # contigs: shorter ones first, in the middle and last (excluded; the numbering follows the Fasta), one exactly fmax long (a
    # single start), one a little longer -- some read starts at len - fmax with f = fmax and touches its contig's last base
    out["contig_edges"] = Case(genome(8, 100, 306, 50, 346, 200), 88, 3000, 100, True, 300, even_table(7), prefix="edge_")
    out["iupac"] = Case(_iupac_genome(), 99, 2000, 100, True, 100, even_table(150), prefix="n")
    out["frag_1"] = Case(genome(9, 3000), 91, 1500, 75, True, 75, [ONE53])                    # f = LEN: the mates overlap fully
    out["frag_4096"] = Case(genome(10, 6000, 300), 92, 1500, 50, True, 50, even_table(4096))
    out["frag_7_all"] = Case(genome(11, 5000), 93, 20000, 36, False, 36, even_table(7), err=(0.0, 0.0))
    out["err_none"] = Case(genome(12, 2500, 1800), 94, 2000, 90, True, 90, even_table(40), err=(0.0, 0.0))
    out["err_all"] = Case(_iupac_genome(), 95, 2000, 90, True, 90, even_table(40), err_thr=ONE53)
    out["stride_even"] = Case(genome(13, 4000), 96, 1100, 101, False, 101, [ONE53], prefix="r")     # 228 bytes a record
    out["stride_odd"] = Case(genome(14, 4000), 97, 1100, 101, False, 101, [ONE53], prefix="rr")     # 229
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """The twin's text of every range of the case: a tuple of bytes, in the order of ``ranges``."""
    c = cases()[name]
    return tuple(c.twin(m, first, count) for m, first, count in c.ranges)


def parse_records(text: bytes, stride: int, prefix: str):
    """Every record as (index, contig number, 1-based start, fragment length, strand, mate, bases, quals)."""
    assert len(text) % stride == 0
    out = []
    for k in range(0, len(text), stride):
        name, seq, plus, ql, rest = text[k:k + stride].split(b"\n")
        assert plus == b"+" and rest == b"" and name.startswith(b"@" + prefix.encode())
        body, mate = name[1 + len(prefix):].split(b"/")
        i, c, s, f, strand = body.split(b"_")
        out.append((int(i), int(c), int(s), int(f), strand.decode(), int(mate), seq, ql))
    return out


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def clean(b: bytes) -> bytes:
    """A, C, G, T kept, every other byte 'N'."""
    return bytes(ch if ch in b"ACGT" else ord("N") for ch in b)


def expected_bases(contigs, c, s, f, strand, mate, length) -> bytes:
    """The error-free bases of a record from its name alone, the way a reader of the documentation would compute them."""
    frag = clean(contigs[c - 1][s - 1:s - 1 + f].tobytes())
    assert len(frag) == f
    if strand == "-":
        frag = frag.translate(_COMP)[::-1]
    return frag[:length] if mate == 1 else frag[-length:].translate(_COMP)[::-1]
