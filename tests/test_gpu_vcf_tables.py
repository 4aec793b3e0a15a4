"""The device VCF renderer (csrc/text_gpu.hip: k_vcf_lines<.., ALL_SNP, GT>, k_vcf_plain, k_len_*, k_scan_u64) on HAND-BUILT
record tables.

Every other GPU test reaches these kernels behind a planner -- the lengths, text offsets and source addresses they see are
whatever the draws give -- and compares with the project's own host renderer.  Here the tables are made by construction
(``tests/vcf_tables.py``; what each one covers is asserted in ``tests/test_vcf_ref_host.py`` from the expected text alone) and
every rendered text is compared, byte for byte, with ``tests/vcf_ref.py`` -- the plain restatement of the reference's lines that
the same file pins to the real reference's bytes.  Each table goes through ``set_records`` (so it passed the library's table
check) and is rendered under each of its names, first with the haploid sample column, then -- ``set_genotypes``, bytes 1, 2, 3
cycling by record -- with the phased one.  All comparisons are exact.
"""
from __future__ import annotations

import bisect
import hashlib

import numpy as np
import pytest

import vcf_ref
import vcf_tables
from mutation_simulator_amd import _ffi
from test_gpu_apply_tables import NAMES
from vcf_tables import expected, tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def explain(got: bytes, want: bytes, body, recs, bases, pool, name):
    """The first differing byte: its line, record, type, text offset mod 16, and whether it lies inside the 16-byte-aligned
    interior of a REF / ALT copy (the part the whole wave copies source -> text) or in what the stage holds."""
    n = min(len(got), len(want))
    bad = np.nonzero(np.frombuffer(got, dtype=np.uint8)[:n] != np.frombuffer(want, dtype=np.uint8)[:n])[0]
    if not len(bad):
        return f"lengths differ: {len(got)} != {len(want)}, equal up to the shorter one"
    d = int(bad[0])
    starts, at = [], 0
    for l in body:
        starts.append(at)
        at += len(l)
    rec = bisect.bisect_right(starts, d) - 1
    while not body[rec]:
        rec -= 1
    line = sum(1 for l in body[:rec] if l)
    where = "the stage's part (fields, short copies, edges)"
    for c in vcf_ref.copies(bases, recs, pool, name, body=body):
        if c.offset <= d < c.offset + c.length:
            r = vcf_tables.interior(c)
            where = f"{c.kind} copy of {c.length} at text offset {c.offset} (mod 16: {c.offset % 16}), source index {c.source} (mod 16: {c.source % 16}), " + \
                    ("inside its aligned interior" if r and r[0] <= d < r[1] else "in front of its aligned interior" if r and d < r[0] else
                     "behind its aligned interior" if r else "which has no interior")
    r = recs[rec]
    return (f"first difference at text offset {d} (mod 16: {d % 16}; {len(bad)} bytes differ, lengths {len(got)} / {len(want)}): "
            f"line {line}, byte {d - starts[rec]} of {len(body[rec])}, record #{rec} (wave {rec // 64}, lane {rec % 64}) {NAMES[int(r['type'])]} pos={r['pos']} "
            f"stop={r['stop']} extra={r['extra']} aux={r['aux']}; {where}; got {got[d:d + 12]!r} want {want[d:d + 12]!r}")


def render_both(eng, key, case, want):
    """One table: installed once, rendered under every name without and with genotypes."""
    bases, recs, pool, names, gt = case
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, recs, pool)
    for genotyped in (False, True):
        if genotyped:
            eng.set_genotypes(cid, gt)
        for name in names:
            body = vcf_ref.rename(want[1 if genotyped else 0], names[0], name)
            text = b"".join(body)
            got = eng.render_vcf_device(cid, name).tobytes()
            assert got == text, f"{key}, name of {len(name)} bytes, {'with' if genotyped else 'no'} genotypes: " + \
                explain(got, text, body, recs, bases, pool, name)
    eng.clear()


def run_part(eng, part):
    want = expected(part)
    for key, case in tables(part).items():
        render_both(eng, key, case, want[key])


# ------------------------------------------------------------------------------ a - e
def test_copy_geometry_grid(eng):
    """(a) Every copy kind x 18 lengths x 16 source residues under 16 names: ~2000 records per render, 32 renders."""
    run_part(eng, "grid")


@pytest.mark.parametrize("part", ["group_limit", "group_limit_snp", "long_in_wave", "long_wave", "name_edges"])
def test_stage_groups(eng, part):
    """(b) The 4096-byte group cut at every phase (general and SNP-only kernel), a 15 kB line at lane 0 / 31 / 63 / opening a second group, a wave of 64 long
    lines, names around the workgroup's 64-byte copy and around VCF_MAX_NAME -- mixed and SNP-only tables."""
    run_part(eng, part)


@pytest.mark.parametrize("part", ["sizes", "suppressed"])
def test_table_sizes_and_suppressed_lines(eng, part):
    """(c) 1 .. 2049 records as SNP-only and as mixed tables; lines suppressed by each route at lane 0, the last valid lane,
    over a wave, a workgroup, every other line and the whole table (no text at all)."""
    run_part(eng, part)
    if part == "suppressed":
        eng.clear()
        bases, recs, pool, names, gt = tables(part)["suppress_snp_on_n_table"]
        cid = eng.add_contig(bases)
        eng.set_records(cid, recs, pool)
        assert len(eng.render_vcf_device(cid, names[0])) == 0
        eng.clear()


def test_contig_edges(eng):
    """(d) Every type at 0 and ending at L - 1, on contigs of 1, 2, 16, 17 and 4099 bases: the 16-byte loads that reach into the
    pads in front of and behind the contig and the pool; the one-base contig whose deletion has no line."""
    run_part(eng, "edges")


def test_digit_counts(eng):
    """(e) POS, END, SVLEN across 9 -> 10 ... 9 999 999 -> 10 000 000 (the SVLEN pair as two linked spans of 10 Mb: 22 MB of
    text), and POS / END across 10^8 on a contig of 100 000 016 bases.  Ten digits and SSink::num's >= 4e9 branch stay with the
    full-size tier (tests/test_gpu_fullsize.py)."""
    run_part(eng, "digits")


# ------------------------------------------------------------------------------ f. more than 1024 length blocks
@pytest.mark.parametrize("key", ["blocks_snp", "blocks_de"])
def test_more_than_1024_length_blocks(eng, key):
    """1024 x 2048 + 2049 records: k_scan_u64's second round of 1024 block sums and the carry between the rounds, 64-bit
    offsets behind it; as an SNP-only table and -- the last record a 1-base DE -- through the general kernel."""
    case = vcf_tables.tables_blocks()[key]
    bases, recs, pool, names, gt = case
    eng.clear()
    cid = eng.add_contig(bases)
    eng.set_records(cid, recs, pool)
    for g in (None, gt):
        if g is not None:
            eng.set_genotypes(cid, gt)
        want = vcf_tables.blocks_text(case, names[0], g)
        got = eng.render_vcf_device(cid, names[0]).tobytes()
        if len(got) != len(want) or hashlib.sha256(got).digest() != hashlib.sha256(want).digest():
            a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            n = min(len(a), len(b))
            bad = np.nonzero(a[:n] != b[:n])[0]
            d = int(bad[0]) if len(bad) else n
            raise AssertionError(f"{key}: lengths {len(got)} / {len(want)}, {len(bad)} bytes differ, first at text offset {d} "
                                 f"(line {want[:d].count(10)}): got {got[d:d + 24]!r} want {want[d:d + 24]!r}")
    eng.clear()


# ------------------------------------------------------------------------------ g. the plain path
@pytest.mark.parametrize("part", vcf_tables.PLAIN_PARTS)
def test_plain_path(eng, part, monkeypatch):
    """(a) and (d) once more through k_vcf_plain (every lane writes its own line byte by byte), forced by the test hook."""
    monkeypatch.setenv("MSIM_DBG_VCF_PLAIN", "1")
    run_part(eng, part)
