"""``tests/vcf_ref.py`` -- the plain restatement of the reference's VCF lines that ``tests/test_gpu_vcf_tables.py`` holds the
device renderer to -- against bytes the real reference produced, the host renderer (``msim_render_vcf`` / ``msim_render_vcf_gt``,
csrc/render.cpp) against ``vcf_ref`` on every hand-built table of ``tests/vcf_tables.py``, and the coverage those tables
promise.  Coverage is a function of the expected text alone, so all of it is checked here, without a GPU; each condition
names the single-constant error of csrc/text_gpu.hip it is there to catch.
"""
from __future__ import annotations

import contextlib
import io
import random

import numpy as np
import pytest

import apply_ref
import vcf_ref
import vcf_tables
from apply_ref import DE, DU, IN, IV, SN, TL, TLI
from helpers import CASES, all_case_names, case_meta, load_json, mask_vcf, sha256
from mutation_simulator_amd import _ffi
from vcf_tables import STAGE, expected, tables

APPLY = load_json("apply.json")


# ------------------------------------------------------------------------------ 1. against the real reference's bytes
@pytest.mark.parametrize("case", APPLY["cases"], ids=lambda c: c["name"])
def test_vcf_ref_equals_reference_on_apply_goldens(case):
    """apply_ref.golden_table ends a DE / DU / IV with the sequence (what APPLY needs); the reference's END and SVLEN are
    those of the mutation list's own stop, so the stops are put back for the lines."""
    recs, pool = apply_ref.golden_table(case)
    stops = {start: stop for name, start, stop in case["muts"] if name in ("DE", "DU", "IV")}
    for i in np.nonzero(np.isin(recs["type"], (DE, DU, IV)))[0]:
        recs["stop"][i] = stops[int(recs["pos"][i])]
    bases = np.frombuffer(case["sequence"].encode(), dtype=np.uint8).copy()
    want = [l.encode() + b"\n" for l in case["vcf_body"]]
    name = want[0].split(b"\t")[0] if want else b"x"
    got = vcf_ref.lines(bases, recs, pool, name)
    assert [l for l in got if l] == want
    assert _ffi.render_vcf(recs, pool, bases, name.decode()) == b"".join(want)
    text = b"".join(want)
    for c in vcf_ref.copies(bases, recs, pool, name):                 # (the geometry helper on the reference's own text)
        src = pool if c.kind == "IN" else bases
        first = text[c.offset:c.offset + 1]
        assert first == (bytes(src[c.source:c.source + 1]) if vcf_ref.COPY_MODE[c.kind] == vcf_ref.RAW else
                         bytes(src[c.source:c.source + 1]).translate(vcf_ref.CONV).translate(vcf_ref.COMP if c.kind.endswith(("ALT", "REV")) else None))


def _with_vcf(name):
    meta = case_meta(name)
    return meta.get("sim") is not None and meta["exception"] is None and "vcf_len" in meta


CLI_CASES = [n for n in all_case_names() if _with_vcf(n)]


def test_the_translocation_goldens_are_among_the_cli_cases():
    assert {"readme_mix_tl", "tl_heavy", "tl_rmt"} <= set(CLI_CASES)


@pytest.mark.parametrize("name", CLI_CASES)
def test_vcf_ref_equals_reference_on_cli_goldens(name, tmp_path):
    """settings -> msim_plan_contig (host-only context) -> the record table the planner leaves -> vcf_ref.lines, contig by
    contig, == the VCF the real reference wrote (the route of test_cabi_host.py::test_host_planner_vcf_matches_reference
    with vcf_ref in the host renderer's place)."""
    import mutation_simulator_amd as msa
    from mutation_simulator_amd import mutator as msa_mutator
    from pipeline import build_settings, prepare
    meta = case_meta(name)
    argv = prepare(meta, tmp_path)
    with contextlib.redirect_stderr(io.StringIO()):
        args, fasta, sim = build_settings(argv)
    random.seed(meta["seed_py"])
    np.random.seed(meta["seed_np"])
    eng = _ffi.Engine(device=-1)
    msa_mutator.export_python_streams(eng)
    eng.set_params(msa_mutator.params_descriptor(sim))
    vw = msa.VcfWriter(tmp_path / "ref.vcf")
    vw.write_header(args.infile.name, fasta, sim.assembly_name, sim.species_name, sim.sample_name)
    full = meta["store"] == "full"
    body = b""
    if full:
        golden = (CASES / name / "expected_ms.vcf").read_bytes()
        body = golden[golden.index(b"\n", golden.index(b"\n#CHROM") + 1) + 1:]
    at = n_tli = 0
    for chrom in sim.chromosomes:
        rec = fasta[chrom.number]
        cid = eng.add_contig(rec.bases)
        eng.plan_contig(cid, msa_mutator.plan_descriptors(chrom))
        recs, pool = eng.fetch_records(cid)
        text = b"".join(vcf_ref.lines(rec.bases, recs, pool, rec.name))
        if full:
            assert text == body[at:at + len(text)], f"contig {rec.name}"
            at += len(text)
        n_tli += int((recs["type"] == TLI).sum())
        vw.write_raw(text)
        eng.clear()
    vw.close()
    vcf = mask_vcf((tmp_path / "ref.vcf").read_bytes())
    assert len(vcf) == meta["vcf_len"] and sha256(vcf) == meta["vcf_sha256"]
    assert not full or at == len(body)
    if name in ("readme_mix_tl", "tl_heavy", "tl_rmt"):
        assert n_tli > 0


# ------------------------------------------------------------------------------ 2. the host renderer on the hand-built tables
@pytest.fixture(scope="module")
def host_eng():
    e = _ffi.Engine(device=-1)
    yield e
    e.close()


@pytest.mark.parametrize("part", vcf_tables.PARTS)
def test_host_renderer_equals_vcf_ref(host_eng, part):
    """Every table under every one of its names, with the haploid and with the genotype column; every table is one the
    library installs (check_record_table passes)."""
    want = expected(part)
    for key, (bases, recs, pool, names, gt) in tables(part).items():
        host_eng.clear()
        host_eng.set_records(host_eng.add_contig(bases), recs, pool)
        for name in names:
            for g, body in ((None, want[key][0]), (gt, want[key][1])):
                text = b"".join(vcf_ref.rename(body, names[0], name))
                assert _ffi.render_vcf_gt(recs, g, pool, bases, name) == text, (key, len(name), g is not None)
            assert _ffi.render_vcf(recs, pool, bases, name) == b"".join(vcf_ref.rename(want[key][0], names[0], name)), key
    host_eng.clear()


def test_one_base_contig_deleted_has_no_line():
    """DE / TL at 0 on a contig of ONE base: REF = seq[0:2] = the base, ALT = REF[-1] -- equal, and the writer drops the line
    (vcf_writer.py:123).  On every longer contig REF has two bytes at least."""
    for key in ("edge_L1_head_DE", "edge_L1_head_TL"):
        assert expected("edges")[key][0] == [b""]
    for key in ("edge_L2_whole_DE", "edge_L2_almost_TL", "edge_L17_whole_TL"):
        assert all(expected("edges")[key][0])


@pytest.mark.parametrize("key", ["blocks_snp", "blocks_de"])
def test_host_renderer_on_more_than_1024_length_blocks(key):
    case = vcf_tables.tables_blocks()[key]
    bases, recs, pool, names, gt = case
    assert len(recs) == 1024 * 2048 + 2049 and (recs["type"][-1] == DE) == (key == "blocks_de")
    assert _ffi.render_vcf(recs, pool, bases, names[0]) == vcf_tables.blocks_text(case, names[0])
    assert _ffi.render_vcf_gt(recs, gt, pool, bases, names[0]) == vcf_tables.blocks_text(case, names[0], gt)


@pytest.mark.parametrize("key", ["size_snp_2049", "suppress_snp_on_n_alternating", "suppress_snp_on_n_table", "names_snp"])
def test_vectorised_snp_text_equals_lines(key):
    """vcf_ref.snp_text (the expected text of the two tables above) is ``lines`` joined."""
    part = {"si": "sizes", "su": "suppressed", "na": "name_edges"}[key[:2]]
    bases, recs, pool, names, gt = tables(part)[key]
    assert vcf_ref.snp_text(bases, recs, names[0]) == b"".join(expected(part)[key][0])
    assert vcf_ref.snp_text(bases, recs, names[0], gt) == b"".join(expected(part)[key][1])
    big = tables("digits")["digits_100M"][0]                           # POS 9, 10, 99, 100 ... 10^8: transitions, some on codes
    snps = np.zeros(16, dtype=_ffi.RECORD_DTYPE)
    snps["pos"] = snps["stop"] = [10 ** k - 2 + j for k in range(1, 9) for j in (0, 1)]
    snps["type"] = SN
    assert vcf_ref.snp_text(big, snps, "d") == b"".join(vcf_ref.lines(big, snps, np.zeros(0, np.uint8), "d"))


# ------------------------------------------------------------------------------ 3. coverage
def _copies(part, key, name=None, genotyped=False):
    bases, recs, pool, names, gt = tables(part)[key]
    name = names[0] if name is None else name
    body = vcf_ref.rename(expected(part)[key][1 if genotyped else 0], names[0], name)
    return body, vcf_ref.copies(bases, recs, pool, name, body=body)


def test_coverage_copy_geometry_grid():
    """(a) What the grid promises, per copy kind (REF / ALT of every type, the three modes of vcf_unit_load / _store):
    - every (kind, length, text offset mod 16): ``len <= VCF_INLINE`` against ``<`` (25 / 26 at every residue), the rounding
      of a copy's interior [ia, ib) (lengths 15..17, 31..33, 47..49 around one, two, three units; at 26..31 an interior
      exists at some residues only), the edges' stage position in front of and behind the gap;
    - per mode all 16 x 16 (source index mod 16, text offset mod 16) at a length >= 48: the unaligned 16-byte load against the
      aligned store, for the reversed mode the load that ends at the source byte;
    - a DU of >= 26 bases whose second ALT copy starts on a 16-byte text boundary: both ALT copies' gaps open in front of the
      SAME stage unit -- a plain store in place of gs[]'s atomicAdd loses one of them."""
    bases, recs, pool, names, gt = tables("grid")["grid"]
    assert [len(n) for n in names] == list(range(4, 20)) and len(recs) == 16 * (18 * 7 - 2 + 1)
    seen, pairs, shared = set(), {m: set() for m in (vcf_ref.RAW, vcf_ref.CONVERTED, vcf_ref.REVCOMP)}, 0
    for name in names:
        body, cs = _copies("grid", "grid", name)
        assert all(body)
        for c in cs:
            seen.add((c.kind, c.length, c.offset % 16))
            if c.length >= 48:
                pairs[vcf_ref.COPY_MODE[c.kind]].add((c.source % 16, c.offset % 16))
            shared += c.kind == "DU_ALT2" and c.length >= 26 and c.offset % 16 == 0
    want = {(kind, n, t) for kind in vcf_ref.COPY_MODE for n in vcf_tables.GRID_LENGTHS for t in range(16)
            if not (n == 1 and kind in ("DE_REF", "TL_REF"))}           # (a deletion's REF holds the anchor base: two bytes at least)
    assert not want - seen, sorted(want - seen)[:10]
    for mode, got in pairs.items():
        assert len(got) == 256, (mode, len(got))
    assert shared >= 1
    seq = bases.tobytes()                                             # the three modes give different bytes on the genome
    span = seq[4096:4096 + 64]
    assert len({span, span.translate(vcf_ref.CONV), span[::-1].translate(vcf_ref.CONV).translate(vcf_ref.COMP)}) == 3
    assert b"U" in seq and span.translate(vcf_ref.CONV)[::-1] != span[::-1].translate(vcf_ref.CONV).translate(vcf_ref.COMP)


def test_coverage_stage_groups():
    """(b) The group cut ``cp - cp_lo + phase <= VCF_STAGE`` (against ``<``, against a cut that forgets the phase): the second
    wave's 64 lines total 4095, 4096, 4097 minus its phase, for every phase; none of its copies has an interior, so its
    compact text is its text.  A 15 kB line at lane 0, 31, 63 and opening a second group; a wave of 64 long lines."""
    seen = set()
    for key, (bases, recs, pool, names, gt) in tables("group_limit").items():
        body, cs = _copies("group_limit", key)
        assert all(body) and len(body) == 128 and not any(vcf_tables.interior(c) for c in cs)
        phase, total = sum(map(len, body[:64])) % 16, sum(map(len, body[64:]))
        assert key == f"limit_phase{phase}_{total}"
        seen.add((phase, total - (STAGE - phase)))
        groups = [g for g in vcf_tables.stage_groups(body, cs) if g[0] == 1]
        assert len(groups) == (1 if phase + total <= STAGE else 2), key
    assert seen == {(ph, d) for ph in range(16) for d in (-1, 0, 1)}
    seen = set()
    for key, (bases, recs, pool, names, gt) in tables("group_limit_snp").items():      # k_vcf_lines<.., ALL_SNP>: phase + stretch <= VCF_STAGE
        body = expected("group_limit_snp")[key][0]
        assert all(body) and len(body) == 128 and np.all(recs["type"] == SN)
        phase, total = sum(map(len, body[:64])) % 16, sum(map(len, body[64:]))
        assert key == f"snplimit_phase{phase}_{total}"
        seen.add((phase, total - (STAGE - phase)))
    assert seen == {(ph, d) for ph in range(16) for d in (-1, 0, 1)}
    for key, lane in (("long_lane0", 0), ("long_lane31", 31), ("long_lane63", 63), ("long_second_group", 32)):
        bases, recs, pool, names, gt = tables("long_in_wave")[key]
        body, cs = _copies("long_in_wave", key)
        assert len(recs) == 64 and recs["type"][lane] == DU and (recs["type"] == DU).sum() == 1 and 15_000 < len(body[lane]) < 15_200
        groups = vcf_tables.stage_groups(body, cs)
        if key == "long_second_group":
            assert sum(map(len, body[:32])) == STAGE and groups[0] == (0, 0, 32) and groups[1][1] == 32
        else:
            assert groups == [(0, 0, 64)]                             # (the long line's interiors are no part of the stage)
    body, cs = _copies("long_wave", "long_wave")
    per_line = np.bincount([c.record for c in cs if vcf_tables.interior(c)], minlength=len(body))
    assert np.all(per_line[:64] >= 1) and len({c.kind for c in cs}) == 10
    assert len([g for g in vcf_tables.stage_groups(body, cs) if g[0] == 0]) >= 2
    for key in ("names_mixed", "names_snp"):
        bases, recs, pool, names, gt = tables("name_edges")[key]
        assert [len(n) for n in names] == [1, 63, 64, 65, 1023, 1024, 1025]          # lname's 64 bytes; VCF_MAX_NAME and one more
        assert np.all(recs["type"] == SN) == (key == "names_snp") and len(recs) > 128
    assert set(np.unique(tables("name_edges")["names_mixed"][1]["type"]).tolist()) == {SN, IN, DE, DU, IV, TL, TLI}


def test_coverage_sizes_and_suppressed_lines():
    """(c) Wave and workgroup tails (valid / last in k_vcf_lines, the last block of k_len_reduce / k_len_offsets) as SNP-only
    and as general tables; every suppression route at every placement -- the intended lines, and only those, are empty."""
    for n in vcf_tables.SIZES:
        snp, mixed = tables("sizes")[f"size_snp_{n}"], tables("sizes")[f"size_mixed_{n}"]
        assert len(snp[1]) == len(mixed[1]) == n and np.all(snp[1]["type"] == SN) and (n == 1 or not np.all(mixed[1]["type"] == SN))
        assert all(expected("sizes")[f"size_snp_{n}"][0])
    sup = vcf_tables.suppressed()
    assert len(sup) == len(vcf_tables.SUPPRESS_ROUTES) * len(vcf_tables.SUPPRESS_PLACES)
    for key, ((bases, recs, pool, names, gt), idx) in sup.items():
        body = expected("suppressed")[key][0]
        assert len(body) == 600 and [i for i, l in enumerate(body) if not l] == idx, key
        route = key.split("_", 1)[1]
        typ = set(recs["type"][idx].tolist())
        assert typ == ({SN} if route.startswith("snp_on_n") else {IV} if route.startswith("palindrome") else {TLI}), key
        if not key.endswith("_table"):
            assert np.all(recs["type"] == SN) == (route.startswith("snp_on_n") and not route.startswith("snp_on_n_mixed")), key
    assert b"".join(expected("suppressed")["suppress_snp_on_n_table"][0]) == b""
    wave = [not l for l in expected("suppressed")["suppress_empty_tli_wave"][0]]
    assert all(wave[128:192]) and not any(wave[:128]) and not any(wave[192:])


def test_coverage_digit_counts():
    """(e) POS, END and SVLEN at 10^k - 1 and 10^k for k = 1..7 (ndigits' comparisons, SSink::num / DSink::num), POS and END
    at 10^8 on the second contig."""
    for key, ks, svlen in (("digits_10M", range(1, 8), True), ("digits_100M", [8], False)):
        text = b"".join(expected("digits")[key][0])
        pos = {int(l.split(b"\t")[1]) for l in text.split(b"\n") if l}
        end = {int(l.split(b"END=")[1].split(b";")[0]) for l in text.split(b"\n") if b"END=" in l}
        sv = {int(l.split(b"SVLEN=")[1].split(b"\t")[0]) for l in text.split(b"\n") if b"SVLEN=" in l}
        for k in ks:
            assert {10 ** k - 1, 10 ** k} <= pos and {10 ** k - 1, 10 ** k} <= end and (not svlen or {10 ** k - 1, 10 ** k} <= sv), (key, k)
    assert len(tables("digits")["digits_100M"][0]) == 100_000_016 and len(tables("digits")["digits_10M"][0]) == 10_000_016
