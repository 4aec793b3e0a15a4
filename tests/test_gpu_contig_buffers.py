"""The device buffers of a contig and of the state structs when a LATER call replaces them: a larger plan of the same contig,
the haplotype hand-overs across such a replacement, ``clear()`` / ``close()`` while a haplotype is selected and tables are
held, the text buffers of the context and of the file channels, the held tables of the compare mode, the counter-based
engine's scratch and two VCF loads in one context.  Every comparison is exact.

The oracle of each step is a FRESH context given only that step's table (``fresh``; its sequence is itself held against
``apply_ref``), ``_ffi.cmp_counts_host``, ``fast_twin`` and ``vcf_replay_ref``.  All tables are hand-built
(``Engine.set_records``) on contigs of 4 096 bases.

Where replacement happens.  A contig's buffers grow by the rule of ``dev_reserve``: a request of ``want`` bytes keeps the
block when it holds ``want`` and else allocates ``want + want/16 + 256`` bytes.  So, with 16-byte records and 4-byte offsets:

* a table of 8 records asks for 128 bytes and gets 392: room for 24 records;
* its offsets ask for 32 bytes and get 290: room for 72 records;
* an empty insert pool asks for 2 * PAD = 128 bytes and gets 392: the first 264 insert bytes fit;
* an output of unchanged length asks for 4 096 + PAD = 4 160 bytes and gets 4 676.

The second table of case 1 -- 600 records of every type, 2 000 insert bytes, 2 532 bases longer -- therefore replaces the record
table, the offsets, the pool and the output at once; the 1 500 records of case 2 exceed what those 600 left (9 600 -> 10 456
bytes hold 653 records).  A change of the rule moves these sizes.
"""
from __future__ import annotations

import numpy as np
import pytest

import apply_ref
import fast_twin as ft
import vcf_replay_ref
from apply_ref import DE, DU, IN, IV, SN, TL, TLI
from mutation_simulator_amd import _ffi, vcf_replay
from test_fast_host import SHAPES, _twin_ranges, assert_plan_equals_twin
from test_gpu_apply_tables import Table, make_bases
from test_gpu_sampler import _params
from test_multimix_host import _range

pytestmark = pytest.mark.gpu

L0 = 4096
ALL = ("SN", "IN", "DE", "DU", "IV", "TL", "TLI_fwd", "TLI_rev")
TYPE_OF = {"SN": SN, "IN": IN, "DE": DE, "DU": DU, "IV": IV, "TL": TL}
HDR = b"##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def dense_table(L, n, pool_bytes=0, seed=1, kinds=("SN",)):
    """``n`` records at a fixed stride over ACGT bases that depend on ``L`` alone (so tables of one length share their contig),
    the kinds in turn; the insertions hold ``pool_bytes`` in all, every other span is 1..3 bases."""
    bases = make_bases(L, 7, iupac=False)
    stride = (L - 80) // n
    span = min(3, stride - 1)
    assert stride >= 1 and (span >= 1 or kinds == ("SN",))
    tab = Table(bases.copy(), seed=seed)
    n_in = sum(1 for i in range(n) if kinds[i % len(kinds)] == "IN")
    assert (n_in > 0) == (pool_bytes > 0) and pool_bytes >= n_in
    j = 0
    for i in range(n):
        kind, pos = kinds[i % len(kinds)], 16 + i * stride
        if kind == "SN":
            tab.add(SN, pos, aux=i % 3)
        elif kind == "IN":
            tab.add(IN, pos, pool_bytes // n_in + (1 if j < pool_bytes % n_in else 0))
            j += 1
        elif kind.startswith("TLI"):
            k = 1 + int(tab.rs.randint(0, 8))
            tab.add(TLI, pos, span=(int(tab.rs.randint(0, L - 16)), k), aux=1 if kind == "TLI_rev" else 0)
        else:
            tab.add(TYPE_OF[kind], pos, 1 + int(tab.rs.randint(0, span)))
    got, recs, pool = tab.done()
    assert np.array_equal(got, bases) and len(recs) == n and len(pool) == pool_bytes
    return bases, recs, pool


@pytest.fixture(scope="module")
def tables():
    t = {"8": dense_table(L0, 8, seed=1),
         "600": dense_table(L0, 600, 2000, seed=2, kinds=ALL),
         "3": dense_table(L0, 3, seed=3, kinds=("SN", "DE", "IV")),
         "1500": dense_table(L0, 1500, 600, seed=4, kinds=ALL),
         "40": dense_table(L0, 40, 90, seed=5, kinds=ALL),
         "600@3001": dense_table(3001, 600, 2000, seed=6, kinds=ALL),
         "600@5003": dense_table(5003, 600, 2000, seed=7, kinds=ALL)}
    assert set(np.unique(t["600"][1]["type"]).tolist()) == {1, 2, 3, 4, 5, 6, 7}
    bases, recs, pool = t["600"]
    t["600b"] = (bases, recs[np.arange(len(recs)) % 3 != 0].copy(), pool)     # two records in three of it, over the same pool
    assert apply_ref.apply(bases, recs, pool).out_len == L0 + 2532
    return t


def snapshot(eng, cid):
    """Everything a contig's buffers hold, through the entry points that read them."""
    eng.apply_contig(cid)
    recs, pool = eng.fetch_records(cid)
    return {"sizes": eng.result_sizes(cid), "seq": eng.fetch_sequence(cid).tobytes(), "recs": recs.tobytes(), "pool": pool.tobytes(),
            "vcf": eng.render_vcf_device(cid, "chrB").tobytes(), "fasta": eng.fetch_sequence_framed(cid, 60).tobytes(),
            "key_error": eng.key_error(cid)}


def same(got, want, what):
    for k in want:
        assert got[k] == want[k], (what, k)


_FRESH = {}


def fresh(tables, name, gt=None, hap=0, with_offsets=False):
    """The snapshot of a fresh context that was given this table (genotypes, selection) alone; made once per key."""
    key = (name, None if gt is None else gt.tobytes(), hap, with_offsets)
    if key not in _FRESH:
        bases, recs, pool = tables[name]
        with _ffi.Engine(0) as eng:
            cid = eng.add_contig(bases)
            eng.set_records(cid, recs, pool, with_offsets=with_offsets)
            if gt is not None:
                eng.set_genotypes(cid, gt)
                eng.select_haplotype(cid, hap)
            snap = snapshot(eng, cid)
        sub = recs if not hap else recs[(gt & hap) != 0]
        want = apply_ref.apply(bases, sub, pool)
        assert want.key_error is None and snap["key_error"] is None
        assert snap["seq"] == want.seq.tobytes() and snap["recs"] == sub.tobytes() and snap["pool"] == pool.tobytes()
        assert snap["fasta"].replace(b"\n", b"") == snap["seq"]
        _FRESH[key] = snap
    return _FRESH[key]


def thirds(n):
    """Genotypes with about a third of the records on each of 1, 2 and 3."""
    return (np.arange(n) % 3 + 1).astype(np.uint8)


# ------------------------------------------------------------------------------ 1. grow, then shrink, one contig
@pytest.mark.parametrize("with_offsets", [False, True], ids=["scan", "offsets"])
def test_grow_then_shrink_one_contig(tables, with_offsets):
    with _ffi.Engine(0) as eng:
        cid = eng.add_contig(tables["8"][0])
        for name in ("8", "600", "3"):                               # (the last: nothing stale is read behind n_rec)
            _, recs, pool = tables[name]
            eng.set_records(cid, recs, pool, with_offsets=with_offsets)
            same(snapshot(eng, cid), fresh(tables, name, with_offsets=with_offsets), name)


# ------------------------------------------------------------------------------ 2. haplotypes across a replacement
@pytest.mark.parametrize("second", ["1500", "40"], ids=["larger", "smaller"])
def test_haplotypes_across_a_replacement(tables, second):
    with _ffi.Engine(0) as eng:
        _, recs, pool = tables["600"]
        cid = eng.add_contig(tables["600"][0])
        eng.set_records(cid, recs, pool)
        gt = thirds(len(recs))
        eng.set_genotypes(cid, gt)
        for hap in (1, 2, 0, 2):
            eng.select_haplotype(cid, hap)
            same(snapshot(eng, cid), fresh(tables, "600", gt, hap), ("600", hap))
        _, recs, pool = tables[second]                               # haplotype 2 is selected: the full table is parked
        eng.set_records(cid, recs, pool)
        same(snapshot(eng, cid), fresh(tables, second), (second, "installed"))
        gt = thirds(len(recs))[::-1].copy()
        eng.set_genotypes(cid, gt)
        assert np.array_equal(eng.fetch_genotypes(cid, len(recs)), gt)
        for hap in (1, 0):
            eng.select_haplotype(cid, hap)
            same(snapshot(eng, cid), fresh(tables, second, gt, hap), (second, hap))


# ------------------------------------------------------------------------------ 3. release_result, then apply again
def test_release_result_then_apply_again(tables):
    with _ffi.Engine(0) as eng:
        _, recs, pool = tables["600"]
        cid = eng.add_contig(tables["600"][0])
        eng.set_records(cid, recs, pool)
        first = snapshot(eng, cid)
        eng.release_result(cid)                                      # (the table goes with the result; the input stays)
        with pytest.raises(_ffi.MsimError, match="before msim_plan_contig"):
            eng.apply_contig(cid)
        eng.set_records(cid, recs, pool)
        same(snapshot(eng, cid), first, "applied again")
        same(first, fresh(tables, "600"), "600")


# ------------------------------------------------------------------------------ 4. clear() and close() with everything in use
def busy_engine(tables):
    """Contig 0 applied on haplotype 1, contig 1's table held by the compare mode, a VCF text rendered."""
    eng = _ffi.Engine(0)
    _, recs, pool = tables["600"]
    c0 = eng.add_contig(tables["600"][0])
    eng.set_records(c0, recs, pool)
    eng.set_genotypes(c0, thirds(len(recs)))
    eng.select_haplotype(c0, 1)
    eng.apply_contig(c0)
    c1 = eng.add_contig(tables["8"][0])
    eng.set_records(c1, tables["8"][1], tables["8"][2])
    eng.cmp_hold(c1)
    assert len(eng.render_vcf_device(c0, "chrB")) > 0
    return eng


def test_clear_with_everything_in_use(tables):
    eng = busy_engine(tables)
    try:
        eng.clear()
        for name in ("600@3001", "600@5003"):
            bases, recs, pool = tables[name]
            cid = eng.add_contig(bases)
            eng.set_records(cid, recs, pool)
            same(snapshot(eng, cid), fresh(tables, name), name)
    finally:
        eng.close()


def test_close_with_everything_in_use(tables):
    busy_engine(tables).close()                                      # (it only has to return)
    with _ffi.Engine(0) as eng:
        bases, recs, pool = tables["600b"]
        cid = eng.add_contig(bases)
        eng.set_records(cid, recs, pool)
        same(snapshot(eng, cid), fresh(tables, "600b"), "600b")


# ------------------------------------------------------------------------------ 5. text buffers
def test_text_buffer_of_the_context(tables):
    with _ffi.Engine(0) as eng:
        cid = eng.add_contig(tables["8"][0])
        for name in ("8", "600", "3"):
            _, recs, pool = tables[name]
            eng.set_records(cid, recs, pool)
            assert eng.render_vcf_device(cid, "chrB").tobytes() == fresh(tables, name)["vcf"], name


def test_text_buffers_of_the_file_channels(tables, tmp_path):
    """Three texts per channel, enqueued back to back: the 8-record contig's, the 600-record contig's, the first again.  A
    channel lends slot 0 unless its job is still queued, so the second text either takes slot 1 (when the first is not yet
    written) or grows slot 0's buffer past what the first left; the third finds a buffer that is large enough.  Which of the
    two happens is the channel thread's timing; the file bytes must equal the ``*_into`` results either way."""
    with _ffi.Engine(0) as eng, open(tmp_path / "o.fa", "w+b") as fa, open(tmp_path / "o.vcf", "w+b") as vc:
        cids, wants = [], {"fa": [], "vcf": []}
        for name in ("8", "600"):
            bases, recs, pool = tables[name]
            cids.append(eng.add_contig(bases))
            eng.set_records(cids[-1], recs, pool)
            eng.apply_contig(cids[-1])
        order = [(cids[0], "8"), (cids[1], "600"), (cids[0], "8")]
        at = 0
        for cid, _ in order:
            at += eng.fetch_sequence_framed_to_file(cid, 60, fa.fileno(), at)
        at = 0
        for cid, _ in order:
            at += eng.render_vcf_device_to_file(cid, "chrB", vc.fileno(), at)
        eng.file_wait()
        for cid, name in order:
            for kind, size, into in (("fa", eng.fetch_sequence_framed_size(cid, 60), lambda o: eng.fetch_sequence_framed_into(cid, 60, o)),
                                     ("vcf", eng.render_vcf_device_size(cid, "chrB"), lambda o: eng.render_vcf_device_into(cid, "chrB", o))):
                out = np.empty(size, dtype=np.uint8)
                assert into(out) == size
                wants[kind].append(out.tobytes())
            assert wants["fa"][-1] == fresh(tables, name)["fasta"] and wants["vcf"][-1] == fresh(tables, name)["vcf"]
    assert (tmp_path / "o.fa").read_bytes() == b"".join(wants["fa"])
    assert (tmp_path / "o.vcf").read_bytes() == b"".join(wants["vcf"])


# ------------------------------------------------------------------------------ 6. held tables
def test_held_table_replaced_and_flags_kept(tables):
    """The second ``cmp_hold`` replaces the held table by a larger one; the first ``cmp_counts`` (600 current records, the held
    table itself: everything matches) grows the calls' flag buffer, the following ones must keep it: 400 current records (two
    in three of the held ones, so that matched and missed records both occur) and 8."""
    bases = tables["8"][0]
    with _ffi.Engine(0) as eng:
        cid = eng.add_contig(bases)
        for name in ("8", "600"):
            eng.set_records(cid, tables[name][1], tables[name][2])
            eng.cmp_hold(cid)
        _, a, pa = tables["600"]
        for name in ("600", "600b", "8"):
            _, b, pb = tables[name]
            eng.set_records(cid, b, pb)
            counts, tallies = eng.cmp_counts(cid)
            held, held_pool, fa, fb = eng.cmp_fetch(cid)
            assert held.tobytes() == a.tobytes() and held_pool.tobytes() == pa.tobytes(), name
            want = _ffi.cmp_counts_host(bases, a, pa, b, pb)
            for what, g, w in zip(("counts", "tallies", "truth flags", "calls flags"), (counts, tallies, fa, fb), want):
                assert g.shape == w.shape and np.array_equal(g, w), (name, what)


# ------------------------------------------------------------------------------ 7. the counter-based engine's scratch
FAST_A = 3000                                                        # the smallest length of test_gpu_fast_rng.py's shapes (snp_tiny)
FAST_SHAPES = {
    "snp_tiny": SHAPES["snp_tiny"][2],
    # 0.3 candidates a base, three in ten of them structural: K = 900 / 2 700 / 8 100 at a / 3a / 9a
    "svmix": lambda L: [_range(0, L - 1, 0.3, {1: 0.7, 2: 0.1, 3: 0.1, 5: 0.1}, {2: (1, 5), 3: (1, 5), 5: (2, 6)})],
}


@pytest.mark.parametrize("shape", sorted(FAST_SHAPES))
def test_fast_engine_scratch_replaced_without_warm_up(shape):
    """Contigs of a, 3a, a, 3a and then 9a, 3a bases in one context, every plan read back at once and compared with
    ``fast_twin``.  Reading a plan back collects the engine, which starts its rotation over the three scratch sets again
    (``fast_plan_collect``: ``cycle_batches = 0``), so all six plans use set 0.

    ``dev_grow`` keeps a buffer that holds ``want`` ELEMENTS and else allocates ``want + want/4 + 1024`` of them.  The
    per-candidate buffers ask for the candidates rounded up to blocks of 2 048 (``OB_BLOCK``):

    * ``svmix``, a (K = 900): one block, 2 048 asked, 3 584 got (``cand_meta``: 2 064 asked, 3 604 got) -- first allocations;
    * 3a (K = 2 700): two blocks, 4 096 (4 112) asked: ``cand_pos``, ``cand_stop``, ``cand_bend`` and ``cand_meta`` are REPLACED,
      6 144 (6 164) got; a and 3a again fit;
    * 9a (K = 8 100): four blocks, 8 192 (8 208) asked: the same four are replaced again; the last 3a fits.

    ``tab``, ``leaves``, ``sub_k``, ``sub_c0``, ``kept``, ``blk_u32``, ``blk_delta`` and the pinned ``h_tab`` ask for tens to hundreds of
    elements at every one of these sizes and stay inside the 1 024 elements of slack of their first allocation.  ``snp_tiny``
    (12 / 36 SNPs) takes the SNP-only route, which has no per-candidate buffer: first allocations and keeping only."""
    mk = FAST_SHAPES[shape]
    assert FAST_A == min(s[0] for s in SHAPES.values())
    if shape == "svmix":
        assert [sum(int(r.k) for r in mk(L)) for L in (FAST_A, 3 * FAST_A, 9 * FAST_A)] == [900, 2700, 8100]
    params, key = _params(titv=2.0), 0xC0FFEE1234
    lengths = (FAST_A, 3 * FAST_A, FAST_A, 3 * FAST_A, 9 * FAST_A, 3 * FAST_A)
    with _ffi.Engine(0, _ffi.RNG_FAST) as eng:
        eng.set_params(params)
        eng.set_fast_key(key)
        for seq, L in enumerate(lengths):
            ranges = mk(L)
            cid = eng.add_contig_synthetic(L, 7)
            eng.plan_contig(cid, ranges)
            recs, pool = eng.fetch_records(cid)
            twin = ft.plan(L, _twin_ranges(ranges), {t: int(params.block[t]) for t in range(1, 8)}, int(params.ti_lim), key, seq)
            assert_plan_equals_twin(recs, pool, eng.plan_was_empty(cid), twin)
        assert eng.stats()["contigs_fast"] == len(lengths)


# ------------------------------------------------------------------------------ 8. two VCF loads in one context
def test_two_vcf_loads_in_one_context(tables):
    """A text of 20 lines, one of 3 000 data lines, then release and both again; the mutated bases against the plain
    restatement of the VCF's meaning."""
    small = dense_table(L0, 18, 30, seed=8, kinds=("SN", "IN", "DE"))
    large = dense_table(L0, 3000, seed=9)
    texts = []
    for bases, recs, pool in (small, large):
        vcf = HDR + _ffi.render_vcf(recs, pool, bases, "ctg")
        assert vcf.count(b"\n") == len(recs) + 2
        texts.append((bases, vcf, vcf_replay_ref.replay(bases.tobytes(), vcf_replay_ref.data_lines(vcf)["ctg"])))
    assert texts[0][1].count(b"\n") == 20
    with _ffi.Engine(0) as eng:
        cid = eng.add_contig(small[0])
        for round_ in range(2):
            for bases, vcf, want in texts:
                vcf_replay.plan_all(eng, np.frombuffer(vcf, dtype=np.uint8), ["ctg"], [cid])
                eng.apply_contig(cid)
                assert eng.fetch_sequence(cid).tobytes() == want, (round_, len(vcf))
            eng.vcf_release()
