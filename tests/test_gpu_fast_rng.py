"""``MSIM_RNG_FAST`` (``--rng fast``): the counter-based PLAN engine on the GPU (csrc/fast_kernels.h, plan_fast.hip).

It is NOT stream-compatible with the reference by design -- every draw is a Philox counter instead of the next word of a
sequential MT19937 stream -- so BIT PARITY WITH THE REFERENCE IS IMPOSSIBLE HERE and is not claimed.  What is checked:

* the kernels against ``tests/fast_twin.py``, the numpy restatement of the engine (tree of hypergeometric draws, leaf
  rejection sampling, per-candidate draws; boundary pass and visit filter written as the reference's sequential loops):
  exact equality of every record, insert pool byte and the plan-was-empty flag, over SNP-only ranges, SV mixes, several
  ranges with their own settings, ``sn_block`` above the sampling distance, dense hot spots, runs of dependent orbit blocks;
* the DISTRIBUTIONS against the ORACLE (the reference's own construction under MT19937): for BASELINE configs[2]'s
  settings on 120 Mb, per-type record counts, length histograms, gaps between records and the kept fraction of the
  candidates, by two-sample chi-square / z tests with stated bounds;
* the properties the construction guarantees (util.py:93-109): exactly k positions per range, inside the range, >= d + 1
  apart; uniformity; transition share;
* APPLY + device text on these records against a plain restatement of ``__mutate_sequence`` fed with the same records and
  against the host VCF renderer (pinned to the reference's goldens) -- everything behind PLAN is the compat path's code;
* determinism, key sensitivity, contig ordinals (``msim_plan_chain`` keeps ranks aligned), what the mode refuses, the CLI.
"""
from __future__ import annotations

import numpy as np
import pytest

import apply_ref
import fast_twin as ft
from inputs import random_bases
from mutation_simulator_amd import _ffi
from test_fast_host import SHAPES, _twin_ranges, assert_plan_equals_twin
from test_gpu_sampler import _params, _snp_range, _sv_range, C3_CHANCES, C3_LENS

pytestmark = pytest.mark.gpu

NAMES = {1: "SN", 2: "IN", 3: "DE", 4: "DU", 5: "IV", 6: "TL", 7: "TLI"}


def _plan(eng, L, ranges, bases=None):
    cid = eng.add_contig(bases) if bases is not None else eng.add_contig_synthetic(L, 7)
    eng.plan_contig(cid, ranges)
    recs, pool = eng.fetch_records(cid)
    return cid, recs.copy(), pool.copy()


def _ti_lim(params):
    return int(params.ti_lim)


def _blocks(params):
    return {t: int(params.block[t]) for t in range(1, 8)}


@pytest.mark.parametrize("orbit", [False, True], ids=["blocklocal", "orbit"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_equals_numpy_restatement(name, orbit, monkeypatch):
    """Both formulations of the boundary pass / visit filter: the block-local kernel (k_fkeep: free candidates + cluster walks;
    the shape with 400 kb deletions makes it hand over to the orbit kernels by itself) and, forced, the orbit kernels alone."""
    if orbit:
        monkeypatch.setenv("MSIM_FAST_FORCE_ORBIT", "1")
    L, blocks, mk = SHAPES[name]
    params = _params({NAMES[t]: v for t, v in (blocks or {}).items()}, titv=2.0)
    ranges = mk(L)
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    eng.set_params(params)
    key = 0xC0FFEE1234
    eng.set_fast_key(key)
    for seq in range(2):
        cid, recs, pool = _plan(eng, L, ranges)
        empty = eng.plan_was_empty(cid)
        twin = ft.plan(L, _twin_ranges(ranges), _blocks(params), _ti_lim(params), key, seq)
        assert_plan_equals_twin(recs, pool, empty, twin)
        eng.clear()
    assert eng.stats()["contigs_fast"] == 2
    import ctypes as C
    n = C.c_uint64()
    assert eng.lib.msim_dbg_fast_replays(eng.h, C.byref(n)) == 0
    # 400 kb deletions at rate 0.001 block ~100 candidates each: no free candidate in a 64-candidate halo -> the block-local
    # kernel hands over and the plan is replayed with the orbit kernels.  Nothing else here comes near that.
    if name == "long_deletions_dependent_blocks":
        assert n.value == (0 if orbit else 2)
    if orbit or name in ("svmix_one_range", "sn_block_7", "sn_block_svmix") or name.startswith("snp"):
        assert n.value == 0
    # (svmix_dense_end -- a candidate every 20 bases, four in five of them an SV of hundreds of bases -- has next to no free
    #  candidate: whether a block finds its anchor within the last 512 candidates of the block before it, the part k_fkeep keeps
    #  in LDS, is luck; either way the records equal the twin's)
    if name == "svmix_dense_end" and not orbit:
        assert n.value in (0, 2)
    eng.close()


def test_big_contig_equals_numpy_restatement():
    """One 40 Mb contig: a splitting tree 12 levels deep, 2 400 leaves, candidates over many orbit blocks."""
    params = _params(titv=2.0)
    L, key = 40_000_000, 99
    for ranges in ([_snp_range(0, L - 1, 400_000)], [_sv_range(0, L - 1, 320_000, C3_CHANCES, C3_LENS)]):
        eng = _ffi.Engine(0, _ffi.RNG_FAST)
        eng.set_params(params)
        eng.set_fast_key(key)
        cid, recs, pool = _plan(eng, L, ranges)
        twin = ft.plan(L, _twin_ranges(ranges), _blocks(params), _ti_lim(params), key, 0)
        assert_plan_equals_twin(recs, pool, eng.plan_was_empty(cid), twin)
        eng.close()


def test_insert_heavy_blocks_equal_numpy_restatement():
    """Nine candidates in ten are insertions: k_femit's LDS list of a block's insertions (half a block's worth) overflows and
    every lane fills its own insert bases instead -- pools and records still equal the twin's."""
    params = _params(titv=2.0)
    L, key = 3_000_000, 1234
    ranges = [_sv_range(0, L - 1, 30_000, {1: 0.1, 2: 0.9}, {2: (1, 30)})]
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    eng.set_params(params)
    eng.set_fast_key(key)
    cid, recs, pool = _plan(eng, L, ranges)
    assert (recs["type"] == 2).sum() > 0.6 * len(recs) and len(pool) > 100_000
    twin = ft.plan(L, _twin_ranges(ranges), _blocks(params), _ti_lim(params), key, 0)
    assert_plan_equals_twin(recs, pool, eng.plan_was_empty(cid), twin)
    eng.close()


def test_properties_at_scale():
    L = 60_000_000
    blocks = {t: 3 for t in ("SN", "IN", "DE", "IV", "DU", "TL", "TLI")}          # min distance d = 3
    params = _params(blocks, titv=2.0)
    rs = [(0, 19_999_999, 200_000), (20_000_000, 20_004_999, 600), (25_000_000, L - 1, 350_000)]
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    eng.set_params(params)
    eng.set_fast_key(77)
    _, recs, _ = _plan(eng, L, [_snp_range(a, b, k) for a, b, k in rs])
    pos = recs["pos"].astype(np.int64)
    assert len(pos) == sum(k for _, _, k in rs)
    assert np.all(np.diff(pos) > 3)                                          # sorted, distinct, at least d + 1 apart
    at = 0
    for a, b, k in rs:
        p = pos[at:at + k]
        at += k
        assert p[0] >= a and p[-1] <= b
        # uniformity of the underlying sample (positions minus their rank shift) over 64 bins
        v = p - a - 3 * np.arange(k)
        n = (b - (k - 1) * 3) - a
        if k >= 64 * 50:
            counts = np.bincount((v * 64 // n).astype(np.int64), minlength=64)
            chi2 = float(((counts - k / 64) ** 2 / (k / 64)).sum())
            assert chi2 < 150, chi2                                          # 63 degrees of freedom: mean 63, sd 11
    aux = recs["aux"]
    p_ti = 2.0 * (1 / 3.0)
    share = float((aux == 0).mean())
    assert abs(share - p_ti) < 5 * np.sqrt(p_ti * (1 - p_ti) / len(aux))
    tv = aux[aux > 0]
    assert abs(float((tv == 1).mean()) - 0.5) < 5 * 0.5 / np.sqrt(len(tv))
    eng.close()


# ---------------------------------------------------------------------------------------------- distributions vs the oracle
def _vcf_table(vcf: bytes):
    """(pos, type id, length) of every record line; type ids as MSIM_*; length = SVLEN (INS / DEL / DUP), span (INV), 1 (SNP)."""
    kinds = {b"INS": 2, b"DEL": 3, b"DUP": 4, b"INV": 5}
    pos, typ, ln = [], [], []
    for line in vcf.split(b"\n"):
        if not line or line.startswith(b"#"):
            continue
        f = line.split(b"\t")
        info = f[7]
        if info == b"." or b"SVTYPE" not in info:
            t, n = 1, 1
        else:
            kv = dict(x.split(b"=") for x in info.split(b";") if b"=" in x)
            t = kinds[kv[b"SVTYPE"]]
            n = int(kv[b"END"]) - int(f[1]) + 1 if t == 5 else int(kv[b"SVLEN"])
        pos.append(int(f[1]))
        typ.append(t)
        ln.append(n)
    return np.array(pos, dtype=np.int64), np.array(typ, dtype=np.int64), np.array(ln, dtype=np.int64)


def _two_sample_chi2(a, b, edges):
    from scipy import stats
    ha, _ = np.histogram(a, bins=edges)
    hb, _ = np.histogram(b, bins=edges)
    keep = (ha + hb) >= 20
    ha, hb = ha[keep].astype(np.float64), hb[keep].astype(np.float64)
    na, nb = ha.sum(), hb.sum()
    chi2 = float((((ha * np.sqrt(nb / na) - hb * np.sqrt(na / nb)) ** 2) / (ha + hb)).sum())
    return chi2, stats.chi2(len(ha) - 1).ppf(1 - 1e-6)


def test_distributions_match_the_oracle_on_config3_settings():
    """BASELINE configs[2]'s SV mix on a 120 Mb contig, `--rng fast` on the device vs the ORACLE (the reference's construction
    under its own MT19937 streams).  Bit parity is impossible (different generator); the two outputs must be samples of the same
    law: per-type record counts within 6 sigma of each other (sigma^2 <= sum of both counts: counts are sums of weakly
    dependent indicators), length histograms and the gaps between consecutive records by two-sample chi-square at p > 1e-6,
    kept fraction of the candidates within 6 sigma, minimum spacing respected."""
    import bench
    from mutation_simulator_amd import mutator as mm
    from oracle import oracle as orc
    from test_gpu_fullsize import C3
    from test_gpu_parity import synth_host
    from test_host_settings import dump_sim
    L = 120_000_000
    sim = bench.workload_settings([L], extra=C3 + ["-sn", "0.005"])
    bases = synth_host(L, 1000)
    o = orc.Oracle()
    o.seed(42, 42)
    _, want_vcf, _, _ = o.run_genome([{"name": "chr1", "long_name": "chr1 synthetic", "lenc": 60, "bases": bases}], dump_sim(sim),
                                     "synthetic.fa")
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    eng.set_params(mm.params_descriptor(sim))
    eng.set_fast_key(2024)
    cid = eng.add_contig_synthetic(L, 1000)
    table = mm.plan_table(sim.chromosomes[0])
    eng.plan_contig(cid, table)
    eng.apply_contig(cid)
    got_vcf = eng.render_vcf_device(cid, "chr1").tobytes()
    n_cand = int(table["k"].sum())
    eng.close()
    po, to, lo = _vcf_table(want_vcf)
    pf, tf, lf = _vcf_table(got_vcf)
    assert np.all(np.diff(pf) > 0)
    # kept fraction of the candidates (the rest was blocked, dropped or invisible: SNP on N does not occur in ACGT input)
    fo, ff = len(po) / n_cand, len(pf) / n_cand
    assert abs(fo - ff) < 6 * np.sqrt((fo * (1 - fo) + ff * (1 - ff)) / n_cand), (fo, ff)
    for t in (1, 2, 3, 4, 5):
        co, cf = int((to == t).sum()), int((tf == t).sum())
        assert co > 1000 and abs(co - cf) < 6 * np.sqrt(co + cf), (t, co, cf)
        if t != 1:
            hi = 50 if t in (2, 3) else 500
            lo_ = 1 if t in (2, 3) else 50
            assert lf[tf == t].min() >= lo_ and lf[tf == t].max() <= hi
            chi2, bound = _two_sample_chi2(lo[to == t], lf[tf == t], np.linspace(lo_ - 0.5, hi + 0.5, 26 if t in (2, 3) else 46))
            assert chi2 < bound, (t, chi2, bound)
    chi2, bound = _two_sample_chi2(np.diff(po), np.diff(pf), np.concatenate((np.arange(1.5, 60, 4), np.geomspace(60, 4000, 40))))
    assert chi2 < bound, (chi2, bound)
    assert np.diff(pf).min() >= 1 and np.diff(po).min() >= 1          # (VCF POS: an SNP at p is p + 1, a DEL at p + 2 is p + 2)


# ---------------------------------------------------------------------------------------------- APPLY + text behind fast records
def _apply_records(bases, recs, pool):
    """__mutate_sequence (mutator.py:318-426) over a finished record table: tests/apply_ref.py, the restatement that
    tests/test_apply_ref_host.py holds against the real reference's bytes."""
    res = apply_ref.apply(bases, recs, pool)
    assert res.key_error is None
    return res.seq


@pytest.mark.parametrize("kind", ["snp", "svmix", "rmt"])
def test_apply_and_text_on_fast_records(kind):
    L = 2_000_000
    bases = random_bases(L, 9)
    params = _params(titv=1.0)
    if kind == "snp":
        ranges = [_snp_range(0, L - 1, 20_000)]
    elif kind == "svmix":
        ranges = [_sv_range(0, L - 1, 16_000, C3_CHANCES, C3_LENS)]
    else:
        ranges = [_sv_range(0, 599_999, 6_000, {3: 0.5, 1: 0.5}, {3: (500, 3000)}), _snp_range(600_000, 600_999, 300),
                  _sv_range(601_000, L - 1, 20_000, C3_CHANCES, C3_LENS)]
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    eng.set_params(params)
    eng.set_fast_key(5)
    cid, recs, pool = _plan(eng, L, ranges, bases=bases)
    eng.apply_contig(cid)
    out_len, n_rec, n_pool = eng.result_sizes(cid)
    got = eng.fetch_sequence(cid)
    want = _apply_records(bases, recs, pool)
    assert n_rec == len(recs) and n_pool == len(pool) and out_len == len(want)
    assert np.array_equal(got, want)
    host_vcf = _ffi.render_vcf(recs, pool, bases, "chrF")
    vcf = eng.render_vcf_device(cid, "chrF").tobytes()
    assert vcf == host_vcf and vcf.count(b"\n") == len(recs)
    framed = eng.fetch_sequence_framed(cid, 60).tobytes()
    assert framed.replace(b"\n", b"") == want.tobytes()
    eng.close()


def test_determinism_keys_and_ordinals():
    params = _params(titv=2.0)
    r = [_sv_range(0, 999_999, 8_000, C3_CHANCES, C3_LENS)]

    def run(key, skip_first):
        eng = _ffi.Engine(0, _ffi.RNG_FAST)
        eng.set_params(params)
        eng.set_fast_key(key)
        out = []
        for i in range(3):
            if i == 0 and skip_first:
                eng.plan_chain(1_000_000, r)                # a contig another rank owns: only its ordinal is consumed
                out.append(None)
                continue
            _, recs, pool = _plan(eng, 1_000_000, r)
            out.append((recs, pool))
            eng.clear()
        eng.close()
        return out
    a, b, c, d = run(11, False), run(11, False), run(12, False), run(11, True)
    for x, y in zip(a, b):
        assert np.array_equal(x[0].view(np.uint8), y[0].view(np.uint8)) and np.array_equal(x[1], y[1])     # same key: same plan
    assert not np.array_equal(a[0][0]["pos"][:1000], a[1][0]["pos"][:1000])          # contig ordinals differ
    assert not np.array_equal(a[0][0]["pos"][:1000], c[0][0]["pos"][:1000])          # keys differ
    assert np.array_equal(a[1][0].view(np.uint8), d[1][0].view(np.uint8)) and np.array_equal(a[2][0].view(np.uint8), d[2][0].view(np.uint8))


def test_refuses_what_it_does_not_cover():
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    eng.set_params(_params(titv=1.0))
    cid = eng.add_contig_synthetic(1_000_000, 1)
    with pytest.raises(_ffi.MsimUnsupported, match="translocations"):
        eng.plan_contig(cid, [_sv_range(0, 999_999, 9_000, {1: 0.5, 6: 0.25, 7: 0.25}, {6: (5, 50)})])
    with pytest.raises(ValueError, match="Sample larger than population"):
        eng.plan_contig(cid, [_snp_range(0, 999_999, 600_000)])                          # k > n: the reference's ValueError
    with pytest.raises(_ffi.MsimUnsupported, match="overlapping"):
        eng.plan_contig(cid, [_snp_range(0, 500_000, 1_000), _snp_range(400_000, 999_999, 1_000)])
    with pytest.raises(ValueError, match="Sample larger than population"):
        eng.plan_chain(1_000_000, [_snp_range(0, 999_999, 600_000)])                     # ... on ranks that do not own the contig too
    eng.close()


def test_cli_rng_fast_end_to_end(tmp_path):
    """``--rng fast`` through the CLI: k SNPs per contig exactly where int(len * rate) says, files consistent with each other
    (every VCF line's REF is the input base, its ALT the output base; nothing else changed), reproducible under --seed,
    different under another seed, identical with --gpus 2; the SV mix runs too (files consistent: mutated length = input
    length + the VCF's net SVLEN) and translocation flags are refused with the library's message."""
    import contextlib
    import io

    import inputs as gin
    from helpers import parse_fasta_bytes
    from mutation_simulator_amd import __main__ as cli
    spec = {"contigs": [{"defline": "f1 fast", "length": 900_000, "bpl": 60, "seed": 1},
                        {"defline": "f2", "length": 5_000, "bpl": 50, "seed": 2},
                        {"defline": "f3", "length": 300_011, "bpl": 70, "seed": 3}]}
    infile = gin.write_input(spec, tmp_path / "in.fa")
    src = parse_fasta_bytes(infile.read_bytes())

    def run(tag, *extra, flags=("-sn", "0.01", "-titv", "2.0")):
        with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
            cli.main(["-q", "--rng", "fast", *extra, "-o", str(tmp_path / tag), str(infile), "args", *flags])
        return (tmp_path / f"{tag}_ms.fa").read_bytes(), (tmp_path / f"{tag}_ms.vcf").read_bytes()
    fa, vcf = run("a", "--seed", "7")
    out = parse_fasta_bytes(fa)
    lines = [l.split(b"\t") for l in vcf.split(b"\n") if l and not l.startswith(b"#")]
    for c_in, c_out in zip(src, out):
        mine = [l for l in lines if l[0] == c_in["name"].encode()]
        assert len(mine) == int(len(c_in["bases"]) * 0.01)
        changed = np.flatnonzero(c_in["bases"] != c_out["bases"])
        assert [int(l[1]) - 1 for l in mine] == changed.tolist()
        assert all(l[3] == bytes([c_in["bases"][p]]) and l[4] == bytes([c_out["bases"][p]]) for l, p in zip(mine, changed))
    assert run("b", "--seed", "7") == (fa, vcf)
    fa2, vcf2 = run("c", "--seed", "8")
    assert fa2 != fa
    import os
    os.environ["MSIM_SHARD_DEVICES"] = "0,0"
    try:
        assert run("d", "--seed", "7", "--gpus", "2") == (fa, vcf)
    finally:
        del os.environ["MSIM_SHARD_DEVICES"]
    sv = ("-sn", "0.005", "-in", "0.001", "-de", "0.001", "-du", "0.0005", "-iv", "0.0005")
    fa3, vcf3 = run("s", "--seed", "7", flags=sv)
    out3 = parse_fasta_bytes(fa3)
    pos3, typ3, len3 = _vcf_table(vcf3)
    names = [l.split(b"\t")[0] for l in vcf3.split(b"\n") if l and not l.startswith(b"#")]
    for c_in, c_out in zip(src, out3):
        mine = np.array([n == c_in["name"].encode() for n in names])
        net = int(len3[mine & (typ3 == 2)].sum() - len3[mine & (typ3 == 3)].sum() + len3[mine & (typ3 == 4)].sum())
        assert len(c_out["bases"]) == len(c_in["bases"]) + net
    assert {1, 2, 3, 4, 5} <= set(typ3.tolist())
    assert run("s2", "--seed", "7", flags=sv) == (fa3, vcf3)
    err = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stderr(err):
        cli.main(["-q", "--rng", "fast", "-o", str(tmp_path / "e"), str(infile), "args", "-sn", "0.01", "-tl", "0.001"])
    assert "fast RNG mode" in err.getvalue()


@pytest.mark.parametrize("workload", ["c2", "c3", "c4", "c4sv"])
def test_full_genome_fast_properties(workload):
    """The bench genome (3 Gb, 24 contigs) through the fast mode with the settings of BASELINE configs[1..3] (+ the RMT file
    with the SV mix as std line): per contig the records sorted and >= 2 apart, SNP-only settings leave exactly sum(k) records
    with every range holding exactly its k positions; result sizes consistent (mutated length = input + the records' net
    length change); APPLY of the largest contig changes the input exactly as the records say (checksum against the plain
    restatement on a 3 Mb window is the rewrite kernels' own test: here the length and the differing-base count)."""
    import bench
    from mutation_simulator_amd import mutator as mm
    lengths = bench.contig_lengths(3_000_000_000)
    sim = bench.build_settings(workload, lengths)
    eng = _ffi.Engine(0, _ffi.RNG_FAST)
    eng.set_params(mm.params_descriptor(sim))
    eng.set_fast_key(2024)
    total = 0
    for chrom in sim.chromosomes:
        L = lengths[chrom.number]
        table = mm.plan_table(chrom)
        cid = eng.add_contig_synthetic(L, 1000 + chrom.number)
        eng.plan_contig(cid, table)
        if chrom.number < 3:
            eng.apply_contig(cid)
        recs, _ = eng.fetch_records(cid)
        pos = recs["pos"].astype(np.int64)
        k = table["k"].astype(np.int64)
        assert np.all(np.diff(pos) > 1)
        if workload in ("c2", "c4"):
            assert len(pos) == int(k.sum())
            drawing = table[k > 0]
            edges = np.searchsorted(pos, drawing["start"].astype(np.int64))
            counts = np.diff(np.concatenate((edges, [len(pos)])))
            assert np.array_equal(counts, drawing["k"].astype(np.int64))                    # every range: exactly its k positions ...
            last = pos[np.cumsum(counts) - 1]
            assert np.all(last <= drawing["stop"].astype(np.int64))                          # ... none beyond its stop
        else:
            assert 0.6 * int(k.sum()) < len(pos) <= int(k.sum())
        if chrom.number < 3:
            out_len, n_rec, _ = eng.result_sizes(cid)
            ln = recs["stop"].astype(np.int64) - pos + 1
            t = recs["type"]
            assert n_rec == len(recs)
            assert out_len == L + int(ln[t == 2].sum() - ln[t == 3].sum() + ln[t == 4].sum())
            if workload in ("c2", "c4") and chrom.number == 0:
                before = eng.read_contig(cid)
                after = eng.fetch_sequence(cid)
                assert int((before != after).sum()) == len(pos)
        total += len(pos)
        eng.clear()
    assert eng.stats()["contigs_fast"] == 24 and total > 5_000_000
    eng.close()


def test_key_error_of_an_apply_behind_a_collected_lane_is_collected():
    """Plan a cycle, synchronise (the lanes' sets are collected), THEN apply a contig of one of those lanes, plan more, synchronise:
    the KeyError word of that APPLY -- a transversion on a base outside AGTCN, mutator.py:449-455 -- must be copied behind its
    rewrite launch, although no pending set covers the lane it ran on (apply_finish joins such launches through their events;
    round-5 advisor finding)."""
    import bench
    from mutation_simulator_amd import mutator as mm
    L = 3_000_000
    lengths = [L] * 4
    sim = bench.build_settings("c2", lengths)
    tables = [mm.plan_table(ch) for ch in sim.chromosomes]
    for bad_slot in (1, 3):
        eng = _ffi.Engine(0, _ffi.RNG_FAST)
        try:
            cids = [eng.add_contig(np.full(L, ord("U"), dtype=np.uint8)) if i == bad_slot else eng.add_contig_synthetic(L, 20 + i)
                    for i in range(4)]
            eng.set_params(mm.params_descriptor(sim))
            eng.set_fast_key(7)
            for i in range(4):                             # cycle 1: everything planned, the good contigs applied
                eng.plan_contig(cids[i], tables[i])
                if i != bad_slot:
                    eng.apply_contig(cids[i])
            eng.sync()                                     # sets collected; nothing wrong so far
            eng.apply_contig(cids[bad_slot])               # asynchronous, on a lane whose set is no longer pending
            good = 0 if bad_slot else 2
            eng.plan_contig(cids[good], tables[good])      # ... more work for the next collection
            eng.apply_contig(cids[good])
            with pytest.raises(KeyError) as ei:
                eng.sync()
            assert ei.value.args[0] == "U"
        finally:
            eng.close()
