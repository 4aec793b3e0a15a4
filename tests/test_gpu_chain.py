"""The liftover chain rendered on the device (csrc/text_gpu.hip: k_chain_*) must be, byte for byte, what the host renderer
``msim_render_chain`` writes for the same record table -- which tests/test_chain_host.py holds against the restatement of the
rewrite loop's walk (tests/chain_ref.py) -- and ``--chain`` must write those bytes without touching the other two files.

Tile edges: the kernels classify / compact the records and scan the gaps in tiles of T = CH_TILE = TX_THREADS * CH_ITEMS, asked
of the library (``_ffi.chain_tile``) so that the cases follow the code: a workgroup's 256 threads take records l, l + 256, ... of a
tile in the compaction (a ballot's 64 bits are consecutive records) and T / 256 consecutive gaps each in the scans.
"""
from __future__ import annotations

import contextlib
import io
import random

import numpy as np
import pytest

import chain_cases
import chain_ref
from chain_cases import DE, DU, IN, IV, SN, TL, TLI
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import mutator as mm
from test_gpu_sampler import (C3_CHANCES, C3_LENS, TL_CHANCES, TL_LENS, _gene_gaps, _params, _rate_range, _rmt_like_ranges, _snp_range,
                              _sv_range)

pytestmark = pytest.mark.gpu

T = _ffi.chain_tile()          # text_gpu.hip: CH_TILE
PER = T // 256                 # consecutive gaps of a thread in the scans (CH_ITEMS)
HAND = chain_cases.hand_cases()


@pytest.fixture(scope="module")
def eng():
    e = _ffi.Engine(0)
    yield e
    e.close()


def device_equals_host(eng, recs, pool_len, length, name="chrT", chain_id=7):
    eng.clear()
    cid = eng.add_contig_synthetic(length, 3)
    eng.set_records(cid, recs, np.full(pool_len, ord("A"), dtype=np.uint8))
    want = _ffi.render_chain(recs, length, name, name, chain_id)
    got = eng.render_chain_device(cid, name, name, chain_id).tobytes()
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{len(got)} bytes, want {len(want)}; first difference at {k}: {got[max(0, k - 60):k + 60]!r} / "
                             f"{want[max(0, k - 60):k + 60]!r}")
    eng.clear()
    return want


# ------------------------------------------------------------------------------ hand-built tables
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_tables(eng, name):
    recs, pool_len, length = HAND[name]
    want = device_equals_host(eng, recs, pool_len, length, name)
    assert want == chain_ref.render(recs, length, name, name, 7)


def test_two_call_protocol_and_names(eng):
    import ctypes as C
    recs, pool_len, length = HAND["every_type_with_snps_between"]
    eng.clear()
    cid = eng.add_contig_synthetic(length, 3)
    lib, need = eng.lib, C.c_uint64()
    assert lib.msim_render_chain_device(eng.h, cid, b"t", b"q", 1, None, 0, C.byref(need)) == _ffi.ERR_ARG      # not planned
    eng.set_records(cid, recs, np.full(pool_len, ord("A"), dtype=np.uint8))
    want = _ffi.render_chain(recs, length, "t", "q", 1)
    assert lib.msim_render_chain_device(eng.h, cid, b"t", b"q", 1, None, 0, C.byref(need)) == _ffi.OK
    assert need.value == len(want)
    out = np.full(len(want) + 4, 0x55, dtype=np.uint8)
    assert lib.msim_render_chain_device(eng.h, cid, b"t", b"q", 1, out.ctypes.data, len(want) - 1, C.byref(need)) == _ffi.ERR_ARG
    assert need.value == len(want) and (out == 0x55).all()
    assert lib.msim_render_chain_device(eng.h, cid, b"t", b"q", 1, out.ctypes.data, len(want), C.byref(need)) == _ffi.OK
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0x55).all()
    # a copy call with other names or another id renders again
    other = _ffi.render_chain(recs, length, "tt", "q", 12345678901)
    out = np.zeros(len(other), dtype=np.uint8)
    assert lib.msim_render_chain_device(eng.h, cid, b"tt", b"q", 12345678901, out.ctypes.data, len(other), C.byref(need)) == _ffi.OK
    assert out.tobytes() == other
    # the VCF text of the same contig is not confused with it
    assert eng.render_vcf_device(cid, "t").tobytes() == _ffi.render_vcf(recs, np.full(pool_len, ord("A"), dtype=np.uint8),
                                                                        eng.read_contig(cid), "t")
    assert eng.render_chain_device(cid, "t", "q", 1).tobytes() == want
    eng.clear()


def test_kernel_time_measurement():
    """``Engine.chain_kernel_ms`` (msim_dbg_chain_ms: HIP events around the chain kernels) switches the measurement on, changes
    no byte of the text and reports the LAST rendering: a positive time where kernels ran -- a wholly deleted contig included,
    whose gaps are counted and summed before it turns out to have no text -- and 0 for a table that needs no kernel."""
    e = _ffi.Engine(0)
    try:
        assert e.chain_kernel_ms() == 0.0                                # (switched on; nothing rendered yet)
        recs, pool_len, length = chain_cases.counted(2 * T + 1, snp_every=1, seed=3)
        device_equals_host(e, recs, pool_len, length)
        assert e.chain_kernel_ms() > 0.0
        recs, pool_len, length = HAND["snp_only"]
        device_equals_host(e, recs, pool_len, length)
        assert e.chain_kernel_ms() == 0.0
        recs, pool_len, length = HAND["wholly_deleted_in_pieces"]
        assert device_equals_host(e, recs, pool_len, length) == b""
        assert e.chain_kernel_ms() > 0.0
        recs, pool_len, length = HAND["no_records"]
        device_equals_host(e, recs, pool_len, length)
        assert e.chain_kernel_ms() == 0.0
    finally:
        e.close()


# ------------------------------------------------------------------------------ tile, workgroup and wavefront edges
@pytest.mark.parametrize("snp_every", [0, 3])
@pytest.mark.parametrize("n_struct", [T - 1, T, T + 1, 2 * T + 1])
def test_structural_counts_at_tile_edges(eng, n_struct, snp_every):
    """With ``snp_every`` = 3 the structural records are every fourth record: the compaction gathers a tile of gaps from four
    tiles of records."""
    recs, pool_len, length = chain_cases.counted(n_struct, snp_every=snp_every, seed=n_struct)
    assert (recs["type"] != SN).sum() == n_struct
    device_equals_host(eng, recs, pool_len, length)


@pytest.mark.parametrize("snp_every", [0, 2])
def test_merged_run_over_three_tiles(eng, snp_every):
    """Deletions back to back from gap T - 10 to gap 3 T + 19: one line whose dt is a difference of two prefixes two tiles apart."""
    recs, pool_len, length = chain_cases.counted(3 * T + 100, snp_every=snp_every, merge_from=T - 10, merge_len=2 * T + 30, seed=9)
    want = device_equals_host(eng, recs, pool_len, length)
    run = recs[recs["type"] != SN][T - 10:3 * T + 20]
    assert (run["type"] == DE).all() and (run["pos"][1:] == run["stop"][:-1] + 1).all()
    dt = int((run["stop"] - run["pos"] + 1).sum())
    assert f"\t{dt}\t0\n".encode() in want


def heads_table(n_gaps, heads, lead=0):
    """``n_gaps`` deletions of two bases back to back, except that the ones in ``heads`` have a base in front of them."""
    return chain_cases.layout([(DE, 2, 1 if k in heads else 0) for k in range(n_gaps)], tail=lead)


W = 64 * PER                   # gaps of a wavefront in the scans


@pytest.mark.parametrize("heads", [
    (0,), (PER - 1,), (0, PER - 1, PER), (W - PER, W - 1), (W,), (W - 1, W), (T - PER, T - 1), (T - 1,), (T,),
    (T - 1, T, T + PER - 1, T + PER), (0, W - 1, W, T - 1, T, T + W - 1, T + W, 2 * T - 1, 2 * T, 2 * T + W - 1), (),
    tuple(range(0, 2 * T + W, PER)), tuple(range(PER - 1, 2 * T + W, PER))])
@pytest.mark.parametrize("tail", [0, 5])
def test_heads_on_lane_wave_and_workgroup_edges(eng, heads, tail):
    """In the scans a thread takes PER consecutive gaps (4 with T = 1024): gaps W - PER .. W - 1 (252-255) are the last lane of
    a wavefront's, W (256) the next wavefront's first, T - PER .. T - 1 (1020-1023) the last lane of a workgroup's, T (1024) the
    next workgroup's first.  Everything between two heads is one merged line; ``tail`` = 0 makes the last run a trailing gap,
    no head at 0 the first one a leading gap."""
    recs, pool_len, length = heads_table(2 * T + W, set(heads), tail)
    want = device_equals_host(eng, recs, pool_len, length)
    if not heads and not tail:
        assert want == b""                                               # deleted from end to end
    else:
        assert want.count(b"\n") - 3 == len(heads) - (0 if tail or not heads else 1)      # header, last block, blank line


def test_snps_interleaved_so_that_compaction_crosses_tiles(eng):
    """Runs of SNPs of every length from 0 to 70 between structural records (more than a wavefront of them, so whole ballots are
    empty), then a stretch of 3 T SNPs with no structural record at all: tiles that contribute nothing."""
    rs = np.random.RandomState(4)
    items = []
    for k in range(3 * T):
        items += [(SN, 1, 0)] * (k % 71)
        items.append((int(rs.choice([IN, DE, DU, IV, TL, TLI])), int(rs.randint(1, 9)), int(rs.randint(0, 3))))
        if k == T + 7:
            items += [(SN, 1, 0)] * (3 * T)
    recs, pool_len, length = chain_cases.layout(items, tail=3)
    device_equals_host(eng, recs, pool_len, length)


def test_a_million_mixed_records(eng):
    """60 Mb, 1.25 M records of all seven types (as tests/test_gpu_apply_tables.py builds them for the offset scan): more than
    1024 tiles, so k_scan_u64 goes round more than once for the tile counts."""
    L, stride = 60_000_000, 48
    rs = np.random.RandomState(71)
    n = (L - 4096) // stride
    recs = np.zeros(n, dtype=_ffi.RECORD_DTYPE)
    pos = (np.arange(n, dtype=np.int64) * stride + rs.randint(0, 8, n)).astype(np.int64)
    typ = rs.choice([SN, IN, DE, DU, IV, TL, TLI], size=n, p=[0.4, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1])
    length = rs.randint(1, 31, n)
    recs["pos"], recs["type"] = pos, typ
    recs["stop"] = np.where(typ == SN, pos, pos + length - 1)
    recs["aux"] = np.where(typ == TLI, 2, 0)
    ins = np.where(typ == IN, length, 0)
    recs["extra"] = np.cumsum(ins) - ins
    span = rs.randint(0, L - 64, n)
    tli = typ == TLI
    recs["extra"][tli] = span[tli]
    recs["stop"][tli] = span[tli] + length[tli] - 1
    assert n > 1024 * T and len(set(typ.tolist())) == 7
    want = device_equals_host(eng, recs, int(ins.sum()), L)
    assert want.count(b"\n") > 700_000


# ------------------------------------------------------------------------------ every engine once
def _engine_case(which):
    rs = np.random.RandomState(6)
    if which == "snp":
        L = 600_000
        return L, [_snp_range(0, L - 1, 6_000)], _ffi.PLAN_AUTO, "contigs_snp"
    if which == "svmix":
        L = 1_200_000                                                   # README flags, translocations included
        return L, [_sv_range(0, L - 1, int(L * 0.06), TL_CHANCES, TL_LENS)], _ffi.PLAN_AUTO, "contigs_svmix"
    if which == "hostcut":
        L = 700_000
        return L, _rmt_like_ranges(L, rs, 20), _ffi.PLAN_AUTO, "contigs_hostcut"
    if which == "hostchain":
        L = 900_000
        gaps = [r for r in (_rate_range(s, e, 0.008, C3_CHANCES, C3_LENS) for s, e in _gene_gaps(L, rs, 300)) if r.k]
        return L, gaps, _ffi.PLAN_AUTO, "contigs_hostchain"
    if which == "host":
        L = 300_000
        return L, [_sv_range(0, L - 1, int(L * 0.06), TL_CHANCES, TL_LENS)], _ffi.PLAN_HOST, "contigs_host"
    L = 400_000
    return L, [_sv_range(0, L - 1, int(L * 0.008), C3_CHANCES, C3_LENS)], _ffi.RNG_FAST, "contigs_fast"


@pytest.mark.parametrize("which", ["snp", "svmix", "hostcut", "hostchain", "host", "fast"])
def test_every_engine_once(which):
    L, ranges, flags, counter = _engine_case(which)
    e = _ffi.Engine(0, flags)
    try:
        if flags == _ffi.RNG_FAST:
            e.set_fast_key(0xC0FFEE)
        else:
            e.seed(2, 3)
        e.set_params(_params(titv=1.0))
        cid = e.add_contig_synthetic(L, 7)
        e.plan_contig(cid, ranges)
        got_planned = e.render_chain_device(cid, "chr1", "chr1", 1).tobytes()          # planned is enough
        e.apply_contig(cid)
        out_len, n_rec, _ = e.result_sizes(cid)
        recs, _ = e.fetch_records(cid)
        want = _ffi.render_chain(recs, L, "chr1", "chr1", 1)
        got = e.render_chain_device(cid, "chr1", "chr1", 1).tobytes()
        assert got == want and got_planned == want
        (ch,) = chain_ref.parse(want)
        assert ch["qSize"] == out_len and ch["tSize"] == L and n_rec == len(recs) > 1000
        assert e.stats()[counter] == 1
        if which in ("snp", "hostcut"):
            assert want == f"chain {L} chr1 {L} + 0 {L} chr1 {L} + 0 {L} 1\n{L}\n\n".encode()
        else:
            assert want.count(b"\n") > 500
    finally:
        e.close()


# ------------------------------------------------------------------------------ the command line
CLI_MIX = ["args", "-sn", "0.005", "-in", "0.001", "-inmax", "50", "-de", "0.001", "-demax", "50", "-du", "0.0005", "-dumin", "50",
           "-dumax", "500", "-iv", "0.0005", "-ivmin", "50", "-ivmax", "500", "-tl", "0.0004", "-tlmin", "10", "-tlmax", "60",
           "-titv", "1.0"]
CLI_CONTIGS = [("big one", 400_000, 60), ("small", 5_000, 70), ("tiny", 700, 50), ("mid", 30_000, 60)]


def _run_cli(argv):
    from mutation_simulator_amd import __main__ as msa_main
    err = io.StringIO()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err):
        try:
            msa_main.main(argv)
        except SystemExit as e:
            raise AssertionError(f"exit {e.code}: {err.getvalue()}")


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    """One genome, the same seeded command without and with --chain, with --bgzip --chain, and the tables the run planned
    (host planner on the same streams: every engine's tables are bit-identical to its)."""
    from inputs import random_bases
    import mutation_simulator_amd as msa
    tmp = tmp_path_factory.mktemp("chain_cli")
    fa = tmp / "g.fa"
    with open(fa, "wb") as f:
        for i, (name, L, bpl) in enumerate(CLI_CONTIGS):
            b = random_bases(L, 40 + i).tobytes()
            f.write(b">" + name.encode() + b"\n" + b"\n".join(b[k:k + bpl] for k in range(0, L, bpl)) + b"\n")
    for sub, extra in (("plain", []), ("chain", ["--chain"]), ("bgzip", ["--bgzip", "--chain"])):
        (tmp / sub).mkdir()
        _run_cli(["-q", "--seed", "77", "-o", str(tmp / sub / "out")] + extra + [str(fa)] + CLI_MIX)
    with contextlib.redirect_stderr(io.StringIO()):
        args = msa.get_args([str(fa)] + CLI_MIX)
        fasta = msa.load_fasta(args.infile)
        sim = msa.SimulationSettings.from_args(args, fasta, True)
    random.seed(77)
    np.random.seed(77)
    e = _ffi.Engine(device=-1)
    mm.export_python_streams(e)
    e.set_params(mm.params_descriptor(sim))
    want = b""
    for chrom in sim.chromosomes:
        rec = fasta[chrom.number]
        cid = e.add_contig(rec.bases)
        e.plan_contig(cid, mm.plan_descriptors(chrom))
        recs, _ = e.fetch_records(cid)
        want += chain_ref.render(recs, len(rec), rec.name, rec.name, chrom.number + 1)
        e.clear()
    e.close()
    fasta.close()
    return tmp, fa, want


def test_cli_chain_file_and_untouched_outputs(cli_run):
    tmp, _, want = cli_run
    assert (tmp / "chain" / "out_ms.chain").read_bytes() == want
    assert want.count(b"chain ") == len(CLI_CONTIGS) and b" big 400000 + " in want and want.count(b"\n") > 1000
    assert not (tmp / "plain" / "out_ms.chain").exists()
    for name in ("out_ms.fa", "out_ms.vcf"):
        assert (tmp / "chain" / name).read_bytes() == (tmp / "plain" / name).read_bytes(), name


def test_cli_bgzip_chain_is_plain(cli_run):
    from mutation_simulator_amd import bgzf
    tmp, _, want = cli_run
    assert (tmp / "bgzip" / "out_ms.chain").read_bytes() == want
    assert sorted(p.name for p in (tmp / "bgzip").iterdir()) == ["out_ms.chain", "out_ms.fa.gz", "out_ms.vcf.gz"]
    assert bgzf.check_file((tmp / "bgzip" / "out_ms.fa.gz").read_bytes()) == (tmp / "plain" / "out_ms.fa").read_bytes()


def test_cli_vcf_mode_gives_the_same_chain(cli_run):
    tmp, fa, want = cli_run
    (tmp / "replay").mkdir()
    _run_cli(["-q", "-o", str(tmp / "replay" / "out"), "--chain", str(fa), "vcf", str(tmp / "plain" / "out_ms.vcf")])
    assert sorted(p.name for p in (tmp / "replay").iterdir()) == ["out_ms.chain", "out_ms.fa"]
    assert (tmp / "replay" / "out_ms.chain").read_bytes() == want
    assert (tmp / "replay" / "out_ms.fa").read_bytes() == (tmp / "plain" / "out_ms.fa").read_bytes()


def test_cli_fast_rng_chain(tmp_path, cli_run):
    """--rng fast --chain: the chain describes the Fasta of that run (qSize per contig = its mutated length)."""
    _, fa, _ = cli_run
    _run_cli(["-q", "--seed", "5", "--rng", "fast", "--chain", "-o", str(tmp_path / "out"), str(fa), "args", "-sn", "0.005", "-in",
              "0.001", "-de", "0.001", "-du", "0.0005", "-iv", "0.0005"])
    chains = chain_ref.parse((tmp_path / "out_ms.chain").read_bytes())
    assert [c["id"] for c in chains] == [1, 2, 3, 4] and [c["tName"] for c in chains] == ["big", "small", "tiny", "mid"]
    lens = []
    for line in (tmp_path / "out_ms.fa").read_bytes().split(b"\n"):
        if line.startswith(b">"):
            lens.append(0)
        elif lens:
            lens[-1] += len(line)
    assert [c["qSize"] for c in chains] == lens and [c["tSize"] for c in chains] == [L for _, L, _ in CLI_CONTIGS]
