"""The SNP sampler's grouped emission (plan_gpu.hip: gpu_emit_flush) end to end against the host planner, at sizes that sit on
the borders of the emission kernels' blocks: an expansion block of the three-launch train is 2048 bitmap words (plan_kernels.h:
EX_WORDS), a super-block four of them; the six-launch train's block 256 words.

What has to hold: the records byte for byte and both streams at the same positions as the sequential host planner
(``_ffi.PLAN_HOST``), and, after ``apply_contig``, the mutated contig's checksum equal to that of the host planner's table
applied -- for both trains and for groups of one and of four contigs.  ``MSIM_AHEAD=2`` makes the three-launch train the one a
context picks by itself at these sizes; ``MSIM_EMIT_TRAIN`` then names it outright."""
from __future__ import annotations

import numpy as np
import pytest

from mutation_simulator_amd import _ffi
from test_gpu_sampler import _next_words, _params, _snp_range

pytestmark = pytest.mark.gpu

B = 2048                 # bitmap words per expansion block


def _contig(words, k, tail_bits=17):
    """An SNP-only contig (one range over all of it, sampling distance 1) whose bitmap has ``words`` words, the last one short
    of ``tail_bits`` bits: the sample's population is n = L - k."""
    n = 64 * words - tail_bits
    L = n + k
    assert 1_000_000 <= L <= 5_000_000
    return L, [_snp_range(0, L - 1, k)]


# bitmap words on the block borders +- 1 (8, 16 and 33 blocks: whole and broken super-blocks), one sample with k / n = 0.27
SHAPES = {
    "8B-1": [_contig(8 * B - 1, 10_000)],
    "8B": [_contig(8 * B, 12_345, tail_bits=0)],
    "8B+1": [_contig(8 * B + 1, 10_000, tail_bits=63)],
    "16B+1": [_contig(16 * B + 1, 40_000)],
    "33B-1": [_contig(33 * B - 1, 90_000)],
    "dense": [_contig(9 * B, 9 * B * 64 * 27 // 100)],
    "chain4": [_contig(8 * B + 1, 30_000), _contig(12 * B - 1, 8_000), _contig(8 * B, 80_000, tail_bits=1),
               _contig(20 * B, 25_000)],
}
_HOST = {}               # shape -> the host planner's result: computed once, shared, never changed


def _run(flags, contigs, titv, seed):
    """Plan every contig, then apply every contig (an emission group goes out with its APPLYs), then read."""
    with _ffi.Engine(0, flags) as eng:
        eng.seed(*seed)
        eng.set_params(_params(titv=titv))
        cids = []
        for L, ranges in contigs:
            cid = eng.add_contig_synthetic(L, 7)
            eng.plan_contig(cid, ranges)
            cids.append(cid)
        for cid in cids:
            eng.apply_contig(cid)
        out = []
        for cid in cids:
            recs, pool = eng.fetch_records(cid)
            out.append((recs.copy(), pool.copy(), eng.result_checksum(cid)))
        st = eng.stats()
        states = [eng.get_mt_state(0), eng.get_mt_state(1)]
    return out, states, st


def _host(shape):
    if shape not in _HOST:
        _HOST[shape] = _run(_ffi.PLAN_HOST, SHAPES[shape], 2.0, (11, 12))
    return _HOST[shape]


@pytest.mark.parametrize("train", [3, 6])
@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_grouped_emission_vs_host_planner(monkeypatch, shape, group, train):
    monkeypatch.setenv("MSIM_AHEAD", "2")
    monkeypatch.setenv("MSIM_EMIT_GROUP", str(group))
    monkeypatch.setenv("MSIM_EMIT_TRAIN", str(train))
    host, hs, hst = _host(shape)
    gpu, gs, gst = _run(_ffi.PLAN_GPU, SHAPES[shape], 2.0, (11, 12))
    for (hr, hpool, hsum), (gr, gpool, gsum) in zip(host, gpu):
        assert hr.shape == gr.shape
        assert np.array_equal(hr.view(np.uint8), gr.view(np.uint8))
        assert np.array_equal(hpool, gpool)
        assert hsum == gsum
    assert hst["py_words"] == gst["py_words"] and hst["np_words"] == gst["np_words"]
    for (hm, hp), (gm, gp) in zip(hs, gs):
        assert _next_words(hm, hp, 8) == _next_words(gm, gp, 8)
    assert gst["contigs_snp"] == len(SHAPES[shape]) and gst["plan_host_ms"] == 0
