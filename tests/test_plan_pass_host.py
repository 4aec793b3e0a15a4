"""``msim_plan_pass`` without a GPU: (1) on a host-only context the pass call is the per-contig calls -- same records, same
insert pools, both streams at the same place -- on the shapes ``tests/test_multi_rank_cpu.py`` uses (the bench genome scaled down,
a rank that owns a subset, ``apply=False``); (2) the segmenting rule (``plan_gpu.hip``: ``pass_segment``, reached through
``msim_dbg_pass_segments``: the function the pass call itself cuts its item list with) on hand-built item lists."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import pytest

from mutation_simulator_amd import _ffi
from mutation_simulator_amd import mutator as mm

MT_N = 624


# ---------------------------------------------------------------------- (1) host-only contexts
def _digest(eng, cids, which):
    out = {}
    for i in which:
        recs, pool = eng.fetch_records(cids[i])
        out[i] = hashlib.sha256(recs.tobytes() + pool.tobytes()).hexdigest()
    return out


def _state(eng):
    return [(hashlib.sha256(eng.get_mt_state(s)[0].tobytes()).hexdigest(), eng.get_mt_state(s)[1]) for s in (0, 1)]


@pytest.fixture(scope="module")
def scaled_bench():
    import bench
    lengths = bench.contig_lengths(6_000_000)              # the bench genome, scaled down 500x
    sim = bench.workload_settings(lengths, extra=["-in", "0.001", "-inmax", "8", "-de", "0.001", "-demax", "9"])
    eng = _ffi.Engine(device=-1)
    eng.set_params(mm.params_descriptor(sim))
    cids = [eng.add_contig(np.zeros(L, dtype=np.uint8)) for L in lengths]
    # the per-contig calls, every contig planned: what every other path is held against
    eng.seed(42, 42)
    for ch in sim.chromosomes:
        eng.plan_contig(cids[ch.number], mm.plan_descriptors(ch))
    want = _digest(eng, cids, range(len(lengths)))
    yield eng, sim, cids, lengths, want, _state(eng)
    eng.close()


def _owned_cases():
    import bench
    from mutation_simulator_amd.sharding import lpt_partition
    lengths = bench.contig_lengths(6_000_000)
    parts = lpt_partition(lengths, 2)
    return [parts[0], parts[1], list(range(len(lengths))), []]


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("walk", [False, True])
def test_pass_equals_per_contig_calls_on_a_host_only_context(scaled_bench, case, walk):
    """``run_sharded_pass`` (one ``plan_pass`` call) against the per-contig calls: a rank's owned subset planned, the rest
    planned in full (``lengths=None``) or only walked (``msim_plan_chain`` items)."""
    from mutation_simulator_amd.sharding import run_sharded_pass
    eng, sim, cids, lengths, want, state = scaled_bench
    owned = _owned_cases()[case]
    eng.seed(42, 42)
    run_sharded_pass(eng, sim, cids, owned, mm.plan_table if walk else mm.plan_descriptors, apply=False,
                     lengths=lengths if walk else None)
    which = owned if walk else range(len(lengths))
    assert _digest(eng, cids, which) == {i: want[i] for i in which}
    assert _state(eng) == state


def test_pass_items_by_hand_and_errors(scaled_bench):
    """The item table itself: walked items carry their length, an unknown contig fails at its turn -- the items in front of it
    are planned, the ones behind it are not."""
    eng, sim, cids, lengths, want, state = scaled_bench
    eng.seed(42, 42)
    items = [(cids[ch.number], mm.plan_descriptors(ch), False) if ch.number % 3 else (None, mm.plan_descriptors(ch), False, lengths[ch.number])
             for ch in sim.chromosomes]
    eng.plan_pass(items)
    mine = [i for i in range(len(lengths)) if i % 3]
    assert _digest(eng, cids, mine) == {i: want[i] for i in mine}
    assert _state(eng) == state
    eng.plan_pass([])                                      # an empty pass is a pass
    assert _state(eng) == state
    eng.seed(42, 42)
    chs = list(sim.chromosomes)
    bad = [(cids[chs[0].number], mm.plan_descriptors(chs[0]), False), (10_000, mm.plan_descriptors(chs[1]), False),
           (cids[chs[2].number], mm.plan_descriptors(chs[2]), False)]
    with pytest.raises(_ffi.MsimError, match="no such contig"):
        eng.plan_pass(bad)
    ref = _ffi.Engine(device=-1)
    try:
        ref.set_params(mm.params_descriptor(sim))
        c0 = ref.add_contig(np.zeros(lengths[chs[0].number], dtype=np.uint8))
        ref.seed(42, 42)
        ref.plan_contig(c0, mm.plan_descriptors(chs[0]))
        assert _state(ref) == _state(eng)                  # (only the first item consumed anything)
    finally:
        ref.close()


# ---------------------------------------------------------------------- (2) the segmenting rule
def _params(titv=2.0):
    from test_gpu_sampler import _params as p
    return p(titv=titv)


def _snp(start, stop, k):
    from test_gpu_sampler import _snp_range
    return _snp_range(start, stop, k)


def _sv(L, k):
    from test_gpu_sampler import C3_CHANCES, C3_LENS, _sv_range
    return _sv_range(0, L - 1, k, C3_CHANCES, C3_LENS)


def _segments(items, py_pos=MT_N, np_pos=MT_N, max_chunks=0, ahead=2, params=None):
    """items: (contig or None, [ranges], length)."""
    lib = _ffi.load()
    table, keep = _ffi.Engine.pass_items([(c, r, False, L) if c is None else (c, r, False) for c, r, L in items])
    seg = (C.c_int32 * max(len(items), 1))()
    p = params or _params()
    assert lib.msim_dbg_pass_segments(C.byref(p), table, len(items), py_pos, np_pos, max_chunks, ahead, seg) == 0
    del keep
    return list(seg)[:len(items)]


def _contig(i, L, k):
    return (i, [_snp(0, L - 1, k)], L)


def test_first_contig_of_a_session_stays_and_the_rest_is_one_segment():
    """Behind an exact position a sample gains nothing from leaving the chain (and its window has no interval to lie in): the
    first contig takes the per-contig path, the eleven behind it are one segment."""
    items = [_contig(i, 3_000_000 + 100_000 * i, 90_000 + 1000 * i) for i in range(12)]
    assert _segments(items) == [0] + [1] * 11
    assert _segments(items, ahead=0) == [0] * 12           # MSIM_NO_AHEAD: nothing leaves the chain, nothing to hoist
    assert _segments(items, ahead=1) == [0] * 12           # MSIM_AHEAD=1: only a rank that walks other ranks' contigs plans ahead
    walked = [(None, r, L) if i in (0, 5) else (c, r, L) for i, (c, r, L) in enumerate(items)]
    assert _segments(walked, ahead=1) == [0] + [1] * 11    # ... from its first walked contig on; walked ones are hoisted as well
    assert _segments(items[:1]) == [0] and _segments([]) == []


def test_items_that_cut_a_segment():
    big = lambda i: _contig(i, 3_000_000, 100_000)
    two_ranges = (3, [_snp(0, 999_999, 30_000), _snp(1_000_000, 2_999_999, 60_000)], 3_000_000)
    nothing = (3, [], 900_000)
    sv = (3, [_sv(2_000_000, 16_000)], 2_000_000)
    small = (3, [_snp(0, 599_999, 100)], 600_000)          # k < 4096: the host planner's
    for cut, exact_behind in ((two_ranges, False), (nothing, False), (sv, True), (small, True)):
        items = [big(0), big(1), big(2), cut, big(4), big(5), big(6)]
        seg = _segments(items)
        assert seg[:4] == [0, 1, 1, 0], (cut, seg)
        # behind an item of the sampler's own the estimate goes on and the next segment starts at once; behind any other engine's
        # the position is exact again, and the first contig there stays on the chain
        assert seg[4:] == ([0, 2, 2] if exact_behind else [2, 2, 2]), (cut, seg)
    # a sample smaller than twice the uncertainty of its start stays on the chain -- and ends the segment in front of it
    items = [big(0), big(1), big(2), _contig(3, 700_000, 4096), big(4), big(5)]
    assert _segments(items) == [0, 1, 1, 0, 2, 2]


def test_a_segment_never_holds_more_sets_than_are_free():
    """32 scratch sets in turn, of which the last eight contigs' may still wait for their emission group: 24 a segment."""
    items = [_contig(i, 5_000_000, 250_000) for i in range(70)]   # (large samples: none smaller than the uncertainty of its start)
    seg = _segments(items)
    assert seg[0] == 0 and seg[1:25] == [1] * 24 and seg[25:49] == [2] * 24 and seg[49:] == [3] * 21


def test_a_rebase_cuts_the_segment_on_the_projected_position():
    """A four-chunk span (MSIM_DBG_JUMP_MAX_CHUNKS=4): the item in front of which the session would be re-based -- judged on the
    bound of the position the items before it leave -- ends the segment and starts, behind the re-base, at an exact position."""
    items = [_contig(i, 2_000_000, 30_000) for i in range(14)]
    seg = _segments(items, max_chunks=4)
    assert seg[0] == 0 and seg[1] == 1
    cuts = [i for i in range(1, 14) if seg[i] == 0]
    assert len(cuts) >= 2                                  # (the session ends every few contigs)
    for i in cuts:                                         # behind each: a new segment, one item later
        assert i + 1 >= 14 or seg[i + 1] == 0 or seg[i + 1] == seg[i - 1] + 1
    # the same list in a full-size span: one segment
    assert _segments(items) == [0] + [1] * 13
    # ... and started where nothing fits any more: the re-base comes in front of the first item, the rest is the same pass
    span = MT_N + 4 * 159_744
    assert _segments(items, py_pos=span - 10, max_chunks=4) == seg
