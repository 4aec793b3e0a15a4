"""The counting passes one behind the other on ONE context: every pass zeroes, fills and fetches a small block of counters (csrc/
counter_trip.h), and this is the test of counters surviving from one user to the next -- ``cmp_counts``, ``cmp_counts_blocks``, the
join, ``cmp_counts_diploid``, the region passes over a diploid and a haploid count, ``cmp_phase_counts``, ``sbs_counts`` and
``context_counts`` in a row, then ``cmp_counts_diploid`` and ``cmp_counts`` again.  Every result equals the library's sequential
restatement and the repeated calls equal their first results; all comparisons are exact integers and bytes.

The tables hold 16 passes and one record: the slot a workgroup adds to (its index & 15) wraps once, so two workgroups share a slot.
"""
from __future__ import annotations

import numpy as np
import pytest

import cmp_twin as tw
from mutation_simulator_amd import _ffi

pytestmark = pytest.mark.gpu

PASS = _ffi.CMP_PASS
N = 16 * PASS + 1
L = 6 * N                                                  # tw.random_tables advances 4.5 bases a record on average
TRUTH, CALLS = _ffi.CMP_TRUTH, _ffi.CMP_CALLS


def tables():
    """(bases, truth, truth pool, calls, calls pool, the calls' second haplotype): two random tables of N records of SNs and short
    indels on a two-letter contig, and the truth without every fifth record."""
    g, a, pa, b, pb, _ = tw.random_tables(41, L=L, n=N)
    assert len(a) == N and len(b) == N, (len(a), len(b))
    return g, a, pa, b, pb, a[np.arange(N) % 5 != 0]


def equal(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert np.array_equal(g, w), (what, k, np.flatnonzero((g != w).reshape(-1))[:8].tolist())


def hold_and_plan(eng, cid, held, current):
    eng.set_records(cid, *held)
    eng.cmp_hold(cid)
    eng.set_records(cid, *current)


def test_passes_in_a_row_leave_each_other_nothing():
    g, a, pa, b, pb, a2 = tables()
    sets = [(np.array([100], dtype=np.uint32), np.array([L // 2], dtype=np.uint32)),
            (np.arange(0, L - 64, 128, dtype=np.uint32), np.arange(64, L, 128, dtype=np.uint32))]
    with _ffi.Engine(0) as eng:
        cid = eng.add_contig(g)
        hold_and_plan(eng, cid, (a, pa), (b, pb))
        first = eng.cmp_counts(cid) + eng.cmp_fetch(cid)[2:]
        equal(first, _ffi.cmp_counts_host(g, a, pa, b, pb), "cmp_counts")
        assert 0 < int(first[0][..., 0].sum()) < N             # some records match, some do not
        blocks = eng.cmp_counts_blocks(cid) + eng.cmp_fetch(cid)[2:]
        equal(blocks, _ffi.cmp_counts_blocks_host(g, a, pa, b, pb), "cmp_counts_blocks")

        eng.cmp_join(cid, TRUTH)                               # haplotypes a and b; the held table is consumed
        hold_and_plan(eng, cid, (b, pb), (a2, pa))
        eng.cmp_join(cid, CALLS)                               # haplotypes b and a2
        ut, uc = _ffi.cmp_join_host(a, pa, b, pb), _ffi.cmp_join_host(b, pb, a2, pa)
        for side, want in ((TRUTH, ut), (CALLS, uc)):
            equal(eng.cmp_fetch_diploid(cid, side, flags=False)[:3], want, ("cmp_join", side))
        diploid = lambda: eng.cmp_counts_diploid(cid) + (eng.cmp_fetch_diploid(cid, TRUTH)[3], eng.cmp_fetch_diploid(cid, CALLS)[3])   # noqa: E731
        first_diploid = diploid()
        equal(first_diploid, _ffi.cmp_counts_diploid_host(g, *ut, *uc), "cmp_counts_diploid")
        assert int(first_diploid[0][..., 1].sum()) > 0         # genotype mismatches: the third outcome is in use

        for s, (starts, ends) in enumerate(sets):
            eng.cmp_regions_set(cid, s, starts, ends)
        eng.cmp_regions_mark(cid, diploid=True)
        marks = eng.cmp_fetch_regions(cid, diploid=True)
        for mask in (1, 3):
            want = _ffi.cmp_counts_regions_host(g, ut[0], ut[1], first_diploid[2], uc[0], uc[1], first_diploid[3], 3, sets, mask)
            equal(eng.cmp_counts_regions(cid, mask, diploid=True) + marks, want, ("cmp_counts_regions, diploid", mask))
        hold_and_plan(eng, cid, (a, pa), (b, pb))              # a fresh hold: the haploid count's tables again
        equal(eng.cmp_counts(cid) + eng.cmp_fetch(cid)[2:], first, "cmp_counts behind the diploid passes")
        eng.cmp_regions_mark(cid)
        marks = eng.cmp_fetch_regions(cid)
        for mask in (2, 3):
            want = _ffi.cmp_counts_regions_host(g, a, pa, first[2], b, pb, first[3], 2, sets, mask)
            equal(eng.cmp_counts_regions(cid, mask) + marks, want, ("cmp_counts_regions, haploid", mask))
            assert 0 < int(want[1][0]) < N

        rs = np.random.RandomState(7)
        words = [rs.randint(0, 4, len(u[0])).astype(np.uint32) for u in (ut, uc)]      # 0: unphased; three phase sets a side
        eng.cmp_phase_set(cid, TRUTH, words[0])
        eng.cmp_phase_set(cid, CALLS, words[1])
        want = _ffi.cmp_phase_host(g, *ut, words[0], *uc, words[1])
        equal((eng.cmp_phase_counts(cid), eng.cmp_fetch_phase(cid, TRUTH)[1]), want, "cmp_phase_counts")
        assert int(want[0][2]) > 0                             # informative pairs

        equal(eng.sbs_counts(cid), _ffi.sbs_counts_host(g, b), "sbs_counts")
        counts, n_valid = eng.context_counts(cid)
        want = _ffi.context_counts_host(g)
        assert np.array_equal(counts, want[0]) and n_valid == want[1] > 0

        equal(diploid(), first_diploid, "cmp_counts_diploid again")
        equal(eng.cmp_counts(cid) + eng.cmp_fetch(cid)[2:], first, "cmp_counts again")
