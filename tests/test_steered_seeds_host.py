"""CPU tier of the steered seeds (tests/golden/steered_seeds.json, searched by tests/golden/find_steered_seeds.py): the
word-level restatement ``stream_ref`` against CPython's own ``random.sample`` / ``random.random`` / ``randint`` and against the
host planner (a host-only context), and -- what keeps the table honest when someone edits it -- every fixture case recomputed
from its seed produces the event it claims.  ``tests/test_gpu_steered.py`` then runs the production engine on the same cases
against the restatement alone."""
from __future__ import annotations

import random

import numpy as np
import pytest

import stream_ref as sr
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import mutator as mm
from steered_run import K_CAP_LIFTED, params as _params, snp_range

CASES = sr.load_cases()
NAMES = [c["name"] for c in CASES]


ARBITRARY = [((1 << 20) - 1, 5000), (1 << 20, 5000), ((1 << 20) + 1, 5000), (1 << 16, 700), ((1 << 16) - 1, 300), ((1 << 16) + 1, 300),
             (1_000_003, 30_000), (70_000, 4_000), (131_071, 21_000), (3_000_000, 1), (50_021, 1_000), (4_194_303, 41_000)]


@pytest.mark.parametrize("n,k", ARBITRARY)
def test_sample_set_path_equals_random_sample(n, k):
    assert n > mm.sample_setsize(k)                                    # (CPython's set path)
    for seed, skip in ((n + k, 0), (n ^ k, 17)):
        words, p, mt = sr.make_stream(seed, skip, 3 * k + 4096)
        ref = random.Random()
        ref.setstate((3, tuple(int(x) for x in mt) + (p,), None))
        want = ref.sample(range(n), k)
        sp = sr.sample_set_path(words, p, n, k)
        assert sp.values == want
        assert [ref.getrandbits(32) for _ in range(8)] == words[sp.cut[k]:sp.cut[k] + 8].tolist()
        assert sp.cut[0] == p and sp.dups == sp.consumed - k and len(sp.cut) == k + 1
        # a prefix of the sample is the smaller sample: one pass yields the cut of every k
        j = max(1, k // 3)
        if n > mm.sample_setsize(j):
            small = sr.sample_set_path(words, p, n, j)
            assert small.values == want[:j] and small.cut[j] == sp.cut[j]


@pytest.mark.parametrize("name", NAMES)
def test_fixture_samples_equal_random_sample(name):
    case = CASES[NAMES.index(name)]
    words, p, mt, plans = sr.plan_case(case)
    ref = random.Random(case["seed"][0])
    for _ in range(case["skip"]):
        ref.getrandbits(32)
    assert ref.getstate()[1][:-1] == tuple(int(x) for x in mt) and ref.getstate()[1][-1] == p
    d = case["d"]
    p_ti = case["titv"] * (1 / (case["titv"] + 1))
    for ranges, cp in zip(sr.case_contigs(case), plans):
        pos = []
        for (start, stop, k), sp in zip(ranges, cp.samples):
            sampl = ref.sample(range(start, stop - (k - 1) * d), k)        # util.py:104
            assert [start + v for v in sp.values] == sampl
            pos += [s + d * r for r, s in enumerate(sorted(sampl))]
        assert cp.recs["pos"].tolist() == pos
        aux = [0 if ref.uniform(0, 1) <= p_ti else 1 + ref.randint(0, 1) for _ in pos]      # mutator.py:436-441, :455
        assert cp.recs["aux"].tolist() == aux
    assert [ref.getrandbits(32) for _ in range(8)] == words[plans[-1].end:plans[-1].end + 8].tolist()


@pytest.mark.parametrize("titv", [0.0, 0.5, 1.0, 2.0, 1e9, 1e300, float("inf")])
def test_snp_draws_equal_a_literal_loop(titv):
    words, p, mt = sr.make_stream(99, 5, 40_000)
    ref = random.Random()
    ref.setstate((3, tuple(int(x) for x in mt) + (p,), None))
    p_ti = titv * (1 / (titv + 1))
    want = [0 if ref.uniform(0, 1) <= p_ti else 1 + ref.randint(0, 1) for _ in range(6000)]
    assert sr.ti_lim_of(titv) == mm.params_descriptor(type("S", (), {"mut_block": {}, "titv": titv})).ti_lim
    sd = sr.snp_draws(words, p, 6000, sr.ti_lim_of(titv))
    assert list(sd.aux) == want
    assert [ref.getrandbits(32) for _ in range(8)] == words[sd.end:sd.end + 8].tolist()
    assert sd.spans[0][0] == p and all(a[1] == b[0] for a, b in zip(sd.spans, sd.spans[1:])) and sd.spans[-1][1] == sd.end


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_host_planner(name):
    case = CASES[NAMES.index(name)]
    words, p, mt, plans = sr.plan_case(case)
    K = sum(len(cp.recs) for cp in plans)
    np_mt, np_pos, np_next = sr.numpy_stream(case["seed"][1], 2 * K)
    eng = _ffi.Engine(-1, _ffi.PLAN_HOST)
    try:
        eng.set_mt_state(0, mt, p)
        eng.set_mt_state(1, np_mt, np_pos)
        eng.set_params(_params(case["d"], case["titv"]))
        for c, cp in zip(case["contigs"], plans):
            cid = eng.add_contig(np.zeros(c["L"], dtype=np.uint8))     # (a host-only context keeps no bases)
            eng.plan_contig(cid, [snp_range(*r) for r in c["ranges"]])
            recs, pool = eng.fetch_records(cid)
            assert recs.tobytes() == cp.recs.tobytes() and len(pool) == 0
            assert not eng.plan_was_empty(cid)
        st = eng.stats()
        assert st["py_words"] == plans[-1].end - p and st["np_words"] == 2 * K
        assert sr.next_words(*eng.get_mt_state(0)) == words[plans[-1].end:plans[-1].end + 8].tolist()
        assert sr.next_words(*eng.get_mt_state(1)) == np_next
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_every_case_produces_the_event_it_claims(name):
    case = CASES[NAMES.index(name)]
    words, p, mt, plans = sr.plan_case(case)
    ci, ri = case["target"]
    sr.check_event(case["event"], words, plans, (ci, ri), sr.case_contigs(case)[ci], case["d"])
    d = case["d"]
    for c in case["contigs"]:                                           # ... and the SNP sampler takes every contig of it
        prev = -1
        for start, stop, k in c["ranges"]:
            n = (stop - (k - 1) * d) - start
            assert k >= 4096 and n > mm.sample_setsize(k) and c["L"] - k > mm.sample_setsize(k) and prev < start <= stop < c["L"]
            prev = stop
    K = sum(r[2] for r in case["contigs"][ci]["ranges"])
    assert 100_000 <= case["contigs"][ci]["L"] <= 5_000_000
    # the restatement's budget: k <= 60 000 (+ the 4096 of a two-range contig's first range), lifted for the named cases only
    assert K <= (160_000 + 4096 if name.replace("two_ranges_", "") in K_CAP_LIFTED else 60_000 + 4096), K


def test_the_fixture_covers_every_event_kind():
    kinds = {c["event"]["kind"] for c in CASES}
    assert kinds == {"cut_word_in_count_block", "cut_word_in_scatter_block", "kth_accept_in_count_block", "no_duplicate",
                     "one_duplicate_redrawn_duplicate", "many_tail_rounds", "rejects_before_cut", "starts_in_copied_state_words",
                     "sample_ends_at", "snp_ends_at", "first_and_last_value", "bin_border_values_with_duplicates",
                     "last_value_of_n", "snp_start_in_block", "snp_last_word_in_block", "random_straddles",
                     "retry_loop_straddles_block", "long_retry_loop", "last_snp_ends_in_retry_loop", "head_duplicate_pair",
                     "head_value_redrawn_late"}
    assert len(set(NAMES)) == len(NAMES)
    assert {c["event"]["n"] for c in CASES if c["event"]["kind"] == "last_value_of_n"} >= {
        1 << 20, (1 << 20) + 1, (1 << 20) - 1, 3 << 20, (3 << 20) + 1, (3 << 20) - 1}
    handover = sr.MT_N + sr.MT_CHUNK_WORDS
    for kind in ("sample_ends_at", "snp_ends_at"):
        assert {c["event"]["at"] for c in CASES if c["event"]["kind"] == kind} == {handover - 1, handover, handover + 1}


def test_the_search_regenerates_the_fixture():
    """Two cheap recipes through the search tool itself (the whole search: ``find_steered_seeds.py --check``)."""
    import find_steered_seeds as fs
    assert list(fs.RECIPES) == NAMES
    for name in ("cut_word_2047_of_count_block", "state_index_623"):
        assert fs.build_case(name) == CASES[NAMES.index(name)]
    assert fs.dumps(CASES) == (fs.OUT).read_text()
