"""CPU tier of the tail-kernel tables: ``tests/sample_tail_ref.py`` (the contract ``tests/test_gpu_sample_tail_tables.py`` holds
k_sample_tail to) against ``tests/stream_ref.py`` -- itself held against ``random.sample`` -- on steered seeds whose events are
this kernel's: a cut on the last / first word of a count block, the k-th accepted draw on a block edge, a duplicate whose
replacement is a duplicate, many rounds, duplicates right behind an inexact start."""
from __future__ import annotations

import numpy as np
import pytest

import sample_tail_ref as tr
import stream_ref as sr

CASES = {c["name"]: c for c in sr.load_cases()}
NAMES = ["cut_word_2047_of_count_block", "cut_word_0_of_count_block", "kth_accept_2047_of_count_block", "kth_accept_0_of_count_block",
         "one_duplicate_redrawn_duplicate", "many_tail_rounds", "rejects_before_cut", "head_duplicate_pair", "head_value_redrawn_late"]
_PLANNED = {}


def _planned(name):
    """(tempered words, the steered sample's SamplePath, n, k) -- planned once per case."""
    if name not in _PLANNED:
        case = CASES[name]
        words, _, _, plans = sr.plan_case(case)
        ci, ri = case["target"]
        start, stop, k = sr.case_contigs(case)[ci][ri]
        n = (stop - (k - 1) * case["d"]) - start
        _PLANNED[name] = (words, plans[ci].samples[ri], n, k)
    return _PLANNED[name]


def test_untemper_inverts_temper():
    rs = np.random.RandomState(5)
    t = rs.randint(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)
    t[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    assert np.array_equal(tr.temper(tr.untemper(t)), t)
    assert np.array_equal(tr.untemper(tr.temper(t)), t)
    # ... and temper is the generator's own: state word 0 of a seeded generator that has not twisted again yields output 0
    import random
    r = random.Random(1)
    r.getrandbits(32)                                       # (forces the first twist; index 1 afterwards)
    st = r.getstate()[1]
    r2 = random.Random(1)
    assert int(tr.temper(np.array([st[0]], dtype=np.uint32))[0]) == r2.getrandbits(32)


@pytest.mark.parametrize("name", NAMES)
def test_rounds_and_cut_equal_the_stream_restatement(name):
    words, sp, n, k = _planned(name)
    s, end = sp.cut[0], sp.cut[k]
    W = min(len(words) - s, (end - s) + 2 * tr.ACC_BLOCK + 1)          # (not a multiple of the block)
    acc, counts, offs = tr.window_tables(words, s, W, n)
    assert np.array_equal(acc[:sp.consumed], np.array(sp.acc_val, dtype=np.uint32))
    bm, dups = tr.bitmap_of(acc[:k], n)
    st, out = tr.sample_tail(words, acc, offs, W, n, k, bm, {"pos": s, "snp_base": s, "dups": dups})
    assert st["flags"] == 0
    assert st["pos"] == end and st["snp_base"] == end
    assert st["accepted_used"] == sp.consumed and sp.consumed - k == sp.dups
    assert tr.bitmap_values(out).tolist() == sorted(sp.values)


@pytest.mark.parametrize("name", ["head_duplicate_pair", "one_duplicate_redrawn_duplicate", "cut_word_0_of_count_block"])
@pytest.mark.parametrize("head", [0, 1, 700])
def test_the_anchored_form_ends_where_the_plain_one_does(name, head):
    """The window anchored ``head`` words behind the exact start: a core of k_core draws from the anchor de-duplicated on its
    own, the accepted draws of [s, H) and the first need0 list entries behind the core inserted in any order (d1 of them were
    there already), then the rounds and the cut -- the same end, the same set."""
    words, sp, n, k = _planned(name)
    s, end = sp.cut[0], sp.cut[k]
    H = s + head
    head_vals = [v for i, v in zip(sp.acc_idx, sp.acc_val) if i < H]
    W = min(len(words) - H, (end - H) + 2 * tr.ACC_BLOCK - 1)
    acc, counts, offs = tr.window_tables(words, H, W, n)
    k_core = k - len(head_vals) - 40                                   # (a_max: any bound of the head's accepted draws)
    bm, dups_core = tr.bitmap_of(acc[:k_core], n)
    need0 = k - k_core + dups_core - len(head_vals)
    fringe = head_vals + acc[k_core:k_core + need0].tolist()
    d1 = 0
    for v in fringe:
        w, b = int(v) >> 5, np.uint32(1 << (int(v) & 31))
        d1 += 1 if bm[w] & b else 0
        bm[w] |= b
    st, out = tr.sample_tail(words, acc, offs, W, n, k_core, bm, {"pos": s, "snp_base": s}, win=(H, need0, d1))
    assert st["flags"] == 0 and st["pos"] == end
    assert st["accepted_used"] == sp.consumed - len(head_vals)
    assert tr.bitmap_values(out).tolist() == sorted(sp.values)


def test_a_short_window_raises_the_flag_and_writes_nothing_else():
    words, sp, n, k = _planned("many_tail_rounds")
    s = sp.cut[0]
    W = sp.acc_idx[sp.consumed - 2] - s + 1                            # ends one accepted draw early
    acc, counts, offs = tr.window_tables(words, s, W, n)
    bm, dups = tr.bitmap_of(acc[:k], n)
    st, _ = tr.sample_tail(words, acc, offs, W, n, k, bm, {"pos": s, "snp_base": s, "dups": dups})
    assert st["flags"] == tr.FLAG_SAMPLE_OVERFLOW and st["pos"] == s and st["accepted_used"] == 0


def test_a_cut_beyond_the_limit_is_clamped():
    words, sp, n, k = _planned("many_tail_rounds")
    s, end = sp.cut[0], sp.cut[k]
    W = (end - s) + 100
    acc, counts, offs = tr.window_tables(words, s, W, n)
    bm, dups = tr.bitmap_of(acc[:k], n)
    st, _ = tr.sample_tail(words, acc, offs, W, n, k, bm, {"pos": s, "snp_base": s, "dups": dups}, pos_limit=end - 1)
    assert st["flags"] == tr.FLAG_SAMPLE_OVERFLOW and st["pos"] == end - 1 and st["accepted_used"] == sp.consumed
    st, _ = tr.sample_tail(words, acc, offs, W, n, k, bm, {"pos": s, "snp_base": s, "dups": dups}, pos_limit=end)
    assert st["flags"] == 0 and st["pos"] == end
