"""CPU tier: the stream-window arithmetic of the device PLAN engines (csrc/plan_windows.h) still computes what it computed when
every engine and ``gpu_plan_make_room`` carried a copy of its own.

``gpu_plan_make_room`` decides from these sums whether a contig's windows fit into what is left of the session's jump-table span;
the engines size their windows with the same functions.  A need that fell below a window would surface as "stream window
overflowed its session's jump-table span" on a 20 Gb genome -- which no test reaches -- so the arithmetic is pinned here:
``tests/golden/stream_need.json`` holds, for 40 range tables, the need (py, np, bad) and, for the first range, the big-sample
window, the small-sample mean and variance bound and the least randint acceptance, RECORDED FROM THE PARENT COMMIT (its own
expressions behind the same export: tests/golden/make_stream_need.py tells how).

Tolerance: each double to a relative 1e-12 -- the expressions are a handful of correctly rounded operations and one log1p, and
inlining may contract a multiply-add differently (a few ulp); 1e-12 is thousands of ulp and, on a window of at most 4e9 words,
0.004 words.  ``bad`` is exact; infinities and NaNs (the big-sample window of a range with k >= n) compare as such.
"""
from __future__ import annotations

import json
import math
import sys
from pathlib import Path

import pytest

from mutation_simulator_amd import _ffi

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_stream_need as msn  # noqa: E402

DOC = json.loads((GOLDEN / "stream_need.json").read_text())
CASES = {c["name"]: c for c in DOC["cases"]}
REL = 1e-12


def _same(got, want):
    if math.isnan(want) or math.isinf(want):
        return math.isnan(got) if math.isnan(want) else got == want
    return abs(got - want) <= REL * abs(want)


def test_table_is_the_recorded_parent_and_covers_the_paths():
    assert DOC["parent"] == "b754764abd8b20d00cff209baa198cc47dd5f343" and len(CASES) == len(DOC["cases"]) >= 40
    assert [{k: v for k, v in c.items() if k != "expect"} for c in DOC["cases"]] == msn.cases()     # the JSON's inputs are the script's
    e = {n: c["expect"] for n, c in CASES.items()}
    assert e["pool_k100"]["small_e"] == e["pool_k100"]["small_v"] == 200.0                          # pool path: 2k / 2k
    assert e["small_k_eq_n_guard"]["small_e"] == 64.0 * 500 / (500 / 512)                           # the 64 k guard
    assert math.isinf(e["small_k_eq_n_guard"]["big_window"]) and math.isfinite(e["big_k_eq_n_guard"]["py"])
    assert all(e[n]["bad"] for n in ("n_lt_k_small", "n_lt_k_pool", "n_lt_k_second_range", "n_2p32", "n_beyond_2p33"))
    assert sum(x["bad"] for x in e.values()) == 5
    assert e["thresholds_0_and_2p53"]["acc_min"] == 1.0 and e["odd_widths"]["acc_min"] == 0.75
    assert e["big_n_2m_plus_1"]["big_window"] > 1.5 * e["big_n_2m_minus_1"]["big_window"]           # p_acc near 1/2 and near 1
    assert len(CASES["table_2000_three_settings"]["ranges"]) == 2000


@pytest.mark.parametrize("name", list(CASES))
def test_stream_need_matches_the_parent(name):
    case = CASES[name]
    got, want = msn.stream_need(_ffi.load(), case), case["expect"]
    print(name, {f: (got[f], want[f]) for f in msn.FIELDS})
    assert got["bad"] is want["bad"]
    for f in msn.FIELDS:
        if f != "bad":
            assert _same(got[f], want[f]), (f, got[f], want[f])
