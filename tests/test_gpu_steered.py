"""The SNP sampler (plan_gpu.hip: plan_contig_gpu) on seeds SEARCHED so that the genuine MT19937 stream puts an event on an
edge of the kernels' tilings: the final accepted draw on the last word of a 2048-word count block, the first-k / tail split on a
block border, a ``randbelow(2)`` retry loop across two absolute 8192-word transducer blocks, the last value of a partial bin,
the end of a sample on the hand-over between two generated chunks, ...  (tests/golden/steered_seeds.json; an arbitrary seed
meets such a word once in thousands of contigs.)  tests/test_steered_seeds_host.py proves on the CPU that every case produces
its event and ties the restatement to ``random.sample`` and to the host planner; here the unmodified production engine must
equal the restatement -- ``stream_ref.plan_snp_contig``, never the host planner -- under every scheduling policy.

Policies libmsim reads per context are set with ``monkeypatch`` before the context exists; ``MSIM_NO_SCAN_FOLD``,
``MSIM_NO_AUX_FOLD`` and ``MSIM_DBG_AHEAD_LOG`` are read once per process, so those runs happen in ONE fresh process per policy
(tests/steered_run.py over every case), whose per-case verdicts the parametrised tests below assert."""
from __future__ import annotations

import functools
import json
import math
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import stream_ref as sr
from mutation_simulator_amd import _ffi
from steered_run import params as _params, run_case, snp_range

pytestmark = pytest.mark.gpu

CASES = sr.load_cases()
NAMES = [c["name"] for c in CASES]
ANCHORED = [c["name"] for c in CASES if c["event"]["kind"].startswith("head_")]

CONTEXT_POLICIES = {                       # read when the context is created
    "default": {},
    "no_ahead": {"MSIM_NO_AHEAD": "1"},
    "emit_group_1": {"MSIM_EMIT_GROUP": "1"},
    "emit_group_4": {"MSIM_EMIT_GROUP": "4"},
}
PROCESS_POLICIES = {                       # read once per process
    "no_ahead_no_scan_fold": ({"MSIM_NO_AHEAD": "1", "MSIM_NO_SCAN_FOLD": "1"}, []),
    "no_aux_fold": ({"MSIM_NO_AUX_FOLD": "1"}, []),
    "ahead_log": ({"MSIM_DBG_AHEAD_LOG": "1"}, ["--ahead-log"] + ANCHORED),
}
CLEAN = ("MSIM_NO_AHEAD", "MSIM_AHEAD", "MSIM_EMIT_GROUP", "MSIM_NO_SCAN_FOLD", "MSIM_NO_AUX_FOLD", "MSIM_NO_EMIT_GROUP",
         "MSIM_EMIT_TRAIN", "MSIM_AHEAD_SIGMA", "MSIM_AHEAD_FIRST", "MSIM_PLAN_MODE")


@functools.lru_cache(maxsize=2)
def _planned(name):
    """The restatement of one case, computed once and shared by its policies (the case is the slowest-varying parameter)."""
    return sr.plan_case(CASES[NAMES.index(name)])


@pytest.mark.parametrize("policy", list(CONTEXT_POLICIES))
@pytest.mark.parametrize("name", NAMES)
def test_steered_case_equals_the_restatement(monkeypatch, name, policy):
    for v in CLEAN:
        monkeypatch.delenv(v, raising=False)
    for k, v in CONTEXT_POLICIES[policy].items():
        monkeypatch.setenv(k, v)
    case = CASES[NAMES.index(name)]
    st = run_case(case, _planned(name))
    if len(case["contigs"]) > 1 and len(case["contigs"][1]["ranges"]) == 1:
        # the second contig's sample is anchored ahead of the chain by default, on the chain with MSIM_NO_AHEAD
        assert st["snp_samples_ahead"] == (0 if policy == "no_ahead" else 1)
    else:
        assert st["snp_samples_ahead"] == 0                            # (a context's first sample starts at an exact position)


@pytest.mark.parametrize("name", NAMES)
def test_steered_case_through_apply(monkeypatch, name):
    """PLAN + APPLY enqueued together (the emission group writes the APPLY tile index from its registers), the mutated sequence
    against ``apply_ref`` on the restatement's table."""
    for v in CLEAN:
        monkeypatch.delenv(v, raising=False)
    run_case(CASES[NAMES.index(name)], _planned(name), apply=True)


_CHILDREN = {}          # policy -> (verdicts, exit status, end of stderr) of its fresh process; failures are kept too
_ABNORMAL = []          # set once a fresh process died of a signal or ran into its limit: nothing more is started on the GPU


def _stop_after_an_abnormal_end():
    if _ABNORMAL:
        pytest.fail(f"a fresh process ended abnormally ({_ABNORMAL[0]}): nothing more from this file runs on the GPU", pytrace=False)


def _fresh_process(policy, tmp_dir):
    if policy in _CHILDREN:
        return _CHILDREN[policy]
    _stop_after_an_abnormal_end()
    env, args = PROCESS_POLICIES[policy]
    out = tmp_dir / f"{policy}.json"
    child_env = {k: v for k, v in os.environ.items() if k not in CLEAN}
    child_env.update(env)
    cmd = [sys.executable, str(Path(__file__).with_name("steered_run.py")), str(out)] + args
    try:
        r = subprocess.run(cmd, env=child_env, capture_output=True, text=True, timeout=600)
        rc, err = r.returncode, r.stderr[-2000:]
    except subprocess.TimeoutExpired as e:
        rc, err = "time limit", str(e.stderr or "")[-2000:]
    results = json.loads(out.read_text()) if out.exists() else {}
    if rc != 0:                                                        # (the script returns 0 whatever its verdicts are)
        _ABNORMAL.append(f"policy {policy}: exit {rc}")
    _CHILDREN[policy] = (results, rc, err)
    return _CHILDREN[policy]


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("steered_children")


@pytest.mark.parametrize("policy,name", [(p, n) for p in ("no_ahead_no_scan_fold", "no_aux_fold") for n in NAMES] +
                         [("ahead_log", n) for n in ANCHORED])
def test_steered_case_under_a_process_wide_policy(policy, name, child_dir):
    """``ahead_log``: the default policy with the engine's own log of the anchored window -- the steered words of cases 18 / 19
    must lie in the head interval [lo, H) it really used (and the late duplicate inside its core)."""
    results, rc, err = _fresh_process(policy, child_dir)
    assert name in results, f"the run ended (exit {rc}) before this case: {results}\n{err}"
    assert results[name] == "ok", results[name]


# ---------------------------------------------------------------------------------------------- more than 8192 count blocks
def _count_blocks(n, k):
    """``nb`` of plan_gpu.hip: enqueue_sample_chain."""
    bits = n.bit_length()
    p_acc = n / float(1 << bits)
    need_acc = -n * math.log1p(-k / n)
    target = need_acc + 16.0 * math.sqrt(need_acc) + 4096.0
    W = int(target / p_acc + 16.0 * math.sqrt(target) / p_acc + 8192.0)
    return (W + sr.ACC_BLOCK - 1) // sr.ACC_BLOCK


@pytest.mark.parametrize("L,k,side", [(100_000_000, 16_500_000, "above"), (74_900_000, 7_700_000, "below"), (75_007_000, 7_807_000, "equal")])
def test_window_count_blocks_around_tail_lds_offs(monkeypatch, L, k, side):
    """A window of more than TAIL_LDS_OFFS = 8192 count blocks: k_sample_tail reads the block offsets from global memory and
    k_scan_u32_w4 runs on the chain (a 3 Gb genome's largest contig has ~1300 blocks); one just below; and exactly 8192, where
    the host already launches the scan (``nb < TAIL_LDS_OFFS`` fails) while the kernel still keeps the offsets in LDS
    (``n_blocks <= TAIL_LDS_OFFS``).  Which branch ran is known from the formula alone: the engine reports none.  Not steered -- the
    host planner is the reference (tens of millions of draws are beyond the Python restatement)."""
    _stop_after_an_abnormal_end()
    for v in CLEAN:
        monkeypatch.delenv(v, raising=False)
    from mutation_simulator_amd.mutator import sample_setsize
    assert L - k > sample_setsize(k)                                   # (the set path: the SNP sampler takes the range)
    nb = _count_blocks(L - k, k)
    assert {"above": nb > sr.TAIL_LDS_OFFS, "below": 0.85 * sr.TAIL_LDS_OFFS < nb < sr.TAIL_LDS_OFFS, "equal": nb == sr.TAIL_LDS_OFFS}[side], nb
    params = _params(1, 2.0)
    out = []
    t0 = time.time()
    for flags in (_ffi.PLAN_HOST, _ffi.PLAN_GPU):
        eng = _ffi.Engine(0, flags)
        try:
            eng.seed(5, 6)
            eng.set_params(params)
            cid = eng.add_contig_synthetic(L, 7)
            eng.plan_contig(cid, [snp_range(0, L - 1, k)])
            recs, pool = eng.fetch_records(cid)
            out.append((recs, eng.stats(), sr.next_words(*eng.get_mt_state(0)), sr.next_words(*eng.get_mt_state(1))))
        finally:
            eng.close()
    print(f"nb {nb}: {time.time() - t0:.1f} s")
    (hr, hst, hpy, hnp), (gr, gst, gpy, gnp) = out
    assert len(gr) == k and np.array_equal(hr.view(np.uint8), gr.view(np.uint8))
    assert (hst["py_words"], hst["np_words"]) == (gst["py_words"], gst["np_words"]) and hpy == gpy and hnp == gnp
    assert gst["plan_gpu_ms"] > 0 and gst["plan_host_ms"] == 0 and gst["contigs_snp"] == 1
