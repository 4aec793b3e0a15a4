"""The chain of an anchored contig as ONE launch (``k_chain_fused``: fringe grid, last workgroup goes on with tail rounds, stream
cut and SNP cut) through the product path, three ways: the default, ``MSIM_NO_CHAIN_FUSE=1`` (the three launches) and the
sequential host planner -- records, insert pools, the words both streams consumed, the next 8 words of both streams and the
per-engine counters.  ``Engine.chains_fused`` says how many contigs took the fused launch, so that a case is known to run what it
is meant for (and the knob to switch it off).

The kernel itself, on hand-built tables: ``tests/test_gpu_chain_step_tables.py``."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from mutation_simulator_amd import _ffi
from test_gpu_ahead import _genome, _same
from test_gpu_sampler import C3_CHANCES, C3_LENS, _params, _snp_range, _sv_range

pytestmark = pytest.mark.gpu

COUNTERS = ("contigs_snp", "contigs_svmix", "contigs_hostcut", "contigs_hostchain", "contigs_host", "snp_samples_ahead", "py_words",
            "np_words", "stream_rebases")


def _run(flags, contigs, params, seed, mode="pass", chain_only=(), apply=False, passes=1):
    """As ``tests/test_gpu_plan_pass.py``'s: nothing synchronises before the last pass is enqueued; then everything is read.
    Also returns the fused launches the context sent."""
    eng = _ffi.Engine(0, flags)
    try:
        eng.seed(*seed)
        eng.set_params(params)
        cids = [None if i in chain_only else eng.add_contig_synthetic(L, 7) for i, (L, _) in enumerate(contigs)]
        for _ in range(passes):
            if mode == "pass":
                eng.plan_pass([(None, r, False, L) if cid is None else (cid, r, apply) for cid, (L, r) in zip(cids, contigs)])
            else:
                for cid, (L, r) in zip(cids, contigs):
                    if cid is None:
                        eng.plan_chain(L, r)
                    else:
                        eng.plan_contig(cid, r)
                        if apply:
                            eng.apply_contig(cid)
        out, applied = [], []
        for cid in cids:
            if cid is None:
                out.append(None)
                continue
            recs, pool = eng.fetch_records(cid)
            out.append((recs.copy(), pool.copy()))
            if apply:
                applied.append((eng.result_checksum(cid), eng.result_sizes(cid)))
        st = eng.stats()
        states = [eng.get_mt_state(0), eng.get_mt_state(1)]
        return out, states, st, applied, eng.chains_fused() if flags != _ffi.PLAN_HOST else 0
    finally:
        eng.close()


def _three_ways(monkeypatch, contigs, params, seed, gpu_flags=_ffi.PLAN_GPU, **kw):
    """Host planner, the three launches, the fused launch; returns (stats, fused launches) of the default."""
    host, hs, hst, happ, _ = _run(_ffi.PLAN_HOST, contigs, params, seed, **kw)
    monkeypatch.setenv("MSIM_NO_CHAIN_FUSE", "1")
    three, ts, tst, tapp, n_three = _run(gpu_flags, contigs, params, seed, **kw)
    monkeypatch.delenv("MSIM_NO_CHAIN_FUSE")
    one, os_, ost, oapp, n_one = _run(gpu_flags, contigs, params, seed, **kw)
    assert n_three == 0
    _same(host, three, hs, ts, hst, tst)
    _same(host, one, hs, os_, hst, ost)
    for key in COUNTERS:
        assert ost[key] == tst[key], (key, ost[key], tst[key])
    assert oapp == tapp == happ
    return ost, n_one


def _big(rs, n, lo=2_000_000, hi=4_000_000, rate=(0.03, 0.05)):
    return _genome(rs, n, lo=lo, hi=hi, rate=rate)


@pytest.mark.parametrize("n_contigs", [2, 9, 40])
def test_passes_of_n_contigs(monkeypatch, n_contigs):
    """Every contig whose sample is an anchored window takes the fused launch (not the first: its start is exact, it samples on
    the chain; nor one smaller than twice the uncertainty of its start); 40 is more than the scratch sets, so every header's
    ticket word is used a second time (zeroed by the prep's count body in between)."""
    rs = np.random.RandomState(200 + n_contigs)
    contigs = _genome(rs, n_contigs, lo=600_000, hi=6_000_000, rate=(0.03, 0.05))
    st, n_fused = _three_ways(monkeypatch, contigs, _params(titv=2.0), (n_contigs, n_contigs + 1))
    assert st["snp_samples_ahead"] == n_fused and n_contigs // 2 <= n_fused < n_contigs


def test_the_per_contig_calls_fuse_as_well(monkeypatch):
    rs = np.random.RandomState(7)
    st, n_fused = _three_ways(monkeypatch, _big(rs, 6), _params(titv=0.5), (3, 4), mode="calls")
    assert n_fused == st["snp_samples_ahead"] >= 4


def test_two_passes_without_a_synchronising_call_between_them(monkeypatch):
    rs = np.random.RandomState(61)
    st, n_fused = _three_ways(monkeypatch, _big(rs, 13), _params(titv=2.0), (12, 13), passes=2)
    assert n_fused == st["snp_samples_ahead"] >= 24


@pytest.mark.parametrize("group", [1, 3, 4])
def test_emission_group_sizes_with_apply(monkeypatch, group):
    """``_three_ways`` compares ``result_checksum`` / ``result_sizes`` of every contig as well."""
    monkeypatch.setenv("MSIM_EMIT_GROUP", str(group))
    rs = np.random.RandomState(70 + group)
    st, n_fused = _three_ways(monkeypatch, _big(rs, 10), _params(titv=2.0), (2, 2), apply=True)
    assert n_fused == st["snp_samples_ahead"] >= 8


@pytest.mark.parametrize("owned", [(0, 4, 8), (1, 2, 3, 9), ()])
def test_walked_contigs_and_an_owned_subset(monkeypatch, owned):
    """Contigs a sharded rank only walks (msim_plan_chain: no emission group, so the scratch set's chain_done event is recorded
    behind the fused launch) between owned ones."""
    rs = np.random.RandomState(21)
    contigs = _big(rs, 10)
    others = tuple(i for i in range(len(contigs)) if i not in owned)
    st, n_fused = _three_ways(monkeypatch, contigs, _params(titv=2.0), (8, 9), chain_only=others, apply=True)
    assert st["contigs_snp"] == len(owned) and n_fused == st["snp_samples_ahead"] == 9


def test_more_walked_contigs_than_scratch_sets(monkeypatch):
    """69 walked contigs: a set's next user waits for the chain_done event behind the fused launch of the one before."""
    rs = np.random.RandomState(11)
    contigs = _genome(rs, 70, lo=3_000_000, hi=5_000_000, rate=(0.04, 0.05))
    st, n_fused = _three_ways(monkeypatch, contigs, _params(titv=2.0), (4, 5), chain_only=tuple(range(1, 70)), mode="calls")
    assert n_fused == st["snp_samples_ahead"] >= 45


def test_the_first_contig_fused_too_in_a_fresh_process(tmp_path):
    """MSIM_AHEAD_FIRST=1 is read once a process, so the comparison runs in a child (tests/chain_fused_run.py): the context's
    first sample is an anchored window whose start is exact -- lo == H, no head blocks, nothing in front of the anchor -- and
    every contig, the first included, takes the fused launch."""
    n_contigs = 5
    out = tmp_path / "ahead_first.json"
    env = {k: v for k, v in os.environ.items() if k not in ("MSIM_NO_CHAIN_FUSE", "MSIM_NO_AHEAD", "MSIM_AHEAD", "MSIM_AHEAD_SIGMA")}
    env["MSIM_AHEAD_FIRST"] = "1"
    r = subprocess.run([sys.executable, str(Path(__file__).with_name("chain_fused_run.py")), str(out), str(n_contigs)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert res["verdict"] == "ok", res
    assert res["n_fused"] == n_contigs and res["snp_samples_ahead"] == n_contigs, res


def test_a_rebase_inside_the_pass(monkeypatch):
    monkeypatch.setenv("MSIM_DBG_JUMP_MAX_CHUNKS", "4")
    rs = np.random.RandomState(51)
    contigs = _genome(rs, 14, lo=1_000_000, hi=3_000_000, rate=(0.01, 0.02))
    st, n_fused = _three_ways(monkeypatch, contigs, _params(titv=2.0), (10, 11), gpu_flags=_ffi.PLAN_AUTO)
    assert st["stream_rebases"] >= 2 and n_fused == st["snp_samples_ahead"] >= 4


def test_contigs_that_stay_on_the_three_launches(monkeypatch):
    """A contig with two drawing ranges (its samples stay on the chain) and an SV-mix contig (another engine) between fused
    ones."""
    rs = np.random.RandomState(31)
    g = _big(rs, 8)
    contigs = g[:3] + [(2_500_000, [_snp_range(0, 999_999, 40_000), _snp_range(1_000_000, 2_499_999, 120_000, True)])] + g[3:5] + \
        [(2_000_000, [_sv_range(0, 1_999_999, 16_000, C3_CHANCES, C3_LENS)])] + g[5:8]
    st, n_fused = _three_ways(monkeypatch, contigs, _params(titv=2.0), (31, 32), gpu_flags=_ffi.PLAN_AUTO)
    assert st["contigs_svmix"] == 1 and n_fused == st["snp_samples_ahead"] and 4 <= n_fused <= 7


@pytest.mark.parametrize("fuse", [True, False])
def test_a_start_outside_its_interval_raises_either_way(monkeypatch, fuse):
    """MSIM_AHEAD_SIGMA=0: a 256-word interval, soon left.  The same error from the fused launch and from the three, and the
    context plans again after a reseed."""
    rs = np.random.RandomState(41)
    contigs = _genome(rs, 16, lo=2_000_000, hi=5_000_000)
    params = _params(titv=2.0)
    host = _run(_ffi.PLAN_HOST, contigs, params, (6, 7))[0]
    monkeypatch.setenv("MSIM_AHEAD_SIGMA", "0")
    if not fuse:
        monkeypatch.setenv("MSIM_NO_CHAIN_FUSE", "1")
    with pytest.raises(_ffi.MsimError, match="overflowed"):
        _run(_ffi.PLAN_GPU, contigs, params, (6, 7))
    eng = _ffi.Engine(0, _ffi.PLAN_GPU)
    try:
        eng.set_params(params)
        cids = [eng.add_contig_synthetic(L, 7) for L, _ in contigs]
        eng.seed(6, 7)
        with pytest.raises(_ffi.MsimError, match="overflowed"):
            eng.plan_pass([(cid, r, False) for cid, (_, r) in zip(cids, contigs)])
            eng.sync()
        assert (eng.chains_fused() > 0) == fuse
        eng.seed(6, 7)
        eng.plan_pass([(cid, r, False) for cid, (_, r) in zip(cids[:1], contigs[:1])])
        recs, pool = eng.fetch_records(cids[0])
        assert np.array_equal(recs.view(np.uint8), host[0][0].view(np.uint8)) and np.array_equal(pool, host[0][1])
    finally:
        eng.close()
