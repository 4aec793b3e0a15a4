"""One steered fixture case (tests/golden/steered_seeds.json) through the production engine, compared with the word-level
restatement ``stream_ref`` alone: records byte for byte, ``plan_was_empty``, both word counts, the final states of both
generators; optionally through APPLY against ``apply_ref``.  Used in-process by tests/test_gpu_steered.py and, run as a
script, in a fresh process for the policies libmsim reads ONCE per process (``MSIM_NO_SCAN_FOLD``, ``MSIM_NO_AUX_FOLD``,
``MSIM_DBG_AHEAD_LOG`` are function-local statics):

    python tests/steered_run.py RESULT.json [--ahead-log] [case names ...]

writes {case name: "ok" | what differed} and stops at the first library error (nothing runs on a device after a fault)."""
from __future__ import annotations

import json
import os
import re
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "mutation-simulator_amd", ROOT / "tests", ROOT / "tests" / "golden"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import numpy as np  # noqa: E402

import apply_ref  # noqa: E402
import stream_ref as sr  # noqa: E402
from mutation_simulator_amd import _ffi  # noqa: E402
from mutation_simulator_amd import mutator as mm  # noqa: E402

# cases whose event needs more draws than the 60 000 the others keep to: the chunk hand-over (160 000 words in one sample) and
# two bin-border values each drawn twice (probability ~ (draws / n)**4 / 4 per seed)
K_CAP_LIFTED = {"sample_ends_at_chunk_border_minus_1", "sample_ends_at_chunk_border_exact", "sample_ends_at_chunk_border_plus_1",
                "bin_border_values_with_duplicates"}


def params(d, titv):
    class S:
        pass
    from mutation_simulator_amd.mut_types import MutType
    S.mut_block = {t: d for t in MutType}
    S.titv = titv
    return mm.params_descriptor(S)


def snp_range(start, stop, k):
    """ARGS-mode type order with p(SN) = 1: the type draw is deterministic (two NumPy words per candidate all the same)."""
    r = _ffi.Range()
    r.start, r.stop, r.k = start, stop, k
    r.setsize = mm.sample_setsize(k)
    r.n_types = 7
    for j, t in enumerate([1, 2, 3, 5, 4, 6, 7]):
        r.types[j] = t
        r.cdf_thr[j] = 1 << 53
    for t in (2, 3, 4, 6):
        r.min_len[t], r.max_len[t] = 1, 2
    r.min_len[5], r.max_len[5] = 2, 3
    return r


def random_bases(L, seed):
    return np.frombuffer(b"AGTC", dtype=np.uint8)[np.random.RandomState(seed).randint(0, 4, size=L)]


def run_case(case, planned, apply=False):
    """Plans every contig of the case first, THEN reads (the second contig's sample is then anchored ahead of the chain under
    the default policy).  Returns the context's stats."""
    words, p, mt, plans = planned
    K = sum(len(cp.recs) for cp in plans)
    np_mt, np_pos, np_next = sr.numpy_stream(case["seed"][1], 2 * K)
    eng = _ffi.Engine(0, _ffi.PLAN_GPU)
    try:
        eng.set_mt_state(0, mt, p)
        eng.set_mt_state(1, np_mt, np_pos)
        eng.set_params(params(case["d"], case["titv"]))
        cids, bases = [], []
        for i, c in enumerate(case["contigs"]):
            if apply:
                bases.append(random_bases(c["L"], 11 + i))
                cid = eng.add_contig(bases[-1])
            else:
                cid = eng.add_contig_synthetic(c["L"], 7)
            eng.plan_contig(cid, [snp_range(*r) for r in c["ranges"]])
            if apply:
                eng.apply_contig(cid)
            cids.append(cid)
        for i, (cid, cp) in enumerate(zip(cids, plans)):
            recs, pool = eng.fetch_records(cid)
            assert recs.shape == cp.recs.shape and len(pool) == 0
            if recs.tobytes() != cp.recs.tobytes():
                bad = np.flatnonzero((recs["pos"] != cp.recs["pos"]) | (recs["aux"] != cp.recs["aux"]) | (recs["stop"] != cp.recs["stop"]) | (recs["type"] != cp.recs["type"]))
                raise AssertionError(f"contig {i}: {len(bad)} of {len(recs)} records differ, first at {bad[:3].tolist()}: "
                                     f"{recs[bad[:3]].tolist()} != {cp.recs[bad[:3]].tolist()}")
            assert not eng.plan_was_empty(cid)
            if apply:
                want = apply_ref.apply(bases[i], cp.recs, np.zeros(0, dtype=np.uint8))
                got = eng.fetch_sequence(cid)
                assert want.key_error is None and len(got) == want.out_len
                assert np.array_equal(got, want.seq), f"contig {i}: mutated sequence differs at {np.flatnonzero(got != want.seq)[:5].tolist()}"
        st = eng.stats()
        assert st["py_words"] == plans[-1].end - p, ("py_words", st["py_words"], plans[-1].end - p)
        assert st["np_words"] == 2 * K
        assert sr.next_words(*eng.get_mt_state(0)) == words[plans[-1].end:plans[-1].end + 8].tolist(), "CPython stream position"
        assert sr.next_words(*eng.get_mt_state(1)) == np_next, "NumPy stream position"
        assert st["plan_gpu_ms"] > 0 and st["plan_host_ms"] == 0 and st["contigs_snp"] == len(case["contigs"])
        return st
    finally:
        eng.close()


AHEAD_LINE = re.compile(r"sample ahead of the chain: K (\d+), start in \[(\d+), (\d+)\], core (\d+) draws")


def check_head_interval(case, planned, log_text):
    """Cases 18 / 19: the steered draws lie where the event wants them relative to the window the engine REALLY anchored (its
    own log line): the head interval [lo, H) in front of the anchor, the core's first k_core accepted draws behind it."""
    words, p, mt, plans = planned
    ci, ri = case["target"]
    k = case["contigs"][ci]["ranges"][ri][2]
    lines = [tuple(int(x) for x in m.groups()) for m in AHEAD_LINE.finditer(log_text)]
    mine = [l for l in lines if l[0] == k]
    assert len(mine) == 1, f"no anchored window for the steered sample in the log: {lines}"
    _, lo, H, core = mine[0]
    a, b = case["event"]["words"]
    sp = plans[ci].samples[ri]
    assert lo <= sp.cut[0] <= H
    assert lo <= a < H, f"word {a} outside the head interval [{lo}, {H})"
    if case["event"]["kind"] == "head_duplicate_pair":
        assert lo <= b < H, f"word {b} outside the head interval [{lo}, {H})"
    else:
        behind = sum(1 for w in sp.acc_idx if H <= w <= b)           # accepted draws of [H, b]: inside the core's first k_core
        assert b >= H and behind <= core, (b, H, behind, core)


def main(argv):
    out = Path(argv[0])
    args = argv[1:]
    ahead_log = "--ahead-log" in args
    names = [a for a in args if not a.startswith("--")]
    results = {}
    for case in sr.load_cases():
        if names and case["name"] not in names:
            continue
        planned = sr.plan_case(case)
        try:
            if ahead_log:
                sys.stderr.flush()
                with tempfile.TemporaryFile() as tf:
                    saved = os.dup(2)
                    os.dup2(tf.fileno(), 2)
                    try:
                        run_case(case, planned)
                    finally:
                        os.dup2(saved, 2)
                        os.close(saved)
                    tf.seek(0)
                    check_head_interval(case, planned, tf.read().decode("utf-8", "replace"))
            else:
                run_case(case, planned)
            results[case["name"]] = "ok"
        except AssertionError as e:
            results[case["name"]] = f"AssertionError: {e}"
        except _ffi.MsimError as e:                                   # a library error: nothing more runs on the device
            results[case["name"]] = f"MsimError: {e}"
            break
        finally:
            out.write_text(json.dumps(results))
    out.write_text(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
