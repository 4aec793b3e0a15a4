"""The step boundary of the bit-compatible engine: host generators -> device streams (``streams_to_device``: one launch per
stream with the state in its arguments, one event) and the drain (the KeyError / length words copied before the pass's one
host wait).  Five contigs of 0.5-1 Mb at -sn 0.01 (k >= 4096: the SNP sampler takes them), planned and applied without a read
in between -- one emission group of four and one contig that the drain flushes -- and every case against the sequential host
planner (``_ffi.PLAN_HOST``) on the same contigs: records, checksums of the mutated contigs, both generators' final states."""
from __future__ import annotations

import random

import numpy as np
import pytest

import apply_ref
from mutation_simulator_amd import _ffi
from test_gpu_sampler import _params, _snp_range

pytestmark = pytest.mark.gpu

LENGTHS = [700_000, 1_000_000, 550_000, 850_000, 620_001]
A, B = (42, 42), (7, 1234)


def _next_words(mt, pos, n=8):
    r = random.Random()
    r.setstate((3, tuple(int(x) for x in mt) + (int(pos),), None))
    return [r.getrandbits(32) for _ in range(n)]


def _add(eng, last=None):
    cids = [eng.add_contig_synthetic(L, 1000 + i) for i, L in enumerate(LENGTHS[:-1])]
    cids.append(eng.add_contig_synthetic(LENGTHS[-1], 1004) if last is None else eng.add_contig(last))
    return cids


def _step(eng, cids, sync=True):
    """bench.one_step's order: plan + apply every contig, nothing read in between, one synchronisation."""
    for cid, L in zip(cids, LENGTHS):
        eng.plan_contig(cid, [_snp_range(0, L - 1, L // 100)])
        eng.apply_contig(cid)
    if sync:
        eng.sync()


def _read(eng, cids, checksums=None):
    out = {"recs": [eng.fetch_records(c)[0].copy() for c in cids],
           "sums": [eng.result_checksum(c) for c in (cids if checksums is None else cids[:checksums])],
           "next": [_next_words(*eng.get_mt_state(s)) for s in (0, 1)]}
    return out


def _same(got, want):
    assert len(got["recs"]) == len(want["recs"])
    for g, w in zip(got["recs"], want["recs"]):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8))
    assert got["sums"] == want["sums"]
    assert got["next"] == want["next"]


def _host(prepare, last=None, checksums=None):
    """The same step through the host planner: ``prepare(eng)`` seeds / sets the generators."""
    with _ffi.Engine(0, _ffi.PLAN_HOST) as eng:
        eng.set_params(_params(titv=2.0))
        cids = _add(eng, last)
        prepare(eng)
        try:
            _step(eng, cids)
            assert last is None
        except KeyError:                                  # (whichever call collects the last contig's APPLY)
            assert last is not None
        return _read(eng, cids, checksums)


@pytest.fixture(scope="module")
def host_a():
    return _host(lambda e: e.seed(*A))


@pytest.fixture(scope="module")
def host_b():
    return _host(lambda e: e.seed(*B))


@pytest.fixture()
def eng():
    with _ffi.Engine(0, _ffi.PLAN_GPU) as e:
        e.set_params(_params(titv=2.0))
        yield e


def test_seeds_a_b_a_in_one_context(eng, host_a, host_b):
    cids = _add(eng)
    got = []
    for seed in (A, B, A):
        eng.seed(*seed)
        _step(eng, cids)
        got.append(_read(eng, cids))
    _same(got[0], host_a)
    _same(got[1], host_b)
    _same(got[2], host_a)
    _same(got[2], got[0])
    st = eng.stats()
    assert st["contigs_snp"] == 15 and st["plan_host_ms"] == 0 and st["plan_gpu_ms"] > 0


def test_a_seed_nothing_was_planned_from_is_forgotten(eng, host_b):
    cids = _add(eng)
    eng.seed(*A)
    eng.seed(*B)
    _step(eng, cids)
    _same(_read(eng, cids), host_b)


def test_numpy_state_right_after_seed(eng):
    eng.seed(*B)
    mt, pos = eng.get_mt_state(1)
    st = np.random.RandomState(B[1]).get_state()
    assert pos == int(st[2]) == 624 and np.array_equal(mt, np.asarray(st[1], dtype=np.uint32))
    mt0, pos0 = eng.get_mt_state(0)
    r = random.Random(B[0])
    assert _next_words(mt0, pos0) == [r.getrandbits(32) for _ in range(8)]


def _state_at(stream, index):
    """(mt, pos) of a generator whose state index is ``index``: 624 = freshly seeded, else that many outputs into its first block."""
    skip = 0 if index == 624 else index
    if stream == 0:
        r = random.Random(99)
        for _ in range(skip):
            r.getrandbits(32)
        st = r.getstate()[1]
        return np.array(st[:624], dtype=np.uint32), int(st[624])
    rs = np.random.RandomState(98)
    if skip:
        rs.bytes(4 * skip)
    st = rs.get_state()
    return np.asarray(st[1], dtype=np.uint32).copy(), int(st[2])


@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("index", [1, 623, 624])
def test_set_mt_state_then_a_step(eng, stream, index):
    mt, pos = _state_at(stream, index)
    assert pos == index

    def prepare(e):
        e.seed(*A)
        e.set_mt_state(stream, mt, pos)
    cids = _add(eng)
    prepare(eng)
    _step(eng, cids)
    _same(_read(eng, cids), _host(prepare))


def test_a_rebase_inside_the_pass(monkeypatch, host_a):
    """A two-chunk jump-table span: the session ends inside the pass, the exact positions go to the host generators and come
    back as a new session's origin -- through the same routine as a reseed."""
    monkeypatch.setenv("MSIM_DBG_JUMP_MAX_CHUNKS", "2")
    with _ffi.Engine(0, _ffi.PLAN_GPU) as e:
        e.set_params(_params(titv=2.0))
        cids = _add(e)
        e.seed(*A)
        _step(e, cids)
        _same(_read(e, cids), host_a)
        st = e.stats()
        assert st["stream_rebases"] >= 1 and st["contigs_snp"] == 5, st["stream_rebases"]


def test_key_error_in_the_last_contig_is_reported_by_the_first_sync(eng, host_a):
    """The last contig -- the one the drain flushes -- holds a stretch of 'X': its first transversion there is a KeyError, which
    the synchronisation behind the pass reports; the other contigs' results are right, and a clean step after it reports none."""
    rng = np.random.default_rng(5)
    last = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, LENGTHS[-1])].copy()
    last[200_000:400_000] = ord("X")
    cids = _add(eng, last)
    eng.seed(*A)
    _step(eng, cids, sync=False)
    with pytest.raises(KeyError) as ei:
        eng.sync()
    recs, pool = eng.fetch_records(cids[-1])
    want = apply_ref.apply(last, recs, pool)
    assert want.key_error is not None and want.key_error[0] == "X" and 200_000 <= want.key_error[1] < 400_000
    assert ei.value.args[0] == "X"
    assert eng.key_error(cids[-1]) == want.key_error
    assert [eng.key_error(c) for c in cids[:-1]] == [None] * 4
    got = _read(eng, cids, checksums=4)
    _same(got, _host(lambda e: e.seed(*A), last, checksums=4))
    # the records do not depend on the bases: the same plan as the clean genome's
    for g, w in zip(got["recs"], host_a["recs"]):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    # a clean step in the same context
    eng.clear()
    cids = _add(eng)
    eng.seed(*A)
    _step(eng, cids)
    assert [eng.key_error(c) for c in cids] == [None] * 5
    _same(_read(eng, cids), host_a)
