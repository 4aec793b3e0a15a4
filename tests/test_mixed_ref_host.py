"""tests/mixed_ref.py -- the plain references the GPU tiers test_gpu_mixed_tables.py / test_gpu_accept_tables.py compare the
device kernels with -- tied, on the CPU tier, to what is already pinned: CPython's and NumPy's own generators, the host's accept
tables (plan_host.cpp: accept_tables_host, which the host walk is tested on) and the host planner's record table
(msim_plan_contig on a host-only context; held against the reference's goldens and the oracle elsewhere).

Translocations are not part of the planner tie: linking draws (``__fix_tl_amount``, ``shuffle``, the coin) are not restated
here, so ``boundary_and_emit``'s linking step is exercised on hand-built decisions only (test_gpu_mixed_tables.py)."""
from __future__ import annotations

import random

import numpy as np
import pytest

import mixed_ref as R
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import mutator as mm
from test_multimix_host import _engine, _range


# ---------------------------------------------------------------------- tempering
def test_untemper_inverts_temper():
    x = np.random.RandomState(3).bytes(4 * 100_000)
    x = np.frombuffer(x, dtype="<u4")
    edge = np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0x9D2C5680, 0xEFC60000], dtype=np.uint32)
    for a in (x, edge):
        assert np.array_equal(R.untemper(R.temper(a)), a)
        assert np.array_equal(R.temper(R.untemper(a)), a)
    assert R.untemper(R.temper(0xDEADBEEF)) == 0xDEADBEEF


def test_temper_is_mt19937s():
    """The state words NumPy holds are the raw ones: tempering the first n of a freshly twisted state gives the n outputs."""
    rs = np.random.RandomState(7)
    out = np.frombuffer(rs.bytes(4 * 600), dtype="<u4")
    _, key, pos = rs.get_state()[:3]
    assert pos == 600
    assert np.array_equal(R.temper(key[:600]), out)
    py = random.Random(11)
    out = [py.getrandbits(32) for _ in range(100)]
    st = py.getstate()[1]
    assert st[624] == 100 and [R.temper(w) for w in st[:100]] == out


# ---------------------------------------------------------------------- types
@pytest.mark.parametrize("chances", [[0.5, 0.5], [0.9, 0.02, 0.02, 0.02, 0.04], [0.3, 0.0, 0.7], [1.0], [0.125] * 8])
def test_types_of_is_numpy_choice(chances):
    k = 5000
    keys = list(range(1, len(chances) + 1))
    rs = np.random.RandomState(5)
    want = rs.choice(keys, p=chances, size=k)                              # mutator.py:170-174
    words = np.frombuffer(np.random.RandomState(5).bytes(8 * k), dtype="<u4")
    cdf = np.cumsum(np.array(chances, dtype=np.float64))
    cdf /= cdf[-1]
    thr = [mm._ceil_scaled(float(c)) for c in cdf]
    assert np.array_equal(R.types_of(words, thr, keys), want)


# ---------------------------------------------------------------------- accept tables
WIDTH_SETS = [[1], [50, 451], [2, 3, 4], [(1 << 24) - 1, 5, 17, 1 << 10], [(1 << 23) - 1, 9, 33, 65, 129],
              [1, 2, 3, 4, 5, (1 << 23) - 1, (1 << 12) + 1, 1 << 22]]


@pytest.mark.parametrize("widths", WIDTH_SETS, ids=lambda w: f"{len(w)}cls")
def test_accept_table_is_the_hosts_on_random_words(widths):
    classes = [R.class_of(w) for w in widths]
    for n in (0, 1, 62, 63, 64, 300):
        words = np.frombuffer(np.random.RandomState(n + len(widths)).bytes(4 * n), dtype="<u4")
        assert np.array_equal(R.accept_table(words, classes), _ffi.accept_tables_host(words, classes))


@pytest.mark.parametrize("n_rejected", [0, 61, 62, 63, 64])
@pytest.mark.parametrize("widths", [[3], [5, 3], [3, 1 << 20, 9, 2, 6]], ids=lambda w: f"{len(w)}cls")
def test_accept_table_is_the_hosts_on_long_rejection_runs(widths, n_rejected):
    classes = [R.class_of(w) for w in widths]
    words = R.rejection_run(n_rejected)
    T = R.accept_table(words, classes)
    assert np.array_equal(T, _ffi.accept_tables_host(words, classes))
    lg, vbits = R.lg_rows_of(len(widths)), 24 if len(widths) <= 4 else 23
    k3 = widths.index(3)
    # 62 rejections: the 63rd word is still in reach; 63 and more: the entry at the run's start is "none"
    assert T[0, k3] == ((((n_rejected + 1) << lg) << vbits) if n_rejected <= 62 else 0)
    assert T[len(words), k3] == 0                                          # the end-of-window sentinel
    cut = words[:n_rejected]                                               # the window ends one word before the accept
    assert not R.accept_table(cut, classes)[:, k3].any()
    assert np.array_equal(R.accept_table(cut, classes), _ffi.accept_tables_host(cut, classes))


def test_accept_tables_host_refuses_what_chain_classes_cannot_make():
    w = np.zeros(4, dtype=np.uint32)
    for bad in ([], [(31, 1)] * 9, [(30, 1)], [(8, 1 << 24)], [(9, (1 << 23))] + [(31, 1)] * 4, [(32, 0)]):
        with pytest.raises(_ffi.MsimError) as e:
            _ffi.accept_tables_host(w, bad)
        assert e.value.code == _ffi.ERR_ARG


# ---------------------------------------------------------------------- the planner tie
def _sample_with_minimum_distance(py, start, stop, k, d):
    """util.py:104-109, on the caller's generator."""
    sampl = py.sample(range(start, stop - (k - 1) * d), k)
    indices = sorted(range(len(sampl)), key=lambda i: sampl[i])
    return sorted([s + d * r for s, r in zip(sampl, sorted(indices, key=lambda i: indices[i]))])


def _reference_run(L, specs, blocks, seed):
    """The reference's order of draws -- per range sample -> choice -> boundary pass (mutator.py:116-123, 144-214) -- with
    CPython's ``random.Random`` and NumPy's ``RandomState`` themselves; the boundary pass is ``boundary_and_emit``'s, which asks
    for a length exactly where __get_stop_position calls randint.  Returns (its result, the literal insert pool)."""
    py, rs = random.Random(seed[0]), np.random.RandomState(seed[1])
    block = {t: 1 for t in range(1, 8)}
    block.update(blocks or {})
    d = min(block.values())                                                # mutator.py:161

    def lengths_of(lens):
        def draw(t, p):
            lo, hi = lens[t]
            if t == R.IV and p + hi >= L - 1:                              # mutator.py:243-244
                return None
            return py.randint(p + lo - 1, p + hi - 1) - p + 1              # :246-262
        return draw

    scratch = np.zeros(1 << 16, dtype=np.uint32)
    out_ranges = []
    for start, stop, rate, chances, lens in specs:
        k = int(((stop - start) + 1) * rate)                               # mutator.py:225
        pos = _sample_with_minimum_distance(py, start, stop, k, d)
        keys = list(chances)
        types = rs.choice(keys, p=[chances[t] for t in keys], size=len(pos))      # mutator.py:170-174
        # the boundary pass of THIS range draws before the next range samples: run it now, on its own, to advance `py`
        drawn = {}
        draw = lengths_of(lens)

        def remember(t, p, draw=draw, drawn=drawn):
            drawn[p] = draw(t, p)
            return drawn[p]
        R.boundary_and_emit(L, block, [{"clip": stop + 1, "pos": pos, "type": types, "length": remember}], scratch)
        out_ranges.append({"clip": stop + 1, "pos": pos, "type": types, "length": (lambda t, p, drawn=drawn: drawn[p])})
    n_words = 1 << 16
    st = rs.get_state()
    words = np.frombuffer(rs.bytes(4 * n_words), dtype="<u4")
    res = R.boundary_and_emit(L, block, out_ranges, words, sn_chained=block[1] != d)
    rs.set_state(st)
    literal = []
    for rec in res["recs"]:
        if rec["type"] == R.IN:
            literal.append("".join(rs.choice(["A", "T", "G", "C"], int(rec["stop"]) + 1 - int(rec["pos"]))))   # mutator.py:471
    return res, np.frombuffer("".join(literal).encode(), dtype=np.uint8)


def _host_plan(L, specs, blocks, seed):
    order = lambda chances: list(chances)
    ranges = [_range(s, e, rate, chances, lens, order(chances)) for s, e, rate, chances, lens in specs]
    eng = _engine(blocks, 1.0, seed)
    cid = eng.add_contig(np.zeros(L, dtype=np.uint8))
    eng.plan_contig(cid, ranges)
    recs, pool = eng.fetch_records(cid)
    eng.close()
    # the mutated length as the liftover chain of this table states it (qSize of the header; msim_render_chain, test_chain_host.py)
    header = _ffi.render_chain(recs, L, "t", "q", 1).split(b"\n", 1)[0].split()
    assert header[0] == b"chain" and int(header[3]) == L
    out_len = int(header[8])
    return recs, pool, out_len


MIX = {1: 0.6, 2: 0.1, 3: 0.1, 4: 0.1, 5: 0.1}
LENS = {2: (1, 50), 3: (1, 60), 4: (5, 70), 5: (2, 40), 6: (1, 1)}
SHAPES = {
    "one_range_sv_mix": (200_000, [(0, 199_999, 0.02, MIX, LENS)], None),
    # three ranges with their own settings; the long deletions / duplications of the first two reach across their range's end
    "three_ranges_spans_cross": (60_000, [(0, 19_999, 0.02, {1: 0.3, 3: 0.5, 4: 0.2}, {3: (200, 900), 4: (100, 800)}),
                                         (20_000, 20_399, 0.05, {1: 0.5, 3: 0.5}, {3: (300, 2000)}),
                                         (20_400, 59_999, 0.02, MIX, LENS)], None),
    "sn_block_3": (120_000, [(0, 59_999, 0.03, MIX, LENS), (60_000, 119_999, 0.02, {1: 0.8, 2: 0.2}, LENS)], {1: 3}),
}


@pytest.mark.parametrize("seed", [(1, 2), (3, 4)])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_boundary_and_emit_reproduces_the_host_planner(shape, seed):
    L, specs, blocks = SHAPES[shape]
    res, literal_pool = _reference_run(L, specs, blocks, seed)
    recs, pool, out_len = _host_plan(L, specs, blocks, seed)
    assert res["n_rec"] == len(recs) > 100
    for f in ("pos", "stop", "type", "extra"):
        assert np.array_equal(res["recs"][f], recs[f]), f
    sv = recs["type"] != R.SN                                              # (an SNP's aux is its transition / transversion draw: another stage)
    assert np.array_equal(res["recs"]["aux"][sv], recs["aux"][sv])
    assert np.array_equal(res["pool"], pool) and np.array_equal(literal_pool, pool)
    assert L + res["len_delta"] == out_len
    assert len(set(recs["type"].tolist())) >= 2
    if shape == "three_ranges_spans_cross":
        assert res["visit_from"][1:].max() > 0, "no span crossed a range border: the shape lost its point"
        skipped = [j for j in range(len(res["cand_pos"])) if res["cand_pos"][j] < res["visit_from"][np.searchsorted(
            [b for b, _ in res["rt"]], j, side="right") - 1]]
        assert skipped, "no candidate inside an earlier range's span"
