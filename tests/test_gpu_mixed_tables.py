"""The device half of the SV-mix and host-chain PLAN engines (plan_kernels.h section 6) on hand-built tables, kernel group by
kernel group, through the engines' own launch helpers (``Engine.candidates``: msim_dbg_candidates; ``Engine.mixed_emit``:
msim_dbg_mixed_emit).  Compared byte for byte with tests/mixed_ref.py, which test_mixed_ref_host.py ties to CPython, NumPy and
the host planner.

  candidate front   k_bitmap_count, k_scan_u32, k_bitmap_expand_cand | k_types_multi; k_nsn_count, k_scan_u32, k_nsn_scatter
  keep -> records   k_stop_scatter, k_link_scatter, k_blk_reduce, k_scan_max_u32, k_keep_flags, k_scan4, k_emit_records, k_pool_fill

The inputs sit where genuine MT19937 streams never put them: a type threshold hit exactly, range borders inside one thread's 8
candidates and on workgroup borders (2048 candidates), blocked ends on / around the next candidate, beyond their range's clip,
saturating at 2^32, carried across more than 1024 workgroups; tombstoned translocations on block edges."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

import mixed_ref as R
from mixed_ref import DE, DU, IN, IV, SN, TL, TLI
from mutation_simulator_amd import _ffi
from test_gpu_emit_train_bitmaps import ONES, _random, _with_bits, _zeros

pytestmark = pytest.mark.gpu

CB = 2048                                                  # candidates per workgroup (CB_BLOCK), 8 per thread
TWO53 = 1 << 53
BLOCK = {SN: 1, IN: 5, DE: 7, DU: 3, IV: 2, TL: 4, TLI: 6}


@pytest.fixture(scope="module")
def eng():
    with _ffi.Engine(0) as e:
        yield e


@contextlib.contextmanager
def refused(check: str):
    """The call must come back with MSIM_ERR_ARG -- every such return of the hooks lies in front of their first allocation and
    launch -- and with the message of the host check that is meant to stop it."""
    with pytest.raises(_ffi.MsimError) as e:
        yield
    assert e.value.code == _ffi.ERR_ARG, str(e.value)
    assert check in str(e.value), str(e.value)


def _params(eng, block):
    p = _ffi.Params()
    for i in range(8):
        p.block[i] = 1
    for t, v in block.items():
        p.block[t] = v
    p.ti_lim = TWO53 // 2
    eng.set_params(p)


def _np_words(n, seed=9):
    return np.frombuffer(np.random.RandomState(seed).bytes(4 * max(n, 1)), dtype="<u4")


# ====================================================================== candidate front
def _type_table(thr, types):
    tt = np.zeros(1, dtype=_ffi.TYPE_TABLE_DTYPE)
    tt["n"] = len(thr)
    tt["thr"][0, :len(thr)] = thr
    tt["type"][0, :len(thr)] = types
    return tt


# eight entries: a type with no chance (two equal thresholds), the last threshold 2^53 (cdf[-1] == 1.0)
THR8 = [1 << 50, 1 << 51, 3 << 50, 3 << 50, 1 << 52, 5 << 50, 7 << 50, TWO53]
TYPES8 = [SN, IN, DE, DU, IV, TL, TLI, SN]
TABLES = {
    "n8": (THR8, TYPES8),
    "n1_sv": ([TWO53], [DE]),                              # only non-SNPs
    "n1_sn": ([TWO53], [SN]),                              # no non-SNP at all
    "n2": ([TWO53 - 1, TWO53], [SN, IN]),                  # the last type is drawn by m = 2^53 - 1 alone
}


def _m_values(k, thr, seed):
    """53-bit samples for k candidates: thr - 1, thr, thr + 1 of every threshold first (where below 2^53), the rest random."""
    rs = np.random.RandomState(seed)
    m = (rs.randint(0, 1 << 26, size=k).astype(np.uint64) << np.uint64(27)) | rs.randint(0, 1 << 27, size=k).astype(np.uint64)
    exact = [x for t in thr for x in (t - 1, t, t + 1) if 0 <= x < TWO53] + [0, TWO53 - 1]
    m[:min(k, len(exact))] = exact[:k]
    return m


def _bitmap_with(k, words, seed):
    bits = np.sort(np.random.RandomState(seed).choice(words * 64, size=k, replace=False))
    return _with_bits(words, bits.tolist())


BITMAPS = {
    "w255": lambda: _random(255, 0.2, 1), "w256": lambda: _random(256, 0.2, 2), "w257": lambda: _random(257, 0.2, 3),
    "empty": lambda: _zeros(3), "one_bit": lambda: _with_bits(257, [256 * 64 + 63]),
    "ones": lambda: np.concatenate([_zeros(2), np.full(40, ONES, dtype=np.uint64), _random(3, 0.5, 4)]),
    "k2047": lambda: _bitmap_with(2047, 300, 5), "k2048": lambda: _bitmap_with(2048, 300, 6), "k2049": lambda: _bitmap_with(2049, 300, 7),
    "k4095": lambda: _bitmap_with(4095, 257, 8), "k4096": lambda: _bitmap_with(4096, 257, 9), "k4097": lambda: _bitmap_with(4097, 257, 10),
}


def _check_front(got, pos, types, all_):
    npos, ntype, nrank = R.compaction(pos, types, all_)
    assert np.array_equal(got["cand_type"], types)
    if pos is not None:
        assert np.array_equal(got["cand_pos"], pos) and np.array_equal(got["nsn_pos"], npos)
    assert got["n_nsn"] == len(nrank)
    assert np.array_equal(got["nsn_type"], ntype) and np.array_equal(got["nsn_rank"], nrank)


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", sorted(BITMAPS))
def test_one_range_front(eng, name, table):
    """("empty": the engines never plan a range without candidates and a grid of no workgroups cannot be launched, so the hook
    returns an empty result without a launch -- those four cases hold the hook to that, they run no kernel.)"""
    bm = BITMAPS[name]()
    thr, types = TABLES[table]
    k = int(np.unpackbits(bm.view(np.uint8)).sum())
    start, d = 1000, 3
    words = R.words_of_m(_m_values(k, thr, k + 1), seed=k)
    got = eng.candidates(R.untemper(words), _type_table(thr, types), bitmap=bm, start=start, d=d)
    _check_front(got, R.positions_of(bm, start, d), R.types_of(words, thr, types), False)


def test_thresholds_hit_exactly(eng):
    """m == thr - 1, thr, thr + 1 for each of eight thresholds: `thr <= m` decides, so thr itself belongs to the NEXT type."""
    k = 64
    m = _m_values(k, THR8, 0)
    words = R.words_of_m(m, seed=1)
    want = R.types_of(words, THR8, TYPES8)
    assert want[0] == SN and want[1] == IN and want[2] == IN             # 2^50 - 1 | 2^50 | 2^50 + 1
    assert want[7] == IV and DU not in want[:24]                          # 3 * 2^50 skips the type with no chance
    got = eng.candidates(R.untemper(words), _type_table(THR8, TYPES8), bitmap=_with_bits(4, range(0, 4 * 64, 4)), start=0, d=1)
    assert np.array_equal(got["cand_type"], want)


def test_single_non_snp_as_last_candidate_of_a_block(eng):
    k = CB + 5
    m = np.zeros(k, dtype=np.uint64)                                     # all SN ...
    m[CB - 1] = TWO53 - 1                                                # ... but the last candidate of workgroup 0
    words = R.words_of_m(m, seed=2)
    bm = _bitmap_with(k, 64, 11)
    got = eng.candidates(R.untemper(words), _type_table(*TABLES["n2"]), bitmap=bm, start=7, d=1)
    _check_front(got, R.positions_of(bm, 7, 1), R.types_of(words, *TABLES["n2"]), False)
    assert got["n_nsn"] == 1 and got["nsn_rank"][0] == CB - 1


def _mix_ranges(bases, n_sets=2):
    rt = np.zeros(len(bases), dtype=_ffi.MIX_RANGE_DTYPE)
    rt["rec_base"] = bases
    rt["clip"] = 0
    rt["set_id"] = np.arange(len(bases)) % n_sets                        # two sets alternating
    return rt


SETS2 = [(THR8, TYPES8), ([1 << 52, TWO53], [IV, SN])]
RANGE_SHAPES = {
    "one_each_20": (20, list(range(20))),                                # eight ranges inside one thread's items
    "one": (4100, [0]),
    "two": (4100, [0, 2049]),
    "on_8t_and_2048b": (4100, [0, 8, 16, 24, 2040, 2048, 2056, 4096]),
    "off_by_one": (4100, [0, 7, 9, 2047, 2049, 4095, 4097]),
    "r5000_one_each": (5000, list(range(5000))),
    "r5000_of_9000": (9000, None),
}


@pytest.mark.parametrize("all_", [False, True])
@pytest.mark.parametrize("shape", sorted(RANGE_SHAPES))
def test_types_by_ordinal_over_many_ranges(eng, shape, all_):
    K, bases = RANGE_SHAPES[shape]
    if bases is None:
        bases = [0] + np.sort(np.random.RandomState(3).choice(np.arange(1, K), size=4999, replace=False)).tolist()
    rt = _mix_ranges(bases)
    sets = np.concatenate([_type_table(*s) for s in SETS2])
    words = R.words_of_m(_m_values(K, THR8, K), seed=K)
    want = np.empty(K, dtype=np.uint8)
    for r, a in enumerate(bases):
        b = bases[r + 1] if r + 1 < len(bases) else K
        thr, types = SETS2[r % 2]
        want[a:b] = R.types_of(words[2 * a:2 * b], thr, types)
    got = eng.candidates(R.untemper(words), sets, K=K, ranges=rt, all=all_)
    assert got["cand_pos"] is None
    _check_front(got, None, want, all_)


def test_the_candidate_hook_refuses_what_the_planners_cannot_produce(eng):
    words = np.zeros(64, dtype=np.uint32)
    bm = _with_bits(1, [3, 9])
    good = _type_table(THR8, TYPES8)
    eng.candidates(words, good, bitmap=bm)
    none, nine = _type_table([TWO53], [SN]), _type_table([TWO53], [SN])
    none["n"], nine["n"] = 0, 9
    for tt in (_type_table([5, 4], [SN, IN]), _type_table([TWO53], [0]), _type_table([TWO53], [8]), none, nine):
        with refused("type table outside 1..8 types"):
            eng.candidates(words, tt, bitmap=bm)
    with refused("fewer than two words each"):
        eng.candidates(words[:3], good, bitmap=bm)
    with refused("positions beyond 2^32"):
        eng.candidates(words, good, bitmap=bm, start=(1 << 32) - 64)
    with refused("a range table starts at candidate 0"):
        eng.candidates(words, good, K=8, ranges=_mix_ranges([1, 2], 1))
    for bases in ([0, 2, 2], [0, 3, 2], [0, 9]):
        with refused("rec_base not strictly increasing below K"):
            eng.candidates(words, good, K=8, ranges=_mix_ranges(bases, 1))
    with refused("set_id out of range"):
        eng.candidates(words, good, K=8, ranges=_mix_ranges([0, 4], 2))                     # set_id 1 of one set
    with refused("msim_dbg_candidates: bad argument"):
        eng.candidates(words, np.concatenate([good] * 9), K=8, ranges=_mix_ranges([0, 1], 1))


# ====================================================================== keep flags through records
def _emit(eng, L, ref, np_words):
    rt = None
    if len(ref["rt"]) > 1 or ref.get("force_rt"):
        rt = np.zeros(len(ref["rt"]), dtype=_ffi.MIX_RANGE_DTYPE)
        rt["rec_base"] = [a for a, _ in ref["rt"]]
        rt["clip"] = [c for _, c in ref["rt"]]
    return eng.mixed_emit(L, ref["cand_pos"], ref["cand_type"], ref["ch_rank"], ref["ch_stop"], R.untemper(np_words),
                          ch_extra=ref["ch_extra"], ch_aux=ref["ch_aux"], ranges=rt,
                          visit_from=ref["visit_from"] if rt is not None else None, sn_chained=ref["sn_chained"])


def _same(got, ref):
    for f in ("n_rec", "n_sn", "pool_len", "len_delta"):
        assert got[f] == ref[f], f
    for f in ("pos", "stop", "extra", "type", "aux", "rsv"):
        assert np.array_equal(got["recs"][f], ref["recs"][f]), f
    assert got["recs"].tobytes() == ref["recs"].tobytes()
    assert np.array_equal(got["rec_off"], ref["rec_off"])
    assert np.array_equal(got["sn_index"], ref["sn_index"])
    assert np.array_equal(got["pool"], ref["pool"])


def _run(eng, L, block, ranges, sn_chained=False, link=None, seed=9):
    """One range goes both ways: without a range table (the SV-mix engine) and as a table of one range (host-chain, n_draw = 1)."""
    _params(eng, block)
    words = _np_words(1 << 16, seed)
    ref = R.boundary_and_emit(L, block, ranges, words, sn_chained=sn_chained, link=link)
    for force_rt in ((False, True) if len(ranges) == 1 else (False,)):
        ref["force_rt"] = force_rt
        _same(_emit(eng, L, ref, words), ref)
    return ref


def _random_link(seed):
    def link(tls, tlis):
        rs = np.random.RandomState(seed)
        longer = tls if len(tls) > len(tlis) else tlis
        drop = [longer[i] for i in rs.choice(len(longer), size=abs(len(tls) - len(tlis)), replace=False)]
        tls = [p for p in tls if p not in drop]
        tlis = [p for p in tlis if p not in drop]
        rs.shuffle(tls)
        return {"tombstones": drop, "pairs": [(a, b, int(rs.randint(0, 2))) for a, b in zip(tls, tlis)]}
    return link


def _random_ranges(k, borders, seed, L, p_types, max_len=40, step=2):
    """k candidates at distinct multiples of ``step`` (an SNP with block 1 never blocks its successor), types drawn with
    ``p_types``, lengths 1..max_len; ``borders``: the first ordinal of every range but the first."""
    rs = np.random.RandomState(seed)
    pos = np.sort(rs.choice(np.arange(1, L // step - 1), size=k, replace=False)) * step
    types = rs.choice(list(p_types), p=list(p_types.values()), size=k)
    lens = rs.randint(1, max_len + 1, size=k).tolist()
    # (an inversion that does not fit is no mutation, mutator.py:243-244: those that would pass the contig's end, and some others)
    lens = [None if (t == IV and (rs.randint(0, 8) == 0 or p + n >= L - 1)) else n for t, n, p in zip(types.tolist(), lens, pos.tolist())]
    cuts = [0] + list(borders) + [k]
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        clip = int(pos[b]) if b < k else L                               # the next range starts where this one's clip is
        out.append({"clip": clip, "pos": pos[a:b].tolist(), "type": types[a:b].tolist(), "length": lens[a:b]})
    return out


P_ALL = {SN: 0.5, IN: 0.1, DE: 0.1, DU: 0.08, IV: 0.08, TL: 0.08, TLI: 0.06}
P_NO_TL = {SN: 0.6, IN: 0.1, DE: 0.1, DU: 0.1, IV: 0.1}


@pytest.mark.parametrize("k", [2047, 2048, 2049, 4095, 4096, 4097])
@pytest.mark.parametrize("with_tl", [False, True])
def test_one_range_every_type(eng, k, with_tl):
    L = 40 * k
    ranges = _random_ranges(k, [], k, L, P_ALL if with_tl else P_NO_TL)
    ref = _run(eng, L, BLOCK, ranges, link=_random_link(k) if with_tl else None)
    assert set(ref["recs"]["type"].tolist()) == set(P_ALL if with_tl else P_NO_TL)
    assert 0 < ref["n_sn"] < ref["n_rec"] < k
    if with_tl:
        assert (ref["ch_aux"] & R.TOMBSTONE).any()


BORDERS = {
    "on_8t_and_2048b": [8, 16, 2040, 2048, 2056, 4096],
    "off_by_one": [7, 9, 2047, 2049, 4095],
    "tiny_ranges": [100, 101, 103, 2048, 2049, 3000],
}


@pytest.mark.parametrize("k", [2047, 2048, 2049, 4095, 4096, 4097, 4100])
@pytest.mark.parametrize("with_tl", [False, True])
@pytest.mark.parametrize("sn_chained", [False, True])
@pytest.mark.parametrize("borders", sorted(BORDERS))
def test_many_ranges(eng, borders, sn_chained, with_tl, k):
    """Long deletions / duplications / inversions on dense candidates: spans cross range borders (visit_from swallows candidates
    of the next range; across a whole tiny range: test_visit_from_across_a_tiny_range), blocked ends exceed their range's clip."""
    L = 12 * k
    block = dict(BLOCK)
    if sn_chained:
        block[SN] = 3                                                     # above the sampling distance: SNPs block, all chained
    ranges = _random_ranges(k, [b for b in BORDERS[borders] if b < k], k + len(borders), L, P_ALL if with_tl else P_NO_TL, max_len=60)
    ref = _run(eng, L, block, ranges, sn_chained=sn_chained, link=_random_link(3) if with_tl else None)
    vf = ref["visit_from"]
    first = [ref["cand_pos"][a] for a, _ in ref["rt"]]
    if k == 4100:                                                         # (every border of the set in use: the shape keeps its point)
        assert any(v > f for v, f in zip(vf[1:], first[1:])), "no span crossed a range border"


def test_blocked_end_on_before_and_behind_the_next_candidate(eng):
    """DE at p, stop s, block 7: range(p, s + 8).  The next SNP at s + 7 (inside), s + 8 (the first one outside), s + 9."""
    pos, typ, ln = [], [], []
    for i, gap in enumerate((7, 8, 9)):
        p = 1000 * (i + 1)
        pos += [p, p + 19 + gap]                                          # stop = p + 19
        typ += [DE, SN]
        ln += [20, None]
    ref = _run(eng, 10_000, BLOCK, [{"clip": 10_000, "pos": pos, "type": typ, "length": ln}])
    assert ref["recs"]["pos"].tolist() == [1000, 2000, 2027, 3000, 3028]
    # the same for an insertion (range(p, p + 1 + 5): its length does not matter) and one thread's 8 items apart
    pos = [100, 105, 200, 206, 300, 307]
    ref = _run(eng, 10_000, BLOCK, [{"clip": 10_000, "pos": pos, "type": [IN, SN] * 3, "length": [30, None] * 3}])
    assert ref["recs"]["pos"].tolist() == [100, 200, 206, 300, 307]


def test_blocked_end_beyond_the_clip(eng):
    """An insertion's blocked range reaches past its range's end; the next range starts a fresh boundary pass (mutator.py:184),
    so its first SNP, right behind the clip, is kept -- and the second range's own insertion blocks as usual."""
    ranges = [{"clip": 150, "pos": [100, 140, 144], "type": [SN, IN, SN], "length": [None, 3, None]},
              {"clip": 400, "pos": [150, 152, 200, 204, 206], "type": [SN, SN, IN, SN, SN], "length": [None, None, 2, None, None]}]
    ref = _run(eng, 400, {**BLOCK, IN: 50}, ranges)
    assert ref["recs"]["pos"].tolist() == [100, 140, 150, 152, 200]


def test_visit_from_across_a_tiny_range(eng):
    """A deletion of range 0 spans the whole of range 1 and the first candidates of range 2: they pass their own ranges' boundary
    passes and are never visited (mutator.py:376)."""
    ranges = [{"clip": 150, "pos": [100], "type": [DE], "length": [301]},                  # stop 400
              {"clip": 160, "pos": [155], "type": [IN], "length": [4]},
              {"clip": 1000, "pos": [200, 300, 400, 402, 500], "type": [SN, DU, SN, SN, IV], "length": [None, 10, None, None, 5]}]
    ref = _run(eng, 1000, BLOCK, ranges)
    assert ref["visit_from"].tolist() == [0, 401, 401]
    assert ref["recs"]["pos"].tolist() == [100, 402, 500] and ref["pool_len"] == 0 and ref["len_delta"] == -301


def test_positions_and_stops_near_2_32(eng):
    """An insertion 10 below the end of a contig of 2^32 - 1 bases with block 100: its blocked end saturates instead of wrapping,
    and the SNPs behind it stay dropped; a deletion clamped to the last base."""
    L = (1 << 32) - 1
    block = {**BLOCK, IN: 100}
    ranges = [{"clip": L, "pos": [5, L - 300, L - 200, L - 11, L - 8, L - 4, L - 2], "type": [SN, DE, SN, IN, SN, SN, SN],
               "length": [None, 50, None, 2, None, None, None]}]
    ref = _run(eng, L, block, ranges)
    assert ref["recs"]["pos"].tolist() == [5, L - 300, L - 200, L - 11] and ref["rec_off"].tolist() == [5, L - 300, L - 250, L - 61]
    ranges = [{"clip": L, "pos": [7, L - 40, L - 20], "type": [SN, DE, SN], "length": [None, 500, None]}]      # stop clamped to L - 1
    ref = _run(eng, L, BLOCK, ranges)
    assert ref["recs"]["stop"].tolist() == [7, L - 1] and ref["len_delta"] == -40


def test_nothing_kept_and_all_snps(eng):
    L = 10_000
    ref = _run(eng, L, BLOCK, [{"clip": L, "pos": [10, 20, 9990], "type": [IV, IV, IV], "length": [None, None, None]}])
    assert ref["n_rec"] == 0 and ref["len_delta"] == 0
    k = CB + 1
    ref = _run(eng, L, BLOCK, [{"clip": L, "pos": list(range(0, 2 * k, 2)), "type": [SN] * k, "length": [None] * k}])
    assert ref["n_rec"] == ref["n_sn"] == k and ref["sn_index"].tolist() == list(range(k))


@pytest.mark.parametrize("total", [0, 1, 2, 3, 4, 5, 1027])
def test_pool_lengths(eng, total):
    """pool_len % 4 of 0..3 (k_pool_fill writes whole dwords), none at all, and more than one workgroup's."""
    L = 100_000
    lens = [total] if total <= 5 else [1, 2, 1000, 24]
    pos = [50 * (i + 1) for i in range(len(lens))]
    if total == 0:
        ranges = [{"clip": L, "pos": [10, 50], "type": [SN, DE], "length": [None, 3]}]
    else:
        ranges = [{"clip": L, "pos": pos, "type": [IN] * len(lens), "length": lens}]
    ref = _run(eng, L, BLOCK, ranges, seed=total)
    assert ref["pool_len"] == total and set(ref["pool"].tolist()) <= set(b"ATGC")


def test_large_length_changes(eng):
    L = 1_500_000_000
    ref = _run(eng, L, BLOCK, [{"clip": L, "pos": [10, 1_200_000_000], "type": [DU, SN], "length": [1_000_000_000, None]}])
    assert ref["len_delta"] == 1_000_000_000 and ref["rec_off"].tolist() == [10, 2_200_000_000]
    ref = _run(eng, L, BLOCK, [{"clip": L, "pos": [10, 1_200_000_000], "type": [DE, SN], "length": [1_000_000_000, None]}])
    assert ref["len_delta"] == -1_000_000_000 and ref["rec_off"].tolist() == [10, 200_000_000]


def test_translocations_on_block_edges(eng):
    """Tombstoned TL / TLI entries as the last candidate of workgroup 0 and the first of workgroup 1; a tombstoned TL that still
    blocks the SNP behind it; linked TLI records with their source span and flags."""
    k = CB + 40
    pos = list(range(10, 10 + 20 * k, 20))
    typ = [SN] * k
    ln = [None] * k
    for j, t, n in ((3, TL, 30), (4, SN, None), (100, TLI, None), (CB - 1, TL, 5), (CB, TLI, None), (CB + 1, TL, 1), (CB + 9, TLI, None),
                    (CB + 20, TLI, None), (CB + 30, TL, 8)):
        typ[j], ln[j] = t, n
    # TLs at 3 (stop covers candidate 4: that SNP is blocked), CB - 1, CB + 1, CB + 30; TLIs at 100, CB, CB + 9, CB + 20
    link = {"tombstones": [], "pairs": [(pos[CB - 1], pos[100], 1), (pos[CB + 30], pos[CB], 1), (pos[CB + 1], pos[CB + 9], 1),
                                        (pos[3], pos[CB + 20], 0)]}
    ref = _run(eng, 20 * k + 100, BLOCK, [{"clip": 20 * k + 100, "pos": pos, "type": typ, "length": ln}], link=link)
    tli = ref["recs"][ref["recs"]["type"] == TLI]
    assert tli["aux"].tolist() == [3, 3, 2, 2] and tli["extra"].tolist() == [pos[CB - 1], pos[CB + 30], pos[CB + 1], pos[3]]
    assert pos[4] not in ref["recs"]["pos"]
    # four TLs, two TLIs: __fix_tl_amount deletes two TLs -- the last candidate of workgroup 0 and the first of workgroup 1, whose
    # span still blocks the SNP behind it
    typ, ln = [SN] * k, [None] * k
    for j, t, n in ((3, TL, 30), (100, TLI, None), (CB - 1, TL, 5), (CB, TL, 30), (CB + 9, TLI, None), (CB + 30, TL, 8)):
        typ[j], ln[j] = t, n
    link = {"tombstones": [pos[CB - 1], pos[CB]], "pairs": [(pos[CB + 30], pos[100], 1), (pos[3], pos[CB + 9], 0)]}
    ref = _run(eng, 20 * k + 100, BLOCK, [{"clip": 20 * k + 100, "pos": pos, "type": typ, "length": ln}], link=link)
    got = set(ref["recs"]["pos"].tolist())
    assert not got & {pos[4], pos[CB - 1], pos[CB], pos[CB + 1]} and pos[CB + 2] in got
    assert np.count_nonzero(ref["ch_aux"] & R.TOMBSTONE) == 2 and ref["n_rec"] == k - 4


def test_unlinked_insertions_have_an_empty_span(eng):
    """No TL on the contig: nothing is linked (mutator.py:130), a TLI keeps start = its position and stop = 0 -- extra > stop, a
    copied span of no bases -- and blocks the absolute range(start, 1 + block)."""
    block = {**BLOCK, TLI: 60}
    ranges = [{"clip": 5000, "pos": [0, 30, 60, 62, 500, 502], "type": [TLI, TLI, SN, SN, TLI, SN], "length": [None] * 6}]
    ref = _run(eng, 5000, block, ranges)
    # candidate 30 and 60 lie in range(0, 61); the TLI at 500 blocks nothing: range(500, 61) is empty
    assert ref["recs"]["pos"].tolist() == [0, 62, 500, 502]
    assert ref["recs"]["extra"].tolist() == [0, 0, 500, 0] and ref["recs"]["stop"].tolist() == [0, 62, 0, 502] and ref["len_delta"] == 1


def test_blocked_end_carried_across_more_than_1024_workgroups(eng):
    """More than 1024 * 2048 candidates, nearly all SNPs; a deletion in workgroup 3 whose blocked range ends in workgroup 1030: the
    running maximum crosses k_scan_max_u32's second chunk of 1024 workgroup maxima, the kept counts and the length change cross
    k_scan4's.  Two insertions behind it take their pool offsets from that carry.  The reference here is numpy's."""
    k = 1024 * CB + 8 * CB + 77
    _params(eng, BLOCK)
    pos = np.arange(k, dtype=np.uint32) * 2 + 10
    typ = np.full(k, SN, dtype=np.uint8)
    j_de, j_end = 3 * CB + 5, 1030 * CB + 100
    j_in = [j_end + 50, k - 3]
    typ[j_de] = DE
    typ[j_in] = IN
    de_stop = int(pos[j_end]) - 8                                         # range(pos, stop + 1 + 7): candidate j_end is the first one outside
    L = int(pos[-1]) + 100
    ch_rank = np.array([j_de] + j_in, dtype=np.uint32)
    ch_stop = np.array([de_stop, pos[j_in[0]] + 4, pos[j_in[1]] + 2], dtype=np.uint32)         # inserts of 5 and 3 bases
    words = _np_words(16)
    got = eng.mixed_emit(L, pos, typ, ch_rank, ch_stop, R.untemper(words))
    blocked = np.zeros(k, dtype=bool)
    blocked[j_de + 1:j_end] = True                                        # SNPs inside range(pos[j_de], de_stop + 8)
    for j in j_in:                                                        # an insertion blocks range(pos, pos + 6): the next two SNPs
        blocked[j + 1:j + 3] = True
    keep = ~blocked
    n_rec = int(keep.sum())
    recs = np.zeros(n_rec, dtype=R.RECORD_DTYPE)
    recs["pos"] = recs["stop"] = pos[keep]
    recs["type"] = typ[keep]
    idx = np.cumsum(keep) - 1
    recs["stop"][idx[ch_rank]] = ch_stop
    recs["extra"][idx[j_in[1]]] = 5
    delta = np.zeros(n_rec, dtype=np.int64)
    delta[idx[j_de]] = -(de_stop - int(pos[j_de]) + 1)
    delta[idx[j_in[0]]], delta[idx[j_in[1]]] = 5, 3
    rec_off = recs["pos"].astype(np.int64) + np.cumsum(delta) - delta
    assert got["n_rec"] == n_rec and got["n_sn"] == n_rec - 3 and got["pool_len"] == 8 and got["len_delta"] == int(delta.sum())
    assert got["recs"].tobytes() == recs.tobytes()
    assert np.array_equal(got["rec_off"], rec_off.astype(np.uint32))
    assert np.array_equal(got["sn_index"], np.flatnonzero(recs["type"] == SN).astype(np.uint32))
    assert got["pool"].tobytes() == bytes(b"ATGC"[int(w) & 3] for w in words[:8])


def test_the_emit_hook_refuses_what_the_planners_cannot_produce(eng):
    _params(eng, BLOCK)
    L = 1000
    words = np.zeros(64, dtype=np.uint32)
    pos, typ = [10, 20, 30, 40], [SN, DE, SN, IN]
    good = dict(cand_pos=pos, cand_type=typ, ch_rank=[1, 3], ch_stop=[25, 41])
    assert eng.mixed_emit(L, np_words=words, **good)["n_rec"] == 3
    D = R.DROPPED
    rt2 = np.zeros(2, dtype=_ffi.MIX_RANGE_DTYPE)
    POS, RANK, STOP = "strictly increasing positions below the contig's length", "ch_rank does not list exactly", "a stop that is neither CHAIN_DROPPED"
    bad = [
        (POS, dict(good, cand_pos=[10, 20, 20, 40])),                     # positions not strictly increasing
        (POS, dict(good, cand_pos=[10, 20, 30, 1000])),                   # ... beyond the contig
        (POS, dict(good, cand_type=[SN, 0, SN, IN])), (POS, dict(good, cand_type=[SN, 8, SN, IN])),
        (RANK, dict(good, ch_rank=[3, 1])), (RANK, dict(good, ch_rank=[1, 2])), (RANK, dict(good, ch_rank=[1], ch_stop=[25])),
        (RANK, dict(good, ch_rank=[0, 1, 3], ch_stop=[10, 25, 41])),      # an SNP on the chain without sn_chained
        ("lists candidates off the chain", dict(good, cand_pos=pos + [50], cand_type=typ + [SN], ch_rank=[1, 3, 4], ch_stop=[25, 41, 50])),
        (STOP, dict(good, ch_stop=[19, 41])),                             # a stop below its position
        (STOP, dict(good, ch_stop=[1000, 41])),                           # a deletion's stop beyond the contig
        (STOP, dict(good, ch_stop=[25, D - 1])),                          # an insert's stop of 2^32 - 2
        ("fewer words / less room than insert bases", dict(good, ch_stop=[25, 200])),
        ("a translocation without ch_extra / ch_aux", dict(good, cand_type=[SN, TL, SN, IN])),
        ("msim_dbg_mixed_emit: bad argument", dict(good, ch_extra=[0, 0])),                     # one of the two only
        ("ch_aux flags outside what linking sets", dict(good, ch_extra=[0, 0], ch_aux=[0x40, 0])),
        ("ch_aux flags outside what linking sets", dict(good, ch_extra=[0, 0], ch_aux=[R.TOMBSTONE, 0])),   # a tombstoned deletion
        ("msim_dbg_mixed_emit: bad argument", dict(good, ranges=rt2)),                          # a range table without visit_from
        ("an SNP could block its successor", dict(good, cand_pos=[10, 11, 30, 40], ch_stop=[15, 41])),
    ]
    for check, kw in bad:
        with refused(check):
            eng.mixed_emit(L, np_words=words, **kw)
    rt2["rec_base"], rt2["clip"] = [1, 2], [25, L]
    with refused("the range table starts at candidate 0"):
        eng.mixed_emit(L, np_words=words, ranges=rt2, visit_from=[0, 0], **good)
    for bases, clips in (([0, 0], [25, L]), ([0, 4], [25, L]), ([0, 2], [20, L]), ([0, 2], [31, L]), ([0, 2], [25, 40])):
        rt2["rec_base"], rt2["clip"] = bases, clips
        with refused("rec_base not strictly increasing below k, or a clip"):
            eng.mixed_emit(L, np_words=words, ranges=rt2, visit_from=[0, 0], **good)
    rt2["rec_base"], rt2["clip"] = [0, 2], [30, L]
    # (a border behind the deletion: the SNP at 30 meets a fresh boundary pass and the walk is past the span, so it is kept)
    assert eng.mixed_emit(L, np_words=words, ranges=rt2, visit_from=[0, 26], **good)["n_rec"] == 4
    # a deletion of range 0 reaching into range 1, whose SNPs are visited all the same (visit_from is taken as given)
    rt2["rec_base"], rt2["clip"] = [0, 1], [50, 100]
    over = dict(cand_pos=[10, 50, 60], cand_type=[DE, SN, SN], ch_rank=[0], ch_stop=[90])       # an SNP 81 bases left of position 60
    with refused("an output offset outside [0, 2^32)"):
        eng.mixed_emit(100, np_words=words, ranges=rt2, visit_from=[0, 0], **over)
    with refused("mutated length or insert bases outside [0, 2^32)"):      # 2^32 - 1 bases and a duplication of 2^31 more
        eng.mixed_emit((1 << 32) - 1, cand_pos=[10], cand_type=[DU], ch_rank=[0], ch_stop=[(1 << 31)], np_words=words)
