"""k_sample_tail -- the sampler's tail rounds and exact stream cut -- on hand-built tables, through ``Engine.sample_tail``
(msim_dbg_sample_tail), against ``tests/sample_tail_ref.py``: the PlanState and every bitmap word, guards included, must be equal.

The windows are made word by word: which words are accepted draws and what they draw is chosen, the rest are rejected draws, and
the engine is handed the inverse tempering of all that.  So the cut can be put on a chosen word of a chosen block (lane and wave
borders of the kernel's layout of the cut's block -- two words per lane of 1024 today: every 2 and every 128 words; the borders
of an eight-words-per-lane layout of 256, every 8 and every 512, are here too, for the four-wave form of NOTES section 30), a
round can be given a chosen number of draws (around one and several trips of 256 and of 1024 lanes), and the block table a
chosen shape (the threshold inside and at the end of a lane's run of counts, at TAIL_LDS_OFFS blocks).  Every case runs in all
the forms the kernel has for it: counts or prefix sums, the list from accepted index 0 or from k."""
from __future__ import annotations

import numpy as np
import pytest

import sample_tail_ref as tr
from mutation_simulator_amd import _ffi

pytestmark = pytest.mark.gpu

B = tr.ACC_BLOCK
N_SMALL = 300_007                                         # 19 bits, 43 % of the draws rejected by value alone
GUARD = 4


@pytest.fixture(scope="module")
def eng():
    with _ffi.Engine(0) as e:
        yield e


class Window:
    """Tempered words [0, p0 + W) whose window words at ``acc_at`` (sorted, relative to p0) draw ``vals`` and whose other window
    words are rejected draws; the words in front of p0 are noise nobody may read."""

    def __init__(self, W, n, acc_at, vals, p0=5, seed=1):
        rng = np.random.default_rng(seed)
        shift = tr.shift_of(n)
        assert n < (1 << (32 - shift)), "a power of two rejects nothing"
        v = rng.integers(n, 1 << (32 - shift), W, dtype=np.uint64)
        v[np.asarray(acc_at, dtype=np.int64)] = np.asarray(vals, dtype=np.uint64)
        t = ((v << np.uint64(shift)) | rng.integers(0, 1 << shift, W, dtype=np.uint64)).astype(np.uint32)
        self.words = np.concatenate([rng.integers(0, 1 << 32, p0, dtype=np.uint64).astype(np.uint32), t])
        self.raw = tr.untemper(self.words)
        self.W, self.n, self.p0, self.shift = W, n, p0, shift
        self.acc, self.counts, self.offs = tr.window_tables(self.words, p0, W, n)
        assert np.array_equal(self.acc, np.asarray(vals, dtype=np.uint32))


def spread(W, count, must=(), seed=2):
    """``count`` accepted-word indices of a window of W words: ``must`` and a random rest, sorted."""
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(W), np.asarray(must, dtype=np.int64))
    pick = rng.choice(rest, count - len(must), replace=False)
    return np.sort(np.concatenate([pick, np.asarray(must, dtype=np.int64)]).astype(np.int64))


def distinct(count, n, seed=3):
    return np.random.default_rng(seed).choice(n, count, replace=False).astype(np.uint32)


def run_all_forms(eng, win, k, state=None, bitmap=None, anchor=None, pos_limit=2 ** 64 - 1, W=None, tables=None):
    """The case through the reference once and through the kernel in every form it allows; returns the reference's state.
    W / tables: a shorter window over the same words, with its (acc, counts, offs)."""
    W = win.W if W is None else W
    acc, counts, offs = (win.acc, win.counts, win.offs) if tables is None else tables
    dups = 0
    first = k if anchor is None else k + anchor[0]
    if bitmap is None:
        bitmap, dups = tr.bitmap_of(acc[:first], win.n)
    st0 = {"pos": win.p0, "snp_base": win.p0, "flags": 0, "dups": 0, "accepted_used": 0}
    if anchor is None:
        st0["dups"] = dups if state is None or "dups" not in state else state["dups"]
        w = None
    else:                                                # the window's origin comes from ps_win; the chain's position is elsewhere
        st0["pos"] = st0["snp_base"] = 3
        w = (win.p0, anchor[0], anchor[1])
    st0.update({f: v for f, v in (state or {}).items() if f != "dups"})
    want_st, want_bm = tr.sample_tail(win.words, acc, offs, W, win.n, k, bitmap, st0, win=w, pos_limit=pos_limit)
    want_full = np.concatenate([np.full(GUARD, 0xEEEEEEEE, np.uint32), want_bm, np.full(GUARD, 0xEEEEEEEE, np.uint32)])
    forms = [(raw_counts, acc_first) for raw_counts in (True, False) for acc_first in (0, k)
             if not (raw_counts and len(counts) > tr.TAIL_LDS_OFFS)]
    assert forms
    for raw_counts, acc_first in forms:
        got_st, got_bm = eng.sample_tail(win.raw, acc[acc_first:], acc_first, counts if raw_counts else offs, raw_counts, W, win.shift,
                                         win.n, k, bitmap, st0, win=w, pos_limit=pos_limit, guard=GUARD)
        assert got_st == want_st, (raw_counts, acc_first, got_st, want_st)
        assert np.array_equal(got_bm, want_full), (raw_counts, acc_first, "bitmap or its guards differ")
    return want_st


# ---------------------------------------------------------------------------------------------- blocks and cut positions
CUT_WORDS = [0, 1, 2, 7, 8, 127, 128, 511, 512, 1535, 1536, 2047]      # first / last word, both sides of lane and wave borders


@pytest.mark.parametrize("n_blocks", [1, 2, 33])
@pytest.mark.parametrize("ragged", [1, -1])
def test_cut_words(eng, n_blocks, ragged):
    """The cut on chosen words of the window's last whole block (and of its ragged last block), W = 2048 q + 1 and 2048 q - 1."""
    W = n_blocks * B + ragged
    blk = (W // B - 1) if W >= B else 0                    # the last block with all its words (or the only, ragged one)
    cut_words = [w for w in CUT_WORDS if blk * B + w < W]
    last = W - 1                                          # ... and the window's very last word
    must = sorted({blk * B + w for w in cut_words} | {last})
    at = spread(W, max(len(must) + 40, W // 3), must)
    win = Window(W, N_SMALL, at, distinct(len(at), N_SMALL), p0=5 + n_blocks)
    for word in must:
        k = int(np.searchsorted(at, word)) + 1            # no duplicate: the k-th accepted draw is the last one consumed
        st = run_all_forms(eng, win, k)
        assert st["pos"] == win.p0 + word + 1 and st["accepted_used"] == k and st["flags"] == 0


@pytest.mark.parametrize("n_blocks", [2, 33])
def test_last_draw_on_the_first_and_last_accepted_draw_of_a_block(eng, n_blocks):
    """A = offs[b] + 1 (the block's first accepted draw: `< A` against `<= A` in the block search) and A = offs[b + 1] (its last);
    with empty blocks in front of and behind b, whose offsets equal their neighbours'."""
    W = n_blocks * B + 1
    rng = np.random.default_rng(7)
    blocks = [0, n_blocks - 1] if n_blocks == 2 else [0, 7, 8, 15, 16, 31, 32]      # (7 | 8, 31 | 32: two lanes' runs of 8 or 32 counts)
    at = np.sort(np.concatenate([b * B + rng.choice(B, 9, replace=False) for b in blocks]))      # every other block is empty
    win = Window(W, N_SMALL, at, distinct(len(at), N_SMALL))
    for j in range(len(blocks)):
        for k in (9 * j + 1, 9 * j + 9):
            st = run_all_forms(eng, win, k)
            assert st["pos"] == win.p0 + int(at[k - 1]) + 1 and st["flags"] == 0


# ---------------------------------------------------------------------------------------------- rounds
@pytest.mark.parametrize("first_round", [0, 1, 255, 256, 257, 4 * 256 - 1, 4 * 256, 4 * 256 + 1, 8 * 256 - 1, 8 * 256 + 1, 12_000])
def test_first_round_sizes(eng, first_round):
    """``first_round`` duplicates among the first k draws: the first round consumes that many more, all new."""
    D, k = first_round, 2 * first_round + 100
    vals = distinct(k + D + 50, N_SMALL)
    vals[k - D:k] = vals[:D]                               # the last D of the first k repeat the first D
    W = (2 * len(vals) // B + 2) * B + 77
    at = spread(W, len(vals), seed=first_round + 1)
    win = Window(W, N_SMALL, at, vals)
    st = run_all_forms(eng, win, k)
    assert st["accepted_used"] == k + D and st["pos"] == win.p0 + int(at[k + D - 1]) + 1 and st["flags"] == 0


def test_a_duplicate_whose_replacement_is_a_duplicate(eng):
    k, W = 500, 2 * B - 1
    vals = distinct(k + 60, N_SMALL)
    vals[k - 1] = vals[0]                                 # one duplicate among the first k
    vals[k] = vals[7]                                     # its replacement: there already
    vals[k + 1] = vals[k - 1]                             # ... and that one's too; the next is new
    at = spread(W, len(vals))
    st = run_all_forms(eng, Window(W, N_SMALL, at, vals), k)
    assert st["accepted_used"] == k + 3 and st["flags"] == 0


@pytest.mark.parametrize("apart", [1, 63, 64, 256, 3 * 256])
def test_two_equal_values_inside_one_batch(eng, apart):
    """Two draws of one round with the same NEW value, ``apart`` list entries from each other (the neighbouring lane, the next
    wave, a lane's next draw in a workgroup of 256; the same trip of 1024 lanes throughout): exactly one of them counts as a
    duplicate."""
    D, k = 1100, 2400
    vals = distinct(k + D + 40, N_SMALL)
    vals[k - D:k] = vals[:D]
    vals[k + 5 + apart] = vals[k + 5]
    W = 4 * B + 9
    at = spread(W, len(vals))
    st = run_all_forms(eng, Window(W, N_SMALL, at, vals), k)
    assert st["accepted_used"] == k + D + 1 and st["flags"] == 0


# ---------------------------------------------------------------------------------------------- the block table
@pytest.fixture(scope="module")
def big():
    """A window of TAIL_LDS_OFFS + 1 blocks with few accepted draws (its prefixes are the windows of the cases below): some
    blocks empty, the draws of the others few enough that a lane's 32 counts matter one by one."""
    nb = tr.TAIL_LDS_OFFS + 1
    W = nb * B
    rng = np.random.default_rng(11)
    per_block = rng.integers(0, 4, nb)
    per_block[[0, 16, 17, 8160, 8175, 8189, 8190, 8191, 8192]] = [1, 2, 0, 3, 1, 2, 1, 2, 3]
    at = np.sort(np.concatenate([b * B + rng.choice(B, c, replace=False) for b, c in enumerate(per_block) if c]))
    n = (1 << 20) + 1
    return Window(W, n, at, distinct(len(at), n), p0=9), per_block


@pytest.mark.parametrize("n_blocks", [tr.TAIL_LDS_OFFS - 1, tr.TAIL_LDS_OFFS, tr.TAIL_LDS_OFFS + 1])
def test_block_counts_around_the_table_size(eng, big, n_blocks):
    """n_blocks below, at and above TAIL_LDS_OFFS (raw counts where the kernel takes them, prefix sums always); the last draw in
    the first block, inside a lane's 32 counts, in the last lane (blocks 8160 ..) and in the window's last block."""
    win, _ = big
    W = n_blocks * B - 3
    tables = tr.window_tables(win.words, win.p0, W, win.n)
    offs = tables[2]
    for b in (0, 16, 18, 8160, 8175, n_blocks - 1):
        if offs[b + 1] == offs[b]:
            continue
        for k in (int(offs[b]) + 1, int(offs[b + 1])):    # the block's first and last accepted draw
            st = run_all_forms(eng, win, k, W=W, tables=tables)
            assert st["flags"] == 0 and (st["pos"] - win.p0 - 1) // B == b and st["accepted_used"] == k


# ---------------------------------------------------------------------------------------------- the anchored form
@pytest.mark.parametrize("d1", [0, 1, 300])
def test_anchored_window(eng, d1):
    """ps_win and hdr given: the window starts at ps_win's position (not the chain's), k + need0 draws are consumed already and
    d1 duplicates are left to replace."""
    k, need0, W = 900, 37, 3 * B + 1
    vals = distinct(k + need0 + 400, N_SMALL)
    vals[k + need0 - d1:k + need0] = vals[:d1]            # the last d1 of the draws consumed already repeat the first d1
    at = spread(W, len(vals))
    win = Window(W, N_SMALL, at, vals, p0=11)
    bitmap, dups = tr.bitmap_of(win.acc[:k + need0], win.n)
    assert dups == d1
    st = run_all_forms(eng, win, k, bitmap=bitmap, anchor=(need0, d1))
    assert st["accepted_used"] == k + need0 + d1 and st["flags"] == 0 and st["pos"] == win.p0 + int(at[k + need0 + d1 - 1]) + 1


# ---------------------------------------------------------------------------------------------- flags and the clamp
def test_overflow_flags_and_the_clamp(eng):
    k, W = 600, 2 * B + 1
    vals = distinct(k + 30, N_SMALL)
    vals[k - 4:k] = vals[:4]
    at = spread(W, len(vals))
    win = Window(W, N_SMALL, at, vals)
    end = win.p0 + int(at[k + 4 - 1]) + 1
    assert run_all_forms(eng, win, k) == {"pos": end, "snp_base": end, "flags": 0, "dups": 4, "accepted_used": k + 4}
    # (1) the window does not even hold the first k accepted draws
    st = run_all_forms(eng, win, len(vals) + 1, state={"dups": 0})
    assert st["flags"] == 1 and st["pos"] == win.p0 and st["accepted_used"] == 0
    # (2) a round asks for more draws than the window holds
    st = run_all_forms(eng, win, k, state={"dups": 31})
    assert st["flags"] == 1 and st["pos"] == win.p0
    # (3) the cut lies beyond the limit: clamped to it, flag raised -- one word short, and exactly at the limit
    st = run_all_forms(eng, win, k, pos_limit=end - 1)
    assert st["flags"] == 1 and st["pos"] == end - 1 and st["snp_base"] == end - 1 and st["accepted_used"] == k + 4
    assert run_all_forms(eng, win, k, pos_limit=end)["flags"] == 0
    # flags that are there already stay
    assert run_all_forms(eng, win, k, state={"flags": 2})["flags"] == 2
    assert run_all_forms(eng, win, k, state={"flags": 2}, pos_limit=end - 1)["flags"] == 3


def test_refuses_what_it_cannot_run(eng):
    k, W = 50, B + 5
    vals = distinct(k + 30, N_SMALL)
    at = spread(W, len(vals))
    win = Window(W, N_SMALL, at, vals)
    bitmap, _ = tr.bitmap_of(win.acc[:k], win.n)
    st = {"pos": win.p0, "snp_base": win.p0}
    ok = dict(words=win.raw, acc=win.acc, acc_first=0, blocks=win.counts, raw_counts=True, W=W, shift=win.shift, n=win.n, k=k,
              bitmap=bitmap, state=st)
    eng.sample_tail(**ok)
    for bad in (dict(W=W + B), dict(words=win.raw[:-1]), dict(acc=win.acc[:-1]), dict(acc_first=k + 1), dict(shift=32),
                dict(acc=np.where(np.arange(len(win.acc)) == 3, win.n, win.acc)), dict(state={"pos": win.p0 + 1, "snp_base": 0})):
        with pytest.raises(_ffi.MsimError):
            eng.sample_tail(**{**ok, **bad})
