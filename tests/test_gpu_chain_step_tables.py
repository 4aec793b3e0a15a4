"""An anchored contig's stream chain -- fringe pass, tail rounds, stream cut, SNP scan and cut -- on hand-built tables, through
``Engine.chain_step`` (msim_dbg_chain_step): the ONE launch the sampler sends (``k_chain_fused``) against the three stand-alone
launches (``k_ahead_fringe``, ``k_sample_tail``, ``k_snp_scan_cut_abs``: held by the existing tests.  The first and the last now
share their bodies with the fused kernel; ``k_snp_scan_cut_abs`` also changed in itself -- it loads its first chunk of block maps
in front of the partial block's scan and raises its flag by ``atomicOr`` -- with the same results).  State,
header, bitmap with its guards, ``win_maps`` with its guard entry and the saved base must be equal byte for byte; where an overflow
flag is raised the fused launch may skip what follows (the pass is discarded), so there the flag and the guards are compared.

The sample part is also held against ``tests/sample_tail_ref.py`` (the fringe pass restated here in a few lines), and the SNP
cut against arithmetic where every uniform is a transition (two words an SNP).

Head interval and window are made word by word, as in ``tests/test_gpu_sample_tail_tables.py``: which words are accepted draws and
what they draw is chosen, the rest are rejected draws."""
from __future__ import annotations

import numpy as np
import pytest

import sample_tail_ref as tr
from mutation_simulator_amd import _ffi
from test_gpu_sample_tail_tables import CUT_WORDS, distinct, spread

pytestmark = pytest.mark.gpu

B = tr.ACC_BLOCK
SNP_BLOCK = 8192
N_SMALL = 300_007                                         # 19 bits, 43 % of the draws rejected by value alone
GUARD = 4
EE = 0xEEEEEEEE
TI_ALL = 1 << 53                                          # every uniform a transition: an SNP is exactly two words
TI_NONE = 0                                               # every SNP a transversion: a randbelow(2) loop behind the uniform
TI_2 = int((2.0 * (1.0 / 3.0)) * (1 << 53)) + 1           # titv 2.0
FLAG_SAMPLE, FLAG_SNP = 1, 2


@pytest.fixture(scope="module")
def eng():
    with _ffi.Engine(0) as e:
        yield e


class Chain:
    """Tempered words: noise [0, lo), the head interval [lo, H) whose words at ``head_at`` draw ``head_vals``, the window
    [H, H + W) whose words at ``win_at`` draw ``win_vals`` (every other word of both a rejected draw), then noise for the SNP
    draws up to the last mapped block."""

    def __init__(self, n, lo, F, head_at, head_vals, W, win_at, win_vals, W2=20_000, seed=1):
        rng = np.random.default_rng(seed)
        shift = tr.shift_of(n)
        assert n < (1 << (32 - shift)), "a power of two rejects nothing"

        def seg(L, at, vals):
            v = rng.integers(n, 1 << (32 - shift), L, dtype=np.uint64)
            v[np.asarray(at, dtype=np.int64)] = np.asarray(vals, dtype=np.uint64)
            return ((v << np.uint64(shift)) | rng.integers(0, 1 << shift, L, dtype=np.uint64)).astype(np.uint32)

        def noise(L):
            return rng.integers(0, 1 << 32, L, dtype=np.uint64).astype(np.uint32)

        H = lo + F
        n_words = ((H + W) // SNP_BLOCK + W2 // SNP_BLOCK + 3) * SNP_BLOCK
        self.words = np.concatenate([noise(lo), seg(F, head_at, head_vals), seg(W, win_at, win_vals), noise(n_words - H - W)])
        self.raw = tr.untemper(self.words)
        self.n, self.shift, self.lo, self.F, self.H, self.W, self.W2 = n, shift, lo, F, H, W, W2
        self.head_at = np.asarray(head_at, dtype=np.int64)
        self.head_vals = np.asarray(head_vals, dtype=np.uint32)
        nbh = (F + B - 1) // B
        self.hcnt = np.zeros(nbh, dtype=np.uint32)
        self.hacc = np.full(nbh * B, 0xFFFFFFFF, dtype=np.uint32)     # (entries nobody wrote are no draws)
        for b in range(nbh):
            sel = (self.head_at >= b * B) & (self.head_at < (b + 1) * B)
            self.hcnt[b] = sel.sum()
            self.hacc[b * B:b * B + int(sel.sum())] = self.head_vals[sel]
        self.acc, self.cnt, self.offs = tr.window_tables(self.words, H, W, n)
        assert np.array_equal(self.acc, np.asarray(win_vals, dtype=np.uint32))

    def head_from(self, s):
        return self.head_vals[self.head_at >= s - self.lo]

    def expect_sample(self, s, K, k_core, bitmap, core_dups, state, pos_limit):
        """(state, bitmap, need0, d1) behind fringe, rounds and cut -- None where the fringe pass flags the sample."""
        if s < self.lo or s > self.H:
            return None
        head = self.head_from(s)
        items = K - k_core + core_dups
        if len(head) > items:
            return None
        need0 = items - len(head)
        bm = np.array(bitmap, dtype=np.uint32, copy=True)
        d1 = 0
        for v in list(head) + list(self.acc[k_core:k_core + need0]):
            w, b = int(v) >> 5, np.uint32(1 << (int(v) & 31))
            d1 += 1 if bm[w] & b else 0
            bm[w] |= b
        st, bm = tr.sample_tail(self.words, self.acc, self.offs, self.W, self.n, k_core, bm, state, win=(self.H, need0, d1),
                                pos_limit=pos_limit)
        return st, bm, need0, d1


def run_both(eng, ch, s, K, k_core, K2, G, ti_lim=TI_ALL, pos_limit=2 ** 64 - 1, snp_limit=2 ** 64 - 1, state=None, core_flags=0,
             head_flags=0, check_ref=True, expect_flag=0, soft_half=1000):
    """The case as three launches and as one; compares them (and the sample part with the reference); returns the fused result."""
    bitmap, core_dups = tr.bitmap_of(ch.acc[:k_core], ch.n)
    st0 = {"pos": s, "snp_base": min(s, ch.H + ch.W), "flags": 0, "dups": 0, "accepted_used": 0, "margin": 0}
    st0.update(state or {})
    tail = ch.acc[k_core:]
    items = K - k_core + core_dups
    if len(tail) < items:                                 # (a window too small for the fringe's share: the list is padded)
        tail = np.concatenate([tail, np.zeros(items - len(tail), dtype=np.uint32)])
    res = {}
    for fused in (False, True):
        res[fused] = eng.chain_step(ch.raw, ti_lim, ch.lo, ch.F, ch.hcnt, ch.hacc, tail, ch.cnt, bitmap, st0, K, k_core, ch.shift, ch.n,
                                    ch.W, ch.W2, K2, G, fused, core_dups=core_dups, core_flags=core_flags, head_flags=head_flags,
                                    expect=ch.lo + ch.F // 2, soft_half=soft_half, pos_limit=pos_limit, snp_limit=snp_limit,
                                    guard=GUARD)
    three, one = res[False], res[True]
    for r in (three, one):                                # no write outside the guards, whatever happened
        assert np.all(r["bitmap"][:GUARD] == EE) and np.all(r["bitmap"][-GUARD:] == EE)
        assert np.all(r["win_maps"][-1] == EE)
    assert one["hdr"][2] == G and three["hdr"][2] == 0    # every workgroup took its ticket
    assert one["state"]["flags"] == three["state"]["flags"] == expect_flag, (one["state"], three["state"])
    sample_flagged = expect_flag & FLAG_SAMPLE and one["state"]["accepted_used"] == 0     # (not the clamp: that one goes on)
    if not sample_flagged:
        assert one["state"] == three["state"], (one["state"], three["state"])
        assert one["hdr"][:2] == three["hdr"][:2] and one["base"] == three["base"]
        assert np.array_equal(one["bitmap"], three["bitmap"]), "bitmap differs"
        assert np.array_equal(one["win_maps"], three["win_maps"]), "win_maps differ"
    if check_ref and not sample_flagged:
        ref_state = {f: st0[f] for f in ("pos", "snp_base", "flags", "dups", "accepted_used")}
        ref_state["flags"] |= core_flags | head_flags
        st, bm, need0, d1 = ch.expect_sample(s, K, k_core, bitmap, core_dups, ref_state, pos_limit)
        assert one["hdr"][:2] == [need0, d1]
        assert np.array_equal(one["bitmap"][GUARD:-GUARD], bm)
        assert one["state"]["accepted_used"] == st["accepted_used"] and one["state"]["snp_base"] == st["snp_base"] == one["base"]
        if ti_lim == TI_ALL and not (expect_flag & FLAG_SNP):
            assert one["state"]["pos"] == st["snp_base"] + 2 * K2
    return one


def make(n_head=600, n_win=3500, lo=37, F=3 * B - 5, W=4 * B + 9, W2=20_000, seed=1, plant=None, head_must=(), win_must=()):
    """A chain with ``n_head`` / ``n_win`` accepted draws, all distinct unless ``plant(head_vals, win_vals)`` says otherwise."""
    head_at = spread(F, n_head, head_must, seed=seed + 1) if F else np.zeros(0, dtype=np.int64)
    win_at = spread(W, n_win, win_must, seed=seed + 2)
    vals = distinct(n_head + n_win, N_SMALL, seed=seed + 3)
    head_vals, win_vals = vals[:n_head].copy(), vals[n_head:].copy()
    if plant:
        plant(head_vals, win_vals)
    return Chain(N_SMALL, lo, F, head_at, head_vals, W, win_at, win_vals, W2=W2, seed=seed)


# ---------------------------------------------------------------------------------------------- grids and item counts
@pytest.fixture(scope="module")
def plain():
    return make()


@pytest.mark.parametrize("G", [1, 2, 3, 64])
@pytest.mark.parametrize("items", [1023, 1024, 1025, 2047, 2048, 2049])
def test_fringe_grids_and_item_counts(eng, plain, G, items):
    """``items`` draws go into the bitmap in the fringe pass (the head's and the first of the tail list), dealt to G workgroups
    in strides of 256 G, four trips in flight a lane: both sides of a trip of one workgroup and of two."""
    k_core = 300
    r = run_both(eng, plain, plain.lo + 700, k_core + items, k_core, 900, G)
    assert r["state"]["flags"] == 0 and r["hdr"][1] == 0


def test_no_head_blocks(eng):
    """lo == H: the start is certain, nothing in front of the anchor."""
    ch = make(n_head=0, F=0)
    for G in (1, 3):
        r = run_both(eng, ch, ch.lo, 1500, 1000, 700, G)
        assert r["hdr"][:2] == [500, 0]


# ---------------------------------------------------------------------------------------------- where the chain starts
@pytest.mark.parametrize("where", ["first", "last", "inner_border", "end_border", "end_ragged"])
def test_starts(eng, where):
    """A start on the interval's first word, on its last word, on an inner head-block border, and at H -- on a block border
    (blk == nbh: no block holds the start) and inside the ragged last block."""
    F = 3 * B if where == "end_border" else 3 * B - 5
    ch = make(F=F, head_must=(0, B - 1, B, F - 1))
    s = {"first": ch.lo, "last": ch.H - 1, "inner_border": ch.lo + B, "end_border": ch.H, "end_ragged": ch.H}[where]
    for G in (1, 2):
        r = run_both(eng, ch, s, 1600, 700, 800, G)
        assert r["state"]["flags"] == 0
        assert r["hdr"][0] == 900 - len(ch.head_from(s))


def test_head_holds_nothing_and_head_holds_everything(eng, plain):
    """h_acc == 0 with head blocks there (no accepted draw from the start on) and h_acc == items (need0 == 0: the tail list is
    not touched by the fringe pass)."""
    ch = plain
    last = int(ch.head_at[-1])
    r = run_both(eng, ch, ch.lo + last + 1, 1200, 800, 500, 2)
    assert r["hdr"][:2] == [400, 0]
    s = ch.lo + int(ch.head_at[100])
    h_acc = len(ch.head_from(s))
    r = run_both(eng, ch, s, 800 + h_acc, 800, 500, 3)
    assert r["hdr"][:2] == [0, 0] and r["state"]["accepted_used"] == 800


# ---------------------------------------------------------------------------------------------- duplicates and rounds
K_CORE, S_OFF, ITEMS = 500, 2500, 1400                    # the cases below: start 2500 words into the interval, 1400 fringe draws


def _dup_chain(plant):
    probe = make()
    h_acc = len(probe.head_from(probe.lo + S_OFF))
    need0 = ITEMS - h_acc
    return make(plant=lambda hv, wv: plant(hv, wv, h_acc, need0)), need0


@pytest.mark.parametrize("d1", [0, 1, 300])
def test_duplicates_left_by_the_fringe_pass(eng, d1):
    """d1 of the fringe's draws are in the bitmap already -- core values met again in the head interval and in the tail list, and
    a head value met again in the tail list; with 300 the rounds take three trips: 300 draws of which 20 are duplicates, 20 of
    which one is, one."""
    def plant(hv, wv, h_acc, need0):
        if d1 >= 1:
            wv[K_CORE + 7] = hv[-3]                        # a head draw again, in the tail list
        if d1 > 1:
            hv[-40:-10] = wv[:30]                          # core values in the head interval
            wv[K_CORE + 20:K_CORE + 20 + d1 - 31] = wv[100:100 + d1 - 31]
            first = K_CORE + need0
            wv[first:first + 20] = wv[40:60]               # round 1: 20 duplicates among its 300
            wv[first + 300] = wv[70]                       # round 2: one among its 20
    ch, need0 = _dup_chain(plant)
    for G in (1, 3):
        r = run_both(eng, ch, ch.lo + S_OFF, K_CORE + ITEMS, K_CORE, 900, G)
        assert r["hdr"][:2] == [need0, d1]
        assert r["state"]["accepted_used"] == K_CORE + need0 + (0 if d1 == 0 else 1 if d1 == 1 else 321)


def test_a_duplicate_whose_replacement_is_a_duplicate(eng):
    def plant(hv, wv, h_acc, need0):
        first = K_CORE + need0
        wv[K_CORE + 3] = wv[5]                             # one duplicate in the fringe's share
        wv[first] = wv[9]                                  # its replacement: there already
        wv[first + 1] = wv[first]                          # ... and that one's too; the next is new
    ch, need0 = _dup_chain(plant)
    r = run_both(eng, ch, ch.lo + S_OFF, K_CORE + ITEMS, K_CORE, 900, 2)
    assert r["hdr"][:2] == [need0, 1] and r["state"]["accepted_used"] == K_CORE + need0 + 3


def test_duplicates_in_the_core(eng):
    """Duplicates the prep found among the core's draws (ps_core->dups) add to the fringe's share."""
    ch = make(plant=lambda hv, wv: wv.__setitem__(slice(200, 260), wv[:60]))
    r = run_both(eng, ch, ch.lo + 900, 1500, 700, 600, 3)
    assert r["hdr"][0] == 800 + 60 - len(ch.head_from(ch.lo + 900)) and r["state"]["flags"] == 0


# ---------------------------------------------------------------------------------------------- the block table and the cut
@pytest.fixture(scope="module")
def big():
    """A window of TAIL_LDS_OFFS blocks with few accepted draws (its prefix of one block less is the other case): some blocks
    empty, the draws of the others few enough that a lane's 32 counts matter one by one."""
    nb = tr.TAIL_LDS_OFFS
    W = nb * B
    rng = np.random.default_rng(11)
    per_block = rng.integers(0, 4, nb)
    per_block[[0, 16, 17, 31, 32, 8159, 8160, 8175, 8189, 8190, 8191]] = [1, 2, 0, 3, 1, 0, 3, 1, 2, 1, 2]
    at = np.sort(np.concatenate([b * B + rng.choice(B, c, replace=False) for b, c in enumerate(per_block) if c]))
    n = (1 << 20) + 1
    vals = distinct(40 + len(at), n, seed=5)
    head_at = spread(B + 3, 40, seed=6)
    return Chain(n, 9, B + 3, head_at, vals[:40], W, at, vals[40:], W2=9000, seed=4)


@pytest.mark.parametrize("n_blocks", [tr.TAIL_LDS_OFFS - 1, tr.TAIL_LDS_OFFS])
def test_block_counts_at_the_table_size(eng, big, n_blocks):
    """8191 and 8192 tail blocks (a lane keeps 32 counts: the last lane full and one short); the last draw consumed in the first
    block, across two lanes' runs of counts (31 | 32), in the last lane (8160 ..) and in the window's last block."""
    ch = big
    W = n_blocks * B - 3
    view = Chain.__new__(Chain)
    view.__dict__.update(ch.__dict__)
    view.W = W
    view.acc, view.cnt, view.offs = tr.window_tables(ch.words, ch.H, W, ch.n)
    s = ch.lo + 500
    h_acc = len(ch.head_from(s))
    for b in (0, 31, 32, 8160, 8175, n_blocks - 1):
        if view.offs[b + 1] == view.offs[b]:
            continue
        for A in (int(view.offs[b]) + 1, int(view.offs[b + 1])):      # the block's first and last accepted draw
            need0 = min(5, A - 1)
            k_core = A - need0
            r = run_both(eng, view, s, k_core + h_acc + need0, k_core, 300, 2)
            assert r["state"]["flags"] == 0 and r["state"]["accepted_used"] == A
            assert (r["base"] - ch.H - 1) // B == b


@pytest.mark.parametrize("blk", [0, 2, 3])
def test_cut_words(eng, blk):
    """The stream cut on chosen words of a window block -- both sides of lane and wave borders of the eight-words-per-lane layout
    of 256 lanes (every 8 and every 512 words) and of the two-words one -- in the first block, an inner one and the last whole
    one, and on the window's very last word."""
    W = 4 * B + 9
    must = sorted({blk * B + w for w in CUT_WORDS} | {W - 1})
    ch = make(n_win=3000, W=W, win_must=must)
    win_at = np.flatnonzero((ch.words[ch.H:ch.H + W] >> np.uint32(ch.shift)) < ch.n)
    s = ch.lo + 4000
    h_acc = len(ch.head_from(s))
    for word in must:
        A = int(np.searchsorted(win_at, word)) + 1        # no duplicate: the A-th accepted draw is the last one consumed
        k_core = max(1, A - 50)
        r = run_both(eng, ch, s, A + h_acc, k_core, 400, 2)
        assert r["base"] == ch.H + word + 1 and r["state"]["accepted_used"] == A and r["state"]["flags"] == 0


@pytest.mark.parametrize("off", [0, 1, SNP_BLOCK - 1])
def test_the_cut_on_both_sides_of_an_snp_block_border(eng, off):
    """The sample ends on the last word of an 8192-word block (the SNP draws start on a block's first word: no partial block), on
    the first word of the next (one word masked) and one word in front of a border (a first block of one live word)."""
    lo, F, W = 37, 3 * B - 5, 5 * B + 9
    H = lo + F
    cut = (H // SNP_BLOCK + 1) * SNP_BLOCK + off           # absolute position behind the last word consumed
    word = cut - 1 - H
    assert 0 < word < W
    ch = make(n_win=3000, W=W, win_must=(word,))
    win_at = np.flatnonzero((ch.words[H:H + W] >> np.uint32(ch.shift)) < ch.n)
    A = int(np.searchsorted(win_at, word)) + 1
    for K2 in (1, 3000):
        r = run_both(eng, ch, ch.lo + 4000, A + len(ch.head_from(ch.lo + 4000)), A - 20, K2, 2)
        assert r["base"] == cut and r["state"]["pos"] == cut + 2 * K2


# ---------------------------------------------------------------------------------------------- the SNP draws
def test_where_the_last_snp_completes(eng, plain):
    """The K-th SNP completing in the partial first block, on a block's last word, on the next block's second word and in the
    window's last block (every uniform a transition: SNP j of the draws completes on word start + 2 j - 1)."""
    ch = plain
    for K in range(1800, 1820):                            # an SNP completes on a block's last word iff the start is even
        start = run_both(eng, ch, ch.lo + 700, K, 600, 1, 1)["base"]
        if start % 2 == 0:
            break
    assert start % 2 == 0
    in_first = (SNP_BLOCK - start % SNP_BLOCK) // 2
    assert in_first > 2
    border = (start // SNP_BLOCK + 1) * SNP_BLOCK
    K_border = (border - start) // 2                       # completes on word border - 1
    last_blk_first = ((start + ch.W2 - 1) // SNP_BLOCK) * SNP_BLOCK
    K_last = (last_blk_first - start) // 2 + 3
    assert start + 2 * K_last <= start + ch.W2
    for K2 in (1, in_first - 1, K_border, K_border + 1, K_last, ch.W2 // 2):
        r = run_both(eng, ch, ch.lo + 700, K, 600, K2, 2)
        assert r["state"]["pos"] == start + 2 * K2 and r["state"]["flags"] == 0


@pytest.mark.parametrize("ti_lim", [TI_NONE, TI_ALL, TI_2])
def test_transition_shares(eng, plain, ti_lim):
    """No transitions (every SNP runs the randbelow(2) loop), only transitions, and titv 2.0 -- three map tables."""
    for K2 in (1, 777, 4000):
        r = run_both(eng, plain, plain.lo + 700, 1800, 600, K2, 3, ti_lim=ti_lim)
        assert r["state"]["flags"] == 0 and r["state"]["pos"] >= r["base"] + 2 * K2


# ---------------------------------------------------------------------------------------------- flags
def test_every_way_to_the_sample_flag(eng, plain):
    ch = plain
    s = ch.lo + 700
    h_acc = len(ch.head_from(s))
    total = len(ch.acc)
    ok = run_both(eng, ch, s, 1800, 600, 500, 2)
    end = ok["base"]
    # the start in front of the interval and behind it
    run_both(eng, ch, ch.lo - 1, 1800, 600, 500, 2, expect_flag=FLAG_SAMPLE, check_ref=False)
    run_both(eng, ch, ch.H + 1, 1800, 600, 500, 2, expect_flag=FLAG_SAMPLE, check_ref=False)
    # more accepted draws in front of the anchor than the sample has room for
    run_both(eng, ch, s, 600 + h_acc - 1, 600, 500, 2, expect_flag=FLAG_SAMPLE, check_ref=False)
    run_both(eng, ch, s, 600 + h_acc, 600, 500, 2)
    # the window does not hold the core's share and the fringe's
    run_both(eng, ch, s, total + h_acc + 1, total - 10, 500, 2, expect_flag=FLAG_SAMPLE, check_ref=False)
    # a round asks for more draws than the window holds
    short = make(plant=lambda hv, wv: wv.__setitem__(slice(3380, 3440), wv[:60]))     # 60 duplicates, 50 draws left
    run_both(eng, short, s, 3450 + len(short.head_from(s)), 3300, 500, 2, expect_flag=FLAG_SAMPLE, check_ref=False)
    # the cut beyond the limit: clamped to it, flag raised, and the SNP draws start there -- one word short, and at the limit
    r = run_both(eng, ch, s, 1800, 600, 500, 2, pos_limit=end - 1, expect_flag=FLAG_SAMPLE)
    assert r["base"] == end - 1 and r["state"]["pos"] == end - 1 + 1000
    assert run_both(eng, ch, s, 1800, 600, 500, 2, pos_limit=end)["base"] == end
    # what the prep flagged reaches the chain's state; flags that are there already stay
    run_both(eng, ch, s, 1800, 600, 500, 2, core_flags=FLAG_SAMPLE, expect_flag=FLAG_SAMPLE)
    run_both(eng, ch, s, 1800, 600, 500, 2, head_flags=FLAG_SAMPLE, expect_flag=FLAG_SAMPLE)
    run_both(eng, ch, s, 1800, 600, 500, 2, state={"flags": FLAG_SNP}, expect_flag=FLAG_SNP)


def test_every_way_to_the_snp_flag(eng, plain):
    ch = plain
    s = ch.lo + 700
    ok = run_both(eng, ch, s, 1800, 600, 500, 2)
    end = ok["state"]["pos"]
    # fewer than K SNPs complete in the window's blocks (two words each; the scan counts the last block to its end)
    off = ok["base"] % SNP_BLOCK
    nb = min(ch.W2 // SNP_BLOCK + 2, (off + ch.W2 + SNP_BLOCK - 1) // SNP_BLOCK)
    run_both(eng, ch, s, 1800, 600, (nb * SNP_BLOCK - off) // 2 + 1, 2, expect_flag=FLAG_SNP)
    # the draws end beyond the host's bound
    run_both(eng, ch, s, 1800, 600, 500, 2, snp_limit=end - 1, expect_flag=FLAG_SNP)
    assert run_both(eng, ch, s, 1800, 600, 500, 2, snp_limit=end)["state"]["pos"] == end


def test_the_margin_used(eng, plain):
    """|start - expected start| in permille of the half-width the host allowed (telemetry; a maximum over the session)."""
    ch = plain
    expect = ch.lo + ch.F // 2
    r = run_both(eng, ch, ch.lo + 700, 1800, 600, 500, 2, soft_half=2000)
    assert r["state"]["margin"] == 1000 * abs(ch.lo + 700 - expect) // 2000
    assert run_both(eng, ch, ch.lo + 700, 1800, 600, 500, 2, soft_half=2000, state={"margin": 999_999})["state"]["margin"] == 999_999


# ---------------------------------------------------------------------------------------------- refusals
def test_refuses_what_it_cannot_run(eng, plain):
    ch = plain
    k_core, K = 600, 1800
    bitmap, dups = tr.bitmap_of(ch.acc[:k_core], ch.n)
    ok = dict(words=ch.raw, ti_lim=TI_ALL, lo=ch.lo, F=ch.F, hcnt=ch.hcnt, hacc=ch.hacc, tail=ch.acc[k_core:], cnt=ch.cnt, bitmap=bitmap,
              state={"pos": ch.lo + 5, "snp_base": ch.lo + 5}, K=K, k_core=k_core, shift=ch.shift, n=ch.n, W=ch.W, W2=ch.W2, K2=100,
              G=2, fused=True, core_dups=dups)
    eng.chain_step(**ok)
    wrong_count = ch.hcnt.copy()
    wrong_count[1] += 1
    for bad in (dict(G=0), dict(G=257), dict(shift=32), dict(K2=0), dict(k_core=K + 1), dict(words=ch.raw[:-2 * SNP_BLOCK]),
                dict(W2=ch.W2 + 2 * SNP_BLOCK), dict(hcnt=wrong_count), dict(hacc=ch.hacc[:-1]), dict(tail=ch.acc[k_core:k_core + 100]),
                dict(tail=np.where(np.arange(len(ch.acc) - k_core) == 3, ch.n, ch.acc[k_core:])),
                dict(state={"pos": ch.lo, "snp_base": ch.H + ch.W + 1}), dict(lo=len(ch.raw))):
        for fused in (True, False):
            with pytest.raises(_ffi.MsimError):
                eng.chain_step(**{**ok, **bad, "fused": fused})
