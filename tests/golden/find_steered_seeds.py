"""Search (CPU only, deterministic) for the (seed, k) pairs of ``steered_seeds.json``: SNP-sampler inputs whose GENUINE MT19937
stream puts an event on an edge of the kernels' tilings -- the final accepted draw on the last word of a count block, a retry
loop across two transducer blocks, the last value of a partial bin, ...  (tests/stream_ref.py names the tilings and states
every event as a predicate; tests/test_steered_seeds_host.py proves each pair, tests/test_gpu_steered.py runs them.)

What keeps it cheap: on a fixed seed and a fixed population size n, ``sample(k + 1)`` is ``sample(k)`` plus one more distinct
draw, so ONE pass yields the cut for every k.  n is held fixed by moving ``stop`` with k, and k is chosen to hit the target
word; with n = 2**m - 1 nearly every word is accepted and the cut advances one word per step.  Seeds are walked only for
events that are not monotone in k (a duplicate pattern, a particular value drawn, a long run of rejected words).  Where the
SNP stage's end matters, its words are followed with a jump table (numpy, doubling) instead of SNP by SNP.

    python tests/golden/find_steered_seeds.py            # rewrites steered_seeds.json
    python tests/golden/find_steered_seeds.py --check    # regenerates and compares byte for byte
"""
from __future__ import annotations

import json
import sys
import time
from math import ceil, log
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import stream_ref as sr  # noqa: E402

OUT = HERE / "steered_seeds.json"
K_MIN = 4096                                   # below: the sampler declines the range (gpu_plan_eligible)
K_MAX = 60000                                  # the restatement stays well under a second
HANDOVER = sr.MT_N + sr.MT_CHUNK_WORDS         # first word of the second generated chunk


def setsize(k):
    return 21 + (4 ** ceil(log(k * 3, 4)) if k > 5 else 0)


def k_cap(n, kmax):
    """Largest k <= kmax whose sample of range(n) still takes the set path (n > setsize(k))."""
    while kmax > K_MIN and n <= setsize(kmax):
        kmax = min(kmax - 1, (4 ** (ceil(log(kmax * 3, 4)) - 1)) // 3)
    return kmax


class SnpJump:
    """next[i]: the word index behind an SNP whose draws start at word i; doubling tables give the index behind K SNPs."""

    def __init__(self, words, ti_lim):
        w = words.astype(np.uint64)
        N = len(w)
        u = ((w[:-1] >> np.uint64(5)) << np.uint64(26)) | (w[1:] >> np.uint64(6))
        trans = np.append(u < np.uint64(ti_lim) if ti_lim < (1 << 64) else np.ones(N - 1, bool), False)
        ok = (words >> np.uint32(31)) == 0
        idx = np.where(ok, np.arange(N), N)
        nxt_ok = np.append(np.minimum.accumulate(idx[::-1])[::-1], [N, N, N])
        i = np.arange(N)
        nxt = np.where(trans, i + 2, nxt_ok[i + 2] + 1)
        nxt = np.append(np.minimum(nxt, N), N)
        self.N, self.t = N, [nxt]

    def end(self, p, K):
        b = 0
        while K:
            if b >= len(self.t):
                self.t.append(self.t[-1][self.t[-1]])
            if K & 1:
                p = int(self.t[b][p])
            K >>= 1
            b += 1
        return p


class Ctx:
    """One seed's stream with everything in front of the steered range already planned."""

    def __init__(self, seed, skip, n_words, titv, d, prefix, first_ranges, n, kmax):
        self.words, self.p0, _ = sr.make_stream(seed, skip, n_words)
        self.ti_lim = sr.ti_lim_of(titv)
        self.d = d
        p = self.p0
        for cp in sr.plan_chain(self.words, p, prefix, d, self.ti_lim):
            p = cp.end
        self.k_other = 0
        for start, stop, k in first_ranges:
            sp = sr.sample_set_path(self.words, p, (stop - (k - 1) * d) - start, k)
            p = sp.cut[k]
            self.k_other += k
        self.s, self.n, self.kmax = p, n, kmax
        self.sp = sr.sample_set_path(self.words, p, n, kmax)
        self._jump = None
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    @property
    def jump(self):
        if self._jump is None:
            self._jump = SnpJump(self.words, self.ti_lim)
        return self._jump

    def snp_end(self, k):
        return self.jump.end(self.sp.cut[k], k + self.k_other)


def make_case(name, seed, skip, titv, d, prefix, first_ranges, start, n, k, event, tail=0):
    stop = start + n + (k - 1) * d
    contigs = [{"L": r[0][1] + 1, "ranges": [list(x) for x in r]} for r in prefix]
    contigs.append({"L": stop + 1 + tail, "ranges": [list(x) for x in first_ranges] + [[start, stop, k]]})
    return {"name": name, "seed": [seed, seed + 1], "skip": skip, "titv": titv, "d": d, "contigs": contigs,
            "target": [len(prefix), len(first_ranges)], "event": event}


def verify(case):
    """The plain restatement on the finished case: it produces the event, and the sampler takes the contig."""
    words, p, _, plans = plan_case(case)
    ci, ri = case["target"]
    sr.check_event(case["event"], words, plans, (ci, ri), [tuple(r) for r in case["contigs"][ci]["ranges"]], case["d"])
    for c in case["contigs"]:
        for start, stop, k in c["ranges"]:
            n = (stop - (k - 1) * case["d"]) - start
            assert k >= K_MIN and n > setsize(k) and c["L"] - k > setsize(k) and c["L"] > stop, case["name"]
    return case


plan_case = sr.plan_case


TWO_RANGE_FIRST = [(0, 32767 + 4096 - 1, 4096)]           # n = stop - (k - 1) = 2**15 - 1, k = 4096 in front of the steered range


def steer(name, pred, *, n, seed0, titv=2.0, d=1, skip=0, kmin=K_MIN, kmax=K_MAX, prefix=(), two_range=False, start=1000, tail=500,
          max_seeds=1000000, wanted=()):
    """First seed >= seed0 and smallest k in [kmin, kmax] for which ``pred(ctx, k)`` returns an event.  ``wanted``: (value,
    times) pairs the event needs among the draws -- seeds whose first words do not hold them are skipped after one numpy pass
    over a short stream (necessary, not sufficient: the predicate decides)."""
    kmax = k_cap(n, kmax)
    first = [tuple((a, b + (d - 1) * (k - 1), k)) for a, b, k in TWO_RANGE_FIRST] if two_range else []
    if two_range:
        start = first[-1][1] + 1 + start
    bits = n.bit_length()
    for seed in range(seed0, seed0 + max_seeds):
        if wanted:
            w, p0, _ = sr.make_stream(seed, skip, int(1.1 * kmax * (1 << bits) / n) + 8192)
            v = w[p0:] >> np.uint32(32 - bits)
            if any(np.count_nonzero(v == val) < times for val, times in wanted):
                continue
        need = int(2.2 * kmax * (1 << bits) / n * (1 + kmax / n)) + 6 * kmax + 200000 + sum(6 * r[2] + 70000 for c in prefix for r in c)
        ctx = Ctx(seed, skip, need, titv, d, list(prefix), first, n, kmax)
        for k in range(kmin, kmax + 1):
            ev = pred(ctx, k)
            if ev == "next seed":
                break
            if ev:
                return verify(make_case(name, seed, skip, titv, d, list(prefix), first, start, n, k, ev, tail))
    raise RuntimeError(f"{name}: no seed found")


# ------------------------------------------------------------------------------------------------ predicates
def cut_rel(block, word):
    kind = "cut_word_in_count_block" if block == sr.ACC_BLOCK else "cut_word_in_scatter_block"

    def pred(c, k):
        rel = c.sp.cut[k] - 1 - c.s
        if rel >= block and rel % block == word:
            return {"kind": kind, "word": word, "s": c.s, "cut": c.sp.cut[k]}
    return pred


def kth_rel(word):
    def pred(c, k):
        kth = c.sp.acc_idx[k - 1]
        if (kth - c.s) % sr.ACC_BLOCK == word and c.sp.cut[k] - 1 > kth:      # (a later cut word: at least one duplicate)
            return {"kind": "kth_accept_in_count_block", "word": word, "s": c.s, "kth_word": kth}
    return pred


def first_k_duplicates(c):
    """Accepted-draw ordinals (0-based) of the duplicate draws, in order."""
    seen, out = set(), []
    for i, v in enumerate(c.sp.acc_val):
        if v in seen:
            out.append(i)
        seen.add(v)
    return out


def no_duplicate(c, k):
    return {"kind": "no_duplicate", "s": c.s, "cut": c.sp.cut[k]} if c.sp.cut[k] - c.s == k else "next seed"


def one_dup_redup(c, k):
    dup = c.memo("dup", lambda: first_k_duplicates(c))
    # k = the ordinal of the second duplicate: the first k draws hold one duplicate, its replacement (draw k) is one again
    if len(dup) >= 3 and dup[1] >= K_MIN and dup[2] > dup[1] + 1 and k == dup[1]:
        return {"kind": "one_duplicate_redrawn_duplicate", "s": c.s, "cut": c.sp.cut[k]}
    return None if len(dup) >= 3 and dup[1] >= K_MIN and dup[2] > dup[1] + 1 and k < dup[1] else "next seed"


def many_rounds(c, k):
    sp = sr.sample_set_path(c.words, c.s, c.n, k)
    return {"kind": "many_tail_rounds", "rounds": sp.rounds, "cut": sp.cut[k]} if sp.rounds >= 4 else "next seed"


def rejects_before_cut(c, k):
    a = c.sp.cut[k] - 1
    j = a - 1
    while j >= c.s and (int(c.words[j]) >> (32 - c.n.bit_length())) >= c.n:
        j -= 1
    if a - 1 - j >= 12:
        return {"kind": "rejects_before_cut", "reject_run": a - 1 - j, "cut": a + 1}


def state_index(c, k):
    return {"kind": "starts_in_copied_state_words", "state_index": c.s, "s": c.s, "cut": c.sp.cut[k]}


def sample_ends_at(at):
    def pred(c, k):
        if c.sp.cut[k] == at:
            return {"kind": "sample_ends_at", "at": at, "cut": at}
        return "next seed" if c.sp.cut[k] > at else None
    return pred


def snp_ends_at(at):
    def pred(c, k):
        e = c.snp_end(k)
        if e == at:
            return {"kind": "snp_ends_at", "at": at, "snp_end": at}
        return "next seed" if e > at + 64 else None
    return pred


def first_and_last_value(c, k):
    vals = c.sp.values
    at = c.memo("at", lambda: 1 + max(vals.index(0), vals.index(c.n - 1)) if 0 in vals and c.n - 1 in vals else None)
    if at is None:
        return "next seed"
    if k >= at:
        return {"kind": "first_and_last_value", "cut": c.sp.cut[k]}


def bin_border_dups(c, k):
    def second_occurrences():
        X, Y = sr.BIN_VALUES - 1, sr.BIN_VALUES
        ix = [i for i, v in enumerate(c.sp.acc_val) if v == X]
        iy = [i for i, v in enumerate(c.sp.acc_val) if v == Y]
        return c.sp.acc_idx[max(ix[1], iy[1])] if len(ix) >= 2 and len(iy) >= 2 else None
    last = c.memo("last", second_occurrences)                                  # the word of the later second occurrence
    if last is None:
        return "next seed"
    if c.sp.cut[k] > last:
        return {"kind": "bin_border_values_with_duplicates", "cut": c.sp.cut[k]}


def last_value(mod=None):
    def pred(c, k):
        vals = c.sp.values
        at = c.memo("at", lambda: 1 + vals.index(c.n - 1) if c.n - 1 in vals else None)
        if at is None:
            return "next seed"
        if k >= at:
            ev = {"kind": "last_value_of_n", "n": c.n, "cut": c.sp.cut[k]}
            if mod:
                ev["mod"] = [mod, c.n % mod]
            return ev
    return pred


def snp_start(word):
    def pred(c, k):
        if c.sp.cut[k] % sr.SNP_BLOCK2 == word:
            return {"kind": "snp_start_in_block", "word": word, "snp_start": c.sp.cut[k]}
    return pred


def snp_last_word(word, all_=None):
    def pred(c, k):
        e = c.snp_end(k)
        if (e - 1) % sr.SNP_BLOCK2 == word and e // sr.SNP_BLOCK2 > c.sp.cut[k] // sr.SNP_BLOCK2:
            ev = {"kind": "snp_last_word_in_block", "word": word, "snp_end": e}
            if all_:
                ev["all"] = all_
            return ev
    return pred


def _spans(c, k):
    return sr.snp_draws(c.words, c.sp.cut[k], k + c.k_other, c.ti_lim)


def random_straddles(border):
    def pred(c, k):
        for a, b in _spans(c, k).spans:
            if (a + 1) % border == 0 and (border == sr.SNP_BLOCK2 or (a + 1) % sr.SNP_BLOCK2 != 0):
                return {"kind": "random_straddles", "border": border, "first_word": a}
    return pred


def retry_straddles(c, k):
    sd = _spans(c, k)
    for i, (a, b) in enumerate(sd.spans):
        if b - a > 3 and (a + 2) // sr.SNP_BLOCK2 < (b - 1) // sr.SNP_BLOCK2:
            return {"kind": "retry_loop_straddles_block", "snp": i}


def long_retry(c, k):
    sd = _spans(c, k)
    for i, (a, b) in enumerate(sd.spans):
        if b - a - 3 >= 10:
            return {"kind": "long_retry_loop", "snp": i, "retries": b - a - 3}


def last_in_retry(c, k):
    e = c.snp_end(k)
    b = c.jump.end(c.sp.cut[k], k + c.k_other - 1)
    if e - b - 3 >= 2:
        return {"kind": "last_snp_ends_in_retry_loop", "snp_end": e}


# ------------------------------------------------------------------------------------------------ anchored windows
N1, N2, K2 = (1 << 20) - 1, (1 << 17) - 1, 20000


def anchored(name, kind, seed0):
    """Second contig of a chain (planned ahead of the chain by default): the first contig's k moves the second sample's exact
    start s along the stream until the draws right behind s do what is wanted."""
    for seed in range(seed0, seed0 + 1000):
        words, p0, _ = sr.make_stream(seed, 0, 400000)
        ti_lim = sr.ti_lim_of(2.0)
        sp1 = sr.sample_set_path(words, p0, N1, K_MIN + 400)
        jump = SnpJump(words, ti_lim)
        shift = np.uint32(32 - N2.bit_length())
        for k1 in range(K_MIN, K_MIN + 400):
            s = jump.end(sp1.cut[k1], k1)
            head = [(s + i, int(words[s + i] >> shift)) for i in range(32) if int(words[s + i] >> shift) < N2]
            ev = None
            if kind == "head_duplicate_pair":
                seen = {}
                for w, v in head:
                    if v in seen:
                        ev = {"kind": kind, "words": [seen[v], w], "s": s}
                        break
                    seen[v] = w
            elif kind == "head_value_redrawn_late":
                sp = sr.sample_set_path(words, s, N2, K2)
                hv = {v: w for w, v in reversed(head)}
                for i in range(K2 // 2, (3 * K2) // 4):
                    if sp.acc_val[i] in hv:
                        ev = {"kind": kind, "words": [hv[sp.acc_val[i]], sp.acc_idx[i]], "s": s}
                        break
            if ev:
                prefix = [[(0, N1 + k1 - 1, k1)]]
                return verify(make_case(name, seed, 0, 2.0, 1, prefix, [], 1000, N2, K2, ev, 500))
    raise RuntimeError(f"{name}: no seed found")


# ------------------------------------------------------------------------------------------------ the table
M20, M22, M17 = (1 << 20) - 1, (1 << 22) - 1, (1 << 17) - 1
RECIPES = {}


SPECS = {}


def recipe(name, fn, **kw):
    SPECS[name] = (fn, kw)
    RECIPES[name] = lambda: fn(name, **kw) if fn is anchored else steer(name, fn, **kw)


# 1: the cut word on the edges of a count block / a scatter block of the window
recipe("cut_word_2047_of_count_block", cut_rel(sr.ACC_BLOCK, sr.ACC_BLOCK - 1), n=M20, seed0=101)
recipe("cut_word_0_of_count_block", cut_rel(sr.ACC_BLOCK, 0), n=M20, seed0=102)
recipe("cut_word_8191_of_scatter_block", cut_rel(sr.SPL_BLOCK, sr.SPL_BLOCK - 1), n=M20, seed0=103)
recipe("cut_word_0_of_scatter_block", cut_rel(sr.SPL_BLOCK, 0), n=M20, seed0=104, d=3)
# 2: the k-th accepted draw (first k into bins / ordered tail list) on the edges of a count block
recipe("kth_accept_2047_of_count_block", kth_rel(sr.ACC_BLOCK - 1), n=M20, seed0=201)
recipe("kth_accept_0_of_count_block", kth_rel(0), n=M20, seed0=202)
# 3-6: duplicate patterns, rejected words in front of the cut
recipe("no_duplicate", no_duplicate, n=M22, seed0=301, kmax=K_MIN)
recipe("one_duplicate_redrawn_duplicate", one_dup_redup, n=M22, seed0=401, kmax=12000)
recipe("many_tail_rounds", many_rounds, n=M17, seed0=501, kmin=21000, kmax=21000)
recipe("rejects_before_cut", rejects_before_cut, n=1 << 20, seed0=601)
# 7 (as reachable): the first sample of a context whose state index is below 624 starts in the copied state words
recipe("state_index_1", state_index, n=M20, seed0=701, skip=1, kmax=K_MIN)
recipe("state_index_623", state_index, n=M20, seed0=702, skip=623, kmax=K_MIN)
# 8: the sample / the SNP stage ends on the hand-over between two generated chunks (the one place k goes beyond 60 000)
for delta, tag in ((-1, "minus_1"), (0, "exact"), (1, "plus_1")):
    recipe(f"sample_ends_at_chunk_border_{tag}", sample_ends_at(HANDOVER + delta), n=M22, seed0=801, kmin=150000, kmax=160000)
    recipe(f"snp_stage_ends_at_chunk_border_{tag}", snp_ends_at(HANDOVER + delta), n=M20, seed0=851, kmin=30000, kmax=50000)
# 9-12: values and bitmap
recipe("first_and_last_value", first_and_last_value, n=M17, seed0=901, d=3, start=0, tail=0, kmax=21845, wanted=((0, 1), (M17 - 1, 1)))
recipe("bin_border_values_with_duplicates", bin_border_dups, n=(1 << 20) + 1, seed0=1001, kmax=150000, start=0, tail=0,
       wanted=((sr.BIN_VALUES - 1, 2), (sr.BIN_VALUES, 2)))
for i, n in enumerate([1 << 20, (1 << 20) + 1, (1 << 20) - 1, 3 << 20, (3 << 20) + 1, (3 << 20) - 1]):
    recipe(f"last_value_of_n_{n}", last_value(), n=n, seed0=1101 + 100 * i, start=0, tail=0, wanted=((n - 1, 1),))
for i, n in enumerate([147776, 147777, 147775]):                                # 64 * 2309 and its neighbours
    recipe(f"last_value_n_mod_64_{n % 64}", last_value(64), n=n, seed0=2701 + 100 * i, start=0, tail=0, kmax=21845,
           wanted=((n - 1, 1),))
for i, n in enumerate([147456, 147457, 147455]):                                # 64 * 256 * 9 and its neighbours
    recipe(f"last_value_n_mod_16384_{n % 16384}", last_value(16384), n=n, seed0=2001 + 100 * i, start=0, tail=0, kmax=21845,
           d=3 if i == 0 else 1, wanted=((n - 1, 1),))
# 13-17: the SNP transducer's absolute blocks
recipe("snp_start_word_0_of_block", snp_start(0), n=M20, seed0=1301)
recipe("snp_start_word_8191_of_block", snp_start(sr.SNP_BLOCK2 - 1), n=M20, seed0=1302)
recipe("snp_last_word_8191_of_block", snp_last_word(sr.SNP_BLOCK2 - 1), n=M20, seed0=1401)
recipe("snp_last_word_0_of_block", snp_last_word(0), n=M20, seed0=1402)
recipe("random_straddles_block", random_straddles(sr.SNP_BLOCK2), n=M20, seed0=1501, kmax=4200)
recipe("random_straddles_lane", random_straddles(sr.SNP_LANE), n=M20, seed0=1502, kmax=4200)
recipe("retry_loop_straddles_block", retry_straddles, n=M20, seed0=1601, kmax=4200, titv=0.5)
recipe("long_retry_loop", long_retry, n=M20, seed0=1602, kmax=4200, titv=0.5)
recipe("last_snp_ends_in_retry_loop", last_in_retry, n=M20, seed0=1603)
recipe("all_transitions_last_word_8191", snp_last_word(sr.SNP_BLOCK2 - 1, "transitions"), n=M20, seed0=1701, titv=1e300)
recipe("all_transitions_last_word_0", snp_last_word(0, "transitions"), n=M20, seed0=1702, titv=1e300)
recipe("all_transversions_last_word_8191", snp_last_word(sr.SNP_BLOCK2 - 1, "transversions"), n=M20, seed0=1703, titv=0.0)
recipe("all_transversions_last_word_0", snp_last_word(0, "transversions"), n=M20, seed0=1704, titv=0.0)
# 18, 19: anchored windows
recipe("head_duplicate_pair", anchored, kind="head_duplicate_pair", seed0=1801)
recipe("head_value_redrawn_late", anchored, kind="head_value_redrawn_late", seed0=1901)


# Every event once more with the steered range as the SECOND range of its contig: more than one drawing range takes the
# ungrouped expansion (k_bitmap_expand, the SNP outcomes patched into the records behind it).  The first range moves the
# stream, so each is searched again.  Not the state-index cases (their event is the context's FIRST sample) and not the
# anchored windows (only a contig with one drawing range is planned ahead of the chain).
for _name, (_fn, _kw) in list(SPECS.items()):
    if _fn is anchored or _name.startswith("state_index"):
        continue
    recipe("two_ranges_" + _name, _fn, **dict(_kw, seed0=_kw["seed0"] + 4000, two_range=True))


def build_case(name):
    return RECIPES[name]()


def dumps(cases):
    return json.dumps(cases, indent=1) + "\n"


def main(argv):
    t0 = time.time()
    cases = []
    for name in RECIPES:
        t = time.time()
        cases.append(build_case(name))
        print(f"{name}: seed {cases[-1]['seed'][0]}, k {cases[-1]['contigs'][-1]['ranges'][-1][2]}  ({time.time() - t:.1f} s)", flush=True)
    text = dumps(cases)
    if "--check" in argv:
        assert OUT.read_text() == text, "steered_seeds.json is not what the search regenerates"
        print(f"identical ({time.time() - t0:.0f} s)")
    else:
        OUT.write_text(text)
        print(f"{len(cases)} cases, {len(text)} bytes, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main(sys.argv[1:])
