"""A word-level restatement of what the SNP sampler decides, independent of libmsim: ``random.sample``'s set path,
``random.random`` / ``randint(0, 1)`` and ``sample_with_minimum_distance`` (util.py:94-109) over an EXPLICIT array of
tempered MT19937 words and a start index.  The words come from CPython's own generator (``random.Random(seed)``), never from
``mt19937.h``; ``tests/test_steered_seeds_host.py`` holds every function here against ``random.sample`` / ``random.random``
themselves and against the host planner.

Because every draw is an index into one array, the restatement can say WHERE things happen: the word that holds the final
accepted draw of a sample, the word of the k-th accepted draw, the words of every SNP.  Those indices, taken relative to the
tilings the kernels use (the constants below), are the "events" of ``tests/golden/steered_seeds.json``: seeds and sample sizes
searched on the CPU so that the genuine stream puts a cut on the last word of a block, a retry loop across two blocks, ...

Plain Python; numpy only for the acceptance filter (``word >> shift < n``) and the record table."""
from __future__ import annotations

import random
from collections import namedtuple
from fractions import Fraction

import numpy as np

# the kernels' tilings (copied, with the symbol they copy)
MT_N = 624                    # mt19937.h MT_N: words [0, 624) of a session are the copied generator state
MT_CHUNK_WORDS = 159744       # mt_jump_table.h MT_CHUNK_WORDS: generated chunk c holds words [624 + c * 159744, ...)
ACC_BLOCK = 2048              # plan_kernels.h ACC_BLOCK: count block of a sample window (k_accept_count, k_sample_tail's cut)
SPL_BLOCK = 8192              # plan_kernels.h SPL_BLOCK: scatter block of a sample window (k_bin_scatter)
SNP_BLOCK2 = 8192             # plan_kernels.h SNP_BLOCK2: ABSOLUTE transducer block (k_snp_maps_abs, k_snp_scan_cut_abs)
SNP_LANE = 32                 # plan_kernels.h SNP_ITEMS2: words of one lane inside a transducer block
BIN_VALUES = 1 << 20          # plan_kernels.h BIN_VALUES: values per de-dup bin (k_bin_scatter, k_bin_dedupe)
BITMAP_WORD = 64              # plan_kernels.h k_bitmap_count / k_bitmap_expand: values per 64-bit bitmap word
EXPAND_BLOCK = 64 * 256       # plan_kernels.h BM_THREADS bitmap words per expansion block
TAIL_LDS_OFFS = 8192          # plan_kernels.h TAIL_LDS_OFFS: count blocks k_sample_tail holds in LDS
SN = 1                        # include/msim.h MSIM_SN

RECORD_DTYPE = np.dtype([("pos", "<u4"), ("stop", "<u4"), ("extra", "<u4"), ("type", "u1"), ("aux", "u1"), ("rsv", "<u2")])


# ------------------------------------------------------------------------------------------------ the stream
def make_stream(seed: int, skip: int, count: int):
    """``random.Random(seed)`` after ``skip`` 32-bit outputs: (words, p, mt) -- ``mt`` the 624 state words and ``p`` the state's
    index as ``getstate()`` reports them (what the engine is handed), ``words[p + i]`` the generator's i-th next output for
    i < count.  Entries below ``p`` are outputs already consumed (zero here: nothing may read them).  skip = 0: the freshly
    seeded state, index 624."""
    r = random.Random(seed)
    for _ in range(skip):
        r.getrandbits(32)
    st = r.getstate()[1]
    mt, p = np.array(st[:MT_N], dtype=np.uint32), int(st[MT_N])
    big = r.getrandbits(32 * count)                      # (CPython fills the integer from its low word up: word i = bits 32 i ..)
    out = np.frombuffer(big.to_bytes(4 * count, "little"), dtype="<u4")
    words = np.zeros(p + count, dtype=np.uint32)
    words[p:] = out
    return words, p, mt


def next_words(mt, pos, n=8):
    """The next ``n`` outputs of the generator whose state is (mt, pos)."""
    r = random.Random()
    r.setstate((3, tuple(int(x) for x in mt) + (int(pos),), None))
    return [r.getrandbits(32) for _ in range(n)]


# ------------------------------------------------------------------------------------------------ random.py
def randbelow(words, p, n):
    """``_randbelow_with_getrandbits`` (n < 2**32): (value, index behind the accepted word)."""
    bits = n.bit_length()
    v = int(words[p]) >> (32 - bits)
    p += 1
    while v >= n:
        v = int(words[p]) >> (32 - bits)
        p += 1
    return v, p


SamplePath = namedtuple("SamplePath", "values cut kth_word dups rounds reject_run acc_idx acc_val consumed")


def sample_set_path(words, p, n, k) -> SamplePath:
    """The set path of ``random.sample(range(n), k)`` from word ``p`` on.

    values: the selected values in draw order; cut[j]: the word index behind the j-th distinct value (cut[0] = p, cut[k] where
    the sample ends); kth_word: the word of the k-th ACCEPTED draw, before any replacement; dups: accepted draws that were
    duplicates; rounds: tail rounds, round r drawing as many replacements as round r-1 found duplicates (round 0: the first k
    accepted draws); reject_run: rejected words directly in front of the final accepted draw; acc_idx / acc_val: word index
    and value of every accepted draw the sample consumed (``consumed`` of them)."""
    bits = n.bit_length()
    v = np.asarray(words[p:]) >> np.uint32(32 - bits)    # getrandbits(bits) of every word
    idx = np.flatnonzero(v < n)                          # the acceptance filter: retry while r >= n
    acc_idx, acc_val = (idx + p).tolist(), v[idx].tolist()
    selected, values, cut = set(), [], [p]
    a = 0
    while len(values) < k:
        j = acc_val[a]
        if j not in selected:
            selected.add(j)
            values.append(j)
            cut.append(acc_idx[a] + 1)
        a += 1
    consumed = a
    # the same sample as rounds over the accepted draws
    seen = set(acc_val[:k])
    need, at, rounds = k - len(seen), k, 0
    while need:
        rounds += 1
        d = 0
        for j in acc_val[at:at + need]:
            if j in seen:
                d += 1
            seen.add(j)
        at, need = at + need, d
    assert at == consumed and seen == selected
    last = acc_idx[consumed - 1]
    before = acc_idx[consumed - 2] if consumed > 1 else p - 1
    return SamplePath(values, cut, acc_idx[k - 1], consumed - k, rounds, last - max(before, p - 1) - 1,
                      acc_idx[:consumed], acc_val[:consumed], consumed)


def ti_lim_of(titv: float) -> int:
    """The integer the transition compare uses: ``p <= p_ti`` with p = u / 2**53 is ``u < floor(p_ti * 2**53) + 1`` (at most
    2**53: every u); a NaN p_ti compares false with everything.  mutator.py:436-438."""
    p_ti = titv * (1 / (titv + 1))
    if p_ti != p_ti:
        return 0
    if p_ti >= 1.0:
        return 1 << 53
    f = Fraction(p_ti) * (1 << 53)
    return min(f.numerator // f.denominator + 1, 1 << 53)


SnpDraws = namedtuple("SnpDraws", "aux end spans")


def snp_draws(words, p, K, ti_lim) -> SnpDraws:
    """K SNP outcomes from word ``p``: ``random()`` = (a >> 5) * 2**26 + (b >> 6) over two words, a transition (aux 0) iff it is
    below ``ti_lim``; else ``randint(0, 1)`` = ``_randbelow(2)``: 2-bit draws until one is < 2, aux = 1 + that column.
    spans[i] = (first word, index behind the last word) of SNP i."""
    aux, spans = bytearray(K), []
    for i in range(K):
        s = p
        u = ((int(words[p]) >> 5) << 26) + (int(words[p + 1]) >> 6)
        p += 2
        if u >= ti_lim:
            c, p = randbelow(words, p, 2)
            aux[i] = 1 + c
        spans.append((s, p))
    return SnpDraws(bytes(aux), p, spans)


ContigPlan = namedtuple("ContigPlan", "recs end samples snp")


def plan_snp_contig(words, p, ranges, d, ti_lim) -> ContigPlan:
    """One SNP-only contig: per drawing range (start, stop, k) in order ``sample_with_minimum_distance`` -- the sample of
    range(start, stop - (k - 1) d), sorted, rank r moved up by d r -- then the outcomes of all SNPs in position order.
    Returns the 16-byte record table, the stream index behind the contig, every range's SamplePath and the SnpDraws."""
    pos, samples = [], []
    for start, stop, k in ranges:
        if k == 0:
            continue
        n = (stop - (k - 1) * d) - start
        sp = sample_set_path(words, p, n, k)
        samples.append(sp)
        p = sp.cut[k]
        pos += [start + v + d * r for r, v in enumerate(sorted(sp.values))]
    K = len(pos)
    sd = snp_draws(words, p, K, ti_lim)
    recs = np.zeros(K, dtype=RECORD_DTYPE)
    recs["pos"] = recs["stop"] = np.array(pos, dtype=np.uint32)
    recs["type"] = SN
    recs["aux"] = np.frombuffer(sd.aux, dtype=np.uint8)
    return ContigPlan(recs, sd.end, samples, sd)


def plan_chain(words, p, contigs, d, ti_lim):
    """Contigs (each a list of ranges) one behind the other on one stream: the list of ContigPlan."""
    out = []
    for ranges in contigs:
        cp = plan_snp_contig(words, p, ranges, d, ti_lim)
        out.append(cp)
        p = cp.end
    return out


def words_needed(contigs, d, ti_lim) -> int:
    """A generous bound of the words a chain consumes (twice the expectation + slack), to size ``make_stream``."""
    total = 0
    p_tv = 1.0 - min(1.0, ti_lim / float(1 << 53))
    for ranges in contigs:
        for start, stop, k in ranges:
            n = (stop - (k - 1) * d) - start
            total += int(2.5 * k * (1 << n.bit_length()) / n * (1.0 + k / n)) + 65536
            total += int(k * (2 + 2 * p_tv) * 1.5) + 65536
    return total


# ------------------------------------------------------------------------------------------------ events
def _snp_retries(words, span):
    """Rejected 2-bit draws of an SNP's randbelow(2) loop (0 for a transition: it has no third word)."""
    return max(0, span[1] - span[0] - 3)


def facts(words, plans, target):
    """What the events are predicates of, for the steered contig ``target`` = (contig, range) of a planned chain."""
    ci, ri = target
    cp = plans[ci]
    sp = cp.samples[ri]
    k = len(sp.values)
    s = sp.cut[0]
    spans = cp.snp.spans
    return {
        "s": s, "cut": sp.cut[k], "cut_word": sp.cut[k] - 1, "kth_word": sp.kth_word, "dups": sp.dups, "rounds": sp.rounds,
        "reject_run": sp.reject_run, "snp_start": spans[0][0], "snp_end": cp.end, "k": k,
        "min_value": min(sp.values), "max_value": max(sp.values),
    }


def _count(sp, value):
    return sp.acc_val.count(value)


def check_event(event: dict, words, plans, target, ranges_of_target, d) -> None:
    """Assert that the planned chain produces ``event`` (``kind`` + the word indices / values it claims)."""
    ci, ri = target
    cp, sp = plans[ci], plans[ci].samples[ri]
    f = facts(words, plans, target)
    start, stop, k = ranges_of_target[ri]
    n = (stop - (k - 1) * d) - start
    kind = event["kind"]
    for key in ("s", "cut", "kth_word", "snp_start", "snp_end"):
        if key in event:
            assert event[key] == f[key], (kind, key, event[key], f[key])
    rel = f["cut_word"] - f["s"]
    spans = cp.snp.spans
    if kind == "cut_word_in_count_block":                 # 1: word 2047 of a count block / word 0 of the next
        assert rel % ACC_BLOCK == event["word"] and event["word"] in (ACC_BLOCK - 1, 0) and rel >= ACC_BLOCK
    elif kind == "cut_word_in_scatter_block":
        assert rel % SPL_BLOCK == event["word"] and event["word"] in (SPL_BLOCK - 1, 0) and rel >= SPL_BLOCK
    elif kind == "kth_accept_in_count_block":             # 2: the first-k / tail split on a block edge (and a tail to split off)
        assert (f["kth_word"] - f["s"]) % ACC_BLOCK == event["word"] and event["word"] in (ACC_BLOCK - 1, 0)
        assert f["dups"] >= 1
    elif kind == "no_duplicate":                          # 3
        assert f["dups"] == 0 and f["rounds"] == 0
    elif kind == "one_duplicate_redrawn_duplicate":       # 4
        assert f["dups"] == 2 and f["rounds"] == 2
    elif kind == "many_tail_rounds":                      # 5
        assert f["rounds"] >= 4 and f["rounds"] == event["rounds"]
    elif kind == "rejects_before_cut":                    # 6
        assert n & (n - 1) == 0 and f["reject_run"] >= 12 and f["reject_run"] == event["reject_run"]
    elif kind == "starts_in_copied_state_words":          # 7 (as reachable): the sample starts below 624 and ends beyond
        assert f["s"] == event["state_index"] < MT_N < f["cut"]
    elif kind == "sample_ends_at":                        # 8
        assert f["cut"] == event["at"]
    elif kind == "snp_ends_at":
        assert f["snp_end"] == event["at"]
    elif kind == "first_and_last_value":                  # 9
        assert f["min_value"] == 0 and f["max_value"] == n - 1
        # the records reach both ends of what util.py:104 can draw: start and stop - 1 ("cannot be 0 or n")
        assert (ri > 0 or cp.recs["pos"][0] == start) and cp.recs["pos"][-1] == stop - 1
    elif kind == "bin_border_values_with_duplicates":     # 10
        assert _count(sp, BIN_VALUES - 1) >= 2 and _count(sp, BIN_VALUES) >= 2
    elif kind == "last_value_of_n":                       # 11, 12
        assert n == event["n"] and f["max_value"] == n - 1
        if "mod" in event:
            m, r = event["mod"]
            assert n % m == r % m
    elif kind == "snp_start_in_block":                    # 13
        assert f["snp_start"] % SNP_BLOCK2 == event["word"] and event["word"] in (0, SNP_BLOCK2 - 1)
    elif kind == "snp_last_word_in_block":                # 14, 17
        assert (f["snp_end"] - 1) % SNP_BLOCK2 == event["word"] and event["word"] in (0, SNP_BLOCK2 - 1)
        if "all" in event:
            want = 0 if event["all"] == "transitions" else None
            assert all((a == 0) if want == 0 else (a != 0) for a in cp.snp.aux)
    elif kind == "random_straddles":                      # 15: the two words of a random() on both sides of a border
        a = event["first_word"]
        assert any(sn[0] == a for sn in spans) and (a + 1) % event["border"] == 0 and event["border"] in (SNP_BLOCK2, SNP_LANE)
        if event["border"] == SNP_LANE:
            assert (a + 1) % SNP_BLOCK2 != 0
    elif kind == "retry_loop_straddles_block":            # 16a: rejected draw(s) on one side, the loop's end on the other
        i = event["snp"]
        a, b = spans[i]
        assert _snp_retries(words, spans[i]) >= 1 and cp.snp.aux[i] != 0
        assert (a + 2) // SNP_BLOCK2 < (b - 1) // SNP_BLOCK2
    elif kind == "long_retry_loop":                       # 16b
        i = event["snp"]
        assert _snp_retries(words, spans[i]) >= 10 and _snp_retries(words, spans[i]) == event["retries"]
    elif kind == "last_snp_ends_in_retry_loop":           # 16c
        assert cp.snp.aux[-1] != 0 and _snp_retries(words, spans[-1]) >= 2
    elif kind == "head_duplicate_pair":                   # 18: both draws within 32 words behind the exact start
        a, b = event["words"]
        ia, ib = sp.acc_idx.index(a), sp.acc_idx.index(b)
        assert f["s"] <= a < b < f["s"] + 32 and sp.acc_val[ia] == sp.acc_val[ib] and ci >= 1
    elif kind == "head_value_redrawn_late":               # 19
        a, b = event["words"]
        ia, ib = sp.acc_idx.index(a), sp.acc_idx.index(b)
        assert f["s"] <= a < f["s"] + 32 and sp.acc_val[ia] == sp.acc_val[ib] and ci >= 1
        assert ib >= k // 2 and ib < (3 * k) // 4         # late, and inside every core (k - a_max > 3 k / 4 for these cases)
    else:
        raise AssertionError(f"unknown event kind {kind!r}")


# ------------------------------------------------------------------------------------------------ the fixture
def load_cases():
    """``tests/golden/steered_seeds.json``: per case the seed pair, the state index (``skip`` outputs already consumed), d, the
    titv argument, the contigs of the chain (L and their ranges as [start, stop, k]), the steered (contig, range) and the
    event it claims."""
    import json
    from pathlib import Path
    return json.loads((Path(__file__).resolve().parent / "golden" / "steered_seeds.json").read_text())


def case_contigs(case):
    return [[tuple(r) for r in c["ranges"]] for c in case["contigs"]]


def plan_case(case):
    """(words, p, mt, [ContigPlan]) of a fixture case, from its seed."""
    ti_lim = ti_lim_of(case["titv"])
    contigs = case_contigs(case)
    words, p, mt = make_stream(case["seed"][0], case["skip"], words_needed(contigs, case["d"], ti_lim))
    return words, p, mt, plan_chain(words, p, contigs, case["d"], ti_lim)


def numpy_stream(seed: int, words_consumed: int):
    """The legacy NumPy generator the type draws come from (``numpy.random.choice``: two words per candidate): the state
    handed to the engine as (mt, index) and the 8 outputs that follow ``words_consumed`` words."""
    rs = np.random.RandomState(seed)
    st = rs.get_state()
    mt, pos = np.array(st[1], dtype=np.uint32), int(st[2])
    rs.bytes(4 * words_consumed)
    return mt, pos, np.frombuffer(rs.bytes(32), dtype="<u4").tolist()
