"""CPU tier: ``tests/snp_ref.py`` against CPython's own generator, and the hand-built cases of ``tests/snp_cases.py`` against what
they claim to hit."""
from __future__ import annotations

import random

import numpy as np
import pytest

import snp_cases
import snp_ref as R
import stream_ref as S

CASES = snp_cases.build()


@pytest.mark.parametrize("seed,titv,K", [(7, 2.0, 4000), (8, 0.5, 3000), (9, 1e9, 2000), (10, 0.0, 2000)])
def test_walk_is_cpythons_draws(seed, titv, K):
    """The words as ``getrandbits(32)`` hands them out from a saved state; from the same state the reference's own sequence of
    ``random() <= p_ti`` / ``randint(0, 1)`` for K SNPs (mutator.py:436-446): outcomes and words consumed must agree."""
    r = random.Random(seed)
    for _ in range(seed * 13):
        r.getrandbits(32)
    state = r.getstate()
    n = 2 * R.BLOCK + 100
    t = np.array([r.getrandbits(32) for _ in range(n)], dtype=np.uint32)
    r.setstate(state)
    p_ti = titv * (1 / (titv + 1))
    want = bytearray()
    for _ in range(K):
        if r.random() <= p_ti:
            want.append(0)
        else:
            want.append(1 + r.randint(0, 1))
    nxt = r.getrandbits(32)
    ti_lim = S.ti_lim_of(titv)
    aux, end, flags = R.draws(t, ti_lim, 0, K)
    assert flags == 0 and aux == bytes(want)
    assert int(t[end]) == nxt                              # the same number of words consumed
    sd = S.snp_draws(t, 0, K, ti_lim)                      # ... and the SNP-by-SNP restatement agrees
    assert sd.aux == aux and sd.end == end
    # the block and lane maps say the same: composing the lanes' maps from state 0 counts every SNP of the whole blocks
    lanes, maps = R.block_tables(t, ti_lim)
    s, total = 0, 0
    for b in range(maps.shape[0]):
        total += int(maps[b, s])
        s = (int(maps[b, 3]) >> (2 * s)) & 3
    assert total == len(R.completions(t, ti_lim, 0))


def test_tempering_and_its_inverse():
    words, p, mt = S.make_stream(5, 1, 600)                # one output taken: the state is twisted, outputs 1.. are its words tempered
    assert np.array_equal(R.temper(mt[p:p + 600 - 1]), words[p:p + 600 - 1])
    t = np.random.RandomState(3).randint(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)
    t[:4] = (0, 0xFFFFFFFF, 0x80000000, 1)
    assert np.array_equal(R.temper(R.untemper(t)), t)
    a, b = R.pair_words(snp_cases.TI23)
    assert ((a >> 5) << 26) | (b >> 6) == snp_cases.TI23


def test_cases_hit_what_they_claim():
    done = lambda name: R.completions(*[CASES[name][i] for i in (0, 1, 2)])
    t, ti_lim, start, K, _ = CASES["zeros_last_on_word_8191"]
    assert done("zeros_last_on_word_8191")[K - 1] == R.BLOCK - 1
    t, ti_lim, start, K, _ = CASES["zeros_odd_start_last_on_word_0"]
    assert done("zeros_odd_start_last_on_word_0")[K - 1] == R.BLOCK
    per_block = lambda name, b: sum(1 for w in done(name) if w // R.BLOCK == b)
    assert per_block("zeros_three_full_blocks", 0) == 4096 and per_block("zeros_odd_start_block_of_4096", 1) == 4096
    assert per_block("block_completes_none", 1) == 0 and per_block("block_completes_none", 0) == 4094
    assert done("ones_loop_never_ends") == []
    for border in (32, 2048, 8192):
        for name, out in ((f"limit_below_border_{border}", 0), (f"limit_at_border_{border}", 2), (f"zero_at_border_{border}", 2)):
            t, ti_lim, start, K, _ = CASES[name]
            aux = R.draws(t, ti_lim, start, K)[0]
            sd = S.snp_draws(t, start, K, ti_lim)
            assert sd.aux == aux
            i = [s for s, _ in sd.spans].index(border - 1)  # an SNP's random() starts on the word before the border
            assert aux[i] == out, name
    t, ti_lim, start, K, _ = CASES["reject_across_lane_and_block"]
    spans = S.snp_draws(t, start, K, ti_lim).spans
    assert (28, 37) in spans and (8185, 8197) in spans
