"""Hand-built TEMPERED word arrays for the SNP transducer's kernels (tests/test_gpu_snp_transducer_words.py runs them through
``Engine.snp_draws`` after the inverse tempering; tests/test_snp_ref_host.py checks on the CPU that they hit what they claim).
A case: name -> (tempered words, ti_lim, start, K, aux_off).  Two or three blocks of 8192 words and a ragged tail of 100 that
no pass may map."""
from __future__ import annotations

import numpy as np

import snp_ref as R
from stream_ref import ti_lim_of

TAIL = 100
ALL = 1 << 53                 # ti_lim: every sample is a transition
TI23 = ti_lim_of(2.0)         # -titv 2.0: 2**53 * 2 / 3, rounded as the product rounds it
ACCEPT_T1 = 0x40000000        # ends a randbelow(2) loop with column 1 (outcome 2)
REJECT = 0xC0000000           # a 2-bit draw >= 2
ONES = 0xFFFFFFFF


def _blank(blocks: int, fill: int = 0):
    return np.full(blocks * R.BLOCK + TAIL, fill, dtype=np.uint32)


def _mix(blocks: int, seed: int):
    return np.random.RandomState(seed).randint(0, 1 << 32, size=blocks * R.BLOCK + TAIL, dtype=np.uint64).astype(np.uint32)


def _pair(t, first: int, u: int):
    t[first], t[first + 1] = R.pair_words(u)


def build():
    cases = {}
    # tempered 0 everywhere: every sample is 0 -- a transition unless ti_lim is 0 -- and every 2-bit draw is accepted
    cases["zeros_three_full_blocks"] = (_blank(3), TI23, 0, 3 * 4096, 0)       # 4096 SNPs per block: the most a block completes
    cases["zeros_last_on_word_8191"] = (_blank(3), TI23, 0, 4096, 1)           # ends on a block's last word
    # from an odd start every random() straddles: words 31|32, 2047|2048, 8191|8192; the last SNP completes on word 0 of block 1
    cases["zeros_odd_start_last_on_word_0"] = (_blank(3), TI23, 1, 4096, 3)
    cases["zeros_odd_start_block_of_4096"] = (_blank(3), TI23, 1, 4095 + 4096 + 17, 15)   # block 1 completes 4096 from state 1
    cases["zeros_ti_lim_0"] = (_blank(3), 0, 0, 5000, 15)                      # no transition at all: three words per SNP
    cases["ones_ti_lim_all"] = (_blank(3, ONES), ALL, 5, 8000, 16)             # sample 2**53 - 1 == ti_lim - 1; start inside a lane
    cases["ones_loop_never_ends"] = (_blank(2, ONES), TI23, 0, 1, 17)          # no block completes an SNP: overflow
    # the sample on a straddling pair exactly at and one below the limit, on a lane, a wave and a block border
    for border in (32, 2048, 8192):
        for delta in (-1, 0):
            t = _blank(3)
            _pair(t, border - 1, TI23 + delta)
            t[border + 1] = ACCEPT_T1                                          # (delta 0: a transversion, column 1)
            cases[f"limit_{'below' if delta else 'at'}_border_{border}"] = (t, TI23, 1, 6000, (border // 32 + delta) % 18)
        t = _blank(3)
        _pair(t, border - 1, ALL - 1)
        cases[f"all_below_border_{border}"] = (t, ALL, 1, 6000, 0)
        t = _blank(3)                                                          # ti_lim 0: sample 0 == ti_lim, SNPs every 3 words
        t[border + 1] = ACCEPT_T1
        cases[f"zero_at_border_{border}"] = (t, 0, (border - 1) % 3, 4000, 16)
    # randbelow(2) loops that reject across a lane border (words 30..35) and across a block border (8187..8195)
    t = _blank(3)
    _pair(t, 28, ALL - 1)
    t[30:36] = REJECT
    t[36] = ACCEPT_T1
    _pair(t, 8185, ALL - 1)                                                    # (SNPs start on odd words behind word 36)
    t[8187:8196] = REJECT
    cases["reject_across_lane_and_block"] = (t, TI23, 0, 7000, 1)
    # ... and through a whole block: block 1 completes nothing, its run is empty
    t = _blank(3)
    _pair(t, 8189, ALL - 1)
    t[8191:2 * 8192 + 5] = REJECT
    t[2 * 8192 + 5] = ACCEPT_T1
    cases["block_completes_none"] = (t, TI23, 1, 4094 + 1 + 17, 3)
    # the genuine mix: start on a lane's first word, on a block's last word
    cases["mix_start_on_lane"] = (_mix(3, 11), TI23, 64, 3000, 3)
    t = _mix(3, 12)
    cases["mix_start_on_block_last_word"] = (t, TI23, 8191, len(R.completions(t, TI23, 8191)) - 7, 17)
    t = _mix(2, 13)
    cases["mix_every_snp_there_is"] = (t, TI23, 0, len(R.completions(t, TI23, 0)), 0)
    return cases


def alignment_sweep():
    """One block of the mix; outcome runs whose first byte sits at offsets 0, 1, 3, 15, 16, 17 and whose length is 1, 15, 16, 17
    (an empty run: block_completes_none, ones_loop_never_ends and every block behind the last SNP)."""
    t = _mix(1, 14)
    return t, TI23, [(off, K) for off in (0, 1, 3, 15, 16, 17) for K in (1, 15, 16, 17)]
