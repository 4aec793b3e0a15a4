"""The SNP sampler's emission train (plan_kernels.h: k_snp_emit_count_b's popcounts, k_bitmap_expand_tiles_b; the six-launch
train's k_bitmap_count_b, k_scan_u32_b, k_bitmap_expand_b) on bitmaps the sampler never produces, through
``Engine.emit_train`` (msim_dbg_emit_train: the launch code of an emission group on the caller's bitmaps).

What has to hold, against numpy: the record of the bit at value v with r bits in front of it is pos = stop = start + v + d r,
type SN, aux = aux8[r], everything else zero; first[t] = (number of records with pos <= t * tile) - 1 for t = 0 .. n_tiles --
what k_tile_index finds on the finished table; and both trains give the same bytes.

The bitmaps sit on the kernels' own borders: an expansion block is B = 2048 words (EX_WORDS), a super-block S = 4 blocks
(EMIT_SUPER), the staging buffer takes 2048 records a round (EX_STAGE: a block of all-ones words holds 64 times that)."""
from __future__ import annotations

import numpy as np
import pytest

from mutation_simulator_amd import _ffi

pytestmark = pytest.mark.gpu

B = 2048                 # words per expansion block
S = 4 * B                # ... per super-block
TILE = 16384
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _random(words, density, seed):
    rs = np.random.RandomState(seed)
    bits = (rs.random_sample(words * 64) < density).astype(np.uint8)
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def _zeros(words):
    return np.zeros(words, dtype=np.uint64)


def _with_bits(words, bits):
    bm = _zeros(words)
    for v in bits:
        bm[v // 64] |= np.uint64(1) << np.uint64(v % 64)
    return bm


def _ones_between_empty_blocks():
    bm = _zeros(3 * B)
    bm[B:2 * B] = ONES
    return bm


def _long_empty_runs():
    """Bits in the first word, one block in the middle and the last word; more than a super-block of empty blocks between."""
    n = 2 * S + 2 * B + 5
    bm = _zeros(n)
    bm[0] = np.uint64(0x8000000000000001)
    bm[S + B + 7:S + B + 40] = _random(33, 0.3, 5)
    bm[n - 1] = np.uint64(0x8000000000000000)
    return bm


# name -> (bitmap, start, room behind the last possible position: the contig's length is made from it)
def _bitmaps():
    out = {
        "one_word": (_random(1, 0.3, 1), 0, 9),
        "bit0_only": (_with_bits(B + 1, [0]), 0, 0),
        "last_bit_only": (_with_bits(B + 1, [(B + 1) * 64 - 1]), 0, 1),
        "empty": (_zeros(3), 0, 0),
        "empty_super": (_zeros(S + 1), 17, 40_000),
        "ones_block": (_ones_between_empty_blocks(), 0, 5),
        "empty_runs": (_long_empty_runs(), 3, 100),
        "r1pct_4M": (_random(1 << 16, 0.01, 2), 0, 77),
        "r30pct_4M": (_random(1 << 16, 0.30, 3), 0, 0),
        "start_and_tail": (_random(B + 300, 0.02, 4), 50_000, 100_000),    # tiles in front of and behind every record
    }
    for i, n in enumerate((B - 1, B, B + 1, S - 1, S, S + 1)):
        out[f"words_{n}"] = (_random(n, 0.05, 10 + i), 5 * i, 1000 * i)
    return out


BITMAPS = _bitmaps()
GROUPS = {                # unequal jobs: the borders between jobs fall inside the count, the expansion and the six-launch grids
    1: ["words_2049"],
    4: ["words_2047", "ones_block", "one_word", "words_8193"],
    8: ["one_word", "words_8191", "empty", "r1pct_4M", "bit0_only", "words_2049", "empty_runs", "start_and_tail"],
}


def _job(name, d):
    bm, start, room = BITMAPS[name]
    n = int(np.unpackbits(bm.view(np.uint8)).sum())
    length = start + 64 * len(bm) + d * n + room
    aux = np.random.RandomState(len(bm) + d).randint(0, 3, size=max(n, 1)).astype(np.uint8)
    return bm, start, length, aux


def _expected(job, d, tile):
    bm, start, length, aux = job
    v = np.flatnonzero(np.unpackbits(bm.view(np.uint8), bitorder="little")).astype(np.uint64)
    recs = np.zeros(len(v), dtype=_ffi.RECORD_DTYPE)
    recs["pos"] = recs["stop"] = np.uint64(start) + v + np.uint64(d) * np.arange(len(v), dtype=np.uint64)
    recs["type"] = 1
    recs["aux"] = aux[:len(v)]
    n_tiles = (length + tile - 1) // tile
    borders = np.arange(n_tiles + 1, dtype=np.uint64) * np.uint64(tile)
    first = np.searchsorted(recs["pos"].astype(np.uint64), borders, side="right").astype(np.int64) - 1
    return recs, first.astype(np.int32)


@pytest.fixture(scope="module")
def eng():
    with _ffi.Engine(0) as e:
        yield e


def _check(eng, jobs, d):
    tile, three = eng.emit_train(jobs, d=d, train=3)
    tile6, six = eng.emit_train(jobs, d=d, train=6)
    assert tile == tile6 == TILE
    for job, (r3, f3), (r6, f6) in zip(jobs, three, six):
        recs, first = _expected(job, d, tile)
        assert r3.shape == recs.shape and r6.shape == recs.shape
        for field in ("pos", "stop", "extra", "type", "aux", "rsv"):
            assert np.array_equal(r3[field], recs[field]), field
        assert np.array_equal(r3.view(np.uint8), r6.view(np.uint8))
        assert f6 is None
        assert np.array_equal(f3, first)


@pytest.mark.parametrize("d", [1, 300])
@pytest.mark.parametrize("name", sorted(BITMAPS))
def test_one_bitmap_against_numpy(eng, name, d):
    _check(eng, [_job(name, d)], d)


@pytest.mark.parametrize("d", [1, 300])
def test_contig_shorter_than_one_tile(eng, d):
    bm = _with_bits(1, [2, 9, 11])
    _check(eng, [(bm, 100, 5000, np.array([2, 0, 1], dtype=np.uint8))], d)


@pytest.mark.parametrize("d", [1, 300])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_groups_of_unequal_jobs(eng, group, d):
    _check(eng, [_job(name, d) for name in GROUPS[group]], d)


def test_the_hook_refuses_what_it_cannot_run(eng):
    job = _job("one_word", 1)
    with pytest.raises(_ffi.MsimError):
        eng.emit_train([job] * 9)
    with pytest.raises(_ffi.MsimError):
        eng.emit_train([job], train=4)
    with pytest.raises(_ffi.MsimError):
        eng.emit_train([(job[0], job[1], job[2], job[3][:1])])       # fewer outcomes than set bits
