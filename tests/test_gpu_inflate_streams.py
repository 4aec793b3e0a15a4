"""The device inflate (csrc/bgzf.hip: k_bgzf_inflate) on hand-built deflate streams: what RFC 1951 allows and zlib's encoder
never writes (tests/inflate_cases.py; tests/test_deflate_build_host.py shows on the CPU that each stream holds what its name
says and that the zlib-made corpora of tests/test_gpu_bgzf_input.py hold none of it).  The expected value is zlib's inflater
throughout (``deflate_build.zlib_verdict``) and equality is exact: the bytes, or the member's offset and the reason.

Accepted members travel together, a few files for all of them; every refused stream has a file of its own, between two sound
members, and the same engine inflates a sound file after every refusal.

"too many symbols" (the step limit) has no case: every symbol produces a byte or ends a block, so ISIZE or the end of the
input is always reached first."""
from __future__ import annotations

import pytest

import inflate_cases as ic
from deflate_build import zlib_verdict
from mutation_simulator_amd import _ffi, bgzf

pytestmark = pytest.mark.gpu

SOUND_FILE = ic.sound_member(ic.SOUND_A) + ic.sound_member(ic.SOUND_B) + bgzf.EOF_BLOCK


@pytest.fixture(scope="module")
def engine():
    eng = _ffi.Engine(0)
    yield eng
    eng.close()


def _inflate_named(engine, names):
    """One file of the accepted members ``names``; a refusal or a difference is reported with the member's name."""
    acc = ic.accepted()
    members = [bgzf.make_member(acc[n][1], acc[n][0]) for n in names]
    want = [acc[n][1] for n in names]
    for n, w in zip(names, want):
        assert zlib_verdict(acc[n][0], len(w)) == ("ok", w), n
    starts = [sum(map(len, members[:k])) for k in range(len(members))]
    try:
        got = engine.bgzf_inflate(b"".join(members) + bgzf.EOF_BLOCK)
    except _ffi.MsimError as e:
        where = [n for n, s in zip(names, starts) if f"offset {s}:" in str(e)]
        pytest.fail(f"{where}: {e}")
    at = 0
    for n, w in zip(names, want):
        assert got[at:at + len(w)] == w, n
        at += len(w)
    assert got == b"".join(want)


@pytest.mark.parametrize("letters", ["ab", "cd", "e", "f", "g", "hi", "r"])
def test_accepted_streams(engine, letters):
    names = [n for n in ic.accepted() if n[0] in letters]
    assert names
    _inflate_named(engine, names)


def test_300_random_streams(engine):
    names = [n for n in ic.accepted() if n.startswith("j_")]
    assert len(names) == 300
    _inflate_named(engine, names)


def _refusal(engine, file):
    with pytest.raises(_ffi.MsimError) as e:
        engine.bgzf_inflate(file)
    assert e.value.code == _ffi.ERR_VALUE
    assert engine.bgzf_inflate(SOUND_FILE) == ic.SOUND_A + ic.SOUND_B          # the same engine goes on
    return str(e.value)


@pytest.mark.parametrize("name", sorted(ic.refused()))
def test_refused_stream(engine, name):
    payload, blk, why = ic.refused()[name]
    assert zlib_verdict(payload, len(blk)) == ("refused", why)
    ahead = ic.sound_member(ic.SOUND_A)
    text = _refusal(engine, ahead + bgzf.make_member(blk, payload) + ic.sound_member(ic.SOUND_B) + bgzf.EOF_BLOCK)
    assert f"member at offset {len(ahead)}: {why}" in text, text


@pytest.mark.parametrize("first, second", [("l_fixed_distance_symbol_30", "o_distance_produced_plus_1_in_first_block"),
                                           ("o_distance_produced_plus_1_in_first_block", "m_len_nlen_mismatch_at_phase_5")])
def test_two_broken_members_the_lower_offset_is_reported(engine, first, second):
    ref = ic.refused()
    assert ref[first][2] != ref[second][2]
    ahead = ic.sound_member(ic.SOUND_A)
    file = (ahead + bgzf.make_member(ref[first][1], ref[first][0]) + ic.sound_member(ic.SOUND_B)
            + bgzf.make_member(ref[second][1], ref[second][0]) + bgzf.EOF_BLOCK)
    text = _refusal(engine, file)
    assert f"member at offset {len(ahead)}: {ref[first][2]}" in text, text
