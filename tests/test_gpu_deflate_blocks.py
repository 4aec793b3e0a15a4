"""The device deflate encoder (csrc/bgzf.hip: k_bgzf_deflate) on hand-built blocks (tests/deflate_cases.py): the sizes around
the thread spans, tiny alphabets, histograms whose Huffman trees pass the 15-bit and the 7-bit limit, planted phrases for
every distance and length symbol, header spellings.  tests/test_deflate_twin_host.py shows on the CPU that the inputs are
sound and that the twin the output is held to writes valid streams.

Nothing here has a tolerance.  Every member is checked as a BGZF member (framing, ISIZE, CRC32, the EOF marker), inflated
by zlib and parsed by the strict scanner; the tokens the device chose are read back from its own output and everything behind
them -- the three tables, HLIT, HDIST, HCLEN, the spelling of the header, the choice between a dynamic and a stored block, every
byte of the payload -- must equal the integer twin (tests/deflate_twin.py).  Which matches to take is the kernel's business
(its costs come from ``__log2f``); that it took the ones a case was built for is the case's ``edge`` predicate."""
from __future__ import annotations

import os

import numpy as np
import pytest

import deflate_cases as dc
import deflate_twin as tw
from deflate_build import scan, zlib_verdict
from mutation_simulator_amd import _ffi, bgzf

pytestmark = pytest.mark.gpu

B = bgzf.BGZF_BLOCK
STAGE = 1024 * B                                                 # the channel's staging: BGZF_PIECE_BLOCKS blocks


@pytest.fixture(scope="module")
def engine():
    eng = _ffi.Engine(0)
    yield eng
    eng.close()


def observed(b, t) -> str:
    """What the summary of a run quotes: printed with ``pytest -s``."""
    if b["type"] != "dynamic":
        return f"stored {t['n']} + 5"
    return (f"n {t['n']} tokens: {b['n_lit']} literals {len(b['matches'])} copies; ll depth {t['ll_depth']} steps {t['ll_steps']} "
            f"max {max(b['ll_lengths'])}; d depth {t['d_depth']} steps {t['d_steps']}; cl depth {t['cl_depth']} steps {t['cl_steps']} "
            f"max {max(b['cl_lengths'])}; hlit {b['hlit']} hdist {b['hdist']} hclen {b['hclen']} cross {b['cross']}; "
            f"distance symbols {sorted({s for s, _ in b['dist_syms']})}; length symbols {sorted({s for s, _ in b['len_syms']})}")


@pytest.mark.parametrize("name", [c[0] for c in dc.cases()])
def test_block(engine, name):
    (data, edge), = [(c[1], c[2]) for c in dc.cases() if c[0] == name]
    gz = engine.bgzf_compress(data)
    assert bgzf.check_file(gz) == data
    members = bgzf.parse_members(gz)
    assert len(members) == (len(data) + B - 1) // B + 1
    assert all(m[2] == B for m in members[:-2]) and gz[-28:] == bgzf.EOF_BLOCK
    for k, (_, bsize, isize, _, payload) in enumerate(members[:-1]):
        blk = data[k * B:(k + 1) * B]
        assert isize == len(blk) and bsize + 1 == len(payload) + 26 <= 65536
        assert zlib_verdict(payload, len(blk)) == ("ok", blk)
        s = scan(payload)
        assert s["trailing_bytes"] == 0 and s["out_len"] == len(blk)
        (b,) = s["blocks"]
        assert b["final"] and b["type"] in ("stored", "dynamic")
        if b["type"] == "stored":
            # One-sided: the tokens the kernel weighed are not in a stored block.  On literal-only tokens the twin must not find
            # a dynamic block smaller than n + 5 -- a header counted too large would force storing; copies the kernel took
            # could only be judged with its parse restated.
            t = tw.encode(tw.literal_tokens(blk), len(blk), blk)
            assert t["stored"], (name, k, t["dyn_bytes"])
        else:
            t = tw.encode(tw.tokens_of(b, blk), len(blk), blk)
            assert not t["stored"], (name, k, t["dyn_bytes"])
            for key in ("ll_lengths", "d_lengths", "cl_lengths", "hlit", "hdist", "hclen", "cl_syms"):
                assert b[key] == t[key], (name, k, key)
        print(f"\n{name}[{k}]: {observed(b, t)}")
        assert payload == t["payload"], (name, k)
        assert edge(s, t), (name, k, observed(b, t))
    assert engine.bgzf_compress(data) == gz


def test_channel_pieces_around_the_staging_size(engine, tmp_path):
    """A channel fed in pieces cut one byte before, at and one byte after its staging size (twice), at the block size +- 1 and
    at single bytes writes the file that one call makes of the whole."""
    total = 2 * STAGE + 70000
    unit = dc.skewed_text(1 << 20, 77)
    data = np.tile(np.frombuffer(unit, dtype=np.uint8), total // len(unit) + 1)[:total]
    cuts = [STAGE - 1, STAGE, STAGE + 1, STAGE + B, STAGE + 2 * B + 1, STAGE + 3 * B, STAGE + 3 * B + 1,
            2 * STAGE - 1, 2 * STAGE, 2 * STAGE + 1, 2 * STAGE + 1 + B - 1, total - 1, total]
    assert cuts == sorted(set(cuts))
    path = tmp_path / "pieces.gz"
    with open(path, "w+b") as f:
        engine.bgzf_open(bgzf.FASTA_CHANNEL, f.fileno())
        at = 0
        for c in cuts:
            engine.bgzf_append(bgzf.FASTA_CHANNEL, data[at:c])
            at = c
        sizes = engine.bgzf_close(bgzf.FASTA_CHANNEL)
    whole = engine.bgzf_compress(data)
    assert sizes == (len(whole), total) and os.path.getsize(path) == len(whole)
    assert path.read_bytes() == whole
    at = 0
    for raw in bgzf.inflate_members(whole):                      # (framing, ISIZE and CRC32 of every member on the way)
        assert raw == data[at:at + len(raw)].tobytes()
        at += len(raw)
    assert at == total
