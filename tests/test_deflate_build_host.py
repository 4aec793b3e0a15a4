"""CPU tier of the hand-built deflate streams (tests/inflate_cases.py) that tests/test_gpu_inflate_streams.py puts through
the device inflate.  Every stream is held to zlib here -- accepted ones inflate to the bytes their tokens describe, refused
ones are refused for the reason the case table states -- and ``deflate_build.scan``, a parser that shares only the RFC's
tables with the writer, says whether a stream really holds the construct it is named for.  The last test runs the same
scanner over the zlib-made files of tests/test_gpu_bgzf_input.py and finds none of these constructs there.

Of the kernel's ten reasons "too many symbols" has no case: every symbol produces a byte or ends a block, and blocks are
bounded by the member's bits, so the step limit cannot be reached before ISIZE or the input runs out."""
from __future__ import annotations

import itertools
import random
import zlib

import pytest

import inflate_cases as ic
from deflate_build import DIST_EXTRA, LEN_EXTRA, Deflate, canonical_codes, scan, zlib_verdict
from mutation_simulator_amd import bgzf


def blocks(name):
    return scan(ic.accepted()[name][0])["blocks"]


def matches(name):
    return [m for b in blocks(name) for m in b.get("matches", ())]


# ------------------------------------------------------------------------------------------------ the writer and the reference
def test_canonical_codes_are_the_rfcs_example():
    assert canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]
    assert canonical_codes([2, 0, 1]) == [0b10, None, 0b0]


def test_writer_replay_and_zlib_agree_on_every_accepted_stream():
    acc = ic.accepted()
    assert len(acc) > 400
    for name, (payload, data) in acc.items():
        assert zlib_verdict(payload, len(data)) == ("ok", data), name
        assert 0 < len(data) <= 65536 and len(bgzf.make_member(data, payload)) <= 65536, name
        assert scan(payload)["out_len"] == len(data), name


def test_zlib_refuses_every_refused_stream_for_the_stated_reason():
    ref = ic.refused()
    for name, (payload, blk, why) in ref.items():
        assert zlib_verdict(payload, len(blk)) == ("refused", why), name
        s = scan(payload, strict=False, limit=len(blk))
        assert s["error"] == (None if why == "data past ISIZE" else why), (name, s)      # the scanner's own opinion
        assert len(blk) > 0 and len(bgzf.make_member(blk, payload)) <= 65536, name
    assert {why for _, _, why in ref.values()} == {"invalid code lengths", "invalid code", "invalid stored block lengths",
                                                   "truncated", "distance too far back", "data past ISIZE"}


def test_zlib_verdict_wording():
    sound = Deflate().fixed(ic.lits(b"GATTACA"), final=True).payload()
    assert zlib_verdict(sound, 7) == ("ok", b"GATTACA")
    assert zlib_verdict(sound, 6) == ("refused", "data past ISIZE")
    assert zlib_verdict(sound, 8) == ("refused", "ISIZE mismatch")
    assert zlib_verdict(sound[:-1], 7) == ("refused", "truncated")
    assert zlib_verdict(b"\x07" + sound, 7) == ("refused", "bad block type")


# ------------------------------------------------------------------------------------------------ coverage, from the scanner
def test_a_runs_across_the_hlit_boundary():
    for name, sym in (("a_run18_across_boundary", 18), ("a_run17_across_boundary", 17), ("a_run16_across_boundary", 16)):
        (b,) = blocks(name)
        assert b["cross"] == [sym] and b["matches"], name
    (b,) = blocks("a_run_ends_on_and_run_starts_on_boundary")
    assert b["ends_on_boundary"] == [18] and b["starts_on_boundary"] == [17] and not b["cross"]


def test_b_16_directly_after_a_zero_run():
    assert blocks("b_16_after_18")[0]["rep_after_zero_run"] == [18]
    assert blocks("b_16_after_17")[0]["rep_after_zero_run"] == [17]


def test_c_code_lengths_at_the_table_edges():
    for name in ("c_litlen_comb_long_codes_on_low_symbols", "c_litlen_comb_long_codes_on_high_symbols"):
        (b,) = blocks(name)
        assert b["ll_defined"] == list(range(1, 16)) and b["ll_used"] == set(range(1, 16)), name      # 10, 11 and 15 among them
    for name in ("c_dist_comb_long_codes_on_low_symbols", "c_dist_comb_long_codes_on_high_symbols"):
        b = blocks(name)[1]
        assert b["d_defined"] == list(range(1, 16)) and b["d_used"] == set(range(1, 16)), name        # 8, 9 and 15 among them
    (b,) = blocks("c_code_length_code_of_7_bits")
    assert b["cl_defined"] == list(range(1, 8)) and b["cl_used"] == set(range(1, 8))
    b = blocks("c_hlit_286_hdist_30_hclen_19")[1]
    assert (b["hlit"], b["hdist"], b["hclen"]) == (286, 30, 19) and b["n_dist_codes"] == 30
    assert {s for s, _ in b["len_syms"]} == set(range(257, 286))
    (b,) = blocks("c_smallest_hclen")
    assert b["hclen"] == 5 and b["n_lit"] == 255
    assert ic.refused()["k_hclen_4_leaves_256_without_a_code"][2] == "invalid code lengths"          # (why 5 is the smallest)


def test_d_distance_sets():
    (b,) = blocks("d_one_distance_code")
    assert b["n_dist_codes"] == 1 and b["d_defined"] == [1] and len(b["matches"]) == 2
    (b,) = blocks("d_no_distance_code")
    assert b["n_dist_codes"] == 0 and b["hdist"] == 1 and not b["matches"] and b["n_lit"] == 4
    (b,) = blocks("d_two_distance_codes")
    assert b["n_dist_codes"] == 2 and {d for _, d, _ in b["matches"]} == {1, 2}
    b = blocks("d_fixed_distance_symbols_0_and_29")[1]
    assert b["type"] == "fixed" and {s for s, _ in b["dist_syms"]} == {0, 29}


def test_e_every_length_and_distance_symbol_at_both_ends_of_its_extra_bits():
    b = blocks("e_every_length_symbol")[1]
    assert b["len_syms"] == {(257 + k, ev) for k in range(29) for ev in (0, (1 << LEN_EXTRA[k]) - 1)}
    assert b["len258_as"] == {284, 285}
    b = blocks("e_every_distance_symbol")[1]
    assert b["dist_syms"] >= {(s, ev) for s in range(30) for ev in (0, (1 << DIST_EXTRA[s]) - 1)}
    assert {24577, 32507, 32767, 32768} <= {d for _, d, _ in b["matches"]}
    assert b["matches"][0][1:] == (32768, 32768) and b["len258_as"] == {284, 285}     # distance = bytes produced so far
    assert [d == pos for _, d, pos in matches("e_distance_reaches_byte_0")] == [True] * 3


def test_f_both_copy_formulations():
    s = scan(ic.accepted()["f_copy_forms"][0])
    pairs = {(length, d) for b in s["blocks"] for length, d, _ in b.get("matches", ())}
    assert pairs == set(itertools.product(ic.F_LENS, ic.F_DISTS))
    assert {d >= length or d >= 320 for length, d in pairs} == {True, False}
    last = s["blocks"][-1]
    assert last["matches"][-1][0] + last["matches"][-1][2] == s["out_len"] and last["final"]          # a match ends at ISIZE
    for b, before in zip(s["blocks"][2::2], s["blocks"][1::2]):                   # fresh stored bytes ahead of every distance
        assert before["type"] == "stored" and before["stored_len"] == b["matches"][0][1]


def test_g_stored_blocks_at_every_bit_phase():
    for phase in range(8):
        for n in ic.G_SIZES:
            first, stored, last = blocks(f"g_stored_{n}_at_phase_{phase}")
            assert (stored["type"], stored["phase"], stored["stored_len"]) == ("stored", phase, n)
            length, dist, pos = last["matches"][0]
            assert pos - dist < first["n_lit"] and pos == first["n_lit"] + n      # from the first block, across the stored one
    assert [b["type"] for b in blocks("g_two_stored_blocks_in_a_row")] == ["fixed", "stored", "stored", "fixed"]
    assert [b["type"] for b in blocks("g_stored_first_and_final")] == ["stored", "fixed", "stored"]


def test_h_bit_reader_tail():
    seen = set()
    for name, (payload, _) in ic.accepted().items():
        if name.startswith("h_"):
            s = scan(payload)
            assert s["trailing_bytes"] == 0 and len(payload) < 16
            seen.add((len(payload) % 4, (s["end_bit"] - 1) % 8))
    assert seen == set(itertools.product(range(4), range(8)))


def test_i_empty_blocks_and_extreme_sizes():
    b = blocks("i_64_empty_fixed_blocks")
    assert len(b) == 65 and all(x["type"] == "fixed" and x["n_lit"] == 0 and not x["matches"] for x in b[:64]) and b[64]["n_lit"]
    for name in ("i_empty_dynamic_block", "i_empty_dynamic_block_of_one_code"):
        first, mid, last = blocks(name)
        assert mid["type"] == "dynamic" and mid["n_lit"] == 0 and not mid["matches"] and first["n_lit"] and last["n_lit"]
    assert blocks("i_empty_dynamic_block_of_one_code")[1]["ll_defined"] == [1]
    assert scan(ic.accepted()["i_isize_1"][0])["out_len"] == 1
    (b,) = blocks("i_isize_65536")
    assert b["n_lit"] == 1 and len(b["matches"]) == 255 and [m[0] for m in b["matches"]].count(258) == 254
    assert scan(ic.accepted()["i_isize_65536"][0])["out_len"] == 65536


def test_j_random_streams():
    names = [n for n in ic.accepted() if n.startswith("j_")]
    assert len(names) == 300
    with_15, with_cross, types, rep_after = 0, 0, set(), 0
    for n in names:
        b = blocks(n)
        types |= {x["type"] for x in b}
        with_15 += any(15 in x.get("ll_used", ()) or 15 in x.get("d_used", ()) for x in b)
        with_cross += any(x.get("cross") for x in b)
        rep_after += any(x.get("rep_after_zero_run") for x in b)
    assert types == {"stored", "fixed", "dynamic"}
    assert with_15 >= 20 and with_cross >= 20, (with_15, with_cross)
    assert rep_after >= 1
    other = ic.random_member(random.Random(ic.SEED))            # fixed seed: the same members every time
    assert other.payload() == ic.accepted()["j_random_000"][0]


def test_r_bytes_behind_the_final_block():
    """zlib's inflater stops at the final block and so does the kernel; ``bgzf.check_file`` asks for more: the deflate data
    must end with the member."""
    payload, data = ic.accepted()["r_bytes_behind_the_final_block"]
    assert scan(payload)["trailing_bytes"] == 3
    with pytest.raises(bgzf.BgzfError, match="do not end with the member"):
        bgzf.check_file(bgzf.make_member(data, payload) + bgzf.EOF_BLOCK)


def test_klmop_defects_sit_early_with_16_sound_bytes_behind():
    for name, (payload, blk, why) in ic.refused().items():
        if name[0] in "klmop":
            s = scan(payload, strict=False, limit=len(blk))
            at = s["past_bit"] if name[0] == "p" else s["error_bit"]
            assert len(payload) - (at + 7) // 8 >= 16, name
    names = set(ic.refused())
    for part in ("litlen_oversubscribed", "litlen_incomplete", "dist_incomplete_two_2bit", "dist_single_code_of_length_2",
                 "code_length_set_incomplete", "code_length_set_of_one_code", "16_as_first", "run_passes", "no_code_for_256",
                 "hlit_287", "hlit_288", "hdist_31", "hdist_32", "litlen_symbol_286", "litlen_symbol_287", "distance_symbol_30",
                 "distance_symbol_31", "unassigned_code", "without_distance_codes", "mismatch_at_phase_2", "mismatch_at_phase_5",
                 "produced_plus_1_in_first", "produced_plus_1_behind_stored", "literal_at_isize", "one_past_isize",
                 "one_byte_too_long"):
        assert sum(part in n for n in names) == 1, part
    texts = {n: scan(p, strict=False)["error_text"] for n, (p, _, _) in ic.refused().items() if n[0] in "klmo"}
    assert texts["k_litlen_oversubscribed"] == "over-subscribed literal/length set"
    assert texts["k_litlen_incomplete"] == "incomplete literal/length set"
    assert texts["k_dist_incomplete_two_2bit_codes"] == texts["k_dist_single_code_of_length_2"] == "incomplete distance set"
    assert texts["k_code_length_set_incomplete"] == texts["k_code_length_set_of_one_code"] == "incomplete code-length set"
    assert texts["k_16_as_first_symbol"] == "repeat without a length before it"
    assert texts["k_run_passes_hlit_hdist_by_one"] == "a run passes HLIT + HDIST"
    assert texts["k_no_code_for_256"] == texts["k_hclen_4_leaves_256_without_a_code"] == "no end-of-block code"
    assert all(texts[f"k_{x}"] == "HLIT / HDIST" for x in ("hlit_287", "hlit_288", "hdist_31", "hdist_32"))
    assert [texts[f"l_fixed_litlen_symbol_{x}"] for x in (286, 287)] == ["length symbol 286", "length symbol 287"]
    assert [texts[f"l_fixed_distance_symbol_{x}"] for x in (30, 31)] == ["distance symbol 30", "distance symbol 31"]
    for n in ("l_unassigned_code_of_a_single_code_distance_set", "l_match_in_a_block_without_distance_codes"):
        assert texts[n].startswith("no distance code"), n
    assert {scan(ic.refused()[n][0], strict=False)["blocks"][1]["phase"] for n in names if n.startswith("m_")} == {2, 5}
    assert texts["o_distance_produced_plus_1_in_first_block"] == "distance 6 with 5 bytes produced"
    assert texts["o_distance_produced_plus_1_behind_stored_block"] == "distance 11 with 10 bytes produced"
    for n, kind in (("p_literal_at_isize", "n_lit"), ("p_match_ends_one_past_isize", "matches")):
        payload, blk, _ = ic.refused()[n]
        assert zlib.decompress(payload, -15)[:len(blk)] == blk                     # (the member's CRC32 is of these bytes)
        cut = scan(payload[:(scan(payload, limit=len(blk))["past_bit"] + 7) // 8], strict=False)
        assert cut["out_len"] == len(blk) + 1 and cut["blocks"][-1][kind], n       # cut behind the symbol that passes ISIZE
    payload, blk, _ = ic.refused()["p_stored_block_one_byte_too_long"]
    first, stored = scan(payload)["blocks"]
    assert stored["type"] == "stored" and first["n_lit"] + stored["stored_len"] == len(blk) + 1
    assert zlib.decompress(payload, -15)[:len(blk)] == blk


def test_n_every_cut_is_where_its_name_says():
    stages = {"n_cut_in_block_header": "block header", "n_cut_in_hclen_lengths": "HCLEN lengths",
              "n_cut_in_code_lengths": "code lengths", "n_cut_in_symbols": "symbols",
              "n_cut_in_length_extra_bits": "length extra bits", "n_cut_in_distance_extra_bits": "distance extra bits",
              "n_cut_in_len_nlen": "LEN / NLEN", "n_cut_in_stored_data": "stored data", "n_no_payload_at_all": "block header",
              "n_cut_one_bit_before_the_end_of_block_code_ends": "symbols"}
    assert {n for n in ic.refused() if n.startswith("n_")} == set(stages)
    for name, stage in stages.items():
        payload = ic.refused()[name][0]
        s = scan(payload, strict=False)
        assert (s["error"], s["stage"]) == ("truncated", stage), (name, s["stage"])
        if stage == "block header" and payload:
            assert s["blocks"][-2]["type"] == "fixed" and len(s["blocks"]) == 3    # the dynamic block's header, 17 bits
    payload = ic.refused()["n_cut_one_bit_before_the_end_of_block_code_ends"][0]
    s = scan(payload + b"\x00")                                  # one more zero bit and the stream is whole
    assert s["end_bit"] == 8 * len(payload) + 1 and s["blocks"][-1]["type"] == "fixed"


# ------------------------------------------------------------------------------------------------ what zlib's encoder never writes
def test_the_existing_zlib_corpora_hold_none_of_this():
    """The files tests/test_gpu_bgzf_input.py decodes, at small sizes (20 000 bytes of each text; of "repeats" the part with
    the periods 20 000 and 32 768, where the long distances are)."""
    import test_gpu_bgzf_input as existing

    n_blocks, max_ll, max_d, max_dist, types = 0, 0, 0, 0, set()
    for name, text in existing.CORPORA.items():
        text = text[-105536:] if name == "repeats" else text[:20000]
        for level, strategy in existing.STRATEGIES:
            for m in bgzf.parse_members(bgzf.zlib_bgzf(text, level, strategy)):
                if not m[2]:
                    continue
                for b in scan(m[4])["blocks"]:
                    n_blocks += 1
                    types.add(b["type"])
                    if b["type"] == "stored":
                        continue
                    assert b["len258_as"] <= {285}
                    max_dist = max([max_dist] + [d for _, d, _ in b["matches"]])
                    if b["type"] == "dynamic":
                        assert not b["cross"], (name, level, strategy)
                        assert b["n_dist_codes"] >= 2, (name, level, strategy)
                        max_ll, max_d = max(max_ll, b["ll_defined"][-1]), max(max_d, b["d_defined"][-1])
    assert types == {"stored", "fixed", "dynamic"} and n_blocks > 50
    assert max_ll < 15 and max_d < 15, (max_ll, max_d)
    assert 20000 <= max_dist <= 32768 - 262, max_dist
