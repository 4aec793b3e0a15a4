"""A liftover chain read off the rewrite loop: ``apply_ref.apply``'s walk (the reference's ``Mutator.__mutate_sequence``,
mutator.py:318-426) with the bytes left out and the coordinates kept.

Nothing here knows about gaps, heads or prefix sums.  The walk stands at reference position ``t`` and mutated position
``q``; whatever it COPIES from the input -- the stretch in front of a record, the base an insertion lands in front of, a
duplication's first copy -- is an aligned run ``(t, q, n)``; an SNP is a copied base with another letter.  Whatever it writes
from elsewhere (an insert, a duplication's second copy, a reverse-complemented span) advances ``q`` alone, whatever it skips
advances ``t`` alone.  Runs that touch in BOTH coordinates are one block; the chain is the list of blocks (UCSC chain format,
reference = target, mutated = query, both strands +).
"""
from __future__ import annotations

SN, IN, DE, DU, IV, TL, TLI = 1, 2, 3, 4, 5, 6, 7


def blocks(recs, length: int):
    """(the aligned blocks [(t, q, n), ...] in order, the mutated length)."""
    runs = []
    at = 0              # next input base to look at (apply_ref: `at`)
    o = 0               # bytes written so far (apply_ref: `o`)

    def copy(t, n):
        nonlocal o
        if n > 0:
            runs.append((t, o, n))
            o += n

    fields = zip(recs["pos"].tolist(), recs["stop"].tolist(), recs["extra"].tolist(), recs["type"].tolist())
    for p, stop, extra, typ in fields:
        assert at <= p < length
        copy(at, p - at)                                              # write(bases[at:p])
        if typ == SN:
            copy(p, 1)                                                # one base, another letter
            at = p + 1
        elif typ == IN:
            o += stop + 1 - p                                         # write(pool[...])
            copy(p, 1)                                                # write(bases[p:p + 1])
            at = p + 1
        elif typ in (DE, TL):
            at = stop + 1
        elif typ == IV:
            o += stop + 1 - p                                         # the span, reverse-complemented: no base of it is copied
            at = stop + 1
        elif typ == DU:
            copy(p, stop + 1 - p)                                     # write(bases[p:stop + 1]) ...
            o += stop + 1 - p                                         # ... twice
            at = stop + 1
        elif typ == TLI:
            o += len(range(extra, stop + 1))                          # write(insert): bases[extra:stop + 1], converted
            copy(p, 1)
            at = p + 1
        else:
            raise AssertionError(typ)
    copy(at, length - at)                                             # write(bases[at:])
    merged = []
    for t, q, n in runs:
        if merged and merged[-1][0] + merged[-1][2] == t and merged[-1][1] + merged[-1][2] == q:
            merged[-1] = (merged[-1][0], merged[-1][1], merged[-1][2] + n)
        else:
            merged.append((t, q, n))
    return merged, o


def render(recs, length: int, t_name: str, q_name: str, chain_id: int) -> bytes:
    """The chain's text; empty when no base is aligned."""
    bl, q_size = blocks(recs, length)
    if not bl:
        return b""
    score = sum(n for _, _, n in bl)
    (t0, q0, _), (t1, q1, n1) = bl[0], bl[-1]
    out = [f"chain {score} {t_name} {length} + {t0} {t1 + n1} {q_name} {q_size} + {q0} {q1 + n1} {chain_id}\n"]
    for (t, q, n), (tn, qn, _) in zip(bl, bl[1:]):
        out.append(f"{n}\t{tn - (t + n)}\t{qn - (q + n)}\n")
    out.append(f"{n1}\n\n")
    return "".join(out).encode()


def parse(text: bytes):
    """The chains of a chain file as dicts (header fields + ``blocks`` [(t, q, n), ...]), for the semantic checks."""
    chains, cur = [], None
    for line in text.decode().split("\n"):
        if line.startswith("chain "):
            f = line.split(" ")
            assert len(f) == 13 and f[4] == "+" and f[9] == "+", line
            cur = {"score": int(f[1]), "tName": f[2], "tSize": int(f[3]), "tStart": int(f[5]), "tEnd": int(f[6]), "qName": f[7],
                   "qSize": int(f[8]), "qStart": int(f[10]), "qEnd": int(f[11]), "id": int(f[12]), "blocks": [], "open": True}
            cur["t"], cur["q"] = cur["tStart"], cur["qStart"]
            chains.append(cur)
        elif line:
            assert cur is not None and cur["open"], line
            f = [int(x) for x in line.split("\t")]
            assert len(f) in (1, 3) and f[0] > 0, line
            cur["blocks"].append((cur["t"], cur["q"], f[0]))
            cur["t"] += f[0]
            cur["q"] += f[0]
            if len(f) == 3:
                assert f[1] + f[2] > 0, line
                cur["t"] += f[1]
                cur["q"] += f[2]
            else:
                assert cur["t"] == cur["tEnd"] and cur["q"] == cur["qEnd"], line
                cur["open"] = False
    assert all(not c["open"] for c in chains)
    return chains
