"""msim_batch_run (an assembly's small contigs in ONE pass) vs the per-contig path, on shapes chosen for the batch's own edges.

The oracle is the project's own per-contig path on a fresh engine: the same seed and params, ``set_plan_mode(PLAN_HOST)``, then
``plan_contig`` / ``apply_contig`` / ``fetch_sequence_framed`` / ``render_vcf_device`` contig by contig.  Both paths plan with the
sequential host planner off the same two streams, so every byte and both stream states are EQUAL -- nothing here has a tolerance.
The expected Fasta text is '>' header '\\n' + the framed body per contig, with a '\\n' in front of a header iff the previous body
ended in the middle of a line (what ``FastaWriter.write_header`` does).

A contig without bases never reaches the per-contig path's APPLY (nothing to launch for): it is planned only -- the streams move as
the batch's do -- and its expected body and VCF text are empty.

The KeyError contig is all ``X``, not ``N``: N is in the reference's transversion dict (N -> N, mutator.py:449-455, see
test_gpu_apply_tables.py), so a contig of N raises nothing; X is outside AGTCN and outside the ambiguity codes."""
from __future__ import annotations

import ctypes as C
import os
import tempfile

import numpy as np
import pytest

from mutation_simulator_amd import _ffi
from mutation_simulator_amd import mutator as mm

pytestmark = pytest.mark.gpu

ARGS_ORDER = [1, 2, 3, 5, 4, 6, 7]          # SN, IN, DE, IV, DU, TL, TLI  (rmt.py:443-450)
SN, IN, DE, DU, IV, TL, TLI = 1, 2, 3, 4, 5, 6, 7
SEED = (20240, 77)


def _params(titv=1.0):
    from mutation_simulator_amd.mut_types import MutType

    class S:
        pass
    S.mut_block = {t: 1 for t in MutType}
    S.titv = titv
    return mm.params_descriptor(S)


def _range(L, rate, chances, lens):
    """The std range over a whole contig, thresholds built like mutator.range_descriptor."""
    r = _ffi.Range()
    r.start, r.stop, r.k = 0, L - 1, int(L * rate)
    r.setsize = mm.sample_setsize(r.k)
    p = np.array([chances.get(t, 0.0) for t in ARGS_ORDER], dtype=np.float64)
    cdf = np.cumsum(p / p.sum())
    cdf /= cdf[-1]
    r.n_types = len(ARGS_ORDER)
    for j, t in enumerate(ARGS_ORDER):
        r.types[j] = t
        r.cdf_thr[j] = mm._ceil_scaled(float(cdf[j]))
    for t in (IN, DE, DU, TL):
        r.min_len[t], r.max_len[t] = lens.get(t, (1, 2))
    r.min_len[IV], r.max_len[IV] = lens.get(IV, (2, 3))
    return r


SNP_ONLY = ({SN: 1.0}, {})
INDELS = ({SN: 0.5, IN: 0.25, DE: 0.25}, {IN: (1, 5), DE: (1, 5)})
# every record type; TL and TLI candidates are paired behind the last range (__link_tls, plan_host.cpp), a surplus is dropped
ALL_TYPES = ({SN: 0.2, IN: 0.15, DE: 0.15, DU: 0.1, IV: 0.1, TL: 0.15, TLI: 0.15}, {IN: (1, 6), DE: (1, 6), DU: (2, 8), IV: (2, 8), TL: (2, 10)})


class Spec:
    """One contig of a batch: its bases as they stand in the file, the file's line geometry, its ranges and names."""

    def __init__(self, i, bases: bytes, lenc=60, eol=b"\n", rate=0.0, mix=SNP_ONLY, last_eol=True):
        self.bases = bases
        self.lenc, self.lenb = lenc, lenc + len(eol)
        lines = [bases[k:k + lenc] for k in range(0, len(bases), lenc)]
        self.body = eol.join(lines) + (eol if lines and last_eol else b"")
        self.ranges = [_range(len(bases), rate, *mix)] if rate > 0 and bases else []
        self.name = f"ctg{i}"
        self.header = f"ctg{i} length={len(bases)} batch test"


def _bases(rs, n, alphabet=b"ACGT"):
    return bytes(rs.choice(np.frombuffer(alphabet, dtype=np.uint8), n).astype(np.uint8)) if n else b""


def _engine():
    eng = _ffi.Engine(0)
    eng.seed(*SEED)
    eng.set_params(_params())
    return eng


class Want:
    pass


def _oracle_run(eng, specs, checkpoints=()):
    """The per-contig path over ``specs`` on ``eng`` (PLAN_HOST); per-contig texts and counts, and the two stream states behind
    every contig count in ``checkpoints`` and behind the last contig."""
    w = Want()
    w.head, w.body, w.vcf, w.empty, w.n_rec, w.states = [], [], [], [], [], {}
    for i, s in enumerate(specs):
        cid = eng.add_contig(np.frombuffer(s.bases.upper(), dtype=np.uint8))
        eng.plan_contig(cid, s.ranges)
        w.empty.append(eng.plan_was_empty(cid))
        w.n_rec.append(eng.result_sizes(cid, applied=False)[1])
        if s.bases:
            eng.apply_contig(cid)
            w.body.append(eng.fetch_sequence_framed(cid, s.lenc).tobytes())
            w.vcf.append(eng.render_vcf_device(cid, s.name).tobytes())
        else:
            w.body.append(b"")
            w.vcf.append(b"")
        w.head.append(b">" + s.header.encode() + b"\n")
        eng.clear()
        if i + 1 in checkpoints or i + 1 == len(specs):
            w.states[i + 1] = [eng.get_mt_state(0), eng.get_mt_state(1)]
    return w


def _expected(w, specs, n):
    """What the batch of the first ``n`` contigs must give, from the oracle's per-contig results."""
    parts = []
    for i in range(n):
        mid_line = i > 0 and w.body[i - 1] != b"" and not w.body[i - 1].endswith(b"\n")
        parts.append((b"\n" if mid_line else b"") + w.head[i] + w.body[i])
    last = w.body[n - 1]
    return {"fasta": b"".join(parts), "vcf": b"".join(w.vcf[:n]), "fasta_bytes": [len(p) for p in parts],
            "vcf_bytes": [len(v) for v in w.vcf[:n]], "empty": [bool(e) for e in w.empty[:n]], "n_records": list(w.n_rec[:n]),
            "last_line_bases": 0 if last.endswith(b"\n") else len(last) - (last.rfind(b"\n") + 1), "states": w.states[n]}


def _table(specs):
    """(msim_batch_contig array, what it points at)."""
    n = len(specs)
    arr = (_ffi.BatchContig * max(n, 1))()
    keep = []
    for i, s in enumerate(specs):
        body = np.frombuffer(s.body, dtype=np.uint8)
        ra = (_ffi.Range * max(len(s.ranges), 1))(*s.ranges)
        nm, hd = s.name.encode(), s.header.encode()
        keep.append((body, ra, nm, hd))
        q = arr[i]
        q.body = body.ctypes.data if len(s.body) else None
        q.body_bytes = len(s.body)
        q.n_bases = len(s.bases)
        q.lenc, q.lenb = s.lenc, s.lenb
        q.ranges = ra
        q.n_ranges = len(s.ranges)
        q.name = nm
        q.header = hd
    return arr, keep


def _batch_run(eng, arr, n):
    """(return code, message) of msim_batch_run: the raw call, so that refusals can be looked at."""
    rc = eng.lib.msim_batch_run(eng.h, arr, n)
    return rc, eng.lib.msim_last_error(eng.h).decode()


def _view(eng):
    fp, vp = C.c_void_p(), C.c_void_p()
    fn, vn, last = C.c_uint64(), C.c_uint64(), C.c_uint64()
    eng._check(eng.lib.msim_batch_view(eng.h, C.byref(fp), C.byref(fn), C.byref(vp), C.byref(vn), C.byref(last)))
    return C.string_at(fp, fn.value) if fn.value else b"", C.string_at(vp, vn.value) if vn.value else b"", last.value


def _sizes_only(eng):
    fn, vn = C.c_uint64(), C.c_uint64()
    eng._check(eng.lib.msim_batch_view(eng.h, None, C.byref(fn), None, C.byref(vn), None))
    return fn.value, vn.value


def _fetch(eng):
    fn, vn = _sizes_only(eng)
    fa, vc = np.full(fn + 8, 0xEE, dtype=np.uint8), np.full(vn + 8, 0xEE, dtype=np.uint8)
    eng._check(eng.lib.msim_batch_fetch(eng.h, C.c_void_p(fa.ctypes.data), fn, C.c_void_p(vc.ctypes.data), vn))
    assert (fa[fn:] == 0xEE).all() and (vc[vn:] == 0xEE).all()      # nothing written behind the texts
    return fa[:fn].tobytes(), vc[:vn].tobytes()


def _fetch_file(eng):
    fn, vn = _sizes_only(eng)
    with tempfile.TemporaryFile() as ff, tempfile.TemporaryFile() as vf:
        eng.batch_fetch_to_files(ff.fileno() if fn else -1, 0, vf.fileno() if vn else -1, 0)
        eng.file_wait()
        return os.pread(ff.fileno(), fn + 1, 0), os.pread(vf.fileno(), vn + 1, 0)


def _batch_sizes(eng, n):
    fb, vb, nr = (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_uint64 * n)()
    em = (C.c_int32 * n)()
    eng._check(eng.lib.msim_batch_sizes(eng.h, n, fb, vb, em, nr))
    return list(fb), list(vb), [bool(e) for e in em], list(nr)


def _same_states(eng, want):
    for stream in (0, 1):
        mt, pos = eng.get_mt_state(stream)
        assert pos == want[stream][1] and np.array_equal(mt, want[stream][0]), f"stream {stream} stands elsewhere"


def _check_batch(eng, specs, want, order=("fetch", "file", "view")):
    """One msim_batch_run over ``specs`` on ``eng`` and everything it can be asked for afterwards, against ``want``."""
    n = len(specs)
    arr, keep = _table(specs)
    rc, msg = _batch_run(eng, arr, n)
    assert rc == _ffi.OK, msg
    for what in order:                       # (the first one that wants the Fasta text frames it; the others find it framed or copy)
        if what == "view":
            fasta, vcf, last = _view(eng)
            assert last == want["last_line_bases"]
        else:
            fasta, vcf = _fetch(eng) if what == "fetch" else _fetch_file(eng)
        assert fasta == want["fasta"], f"Fasta text ({what})"
        assert vcf == want["vcf"], f"VCF text ({what})"
    fb, vb, em, nr = _batch_sizes(eng, n)
    assert fb == want["fasta_bytes"] and vb == want["vcf_bytes"] and em == want["empty"] and nr == want["n_records"]
    _same_states(eng, want["states"])
    del keep


# ---------------------------------------------------------------------------------------------------------------- line ends
LENC = 7


def _line_end_specs():
    rs = np.random.RandomState(11)
    specs = []
    for i, L in enumerate([0, 1, LENC - 1, LENC, LENC + 1, 2 * LENC, 2 * LENC + 1]):      # LF input, dense SNPs + indels
        specs.append(Spec(len(specs), _bases(rs, L), LENC, b"\n", rate=0.3, mix=INDELS, last_eol=bool(i & 1)))
    for L in [LENC, 2 * LENC + 1, 3 * LENC - 1]:                                           # CRLF input, SNPs only: the length stays
        specs.append(Spec(len(specs), _bases(rs, L), LENC, b"\r\n", rate=0.3))
    specs.append(Spec(len(specs), _bases(rs, 40, b"acgtACGT"), LENC, b"\n", rate=0.2))     # lower-case bases
    specs.append(Spec(len(specs), _bases(rs, 2 * LENC), LENC, b"\n"))                      # n_ranges = 0, ends on a full line
    specs.append(Spec(len(specs), _bases(rs, 23), 5, b"\n", rate=0.2, mix=INDELS))         # other line widths beside it
    specs.append(Spec(len(specs), _bases(rs, 30), 10, b"\r\n", rate=0.2, mix=INDELS))
    specs.append(Spec(len(specs), b"", LENC))                                              # a null body in the middle ...
    specs.append(Spec(len(specs), _bases(rs, LENC + 3), LENC, b"\n", rate=0.3, mix=INDELS))
    specs.append(Spec(len(specs), b"", LENC))                                              # ... and as the last contig
    return specs


def test_line_ends():
    specs = _line_end_specs()
    n = len(specs)
    with _engine() as o:
        o.set_plan_mode(_ffi.PLAN_HOST)
        w = _oracle_run(o, specs, checkpoints=(n - 1,))
    with _engine() as eng:                                   # the last contig a null body
        _check_batch(eng, specs, _expected(w, specs, n))
    want = _expected(w, specs, n - 1)                        # the last contig ends in the middle of a line
    assert want["last_line_bases"] != 0
    with _engine() as eng:
        _check_batch(eng, specs[:-1], want, order=("view", "fetch", "file"))
    with _engine() as o, _engine() as eng:                   # a batch of one contig of one base
        o.set_plan_mode(_ffi.PLAN_HOST)
        _check_batch(eng, specs[1:2], _expected(_oracle_run(o, specs[1:2]), specs[1:2], 1), order=("file", "view"))


# ------------------------------------------------------------------------------------------------------------------- slices
SLICE_COUNTS = (63, 64, 128, 200)            # parallel_slices: min(threads, n / 64) parts -> 1, 1, 2, 3 (200 = 66 + 67 + 67)


@pytest.fixture(scope="module")
def slice_case():
    rs = np.random.RandomState(12)
    specs = [Spec(i, _bases(rs, int(rs.randint(30, 401))), int(rs.choice([50, 60, 61])), b"\n", rate=0.05, mix=INDELS)
             for i in range(max(SLICE_COUNTS))]
    with _engine() as o:
        o.set_plan_mode(_ffi.PLAN_HOST)
        return specs, _oracle_run(o, specs, checkpoints=SLICE_COUNTS)     # (a batch of the first n contigs: the oracle's first n)


@pytest.mark.parametrize("n", SLICE_COUNTS)
def test_slices(slice_case, n):
    specs, w = slice_case
    want = _expected(w, specs, n)
    assert sum(1 for v in want["vcf_bytes"] if v) > n // 2              # VCF lines in every slice: vcf0 is rebased for real
    with _engine() as eng:
        _check_batch(eng, specs[:n], want)


# --------------------------------------------------------------------------------------------------------- all record types
# seed picked with the host planner (host-only context, no GPU) so that a contig behind the first holds an IN and a TLI:
# with (20240, 77) the five contigs hold, per type SN IN DE DU IV TL TLI, ALL_TYPES_COUNTS
ALL_TYPES_LENS = (2000, 1777, 2048, 1913, 2222)
ALL_TYPES_COUNTS = [[3, 4, 2, 1, 3, 1, 1], [4, 1, 4, 1, 1, 2, 2], [4, 5, 2, 1, 3, 1, 1], [5, 6, 1, 0, 0, 2, 2], [5, 5, 1, 1, 2, 4, 4]]


def _all_type_specs(first=0):
    rs = np.random.RandomState(13)
    return [Spec(first + i, _bases(rs, L), 60, b"\n", rate=0.01, mix=ALL_TYPES) for i, L in enumerate(ALL_TYPES_LENS)]


def test_all_record_types():
    specs = _all_type_specs()
    counts = np.zeros((len(specs), 8), dtype=int)
    with _engine() as o:
        o.set_plan_mode(_ffi.PLAN_HOST)
        for i, s in enumerate(specs):                                    # the types, contig by contig, off the same streams
            cid = o.add_contig(np.frombuffer(s.bases, dtype=np.uint8))
            o.plan_contig(cid, s.ranges)
            recs, _ = o.fetch_records(cid)
            counts[i] = np.bincount(recs["type"], minlength=8)
            o.clear()
    assert counts[:, 1:].tolist() == ALL_TYPES_COUNTS
    assert (counts[:, 1:].sum(axis=0) > 0).all(), counts                 # every type occurs ...
    assert counts[1:, IN].sum() > 0 and counts[1:, TLI].sum() > 0, counts    # ... IN (pool rebase) and TLI (span rebase) behind contig 0
    assert (counts[:, 1:].sum(axis=1) >= 3).all(), counts
    with _engine() as o:
        o.set_plan_mode(_ffi.PLAN_HOST)
        w = _oracle_run(o, specs)
    assert w.n_rec == counts[:, 1:].sum(axis=1).tolist()
    with _engine() as eng:
        _check_batch(eng, specs, _expected(w, specs, len(specs)))


# ------------------------------------------------------------------------------------------------- batches in a row, KeyError
def _mixed_specs(rs, n, lo, hi, first=0):
    return [Spec(first + i, _bases(rs, int(rs.randint(lo, hi))), 60, b"\n", rate=0.02, mix=ALL_TYPES) for i in range(n)]


def test_batches_in_a_row():
    """A larger batch, a smaller one, a larger one again on ONE engine: the buffers are reused and regrown, no text shows its
    predecessor's tail, and the streams carry through."""
    rs = np.random.RandomState(14)
    runs = [_mixed_specs(rs, 40, 1500, 2500), _mixed_specs(rs, 3, 40, 90, 40), _mixed_specs(rs, 70, 2500, 4000, 43)]
    with _engine() as o, _engine() as eng:
        o.set_plan_mode(_ffi.PLAN_HOST)
        for k, specs in enumerate(runs):
            w = _oracle_run(o, specs)                                    # (the oracle engine's streams carry through as well)
            _check_batch(eng, specs, _expected(w, specs, len(specs)), order=("view", "fetch", "file") if k != 1 else ("file", "fetch", "view"))


def _next_contig_id(eng):
    return eng.add_contig(np.frombuffer(b"ACGT", dtype=np.uint8))


def _key_contig(eng):
    fn = eng.lib.msim_batch_key_contig
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int)]
    who = C.c_int(-2)
    eng._check(fn(eng.h, C.byref(who)))
    return who.value


def test_key_error():
    rs = np.random.RandomState(15)
    good = _mixed_specs(rs, 5, 300, 600)
    bad = Spec(99, b"X" * 200, 60, b"\n", rate=0.2)       # 40 SNPs at titv 1: one of them surely is a transversion
    specs = good[:2] + [bad] + good[2:]
    with _engine() as o:                                  # the per-contig path's message for that contig
        o.set_plan_mode(_ffi.PLAN_HOST)
        _oracle_run(o, specs[:2])
        cid = o.add_contig(np.frombuffer(bad.bases, dtype=np.uint8))
        o.plan_contig(cid, bad.ranges)
        o.apply_contig(cid)
        want_rc = o.lib.msim_result_sizes(o.h, cid, C.byref(C.c_uint64()), None, None)
        want_msg = o.lib.msim_last_error(o.h).decode()
    assert want_rc == _ffi.ERR_KEY and want_msg == "KeyError: 'X'"
    with _engine() as eng:
        first = _next_contig_id(eng)
        arr, keep = _table(specs)
        rc, msg = _batch_run(eng, arr, len(specs))
        assert (rc, msg) == (want_rc, want_msg)
        assert _key_contig(eng) == 2
        assert _next_contig_id(eng) == first + 1          # the super-contig has left the context
        # a batch without that contig, on the same engine from the same stream states, gives the oracle's bytes
        eng.seed(*SEED)
        with _engine() as o:
            o.set_plan_mode(_ffi.PLAN_HOST)
            w = _oracle_run(o, good)
        _check_batch(eng, good, _expected(w, good, len(good)))
        assert _key_contig(eng) == -1
        assert _next_contig_id(eng) == first + 2
        del keep


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refusal_cases():
    rs = np.random.RandomState(16)

    def base():
        return [Spec(i, _bases(rs, 50), 20, b"\n", rate=0.1) for i in range(3)]
    a = base()
    a[1].lenb = a[1].lenc - 1                             # lenb < lenc
    b = base()
    b[2].body = b[2].body[:40]                            # 50 bases at 20 per line need 52 bytes of text
    c = base()
    c[0].name = None                                      # a null name
    return {"lenb < lenc": (a, 3), "short body": (b, 3), "null name": (c, 3), "n < 1": (base(), 0)}


@pytest.mark.parametrize("case", ["lenb < lenc", "short body", "null name", "n < 1"])
def test_refusals(case):
    specs, n = _refusal_cases()[case]
    with _engine() as eng:
        first = _next_contig_id(eng)
        states = [eng.get_mt_state(0), eng.get_mt_state(1)]
        names = [s.name for s in specs]
        for s in specs:
            s.name = s.name or "x"
        arr, keep = _table(specs)
        for i, nm in enumerate(names):
            if nm is None:
                arr[i].name = None
        rc, _ = _batch_run(eng, arr, n)
        assert rc == _ffi.ERR_ARG
        assert eng.stats()["apply_launches"] == 0 and eng.stats()["contigs_batch"] == 0     # nothing planned, nothing launched
        _same_states(eng, states)
        assert _next_contig_id(eng) == first + 1
        del keep
