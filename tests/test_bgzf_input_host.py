"""BGZF-compressed Fasta input without a GPU: the host pass over the member chain (msim_bgzf_probe), the output names, the
refusals that come before any device work, and detection of the format by content."""
from __future__ import annotations

import contextlib
import gzip
import io
import struct

import numpy as np
import pytest

import mutation_simulator_amd as msa
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import __main__ as msa_main
from mutation_simulator_amd import bgzf, fasta_io

B = bgzf.BGZF_BLOCK


def _text(n: int) -> bytes:
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(n).integers(0, 4, n)].tobytes()


@pytest.mark.parametrize("n,members", [(0, 1), (1, 2), (B, 2), (B + 1, 3), (10 * B + 17, 12)])
def test_probe_counts(n, members):
    gz = bgzf.zlib_bgzf(_text(n), 6)
    assert len(bgzf.parse_members(gz)) == members
    assert _ffi.bgzf_probe(gz) == (n, members)                  # (empty members -- the EOF marker -- count)


def _value_error(data, *words):
    with pytest.raises(_ffi.MsimError) as e:
        _ffi.bgzf_probe(data)
    assert e.value.code == _ffi.ERR_VALUE
    assert all(w in str(e.value) for w in words), str(e.value)


def test_probe_refuses_what_is_not_bgzf():
    _value_error(gzip.compress(_text(1000)), "BGZF framing")
    _value_error(b">chr1\nACGT\n", "not gzip")
    gz = bgzf.zlib_bgzf(_text(3 * B), 6)
    members = bgzf.parse_members(gz)
    off, bsize = members[1][0], members[1][1]
    _value_error(gz[:off + bsize // 2], f"offset {off}", "truncated")               # cut in the middle of a member
    bad = bytearray(gz[:members[2][0]])                                             # two members, the second's BSIZE too large
    struct.pack_into("<H", bad, off + 16, bsize + 100)
    _value_error(bytes(bad), f"offset {off}", "BSIZE")
    bad = bytearray(gz)
    bad[off + 12] = ord("X")                                                        # no BC subfield
    _value_error(bytes(bad), f"offset {off}", "BGZF framing")


def test_probe_concatenated_files_and_missing_eof():
    a, b = bgzf.zlib_bgzf(_text(B + 5), 1), bgzf.zlib_bgzf(_text(777), 9)
    assert _ffi.bgzf_probe(a + b) == (B + 5 + 777, 3 + 2)       # an EOF marker in the middle
    assert a.endswith(bgzf.EOF_BLOCK)
    assert _ffi.bgzf_probe(a[:-28]) == (B + 5, 2)               # files of older writers lack the marker


def _fasta() -> bytes:
    t = _text(6000).decode()
    return (">chr1 test\n" + "\n".join(t[a:a + 60] for a in range(0, 6000, 60)) + "\n").encode()


@pytest.mark.parametrize("infile,fa,vcf", [
    ("genome.fa.gz", "genome_ms.fa", "genome_ms.vcf"),
    ("genome.fasta.bgz", "genome_ms.fasta", "genome_ms.vcf"),
    ("genome.fa", "genome_ms.fa", "genome_ms.vcf"),
])
def test_output_names(infile, fa, vcf, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "dir").mkdir()
    infile = "dir/" + infile
    (tmp_path / infile).write_bytes(_fasta() if infile.endswith(".fa") else bgzf.zlib_bgzf(_fasta(), 6))
    for bgzip in (False, True):
        gz = ".gz" if bgzip else ""
        extra = ["--bgzip"] if bgzip else []
        args = msa.get_args([infile] + extra + ["args", "-sn", "0.01"])
        assert (str(args.outfasta), str(args.outvcf)) == (fa + gz, vcf + gz)
        args = msa.get_args([infile, "-o", "out/x"] + extra + ["args", "-sn", "0.01"])
        suffix = fa[fa.index("_ms") + 3:]
        assert (str(args.outfasta), str(args.outvcf)) == ("out/x_ms" + suffix + gz, "out/x_ms.vcf" + gz)
        args = msa.get_args([infile, "-o", "."] + extra + ["args", "-sn", "0.01"])                # (a directory: the input's stem)
        assert (str(args.outfasta), str(args.outvcf)) == (fa + gz, vcf + gz)


def test_text_input_named_gz_keeps_the_reference_names(tmp_path):
    infile = tmp_path / "g.fa.gz"
    infile.write_bytes(_fasta())                                # text, whatever the name says
    args = msa.get_args([str(infile), "-o", str(tmp_path / "base"), "args", "-sn", "0.01"])
    assert (args.outfasta.name, args.outvcf.name) == ("base_ms.gz", "base_ms.vcf")


def _refused(monkeypatch, argv, word):
    """main(argv) must exit with 1 and an ERROR: line that holds `word`, before any device is opened."""
    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(_ffi, "warm_up_async", no_device)
    monkeypatch.setattr(_ffi, "Engine", no_device)
    err = io.StringIO()
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(SystemExit) as e:
            msa_main.main(argv)
    assert e.value.code == 1
    assert any(line.startswith("ERROR:") and word in line for line in err.getvalue().splitlines()), err.getvalue()


def test_plain_gzip_input_is_refused(monkeypatch, tmp_path):
    infile = tmp_path / "genome.fa.gz"
    infile.write_bytes(gzip.compress(_fasta()))
    with pytest.raises(msa.UnsupportedCompressionFormat):
        msa.load_fasta(infile)
    _refused(monkeypatch, ["-c", "-o", str(tmp_path / "out"), str(infile), "args", "-sn", "0.01"], "bgzip")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["genome.fa.gz"]
    assert msa.UnsupportedCompressionFormat in msa_main._INIT_ERRORS


def test_bgzf_input_refused_with_several_gpus(monkeypatch, tmp_path):
    infile = tmp_path / "genome.fa.gz"
    infile.write_bytes(bgzf.zlib_bgzf(_fasta(), 6))
    _refused(monkeypatch, ["-c", "--gpus", "2", "-o", str(tmp_path / "out"), str(infile), "args", "-sn", "0.01"], "--gpus 1")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["genome.fa.gz"]


def test_text_named_gz_loads_as_text(tmp_path):
    infile = tmp_path / "x.fa.gz"
    infile.write_bytes(_fasta())
    fa = msa.load_fasta(infile)
    assert not fa.compressed and list(fa.keys()) == ["chr1"] and len(fa["chr1"]) == 6000
    assert fa.text.tobytes() == _fasta()
    assert fasta_io.is_gzip(infile) is False
