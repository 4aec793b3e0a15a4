"""--bgzip without a GPU: output names, the refusals that come before any device work, and the pure-Python BGZF
checker the GPU tests rely on (exercised on a zlib-made file)."""
from __future__ import annotations

import contextlib
import io
import zlib

import pytest

import mutation_simulator_amd as msa
from mutation_simulator_amd import _ffi
from mutation_simulator_amd import __main__ as msa_main
from mutation_simulator_amd import bgzf

from helpers import CASES, case_input_bytes, case_meta


def test_bgzip_output_names():
    args = msa.get_args(["dir/genome.fa", "-o", "out/genome", "--bgzip", "args", "-sn", "0.01"])
    assert str(args.outfasta).endswith("genome_ms.fa.gz")
    assert str(args.outvcf).endswith("genome_ms.vcf.gz")
    plain = msa.get_args(["dir/genome.fa", "-o", "out/genome", "args", "-sn", "0.01"])
    assert str(plain.outfasta).endswith("genome_ms.fa") and str(plain.outvcf).endswith("genome_ms.vcf")
    assert plain.bgzip is False


def _refused(monkeypatch, argv):
    """main(argv) must exit with 1 and an ERROR: line before any device is opened."""
    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(_ffi, "warm_up_async", no_device)
    monkeypatch.setattr(_ffi, "Engine", no_device)
    err = io.StringIO()
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(SystemExit) as e:
            msa_main.main(argv)
    assert e.value.code == 1
    assert any(line.startswith("ERROR:") and "--bgzip" in line for line in err.getvalue().splitlines()), err.getvalue()


def test_bgzip_refused_with_it_mode(monkeypatch, tmp_path):
    meta = case_meta("it_only_4ctg")
    infile = tmp_path / meta["infile_name"]
    infile.write_bytes(case_input_bytes(meta))
    _refused(monkeypatch, ["-c", "--bgzip", "-o", str(tmp_path / "out"), str(infile), "it", "0.5"])
    assert not list(tmp_path.glob("out*"))


def test_bgzip_refused_with_it_lines_in_rmt(monkeypatch, tmp_path):
    meta = case_meta("it_rmt_mutations")
    infile = tmp_path / meta["infile_name"]
    infile.write_bytes(case_input_bytes(meta))
    rmt = tmp_path / "case.rmt"
    rmt.write_text((CASES / "it_rmt_mutations" / "case.rmt").read_text())
    _refused(monkeypatch, ["-c", "--bgzip", "-o", str(tmp_path / "out"), str(infile), "rmt", str(rmt)])
    assert not list(tmp_path.glob("out*"))


def test_bgzip_refused_with_several_gpus(monkeypatch, tmp_path):
    _refused(monkeypatch, ["-c", "--bgzip", "--gpus", "2", "-o", str(tmp_path / "out"), str(tmp_path / "in.fa"),
                           "args", "-sn", "0.01"])


def _corpus():
    parts = [b">chr1 test\n"]
    for i in range(3000):
        parts.append(b"ACGTTGCANNNNACGT" * 3 + f"{i:012d}\n".encode())
    return b"".join(parts)


def test_checker_accepts_zlib_bgzf():
    data = _corpus()
    assert len(data) > 2 * bgzf.BGZF_BLOCK
    for level in (1, 6):
        gz = bgzf.zlib_bgzf(data, level)
        assert bgzf.check_file(gz) == data
        members = bgzf.parse_members(gz)
        assert [m[2] for m in members[:-1]] == [bgzf.BGZF_BLOCK] * (len(members) - 2) + [len(data) % bgzf.BGZF_BLOCK]
        assert members[-1][2] == 0 and gz[members[-1][0]:] == bgzf.EOF_BLOCK
        import gzip
        assert gzip.decompress(gz) == data                      # a multi-member gzip file as well
    assert bgzf.check_file(bgzf.zlib_bgzf(b"")) == b"" and bgzf.zlib_bgzf(b"") == bgzf.EOF_BLOCK


def test_checker_rejects_broken_files():
    gz = bytearray(bgzf.zlib_bgzf(_corpus()))
    with pytest.raises(bgzf.BgzfError):
        bgzf.check_file(bytes(gz[:-28]))                        # no EOF marker
    bad = bytearray(gz)
    bad[16] ^= 1                                                # BSIZE off by one
    with pytest.raises((bgzf.BgzfError, zlib.error)):
        bgzf.check_file(bytes(bad))
    members = bgzf.parse_members(bytes(gz))
    off, bsize = members[0][0], members[0][1]
    bad = bytearray(gz)
    bad[off + bsize - 7] ^= 0xFF                                # CRC32 of the first member
    with pytest.raises(bgzf.BgzfError):
        bgzf.check_file(bytes(bad))
    bad = bytearray(gz)
    bad[12] = ord("X")                                          # no BC subfield
    with pytest.raises(bgzf.BgzfError):
        bgzf.check_file(bytes(bad))
