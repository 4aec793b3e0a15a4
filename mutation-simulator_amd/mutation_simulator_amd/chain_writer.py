"""``<outbase>_ms.chain``: the liftover chains of a run, one per contig, in contig order (``--chain``).

The text comes rendered from libmsim (``msim_render_chain_device``: the contig's mutation table in HBM as a UCSC chain,
reference = target, mutated genome = query); this only appends it.  The file is plain text also under ``--bgzip``.
"""
from __future__ import annotations

from pathlib import Path


class ChainWriterError(Exception):
    """The chain file cannot be written."""


class ChainWriter:
    def __init__(self, path: Path):
        self._path = Path(path)
        try:
            self._file = open(self._path, "wb")
        except OSError as e:
            raise ChainWriterError(f"Cannot write chain file {self._path} ({e.strerror})") from None

    def write_contig(self, engine, contig: int, name: str, number: int):
        """Append the chain of the engine's planned contig ``contig``: tName = qName = ``name``, id = ``number`` + 1."""
        text = engine.render_chain_device(contig, name, name, number + 1)
        if len(text):
            self._file.write(memoryview(text))

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None
