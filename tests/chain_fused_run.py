"""The three-way comparison of tests/test_gpu_chain_fused.py (host planner, the three chain launches, the fused launch) in a
process of its own, for what libmsim reads ONCE per process: ``MSIM_AHEAD_FIRST`` is a function-local static, so a test that sets
it inside a suite run never reaches the library.  With it set a context's FIRST sample is an anchored window too -- the start is
exact (``lo == H``: no head blocks, ``est.v == 0``) -- and takes the fused launch like the others.

    MSIM_AHEAD_FIRST=1 python tests/chain_fused_run.py RESULT.json N_CONTIGS

writes {"verdict": "ok" | what differed, "n_fused": ..., "snp_samples_ahead": ..., "n_contigs": ...} and stops at the first library
error (nothing runs on a device after a fault)."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "mutation-simulator_amd", ROOT / "tests", ROOT / "tests" / "golden"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import numpy as np  # noqa: E402

from test_gpu_chain_fused import _big, _three_ways  # noqa: E402
from test_gpu_sampler import _params  # noqa: E402


class _Env:
    """What ``_three_ways`` asks of pytest's monkeypatch."""

    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k):
        os.environ.pop(k, None)


def main():
    out, n_contigs = Path(sys.argv[1]), int(sys.argv[2])
    res = {"n_contigs": n_contigs}
    try:
        st, n_fused = _three_ways(_Env, _big(np.random.RandomState(5), n_contigs), _params(titv=2.0), (9, 9))
        res.update(verdict="ok", n_fused=n_fused, snp_samples_ahead=st["snp_samples_ahead"])
    except AssertionError as e:
        res["verdict"] = f"differs: {str(e)[:500]}"
    out.write_text(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
