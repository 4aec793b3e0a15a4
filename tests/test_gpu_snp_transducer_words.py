"""The SNP ti/tv transducer's kernels -- k_snp_maps_abs, k_snp_scan_cut_abs, the outcome pass -- on hand-built words, through
``Engine.snp_draws`` (msim_dbg_snp_draws), against ``tests/snp_ref.py``: every SnpLane word, every block map, the end position,
the flags and every outcome byte must be equal, and nothing outside the outcomes' bytes or the mapped blocks may be written.
The words go in through the inverse tempering, so the tempered values are the chosen ones (tests/snp_cases.py)."""
from __future__ import annotations

import numpy as np
import pytest

import snp_cases
import snp_ref as R
from mutation_simulator_amd import _ffi

pytestmark = pytest.mark.gpu

CASES = snp_cases.build()
GUARD = 0xEE


@pytest.fixture(scope="module")
def eng():
    with _ffi.Engine(0) as e:
        yield e


def check(res, t, ti_lim, start, K, aux_off, tables=None):
    lanes, maps = tables if tables is not None else R.block_tables(t, ti_lim)
    nb = lanes.shape[0]
    assert np.array_equal(res["lanes"][:nb], lanes)
    assert np.array_equal(res["maps"][:nb], maps)
    # the ragged tail is no block: the guard behind the mapped ones is untouched
    assert (res["lanes"][nb:].view(np.uint8) == GUARD).all() and (res["maps"][nb:].view(np.uint8) == GUARD).all()
    aux, end, flags = R.draws(t, ti_lim, start, K)
    assert res["flags"] == flags and res["end_pos"] == end
    got = res["aux"]
    assert got.shape[0] == aux_off + K + 16
    assert (got[:aux_off] == GUARD).all(), "bytes in front of the outcomes written"
    assert bytes(got[aux_off:aux_off + len(aux)]) == aux
    assert (got[aux_off + len(aux):] == GUARD).all(), "bytes behind the outcomes written"


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_words(eng, name):
    t, ti_lim, start, K, aux_off = CASES[name]
    check(eng.snp_draws(R.untemper(t), ti_lim, start, K, aux_off), t, ti_lim, start, K, aux_off)


def test_outcome_run_alignment(eng):
    t, ti_lim, sweep = snp_cases.alignment_sweep()
    raw, tables = R.untemper(t), R.block_tables(t, ti_lim)
    for aux_off, K in sweep:
        check(eng.snp_draws(raw, ti_lim, 0, K, aux_off), t, ti_lim, 0, K, aux_off, tables)


def test_refuses_what_it_cannot_run(eng):
    raw = np.zeros(R.BLOCK + 100, dtype=np.uint32)
    for kw in (dict(start=R.BLOCK, K=1), dict(start=0, K=0), dict(start=0, K=1, aux_off=64)):
        with pytest.raises(_ffi.MsimError):
            eng.snp_draws(raw, 1 << 53, **kw)
    with pytest.raises(_ffi.MsimError):
        eng.snp_draws(raw[:100], 1 << 53, 0, 1)            # not one whole block
