"""The accept-table kernels of the SV-mix and host-chain engines (plan_kernels.h: k_accept_tables, k_accept_tables_ps) on word
windows built to sit on their borders, through ``Engine.accept_tables`` (msim_dbg_accept_tables: the engines' own launch
helpers over the caller's words).  Both kernels must give the same bytes, and rows below the class count must equal
``mixed_ref.accept_table`` -- the literal retry loop of randint, started at every word of the window (tied to the host's tables
and to CPython in test_mixed_ref_host.py).

Borders: the slot grid's 256-thread blocks ((n + 1) << lg_rows slots); a retry loop of exactly 62, 63 and 64 rejected words around
CHAIN_TABLE_REACH (probability 2^-63 on a genuine stream); an accepted word that is the window's last; a window that ends one word
before the accept (the word behind it accepts: a kernel that reads past the window finds it); entry n, the sentinel; n = 0; the
widest value a table entry holds at either entry layout (2^24 - 1 up to four classes, 2^23 - 1 beyond)."""
from __future__ import annotations

import numpy as np
import pytest

import mixed_ref as R
from mutation_simulator_amd import _ffi

pytestmark = pytest.mark.gpu

# class count -> widths: 1, 2, 3; 2^k and 2^k + 1; the widest value of the entry layout
WIDTHS = {
    1: [3],
    2: [1, 2],
    3: [3, 1 << 10, (1 << 10) + 1],
    4: [(1 << 24) - 1, 2, (1 << 16) + 1, 5],
    5: [(1 << 23) - 1, 1, 3, 1 << 8, (1 << 8) + 1],
    8: [1, 2, 3, 4, 5, (1 << 23) - 1, (1 << 12) + 1, 1 << 22],
}
P0 = 37                                                    # the window starts inside the words given


@pytest.fixture(scope="module")
def eng():
    with _ffi.Engine(0) as e:
        yield e


def _window(n: int, seed: int) -> np.ndarray:
    """TEMPERED words: P0 random ones, the window of n, 4 behind it.  In the window: runs of 62 / 63 / 64 rejected words with an
    accepted one behind each (where n has room), 5 rejected words and an accepted one as the window's LAST word; the first word
    behind the window is accepted by every class."""
    w = np.frombuffer(np.random.RandomState(seed).bytes(4 * (P0 + n + 4)), dtype="<u4").copy()
    win = w[P0:P0 + n]
    at = 10
    for run in (62, 63, 64):
        words = R.rejection_run(run, tail=0)
        if at + len(words) + 8 <= n:
            win[at:at + len(words)] = words
        at += len(words) + 15
    if n >= 6:
        win[n - 6:n] = R.rejection_run(5, tail=0)
    w[P0 + n] = 0x2A
    return w


def _check(eng, widths, n, seed):
    classes = [R.class_of(x) for x in widths]
    w = _window(n, seed)
    T, T_ps = eng.accept_tables(R.untemper(w), n, P0, classes)
    want = R.accept_table(w[P0:P0 + n], classes)
    assert T.shape == want.shape == (n + 1, 1 << R.lg_rows_of(len(classes)))
    assert np.array_equal(T, T_ps), "k_accept_tables and k_accept_tables_ps differ"
    assert np.array_equal(T[:, :len(classes)], want[:, :len(classes)])
    assert not T[:, len(classes):].any(), "a row beyond the class count was written"
    assert not T[n].any(), "entry n is the end-of-window sentinel"
    return T, want


@pytest.mark.parametrize("n1", [255, 256, 257, 513])
@pytest.mark.parametrize("n_classes", sorted(WIDTHS))
def test_tables_against_the_retry_loop(eng, n_classes, n1):
    """n + 1 = n1 positions: the slot count (n1 << lg_rows) lies on, one row below and one row above a multiple of 256."""
    widths = WIDTHS[n_classes]
    T, want = _check(eng, widths, n1 - 1, 100 * n_classes + n1)
    n = n1 - 1
    lg, vbits = R.lg_rows_of(n_classes), 24 if n_classes <= 4 else 23
    # the window holds what it was built for (entries of the reference, so a failure here is the test's own)
    assert want[10, 0] == ((63 << lg) << vbits)                      # 62 rejected, the 63rd word accepted: still in reach
    assert want[10 + 63 + 15, 0] == 0 and want[10 + 63 + 15 + 1, 0] == ((63 << lg) << vbits)      # 63 rejected: out of reach by one
    if n >= 10 + 78 + 79 + 65 + 8:
        assert want[10 + 78 + 79, 0] == 0 and want[10 + 78 + 79 + 1, 0] == 0 and want[10 + 78 + 79 + 2, 0] == ((63 << lg) << vbits)
    assert want[n - 1, 0] >> vbits == 1 << lg                        # the accepted word that is the window's last
    assert want[n - 6, 0] >> vbits == 6 << lg


@pytest.mark.parametrize("n_classes", sorted(WIDTHS))
def test_window_that_ends_one_word_before_the_accept(eng, n_classes):
    """The same words, the window one shorter: its last words are rejected ones, the accept lies just outside."""
    n = 300
    classes = [R.class_of(x) for x in WIDTHS[n_classes]]
    w = _window(n, 7 + n_classes)
    T, T_ps = eng.accept_tables(R.untemper(w), n - 1, P0, classes)
    want = R.accept_table(w[P0:P0 + n - 1], classes)
    assert np.array_equal(T, T_ps) and np.array_equal(T[:, :len(classes)], want[:, :len(classes)])
    assert not T[n - 6:, :].any(), "a loop ran past the end of the window"


@pytest.mark.parametrize("n_classes", sorted(WIDTHS))
@pytest.mark.parametrize("n", [0, 1, 62, 63, 64])
def test_short_windows(eng, n_classes, n):
    _check(eng, WIDTHS[n_classes], n, n + n_classes)


def test_widest_values_come_back_whole(eng):
    """A value of width - 1 at 2^24 - 1 (four classes) and 2^23 - 1 (five): every value bit of the entry set, the count above it."""
    for n_classes, bits in ((4, 24), (5, 23)):
        widths = WIDTHS[n_classes]
        sh, width = R.class_of(widths[0])
        w = np.full(P0 + 8 + 4, ((width - 2) << sh) | 0x1F, dtype=np.uint32)
        classes = [R.class_of(x) for x in widths]
        T, T_ps = eng.accept_tables(R.untemper(w), 8, P0, classes)
        lg = R.lg_rows_of(n_classes)
        assert np.array_equal(T, T_ps)
        assert T[0, 0] == (((1 << lg) << bits) | (width - 2)) and width - 2 == (1 << bits) - 3
        assert np.array_equal(T[:, :n_classes], R.accept_table(w[P0:P0 + 8], classes)[:, :n_classes])


def test_the_hook_refuses_what_the_planners_cannot_produce(eng):
    w = np.zeros(64, dtype=np.uint32)
    ok = [R.class_of(3)]
    eng.accept_tables(w, 10, 54, ok)                                 # p0 + n == the words given: the last one it may ask for
    for classes, n, p0 in ((ok, 11, 54), (ok, 10, 65), ([], 4, 0), (ok * 9, 4, 0), ([(29, 3)], 4, 0), ([(32, 0)], 4, 0),
                           ([(8, 1 << 24)], 4, 0), ([(9, 1 << 23)] + ok * 4, 4, 0)):
        with pytest.raises(_ffi.MsimError, match="msim_dbg_accept_tables: window outside the words given, or a class") as e:
            eng.accept_tables(w, n, p0, classes)
        assert e.value.code == _ffi.ERR_ARG                            # (returned in front of the first allocation and launch)
