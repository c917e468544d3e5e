"""Helpers of the guard-band tests (test knob IPM_TEST_ALLOC_GUARD, csrc/host_handle.h).  A feature test adds a
guarded cell in two lines:

    with guard_bands.guard(monkeypatch, 0xFF):
        ... build handles, run ...; guard_bands.assert_intact()          # after every operation
    guard_bands.assert_released()                                        # after the handles are closed

guard() sets the knob for the handles built inside it; assert_intact() compares every live band of the process NOW and fails with
the damaged ones (tag, side, first damaged offset, count); assert_released() asserts that nothing guarded is left alive and that
the violation log -- what dev_free and ipm_destroy found when they compared before releasing -- is empty."""
import contextlib

import numpy as np

from interiorpointmethod_amd import _lib

KNOB = "IPM_TEST_ALLOC_GUARD"
BAND = 131072                 # one 128 x 128 tile of doubles: a whole-tile overrun on either side lands inside a band
BYTES = (0xFF, 0x00)          # a stray 0.0 is invisible in a 0x00 band, a stray NaN / -1 in a 0xFF one
N_NVEC, N_MVEC = 11, 7        # csrc/host_handle.h: x s c rc d v q dxa dsa dx ds | y b rb t1 t2 dya dy
NVEC = ("x", "s", "c", "rc", "d", "v", "q", "dxa", "dsa", "dx", "ds")
MVEC = ("y", "b", "rb", "t1", "t2", "dya", "dy")


@contextlib.contextmanager
def guard(monkeypatch, byte, band=BAND):
    """The knob set (byte None: unset) for everything allocated inside the block."""
    with monkeypatch.context() as mp:
        if byte is None:
            mp.delenv(KNOB, raising=False)
        else:
            mp.setenv(KNOB, "%d:%d" % (band, byte))
        yield


def _short(b):
    return (b["tag"], "behind" if b["side"] else "before", b["first_bad"], b["bad_count"])


def assert_intact(handle=None, where=""):
    """Every live band of the handle (its C pointer), or of the process, holds its band byte."""
    bad = _lib.guard_check(handle)
    assert not bad, ("damaged guard bands " + where, [_short(b) for b in bad])


def assert_released(where=""):
    live, log = _lib.guard_list(), _lib.guard_log()
    assert not log, ("damage found when guarded memory was released " + where, [_short(b) for b in log])
    assert not live, ("guarded memory still alive " + where, [b["tag"] for b in live])


def tails(sv):
    """The padding tails [n, np) of the eleven n-vectors and [m, mp) of the seven m-vectors of a guarded solver whose workspace is a
    torch tensor, read through the listing's addresses: name -> bytes (an empty string where there is no padding)."""
    bands = {(b["tag"], b["side"]): b for b in sv.guard_bands()}
    base = sv._ws.data_ptr()
    out = {}
    for tag, names, count, rows in (("ws:nvec", NVEC, N_NVEC, sv.n), ("ws:mvec", MVEC, N_MVEC, sv.m)):
        b = bands[(tag, 1)]
        ld = b["inner_bytes"] // (8 * count)
        assert ld * 8 * count == b["inner_bytes"] and ld >= rows
        off = b["inner"] - base
        mem = sv._ws[off:off + b["inner_bytes"]].cpu().numpy().view(np.float64).reshape(count, ld)
        for i, nm in enumerate(names):
            out[nm] = mem[i, rows:].tobytes()
    return out


def nonzero_tails(sv):
    return sorted(nm for nm, t in tails(sv).items() if any(t))


class Checked:
    """A solver seen through the guard: after every method call `after(solver, method name)` runs (compare the bands, read the
    tails); attributes pass through.  What is written for a solver (an _observe of test_gpu_residue.py) runs on it unchanged."""

    def __init__(self, sv, after):
        object.__setattr__(self, "_sv", sv)
        object.__setattr__(self, "_after", after)

    def __getattr__(self, name):
        v = getattr(self._sv, name)
        if name.startswith("_") or not callable(v):
            return v

        def call(*a, **k):
            r = v(*a, **k)
            self._after(self._sv, name)
            return r
        return call

    def __setattr__(self, name, value):
        setattr(self._sv, name, value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._sv.close()
        return False
