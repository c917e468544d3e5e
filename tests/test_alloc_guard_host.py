"""Host tests (no GPU) of the guard-band knob IPM_TEST_ALLOC_GUARD (csrc/host_handle.h): the three sizing calls with
the knob unset and set, the layout of the guarded workspace (ipm_debug_guard_layout, the listing's host part), the band comparator
(ipm_debug_guard_compare: what ipm_debug_guard_check, dev_free and ipm_destroy compare with) and the malformed values of the knob."""
import ctypes as C

import numpy as np
import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib

import guard_bands as GB

REGIONS = 20          # make_layout: A B inv nvec mvec atp part det sc fixed hist snap slab order rowptr colptr colind rowind rval cval
# (m, n, nnz, flags) -> what ipm_workspace_bytes, ipm_workspace_bytes_csc (sparse shapes only) and ipm_workspace_bytes_opts returned
# before the knob existed; 2048 / 2176 / 7296 rows are 16, 17 and 57 blocks (57: mp is padded to 64 blocks, whole groups of 8)
SHAPES = {
    (1, 1, 0, 0): (67552000, None, 67552000),
    (128, 256, 0, 0): (67771648, None, 67771648),
    (130, 257, 0, 0): (68710144, None, 68710144),
    (2048, 4096, 0, 0): (171575040, None, 171575040),
    (300, 513, 2000, 0): (70662912, 68922624, 68922624),
    (300, 513, 2000, _lib.FLAG_SPARSE_FACTOR): (70662912, 68922624, 240896),
    (2048, 64, 0, 0): (104063232, None, 104063232),
    (2176, 64, 0, 0): (108593408, None, 108593408),
    (7296, 64, 0, 0): (617217792, None, 617217792),
}


def _opts(nnz, flags):
    o = _lib.Options()
    ipm.load_library().ipm_default_options(C.byref(o))
    o.sparse_nnz, o.flags = nnz, flags
    return o


def _sizes(m, n, nnz, flags):
    lib, b, out = ipm.load_library(), C.c_size_t(0), []
    assert lib.ipm_workspace_bytes(m, n, C.byref(b)) == _lib.IPM_OK
    out.append(b.value)
    if nnz:
        assert lib.ipm_workspace_bytes_csc(m, n, nnz, C.byref(b)) == _lib.IPM_OK
    out.append(b.value if nnz else None)
    o = _opts(nnz, flags)
    assert lib.ipm_workspace_bytes_opts(m, n, C.byref(o), C.byref(b)) == _lib.IPM_OK
    out.append(b.value)
    return tuple(out)


def _layout(m, n, nnz, flags):
    lib, o = ipm.load_library(), _opts(nnz, flags)
    out, count, total, band = (_lib.GuardBand * 32)(), C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
    assert lib.ipm_debug_guard_layout(m, n, C.byref(o), out, 32, C.byref(count), C.byref(total), C.byref(band)) == _lib.IPM_OK
    return [out[i].as_dict() for i in range(count.value)], total.value, band.value


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sizes_unset_are_the_old_ones_and_set_add_the_bands(monkeypatch, shape):
    with GB.guard(monkeypatch, None):
        assert _sizes(*shape) == SHAPES[shape]
        regions, total, band = _layout(*shape)
        assert band == 0 and total == SHAPES[shape][2] and len(regions) == REGIONS and all(r["bytes"] == 0 for r in regions)
    for byte in GB.BYTES:
        with GB.guard(monkeypatch, byte):
            got = _sizes(*shape)
        assert [g - w for g, w in zip(got, SHAPES[shape]) if w is not None] == [GB.BAND * (REGIONS + 1)] * (3 if shape[2] else 2)
    with GB.guard(monkeypatch, None):
        assert _sizes(*shape) == SHAPES[shape]                 # read at every call: unset again, the old sizes again


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_guarded_layout(monkeypatch, shape):
    with GB.guard(monkeypatch, None):
        plain, _, _ = _layout(*shape)
    with GB.guard(monkeypatch, 0xFF):
        regions, total, band = _layout(*shape)
        assert total == _sizes(*shape)[2]
    assert band == GB.BAND and len(regions) == REGIONS
    assert [(r["tag"], r["inner_bytes"]) for r in regions] == [(r["tag"], r["inner_bytes"]) for r in plain]      # the same regions, the same sizes
    assert regions[0]["inner"] == band                                           # a band before the first region
    for r, nxt in zip(regions, regions[1:] + [None]):
        assert r["inner"] % 256 == 0 and r["byte"] == 0xFF
        end = r["inner"] + r["inner_bytes"]
        limit = nxt["inner"] if nxt else total
        assert limit - end >= band, (r["tag"], "less than a band to the next region (a zero-length one included) or to the end")
        assert r["bytes"] == limit - end and limit - end < band + 256          # the band behind: from the last byte asked for, rounding included
    assert regions[-1]["inner"] + regions[-1]["inner_bytes"] + band <= total    # the band behind the last lies inside the total
    # the guarded regions lie in the order and at the distances of the plain ones, one band more per region
    assert [r["inner"] - (i + 1) * band for i, r in enumerate(regions)] == [r["inner"] for r in plain]


def _compare(buf, byte):
    first, count = C.c_int64(-7), C.c_int64(-7)
    raw = buf.tobytes()
    assert ipm.load_library().ipm_debug_guard_compare(raw, len(raw), byte, C.byref(first), C.byref(count)) == _lib.IPM_OK
    return first.value, count.value


@pytest.mark.parametrize("byte", GB.BYTES)
def test_band_comparator(byte):
    n = 4096
    clean = np.full(n, byte, dtype=np.uint8)
    assert _compare(clean, byte) == (-1, 0)
    for off in (0, n - 1, 1000):
        b = clean.copy()
        b[off] ^= 0x01
        assert _compare(b, byte) == (off, 1)
    b = clean.copy()
    b[[7, 9, n - 1]] = byte ^ 0x80
    assert _compare(b, byte) == (7, 3)
    assert _compare(clean, byte ^ 0xFF) == (0, n)                               # the other band byte: every byte is damage
    # a block's two bands are two records: damage before and behind is reported separately
    left, right = clean.copy(), clean.copy()
    left[n - 1] ^= 0xFF
    assert _compare(left, byte) == (n - 1, 1) and _compare(right, byte) == (-1, 0)
    right[0] ^= 0xFF
    left[n - 1] = byte
    assert _compare(left, byte) == (-1, 0) and _compare(right, byte) == (0, 1)
    lib = ipm.load_library()
    assert lib.ipm_debug_guard_compare(None, 4, byte, None, None) == -1 and lib.ipm_debug_guard_compare(b"abcd", 4, 256, None, None) == -1


@pytest.mark.parametrize("value", ["", "1000", "100:255", "-131072", "-256:0", "band", "131072x", "131072:", "131072:256", "131072:-1", "131072:ff",
                                   "131072:0:0", "0", "0:255", "1e5", " "])
def test_malformed_knob_is_the_knob_unset(monkeypatch, value):
    shape = (130, 257, 0, 0)
    monkeypatch.setenv(GB.KNOB, value)
    assert _sizes(*shape) == SHAPES[shape]
    assert _layout(*shape)[2] == 0


def test_knob_forms(monkeypatch):
    shape = (130, 257, 0, 0)
    for value, band, byte in (("256", 256, 0xFF), ("256:0", 256, 0), ("131072:255", 131072, 255), ("512:7", 512, 7)):
        monkeypatch.setenv(GB.KNOB, value)
        regions, total, got = _layout(*shape)
        assert got == band and total == SHAPES[shape][0] + band * (REGIONS + 1) and {r["byte"] for r in regions} == {byte}


def test_no_live_band_and_an_empty_log_without_a_device():
    assert _lib.guard_list() == [] and _lib.guard_check() == [] and _lib.guard_log() == []
