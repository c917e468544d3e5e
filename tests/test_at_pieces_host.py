"""Host tests (no GPU) of the piece schedule of the streamed A^T dy (csrc/host_factor_solve.h: at_piece_schedule, through the
debug entry ipm_debug_at_pieces).

The backward sweep of the grouped solve makes dy final in EVENTS: first the block steps behind the last full 1024-row group
(ragged block counts), then the groups nG-1 .. 0.  The pass over A reads dy by row chunks (rows_per_chunk rows each); a chunk may
run once ALL its rows are final.  Checked for every block count the GPU tests and the benchmark use, plus the edges: chunks that
straddle a group boundary (24 blocks: 96-row chunks), a ragged tail (18 blocks) and a tail smaller than one chunk (33 blocks: the
piece of the first event is empty)."""
import ctypes as C

import pytest

import interiorpointmethod_amd as ipm

NB, GS = 128, 8


def pieces_of(nblk, layout=(0, 0, 0, 0)):
    lib = ipm.load_library()
    lay = (C.c_int32 * 4)(*layout)
    count = C.c_int32(0)
    out = (C.c_int32 * (3 * 64))()
    assert lib.ipm_debug_at_pieces(nblk, lay, out, 64, C.byref(count)) == 0
    ev = [tuple(out[3 * e:3 * e + 3]) for e in range(count.value)]
    return tuple(lay), ev


def expected_events(nblk, gsz):
    """first final row of every sweep event, in sweep order"""
    nG = nblk // gsz
    first = [nG * gsz * NB] if nblk > nG * gsz else []
    return first + [g * gsz * NB for g in range(nG - 1, -1, -1)]


@pytest.mark.parametrize("nblk", [16, 18, 20, 24, 32, 40, 64, 33])
def test_pieces_tile_the_chunks_and_respect_the_sweep(nblk):
    (mp, gsz, rc, rpc), ev = pieces_of(nblk)
    assert mp == nblk * NB and gsz == GS and rc * rpc == mp            # the layout ipm_create gives a dense handle of nblk blocks
    assert [f for f, _, _ in ev] == expected_events(nblk, gsz)         # one piece per event, ordered as the sweep
    seen = []
    for first, c0, c1 in ev:
        assert 0 <= c0 <= c1 <= rc
        for by in range(c0, c1):
            assert by * rpc >= first, (nblk, first, by)                # every row of the chunk is final at this event
            seen.append(by)
    assert sorted(seen) == list(range(rc)) and len(set(seen)) == rc    # every row chunk in exactly one piece
    # ... and in the EARLIEST event that allows it (a chunk that straddles a boundary goes with the later event, no later)
    for e, (first, c0, c1) in enumerate(ev[1:], 1):
        for by in range(c0, c1):
            assert by * rpc < ev[e - 1][0]
    assert ev[-1][0] == 0 and ev[-1][1] == 0                           # the last event's piece starts at chunk 0: the main stream's
    assert ev[-1][2] > 0                                               # ... and is never empty


def test_edges_by_name():
    lay, ev = pieces_of(16)
    assert lay == (2048, 8, 32, 64) and ev == [(1024, 16, 32), (0, 0, 16)]                      # chunks aligned to the groups
    lay, ev = pieces_of(24)
    assert lay == (3072, 8, 32, 96)                                                            # 96-row chunks straddle 1024 and 2048
    assert ev == [(2048, 22, 32), (1024, 11, 22), (0, 0, 11)]
    lay, ev = pieces_of(18)
    assert lay == (2304, 8, 32, 72) and ev == [(2048, 29, 32), (1024, 15, 29), (0, 0, 15)]     # 2 groups + 2 block steps
    lay, ev = pieces_of(33)
    assert lay[3] == 132 and ev[0] == (4096, 32, 32)                                           # tail of 128 rows < one chunk: empty
    assert sum(1 for _, c0, c1 in ev if c1 == c0) == 1
    lay, ev = pieces_of(32)
    assert ev == [(3072, 24, 32), (2048, 16, 24), (1024, 8, 16), (0, 0, 8)]                    # the headline size: a quarter of A each


def test_a_layout_that_does_not_tile_the_rows_is_refused():
    # rc_chunks * rows_per_chunk != mp: no schedule (the caller then keeps the single pass)
    _, ev = pieces_of(16, (2048, 8, 32, 63))
    assert ev == []
    _, ev = pieces_of(16, (2048, 8, 1, 2048))                          # one chunk: everything waits for the last event
    assert ev == [(1024, 1, 1), (0, 0, 1)]
