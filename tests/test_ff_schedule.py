"""CPU tests of the work list of the fused formation + factorization (csrc/ff_schedule.h, exported host-only through
ipm_debug_ff_schedule): the list is replayed IN ORDER against the dependency rules the device kernel waits on
(csrc/form_factor.h) with the pivot chain advanced as far as its inputs allow before every item.  An item whose inputs
are not all produced by EARLIER items (or by chain steps that themselves only need earlier items) could leave a worker
waiting for a ticket nobody holds -- the one way the persistent launch could hang -- so that is what is asserted, together
with completeness: every tile receives its formation chunks, its base exactly once, every column of L up to its limit
exactly once and in order, and its panel solve exactly once, last."""
import ctypes as C

import numpy as np
import pytest

from ff_cases import KNOBS, MODELS, pair_chunks
from interiorpointmethod_amd import _lib

F, T, D = 0, 1, 2
NSTAGES = 512          # BK = 16 stages of the K = 8192 formation the debug entry point models
INIT, ADD_BASE, PANEL, SIG_DIAG0 = 1, 2, 4, 8


def schedule(nblk, q, workers):
    lib = _lib.load()
    cap = 200000
    items = (C.c_ubyte * (8 * cap))()
    count = C.c_int32(0)
    ntile = nblk * (nblk + 1) // 2
    tile_items = (C.c_int32 * ntile)()
    sim = (C.c_double * 2)()
    rc = lib.ipm_debug_ff_schedule(nblk, q, workers, items, cap, C.byref(count), tile_items, sim)
    assert rc == 0 and 0 < count.value <= cap
    raw = np.frombuffer(items, dtype=np.uint8)[:8 * count.value].reshape(-1, 8)
    arr = raw.astype(int)
    # F items carry their stage range [s0, s1) as two uint16 in the last four bytes: columns 8, 9 of the table
    st = raw[:, 4:8].copy().view(np.uint16).astype(int)
    arr = np.concatenate([arr, st], axis=1)
    return arr, np.array(tile_items[:]), (sim[0], sim[1])


def tid(i, c):
    return i * (i + 1) // 2 + c


def replay(nblk, q, items, tile_items, q_last=0):
    """Replay the list in order; returns the number of chain steps completed at the end.  q_last: IPM_FF_Q_LAST in effect."""
    ntile = nblk * (nblk + 1) // 2
    fcount = np.zeros(ntile, int)
    base = np.zeros(ntile, int)
    applied = np.zeros(ntile, int)
    paneled = np.zeros(ntile, int)
    nit = np.zeros(ntile, int)
    final = [[False] * (r + 1) for r in range(nblk)]            # final[r][j]: tile (r, j) is L
    potrf = [False] * nblk
    chain = {"k": 0, "phase": 0}
    limit = lambda i, c: (max(c - 1, 0) if i == c else c)                          # noqa: E731
    needs_panel = lambda i, c: i > c + 1                                           # noqa: E731
    done = lambda i, c: base[tid(i, c)] == 1 and applied[tid(i, c)] == limit(i, c) and nit[tid(i, c)] == tile_items[tid(i, c)]   # noqa: E731

    def advance():
        while chain["k"] < nblk:
            k = chain["k"]
            if chain["phase"] == 0:
                if k == 0 and not done(0, 0):
                    return
                potrf[k] = True                                    # (k > 0: its diagonal tile was completed by phase 2 of step k-1)
                if k + 1 >= nblk:
                    chain["k"] = nblk
                    return
                chain["phase"] = 1
            if chain["phase"] == 1:
                if not done(k + 1, k):
                    return
                final[k + 1][k] = True
                chain["phase"] = 2
            if chain["phase"] == 2:
                if not done(k + 1, k + 1):
                    return
                chain["k"], chain["phase"] = k + 1, 0

    fcover = {}
    # chunks per tile: q for ordinary tiles, more (shorter ones) for the block rows the chain needs first
    qtile = np.zeros(ntile, int)
    for (typ, i, c, qq, *_r) in items:
        if typ == F:
            for ii in (i, i + 1):
                if c <= ii < nblk:
                    qtile[tid(ii, c)] = max(qtile[tid(ii, c)], qq + 1)
    assert qtile.min() >= 1 and np.all(qtile[tid(nblk - 1, 0):] == min(q_last or q, 512)) or nblk <= 8
    for n, (typ, i, c, qq, j0, j1, flags, seq, s0, s1) in enumerate(items):
        if typ == D:                         # max diag(B) of row block i: the items the chain-in-kernel launch starts with
            assert n < nblk and i == n
            continue
        advance()
        if typ == T:
            assert c <= i < nblk
        t = tid(i, c) if c <= i else -1
        if typ == F:
            # a formation item covers the tile PAIR (i, c), (i + 1, c), i even (a half above the diagonal / below the matrix is dropped)
            assert i % 2 == 0 and c <= min(i + 1, nblk - 1) and 0 <= qq < 16 and 0 <= s0 <= s1 <= NSTAGES
            for ii in (i, i + 1):
                if c <= ii < nblk:
                    tt = tid(ii, c)
                    assert (tt, qq) not in fcover
                    fcover[(tt, qq)] = (s0, s1)
                    fcount[tt] += 1
            continue
        assert typ == T
        assert seq == nit[t] + 1, (n, i, c, "sequence")
        assert bool(flags & INIT) == (nit[t] == 0), (n, i, c, "INIT on the first item only")
        assert j0 == applied[t] and j0 <= j1 <= limit(i, c), (n, i, c, j0, j1)
        if flags & ADD_BASE:
            assert fcount[t] == qtile[t] and base[t] == 0, (n, i, c, "base before its chunks, or twice")
            base[t] = 1
        for j in range(j0, j1):
            assert final[i][j] and final[c][j], (n, i, c, j, "operand tile not final at this point of the list")
        applied[t] = j1
        if flags & PANEL:
            assert needs_panel(i, c) and base[t] == 1 and applied[t] == limit(i, c) and not paneled[t], (n, i, c)
            assert potrf[c], (n, i, c, "panel solve before its diagonal block is factored")
            paneled[t] = 1
            final[i][c] = True
        assert bool(flags & SIG_DIAG0) == (i == 0 and c == 0)
        nit[t] += 1
        assert not (paneled[t] and not (flags & PANEL)), (n, i, c, "an item after the panel solve")
    advance()
    for i in range(nblk):
        for c in range(i + 1):
            t = tid(i, c)
            cuts = sorted(fcover[(t, k)] for k in range(qtile[t]))    # the chunks tile the K loop exactly once
            assert cuts[0][0] == 0 and cuts[-1][1] == NSTAGES and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])), (i, c, cuts)
            assert fcount[t] == qtile[t] and base[t] == 1 and applied[t] == limit(i, c), (i, c)
            assert paneled[t] == (1 if needs_panel(i, c) else 0) and nit[t] == tile_items[t] >= 1, (i, c)
    return chain["k"]


@pytest.mark.parametrize("nblk,q,workers", [(3, 2, 4), (4, 4, 248), (8, 4, 31), (16, 4, 248), (32, 4, 248), (32, 8, 248),
                                            (32, 4, 120), (33, 3, 248), (64, 4, 248)])
def test_work_list_is_complete_and_every_item_follows_what_it_needs(built_lib, nblk, q, workers):
    items, tile_items, sim = schedule(nblk, q, workers)
    assert replay(nblk, q, items, tile_items) == nblk
    assert sim[0] > 0 and sim[1] > 0


def test_work_list_is_deterministic_and_its_simulated_time_beats_the_serial_path(built_lib):
    a, ta, sa = schedule(32, 4, 248)
    b, tb, sb = schedule(32, 4, 248)
    assert np.array_equal(a, b) and np.array_equal(ta, tb) and sa == sb
    # the model's own estimate at the headline size: formation + factorization well under the 4.3 ms of the serial path
    assert sa[0] < 4100.0, sa
    n_t = int((a[:, 0] == T).sum())
    assert n_t < 6000          # batching keeps the read-modify-write passes per tile small (pure right-looking: 5456 + 528)


# -------------------------------------------------------------------------------- every generator setting yields a valid list
# Each knob alone and the duration-model perturbations that the GPU order-invariance test runs, from 16 blocks (the default rule's
# lower end) to FF_MAX_NBLK = 96 (tile indices and column ranges of a work item are unsigned char fields, the largest values only
# occur there).  251 workers = the launch on 256 CUs (256 - 1 - FF_CRIT_WGS).
SETTINGS = KNOBS + [("IPM_FF_MODEL", m) for m in MODELS]


def _check_cuts(nblk, q, items, stagger=0.3, q_last=0):
    """The F items carry exactly the K-chunk cuts of the generator's formula (restated in ff_cases.pair_chunks)."""
    want = pair_chunks(nblk, q, NSTAGES, stagger=stagger, q_last=q_last)
    got = {}
    for (typ, i, c, qq, _j0, _j1, _fl, _sq, s0, s1) in items:
        if typ == F:
            got.setdefault((int(i), int(c)), {})[int(qq)] = (int(s0), int(s1))
    assert sorted(got) == sorted(want)
    for key, cuts in want.items():
        assert [got[key][k] for k in range(len(cuts))] == cuts, key


@pytest.mark.parametrize("nblk", [16, 33, 72, 96])
@pytest.mark.parametrize("var,val", SETTINGS, ids=[f"{k[7:]}={v}" for k, v in SETTINGS])
def test_every_generator_setting_gives_a_complete_list_in_dependency_order(built_lib, monkeypatch, var, val, nblk):
    monkeypatch.setenv(var, val)
    q, workers = 4, 251
    items, tile_items, sim = schedule(nblk, q, workers)
    q_last = int(val) if var == "IPM_FF_Q_LAST" else 0
    assert replay(nblk, q, items, tile_items, q_last=q_last) == nblk
    assert sim[0] > 0 and sim[1] > 0
    _check_cuts(nblk, q, items, stagger=float(val) if var == "IPM_FF_STAGGER" else 0.3, q_last=q_last)
    assert (items[:nblk, 0] == D).all() and not (items[nblk:, 0] == D).any()        # FF_D items, one per block, head every list
    t = items[items[:, 0] == T]
    if var == "IPM_FF_BATCH":                                                        # the bulk items really are that wide
        assert (t[:, 5] - t[:, 4]).max() == int(val)
    if var == "IPM_FF_TAIL":                                                         # the last `tail` columns one item each
        i, c = nblk - 1, nblk - 3
        cols = [(j0, j1) for (_ty, ii, cc, _q, j0, j1, *_r) in t if ii == i and cc == c]
        assert cols[-int(val):] == [(j, j + 1) for j in range(c - int(val), c)], cols


def test_chain_mode_0_is_refused_by_the_generator_too(built_lib, monkeypatch):
    """The structure IPM_FF_CHAIN_MODE=0 selected has been removed: the debug entry point refuses it as ipm_create does (asserted on
    the GPU in tests/test_gpu_ff_schedule.py) and models no other structure in its place."""
    lib = _lib.load()
    count = C.c_int32(0)
    monkeypatch.setenv("IPM_FF_CHAIN_MODE", "0")
    assert lib.ipm_debug_ff_schedule(16, 4, 251, None, 0, C.byref(count), None, None) != 0
    assert "IPM_FF_CHAIN_MODE=0" in lib.ipm_last_error(None).decode()
    monkeypatch.setenv("IPM_FF_CHAIN_MODE", "1")
    assert lib.ipm_debug_ff_schedule(16, 4, 251, None, 0, C.byref(count), None, None) == 0 and count.value > 0


def _producers(items, nblk):
    """For every T item (list position): the positions of the list items it waits for -- the formation chunks of its tile (when it
    adds the base), the tile's previous T item, and the items that finalise the L tiles (i, j), (c, j) it applies.  (A sub-diagonal
    tile (k+1, k) is finalised by the chain after the tile's last T item: that item stands in for it.)"""
    last_t, fpos = {}, {}
    for n, (typ, i, c, *_r) in enumerate(items):
        if typ == F:
            for ii in (i, i + 1):
                if c <= ii < nblk:
                    fpos.setdefault((ii, c), []).append(n)
        elif typ == T:
            last_t[(i, c)] = n
    prev, out = {}, {}
    for n, (typ, i, c, _q, j0, j1, flags, _seq, *_r) in enumerate(items):
        if typ != T:
            continue
        p = list(fpos[(i, c)]) if flags & ADD_BASE else []
        if (i, c) in prev:
            p.append(prev[(i, c)])
        for j in range(j0, j1):
            p += [last_t[(i, j)], last_t[(c, j)]]
        prev[(i, c)] = n
        out[n] = p
    return out


@pytest.mark.parametrize("nblk", [16, 32, 33])
def test_model_perturbations_reorder_the_list_without_changing_any_item(built_lib, monkeypatch, nblk):
    """What the GPU order-invariance test relies on: under each IPM_FF_MODEL perturbation the list for the handle's own
    (nblk, Q = 4, 251 workers, 512 stages = n of 8192) has a different ORDER but the same multiset of items -- type, tile, chunk,
    stage cuts, column range, flags, sequence number -- so every tile's arithmetic is unchanged and the results must be bitwise
    equal.  And EVERY perturbation, at every one of these block counts, puts some update item right behind (within two positions
    of) the last item it waits for, so that on the device each GPU shape really races a hand-off between neighbouring workers
    (3 to 8 such items per list today)."""
    base, tb, _ = schedule(nblk, 4, 251)
    key = lambda a: sorted(map(tuple, a.tolist()))                                 # noqa: E731
    for m in MODELS:
        monkeypatch.setenv("IPM_FF_MODEL", m)
        items, ti, _ = schedule(nblk, 4, 251)
        assert items.shape == base.shape and np.array_equal(ti, tb), m
        assert not np.array_equal(items, base), (m, "the perturbation does not reorder the list")
        assert key(items) == key(base), (m, "the perturbation changes an item")
        assert replay(nblk, 4, items, ti) == nblk
        gaps = [n - max(p) for n, p in _producers(items, nblk).items() if p]
        assert min(gaps) >= 1
        assert sum(1 for g in gaps if g <= 2) > 0, (m, nblk, "no update item right behind its producer")
