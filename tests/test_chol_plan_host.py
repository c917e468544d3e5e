"""Host tests (no GPU) of the step plan of the dense blocked Cholesky (csrc/chol_plan.h: chol_step_plan, through the debug entry
ipm_debug_chol_plan).  enqueue_factor (csrc/host_factor_solve.h) walks that plan and decides nothing, so what can go wrong in the
schedule -- a tile that misses a column's contribution or receives it twice, a reader that is not ordered behind its writer, a poll
whose count its signaller never reaches, a device-side wait enqueued in front of its signaller, a wide poller -- shows here.

launches() RESTATES the launch rule: it turns the records of a plan into the launches and stream operations enqueue_factor issues, in
enqueue order on the main and the bulk stream, each launch with the tiles it reads and writes and its workgroup count from the tile
shapes of its kernel.  replay() then walks them with the happens-before relation of the two streams: same stream and earlier, or the
reader waits for a counter or an event that the writer signals or records after its own work."""
import ctypes as C

import pytest

import interiorpointmethod_amd as ipm

NB = 128
WORDS = 15
FIELDS = ("potrf_panels", "rows", "rem", "shape", "g0", "gend", "kcols", "window", "crit_wait", "crit_count", "crit_flag", "poll_count",
          "bulk", "bulk_count", "bulk_event")
NARROW, WIDE, LOOKAHEAD = 0, 1, 2
NONE, COUNTER, EVENT = 0, 1, 2
MAIN, BULK = 0, 1
ALL_NBLK = (1, 2, 3, 4, 8, 9, 16, 18, 33, 47, 48, 49, 96, 128)


def plan_of(nblk, lookahead=1, polling=1, two_level=1, group_steps=0, ss_small_blocks=16, shift=0, env_last=None, m=0):
    lib = ipm.load_library()
    knobs = (C.c_int32 * 6)(lookahead, polling, two_level, group_steps, ss_small_blocks, shift)
    env = None if env_last is None else (C.c_int32 * nblk)(*env_last)
    totals = (C.c_int32 * 5)()
    words = (C.c_int32 * (WORDS * nblk))()
    assert lib.ipm_debug_chol_plan(nblk, m, knobs, env, totals, words, nblk) == 0
    steps = [dict(zip(FIELDS, words[WORDS * k:WORDS * (k + 1)])) for k in range(nblk)]
    return dict(zip(("lookahead", "polling", "gs", "counter_steps", "event_steps"), totals)), steps


def lower_tiles(rows, skip_first=0):
    return [(i, j) for i in rows for j in rows if j <= i][skip_first:]


def launches(nblk, totals, steps):
    """The operations of one factorization in enqueue order.  A launch: dict(op="launch", name, k, stream, wgs, panel=(rows, column)
    | update=(tiles, columns) | potrf=k, wait=None | (kind, id, count), signal=None | id).  Stream operations: dict(op="record" |
    "wait", stream, event)."""
    ops = []

    def launch(name, k, stream, wgs, wait=None, signal=None, **what):
        ops.append(dict(op="launch", name=name, k=k, stream=stream, wgs=wgs, wait=wait, signal=signal, **what))

    la = totals["lookahead"]
    sb = BULK if la else MAIN
    for k, s in enumerate(steps):
        launch("potrf", k, MAIN, 1, potrf=k)
        nb = s["rem"] // NB
        assert s["rem"] == nb * NB and 0 <= nb <= nblk - 1 - k
        if nb > 0:
            rows = list(range(k + 1, k + 1 + nb))
            cols = list(range(k - s["kcols"] + 1, k + 1))
            if s["shape"] == NARROW:                         # 32 x 128 panel strips, 64 x 64 update tiles
                launch("panel", k, MAIN, s["rem"] // 32, panel=(rows, k))
                launch("update", k, MAIN, (s["rem"] // 64) * (s["rem"] // 64 + 1) // 2, update=(lower_tiles(rows), cols))
            elif s["shape"] == WIDE:                         # 64 x 128 panel strips, 128 x 128 update tiles
                launch("panel", k, MAIN, s["rem"] // 64, panel=(rows, k))
                launch("update", k, MAIN, nb * (nb + 1) // 2, update=(lower_tiles(rows), cols))
            else:
                assert s["shape"] == LOOKAHEAD
                wait = None
                if s["crit_wait"] == COUNTER:
                    wait = ("counter", ("bulk", k - 1), s["crit_count"])
                elif s["crit_wait"] == EVENT:
                    ops.append(dict(op="wait", stream=MAIN, event=("bulk", k - 1)))
                launch("crit_panel", k, MAIN, NB // 32, wait=wait, signal=("crit", k) if s["crit_flag"] else None, panel=([k + 1], k))
                if not s["crit_flag"]:
                    ops.append(dict(op="record", stream=MAIN, event=("crit", k)))
                launch("crit_update", k, MAIN, 10, update=([(k + 1, k + 1)], cols))
                if not s["crit_flag"]:
                    ops.append(dict(op="wait", stream=sb, event=("crit", k)))
                if s["bulk"] != NONE:
                    wait = ("counter", ("crit", k), s["poll_count"]) if s["crit_flag"] else None
                    launch("bulk_panel", k, sb, (s["rem"] - NB) // 64, wait=wait, panel=(rows[1:], k))
                    if s["window"]:                          # one rectangular GEMM; its tiles above the diagonal are read by nobody
                        tiles = [(i, j) for i in rows[1:] for j in range(k + 1, k + 1 + s["window"])]
                        wgs = len(tiles)
                        tiles = [(i, j) for i, j in tiles if j <= i]
                    else:
                        tiles = lower_tiles(rows, skip_first=1)
                        wgs = len(tiles)
                    assert s["bulk_count"] == (wgs if s["bulk"] == COUNTER else 0)
                    launch("bulk_update", k, sb, wgs, signal=("bulk", k) if s["bulk"] == COUNTER else None, update=(tiles, cols),
                           window=s["window"])
        if s["bulk_event"]:
            ops.append(dict(op="record", stream=sb, event=("bulk", k)))
    if la:
        ops.append(dict(op="wait", stream=MAIN, event=("bulk", nblk - 2)))
    return ops


def replay(nblk, totals, steps, env_last=None):
    """Walks the operations and asserts the rules of the module docstring -> the launches."""
    ops = launches(nblk, totals, steps)
    inside = (lambda i, c: True) if env_last is None else (lambda i, c: i <= env_last[c])
    stream_hb = {MAIN: 0, BULK: 0}                 # bit set of the launches ordered before whatever the stream gets next
    event_hb, counter = {}, {}                     # event -> bit set at its record; counter -> (launch number, its bit set, workgroups)
    got = {}                                       # tile -> [columns applied (bit set), writers (bit set of launches)]
    panel_of, potrf_of = {}, {}
    done = []
    for o in ops:
        if o["op"] == "record":
            assert o["event"] not in event_hb
            event_hb[o["event"]] = stream_hb[o["stream"]]
            continue
        if o["op"] == "wait":
            assert o["event"] in event_hb, ("an event is waited for before it is recorded", o)
            stream_hb[o["stream"]] |= event_hb[o["event"]]
            continue
        n = len(done)
        hb = stream_hb[o["stream"]]
        if o["wait"]:
            _, cid, count = o["wait"]
            assert totals["polling"], "a counter in a plan without device polling"
            assert cid in counter, ("the signaller of a device-side wait is enqueued behind its waiter", o["name"], o["k"])     # enqueue order
            sn, shb, swgs = counter[cid]
            assert count == swgs, ("a poll waits for %d workgroups, its signaller has %d" % (count, swgs), o["name"], o["k"])   # counts
            assert o["wgs"] <= 64, ("a poller of %d workgroups" % o["wgs"], o["name"], o["k"])                                 # poller size
            hb |= shb | (1 << sn)
        before = lambda mask: mask & ~hb == 0      # noqa: E731   every launch of the set happens before this one

        def complete(i, j, who):
            """tile (i, j) holds the contribution of every column left of j that reaches row i, each applied once, all before `who`"""
            need = sum(1 << c for c in range(j) if inside(i, c))
            have, writers = got.get((i, j), (0, 0))
            assert have == need, ("tile (%d,%d) holds columns %s, needs %s" % (i, j, bin(have), bin(need)), who)
            assert before(writers), ("tile (%d,%d) is read before its updates are ordered" % (i, j), who)

        if "potrf" in o:
            k = o["potrf"]
            complete(k, k, o)
            potrf_of[k] = n
        elif "panel" in o:
            rows, c = o["panel"]
            assert before(1 << potrf_of[c]), o
            for i in rows:
                assert inside(i, c), ("a panel row below the envelope", i, c)
                assert (i, c) not in panel_of
                complete(i, c, o)
                panel_of[(i, c)] = n
        else:
            tiles, cols = o["update"]
            need_rows = {r for t in tiles for r in t}
            for c in cols:
                for r in need_rows:
                    assert inside(r, c), ("an update reads below the envelope", r, c)
                    assert (r, c) in panel_of and before(1 << panel_of[(r, c)]), ("an update reads a panel that is not ordered before it", r, c, o["name"], o["k"])
            mask = sum(1 << c for c in cols)
            for t in tiles:
                assert inside(t[0], t[1]) and t not in panel_of and t[0] not in potrf_of
                have, writers = got.get(t, (0, 0))
                assert have & mask == 0, ("a column reaches tile %s twice" % (t,), o["name"], o["k"])
                assert before(writers), ("two updates of tile %s are not ordered" % (t,), o["name"], o["k"])
                got[t] = (have | mask, writers | (1 << n))
            if o["signal"]:
                assert o["wgs"] <= 1024 or o["window"], ("a counter-signalling bulk update of %d workgroups" % o["wgs"], o["k"])
        if o["signal"]:
            assert totals["polling"] and o["signal"] not in counter
            counter[o["signal"]] = (n, hb, o["wgs"])
        stream_hb[o["stream"]] = hb | (1 << n)
        done.append(o)
    # the main stream ends behind everything, and every block column was factored and solved down to its envelope
    assert stream_hb[MAIN] == (1 << len(done)) - 1
    assert sorted(potrf_of) == list(range(nblk))
    assert set(panel_of) == {(i, c) for c in range(nblk) for i in range(c + 1, nblk) if inside(i, c)}
    if not totals["polling"]:
        assert not counter and all(s["crit_wait"] != COUNTER and not s["crit_flag"] and s["bulk"] != COUNTER for s in steps)
    return done


def check_schedule_words(nblk, totals, steps, lookahead, two_level=1, group_steps=0, envelope=False):
    la = bool(lookahead) and nblk > 2
    assert totals["lookahead"] == int(la)
    assert totals["counter_steps"] + totals["event_steps"] == sum(1 for s in steps if s["bulk"] != NONE)
    assert totals["counter_steps"] == sum(1 for s in steps if s["bulk"] == COUNTER)
    if not la or envelope or not two_level:
        want = 1
    elif group_steps > 0:
        want = group_steps if nblk >= 8 else 1
    else:
        want = 4 if nblk >= 96 else 3 if nblk >= 48 else 1
    assert totals["gs"] == want
    for k, s in enumerate(steps):
        assert (s["g0"], s["gend"]) == ((k // want * want, min(k // want * want + want, nblk)) if want > 1 else (k, k + 1))


@pytest.mark.parametrize("polling", [0, 1])
@pytest.mark.parametrize("lookahead", [0, 1])
@pytest.mark.parametrize("nblk", ALL_NBLK)
def test_default_plans_cover_every_tile_in_order(nblk, lookahead, polling):
    totals, steps = plan_of(nblk, lookahead, polling)
    assert totals["polling"] == int(bool(lookahead) and nblk > 2 and bool(polling))
    done = replay(nblk, totals, steps)
    check_schedule_words(nblk, totals, steps, lookahead)
    if not totals["lookahead"]:                              # one stream: wide tiles while more than 16 blocks trail, then narrow ones
        assert [s["shape"] for s in steps[:-1]] == [WIDE if nblk - 1 - k > 16 else NARROW for k in range(nblk - 1)]
        assert all(o["stream"] == MAIN for o in done)
    elif totals["polling"]:
        assert any(o["wait"] for o in done) == (nblk > 2)


@pytest.mark.parametrize("polling", [0, 1])
@pytest.mark.parametrize("nblk", [4, 8, 9, 16, 18])
@pytest.mark.parametrize("gs", [2, 3, 4])
def test_forced_groups(nblk, gs, polling):
    """4 blocks: below the 8 from which a forced group size counts; 8, 9, 16, 18: every gs both divides one of them and leaves a ragged
    last group in another (9 = 4 + 4 + 1: a last group of one column)."""
    totals, steps = plan_of(nblk, 1, polling, group_steps=gs)
    replay(nblk, totals, steps)
    check_schedule_words(nblk, totals, steps, 1, group_steps=gs)
    if nblk >= 8:
        assert any(s["window"] for s in steps) and any(s["kcols"] == gs for s in steps)
        assert all(s["kcols"] == (k - s["g0"] + 1 if k + 1 == s["gend"] else 1) for k, s in enumerate(steps) if s["rem"] > 0)


def test_two_level_switch_and_lockstep_tiles():
    totals, steps = plan_of(49, 1, 1, two_level=0)
    replay(49, totals, steps)
    check_schedule_words(49, totals, steps, 1, two_level=0)
    totals, steps = plan_of(33, 0, 0, ss_small_blocks=1 << 20)          # a lockstep handle: one tile shape at every step
    replay(33, totals, steps)
    assert all(s["shape"] == NARROW for s in steps)


def banded(nblk, width=2):
    return [min(k + width, nblk - 1) for k in range(nblk)]


def staircase(nblk, tread=3):
    """Diagonal blocks of `tread` block columns, every third one coupled to the next: columns with nothing below their diagonal block."""
    last = [min((k // tread) * tread + tread - 1, nblk - 1) for k in range(nblk)]
    for k in range(0, nblk, 3 * tread):
        last[k:k + tread] = [min(k + 2 * tread - 1, nblk - 1)] * len(last[k:k + tread])
    out, hi = [], 0
    for v in last:
        hi = max(hi, v)
        out.append(hi)
    return out


@pytest.mark.parametrize("polling", [0, 1])
@pytest.mark.parametrize("lookahead", [0, 1])
@pytest.mark.parametrize("shape", ["banded", "staircase"])
@pytest.mark.parametrize("nblk", [3, 9, 18, 49])
def test_envelope_plans_stay_inside_the_envelope(nblk, shape, lookahead, polling):
    env = banded(nblk) if shape == "banded" else staircase(nblk)
    assert all(env[k] >= k for k in range(nblk)) and env == sorted(env)
    totals, steps = plan_of(nblk, lookahead, polling, env_last=env)
    assert [s["rem"] for s in steps] == [(env[k] - k) * NB for k in range(nblk)]
    if shape == "staircase" and nblk > 3:
        assert any(s["rem"] == 0 for s in steps[:-1])
    replay(nblk, totals, steps, env_last=env)
    check_schedule_words(nblk, totals, steps, lookahead, envelope=True)


@pytest.mark.parametrize("shift", [0, 1])
def test_potrf_panels_follow_the_rows_of_the_lp(shift):
    m = 9 * NB - 100                                                    # 28 rows of the LP in the last block: two 16-wide panels
    totals, steps = plan_of(9, 1, 1, shift=shift, m=m)
    assert [s["rows"] for s in steps] == [m - k * NB for k in range(9)]
    assert [s["potrf_panels"] for s in steps] == [8] * 8 + [8 if shift else 2]
    totals, steps = plan_of(18, 1, 1, m=16 * NB + 1)                    # a block of padding only: one panel
    assert [s["potrf_panels"] for s in steps[15:]] == [8, 1, 1] and steps[17]["rows"] == 1 - NB


def test_both_sides_of_the_polling_bounds():
    """49 blocks in groups of 3: deferred updates above and below 1024 workgroups, bulk panels above and below 64."""
    totals, steps = plan_of(49, 1, 1)
    full = [s for s in steps if s["bulk"] != NONE and not s["window"]]
    wgs = lambda s: (s["rem"] // NB) * (s["rem"] // NB + 1) // 2 - 1          # noqa: E731
    assert any(s["bulk"] == EVENT for s in full) and any(s["bulk"] == COUNTER for s in full)
    assert all((s["bulk"] == COUNTER) == (wgs(s) <= 1024) for s in full)
    assert all(s["bulk"] == COUNTER for s in steps if s["window"])
    assert all(bool(s["crit_flag"]) == (NB < s["rem"] and (s["rem"] - NB) // 64 <= 64) for s in steps)
    assert any(s["crit_flag"] for s in steps) and any(not s["crit_flag"] and s["rem"] > NB for s in steps)
