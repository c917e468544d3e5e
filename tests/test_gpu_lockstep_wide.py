"""GPU tests (-m gpu) of the LOCKSTEP BATCH at 64 LPs per launch and beyond (csrc/lockstep.h, host_lockstep.h, lockstep_merge.h).

Every wrapper kernel of the batch finds its LP with LS_ENTER: each wave loads recs[lane].start for lane < count, ballots
start <= blockIdx.x and takes popcount - 1; up to LS_MAX_GROUP = 64 LPs share a launch, a step of more is cut into launches of 64.
The other GPU tests put two to six LPs into a batch, so lanes 32 .. 63 of that look-up, a full launch, the 64 + k cut, large
`start` entries and a schedule re-merged while the active count crosses 64 ran nowhere.  Here they do (cells:
tests/lockstep_wide_cases.py; what each is, and which kernel types no wide launch covers: its docstring).

The oracle is the project's own claim: an LP of a batch ends BIT-IDENTICAL to the same handle solved alone with ipm_solve (status,
iteration count, statistics, every history record, (x, y, s), the certificate).  The single-LP kernels are held to the longdouble
oracle elsewhere (test_gpu_iteration_edges.py, test_gpu_late_iteration.py); four LPs of two66 -- batch positions 0, 32, 63 and 64
-- are held to it here as well, with the bounds of test_gpu_iteration_edges.py.

No test can pass without reaching its edge: LockstepBatch.schedule() (ipm_debug_batch_schedule) returns the launches of the last
step, and each test asserts that they are what the CPU merge (ipm_debug_ls_merge) makes of the LPs' own programs -- recorded
beforehand from batches of ONE handle each -- launch by launch: type, member count (64, then the rest), packed grid = the sum of
the members' own grids, dynamic LDS = their maximum.

Wall time per test on an MI355X (pytest --durations, whole file 5.9 s): the 70 `two` handles of the module 1.8 s (set-up of the
first test that uses them), six66 1.4 s, three66 0.5 s, mixed66 0.3 s, detect66 0.3 s, two66 with its four oracle LPs 0.2 s, sparse66
0.2 s, the crossing, both late joins and the small-cap test below 0.1 s each (their solves alone are shared with two66's handles).
Schedules seen there: two66 56 launches (a program of 28, each cut 64 + 2), three66 70 (35), six66 120 (60), detect66 56, sparse66 54,
mixed66 95 (75 merged steps for a longest program of 60, 20 of them cut).
"""
import ctypes as C

import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib

import iteration_oracle as IO
import lockstep_wide_cases as W
from test_gpu_iteration_edges import _assert_all, _bound, _srel
from test_lockstep_merge import merge

pytestmark = pytest.mark.gpu

G = W.LS_MAX_GROUP
STAT_KEYS = ("status", "iterations", "pivots_fixed", "auto_regularized", "objective", "rp_norm", "rd_norm", "gap")


def _make(p, **opts):
    """A lockstep handle of the LP; check_every = 1: a batch step is one iteration (a solve's result does not depend on it)."""
    return ipm.IpmSolver(p.A, p.b, p.c, lockstep=True, factor="dense", check_every=1, **opts)


def _hex(v):
    return float(v).hex() if isinstance(v, float) else v


def _result(sv, st):
    """Everything a solve leaves behind, in a form that compares bit for bit (NaN included)."""
    cert = sv.certificate()
    if cert is not None:
        cert = tuple(_hex(cert[k]) for k in ("kind", "k", "normalization", "violation")) + tuple(cert[k].tobytes() for k in ("x", "y", "z"))
    return dict(stats=tuple(_hex(st[k]) for k in STAT_KEYS), hist=[tuple(_hex(v) for v in rec.values()) for rec in sv.history()],
                bits=[v.tobytes() for v in sv.get_state()], cert=cert)


def _alone(sv, p, cap):
    sv.set_state(*p.state())
    return _result(sv, sv.solve(tol=1e-8, max_iter=cap))


def _program(sv, p):
    """The handle's own launch program [(type, grid, lds)]: the schedule of a batch of this one handle."""
    sv.set_state(*p.state())
    with ipm.LockstepBatch(tol=1e-8, max_iter=1) as bt:
        bt.add(sv)
        bt.step()
        sch = bt.schedule()
        for _ in range(3):
            if bt.active:
                bt.step()
        assert bt.active == 0
    assert sch and all(st["members"] == 1 for st in sch)
    return [(st["type"], st["blocks"], st["lds"]) for st in sch]


def _check_schedule(sch, progs):
    """The launches of one step of a batch whose active LPs have the programs `progs` (batch order): exactly what the CPU merge
    makes of their type lists, with the packed grids and the LDS of the members.  -> the plan [(type, [(LP, position)])]."""
    plan = merge([[t for t, _, _ in pr] for pr in progs], max_group=G)
    assert [(st["type"], st["members"]) for st in sch] == [(t, len(mem)) for t, mem in plan]
    for st, (t, mem) in zip(sch, plan):
        assert 1 <= st["members"] <= G
        assert st["blocks"] == sum(progs[i][j][1] for i, j in mem), (W.LS_TYPES[t], st)
        assert st["lds"] == max(progs[i][j][2] for i, j in mem), (W.LS_TYPES[t], st)
    return plan


def _assert_cut(sch, types, rest, what):
    """Every type of `types` is launched at least once with exactly 64 members, and behind EVERY launch of 64 members comes the
    same type with the `rest` members that did not fit."""
    for t in sorted(types):
        assert any(st["type"] == t and st["members"] == G for st in sch), (what, W.LS_TYPES[t])
    for k, st in enumerate(sch):
        if st["members"] == G:
            assert k + 1 < len(sch) and (sch[k + 1]["type"], sch[k + 1]["members"]) == (st["type"], rest), (what, W.LS_TYPES[st["type"]], k)


def _types(prog):
    return [t for t, _, _ in prog]


def _one_template(progs, what):
    """The LPs of a family differ in their grids, never in the sequence of their launches."""
    for k, pr in enumerate(progs):
        assert _types(pr) == _types(progs[0]), (what, k)


def _run_batch(svs, lps, caps):
    """All handles into one LockstepBatch (cap per handle), stepped to the end -> [(active before the step, schedule, finished)]."""
    for sv, p in zip(svs, lps):
        sv.set_state(*p.state())
    trace = []
    with ipm.LockstepBatch(tol=1e-8) as bt:
        for sv, cap in zip(svs, caps):
            bt.max_iter = cap
            bt.add(sv)
        for _ in range(max(caps) + 3):
            if not bt.active:
                break
            before = bt.active
            done = bt.step()
            trace.append((before, bt.schedule(), done))
        assert bt.active == 0
    return trace


def _assert_same(what, sv, ref):
    got = _result(sv, sv.stats)
    for k in ("stats", "hist", "bits", "cert"):
        assert got[k] == ref[k], (what, k, got[k] if k != "bits" else "...", ref[k] if k != "bits" else "...")


class Family:
    """Handles of one family with what the tests share about them: the solve alone (per iteration cap) and the launch program."""

    def __init__(self, entries, opts=lambda family: {}):
        self.lps = [W.lp(f, s) for f, s in entries]
        self.svs = []
        try:
            for (f, _), p in zip(entries, self.lps):
                self.svs.append(_make(p, **opts(f)))
        except Exception:
            self.close()
            raise
        self._alone, self._prog = {}, {}

    def close(self):
        for sv in self.svs:
            sv.close()

    def alone(self, i, cap):
        if (i, cap) not in self._alone:
            self._alone[(i, cap)] = _alone(self.svs[i], self.lps[i], cap)
        return self._alone[(i, cap)]

    def program(self, i):
        if i not in self._prog:
            self._prog[i] = _program(self.svs[i], self.lps[i])
        return self._prog[i]


@pytest.fixture(scope="module")
def two():
    """The 70 `two` handles of join70 (two66, cross64 and cap5 are its first 66, 67 and 5), created once for the module."""
    fam = Family(W.CELLS["join70"])
    yield fam
    fam.close()


def _assert_family(fam, i, family):
    sv = fam.svs[i]
    sch = sv.schedule()
    gsz, ng = W.groups(family)
    assert ipm.lockstep_eligible(sv) and sch["fused_small"] == 0 and sv.factor == "dense" and not sv.bounded
    assert sch["blocks"] == W.BLOCKS[family] and sch["grouped_trsv"] == (1 if gsz else 0) and sch["group_blocks"] == gsz
    assert (sch["blocks"] // gsz if gsz else 0) == ng
    types = {W.LS_TYPES[t] for t, _, _ in fam.program(i)}
    print("TYPES %s (%d x %d): %d launches, %s" % (family, sv.m, sv.n, len(fam.program(i)), " ".join(sorted(types))))
    must, must_not = W.MUST[family]
    assert must <= types and not (must_not & types), (family, sorted(must - types), sorted(must_not & types))
    return types


def _wide(name, fam, idx, families, detect=False):
    """The body of the wide test for the handles fam.svs[idx]: programs, alone, the batch through LockstepBatch (for the schedule)
    and through solve_lockstep (ipm_solve_batch), both bit-identical to alone."""
    svs, lps = [fam.svs[i] for i in idx], [fam.lps[i] for i in idx]
    n = len(svs)
    assert n == 66
    progs = [fam.program(i) for i in idx]
    per_family = {}
    for k, i in enumerate(idx):
        f = W.base(families[k])
        if f not in per_family:
            names = _assert_family(fam, i, f)
            if detect:
                assert {"PREPARE_DETECT", "STOP_TEST_DETECT"} <= names and not ({"PREPARE", "STOP_TEST"} & names)
            per_family[f] = {W.LS[nm] for nm in names}
        assert {t for t, _, _ in progs[k]} == per_family[f], (name, k)
    ref = [fam.alone(i, 2) for i in idx]
    fired = [r["cert"] is not None for r in ref]
    if detect:
        assert fired == ["+" in f for f in families]                  # two in three are built to fire, at k = 0
        assert [r["stats"][:2] for r in ref] == [{"two": (2, 2), "two+primal": (5, 0), "two+dual": (6, 0)}[f] for f in families]
    else:
        assert not any(fired) and all(r["stats"][:2] == (2, 2) and len(r["hist"]) == 2 for r in ref)

    trace = _run_batch(svs, lps, [2] * n)
    assert trace[0][0] == n and sorted(id(s) for t in trace for s in t[2]) == sorted(id(s) for s in svs)
    active = list(range(n))
    for before, sch_k, done in trace:                                  # every step's schedule, as LPs leave (detect66: the fired ones)
        assert before == len(active)
        _check_schedule(sch_k, [progs[i] for i in active])
        gone = {id(s) for s in done}
        active = [i for i in active if id(svs[i]) not in gone]
    assert not active
    sch = trace[0][1]
    if len(per_family) == 1:
        _one_template(progs, name)
        cut_types = set(_types(progs[0]))                              # every launch of the program is cut 64 + 2
    else:
        # the programs begin alike (residuals, stop test, formation, the first pivot block): those launches serve all 66
        first = [_types(progs[[W.base(f) for f in families].index(g)]) for g in per_family]
        shared = 0
        while all(shared < len(p) for p in first) and len({p[shared] for p in first}) == 1:
            shared += 1
        assert shared >= 4
        cut_types = set(first[0][:shared])
    _assert_cut(sch, cut_types, n - G, name)
    print("SCHEDULE %s: %d launches, largest %d members, at 64 members: %s" % (
        name, len(sch), max(st["members"] for st in sch), " ".join(sorted({W.LS_TYPES[st["type"]] for st in sch if st["members"] == G}))))
    if len(per_family) > 1:
        # the three programs side by side: a type only one family has is launched once for all of that family's LPs, and the
        # schedule is the longest program plus what the CPU merge says the others add, plus one launch per step that had to be cut
        count = {f: sum(W.base(x) == f for x in families) for f in per_family}
        for f, types in per_family.items():
            own = types - set.union(*[t for g, t in per_family.items() if g != f])
            for t in own:
                assert all(st["members"] == count[f] for st in sch if st["type"] == t), (name, f, W.LS_TYPES[t])
        whole = merge([[t for t, _, _ in pr] for pr in progs], max_group=1 << 20)
        longest = max(len(pr) for pr in progs)
        cut = sum(len(mem) > G for _, mem in whole)
        print("MIXED %s: longest program %d, merged %d steps, %d of them cut -> %d launches" % (name, longest, len(whole), cut, len(sch)))
        assert len(sch) <= longest + (len(whole) - longest) + cut
    for k, (sv, r) in enumerate(zip(svs, ref)):
        _assert_same("%s[%d] LockstepBatch" % (name, k), sv, r)

    for sv, p in zip(svs, lps):
        sv.set_state(*p.state())
    stats = ipm.solve_lockstep(svs, tol=1e-8, max_iter=2)
    for k, (sv, st, r) in enumerate(zip(svs, stats, ref)):
        assert sv.stats is st
        _assert_same("%s[%d] solve_lockstep" % (name, k), sv, r)


def test_wide_batch_is_bit_identical_two66(two):
    idx = list(range(66))
    _wide("two66", two, idx, [f for f, _ in W.CELLS["two66"]])
    # four LPs against the longdouble oracle: lane 0, the first lane of the upper half-wave, the last lane, the first LP of the
    # split-off launch -- the comparison of test_gpu_iteration_edges.test_lockstep_pair_past_the_stride, its bounds
    for pos in W.ORACLE_POSITIONS:
        fam, seed = W.CELLS["two66"][pos]
        o = IO.iterate(W.case(fam, seed))
        hist = two.svs[pos].history()
        assert len(hist) == 2
        e = {k: _srel(hist[0][k], o[k]) for k in ("gap", "mu", "sigma", "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "objective")}
        e["rp_norm"] = IO.residual_rel(hist[0]["rp_norm"], o["rp_norm"], o["b_norm"])
        e["rd_norm"] = IO.residual_rel(hist[0]["rd_norm"], o["rd_norm"], o["c_norm"])
        _assert_all("two66[%d]" % pos, {"hist." + k: v for k, v in e.items()}, {"hist." + k: _bound(k) for k in e})


@pytest.mark.parametrize("name", ["three66", "six66", "mixed66", "detect66", "sparse66"])
def test_wide_batch_is_bit_identical(name, monkeypatch):
    entries = W.CELLS[name]
    opts = lambda family: {}                                          # noqa: E731
    if name == "detect66":
        # the LPs built to fire get the tolerance they are built for; the plain ones keep the default 1e-8 and run their two iterations
        opts = lambda family: dict(detect_infeasibility=True, infeasibility_tol=W.DETECT_TOL if "+" in family else (1e-8, 1e-8))      # noqa: E731
    if name == "sparse66":
        monkeypatch.setenv("IPM_LIST_FORM", "0")                      # read by ipm_create: formation by adat_sparse_kernel
    fam = Family(entries, opts)
    monkeypatch.delenv("IPM_LIST_FORM", raising=False)
    try:
        if name == "sparse66":
            types = {W.LS_TYPES[t] for t, _, _ in fam.program(0)}
            assert "ADAT_SPARSE" in types and "ADAT_LIST" not in types
            monkeypatch.setitem(W.MUST, "two", (W.MUST["two"][0] - {"ZERO", "ADAT_LIST"} | {"ADAT_SPARSE"}, W.MUST["two"][1] - {"ADAT_SPARSE"} | {"ADAT_LIST"}))
        _wide(name, fam, list(range(66)), [f for f, _ in entries], detect=name == "detect66")
    finally:
        fam.close()


def test_active_count_crossing_64(two):
    """67 LPs with iteration caps 3, 1, 2 by position: the schedule is merged again each time LPs leave, 67 (64 + 3) -> 45 -> 23
    active.  An LP with cap c is seen finished by the step that runs its stop test of iteration c: step c + 1."""
    n = 67
    svs, lps = two.svs[:n], two.lps[:n]
    caps = [W.cross_cap(k) for k in range(n)]
    progs = [two.program(i) for i in range(n)]
    _one_template(progs, "cross64")
    ref = [two.alone(i, caps[i]) for i in range(n)]
    trace = _run_batch(svs, lps, caps)
    assert [t[0] for t in trace] == [67, 67, 45, 23]
    active = list(range(n))
    for step, (before, sch, done) in enumerate(trace):
        assert before == len(active)
        plan = _check_schedule(sch, [progs[i] for i in active])
        assert max(st["members"] for st in sch) == min(G, before)
        if before > G:
            _assert_cut(sch, set(_types(progs[0])), before - G, "cross64 step %d" % step)
        else:
            assert [(st["type"], st["members"]) for st in sch] == [(t, before) for t in _types(progs[0])]
        assert all(len(mem) <= G for _, mem in plan)
        left = [i for i in active if caps[i] == step]                 # (nobody at step 0)
        assert sorted(id(s) for s in done) == sorted(id(svs[i]) for i in left), step
        active = [i for i in active if caps[i] != step]
    assert not active
    for k in range(n):
        assert svs[k].stats["iterations"] == caps[k]
        _assert_same("cross64[%d]" % k, svs[k], ref[k])


@pytest.mark.parametrize("start,late", W.JOINS, ids=["%d+%d" % j for j in W.JOINS])
def test_late_join_grows_past_64(two, start, late):
    """LPs that join after the first step start at THEIR iteration 0 beside neighbours one iteration in, in a schedule cut at 64.
    20 + 46: the device table of the records (sized for 1.5 x the first schedule) is replaced by a larger one while in use."""
    n = start + late
    svs, lps = two.svs[:n], two.lps[:n]
    progs = [two.program(i) for i in range(n)]
    _one_template(progs, "join70")
    ref = [two.alone(i, 3) for i in range(n)]
    for sv, p in zip(svs, lps):
        sv.set_state(*p.state())
    done = []
    with ipm.LockstepBatch(tol=1e-8, max_iter=3) as bt:
        for sv in svs[:start]:
            bt.add(sv)
        done += bt.step()
        first = bt.schedule()
        for sv in svs[start:]:
            bt.add(sv)
        assert bt.active == n and not done
        done += bt.step()
        second = bt.schedule()
        for _ in range(6):
            if bt.active:
                done += bt.step()
        assert bt.active == 0
    _check_schedule(first, progs[:start])
    assert all(st["members"] == start for st in first)
    _check_schedule(second, progs)
    _assert_cut(second, set(_types(progs[0])), n - G, "join %d+%d" % (start, late))
    assert sorted(id(s) for s in done) == sorted(id(s) for s in svs)
    assert [id(s) for s in done[:start]] == [id(s) for s in svs[:start]]          # the early LPs finish one step before the late ones
    for k in range(n):
        hist = svs[k].history()
        assert [rec["k"] for rec in hist] == [0, 1, 2], k
        _assert_same("join[%d]" % k, svs[k], ref[k])


def test_step_reports_every_finished_handle_with_a_small_cap(two):
    """ipm_batch_step with a `finished` array smaller than the number of handles that finish at once (ctypes: LockstepBatch always
    passes a large enough one): every handle is reported exactly once, two per call, also by calls that find nothing active."""
    lib = _lib.load()
    n, cap = 5, 2
    svs, lps = two.svs[:n], two.lps[:n]
    ref = [two.alone(i, 1) for i in range(n)]
    prog0 = two.program(0)
    _one_template([two.program(i) for i in range(n)], "cap5")
    for sv, p in zip(svs, lps):
        sv.set_state(*p.state())
    bt = C.c_void_p()
    assert lib.ipm_batch_create(0, None, C.byref(bt)) == _lib.IPM_OK
    try:
        for k, sv in enumerate(svs):
            idx = C.c_int32(-1)
            assert lib.ipm_batch_add(bt, sv._h, 1e-8, 1e-8, 1e-8, 1, C.byref(idx)) == _lib.IPM_OK and idx.value == k
        fin = (C.c_int32 * (cap + 2))(*([-7] * (cap + 2)))
        nf, na = C.c_int32(-1), C.c_int32(-1)
        calls = []
        for _ in range(6):
            assert lib.ipm_batch_step(bt, fin, cap, C.byref(nf), C.byref(na)) == _lib.IPM_OK, lib.ipm_batch_last_error(bt)
            assert 0 <= nf.value <= cap and fin[cap] == -7 and fin[cap + 1] == -7           # never past the capacity
            calls.append((nf.value, na.value, [fin[k] for k in range(nf.value)]))
        # check_every = 1: the first step runs iteration 0, the second one's stop test ends all five (cap 1 reached)
        assert [(c[0], c[1]) for c in calls] == [(0, 5), (2, 0), (2, 0), (1, 0), (0, 0), (0, 0)], calls
        seen = [i for c in calls for i in c[2]]
        assert seen == [0, 1, 2, 3, 4]                                                     # each once, oldest first
        # the schedule hook with too small an array: IPM_ERR_INVALID_ARG, the step count reported, nothing written
        steps, words = C.c_int32(-1), (C.c_int32 * 8)(*([-7] * 8))
        assert lib.ipm_debug_batch_schedule(bt, words, 7, C.byref(steps)) == -1 and steps.value == len(prog0) and list(words) == [-7] * 8
        big = (C.c_int32 * (4 * steps.value))()
        assert lib.ipm_debug_batch_schedule(bt, big, 4 * steps.value, C.byref(steps)) == _lib.IPM_OK
        assert [big[4 * k] for k in range(steps.value)] == _types(prog0) and all(big[4 * k + 1] == n for k in range(steps.value))
        for k, sv in enumerate(svs):
            st = _lib.Stats()
            assert lib.ipm_batch_stats(bt, k, C.byref(st)) == _lib.IPM_OK
            sv.stats = st.as_dict()
            assert (st.status, st.iterations) == (2, 1)
            _assert_same("cap5[%d]" % k, sv, ref[k])
    finally:
        lib.ipm_batch_destroy(bt)
