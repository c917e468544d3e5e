"""CPU side of tests/test_gpu_sparse_structures.py: the constructed cases of tests/sparse_cases.py reach the regime changes of the
multifrontal sparse Cholesky they are named for (so that none loses its edge silently when the symbolic analysis changes), the
derived bounds (F) and (S) are attainable (the sequential fp64 oracle meets them on every case and both scalings), and the guard
cases have the preconditions the device assertions rest on.  Everything comes out of the product's own analysis
(oracle.sparse_chol.panel_table: order_rows + analyse with wcap 32, lds 7680, relax 1); the kernel's decisions are restated here from
csrc/sparse_chol.h and csrc/host_sparse_setup.h."""
import numpy as np
import pytest

import iteration_oracle as IO
import sparse_cases as SC
import test_iteration_oracle_host as TH


@pytest.fixture(scope="module", autouse=True)
def _oracle(built_lib):
    SC.SO.load()


# (w, r, children, mode) cells every case must contain, and what else it pins
EXPECT = {
    "clique64": dict(m=130, lds=4096, cells=[(32, 64, 0, "front")]),
    "clique65": dict(m=130, lds=4096, cells=[(32, 65, 0, "panel"), (32, 33, 1, "front")]),
    "clique240_87_88": dict(m=415, lds=7680, tasks=3, cells=[(32, 240, 0, "panel"), (32, 87, 0, "front"), (32, 88, 0, "panel")]),
    "clique241": dict(m=241, cells=[(31, 241, 0, "panel")]),
    "star13": dict(m=130, fan_in=0, cells=[(2, 2, 12, "front")]),
    "star14": dict(m=130, fan_in=2, height=3, cells=[(2, 2, 2, "front"), (0, 2, 8, "front"), (0, 2, 5, "front")]),
    "star65": dict(m=130, fan_in=8, height=3, cells=[(2, 2, 8, "front"), (0, 2, 8, "front")]),
    "star97": dict(m=130, fan_in=12, height=3, cells=[(2, 2, 12, "front"), (0, 2, 8, "front")]),
    "star106": dict(m=130, fan_in=15, height=4, cells=[(2, 2, 2, "front"), (0, 2, 8, "front"), (0, 2, 6, "front")]),
    "cstar_40_3_14": dict(m=130, fan_in=0, cells=[(32, 46, 12, "front"), (3, 43, 0, "front")]),
    "cstar_70_2_30": dict(m=130, lds=4096, cells=[(2, 72, 0, "panel"), (0, 74, 8, "panel"), (32, 74, 4, "panel")]),
    "bigborder_300_20": dict(m=320, panels=31, tasks=22, fan_in=3,
                             cells=[(1, 301, 0, "panel"), (0, 302, 8, "panel"), (25, 302, 3, "panel"), (27, 277, 1, "panel"),
                                    (30, 250, 1, "panel"), (32, 220, 1, "panel")]),
    "path300": dict(m=300, height=75, panels=75, tasks=2, cells=[(4, 5, 0, "front"), (4, 5, 1, "front")]),
    "nd_4_20": dict(m=300, panels=13, tasks=7, fan_in=0,
                    cells=[(20, 80, 0, "panel"), (32, 80, 2, "panel"), (32, 80, 3, "panel"), (32, 48, 1, "front")]),
    "random400": dict(m=400, fan_in=4, cells=[(32, 91, 3, "panel"), (7, 82, 2, "panel"), (4, 66, 9, "panel")]),
}


def test_the_table_covers_every_case():
    assert set(EXPECT) == set(SC.NAMES)


@pytest.mark.parametrize("name", SC.NAMES)
def test_each_case_reaches_its_edge(name):
    e, t, A = EXPECT[name], SC.tree(name), SC.matrix(name)
    assert A.shape[0] == e["m"] >= SC.MIN_ROWS and sorted(t.perm.tolist()) == list(range(e["m"]))
    # B = A diag(d) A^T has exactly the pattern of the cliques: the unit columns add the diagonal only
    assert np.array_equal(A[:, :e["m"]].toarray(), np.eye(e["m"]))
    for cell in e["cells"]:
        assert t.has(*cell), (name, cell, sorted(t.cells()))
    ntask = t.tasks()[1]
    for key, got in (("lds", t.lds), ("height", t.height), ("panels", t.nsn), ("tasks", ntask), ("fan_in", int(t.fan_in.sum()))):
        if key in e:
            assert got == e[key], (name, key, got)
    # the structure is a tree the kernels can walk: children before parents, a child's rows below its panel inside the parent's front
    assert int(t.w.sum()) == e["m"] and np.all(t.nchild <= 12) and np.all(t.r * t.w <= SC.PANEL) and np.all(t.w <= SC.WCAP)
    for J in range(t.nsn):
        pj = int(t.parent[J])
        if pj >= 0:
            assert pj > J and set(t.rows[J][t.w[J]:].tolist()) <= set(t.rows[pj].tolist())
        else:
            assert t.p[J] == 0
    if name.startswith(("star", "cstar_40", "clique6")):       # the forest edge: the padding rows are one-row roots
        assert int(((t.w == 1) & (t.r == 1) & (t.parent < 0)).sum()) >= 20


def _fan_in_levels(t):
    """Largest number of fan-in nodes on one path to the root."""
    depth = np.zeros(t.nsn, dtype=np.int64)
    for J in range(t.nsn - 1, -1, -1):
        pj = int(t.parent[J])
        depth[J] = int(t.fan_in[J]) + (depth[pj] if pj >= 0 and t.fan_in[pj] else 0)
    return int(depth.max())


def _child_p(t):
    """p of every node that has a parent (pc of the extend-add and of the update vectors)."""
    return t.p[t.parent >= 0]


def test_the_cases_cover_every_regime_of_the_kernels():
    """Each regime change named in the module docstring of tests/test_gpu_sparse_structures.py, by the case that pins it."""
    T = {name: SC.tree(name) for name in SC.NAMES}

    def ksteps(name):
        t = T[name]
        return set(t.ksteps[t.mfma()].tolist())

    # the MFMA update of panel mode: odd and even k-step counts (the tail step `if (kk < ksteps)`), one k-step, a last tile with
    # one live row (p = 33), more tiles than waves (p >= 33: 6 tiles, 4 waves), p no multiple of 16
    assert {7, 8} <= ksteps("bigborder_300_20") and ksteps("cstar_70_2_30") >= {1} and ksteps("clique65") == {8}
    t = T["clique65"]
    assert set(t.p[t.mfma()].tolist()) == {33}
    t = T["cstar_70_2_30"]
    assert np.all(t.p[t.mfma() & (t.w == 2)] == 70) and 70 % 16 != 0
    # front against panel mode at both handle-dependent boundaries: r = 64 | 65 with lds = 4096, r = 87 | 88 with lds = 7680
    assert T["clique64"].lds == T["clique65"].lds == SC.FRONT and T["clique240_87_88"].lds == SC.PANEL
    assert T["clique64"].has(32, 64, 0, "front") and T["clique65"].has(32, 65, 0, "panel")
    assert T["clique240_87_88"].has(32, 87, 0, "front") and T["clique240_87_88"].has(32, 88, 0, "panel")
    # panel width against the LDS budget: r w = 7680 exactly with w = 32; w = 31 = 7680 // 241 with columns left over
    t = T["clique240_87_88"]
    assert int((t.r * t.w).max()) == SC.PANEL == 32 * 240
    t = T["clique241"]
    J = int(np.flatnonzero(t.r == 241)[0])
    assert t.w[J] == SC.PANEL // 241 == 31 and t.p[J] > 0 and t.c0[t.parent[J]] == t.c0[J] + 31
    # extend-add: 12 children without fan-in against 13 with; two levels of fan-in with a pass-through single; a fan-in node in
    # each mode; a child of more than SPC_BATCH * NT entries; a child's update vector longer than the workgroup
    assert T["star13"].has(2, 2, 12) and not T["star13"].fan_in.any() and int(T["star14"].fan_in.sum()) == 2
    assert T["cstar_40_3_14"].has(32, 46, 12, "front") and T["star97"].has(2, 2, 12)
    assert _fan_in_levels(T["star106"]) == 2 and _fan_in_levels(T["star97"]) == 1 and _fan_in_levels(T["bigborder_300_20"]) == 1
    t = T["star106"]          # the pass-through single: a leaf whose parent is a SECOND-level fan-in node
    leaf_under = [J for J in range(t.nsn) if t.w[J] > 0 and t.parent[J] >= 0 and t.fan_in[t.parent[J]] and
                  any(t.fan_in[K] and t.parent[K] == t.parent[J] for K in range(t.nsn))]
    assert len(leaf_under) == 1
    assert (T["star14"].fan_in & T["star14"].front).any() and (T["cstar_70_2_30"].fan_in & ~T["cstar_70_2_30"].front).any()
    assert (T["random400"].fan_in & ~T["random400"].front).any()
    assert (T["bigborder_300_20"].fan_in & ~T["bigborder_300_20"].front).any()
    assert _child_p(T["bigborder_300_20"]).max() > SC.NT and _child_p(T["bigborder_300_20"]).max() ** 2 > SC.BATCH * SC.NT
    assert _child_p(T["clique240_87_88"]).max() ** 2 > SC.BATCH * SC.NT and _child_p(T["cstar_40_3_14"]).max() == 40
    # tree shape: a chain 75 panels tall; parent links partly inside a task and partly hand-offs between tasks
    assert T["path300"].height == 75
    for name in ("bigborder_300_20", "nd_4_20", "clique240_87_88", "path300"):
        t = T[name]
        taskof, ntask = t.tasks()
        assert 1 < ntask < t.nsn, name
        link = t.parent >= 0
        same = taskof[link] == taskof[t.parent[link]]
        assert same.any() and ((~same).any() or name == "clique240_87_88"), name      # three disjoint cliques: three whole-tree tasks


@pytest.mark.parametrize("D", SC.DS)
@pytest.mark.parametrize("name", SC.NAMES)
def test_the_bounds_are_attainable(name, D):
    """The sequential fp64 restatement of the device's scheme (oracle/sparse_chol_oracle.cpp) meets (F) and (S) with no extra margin,
    guards nothing, keeps its factor inside the panels' structure, and walks the tree that panel_table reports."""
    ref = SC.reference(name, D)
    ora = SC.SO.factor_solve(ref.A, ref.d, ref.rhs)
    t = ref.tree
    assert np.array_equal(ora["perm"], ref.perm) and ora["fixed"] == 0
    st = ora["stats"]
    assert (int(st["panels"]), int(st["height"]), int(st["widest_front"]), int(st["fan_in_nodes"])) == \
        (t.nsn, t.height, t.rmax, int(t.fan_in.sum()))
    f, s = SC.check_factor(ora["L"], ref), SC.check_solve(ora["z"], ref)
    print("RATIO host %s D=%g F %.4f S %.4f" % (name, D, f, s))
    assert f <= 1.0 and s <= 1.0 and SC.outside_structure(ora["L"], ref) == 0


def test_a_dropped_update_term_breaks_the_bounds():
    """The bounds are tight enough to notice what the issue names: a perturbation of relative size 1e-9 of one entry of the factor
    (a dropped update term) passes a 1e-8 comparison and fails (F) and (S)."""
    ref = SC.reference("nd_4_20", 0.3)
    ora = SC.SO.factor_solve(ref.A, ref.d, ref.rhs)
    L = ora["L"].copy()
    L[-1, -2] *= 1.0 + 1e-9
    assert SC.check_factor(L, ref) > 1.0
    z = ora["z"].copy()
    z[ref.perm[-1]] *= 1.0 + 1e-9
    assert SC.check_solve(z, ref) > 1.0


@pytest.mark.parametrize("name", sorted(SC.GUARD_CASES))
def test_guard_preconditions(name):
    base, src, dst, want = SC.GUARD_CASES[name]
    A, A0 = SC.matrix(name), SC.matrix(base)
    m = A.shape[0]
    # row dst is a copy of row src, its own unit column is empty, nothing else moved
    assert np.array_equal(A[dst].toarray(), A0[src].toarray()) and A[:, dst].nnz == 0
    others = np.setdiff1d(np.arange(m), [dst])
    assert (A[others] != A0[others]).nnz == 0
    place = SC.guard_place(name)
    for key, val in want.items():
        assert place[key] == val, (name, key, place)
    g = SC.guard(name)
    t = SC.tree(name)
    assert g.guarded.tolist() == [place["col"]] == [int(max(t.pos[src], t.pos[dst]))]
    k = g.ref.k
    assert np.all(g.pivots[g.guarded] <= 1e-3 * g.thresh)
    assert np.all(k * SC.U * g.diag[g.guarded] <= 0.1 * g.thresh)
    assert np.all(np.delete(g.pivots, g.guarded) >= 1e3 * g.thresh)
    ora = SC.SO.factor_solve(A, g.ref.d, g.ref.rhs, eps=SC.GUARD_EPS, big=SC.GUARD_BIG)
    assert ora["fixed"] == 1 and np.flatnonzero(np.diag(ora["L"]) > 1e30).tolist() == g.guarded.tolist()
    assert SC.check_factor(ora["L"], g.ref) <= 1.0 and SC.check_solve(ora["z"], g.ref) <= 1.0


def test_the_guard_cases_cover_every_place():
    P = {name: SC.guard_place(name) for name in SC.GUARD_CASES}
    assert any(p["first"] for p in P.values()) and any(p["last32"] for p in P.values())
    assert any(p["mode"] == "panel" and not p["first"] and not p["last32"] for p in P.values())
    assert any(p["mode"] == "front" and not p["root"] for p in P.values())
    assert any(p["root"] for p in P.values()) and any(p["p"] > SC.NT for p in P.values())


@pytest.mark.parametrize("bounded", [False, True], ids=["free", "bounded"])
@pytest.mark.parametrize("name", ["bigborder_300_20", "nd_4_20", "star106"])
def test_iteration_cases_meet_the_host_condition(name, bounded):
    """The condition under which tests/test_gpu_iteration_edges.py's bounds mean something (its FLOOR): the fp64 restatements of one
    iteration agree with the longdouble oracle to 1e-12 on the cases of check (e), whose ratio tests have a separated blocker."""
    case = SC.iteration_case(name, bounded)
    assert case.bounded == bounded and sparse_pattern_kept(case, name)
    o = IO.iterate(case)
    (xn, yn, sn, wn, zn), rec = TH._fp64_iteration(case, IO.ETA)
    err = {"x": IO.rel(xn, o["xn"]), "y": IO.rel(yn, o["yn"]), "s": IO.rel(sn, o["sn"]), "w": IO.rel(wn, o["wn"]), "z": IO.rel(zn, o["zn"])}
    for k in ("mu", "sigma", "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d"):
        err[k] = IO.rel(rec[k], o[k])
    assert max(err.values()) <= TH.TOL, (name, err)
    assert min(o["sep_p"], o["sep_d"], o["sep_aff_p"], o["sep_aff_d"]) >= 1e-3


def sparse_pattern_kept(case, name):
    """The dense image the Case carries gives back the case's sparse matrix: the solver of check (e) walks the same tree."""
    from scipy import sparse
    return (sparse.csc_matrix(case.A) != SC.matrix(name)).nnz == 0
