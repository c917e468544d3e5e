"""The cells of tests/lockstep_wide_cases.py are what their names claim, checked without a GPU: block counts and the group layout
the families are chosen for (against the library's own group_size, through ipm_debug_at_pieces), LPs that are pairwise different
with no empty row or column, a product list inside the rule of the list formation, the host condition of
tests/test_iteration_oracle_host.py for the four LPs the GPU file holds to the longdouble oracle -- and the schedule merge
(csrc/lockstep_merge.h, through ipm_debug_ls_merge) at exactly 64, 65, 128 and 129 members: the member counts of the launches a
step is cut into, and the batch order inside them."""
import ctypes as C

import numpy as np
import pytest

import iteration_oracle as IO
import lockstep_wide_cases as W
from interiorpointmethod_amd import _lib
from test_iteration_oracle_host import SEPARATION, TOL, _fp64_iteration
from test_lockstep_merge import check, merge


def test_type_table_matches_the_header():
    """LS_TYPES restates enum LsType of csrc/lockstep.h: same names, same order, LS_NTYPES last."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "lockstep.h")).read()
    body = re.search(r"enum LsType \{(.*?)\};", src, re.S).group(1)
    names = [t.strip() for t in body.replace("\n", " ").split(",")]
    assert names[0] == "LS_SPMV_CSR = 0" and names[-1] == "LS_NTYPES"
    assert ["LS_SPMV_CSR"] + names[1:-1] == ["LS_" + nm for nm in W.LS_TYPES]
    assert int(re.search(r"LS_MAX_GROUP = (\d+)", src).group(1)) == W.LS_MAX_GROUP
    assert (W.LS["PREPARE_DETECT"], W.LS["STOP_TEST_DETECT"]) == (27, 28)


@pytest.mark.parametrize("family", sorted(W.BLOCKS))
def test_family_layout(family):
    lib = _lib.load()
    nblk = W.BLOCKS[family]
    layout, count = (C.c_int32 * 4)(0, 0, 0, 0), C.c_int32(0)
    assert lib.ipm_debug_at_pieces(nblk, layout, None, 0, C.byref(count)) == _lib.IPM_OK
    assert layout[0] == 128 * nblk <= W.LIST_MAX_MP and layout[1] == W.group_size(nblk)
    assert W.groups(family) == {"two": (2, 1), "three": (0, 0), "six": (2, 3)}[family]
    lo, hi = W.M_RANGE[family]
    ms = {W.shape(family, s)[0] for s in range(70)}
    assert min(ms) == lo and max(ms) == hi and len(ms) >= 6          # both ends of the block count, several sizes in between
    assert -(-lo // 128) == -(-hi // 128) == nblk and lo > 128
    for nb in range(1, 40):                                          # the restatement, against the library at every block count
        lay = (C.c_int32 * 4)(0, 0, 0, 0)
        assert lib.ipm_debug_at_pieces(nb, lay, None, 0, C.byref(count)) == _lib.IPM_OK
        assert lay[1] == W.group_size(nb), nb


def test_cells_have_the_sizes_and_the_order_they_claim():
    for name in ("two66", "three66", "six66", "mixed66", "detect66", "sparse66"):
        assert len(W.CELLS[name]) == 66 == W.LS_MAX_GROUP + 2
    assert len(W.CELLS["cross64"]) == 67 and len(W.CELLS["join70"]) == 70 and len(W.CELLS["cap5"]) == 5
    for name, fam in (("two66", "two"), ("three66", "three"), ("six66", "six"), ("sparse66", "two"), ("cross64", "two"), ("join70", "two")):
        assert {f for f, _ in W.CELLS[name]} == {fam}
    fams = [f for f, _ in W.CELLS["mixed66"]]
    assert [fams.count(f) for f in ("two", "three", "six")] == [44, 14, 8]
    runs = 1 + sum(a != b for a, b in zip(fams, fams[1:]))
    assert runs >= 40                                                 # interleaved, not sorted (sorted: 3 runs)
    assert {"two", "three", "six"} <= set(fams[:12]) and len(set(fams[W.LS_MAX_GROUP - 8:])) >= 2
    assert [f for f, _ in W.CELLS["detect66"]][:3] == ["two", "two+primal", "two+dual"]
    for pos in W.ORACLE_POSITIONS:
        assert W.CELLS["two66"][pos] == ("two", pos)
    assert W.ORACLE_POSITIONS == (0, 32, 63, 64)
    caps = [W.cross_cap(p) for p in range(67)]
    assert [caps.count(k) for k in (1, 2, 3)] == [22, 22, 23] and caps[:3] == [3, 1, 2]
    for start, late in W.JOINS:
        assert start + late > W.LS_MAX_GROUP and start + late <= 70
    assert W.JOINS[0] == (60, 10) and W.JOINS[1][0] + W.JOINS[1][1] > 1.5 * W.JOINS[1][0] + 1      # the table of ipm_batch_step grows by half


@pytest.mark.parametrize("name", sorted(W.CELLS))
def test_cell_lps(name):
    lps = W.cell(name)
    seen = set()
    for (fam, seed), p in zip(W.CELLS[name], lps):
        m, n, density = W.shape(fam, seed)
        lo, hi = W.M_RANGE[W.base(fam)]
        assert (p.m, p.n) == (m, n) == p.A.shape and lo <= m <= hi and -(-m // 128) == W.BLOCKS[W.base(fam)]
        assert (m + 40 <= n <= m + 350) or (W.base(fam) == "two" and n == 513)
        cnt_c, cnt_r = np.diff(p.A.indptr), np.bincount(p.A.indices, minlength=m)
        assert cnt_c.min() >= 1 and cnt_r.min() >= 1                  # no empty column, no empty row
        assert p.A.nnz <= 1.3 * density * m * n + m + n
        terms = int((cnt_c.astype(np.int64) * (cnt_c + 1) // 2).sum())
        assert terms <= W.LIST_MAX_TERMS // 16                        # the product list fits with room to spare: list formation
        assert np.all(p.x > 0) and np.all(p.s > 0) and p.y.shape == (m,)
        key = (p.A.data.tobytes(), p.A.indices.tobytes(), p.b.tobytes(), p.c.tobytes())
        assert key not in seen
        seen.add(key)
    assert len(seen) == len(lps)
    if name == "two66":
        assert sum(p.n == 513 for p in lps) >= 3 and len({(p.m, p.n) for p in lps}) >= 60
        assert len({-(-max(p.m, p.n) // 256) for p in lps}) == 3      # one, two and three blocks in the vector kernels' grids


@pytest.mark.parametrize("pos", W.ORACLE_POSITIONS)
def test_oracle_lps_meet_the_host_condition(pos):
    """What tests/test_iteration_oracle_host.py asserts for every case the oracle is used on: fp64 arithmetic alone agrees with the
    longdouble oracle to 1e-12, and no ratio test has a runner-up closer than 1e-6 to its blocker."""
    fam, seed = W.CELLS["two66"][pos]
    case = W.case(fam, seed)
    assert np.array_equal(W.lp(fam, seed).A.toarray(), case.A) and not case.bounded
    o = IO.iterate(case)
    (xn, yn, sn, _, _), rec = _fp64_iteration(case, IO.ETA)
    err = {"x": IO.rel(xn, o["xn"]), "s": IO.rel(sn, o["sn"]), "ATy": IO.rel(case.A.T @ np.ravel(yn), o["atyn"])}
    for k in ("mu", "mu_aff", "sigma", "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "gap", "objective"):
        err[k] = IO.rel(rec[k], o[k])
    err["rp_norm"] = IO.residual_rel(rec["rp_norm"], o["rp_norm"], o["b_norm"])
    err["rd_norm"] = IO.residual_rel(rec["rd_norm"], o["rd_norm"], o["c_norm"])
    print(pos, (case.m, case.n), {k: "%.1e" % v for k, v in err.items()})
    assert max(err.values()) <= TOL, (pos, err)
    for k in ("sep_aff_p", "sep_aff_d", "sep_p", "sep_d"):
        assert o[k] >= SEPARATION, (pos, k, o[k])
    assert not IO.converged(case, 1e-8)


def test_fire_lps_fire_their_test():
    for pos, (fam, seed) in enumerate(W.CELLS["detect66"][:6] + W.CELLS["detect66"][60:]):
        if fam == "two":
            continue
        q = IO.infeasibility(W.case_uncached(fam, seed))
        if fam.endswith("+primal"):
            assert q["beta"] > 0 and 0 < q["vp"] <= W.DETECT_TOL[0] * q["beta"] / 1.9, (fam, seed)
        else:
            assert q["beta"] <= 0 and q["gamma"] > 0 and 0 < q["vd"] <= W.DETECT_TOL[1] * q["gamma"] / 1.9, (fam, seed)


# ---- the merge at the group limit ------------------------------------------------------------------------------------------
def _split(members):
    """The launches a step of that many members must be cut into."""
    return [W.LS_MAX_GROUP] * (members // W.LS_MAX_GROUP) + ([members % W.LS_MAX_GROUP] if members % W.LS_MAX_GROUP else [])


@pytest.mark.parametrize("members", [64, 65, 128, 129])
@pytest.mark.parametrize("aligned", [1, 0])
def test_merge_at_the_group_limit(members, aligned):
    """Programs of one template: every step of the template becomes launches of 64; 64 + 1; 64 + 64; 64 + 64 + 1 members, in the
    template's order, and the members of a launch are consecutive LPs in batch order, the first launch starting at LP 0."""
    prog = W.template(2, "group")
    progs = [list(prog) for _ in range(members)]
    plan = merge(progs, max_group=W.LS_MAX_GROUP, aligned=aligned)
    check(progs, plan, W.LS_MAX_GROUP)
    parts = _split(members)
    assert parts == {64: [64], 65: [64, 1], 128: [64, 64], 129: [64, 64, 1]}[members]
    assert len(plan) == len(prog) * len(parts)
    for s, (t, mem) in enumerate(plan):
        pos, part = divmod(s, len(parts))
        assert t == prog[pos] and len(mem) == parts[part], (s, t, len(mem))
        first = part * W.LS_MAX_GROUP
        assert mem == [(first + k, pos) for k in range(parts[part])], s


def test_merge_of_the_mixed_cell_template():
    """Three templates of three lengths in the order of mixed66: every LP's order kept, no launch above 64 members, the launches of
    a step in batch order, and a schedule of about the longest template (what the GPU file asserts of the real programs)."""
    tmpl = {"two": W.template(2, "group"), "three": W.template(3, "block"), "six": W.template(6, "group")}
    progs = [tmpl[fam] for fam, _ in W.CELLS["mixed66"]]
    plan = merge(progs, max_group=W.LS_MAX_GROUP)
    check(progs, plan, W.LS_MAX_GROUP)
    whole = merge(progs, max_group=1 << 20)
    # no common supersequence is shorter than the longest template plus the launches of another whose type it does not hold (the
    # block steps of `three`: 2 solves x (3 forward + 3 backward)); the alignment reaches that bound here
    alone = sum(t not in set(tmpl["six"]) for t in tmpl["three"])
    assert alone == 12 and len(whole) == len(tmpl["six"]) + alone
    assert len(plan) == len(whole) + sum(len(mem) > W.LS_MAX_GROUP for _, mem in whole)
    for t, mem in plan:
        assert [i for i, _ in mem] == sorted(i for i, _ in mem)
    wide = [(t, mem) for t, mem in whole if len(mem) == 66]
    assert wide and {t for t, _ in wide} >= {W.LS[nm] for nm in ("SPMV_CSR", "STOP_TEST", "ADAT_LIST", "POTRF", "UPDATE")}
