"""Host conditions of tests/test_gpu_mcc.py (no GPU): the centrality-corrector oracle of tests/mcc_oracle.py is what it says, and its
cells have the properties the device test leans on.

 - K = 0 IS iteration_oracle.iterate: same arrays, bit for bit.
 - every accepted candidate solves the Newton system of its complementarity terms, in longdouble:
   A dx = -r_b, A^T dy + ds - dz = -r_c, dx + dw = -r_u on U, S dx + X ds = -r3g, Z dw + W dz = -r4g.  Each residual is measured
   against the largest of the terms it sums (for A dx, |A| |dx|: in the full-step case r_b and A dx are both zero to rounding, and
   only the terms of the products say what rounding is).  Bound: these are residuals of a longdouble Cholesky solve with
   cond(A Theta A^T) below 1e4 at these cells: 1e-15 is three decimal orders above the 64-bit mantissa (1.1e-19) times that.
 - the oracle's own statements run in fp64 (prec=np.float64: LAPACK's Cholesky, fp64 Mehrotra part) agree with it below 1e-12, the
   floor tests/test_iteration_oracle_host.py holds its restatements to (TOL there) and the floor of the device bounds: that is the
   conditioning of the cells.  Separately, ONE round is restated here from the issue's text with nothing of mcc_oracle in it
   (_independent_round: the full KKT system of the round solved by LAPACK's LU instead of the normal equations, np.clip for the box,
   its own ratio tests and accept rule) and must give the oracle's candidate, step lengths, margin and decision.  The KKT solve
   carries cond(KKT), up to 1e6 here, so its bound is 1e-9 on the vectors (1e6 x 2.2e-16 with a decimal to spare) -- far below what a
   transcription error in the target or the accept rule would leave (a wrong constant moves the candidate by 1e-2 and more).
 - preconditions of the GPU cells: every accept margin at least 1e-6 in magnitude (rounding, 1e-12 on the step lengths, cannot flip
   a decision); a cell whose rounds 1 and 2 are both accepted; a cell with a rejected round while K leaves rounds over; a cell whose
   blocking component after a round is a w or a z component.  The full-step case does NOT reject, against the issue's expectation:
   only its dual step starts at eta (0.91), its primal step starts at 0.80 and a round lifts it to 0.82; the rejecting cell is
   dense/129x16385, whose first round loses 0.38 in the dual step.
 - the C entry point refuses NULL, -1 and IPM_MAX_CORRECTORS + 1 without a device; the header declares both functions.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iteration_oracle as IO
import mcc_oracle as M
from interiorpointmethod_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12               # tests/test_iteration_oracle_host.py: TOL
MARGIN = 1e-6
NEWTON = 1e-15
HOST_CELLS = [c for c in M.CELLS if "16385" not in c] + ["dense/129x16385"]     # cells of the Newton / fp64 comparisons (the other
                                                                                # large cells cost 4 s of longdouble each; the
                                                                                # preconditions below take every cell's oracle)


@pytest.mark.parametrize("name", ["dense/130x257b", "dense/300x513"])
def test_k0_is_the_iteration_oracle(name):
    case = M.get(name)
    o, ref = M.iterate(case, 0), IO.iterate(case)
    assert o["rounds"] == [] and o["rounds_run"] == 0
    for k in ("dx", "dy", "ds", "dw", "dz", "atdy", "xn", "yn", "sn", "wn", "zn", "atyn"):
        assert np.array_equal(o[k], ref[k]), k
    assert o["alpha_p"] == ref["alpha_p"] and o["alpha_d"] == ref["alpha_d"]
    t = M.truncate(M.oracle(name), 0, case)                       # the prefix route gives the same
    for k in ("dx", "dy", "xn", "yn", "sn", "wn", "zn"):
        assert np.array_equal(t[k], ref[k]), k


def _rel(res, *terms):
    scale = max(float(IO.norm(t)) for t in terms)
    return float(IO.norm(res)) / scale


@pytest.mark.parametrize("name", HOST_CELLS)
def test_accepted_candidates_solve_the_newton_system(name):
    case, o = M.get(name), M.oracle(name)
    A = case.A.astype(IO.LD)
    x, s, w, z = (np.asarray(v, dtype=IO.LD) for v in (case.x, case.s, case.w, case.z))
    U = case.U
    n_acc = 0
    for r in o["rounds"]:
        if not r["accepted"]:
            continue
        n_acc += 1
        e = {"A dx": _rel(A @ r["dx"] + o["rb"], np.abs(A) @ np.abs(r["dx"]), o["rb"]),
             "dual": _rel(r["atdy"] + r["ds"] - r["dz"] + o["rc"], r["atdy"], r["ds"], o["rc"]),
             "A^T dy": IO.rel(A.T @ r["dy"], r["atdy"]),
             "bound": _rel((r["dx"] + r["dw"] + o["ru"])[U], r["dx"], o["ru"]) if U.any() else 0.0,
             "xs": _rel(s * r["dx"] + x * r["ds"] + r["r3g"], s * r["dx"], r["r3g"]),
             "wz": _rel((z * r["dw"] + w * r["dz"] + r["r4g"])[U], r["r4g"][U]) if U.any() else 0.0}
        print("NEWTON", name, {k: "%.1e" % v for k, v in e.items()})
        assert all(v <= NEWTON for v in e.values()), (name, e)
        assert np.all(r["dw"][~U] == 0) and np.all(r["dz"][~U] == 0) and np.all(r["r4g"][~U] == 0)
    assert n_acc == o["rounds_accepted"]


@pytest.mark.parametrize("name", HOST_CELLS)
def test_fp64_restatement_agrees(name):
    case, o = M.get(name), M.oracle(name)
    f = M.iterate(case, M.MAX_K, prec=np.float64)
    assert f["rounds_run"] == o["rounds_run"] and [r["accepted"] for r in f["rounds"]] == [r["accepted"] for r in o["rounds"]]
    e = {}
    for i, (rf, ro) in enumerate(zip(f["rounds"], o["rounds"])):
        for k in ("dx", "ds", "dy") + (("dw", "dz") if case.bounded else ()):
            e["r%d.%s" % (i + 1, k)] = IO.rel(rf[k], ro[k])
        for k in ("alpha_hat_p", "alpha_hat_d"):
            e["r%d.%s" % (i + 1, k)] = float(abs(IO.LD(rf[k]) - ro[k]) / ro[k])
        assert abs(float(rf["margin"]) - float(ro["margin"])) <= 4 * TOL
    for k in ("xn", "yn", "sn") + (("wn", "zn") if case.bounded else ()):
        e[k] = IO.rel(f[k], o[k])
    print("FP64", name, "max %.1e" % max(e.values()))
    assert all(v <= TOL for v in e.values()), (name, {k: v for k, v in e.items() if v > TOL})


def _independent_round(case, m, eta):
    """One round restated from the rule's text, in fp64, from Mehrotra's results `m` (iteration_oracle.iterate): the unreduced Newton
    system [A 0 0 0 0; 0 A^T I 0 -I; I 0 0 I 0; S 0 X 0 0; 0 0 0 Z W] (dx, dy, ds, dw, dz) = -(r_b, r_c, r_u, r3g, r4g), the bound rows
    and columns on U only."""
    f = lambda v: np.asarray(v, dtype=np.float64)
    A, b, c, x, y, s, w, z = case.A, case.b, case.c, case.x, case.y, case.s, case.w, case.z
    U = np.flatnonzero(case.U)
    mm, n, k = case.m, case.n, U.size
    dx, ds, dw, dz = f(m["dx"]), f(m["ds"]), f(m["dw"]), f(m["dz"])
    sm = float(m["sigma"] * m["mu"])
    ap, ad = float(m["alpha_p"]), float(m["alpha_d"])
    tp, td = min(1.0, ap + 0.1), min(1.0, ad + 0.1)

    def corr(v):
        return np.maximum(np.clip(v, 0.1 * sm, 10.0 * sm) - v, -10.0 * sm)

    r3g = x * s + f(m["dxa"]) * f(m["dsa"]) - sm - corr((x + tp * dx) * (s + td * ds))
    r4g = (w * z + f(m["dwa"]) * f(m["dza"]) - sm - corr((w + tp * dw) * (z + td * dz)))[U]
    N = n + mm + n + 2 * k
    K = np.zeros((N, N))
    ox, oy, os_, ow, oz = 0, n, n + mm, 2 * n + mm, 2 * n + mm + k
    K[:mm, ox:ox + n] = A
    K[mm:mm + n, oy:oy + mm] = A.T
    K[mm:mm + n, os_:os_ + n] = np.eye(n)
    K[mm + U, oz + np.arange(k)] = -1.0
    r = mm + n
    K[r + np.arange(k), ox + U] = 1.0
    K[r + np.arange(k), ow + np.arange(k)] = 1.0
    r += k
    K[r + np.arange(n), ox + np.arange(n)] = s
    K[r + np.arange(n), os_ + np.arange(n)] = x
    r += n
    K[r + np.arange(k), ow + np.arange(k)] = z[U]
    K[r + np.arange(k), oz + np.arange(k)] = w[U]
    rhs = -np.concatenate([A @ x - b, A.T @ y + s - np.where(case.U, z, 0.0) - c, (x + w - case.u)[U], r3g, r4g])
    sol = np.linalg.solve(K, rhs)
    cx, cy, cs = sol[ox:ox + n], sol[oy:oy + mm], sol[os_:os_ + n]
    cw, cz = np.zeros(n), np.zeros(n)
    cw[U], cz[U] = sol[ow:ow + k], sol[oz:oz + k]

    def step(v, dv, vb, dvb):
        cand = [1.0 / eta] + [-a / da for a, da in zip(np.concatenate([v, vb[U]]), np.concatenate([dv, dvb[U]])) if da < 0]
        return min(1.0, eta * min(min(cand), 1.0))

    ahp, ahd = step(x, cx, w, cw), step(s, cs, z, cz)
    margin = ahp + ahd - ap - ad - 0.1 * 0.1
    return dict(dx=cx, dy=cy, ds=cs, dw=cw, dz=cz, alpha_hat_p=ahp, alpha_hat_d=ahd, margin=margin, accepted=margin >= 0)


KKT_TOL = 1e-9


@pytest.mark.parametrize("name", ["dense/5x65b", "dense/130x257b", "dense/300x513", "sparse/130x257b"])
def test_independent_restatement_of_one_round(name):
    case, o = M.get(name), M.oracle(name)
    r = o["rounds"][0]
    g = _independent_round(case, o["mehrotra"], IO.ETA)
    e = {k: IO.rel(g[k], r[k]) for k in ("dx", "dy", "ds") + (("dw", "dz") if case.bounded else ())}
    e["alpha_hat_p"] = abs(g["alpha_hat_p"] - float(r["alpha_hat_p"]))
    e["alpha_hat_d"] = abs(g["alpha_hat_d"] - float(r["alpha_hat_d"]))
    e["margin"] = abs(g["margin"] - float(r["margin"]))
    print("KKT", name, {k: "%.1e" % v for k, v in e.items()})
    assert all(v <= KKT_TOL for v in e.values()), (name, e)
    assert g["accepted"] == r["accepted"]


def test_preconditions_of_the_gpu_cells():
    both = rejected_early = bound_blocker = False
    for name in M.CELLS:
        o = M.oracle(name)                                            # the longdouble oracle the device test compares against
        acc = [r["accepted"] for r in o["rounds"]]
        print("CELL", name, acc, ["%.2e" % float(r["margin"]) for r in o["rounds"]], [(r["argmin_p"][0], r["argmin_d"][0]) for r in o["rounds"]])
        assert all(abs(float(r["margin"])) >= MARGIN for r in o["rounds"]), name
        assert len(acc) == M.MAX_K or not acc[-1]                     # the chain ends only at a rejected round
        both |= len(acc) >= 2 and acc[0] and acc[1]
        rejected_early |= (not acc[-1]) and len(acc) < M.MAX_K       # K = MAX_K leaves rounds over behind the rejected one
        bound_blocker |= any(r["accepted"] and 1 in (r["argmin_p"][0], r["argmin_d"][0]) for r in o["rounds"])
    assert both and rejected_early and bound_blocker
    first = M.oracle("dense/129x16385")["rounds"]
    assert len(first) == 1 and not first[0]["accepted"]              # the cell the device test takes its dead chain from
    full = M.oracle("full")
    assert full["mehrotra"]["alpha_d"] == IO.LD(IO.ETA) and full["mehrotra"]["alpha_p"] < 0.85      # (module docstring)


def test_constants_match_the_rules():
    src = open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "iteration_rules.h")).read()
    m = re.search(r"MCC_DELTA = ([\d.]+), MCC_GAMMA = ([\d.]+), MCC_BETA_MIN = ([\d.]+), MCC_BETA_MAX = ([\d.]+);", src)
    assert m and tuple(float(v) for v in m.groups()) == (M.DELTA, M.GAMMA, M.BETA_MIN, M.BETA_MAX)


def test_entry_point_refuses_bad_arguments_without_a_device(built_lib):
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    assert "int ipm_set_centrality_correctors(ipm_handle* h, int32_t k);" in header
    assert "int ipm_get_corrector_info(ipm_handle* h, int64_t out[4]);" in header
    assert re.search(r"#define IPM_MAX_CORRECTORS (\d+)", header).group(1) == str(_lib.MAX_CORRECTORS) == "8"
    err = -1                                                          # IPM_ERR_INVALID_ARG
    assert lib.ipm_set_centrality_correctors(None, 1) == err
    assert b"NULL" in lib.ipm_last_error(None)
    for k in (-1, _lib.MAX_CORRECTORS + 1):                           # the range check reads nothing of the handle
        assert lib.ipm_set_centrality_correctors(None, k) == err
        assert b"outside 0 .. 8" in lib.ipm_last_error(None)
    out = (C.c_int64 * 4)()
    assert lib.ipm_get_corrector_info(None, out) == err


@pytest.mark.parametrize("setter,kmax", [("ipm_set_centrality_correctors", _lib.MAX_CORRECTORS), ("ipm_set_refinement", _lib.MAX_REFINE)])
def test_both_round_setters_share_the_argument_rules_without_a_device(built_lib, setter, kmax):
    """The one statement of the setters' argument rules (host_iteration.h, rounds_set): NULL and the range, in messages that name the
    call; the range check comes first (it reads nothing of the handle)."""
    lib = _lib.load()
    call, err = getattr(lib, setter), -1                             # IPM_ERR_INVALID_ARG
    for k in (0, 1, kmax):
        assert call(None, k) == err
        assert lib.ipm_last_error(None) == ("%s: NULL handle" % setter).encode()
    for k in (-1, kmax + 1):
        assert call(None, k) == err
        assert lib.ipm_last_error(None) == ("%s: k = %d outside 0 .. %d" % (setter, k, kmax)).encode()
