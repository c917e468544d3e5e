"""The QP oracle of tests/qp_oracle.py held to itself on the CPU, before tests/test_gpu_qp.py holds the device to it:

  * the float64 restatement of one iteration agrees with the longdouble one to 1e-12 on every case used on the GPU;
  * with g = 0 and the one-step rule switched off the oracle IS iteration_oracle.iterate, bit for bit;
  * the oracle's directions satisfy the Newton equations of the QP in longdouble, written without the elimination;
  * the float64 loop reaches every constructed optimum of workloads.separable_qp that the GPU solves.

Bounds.  1e-12: iteration_oracle's own floor for fp64 restatements (test_iteration_oracle_host.py).  Newton equations: 1e-12
relative to the largest term of the row -- a Cholesky solve leaves a residual of m eps cond(B) at the worst: m <= 520, the
longdouble eps 5.4e-20, and cond(A Theta A^T) <= 16 ((sqrt n + sqrt m) / (sqrt n - sqrt m))^2 = 1.2e4 for the 520 x 600 Gaussian A
with theta spread over a factor 16, so 3.4e-13; a wrong or missing term of the system is an error of order 0.1 (observed: at most
4.4e-16).  Constructed optimum: the stop test leaves x_j s_j <= gap <= 1e-8 and s* >= 0.5 on the columns at zero, so |x_j| <= 2e-8
there; one decade for the active columns, which follow through A: 1e-7 (observed: at most 4.5e-12).
"""
import numpy as np
import pytest

import iteration_oracle as IO
import qp_oracle as Q

LD = IO.LD
VECTORS = ("dxa", "dya", "dsa", "dwa", "dza", "atdya", "dx", "dy", "ds", "dw", "dz", "atdy", "xn", "yn", "sn", "wn", "zn", "atyn")
SCALARS = ("alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "mu", "mu_aff", "sigma", "gap", "objective", "rp_norm", "rd_norm")


@pytest.mark.parametrize("name", sorted(Q.ITER_CASES))
def test_float64_restatement_agrees_with_longdouble(name):
    case, g = Q.get(name)
    o, f = Q.oracle(name), Q.iterate(case, g, T=np.float64)
    errs = {k: IO.rel(f[k], o[k]) for k in VECTORS}
    errs.update({k: float(abs(LD(f[k]) - o[k]) / abs(o[k])) for k in SCALARS if k not in ("rp_norm", "rd_norm")})
    errs["rp_norm"] = IO.residual_rel(f["rp_norm"], o["rp_norm"], o["b_norm"])
    errs["rd_norm"] = IO.residual_rel(f["rd_norm"], o["rd_norm"], o["c_norm"])
    for k in sorted(errs):
        print("HOST64 %s %s %.3e" % (name, k, errs[k]))
    bad = {k: v for k, v in errs.items() if not v <= 1e-12}
    assert not bad, (name, bad)
    assert o["alpha_p"] == o["alpha_d"] and o["alpha_aff_p"] == o["alpha_aff_d"]
    assert g[0] > 0 and np.all(g[1::2] == 0) and np.all(g[0::2] > 0)          # LP and QP columns mix


@pytest.mark.parametrize("name", ["dense/400x520b", "dense/520x600", "sparse/130x300b"])
def test_zero_term_is_the_lp_oracle(name):
    case, _ = Q.get(name)
    o = IO.iterate(case)
    q = Q.iterate(case, np.zeros(case.n), one_step=False)
    for k in VECTORS + SCALARS + ("b_norm", "c_norm", "aty"):
        assert np.array_equal(np.asarray(q[k]), np.asarray(o[k])), (name, k)
    one = Q.iterate(case, np.zeros(case.n), one_step=True)                # the rule alone: the minimum of each pair
    assert one["alpha_aff_p"] == one["alpha_aff_d"] == min(o["alpha_aff_p"], o["alpha_aff_d"])


@pytest.mark.parametrize("name", sorted(Q.ITER_CASES))
def test_newton_equations_hold(name):
    case, g = Q.get(name)
    o = Q.oracle(name)
    A = case.A.astype(LD)
    g = g.astype(LD)
    x, s, w, z = (np.asarray(v, dtype=LD) for v in (case.x, case.s, case.w, case.z))
    U = case.U
    sm = o["sigma"] * o["mu"]
    for tag, (dx, dy, ds, dw, dz), r3, r4 in (("aff", [o[k] for k in ("dxa", "dya", "dsa", "dwa", "dza")], x * s, w * z),
                                               ("cor", [o[k] for k in ("dx", "dy", "ds", "dw", "dz")], o["r3c"], o["r4c"])):
        rows = {
            "primal": (A @ dx + o["rb"], [A @ dx, o["rb"]]),
            "dual": (dy @ A + ds - dz - g * dx + o["rc"], [dy @ A, ds, dz, g * dx, o["rc"]]),
            "xs": (s * dx + x * ds + r3, [s * dx, x * ds, r3]),
            "bound": ((dx + dw + o["ru"])[U], [dx[U], dw[U], o["ru"][U]]),
            "wz": ((z * dw + w * dz + r4)[U], [(z * dw)[U], (w * dz)[U], r4[U]]),
        }
        for row, (res, terms) in rows.items():
            if res.size == 0:
                continue
            scale = max(float(np.abs(t).max()) for t in terms)
            err = float(np.abs(res).max()) / scale
            print("NEWTON %s %s %s %.3e" % (name, tag, row, err))
            assert err <= 1e-12, (name, tag, row, err)
    assert np.array_equal(o["r3c"], x * s + o["dxa"] * o["dsa"] - sm)


@pytest.mark.parametrize("name", sorted(Q.SOLVE_PROBLEMS))
def test_float64_loop_reaches_the_constructed_optimum(name):
    A, b, c, g, u, xs, ys = Q.problem(name)
    r = Q.host_loop(name)
    print("LOOP64 %s iterations %d x_err %.3e obj_err %.3e" % (name, r["iterations"], r["x_err"], abs(r["objective"] - r["obj_star"]) / abs(r["obj_star"])))
    assert r["converged"] and r["iterations"] <= 30
    assert r["x_err"] <= 1e-7
    assert abs(r["objective"] - r["obj_star"]) <= 1e-7 * abs(r["obj_star"])
    rp, rd, gap = Q.stop_test_ld(A, b, c, g, u, r["x"], r["y"], r["s"], r["w"], r["z"])
    assert rp <= 2 * Q.TOL and rd <= 2 * Q.TOL and gap <= 2 * Q.TOL


def test_builder_asserts_its_condition():
    from interiorpointmethod_amd.workloads import separable_qp
    with pytest.raises(AssertionError):
        separable_qp(400, 520, 0)                     # 0.75 * 520 = 390 < 1.25 * 400 active columns
    A, b, c, g, u, xs, ys = separable_qp(60, 150, 0, bounded=True, mixed=True)
    assert u is not None and np.all(xs <= u) and np.any(xs == u) and np.any(g == 0) and np.all(g[xs > 0] > 0)
    assert np.array_equal(b, A @ xs)
