"""CPU tests of the NumPy restatement of iterative refinement (tests/refine_oracle.py; the rule: csrc/iteration_rules.h,
refine_decide) against an np.longdouble reference -- a double solve refined with extended-precision residuals until
stationary.

Every family x size is first asked what tests/test_gpu_refine.py will assert of the DEVICE, of the oracle alone:
  * the forward error at k = 0 exceeds 100 x the error at k = 2 (refine_oracle.oracle_meets);
  * the oracle's own error at k = 2 is stable under a different, equally legitimate double-precision factorization (LAPACK's
    blocked Cholesky of B formed from the columns in reverse order, refine_oracle.other_solver): the two agree within 4 = sqrt(16).  The GPU test allows the
    device 16 x the oracle's error "for a different factorization and summation order"; a case in which two host factorizations
    already differ by more than the square root of that margin cannot be asserted of a third.
Families that miss are dropped HERE (refine_oracle.kept_cases is what the GPU test parametrises over) and listed by the test.

Figures of the 30 cells (forward error at k = 0 / 1 / 2):
    p0-shift1e-6/130x260   9.2e-06 / 1.1e-10 / 1.5e-15        p4-shift0/130x260      9.4e-12 / 6.8e-16 / 6.9e-16
    p4-shift1e-8/130x260   1.8e-04 / 3.6e-08 / 7.2e-12        p8-shift0/130x260      3.9e-07 / 3.1e-13 / 8.6e-16
    p8-shift1e-12/130x260  6.9e-04 / 5.2e-07 / 4.0e-10        p4-shift0/257x300      6.4e-09 / 9.7e-16 / 9.7e-16
  dropped by the first condition: p4-shift1e-8/257x300 (cond 5.6e8: 0.24 / 0.062 / 0.017), p8-shift0/257x300 (cond 1.2e16),
  p8-shift1e-12/130x173 and /257x300 (cond 1e14 .. 4e15: the shifted solve has no correct digit and the half rule ends the rounds);
  dropped by the second: p8-shift0/130x173 (cond 2.2e14: 4.6e-09 with one factorization, 1.2e-07 with the other).
"""
import numpy as np
import pytest

import refine_oracle as R

ALL = [(f[0], m, n) for f in R.FAMILIES for (m, n) in R.SIZES]


def test_the_kept_cases_meet_what_the_gpu_test_asserts():
    kept = R.kept_cases()
    dropped = [k for k in ALL if k not in kept]
    print("DROPPED", dropped)
    # every family keeps its two square-ish sizes at both m: the GPU test has all five table rows to run on
    for f in R.FAMILIES:
        for m in (130, 257):
            assert (f[0], m, 2 * m) in kept and (f[0], m, 2 * m + 1) in kept, (f[0], m)
    for key in kept:
        c = R.get(*key)
        print("ERR %s cond %.1e  k=0 %.3e  k=1 %.3e  k=2 %.3e  rho %s" % (c.name, c.cond(), c.err[0], c.err[1], c.err[2],
                                                                            ["%.2e" % v for v in c.runs[2]["rho"]]))
        assert c.err[0] > R.GAIN * c.err[2]
        assert c.runs[2]["reverts"] == 0 and c.runs[2]["applied"] >= 1


@pytest.mark.parametrize("key", ALL, ids=lambda k: "%s-%dx%d" % k)
def test_oracle_error_under_another_factorization(key):
    """Kept cases are stable; a case dropped for instability alone is named."""
    c = R.get(*key)
    print("STABLE %s  guarded-loop %.3e  lapack %.3e  kept %s" % (c.name, c.err[2], c.err2_other, R.oracle_meets(c)))
    if key in R.kept_cases():
        assert R.stable(c) and c.err[0] > R.GAIN * c.err[2]
    else:
        assert not (R.stable(c) and c.err[0] > R.GAIN * c.err[2])


def test_the_bounded_handles_cases_meet_it_too():
    """refine_oracle.get_theta: d with theta = 1 / (1/d + 1) on every third column, what the bounded handle of the GPU test
    computes from its state.  Evaluated and kept or dropped by the same predicate; all ten rows the GPU test draws from pass."""
    rows = [k for k in R.kept_cases() if (k[1], k[2]) in ((130, 260), (257, 515))]
    assert len(rows) == 10
    for key in rows:
        c = R.get_theta(*key)
        print("THETA %s  k=0 %.3e  k=2 %.3e  other factorization %.3e  kept %s" % (c.name, c.err[0], c.err[2], c.err2_other, R.oracle_meets(c)))
        assert R.oracle_meets(c) and np.all(c.d > 0)


def test_the_reference_is_stationary_and_accurate():
    """The reference satisfies the unshifted equations to extended precision: its residual is below 2^-60 ||t|| cond-free."""
    for key in [("p0-shift1e-6", 130, 260), ("p8-shift0", 130, 260)]:
        c = R.get(*key)
        r = R.residual_norm(c.A, c.d, c.t, c.ref)
        assert r <= 2.0 ** -50 * np.linalg.norm(c.t) * max(1.0, c.cond() * 2.0 ** -10), (key, r)


def test_rounds_are_counted_and_k0_is_the_plain_solve():
    c = R.get("p0-shift1e-6", 130, 260)
    assert c.runs[0]["applied"] == 0 and c.runs[0]["rho"] == [] and np.array_equal(c.runs[0]["dy"], c.runs[0]["dy0"])
    assert c.runs[1]["applied"] == 1 and len(c.runs[1]["rho"]) == 1
    assert c.runs[2]["applied"] == 2 and c.runs[2]["rho"][1] < 0.5 * c.runs[2]["rho"][0]


# ---- rules 3 and 4 on the constructed case: a duplicated row, a 1e64 pivot, an inconsistent right-hand side -----------------
def test_half_rule_on_the_inconsistent_duplicated_row():
    D = R.DuplicatedRow()
    f = R.Factor(D.A, D.d, eps=D.eps)
    assert f.fixed == [D.dup] and f.L[D.dup, D.dup] == np.sqrt(R.BIG)
    t = D.inconsistent()
    o = R.refine(D.A, D.d, t, 3, f.solve)
    # the residual cannot leave e_dup (t_dup - t_src): the first correction is applied, the second round sees no halving
    assert o["applied"] == 1 and o["half"] + o["reverts"] == 1 and len(o["rho"]) == 2
    assert abs(o["rho"][0] - 1.0) < 1e-12 and abs(o["rho"][1] - 1.0) < 1e-12
    if o["rho"][1] > o["rho"][0]:
        assert o["reverts"] == 1 and np.array_equal(o["dy"], o["dy0"])
    else:
        assert o["half"] == 1
    assert R.residual_norm(D.A, D.d, t, o["dy"]) <= R.residual_norm(D.A, D.d, t, o["dy0"]) * (1 + 1e-12)
    # the consistent right-hand side on the same factor: no revert
    o = R.refine(D.A, D.d, D.consistent(), 3, f.solve)
    assert o["reverts"] == 0 and o["applied"] >= 1


def test_revert_restores_the_copy_bitwise():
    """Rule 3 needs a correction that makes the residual grow: the same guarded factor with a 1e-2 shift, and a solver that
    overshoots (2.5 B~^-1: the residual's iteration matrix is then about -1.5 I on the range).  Round 1 applies, round 2 measures
    rho_2 > rho_1 and puts (dy, a) back: bitwise the unrefined solve."""
    D = R.DuplicatedRow()
    f = R.Factor(D.A, D.d, shift=1e-2, eps=D.eps)
    t = D.consistent()
    calls = []

    def solve(r):
        calls.append(1)
        return f.solve(r) * (1.0 if len(calls) == 1 else 2.5)

    o = R.refine(D.A, D.d, t, 4, solve)
    assert o["applied"] == 1 and o["reverts"] == 1 and o["half"] == 0 and len(o["rho"]) == 2 and o["rho"][1] > o["rho"][0]
    assert np.array_equal(o["dy"], o["dy0"]) and np.array_equal(o["a"], D.A.T @ o["dy0"])
    assert len(calls) == 2          # the rounds ended: no third solve
