"""Host checks (no GPU) of the exact guard cases in guard_cases.py: every claim test_gpu_pivot_guard.py relies on."""
import numpy as np
import pytest

from guard_cases import BIG, EPS, GuardCase, auto_shift_boundary, guard_rows, host_guarded_factor

SIZES = [1, 17, 128, 129, 300, 700, 1100, 2100, 2500]


def _cases(m):
    yield GuardCase(m)
    if m >= 17:
        yield GuardCase(m, boundary=True, negative=True, seed=1)
        yield GuardCase(m, boundary=True, negative=True, seed=2, eps=2.0 ** -60)


@pytest.mark.parametrize("m", SIZES)
def test_structure_and_exact_formation(m):
    for c in _cases(m):
        N = c.N
        assert np.all(np.tril(N, -1) == N) and not np.any(N @ N)              # strictly lower, N N = 0
        hubs = np.flatnonzero(np.any(N, axis=0))
        assert np.all(np.count_nonzero(N, axis=0)[hubs] == 1)                # every hub serves one row
        assert not set(hubs) & set(c.guarded) and not set(hubs) & set(c.decoupled)
        assert not set(hubs) & set(np.flatnonzero(np.any(N, axis=1)))        # hubs are never coupled or dependent
        assert m == 1 or (0 in c.guarded and 0 in c.empty and not np.any(c.A[0]))
        assert set(guard_rows(m)) <= set(c.guarded)
        for j in c.dependent:                                                # an exact combination of its hub rows
            assert c.L0[j, j] == 0.0 and np.any(c.A[j])
            assert np.array_equal(c.A[j], N[j] @ c.A)
        B = c.B()
        # exact in fp64: the integer product L0 L0^T off the decoupled rows, d_j alone on them, whatever the order of the sum
        assert np.all(np.abs(c.L0) <= 1) and np.all(c.L0 == np.round(c.L0))
        Bi = c.L0 @ c.L0.T                     # entries of magnitude <= m: every partial sum is an exact fp64 integer
        dec = np.array(sorted(c.decoupled), dtype=np.int64)
        Bi[dec, dec] = [c.decoupled[r] for r in dec]
        assert np.array_equal(B, Bi)
        Ar = np.ascontiguousarray(c.A[:, ::-1])
        assert np.array_equal(B, (Ar * c.d[::-1]) @ Ar.T)
        assert np.array_equal(B, B.T)
        assert np.max(np.diag(B)) == c.maxdiag and np.max(np.abs(B)) == c.maxdiag
        Bs = c.B(4.0 ** -70)
        assert np.array_equal(Bs, B * 2.0 ** -140)                           # scaling d by 4^k scales B exactly


@pytest.mark.parametrize("m", [1, 17, 128, 129, 300, 700])
def test_rank_and_reduced_system(m):
    for c in _cases(m):
        B = c.B()
        # without the decoupled rows (whose tiny diagonals a rank test cannot tell from zero) B has rank deficiency exactly
        # the number of dependent and empty rows
        rest = np.array([j for j in range(m) if j not in c.decoupled], dtype=np.int64)
        Br = B[np.ix_(rest, rest)]
        assert len(rest) - (np.linalg.matrix_rank(Br) if len(rest) else 0) == len(c.dependent) + len(c.empty)
        assert set(c.guarded) - set(c.decoupled) == set(c.dependent) | set(c.empty)
        # the reduced system is nonsingular: full rank off the decoupled rows, a positive diagonal alone on them
        kc = np.array([j for j in c.keep if j not in c.decoupled], dtype=np.int64)
        assert len(kc) == 0 or np.linalg.matrix_rank(B[np.ix_(kc, kc)]) == len(kc) and np.all(np.isfinite(np.linalg.cholesky(B[np.ix_(kc, kc)])))
        for r in c.decoupled:
            assert np.count_nonzero(B[r]) == 1 and (r not in c.keep or B[r, r] > 0)


@pytest.mark.parametrize("m", [1, 17, 128, 129, 300])
def test_host_guarded_factor_is_the_closed_form(m):
    for c in list(_cases(m))[-2:]:
        B = c.B()
        L, fixed = host_guarded_factor(B, eps=c.eps)
        assert fixed == c.guarded
        E = c.expected_factor()
        keep, g = c.keep, c.guarded
        inexact = c.inexact_diag()
        Lc, Ec = L.copy(), E.copy()
        for r in inexact:
            assert abs(Lc[r, r] - Ec[r, r]) <= 2 * np.spacing(Ec[r, r])
            Lc[r, r] = Ec[r, r]
        assert np.array_equal(Lc[:, keep], Ec[:, keep])                      # bitwise: unit pivots, integer updates
        assert np.all(np.abs(np.diag(L)[g] - np.sqrt(BIG)) <= 2 * np.spacing(np.sqrt(BIG)))
        assert np.all(np.tril(L, -1)[:, g] == 0.0)                            # host order: exactly zero
        for k in ((-150, -70, 70) if m <= 129 else (-70,)):                 # same decisions, L scaled by exactly 2^k
            Ls, fs = host_guarded_factor(c.B(4.0 ** k), eps=c.eps)
            assert fs == c.guarded
            assert np.array_equal(Ls[:, keep], L[:, keep] * 2.0 ** k)


def test_threshold_rows_sit_exactly_at_the_threshold():
    for eps in (EPS, 2.0 ** -60):
        c = GuardCase(300, boundary=True, negative=True, eps=eps)
        B = c.B()
        t = eps * np.max(np.diag(B))
        assert B[c.role["t"], c.role["t"]] == t
        assert B[c.role["t-"], c.role["t-"]] == np.nextafter(t, 0) and B[c.role["t+"], c.role["t+"]] == np.nextafter(t, np.inf)
        assert c.role["t+"] not in c.guarded and {c.role["t-"], c.role["t"], c.role["neg"]} <= set(c.guarded)


def test_nan_diagonal_never_wins_the_max_on_the_host():
    c = GuardCase(129, boundary=True, seed=3)
    B = c.B()
    plain = [j for j in c.keep if j not in c.decoupled and not np.any(c.N[j]) and not np.any(c.N[:, j])]
    j = plain[3]
    B[j, :] = 0.0
    B[:, j] = 0.0
    B[j, j] = np.nan
    L, fixed = host_guarded_factor(B)
    assert fixed == sorted(c.guarded + [int(j)])


@pytest.mark.parametrize("m", [27, 120, 200, 300, 1000])
def test_auto_shift_boundary(m):
    k = auto_shift_boundary(m)
    assert not (float(k) > 0.05 * float(m)) and float(k + 1) > 0.05 * float(m)
    assert k == int(0.05 * m + 1e-9) or float(k) == 0.05 * m


def test_reduced_solution_drops_the_guarded_rows():
    c = GuardCase(300, boundary=True, negative=True)
    B = c.B()
    rhs = np.random.default_rng(0).standard_normal(c.m)
    z = c.reduced_solution(B, rhs)
    L, _ = host_guarded_factor(B)
    zh = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    assert np.all(np.abs(zh[c.guarded]) <= 1e-60 * np.linalg.norm(rhs))
    assert np.max(np.abs(zh[c.keep] - z[c.keep])) <= 1e-10 * np.max(np.abs(z))
