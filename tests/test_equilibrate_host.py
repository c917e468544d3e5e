"""Power-of-two Ruiz equilibration, host side (no GPU): properties of the NumPy restatement of the rule (tests/equilibrate_oracle.py),
the ABI additions, and the `scale` keyword's plumbing."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import interiorpointmethod_amd as ipm                              # noqa: E402
from interiorpointmethod_amd import _lib, api, batch, batches, handle      # noqa: E402

import equilibrate_oracle as EO                                    # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipm_hip.h")


def wild_matrix(m, n, seed, density=0.3):
    """Entries +-2^U(-40, 40) U(1, 2); row 1 and column 2 empty (when they exist); as CSC triplets WITH duplicate entries."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    mask[0, 0] = True
    if m > 2:
        mask[1, :] = False
    if n > 3:
        mask[:, 2] = False
    i, j = np.nonzero(mask)
    v = rng.choice([-1.0, 1.0], i.size) * 2.0 ** rng.uniform(-40, 40, i.size) * rng.uniform(1, 2, i.size)
    k = max(1, i.size // 5)                                        # a fifth of the entries twice: duplicates sum
    i, j, v = np.concatenate([i, i[:k]]), np.concatenate([j, j[:k]]), np.concatenate([v, 0.5 * v[:k]])
    return sparse.csc_matrix(sparse.coo_matrix((v, (i, j)), shape=(m, n)))


@pytest.mark.parametrize("m,n,seed", [(1, 1, 0), (3, 5, 1), (40, 90, 2), (130, 257, 3)])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_oracle_properties(m, n, seed, kind):
    A = wild_matrix(m, n, seed)
    D = A.toarray()
    M = A if kind == "sparse" else D
    er, ec, changed = EO.ruiz(M, 64)
    assert changed < 64, "the fixed point was not reached"
    r, c = EO.factors(er, ec)
    for f in (r, c):                                               # every factor is a power of two
        mant, _ = np.frexp(f)
        assert np.all(mant == 0.5)
    empty_r, empty_c = np.abs(D).max(axis=1) == 0, np.abs(D).max(axis=0) == 0
    assert np.all(r[empty_r] == 1.0) and np.all(c[empty_c] == 1.0)
    if m > 2:
        assert empty_r[1]
    if n > 3:
        assert empty_c[2]
    rmax, cmax = EO.maxima(M, er, ec)
    for mx, empty in ((rmax, empty_r), (cmax, empty_c)):           # the fixed point: every non-empty maximum in [0.5, 2)
        assert np.all((mx[~empty] >= 0.5) & (mx[~empty] < 2.0)) and np.all(mx[empty] == 0.0)
    er2, ec2, changed2 = EO.ruiz(M, changed + 1)                   # a further pass is the identity
    assert changed2 == changed and np.array_equal(er2, er) and np.array_equal(ec2, ec)
    er1, ec1, ch1 = EO.ruiz(M, 1)                                  # the cap caps
    assert ch1 == min(1, changed)
    # dense and sparse agree, and the prescaled arrays are R A C etc. exactly
    era, eca, cha = EO.ruiz(D, 64)
    assert cha == changed and np.array_equal(era, er) and np.array_equal(eca, ec)
    rng = np.random.default_rng(seed + 100)
    b, cc = rng.standard_normal(m), rng.standard_normal(n)
    u = np.where(rng.random(n) < 0.5, rng.uniform(1, 3, n), np.inf)
    A2, b2, c2, u2 = EO.prescale(M, b, cc, u, er, ec)
    A2 = A2.toarray() if sparse.issparse(A2) else A2
    want = np.array([[np.ldexp(D[i, j], int(er[i] + ec[j])) for j in range(n)] for i in range(m)]).reshape(m, n)
    assert np.array_equal(A2, want)
    assert np.array_equal(A2, r[:, None] * D * c[None, :])         # (multiplying by powers of two is the same thing)
    assert np.array_equal(b2, r * b) and np.array_equal(c2, c * cc) and np.array_equal(u2, u / c)
    assert np.all(np.isinf(u2) == np.isinf(u))


def test_shift_is_floor_division():
    v = np.array([0.0, 0.25, 0.4999, 0.5, 1.0, 1.9999, 2.0, 3.9, 4.0, 2.0 ** -3, 2.0 ** -4, 2.0 ** 101])
    # frexp exponents: -, -1, -1, 0, 1, 1, 2, 2, 3, -2, -3, 102
    assert list(EO.shift(v)) == [0, 1, 1, 0, 0, 0, -1, -1, -1, 1, 2, -51]


def test_header_and_exports(built_lib):
    txt = open(HEADER).read()
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt) and _lib.ABI_VERSION == 4
    for name, args in (("ipm_equilibrate", ["ipm_handle*", "int32_t", "double"]),
                       ("ipm_get_scaling", ["ipm_handle*", "double*", "double*"])):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
        assert decl, "include/ipm_hip.h does not declare %s" % name
        types = [re.sub(r"\s*\w+(\[\d+\])?$", "", a.strip()).replace(" ", "") for a in decl.group(1).split(",")]
        assert types == args, (name, types)
        assert hasattr(C.CDLL(built_lib), name) and name in _lib.EXPORTS
    lib = _lib.load()
    assert lib.ipm_abi_version() == 4
    assert lib.ipm_equilibrate(None, 16, None) == -1 and lib.ipm_get_scaling(None, None, None) == -1


def test_bogus_scale_is_refused_before_any_handle(monkeypatch):
    made = []
    monkeypatch.setattr(batches, "IpmSolver", lambda *a, **k: made.append(1))
    monkeypatch.setattr(api, "IpmSolver", lambda *a, **k: made.append(1))
    monkeypatch.setattr(_lib, "load", lambda: made.append(2))
    A = np.array([[1.0, 2.0]])
    b, c = np.ones(1), np.ones(2)
    with pytest.raises(ValueError, match="scale"):
        handle.IpmSolver(A, b, c, scale="bogus")
    with pytest.raises(ValueError, match="scale"):
        ipm.solve_with_info(A, b, c, scale="bogus")
    with pytest.raises(ValueError, match="scale"):
        ipm.solve(A, b, c, scale="bogus")
    with pytest.raises(ValueError, match="scale"):
        ipm.interior_sparse(A, b, c, scale="bogus")
    with pytest.raises(ValueError, match="scale"):
        ipm.solve_small_batch([(A, b, c)], scale="bogus")
    with pytest.raises(ValueError, match="scale"):
        batch.solve_shard_lockstep([(A, b, c)], [0], scale="bogus")
    assert not made


def test_scale_reaches_the_solver(monkeypatch):
    """solve_with_info, solve_small_batch and the general-form entry hand `scale` and `scale_passes` to IpmSolver."""
    seen = []

    class Stop(Exception):
        pass

    def fake(*a, **k):
        seen.append((k.get("scale"), k.get("scale_passes")))
        raise Stop

    monkeypatch.setattr(api, "IpmSolver", fake)
    monkeypatch.setattr(batches, "IpmSolver", fake)
    A = np.array([[1.0, 2.0]])
    b, c = np.ones(1), np.ones(2)
    with pytest.raises(Stop):
        ipm.solve_with_info(A, b, c, scale="ruiz", scale_passes=5)
    with pytest.raises(Stop):
        ipm.solve_small_batch([(A, b, c)], scale="ruiz")
    with pytest.raises(Stop):
        ipm.new_interior_sparse(c, Aeq=sparse.csc_matrix(A), beq=b, lb=np.zeros(2), ub=np.full(2, np.inf), scale="ruiz", scale_passes=3)
    with pytest.raises(Stop):
        ipm.solve_with_info(A, b, c)
    assert seen == [("ruiz", 5), ("ruiz", handle.SCALE_PASSES), ("ruiz", 3), (None, None)]


def test_run_batch_passes_scale_on(monkeypatch):
    seen = {}

    def fake(problems, ids, **kw):
        seen.update(kw)
        return np.zeros((len(ids), batch.NF))
    monkeypatch.setattr(batch, "solve_shard_lockstep", fake)
    A = np.ones((200, 3))
    batch.run_batch([(A, None, None)], workers=2, lockstep=True, scale="ruiz")
    assert seen.get("scale") == "ruiz"
    got = {}
    monkeypatch.setattr(batch, "solve_with_info", lambda *a, **k: (got.update(k), (None, None, None, {}))[1])
    batch.solve_one((A, None, None), scale="ruiz", scale_passes=7)
    assert got.get("scale") == "ruiz" and got.get("scale_passes") == 7
