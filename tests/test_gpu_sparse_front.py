"""The sparse-A front end at the structural edges of its kernels: ipm_set_A_csc (csrc/host_sparse_setup.h), the three formation kernels and
the two SpMVs of csrc/sparse_ops.h, and the tile envelope where it meets the grouped substitutions (csrc/host_factor_solve.h).  Cases and
references: tests/sparse_front_cases.py (tests/test_sparse_front_cases_host.py proves on the CPU that each case reaches its edge).

Which kernel a cell reaches follows from the size rules, there is no run-time flag: a sparse handle with the dense-tile factor and
128 < m forms B with adat_list_kernel up to 1536 padded rows (IPM_LIST_FORM=0: adat_sparse_kernel), with adat_sparse_kernel up to
SP_LDS_MAX_MP padded rows (parsed from csrc/sparse_ops.h) and with adat_sparse_global_kernel beyond; sparse_front_cases.formation_kernel
restates that rule and every cell asserts what it expects of it, next to sv.sparse, sv.factor and schedule().

References: EXACT data must come back bitwise, on every path and between the paths; ROUNDED data within the derived componentwise bound
(t + 2) 2^-53 sum_j |a_ij d_j a_kj|, entries without a shared column exactly 0.0; the two row-owner paths agree bitwise on rounded data
too (the contract of adat_list_kernel).  Solves: ||z - z_ref|| / ||z_ref|| <= 8 m 2^-53 kappa against scipy's spsolve on the CPU-formed B.
Every cell prints its ratios to the bounds (RATIO lines) before it asserts.

Observed on an MI355X (first run of this file, for the record: the bounds stay the derived ones): exact data bitwise on all three paths
of all 21 formation cases; rounded data 0.46 .. 0.64 of the bound on every path, list and row-owner bitwise equal; solves 2e-16 .. 5e-16
against tolerances of 2e-11 .. 5e-8; factor residuals 0.002 .. 0.004 of the bound, no nonzero outside a predicted envelope; the residual
norms of the SpMV case exactly 0.0 and 53.563046963368315 / 52.459508194416 as computed from the integers.  The two LDS-limit cells take
about 0.02 s each for formation, factorization, solve and spsolve together (handle and case construction below 0.01 s).
"""
import ctypes as C
import functools
import math
import time

import numpy as np
import pytest

import interiorpointmethod_amd as ipm

import sparse_front_cases as FC

pytestmark = pytest.mark.gpu

ENV = ("IPM_LIST_FORM", "IPM_ENVELOPE", "IPM_FACTOR", "IPM_FUSED_SMALL", "IPM_GROUPED_TRSV", "IPM_RAGGED_GROUPS", "IPM_FUSED_FACTOR")
PATHS = ("list", "rows", "dense")          # sparse handle; sparse handle under IPM_LIST_FORM=0; dense=True handle


def _env(monkeypatch, **more):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def _sparse(A, b=None, c=None):
    m, n = A.shape
    sv = ipm.IpmSolver(A, np.zeros(m) if b is None else b, np.zeros(n) if c is None else c, factor="dense", reorder=None)
    assert sv.sparse and sv.factor == "dense" and sv._perm is None and sv.schedule()["fused_small"] == 0
    return sv


def _handle(monkeypatch, path, A):
    _env(monkeypatch, **({"IPM_LIST_FORM": "0"} if path == "rows" else {}))
    if path == "dense":
        sv = ipm.IpmSolver(A, np.zeros(A.shape[0]), np.zeros(A.shape[1]), dense=True)
        assert not sv.sparse
        return sv
    return _sparse(A)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------------------------------------------------------- formation
FORMATION = {"long_row_%d" % r: functools.partial(FC.long_row, r) for r in (255, 256, 257, 512, 513)}
FORMATION.update({"long_column_%d" % c: functools.partial(FC.long_column, c) for c in (255, 256, 257, 600)})
FORMATION["long_cross"] = FC.long_cross
FORMATION["term_counts"] = FC.term_counts
FORMATION["empty_row_and_column"] = FC.empty_row_and_column
FORMATION.update({"banded_%d" % m: functools.partial(FC.banded, m) for m in FC.TILE_EDGE_ROWS + FC.SWITCH_ROWS})


@functools.lru_cache(maxsize=None)
def _formation_reference(name):
    """Computed once per case, shared and left unchanged: (A exact, d exact, B exact, A rounded, d rounded, ref, S, t)."""
    A = FORMATION[name]()
    n = A.shape[1]
    de = FC.exact_d(n, 31)
    Be, _ = FC.Terms(A).exact(de)
    Ar, dr = FC.as_real(A, 32), FC.rounded_d(n, 33)
    T = FC.Terms(Ar)
    ref, S = T.rounded(dr)
    out = (FC.as_float(A), de, Be, Ar, dr, ref, S, T.counts())
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(FORMATION))
def test_formation_exact_and_rounded_on_every_path(monkeypatch, name):
    Ae, de, Be, Ar, dr, ref, S, T = _formation_reference(name)
    m = Ae.shape[0]
    assert FC.formation_kernel(m) == ("adat_list_kernel" if m <= 1536 else "adat_sparse_kernel")
    assert FC.formation_kernel(m, list_form=False) == "adat_sparse_kernel"
    exact, rounded = {}, {}
    for path in PATHS:
        with _handle(monkeypatch, path, Ae) as sv:
            exact[path] = sv.form_normal_matrix(de)
        with _handle(monkeypatch, path, Ar) as sv:
            rounded[path] = sv.form_normal_matrix(dr)
    ratios = {p: FC.rounded_ratio(rounded[p], ref, S, T) for p in PATHS}
    print("RATIO %s formation: %s; exact mismatches: %s" % (
        name, ", ".join("%s %.3f" % (p, ratios[p][0]) for p in PATHS),
        ", ".join("%s %d" % (p, int(np.count_nonzero(exact[p] != Be))) for p in PATHS)))
    for p in PATHS:
        assert _bits(exact[p]) == _bits(Be), (name, p, "exact data must come back bitwise")
    for p in PATHS:
        ratio, zeros = ratios[p]
        assert zeros, (name, p, "an entry without a shared column is not exactly 0.0")
        assert ratio <= 1.0, (name, p, ratio)
    assert _bits(rounded["list"]) == _bits(rounded["rows"]), (name, "list and row-owner formation differ on rounded data")


def test_empty_row_is_one_guarded_pivot(monkeypatch):
    """The diagonal entry of the empty row is a list entry with zero terms: B carries an exact 0.0 there, the factorization guards
    exactly that pivot and the solve stays finite."""
    A = FC.as_float(FC.empty_row_and_column())
    m, n = A.shape
    d = FC.solve_d(n, 41)
    rhs = np.random.default_rng(42).standard_normal(m)
    for path in PATHS:
        with _handle(monkeypatch, path, A) as sv:
            B = sv.form_normal_matrix(d)
            assert B[17, 17] == 0.0 and not np.signbit(B[17, 17]) and np.all(B[17] == 0.0) and np.all(B[:, 17] == 0.0), path
            z = sv.normal_solve(rhs, d)
            assert sv.last_pivots_fixed == 1 and np.all(np.isfinite(z)), (path, sv.last_pivots_fixed)
            keep = np.setdiff1d(np.arange(m), [17])
            Bk = FC.normal_matrix(A, d)[keep][:, keep]
            tol, kappa = FC.solve_tolerance(Bk, d[keep], m)
            zr = FC.solve_reference(Bk, rhs[keep])
            err = float(np.linalg.norm(z[keep] - zr) / np.linalg.norm(zr))
            print("RATIO empty row %s: solve %.3g of %.3g (kappa <= %.3g)" % (path, err, tol, kappa))
            assert err <= tol, (path, err, tol)


def _solve_check(sv, A, d, rhs, label):
    m = A.shape[0]
    B = FC.normal_matrix(A, d)
    tol, kappa = FC.solve_tolerance(B, d[:m], m)
    zr = FC.solve_reference(B, rhs)
    z = sv.normal_solve(rhs, d)
    err = float(np.linalg.norm(z - zr) / np.linalg.norm(zr))
    print("RATIO %s: solve %.3g of %.3g = %.4f (kappa <= %.4g), pivots fixed %d" % (label, err, tol, err / tol, kappa, sv.last_pivots_fixed))
    assert sv.last_pivots_fixed == 0, (label, sv.last_pivots_fixed)
    assert np.all(np.isfinite(z)) and err <= tol, (label, err, tol)
    return z


@pytest.mark.parametrize("m", FC.TILE_EDGE_ROWS)
def test_row_counts_at_the_tile_edges_solve(monkeypatch, m):
    """The solve reads what form_normal_matrix hides by mirroring the lower triangle: the upper halves of the 16 x 16 diagonal tiles
    (the list builder clips them with min(i | 15, m - 1)) and the unit diagonal of the padding rows."""
    A = FC.as_float(FC.banded(m))
    d = FC.solve_d(A.shape[1], 50 + m)
    rhs = np.random.default_rng(m).standard_normal(m)
    zs = {}
    for path in PATHS:
        with _handle(monkeypatch, path, A) as sv:
            zs[path] = _solve_check(sv, A, d, rhs, "banded_%d %s" % (m, path))
    assert _bits(zs["list"]) == _bits(zs["rows"])


# ------------------------------------------------------------------------------------------------------------------- the LDS limit
@pytest.mark.parametrize("which", ("lds", "global"))
def test_formation_at_the_lds_limit(monkeypatch, which):
    """m = SP_LDS_MAX_MP: the largest LDS accumulator of adat_sparse_kernel (8 SP_LDS_MAX_MP bytes dynamic + 4 KB static of the 160 KB);
    m = SP_LDS_MAX_MP + 1: adat_sparse_global_kernel.  B (3 GB) is not fetched: the observable is the solve.
    The cell prints where its time goes (TIMES line); the module docstring records what an MI355X took."""
    _env(monkeypatch)
    lds = FC.sp_lds_max_mp()
    m = lds + (which == "global")
    assert FC.formation_kernel(m) == ("adat_sparse_kernel" if which == "lds" else "adat_sparse_global_kernel")
    t0 = time.perf_counter()
    A = FC.as_float(FC.lds_limit(m))
    d = FC.solve_d(A.shape[1], 60)
    rhs = np.random.default_rng(61).standard_normal(m)
    t1 = time.perf_counter()
    with _sparse(A) as sv:
        sch = sv.schedule()
        assert sch["blocks"] * 128 == FC.padded_rows(m) and sch["envelope"] == 1, sch
        assert (sch["blocks"] * 128 <= lds) == (which == "lds")
        t2 = time.perf_counter()
        _solve_check(sv, A, d, rhs, "lds_limit %s m=%d" % (which, m))
        t3 = time.perf_counter()
    print("TIMES lds_limit %s: case %.2f s, handle %.2f s, solve + reference %.2f s" % (which, t1 - t0, t2 - t1, t3 - t2))


# ------------------------------------------------------------------------------------------------------------------- SpMVs
def _close_ulp(got, want, ulps=4):
    return abs(got - want) <= ulps * np.spacing(want)


def test_spmv_residuals_are_exact(monkeypatch):
    """spmv_csr_kernel (r_b = A x - b) and spmv_csc_t_kernel (r_c = A^T y + s - c) on integer data with a 600-nonzero row, a 600-nonzero
    column, an empty row and an empty column: both residual norms of the matching state are exactly 0.0, and one unit step along the
    long column / long row leaves exactly that integer column / row as the residual (its 2-norm, sqrt of an integer, to 4 ulp)."""
    _env(monkeypatch)
    c = FC.spmv_case()
    A = FC.as_float(c["A"])
    x, y, s = (c[k].astype(np.float64) for k in ("x", "y", "s"))

    def norms(sv, x_, y_):
        sv.set_state(x_, y_, s)
        sv.iterate(1)
        rec = sv.history()[-1]                  # the record of the iteration just run: the norms of the state it started from
        assert rec["k"] == 0
        return rec["rp_norm"], rec["rd_norm"]

    with _sparse(A, c["b"].astype(np.float64), c["c"].astype(np.float64)) as sv:
        rp, rd = norms(sv, x, y)
        print("RATIO spmv: matching state rp %r rd %r" % (rp, rd))
        assert rp == 0.0 and rd == 0.0
        x2 = x.copy(); x2[c["col"]] += 1.0
        want = math.sqrt(int(np.sum(c["A"][:, [c["col"]]].toarray().astype(np.int64) ** 2)))
        rp, rd = norms(sv, x2, y)
        print("RATIO spmv: x + e_col rp %r (want %r) rd %r" % (rp, want, rd))
        assert want > 20.0 and _close_ulp(rp, want) and rd == 0.0
        y2 = y.copy(); y2[c["row"]] += 1.0
        want = math.sqrt(int(np.sum(c["A"][[c["row"]], :].toarray().astype(np.int64) ** 2)))
        rp, rd = norms(sv, x, y2)
        print("RATIO spmv: y + e_row rp %r rd %r (want %r)" % (rp, rd, want))
        assert want > 20.0 and rp == 0.0 and _close_ulp(rd, want)


# ------------------------------------------------------------------------------------------------------------------- raw CSC ingest
def _set_csc(sv, raw):
    cp, ri, cv = (np.ascontiguousarray(v) for v in raw)
    assert cp.dtype == np.int32 and ri.dtype == np.int32 and cv.dtype == np.float64
    return sv._lib.ipm_set_A_csc(sv._h, cp.ctypes.data_as(C.POINTER(C.c_int32)), ri.ctypes.data_as(C.POINTER(C.c_int32)),
                                 cv.ctypes.data_as(C.POINTER(C.c_double)), int(cv.shape[0]))


def _ingest_data():
    A = FC.ingest_base()
    other = A.copy()
    other.data = np.where(np.arange(other.nnz) % 3 == 0, other.data, -other.data)      # same pattern, other values
    d = FC.exact_d(A.shape[1], 71)
    return A, other, d, FC.Terms(A).exact(d)[0], FC.Terms(other).exact(d)[0], FC.ingest_pair_positions(A)


@pytest.mark.parametrize("list_form", ("unset", "0"))
def test_raw_csc_ingest_canonicalises_on_a_sparse_handle(monkeypatch, list_form):
    """ipm_set_A_csc on a live handle, as the C driver calls it: shuffled columns, entries split in two halves, cancelling pairs outside
    the pattern.  Before every variant the handle is given another matrix of the same pattern, so an ingest that did nothing fails."""
    _env(monkeypatch, **({} if list_form == "unset" else {"IPM_LIST_FORM": list_form}))
    A, other, d, B_A, B_other, pos = _ingest_data()
    assert not np.array_equal(B_A, B_other)
    with _sparse(FC.as_float(A)) as sv:                       # nnz_cap = nnz(A)
        assert _bits(sv.form_normal_matrix(d)) == _bits(B_A)
        for kw in (dict(shuffle=True), dict(split=True), dict(shuffle=True, split=True)):
            assert _set_csc(sv, FC.raw_csc(other)) == 0 and _bits(sv.form_normal_matrix(d)) == _bits(B_other), kw
            raw = FC.raw_csc(A, **kw)
            assert raw[2].shape[0] > A.nnz or not kw.get("split")          # the raw count exceeds nnz_cap, the de-duplicated one does not
            assert _set_csc(sv, raw) == 0, (kw, sv._lib.ipm_last_error(sv._h))
            assert _bits(sv.form_normal_matrix(d)) == _bits(B_A), kw
        # the cap is applied AFTER de-duplication: the cancelling pairs leave explicit zeros behind, five entries more than the cap
        assert _set_csc(sv, FC.raw_csc(other)) == 0
        assert _set_csc(sv, FC.raw_csc(A, shuffle=True, split=True, pairs=pos)) == -1
        assert b"exceeds" in sv._lib.ipm_last_error(sv._h)
        assert _bits(sv.form_normal_matrix(d)) == _bits(B_other)           # ... and the handle still serves the previous A
        for name, (raw, code) in sorted(FC.rejected_inputs(A).items()):
            assert _set_csc(sv, raw) == code, name
            assert _bits(sv.form_normal_matrix(d)) == _bits(B_other), name
        assert sv.schedule()["fused_small"] == 0
    with _sparse(FC.with_explicit_zeros(A, pos)) as sv:       # a handle sized for the pairs
        assert _bits(sv.form_normal_matrix(d)) == _bits(B_A)
        assert _set_csc(sv, FC.raw_csc(other)) == 0 and _bits(sv.form_normal_matrix(d)) == _bits(B_other)
        assert _set_csc(sv, FC.raw_csc(A, shuffle=True, split=True, pairs=pos)) == 0, sv._lib.ipm_last_error(sv._h)
        assert _bits(sv.form_normal_matrix(d)) == _bits(B_A)


def test_raw_csc_ingest_on_a_dense_handle(monkeypatch):
    """The dense-image branch of ipm_set_A_csc.  After a rejection the code has touched nothing on the device (the image is checked on
    the host before the upload): the handle serves the previous A, and exactly that is asserted."""
    _env(monkeypatch)
    A, other, d, B_A, B_other, pos = _ingest_data()
    with ipm.IpmSolver(FC.as_float(A), np.zeros(A.shape[0]), np.zeros(A.shape[1]), dense=True) as sv:
        dense_bits = _bits(sv.form_normal_matrix(d))
    assert dense_bits == _bits(B_A)
    with ipm.IpmSolver(FC.as_float(other), np.zeros(A.shape[0]), np.zeros(A.shape[1]), dense=True) as sv:
        assert not sv.sparse and _bits(sv.form_normal_matrix(d)) == _bits(B_other)
        assert _set_csc(sv, FC.raw_csc(A, shuffle=True, split=True, pairs=pos)) == 0, sv._lib.ipm_last_error(sv._h)
        assert _bits(sv.form_normal_matrix(d)) == dense_bits
        assert _set_csc(sv, FC.raw_csc(other, shuffle=True)) == 0 and _bits(sv.form_normal_matrix(d)) == _bits(B_other)
        for name, (raw, code) in sorted(FC.rejected_inputs(A).items()):
            assert _set_csc(sv, raw) == code, name
            assert _bits(sv.form_normal_matrix(d)) == _bits(B_other), name
        rhs = np.arange(1.0, A.shape[0] + 1.0)
        z = sv.normal_solve(rhs, FC.solve_d(A.shape[1], 72))
        assert sv.last_pivots_fixed == 0 and np.all(np.isfinite(z))         # still a working handle


# ------------------------------------------------------------------------------------------------------------------- envelope
@functools.lru_cache(maxsize=None)
def _envelope_reference(name):
    A = FC.envelope_case(name)
    m, n = A.shape
    d = FC.solve_d(n, 81)
    ref, _ = FC.Terms(A).rounded(d)
    ref.setflags(write=False)
    return FC.as_float(A), d, ref, FC.envelope_prediction(A)


@pytest.mark.parametrize("envelope", ("unset", "0"))
@pytest.mark.parametrize("name", sorted(FC.ENVELOPES))
def test_envelope_meets_the_grouped_substitutions(monkeypatch, name, envelope):
    """schedule()["envelope"] is the host prediction; the solve meets the bound with and without the envelope; with it, the factor is
    exactly zero in every tile outside the predicted envelope and |L L^T - B| <= (m + 2) 2^-53 |L| |L|^T componentwise (B in longdouble;
    the float64 products of the check itself spend a part of that bound, never widen it)."""
    _env(monkeypatch, **({} if envelope == "unset" else {"IPM_ENVELOPE": envelope}))
    m, _, flag = FC.ENVELOPES[name]
    A, d, Bref, (last, first, predicted) = _envelope_reference(name)
    assert predicted == flag
    rhs = np.random.default_rng(82).standard_normal(m)
    nblk = m // 128
    with _sparse(A) as sv:
        sch = sv.schedule()
        assert sch["envelope"] == (flag if envelope == "unset" else 0), sch
        assert sch["blocks"] == nblk and sch["grouped_trsv"] == 1, sch
        _solve_check(sv, A, d, rhs, "envelope %s IPM_ENVELOPE=%s" % (name, envelope))
        if envelope != "unset":
            return
        L = sv.get_factor()
    outside = 0
    if flag:
        for k in range(nblk):
            outside += int(np.count_nonzero(L[(last[k] + 1) * 128:, k * 128:(k + 1) * 128]))
    resid = np.abs((L @ L.T).astype(np.longdouble) - Bref).astype(np.float64)
    bound = (m + 2) * FC.U * (np.abs(L) @ np.abs(L).T)
    low = np.tril(np.ones((m, m), dtype=bool))
    ok = bound > 0
    ratio = float(np.max(resid[low & ok] / bound[low & ok]))
    print("RATIO envelope %s: factor residual %.4f of the bound, nonzeros outside the envelope %d" % (name, ratio, outside))
    assert outside == 0
    assert np.all(resid[low & ~ok] == 0.0)
    assert ratio <= 1.0, ratio
