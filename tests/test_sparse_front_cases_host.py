"""CPU checks of tests/sparse_front_cases.py: every builder is deterministic and reaches the edge its name states, the exact references
stay in the range where every partial sum is an exact double, the envelope predictions are the listed ones, and the rounded bound
holds for NumPy's own float64 product (a sanity check of the bound, not of any kernel)."""
import numpy as np
import pytest
from scipy import sparse

from interiorpointmethod_amd import analysis

import sparse_front_cases as FC


def _formation_cases():
    cases = {"long_row_%d" % r: (lambda r=r: FC.long_row(r)) for r in (255, 256, 257, 512, 513)}
    cases.update({"long_column_%d" % c: (lambda c=c: FC.long_column(c)) for c in (255, 256, 257, 600)})
    cases["long_cross"] = FC.long_cross
    cases["term_counts"] = FC.term_counts
    cases["empty_row_and_column"] = FC.empty_row_and_column
    cases.update({"banded_%d" % m: (lambda m=m: FC.banded(m)) for m in FC.TILE_EDGE_ROWS + FC.SWITCH_ROWS})
    cases["ingest_base"] = FC.ingest_base
    return cases


CASES = _formation_cases()


def _same(A, B):
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and \
        np.array_equal(A.data, B.data)


@pytest.mark.parametrize("name", sorted(CASES))
def test_builders_are_deterministic_integer_and_canonical(name):
    A, A2 = CASES[name](), CASES[name]()
    assert _same(A, A2) and A.dtype == np.int64 and A.has_sorted_indices
    assert np.all(A.data != 0) and np.abs(A.data).max() <= 3
    R, R2 = FC.as_real(A, 3), FC.as_real(A, 3)
    assert _same(R, R2) and np.array_equal(R.indices, A.indices) and np.all(np.sign(R.data) == np.sign(A.data))


def test_other_builders_are_deterministic():
    for name in FC.ENVELOPES:
        assert _same(FC.envelope_case(name), FC.envelope_case(name))
    assert _same(FC.lds_limit(2000), FC.lds_limit(2000))
    a, b = FC.spmv_case(), FC.spmv_case()
    assert _same(a["A"], b["A"]) and all(np.array_equal(a[k], b[k]) for k in ("x", "y", "s", "b", "c"))
    A = FC.ingest_base()
    pos = FC.ingest_pair_positions(A)
    assert pos == FC.ingest_pair_positions(A)
    for kw in (dict(shuffle=True), dict(split=True), dict(pairs=pos), dict(shuffle=True, split=True, pairs=pos)):
        assert all(np.array_equal(u, v) for u, v in zip(FC.raw_csc(A, **kw), FC.raw_csc(A, **kw)))
    for n in (5, 700):
        for f in (FC.exact_d, FC.rounded_d, FC.solve_d):
            assert np.array_equal(f(n, 4), f(n, 4))


def test_exact_d_is_k_times_a_power_of_two():
    d = FC.exact_d(5000, 1)
    mant, _ = np.frexp(d)
    assert np.all(np.isin(mant * 8, [4, 5, 6, 7])) and d.min() >= 2.0 ** -8 and d.max() <= 7 * 2.0 ** 8
    assert set(np.unique(mant * 8)) == {4.0, 5.0, 6.0, 7.0}                # k = 1, 2, 4 -> 4; 5; 3, 6 -> 6; 7


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_reference_stays_exact_and_float64_reproduces_it(name):
    """Below 2^50 (asserted inside), and two float64 summation orders -- NumPy's dense product and the product with rows and columns
    reversed -- give the int64 reference bit for bit."""
    A = CASES[name]()
    d = FC.exact_d(A.shape[1], 11)
    B, mag = FC.Terms(A).exact(d)
    assert mag < 2 ** 50
    Ad = A.toarray().astype(np.float64)
    assert np.array_equal((Ad * d) @ Ad.T, B)
    Ar = np.ascontiguousarray(Ad[:, ::-1])
    assert np.array_equal((Ar * d[::-1]) @ Ar.T, B)
    assert np.array_equal(B, B.T)


def test_largest_exact_magnitudes():
    """The issue's own probe: a 600-nonzero row and a 650-nonzero column at m = 700, n = 1300 stay far below 2^50."""
    rng = np.random.default_rng(0)
    m, n = 700, 1300
    rows = np.concatenate([np.full(600, 3), rng.choice(m, size=650, replace=False)])
    cols = np.concatenate([rng.choice(n, size=600, replace=False), np.full(650, 8)])
    A = FC._csc(m, n, rows, cols, FC._nonzero_ints(rng, rows.shape[0]))
    _, mag = FC.Terms(A).exact(FC.exact_d(n, 2))
    assert mag < 2 ** 34


@pytest.mark.parametrize("name", sorted(CASES))
def test_rounded_bound_holds_for_numpys_float64_product(name):
    A = FC.as_real(CASES[name](), 5)
    d = FC.rounded_d(A.shape[1], 6)
    T = FC.Terms(A)
    ref, S = T.rounded(d)
    cnt = T.counts()
    Ad = A.toarray()
    ratio, zeros = FC.rounded_ratio((Ad * d) @ Ad.T, ref, S, cnt)
    assert zeros and ratio <= 1.0, ratio
    P = (A != 0).astype(np.int64)
    assert np.array_equal(cnt, (P @ P.T).toarray())
    wrong = (Ad * d) @ Ad.T
    i, k = np.unravel_index(np.argmax(cnt), cnt.shape)
    wrong[i, k] *= 1.0 + 1e-9                                               # a dropped term of relative size 1e-9 must not pass
    assert FC.rounded_ratio(wrong, ref, S, cnt)[0] > 1.0


@pytest.mark.parametrize("r", (255, 256, 257, 512, 513))
def test_long_row_length(r):
    A = sparse.csr_matrix(FC.long_row(r))
    cnt = np.diff(A.indptr)
    assert A.shape == (130, 600) and cnt[7] == r and np.delete(cnt, 7).max() == 3
    assert FC.formation_kernel(130) == "adat_list_kernel" and FC.formation_kernel(130, list_form=False) == "adat_sparse_kernel"


@pytest.mark.parametrize("c", (255, 256, 257, 600))
def test_long_column_length(c):
    A = FC.long_column(c)
    cnt = np.diff(A.indptr)
    assert A.shape == (640, 200) and cnt[5] == c and np.delete(cnt, 5).max() == 3


def test_long_cross():
    A = FC.long_cross()
    assert np.diff(A.indptr)[5] == 600 and np.diff(sparse.csr_matrix(A).indptr)[9] == 513 and A[9, 5] != 0


def test_term_counts_are_what_the_pairs_say():
    A = FC.term_counts()
    assert A.shape[0] == 160
    P = (A != 0).astype(np.int64)
    T = (P @ P.T).toarray()
    assert np.array_equal(T, FC.Terms(A).counts())
    pairs = FC.term_count_pairs()
    assert len(pairs) == 27 and sorted({t for _, t in pairs}) == list(FC.TERM_COUNTS)
    for (where, t), (i, k) in pairs.items():
        assert i < k and T[i, k] == t and T[k, i] == t and T[i, i] == t + 1 and T[k, k] == t + 1, (where, t)
        if where == "tile":
            assert i // 16 == k // 16
        elif where == "block":
            assert i // 16 != k // 16 and i // 128 == k // 128
        else:
            assert i // 128 != k // 128
    off = T - np.diag(np.diag(T))
    assert np.count_nonzero(off) == 2 * sum(1 for (_, t) in pairs if t > 0)


def test_empty_row_and_column():
    A = FC.empty_row_and_column()
    assert np.diff(sparse.csr_matrix(A).indptr)[17] == 0 and np.diff(A.indptr)[17] == 0
    assert np.count_nonzero(np.diff(sparse.csr_matrix(A).indptr) == 0) == 1 and np.count_nonzero(np.diff(A.indptr) == 0) == 1
    assert FC.Terms(A).counts()[17, 17] == 0
    B = FC.normal_matrix(A, FC.solve_d(A.shape[1], 1)).toarray()
    keep = np.setdiff1d(np.arange(200), [17])
    assert np.all(B[17] == 0.0) and np.linalg.eigvalsh(B[np.ix_(keep, keep)]).min() >= 0.5


def test_formation_kernel_by_size():
    lds = FC.sp_lds_max_mp()
    assert lds % 128 == 0 and lds * 8 + 4096 <= 160 * 1024                  # the accumulator row and the 4 KB of metadata fit the LDS
    assert FC.padded_rows(1536) == 1536 and FC.padded_rows(1537) == 1664 and FC.padded_rows(2304) == 2304
    assert FC.formation_kernel(1536) == "adat_list_kernel" and FC.formation_kernel(1537) == "adat_sparse_kernel"
    assert FC.padded_rows(lds) == lds and FC.formation_kernel(lds) == "adat_sparse_kernel"
    assert FC.padded_rows(lds + 1) > lds and FC.formation_kernel(lds + 1) == "adat_sparse_global_kernel"


def test_lds_limit_matrix():
    lds = FC.sp_lds_max_mp()
    for m in (lds, lds + 1):
        A = FC.lds_limit(m)
        nblk = (m + 127) // 128
        assert A.shape == (m, m + 40 * (nblk - 1))
        cnt = np.diff(sparse.csr_matrix(A).indptr)
        assert cnt.max() == 300 and np.count_nonzero(cnt > 256) == 1 and np.diff(A.indptr).max() <= 3
        last, first, flag = FC.envelope_prediction(A)
        assert flag == 1 and (last - np.arange(nblk)).max() <= 8
        d = FC.solve_d(A.shape[1], 3)
        tol, kappa = FC.solve_tolerance(FC.normal_matrix(A, d), d[:m], m)
        assert kappa < 1e4 and tol < 1e-6


@pytest.mark.parametrize("name", sorted(FC.ENVELOPES))
def test_envelope_predictions(name):
    m, pairs, flag = FC.ENVELOPES[name]
    A = FC.envelope_case(name)
    assert A.shape[0] == m and np.array_equal(A[:, :m].toarray(), np.eye(m))
    last, first, got = FC.envelope_prediction(A)
    assert got == flag
    P = sparse.csr_matrix(abs(A) @ abs(A).T)
    work, dense = analysis._tile_envelope_work(P)
    assert int(work < 0.8 * dense) == flag                                  # the package's own host rule says the same
    assert np.array_equal(last - np.arange(last.shape[0]), analysis._tile_envelope_heights(P))
    nblk = m // 128
    want = np.arange(nblk)
    for a, b in pairs:
        want[a] = max(want[a], b)
    assert np.array_equal(last, np.maximum.accumulate(want))
    for i in range(nblk):
        assert last[first[i]] >= i and (first[i] == 0 or last[first[i] - 1] < i)
    if name == "corner2048":
        assert np.all(last == nblk - 1) and work == dense
    if name == "two_groups2048":
        assert last[7] == 7 and first[8] == 8                              # forward: below clips to 0; backward: left is 0
    if name == "ragged2304":
        assert last[7] == 9 and first[8] == 6 and nblk % 8 == 2             # the envelope crosses the group boundary; two block steps
    if name == "fill2304":
        assert np.all(last[2:12] == 12) and first[12] == 2


def test_envelope_structures_go_to_the_sparse_factor_by_default(built_lib):
    """Why the GPU tests force factor="dense": the auto rule (host code of the library: ipm_order_rows) sends them to the multifrontal
    factor."""
    for name in ("ragged2304", "fill2304"):
        A = FC.as_float(FC.envelope_case(name))
        P = analysis.prepare(A, np.zeros(A.shape[0]), np.zeros(A.shape[1]))
        assert P.factor == "sparse", name


def test_spmv_case():
    c = FC.spmv_case()
    A = c["A"]
    assert A.shape == (640, 700)
    rc, cc = np.diff(sparse.csr_matrix(A).indptr), np.diff(A.indptr)
    assert rc[c["row"]] == 600 and cc[c["col"]] == 600 and rc[c["empty_row"]] == 0 and cc[c["empty_col"]] == 0
    assert np.all(c["x"] > 0) and np.all(c["s"] > 0) and c["b"].dtype == np.int64 and c["c"].dtype == np.int64
    Ad = A.toarray()
    assert np.array_equal(Ad @ c["x"], c["b"]) and np.array_equal(Ad.T @ c["y"] + c["s"], c["c"])
    assert np.abs(c["b"]).max() < 2 ** 20 and np.abs(c["c"]).max() < 2 ** 20
    # the two perturbed states leave an integer column / row as the residual; a lane-pair dropped from the 16-lane reduction changes it
    assert np.count_nonzero(Ad[:, c["col"]]) == 600 and np.count_nonzero(Ad[c["row"]]) == 600


def test_raw_csc_variants_are_the_same_matrix():
    A = FC.ingest_base()
    assert A.shape[0] == 200
    pos = FC.ingest_pair_positions(A)
    assert len({j for _, j in pos}) == len(pos) and all(A[i, j] == 0 for i, j in pos)
    ref = A.toarray().astype(np.float64)
    for kw in (dict(), dict(shuffle=True), dict(split=True), dict(pairs=pos), dict(shuffle=True, split=True, pairs=pos)):
        cp, ri, cv = FC.raw_csc(A, **kw)
        M = sparse.csc_matrix((cv, ri, cp), shape=A.shape)
        assert np.array_equal(M.toarray(), ref), kw
        if kw.get("split"):
            assert cp[-1] >= A.nnz + A.nnz // 5
        if kw.get("shuffle"):
            assert not M.has_sorted_indices
    Z = FC.with_explicit_zeros(A, pos)
    assert Z.nnz == A.nnz + len(pos) and np.array_equal(Z.toarray(), ref)
    cp, ri, cv = FC.raw_csc(A, shuffle=True, split=True, pairs=pos)
    M = sparse.csc_matrix((cv, ri, cp), shape=A.shape)
    M.sum_duplicates()
    M.sort_indices()
    assert np.array_equal(M.indptr, Z.indptr) and np.array_equal(M.indices, Z.indices) and np.array_equal(M.data, Z.data)


def test_rejected_inputs():
    A = FC.ingest_base()
    rej = FC.rejected_inputs(A)
    assert sorted(rej) == ["colptr", "nan", "row_m", "row_minus_1"]
    nnz = A.nnz
    for name, ((cp, ri, cv), code) in rej.items():
        assert cp[0] == 0 and cp[-1] == nnz and ri.shape[0] == nnz and cv.shape[0] == nnz
        assert code == (-6 if name == "nan" else -1)
        assert cp.min() >= 0 and cp.max() <= nnz                           # no reader is sent past the arrays
    cp = rej["colptr"][0][0]
    j = int(np.argmax(np.diff(cp) < 0))
    assert np.count_nonzero(np.diff(cp) < 0) == 1 and np.all(np.diff(cp[:j + 1]) >= 0)
    assert rej["row_m"][0][1].max() == 200 and rej["row_minus_1"][0][1].min() == -1 and np.isnan(rej["nan"][0][2]).sum() == 1
