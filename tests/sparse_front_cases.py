"""Host-only builders and references for the sparse-A front end (csrc/sparse_ops.h, ipm_set_A_csc in csrc/host_sparse_setup.h, the tile
envelope where it meets the grouped substitutions of csrc/host_factor_solve.h).  Nothing here imports the library: tests/
test_sparse_front_cases_host.py proves on the CPU that each builder reaches the edge its name states, tests/test_gpu_sparse_front.py runs
the kernels on them.

Two references of B = A diag(d) A^T, both from the TERM TABLE of A (one record per column j and pair of rows (i, k) of that column):

EXACT.    A has integer entries in [-3, 3] and d_j = k 2^e with k in 1..7, e in -8..8.  Every product a_ij d_j a_kj is then a multiple of
          2^-8 below 63 * 2^8, and every partial sum of an entry of B is a multiple of 2^-8 below 2^-8 * 2^53 as long as
          2^8 sum_j |a_ij d_j a_kj| < 2^53 (exact_reference asserts < 2^50): an exact double in any order and any association.  The
          reference is summed in int64 (scaled by 2^8); a kernel must reproduce it BITWISE, whatever its summation order.
ROUNDED.  A and d real, d = 10^U(-6, 6).  The reference is summed in np.longdouble (x87: 64 bits of significand).  A kernel that forms
          coef = fl(a_ij d_j), then fl(coef a_kj) (two roundings per term), and adds the t_ik terms in some order (t_ik - 1 additions)
          obeys, to first order,     |B_ik - ref_ik| <= (t_ik + 2) 2^-53 sum_j |a_ij d_j a_kj|
          (2 roundings of relative size u = 2^-53 on every term, and every term passes through at most t - 1 additions: (t + 1) u; the
          bound carries one more u for the second-order terms and the reference's own 2^-64 t error).  t_ik = 0: exactly 0.0.

Solve bound (solve_tolerance): for A = [I | C], B = D_1 + C D_2 C^T with D_1 = d of the identity columns, so lambda_min(B) >= min D_1 and
kappa_2(B) <= ||B||_2 / min D_1 <= ||B||_1 / min D_1 (B symmetric).  Tolerance on ||z - z_ref||_2 / ||z_ref||_2: 8 m 2^-53 kappa -- the
textbook Cholesky-solve bound has a constant of order m; 8 covers the substitutions that multiply by explicit block and group inverses.
"""
import re
import os

import numpy as np
from scipy import sparse

U = 2.0 ** -53
NB = 128                 # rows of a block of the blocked Cholesky (csrc: NB)
GS = 8                   # blocks of a group of the grouped substitutions (csrc: GS_MAX; groups from 16 blocks on, ragged)
LIST_MAX_MP = 1536       # sparse handles up to this many padded rows form B from the product list (host_sparse_setup.h: want_list)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sp_lds_max_mp():
    """SP_LDS_MAX_MP as csrc/sparse_ops.h states it: the last padded row count adat_sparse_kernel serves from LDS."""
    with open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "sparse_ops.h")) as f:
        mt = re.search(r"constexpr\s+int\s+SP_LDS_MAX_MP\s*=\s*(\d+)\s*;", f.read())
    assert mt, "csrc/sparse_ops.h no longer defines SP_LDS_MAX_MP"
    return int(mt.group(1))


def padded_rows(m):
    """mp of the handle's layout (host_handle.h: make_layout): 128-row blocks, padded on to whole groups of 8 blocks when that costs
    at most 1/8 more blocks (from 16 blocks on)."""
    nb = (m + NB - 1) // NB
    nb8 = (nb + GS - 1) // GS * GS
    if nb >= 2 * GS and (nb8 - nb) * 8 <= nb:
        nb = nb8
    return nb * NB


def formation_kernel(m, list_form=True):
    """The kernel that forms B on a sparse handle of m > 128 rows with the dense-tile factor (host_factor_solve.h: enqueue_form)."""
    mp = padded_rows(m)
    if list_form and mp <= LIST_MAX_MP:
        return "adat_list_kernel"
    return "adat_sparse_kernel" if mp <= sp_lds_max_mp() else "adat_sparse_global_kernel"


# ------------------------------------------------------------------------------------------------------------------- data
def _nonzero_ints(rng, size):
    v = rng.integers(1, 4, size=size)
    return v * rng.choice([-1, 1], size=size)


def _csc(m, n, rows, cols, vals):
    """int64 CSC from triplets; a repeated position keeps its first value (the builders place structure, not sums)."""
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.int64)
    key = cols * m + rows
    _, first = np.unique(key, return_index=True)
    A = sparse.csc_matrix((vals[first], (rows[first], cols[first])), shape=(m, n), dtype=np.int64)
    A.sort_indices()
    assert A.nnz == first.shape[0] and np.all(A.data != 0)
    return A


def exact_d(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 8, size=n).astype(np.float64) * 2.0 ** rng.integers(-8, 9, size=n)


def rounded_d(n, seed):
    return 10.0 ** np.random.default_rng(seed).uniform(-6.0, 6.0, n)


def solve_d(n, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, n)


def as_real(A, seed):
    """The pattern of the integer matrix A with real values: every entry times a factor in [0.5, 1.5)."""
    R = sparse.csc_matrix(A, dtype=np.float64, copy=True)
    R.data = R.data * np.random.default_rng(seed).uniform(0.5, 1.5, R.nnz)
    return R


def as_float(A):
    return sparse.csc_matrix(A, dtype=np.float64, copy=True)


# ------------------------------------------------------------------------------------------------------------------- references
class Terms:
    """Term table of A: for every column j and every ordered pair (i, k) of its rows one record, grouped by entry (i, k) of B."""

    def __init__(self, A):
        A = sparse.csc_matrix(A)
        A.sort_indices()
        self.m = A.shape[0]
        cnt = np.diff(A.indptr).astype(np.int64)
        ncol = cnt.shape[0]
        rep = np.repeat(cnt, cnt)                                   # per nonzero: the length of its column
        first = np.repeat(np.arange(A.nnz, dtype=np.int64), rep)    # left nonzero of every pair
        start = np.repeat(np.repeat(A.indptr[:-1].astype(np.int64), cnt), rep)
        off = np.arange(first.shape[0], dtype=np.int64) - np.repeat(np.cumsum(rep) - rep, rep)
        second = start + off
        self.col = np.repeat(np.repeat(np.arange(ncol, dtype=np.int64), cnt), rep)
        flat = A.indices[first].astype(np.int64) * self.m + A.indices[second]
        order = np.argsort(flat, kind="stable")
        self.first, self.second, self.col, flat = first[order], second[order], self.col[order], flat[order]
        self.entry, self.seg = np.unique(flat, return_index=True)    # distinct entries (i * m + k) and where their terms begin
        self.data = A.data

    def _dense(self, values, dtype):
        out = np.zeros(self.m * self.m, dtype=dtype)
        if values.shape[0]:
            out[self.entry] = np.add.reduceat(values, self.seg)
        return out.reshape(self.m, self.m)

    def counts(self):
        """t_ik: the columns that rows i and k share."""
        return self._dense(np.ones(self.first.shape[0], dtype=np.int64), np.int64)

    def exact(self, d):
        """-> (B as float64, max over entries of 2^8 sum_j |a_ij d_j a_kj|).  Integer A, d = k 2^e with e >= -8."""
        a = self.data.astype(np.int64)
        d8 = np.asarray(d, dtype=np.float64) * 256.0
        di = d8.astype(np.int64)
        assert np.array_equal(di.astype(np.float64), d8) and np.array_equal(a.astype(self.data.dtype), self.data)
        prod = a[self.first] * di[self.col] * a[self.second]
        B8 = self._dense(prod, np.int64)
        mag = int(self._dense(np.abs(prod), np.int64).max())
        assert mag < 2 ** 50, "exact case leaves the range in which every partial sum is an exact double"
        return B8.astype(np.float64) / 256.0, mag

    def rounded(self, d):
        """-> (ref as longdouble, S = sum_j |a_ij d_j a_kj| as float64 rounded up by one ulp)."""
        a = self.data.astype(np.longdouble)
        dl = np.asarray(d, dtype=np.float64).astype(np.longdouble)
        prod = a[self.first] * dl[self.col] * a[self.second]
        ref = self._dense(prod, np.longdouble)
        S = np.nextafter(self._dense(np.abs(prod), np.longdouble).astype(np.float64), np.inf)
        return ref, S


def rounded_bound(T, S):
    return (T + 2.0) * U * S


def rounded_ratio(B, ref, S, T):
    """(largest |B - ref| / bound over the entries with t > 0, are the t = 0 entries all exactly 0.0?)"""
    err = np.abs(np.asarray(B, dtype=np.float64).astype(np.longdouble) - ref).astype(np.float64)
    bound = rounded_bound(T, S)
    nz = T > 0
    ratio = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    return ratio, bool(np.all(np.asarray(B)[~nz] == 0.0))


def normal_matrix(A, d):
    """A diag(d) A^T as float64 CSC: what the solve references factor."""
    A = sparse.csc_matrix(A, dtype=np.float64)
    return sparse.csc_matrix((A @ sparse.diags(np.asarray(d, dtype=np.float64))) @ A.T)


def solve_tolerance(B, d_identity, m):
    """(8 m 2^-53 kappa, kappa) with kappa = ||B||_1 / min d over the identity columns (module docstring)."""
    kappa = float(abs(B).sum(axis=0).max()) / float(np.min(d_identity))
    return 8.0 * m * U * kappa, kappa


def solve_reference(B, rhs):
    from scipy.sparse.linalg import spsolve
    return spsolve(sparse.csc_matrix(B), rhs)


# ------------------------------------------------------------------------------------------------------------------- formation cases
def long_row(r, m=130, n=600, row=7, seed=1):
    """One row with exactly r nonzeros (columns 0 .. r-1), every other row three: the 256-nonzero chunk loop of adat_sparse_kernel
    takes a second (r > 256) and third (r > 512) trip for that row only."""
    rng = np.random.default_rng(seed * 1000 + r)
    rows, cols = [np.full(r, row)], [np.arange(r)]
    for i in range(m):
        if i != row:
            rows.append(np.full(3, i)); cols.append(rng.choice(n, size=3, replace=False))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc(m, n, rows, cols, _nonzero_ints(rng, rows.shape[0]))


def long_column(c, m=640, n=200, col=5, seed=2):
    """One column with exactly c nonzeros, every other column three: the 256-lane stride over a column (q += 256) takes a second
    (c > 256) and third (c > 512) trip in every row of B that column touches."""
    rng = np.random.default_rng(seed * 1000 + c)
    rows, cols = [np.sort(rng.choice(m, size=c, replace=False))], [np.full(c, col)]
    for j in range(n):
        if j != col:
            rows.append(rng.choice(m, size=3, replace=False)); cols.append(np.full(3, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc(m, n, rows, cols, _nonzero_ints(rng, rows.shape[0]))


def long_cross(m=640, n=600, row=9, col=5, r=513, c=600, seed=3):
    """A 513-nonzero row and a 600-nonzero column that cross in a nonzero."""
    rng = np.random.default_rng(seed)
    others = np.sort(rng.choice(np.setdiff1d(np.arange(m), [row]), size=c - 1, replace=False))
    rows = [np.full(r, row), others]
    cols = [np.arange(r), np.full(c - 1, col)]             # the row's columns 0 .. r-1 include `col`: the crossing
    for j in range(r, n):
        rows.append(rng.choice(np.setdiff1d(np.arange(m), [row]), size=2, replace=False)); cols.append(np.full(2, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc(m, n, rows, cols, _nonzero_ints(rng, rows.shape[0]))


TERM_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 24)


def term_count_pairs():
    """{(placement, t): (i, k)} with i < k: inside one 16 x 16 diagonal tile, across two tiles of one 128-block, across two blocks."""
    pairs = {}
    for p, t in enumerate(TERM_COUNTS):
        pairs[("tile", t)] = (2 * p, 2 * p + 1)
        pairs[("block", t)] = (20 + p, 40 + p)
        pairs[("blocks", t)] = (60 + p, 130 + p)
    return pairs


def term_counts(m=160, seed=4):
    """[I | P]: every pair of term_count_pairs() owns t private columns, so its two rows share exactly t columns (and the diagonal
    entries of its rows carry t + 1 terms).  The list kernel takes the terms eight at a time and then one by one."""
    rng = np.random.default_rng(seed)
    rows, cols = [np.arange(m)], [np.arange(m)]
    n = m
    for (_, t), (i, k) in sorted(term_count_pairs().items()):
        for _ in range(t):
            rows.append(np.array([i, k])); cols.append(np.array([n, n]))
            n += 1
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc(m, n, rows, cols, _nonzero_ints(rng, rows.shape[0]))


def empty_row_and_column(m=200, extra=260, hole=17, seed=5):
    """[I | R] with row `hole` emptied: that row and column `hole` (its identity column) are both empty.  B[hole, hole] is a list entry
    with zero terms; every other row keeps its identity column, so B is positive definite off that row: ONE guarded pivot."""
    rng = np.random.default_rng(seed)
    keep = np.setdiff1d(np.arange(m), [hole])
    rows, cols = [keep], [keep]
    for j in range(extra):
        rows.append(rng.choice(keep, size=3, replace=False)); cols.append(np.full(3, m + j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc(m, m + extra, rows, cols, _nonzero_ints(rng, rows.shape[0]))


def banded(m, offsets=(1, 5), seed=6):
    """[I | C]: for every offset o and row i < m - o one column of C with entries in rows i and i + o."""
    rng = np.random.default_rng(seed * 100000 + m)
    rows, cols = [np.arange(m)], [np.arange(m)]
    n = m
    for o in offsets:
        k = m - o
        if k <= 0:
            continue
        i = np.arange(k)
        rows += [i, i + o]; cols += [n + i, n + i]
        n += k
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = _nonzero_ints(rng, rows.shape[0])
    vals[:m] = 1
    return _csc(m, n, rows, cols, vals)


TILE_EDGE_ROWS = (129, 143, 144, 145, 255, 256, 257)
SWITCH_ROWS = (LIST_MAX_MP, LIST_MAX_MP + 1)


# ------------------------------------------------------------------------------------------------------------------- block couplings
def coupled_blocks(m, pairs, per_pair=6, seed=7, long_row=None):
    """[I | C]: per_pair columns of C for every (a, b) of `pairs`, each with one entry in a row of 128-block a and one in a row of
    block b.  long_row = (row, count, blocks): `row` gets entries of +-1 in further columns of C that touch `blocks` only, until it
    holds exactly `count` nonzeros."""
    rng = np.random.default_rng(seed)
    nblk = (m + NB - 1) // NB
    rows, cols, vals = [np.arange(m)], [np.arange(m)], [np.ones(m, dtype=np.int64)]
    n = m
    colblocks = []
    for a, b in pairs:
        assert 0 <= a <= b < nblk
        ra = a * NB + rng.integers(0, min(NB, m - a * NB), size=per_pair)
        rb = b * NB + rng.integers(0, min(NB, m - b * NB), size=per_pair)
        if a == b:
            rb = np.where(rb == ra, a * NB + (rb - a * NB + 1) % min(NB, m - a * NB), rb)
        j = n + np.arange(per_pair)
        rows += [ra, rb]; cols += [j, j]; vals += [_nonzero_ints(rng, per_pair), _nonzero_ints(rng, per_pair)]
        colblocks += [(a, b)] * per_pair
        n += per_pair
    if long_row is not None:
        row, count, blocks = long_row
        lo, hi = min(blocks), max(blocks)
        cand = np.array([m + q for q, (a, b) in enumerate(colblocks) if lo <= a and b <= hi], dtype=np.int64)
        have = np.concatenate(cols)[np.concatenate(rows) == row]
        cand = np.setdiff1d(cand, have)
        need = count - have.shape[0]
        assert 0 < need <= cand.shape[0]
        pick = np.sort(rng.choice(cand, size=need, replace=False))
        rows.append(np.full(need, row)); cols.append(pick); vals.append(rng.choice([-1, 1], size=need))
    return _csc(m, n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def lds_limit(m, seed=8):
    """The matrix of the LDS-limit cases: 40 columns of C per pair of neighbouring 128-blocks, and one row in the middle block with
    exactly 300 nonzeros (a second trip of the 256-nonzero chunk loop) that stay within four blocks of its own."""
    nblk = (m + NB - 1) // NB
    k0 = nblk // 2
    return coupled_blocks(m, [(k, k + 1) for k in range(nblk - 1)], per_pair=40, seed=seed,
                          long_row=(k0 * NB + 3, 300, (k0 - 4, k0 + 4)))


def envelope_prediction(A):
    """The host rule of ipm_set_A_csc (and analysis._tile_envelope_work) -> (last, first, flag): last[k] = last 128-row block with a
    structural nonzero at or left of block column k (monotone), first[i] = first block column with last >= i, flag = the envelope
    removes at least a fifth of the block work."""
    A = sparse.csc_matrix(A)
    A.sort_indices()
    nblk = (A.shape[0] + NB - 1) // NB
    last = np.arange(nblk)
    for j in range(A.shape[1]):
        r = A.indices[A.indptr[j]:A.indptr[j + 1]]
        if r.shape[0]:
            np.maximum.at(last, r // NB, r[-1] // NB)
    last = np.maximum.accumulate(last)
    first = np.array([int(np.argmax(last >= i)) for i in range(nblk)])
    k = np.arange(nblk)
    work, dense = float(np.sum((last - k) ** 2)), float(np.sum((nblk - 1 - k) ** 2))
    return last, first, int(work < 0.8 * dense)


def _chain(nblk):
    return [(k, k + 1) for k in range(nblk - 1)]


# name -> (m, block pairs, predicted envelope flag, what the structure does to enqueue_potrs_grouped)
ENVELOPES = {
    "band1024": (1024, _chain(8), 1),                                            # one group: nothing below it, nothing left of it
    "two_groups2048": (2048, [(k, k + 1) for k in range(15) if k != 7], 1),      # no coupling between the groups: below = 0, left = 0
    "ragged2304": (2304, _chain(18) + [(k, k + 2) for k in range(16)], 1),       # crosses the group boundary; blocks 16, 17: block steps
    "fill2304": (2304, _chain(18) + [(2, 12)], 1),                               # monotone fill widens block columns 3 .. 11
    "corner2048": (2048, [(0, 15)], 0),                                          # work = dense: the envelope must stay off
}


def envelope_case(name):
    m, pairs, _ = ENVELOPES[name]
    return coupled_blocks(m, pairs, per_pair=1 if name == "corner2048" else 6, seed=20 + sorted(ENVELOPES).index(name))


# ------------------------------------------------------------------------------------------------------------------- SpMV case
def spmv_case(m=640, n=700, row=11, col=13, empty_row=200, empty_col=300, seed=9):
    """Integer A with a 600-nonzero row, a 600-nonzero column, an empty row and an empty column, and integer (x, y, s) with x, s > 0:
    b = A x and c = A^T y + s in int64, so both residuals of that state are exactly zero in any summation order."""
    rng = np.random.default_rng(seed)
    free_r = np.setdiff1d(np.arange(m), [row, empty_row])
    free_c = np.setdiff1d(np.arange(n), [col, empty_col])
    rows = [np.full(599, row), rng.choice(free_r, size=599, replace=False), np.array([row])]
    cols = [rng.choice(free_c, size=599, replace=False), np.full(599, col), np.array([col])]
    for j in free_c:
        rows.append(rng.choice(free_r, size=2, replace=False)); cols.append(np.full(2, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = _csc(m, n, rows, cols, _nonzero_ints(rng, rows.shape[0]))
    x, s, y = rng.integers(1, 6, size=n), rng.integers(1, 6, size=n), rng.integers(-4, 5, size=m)
    b, c = A @ x, A.T @ y + s
    return dict(A=A, x=x, y=y, s=s, b=b, c=c, row=row, col=col, empty_row=empty_row, empty_col=empty_col)


# ------------------------------------------------------------------------------------------------------------------- raw CSC ingest
def ingest_base(m=200, seed=10):
    return banded(m, offsets=(1, 3, 64), seed=seed)


def ingest_pair_positions(A, count=5, seed=11):
    """`count` positions (i, j) outside the pattern of A, in distinct columns."""
    rng = np.random.default_rng(seed)
    A = sparse.csc_matrix(A)
    out = []
    for j in rng.choice(A.shape[1], size=count, replace=False):
        inside = A.indices[A.indptr[j]:A.indptr[j + 1]]
        out.append((int(rng.choice(np.setdiff1d(np.arange(A.shape[0]), inside))), int(j)))
    return out


def raw_csc(A, shuffle=False, split=False, pairs=(), seed=12):
    """(colptr, rowind, val) of A as a C caller may send it: the entries of every column shuffled, every fifth entry sent as two
    halves v / 2 + v / 2 (exact), and for every position of `pairs` the two entries +w and -w."""
    rng = np.random.default_rng(seed)
    A = sparse.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    extra = {}
    for q, (i, j) in enumerate(pairs):
        extra.setdefault(j, []).append((i, 1.5 + q))
    cp, ri, cv = [0], [], []
    seen = 0
    for j in range(A.shape[1]):
        r = list(A.indices[A.indptr[j]:A.indptr[j + 1]])
        v = list(A.data[A.indptr[j]:A.indptr[j + 1]])
        rr, vv = [], []
        for i, a in zip(r, v):
            if split and seen % 5 == 0:
                rr += [i, i]; vv += [a / 2.0, a / 2.0]
            else:
                rr.append(i); vv.append(a)
            seen += 1
        for i, w in extra.get(j, ()):
            rr += [i, i]; vv += [w, -w]
        if shuffle:
            p = rng.permutation(len(rr))
            rr, vv = [rr[t] for t in p], [vv[t] for t in p]
        ri += rr; cv += vv
        cp.append(len(ri))
    return np.asarray(cp, dtype=np.int32), np.asarray(ri, dtype=np.int32), np.asarray(cv, dtype=np.float64)


def with_explicit_zeros(A, positions):
    """A (float64 CSC, sorted) with an explicit 0.0 stored at every position: what the cancelling pairs leave behind."""
    A = sparse.csc_matrix(A, dtype=np.float64)
    cp, ri, cv = raw_csc(A)
    cols = np.repeat(np.arange(A.shape[1]), np.diff(cp))
    rows = np.concatenate([ri, [i for i, _ in positions]]).astype(np.int64)
    cols = np.concatenate([cols, [j for _, j in positions]]).astype(np.int64)
    vals = np.concatenate([cv, np.zeros(len(positions))])
    order = np.lexsort((rows, cols))
    Z = sparse.csc_matrix((vals[order], rows[order], np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))])),
                          shape=A.shape)
    assert Z.nnz == A.nnz + len(positions) and Z.has_sorted_indices
    return Z


def rejected_inputs(A):
    """{name: ((colptr, rowind, val), error code of include/ipm_hip.h)}: the four inputs ipm_set_A_csc must refuse.  The colptr of
    "colptr" steps back in the middle but never points past nnz, so no reader runs off the arrays before it notices."""
    m = A.shape[0]
    out = {}
    for name in ("row_m", "row_minus_1", "colptr", "nan"):
        cp, ri, cv = raw_csc(A)
        j = A.shape[1] // 2
        if name == "row_m":
            ri[cp[j]] = m
        elif name == "row_minus_1":
            ri[cp[j]] = -1
        elif name == "colptr":
            assert cp[j + 1] + 1 <= cp[-1] and cp[j - 1] <= cp[j + 1] + 1
            cp[j] = cp[j + 1] + 1
        else:
            cv[cp[j]] = np.nan
        out[name] = ((cp, ri, cv), -6 if name == "nan" else -1)          # IPM_ERR_INVALID_INPUT / IPM_ERR_INVALID_ARG
    return out
