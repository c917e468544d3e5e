"""Constructed inputs for the multifrontal sparse Cholesky (csrc/sparse_chol.h, sparse_symbolic.h, host_sparse_setup.h), their
longdouble reference and the derived error bounds, shared by tests/test_sparse_cases_host.py and
tests/test_gpu_sparse_structures.py.  Test infrastructure only: a helper module, not a test.  No data files.

PATTERNS.  A pattern is a list of cliques on the rows, and A = [ I | one column per clique ]: the unit columns keep
B = A diag(d) A^T positive definite and the pattern of B is exactly the union of the cliques.  From Python an LP of at most 128
rows never builds a sparse factor (analysis._factor_path), so every case is padded to at least 130 rows with isolated rows, which
are also the forest edge (roots with r = w = 1).

VALUES.  Clique entries +-U(0.5, 2); d = 10^U(-D, D) with D = 0.3 and D = 6 (condition numbers of B up to 6e13 without a guarded
pivot).

REFERENCE, all np.longdouble: B formed clique by clique from A and d, permuted by the device's row order, factored with
iteration_oracle.cholesky; guarded_cholesky takes the device's eps, big and shift.

BOUNDS, derived (not measured).  u = 2^-53, k = m + 2 + the most nonzeros in a row of A, Lh = the reference factor.
    (F)  |L L^T - B_p|_ij <= k u sqrt(B_ii B_jj)                for every i, j            (Higham, Accuracy and Stability, Thm 10.3
         with (|L||L^T|)_ij <= sqrt(b_ii b_jj), plus the rounding of the formation); outside the symbolic structure L is exactly 0
    (S)  |B z - rhs|_i <= (3k+1) u (|Lh||Lh^T||z|)_i + k u (|A| diag(d) |A^T| |z|)_i + u |rhs_i|      (Thm 10.4 plus the formation)
check_factor / check_solve return the largest ratio of an error to its bound: a test asserts ratio <= 1.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
from scipy import sparse

import iteration_oracle as IO
from oracle import sparse_chol as SO

LD = np.longdouble
U = 2.0 ** -53
MIN_ROWS = 130           # analysis.FUSED_SMALL_MAX_ROWS + 2: the smallest LP that builds a sparse factor from Python
WCAP, PANEL, FRONT = 32, 7680, 4096      # SPC_WCAP, SPC_PANEL, SPC_FRONT of csrc/sparse_chol.h
NT, BATCH = 256, 8                       # SPC_THREADS, SPC_BATCH
DS = (0.3, 6.0)


# ---------------------------------------------------------------------------------------------------------------------------
# patterns: name -> (rows before padding, list of cliques)
# ---------------------------------------------------------------------------------------------------------------------------
def _clique(*sizes):
    out, at = [], 0
    for s in sizes:
        out.append(np.arange(at, at + s))
        at += s
    return at, out


def _star(leaves):
    """Rows 0 .. leaves - 1 each adjacent to the root only.  The root is the LAST row of the star: minimum degree breaks the final tie
    (root against last leaf, both of degree 1) to the lowest index, so the root is eliminated last and keeps leaves - 1 children
    (the last leaf is amalgamated into its panel)."""
    return leaves + 1, [np.array([i, leaves]) for i in range(leaves)]


def _cstar(root, leaf, leaves):
    """A root clique; `leaves` cliques of `leaf` new rows each, every one attached to the whole root."""
    core = np.arange(root)
    cl = [core]
    for t in range(leaves):
        cl.append(np.concatenate([core, root + t * leaf + np.arange(leaf)]))
    return root + leaf * leaves, cl


def _bigborder(core, border):
    """A clique of `core` rows plus `border` rows each adjacent to all of it (and to no other border row)."""
    c = np.arange(core)
    return core + border, [c] + [np.concatenate([c, [core + t]]) for t in range(border)]


def _path(m):
    return m, [np.array([i, i + 1]) for i in range(m - 1)]


def _nested_dissection(depth, sep):
    """Complete binary separator tree with `depth` levels of `sep` rows per node (heap numbering); each leaf of the tree forms a
    clique with all its ancestors."""
    nodes = 2 ** depth - 1
    cl = []
    for leaf in range(2 ** (depth - 1) - 1, nodes):
        chain, v = [], leaf
        while True:
            chain.append(v)
            if v == 0:
                break
            v = (v - 1) // 2
        cl.append(np.sort(np.concatenate([v * sep + np.arange(sep) for v in chain])))
    return nodes * sep, cl


RANDOM400_SEED = 21      # two stars wide enough for fan-in nodes, both in panel mode (r = 82 and r = 91)


def _random400():
    R = sparse.random(400, 900, 0.004, random_state=np.random.RandomState(RANDOM400_SEED), format="csc")
    cl = [np.sort(R.indices[R.indptr[j]:R.indptr[j + 1]]) for j in range(900)]
    return 400, [c for c in cl if c.size >= 2]


PATTERNS = {
    "clique64": lambda: _clique(64),
    "clique65": lambda: _clique(65),
    "clique240_87_88": lambda: _clique(240, 87, 88),
    "clique241": lambda: _clique(241),
    "star13": lambda: _star(13),
    "star14": lambda: _star(14),
    "star65": lambda: _star(65),
    "star97": lambda: _star(97),
    "star106": lambda: _star(106),
    "cstar_40_3_14": lambda: _cstar(40, 3, 14),
    "cstar_70_2_30": lambda: _cstar(70, 2, 30),
    "bigborder_300_20": lambda: _bigborder(300, 20),
    "path300": lambda: _path(300),
    "nd_4_20": lambda: _nested_dissection(4, 20),
    "random400": _random400,
}
NAMES = tuple(PATTERNS)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def matrix(name):
    """A = [ I | one column per clique ] as CSC, m >= MIN_ROWS.  Treat as read-only."""
    if name in GUARD_CASES:
        return _guard_matrix(name)
    m0, cliques = PATTERNS[name]()
    m = max(m0, MIN_ROWS)
    rng = np.random.default_rng(_seed("A", name))
    rows, cols, vals = [np.arange(m)], [np.arange(m)], [np.ones(m)]
    for t, c in enumerate(cliques):
        rows.append(np.asarray(c))
        cols.append(np.full(len(c), m + t))
        vals.append(rng.uniform(0.5, 2.0, len(c)) * rng.choice([-1.0, 1.0], len(c)))
    A = sparse.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m, m + len(cliques)))
    A.sort_indices()
    return A


def dvec(name, D):
    rng = np.random.default_rng(_seed("d", name, D))
    return 10.0 ** rng.uniform(-D, D, matrix(name).shape[1])


def rhs(name):
    return np.random.default_rng(_seed("rhs", name)).standard_normal(matrix(name).shape[0])


# ---------------------------------------------------------------------------------------------------------------------------
# the panel tree of a case and the regimes of sp_chol_kernel its nodes fall into
# ---------------------------------------------------------------------------------------------------------------------------
class Tree:
    """Panel table of oracle.sparse_chol.panel_table plus what the kernels derive from it.  Per node: c0, w, r, p = r - w, nchild,
    parent, front (whole front in LDS: r * r <= lds), ksteps (MFMA k-steps of the panel-mode update), level (1 = leaf)."""

    def __init__(self, A):
        t = SO.panel_table(A)
        self.perm, self.rows = t["perm"], t["rows"]
        self.c0, self.w, self.r, self.nchild, self.parent = t["c0"], t["w"], t["r"], t["nchild"], t["parent"]
        self.p = self.r - self.w
        self.nsn = len(self.w)
        self.rmax = int(self.r.max())
        self.panel_max = int((self.r * self.w).max())
        # host_sparse_setup.h: sp_lds_doubles = max(16, panel_max, min(rmax^2, SPC_FRONT))
        self.lds = max(16, self.panel_max, min(self.rmax * self.rmax, FRONT))
        self.front = self.r * self.r <= self.lds
        self.ksteps = (self.w + 3) // 4
        self.level = np.ones(self.nsn, dtype=np.int64)
        for J in range(self.nsn):
            if self.parent[J] >= 0:
                assert self.parent[J] > J
                self.level[self.parent[J]] = max(self.level[self.parent[J]], self.level[J] + 1)
        self.height = int(self.level.max())
        self.fan_in = self.w == 0
        self.pos = np.empty_like(self.perm)           # pos[caller's row] = device row
        self.pos[self.perm] = np.arange(len(self.perm))

    def mfma(self):
        """Nodes whose update runs on the matrix cores: panel mode with columns and rows below."""
        return (~self.front) & (self.w > 0) & (self.p > 0)

    def cells(self):
        """{(w, r, nchild, 'front' | 'panel')} over the nodes."""
        return {(int(w), int(r), int(c), "front" if f else "panel") for w, r, c, f in zip(self.w, self.r, self.nchild, self.front)}

    def has(self, w, r, nchild=None, mode=None):
        return any(cw == w and cr == r and (nchild is None or cc == nchild) and (mode is None or cm == mode)
                   for cw, cr, cc, cm in self.cells())

    def panel_of(self, col):
        """The node (w > 0) that owns device column `col`."""
        J = np.flatnonzero((self.w > 0) & (self.c0 <= col) & (col < self.c0 + self.w))
        assert J.size == 1
        return int(J[0])

    def structure(self):
        """Boolean m x m mask of the entries of L the panels store (device order, lower triangle)."""
        m = len(self.perm)
        S = np.zeros((m, m), dtype=bool)
        for J in range(self.nsn):
            for b in range(int(self.w[J])):
                S[self.rows[J][b:], self.c0[J] + b] = True
        return S

    def tasks(self):
        """The task partition of host_sparse_setup.h::build_sparse_factor restated -> (task of every node, number of tasks)."""
        nsn = self.nsn
        sub = np.zeros(nsn)
        total = 0.0
        for J in range(nsn):
            cst = 1.0 + float(self.r[J]) * float(self.r[J]) / 1024.0 + 0.5 * float(self.nchild[J])
            sub[J] += cst
            total += cst
            if self.parent[J] >= 0:
                sub[self.parent[J]] += sub[J]
        T = max(8.0, total / 1536.0)
        topkids = np.zeros(nsn, dtype=np.int64)
        for J in range(nsn):
            if sub[J] > T and self.parent[J] >= 0:
                topkids[self.parent[J]] += 1
        taskof = np.full(nsn, -1, dtype=np.int64)
        ntask = 0
        for J in range(nsn - 1, -1, -1):
            pj = int(self.parent[J])
            if not sub[J] > T:
                join = pj >= 0 and not sub[pj] > T
            else:
                join = pj >= 0 and topkids[pj] == 1
            if join:
                taskof[J] = taskof[pj]
            else:
                taskof[J] = ntask
                ntask += 1
        return ntask - 1 - taskof, ntask


@functools.lru_cache(maxsize=None)
def tree(name):
    return Tree(matrix(name))


# ---------------------------------------------------------------------------------------------------------------------------
# longdouble reference and the bounds
# ---------------------------------------------------------------------------------------------------------------------------
def normal_matrix(A, d, absolute=False):
    """A diag(d) A^T (or |A| diag(d) |A^T|) in longdouble, column by column of A: exactly the union of the cliques."""
    A = sparse.csc_matrix(A)
    m, n = A.shape
    B = np.zeros((m, m), dtype=LD)
    for j in range(n):
        lo, hi = A.indptr[j], A.indptr[j + 1]
        if hi == lo:
            continue
        idx = A.indices[lo:hi]
        a = A.data[lo:hi].astype(LD)
        if absolute:
            a = np.abs(a)
        B[np.ix_(idx, idx)] += LD(d[j]) * np.outer(a, a)
    return B


def guarded_cholesky(B, eps, big, shift_rel=0.0):
    """Left-looking longdouble Cholesky of B + shift I with the device's guard: thresh = eps max diag(B), shift = shift_rel max
    diag(B); a pivot that is not above thresh is replaced by big -> (L, guarded positions, pivots before the guard)."""
    m = B.shape[0]
    md = B.diagonal().max()
    thresh, shift = LD(eps) * md, LD(shift_rel) * md
    L = np.zeros((m, m), dtype=LD)
    fixed, piv = [], np.zeros(m, dtype=LD)
    for j in range(m):
        v = B[j:, j] - L[j:, :j] @ L[j, :j]
        v0 = v[0] + shift
        piv[j] = v0
        if not v0 > thresh:
            v0 = LD(big)
            fixed.append(j)
        L[j, j] = np.sqrt(v0)
        L[j + 1:, j] = v[1:] / L[j, j]
    return L, np.array(fixed, dtype=np.int64), piv


class Reference:
    """Everything the bounds need for one (case, D, shift), in longdouble.  B and absB in the caller's row order; Bp (shift included)
    and Lh in the device's."""

    def __init__(self, name, D, shift_rel=0.0, drop=()):
        A = matrix(name)
        self.name, self.D = name, D
        self.A, self.d, self.rhs = A, dvec(name, D), rhs(name)
        self.tree = tree(name)
        self.perm = self.tree.perm
        m = A.shape[0]
        self.m = m
        self.k = m + 2 + int(np.diff(sparse.csr_matrix(A).indptr).max())
        self.B0 = normal_matrix(A, self.d)
        self.maxdiag = self.B0.diagonal().max()
        self.shift = LD(shift_rel) * self.maxdiag
        self.B = self.B0 + self.shift * np.eye(m, dtype=LD)
        self.absB = normal_matrix(A, self.d, absolute=True) + self.shift * np.eye(m, dtype=LD)
        self.Bp = self.B[np.ix_(self.perm, self.perm)]
        # rows (device order) left out of every comparison: the guarded ones of a guard case
        self.drop = np.array(sorted(drop), dtype=np.int64)
        self.keep = np.setdiff1d(np.arange(m), self.drop)
        self.Lh = IO.cholesky(self.Bp[np.ix_(self.keep, self.keep)])

    def factor_bound(self):
        dg = self.Bp.diagonal()[self.keep]
        return LD(self.k * U) * np.sqrt(np.outer(dg, dg))


@functools.lru_cache(maxsize=None)
def reference(name, D, shift_rel=0.0):
    return Reference(name, D, shift_rel)


def check_factor(L, ref):
    """(F) on a float64 factor in device order -> the largest |L L^T - B_p|_ij / bound_ij (over the kept rows)."""
    Lk = np.asarray(L, dtype=np.float64)[np.ix_(ref.keep, ref.keep)].astype(LD)
    R = IO._normal_matrix(Lk, np.ones(Lk.shape[0], dtype=LD)) - ref.Bp[np.ix_(ref.keep, ref.keep)]
    return float((np.abs(R) / ref.factor_bound()).max())


def shift_ratio(L, ref):
    """(c): the largest |diag(L L^T - B0_p) - shift| / (F)'s diagonal bound."""
    Ll = np.asarray(L, dtype=np.float64).astype(LD)
    dg = (Ll * Ll).sum(axis=1) - ref.B0.diagonal()[ref.perm]
    return float((np.abs(dg - ref.shift) / (LD(ref.k * U) * ref.Bp.diagonal())).max())


def outside_structure(L, ref):
    """Number of nonzero entries of L outside the panels' structure (upper triangle included)."""
    return int(np.count_nonzero(np.asarray(L)[~ref.tree.structure()]))


def check_solve(z, ref):
    """(S) on a float64 solution in the caller's row order -> the largest |B z - rhs|_i / bound_i (over the kept rows)."""
    perm = ref.perm
    zp = np.asarray(z, dtype=np.float64).ravel().astype(LD)[perm]            # device order
    keep = ref.keep
    zk = zp[keep]
    rp = ref.rhs.astype(LD)[perm][keep]
    res = np.abs(ref.Bp[np.ix_(keep, keep)] @ zk - rp)
    absL = np.abs(ref.Lh)
    absBp = ref.absB[np.ix_(perm, perm)][np.ix_(keep, keep)]
    bound = LD((3 * ref.k + 1) * U) * (absL @ (absL.T @ np.abs(zk))) + LD(ref.k * U) * (absBp @ np.abs(zk)) + LD(U) * np.abs(rp)
    return float((res / bound).max())


# ---------------------------------------------------------------------------------------------------------------------------
# guard cases: one row of a clique copied onto another row of the same clique (the copy's own unit column becomes empty), so that
# B has two equal rows and the later of the two in device order meets a pivot that is zero to rounding.  The pairs were chosen by
# a search on the CPU for the place of that column in the panel tree; tests/test_sparse_cases_host.py asserts the place.
# name -> (base case, source row, row overwritten, what the guarded column is)
# ---------------------------------------------------------------------------------------------------------------------------
GUARD_EPS, GUARD_BIG, GUARD_D = 1e-10, 1e64, 0.3
GUARD_CASES = {
    "guard_panel_first": ("bigborder_300_20", 97, 145, dict(first=True, mode="panel", w=32, r=156)),
    "guard_panel_last32": ("bigborder_300_20", 79, 112, dict(last32=True, mode="panel", w=32, r=220)),
    "guard_panel_inside": ("clique65", 1, 4, dict(first=False, last32=False, mode="panel", w=32, r=65)),
    "guard_front_inside": ("clique240_87_88", 247, 244, dict(first=False, last32=False, mode="front", root=False, w=32, r=87)),
    "guard_root": ("nd_4_20", 6, 270, dict(root=True, mode="front", w=17, r=17)),
    "guard_p277": ("bigborder_300_20", 3, 10, dict(mode="panel", p=277, w=25, r=302)),
}


def _guard_matrix(name):
    base, src, dst, _ = GUARD_CASES[name]
    A = sparse.lil_matrix(matrix(base))
    A[dst, :] = A[src, :]
    A = sparse.csc_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return A


class Guard:
    """Reference of a guard case: the guarded set of the longdouble factorization with the device's eps and big, its pivots, and the
    Reference of the system without the guarded rows and columns."""

    def __init__(self, name):
        self.name = name
        A = matrix(name)
        d = dvec(name, GUARD_D)
        t = tree(name)
        B = normal_matrix(A, d)
        Bp = B[np.ix_(t.perm, t.perm)]
        self.thresh = LD(GUARD_EPS) * B.diagonal().max()
        _, self.guarded, self.pivots = guarded_cholesky(Bp, GUARD_EPS, GUARD_BIG)
        self.diag = Bp.diagonal()
        self.ref = Reference(name, GUARD_D, drop=tuple(int(g) for g in self.guarded))


@functools.lru_cache(maxsize=None)
def guard(name):
    return Guard(name)


def guard_place(name):
    """Where the guarded column of a guard case sits: dict(first, last32, mode, root, p) of its panel."""
    base, src, dst, _ = GUARD_CASES[name]
    t = tree(name)
    col = int(max(t.pos[src], t.pos[dst]))
    J = t.panel_of(col)
    return dict(col=col, node=J, first=bool(col == t.c0[J]), last32=bool(t.w[J] == 32 and col == t.c0[J] + 31),
                mode="front" if t.front[J] else "panel", root=bool(t.parent[J] < 0), p=int(t.p[J]), w=int(t.w[J]), r=int(t.r[J]))


# ---------------------------------------------------------------------------------------------------------------------------
# one interior-point iteration on the A of a case (tests/iteration_oracle.Case)
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def iteration_case(name, bounded):
    """As iteration_oracle.interior_case, on the case's A: x, s, w, z ~ U(0.5, 2), y ~ N(0, 1), half the columns bounded with
    u = x + w +- U(0, 0.3), b = A U(0.5, 2), c ~ N(0, 1)."""
    A = matrix(name).toarray()
    m, n = A.shape
    rng = np.random.default_rng(_seed("iter", name, bounded))
    x, s = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    y = rng.standard_normal(m)
    xb = rng.uniform(0.5, 2.0, n)
    c = rng.standard_normal(n)
    u, w, z = np.full(n, np.inf), np.zeros(n), np.zeros(n)
    if bounded:
        cols = np.sort(rng.permutation(n)[: max(1, n // 2)])
        w[cols] = rng.uniform(0.5, 2.0, cols.size)
        z[cols] = rng.uniform(0.5, 2.0, cols.size)
        u[cols] = x[cols] + w[cols] + rng.uniform(-0.3, 0.3, cols.size)
    return IO.Case(A=A, b=A @ xb, c=c, u=u, x=x, y=y, s=s, w=w, z=z, xb=xb, c_dual=False)
