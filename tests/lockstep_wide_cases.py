"""The cells of tests/test_gpu_lockstep_wide.py: lockstep batches (csrc/lockstep.h) of 66 to 70 LPs, past the 64 LPs one launch
serves (LS_MAX_GROUP), where every GPU test before it put two to six LPs into a batch.  Shared with
tests/test_lockstep_wide_cases_host.py, which asserts without a GPU that every cell is what its name claims.  Test infrastructure
only: a helper module, not a test.

Every LP is IO.sparsify(IO.interior_case(m, n, False, seed), density, seed) handed over as a csc_matrix, with a seed of its own; the
state one solve starts from is the case's (x, y, s).  Shapes vary inside a family on purpose: the grids of the vector kernels
(ceil(max(m, n) / 256) blocks), of the sparse products and of the product-list formation differ from LP to LP, so the `start`
table of a packed launch is not uniform.

FAMILIES -- the smallest block counts at which each group of kernel types enters a handle's launch program.  The rule is
group_size(nblk, ragged = true) of csrc/ipm_api.hip (restated in group_size below; the host test compares it with the library's
through ipm_debug_at_pieces): below 16 blocks, gsz = the largest of 8 / 4 / 2 that divides nblk (8 + leftover for 9 .. 15 blocks
that only 2 or nothing divides), else 0; nG = nblk // gsz groups get explicit inverses (enqueue_group_inverses), gsz = 0 means
block-step substitutions (enqueue_block_steps).

    two     2 blocks (m cycles through 129, 130, 191, 192, 255, 256): gsz = 2, nG = 1.  The program holds the group-inverse
            launches (LS_GROUP_DIAG_T and the three products of the one level 128 -> 256; one pair in one group is batch = batch2 = 1,
            which ls_gemm_hook records as the plain LS_GEMM_32_32_32, not the batched type) and the diagonal LS_GEMV_N of the
            sweeps.  One group has nothing below or left of it: no off-diagonal LS_GEMV_N, no LS_GEMV_T, no LS_SUB_PARTIALS.
    three   3 blocks (m in 257 .. 384): no power of two divides 3, gsz = 0: LS_TRSV_FWD / LS_TRSV_BWD block steps, no group kernel.
    six     6 blocks (m in 641 .. 768): gsz = 2, nG = 3: LS_GROUP_DIAG_T over three groups (96 blocks of the packed (4, 4, 6) grid),
            LS_GEMM_32_32_32_BATCHED with batch = 1, batch2 = 3, the off-diagonal LS_GEMV_N, and LS_GEMV_T + LS_SUB_PARTIALS for the
            two groups with columns left of them.

n = m + 40 + (37 seed mod 311), so m + 40 <= n <= m + 350; every 13th seed of `two` has n = 513 instead, one column past two
blocks of the vector kernels.  Densities (two 5 .. 9 %, three 4 .. 5.5 %, six 2 .. 3 %) keep the product list far below its cap of
2^24 terms, and every family stays at or below 1536 padded rows: the formation is LS_ZERO + LS_ADAT_LIST (host_sparse_setup.h,
want_list).  IPM_LIST_FORM=0 at creation turns that off: cell sparse66 runs LS_ADAT_SPARSE instead.

CELLS -- lists of (family, seed) in batch order.  "two+primal" / "two+dual" are `two` LPs whose (b, c) went through
IO.primal_fire_case / IO.dual_fire_case: with infeasibility_tol = (0.5, 0.5) a test of the infeasibility tests fires at k = 0 (the
plain LPs of detect66 keep the default tolerance 1e-8: at 0.5 a random interior state fires, too).

    two66, three66, six66   66 LPs of one family: every launch of the program is a 64 + 2 split
    mixed66                 44 two, 14 three, 8 six, spread evenly over the batch order: three program lengths out of phase
    detect66                66 `two` LPs for handles with detect_infeasibility=True (types 27, 28): plain, primal, dual by position mod 3
    sparse66                the LPs of two66, for handles created under IPM_LIST_FORM=0
    cross64                 67 `two` LPs with iteration caps 3, 1, 2 by position mod 3: the active count goes 67, 67, 45, 23
    join70                  70 `two` LPs: 60 + 10 (a 64 + 6 split after the join) and 20 + 46 (the record table must grow)
    cap5                    5 `two` LPs for ipm_batch_step with cap = 2

Kernel types a launch of 64 members covers (MI355X run of the GPU file): all but four.  LS_ADAT_SPARSE_GLOBAL needs more than 19456
padded rows; LS_GEMM_64_128_16, LS_GEMM_128_128_16 and LS_CHOL_UPDATE are the panel / update shapes of handles with more blocks
than six (every family here factors with LS_GEMM_32_128_32 panels and LS_GEMM_64_64_16 updates), and 66 copies of such an LP are
too heavy for a test.  The Netlib batches of tests/test_gpu_lockstep.py cover those four at two to six members.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy import sparse

import iteration_oracle as IO

LS_TYPES = ("SPMV_CSR", "SPMV_CSC_T", "PREPARE", "STOP_TEST", "ZERO", "ADAT_LIST", "ADAT_SPARSE", "ADAT_SPARSE_GLOBAL", "MAXDIAG",
            "POTRF", "GEMM_32_128_32", "GEMM_64_64_16", "GEMM_64_128_16", "GEMM_128_128_16", "GEMM_32_32_32", "CHOL_UPDATE", "TRSV_FWD",
            "TRSV_BWD", "DIRECTION", "MU_AFF", "CORR_RHS", "UPDATE", "GEMV_N", "GEMV_T", "SUB_PARTIALS", "GROUP_DIAG_T",
            "GEMM_32_32_32_BATCHED", "PREPARE_DETECT", "STOP_TEST_DETECT")          # enum LsType of csrc/lockstep.h, in order
LS = {nm: k for k, nm in enumerate(LS_TYPES)}
LS_MAX_GROUP = 64                # csrc/lockstep.h
GS_MAX = 8                       # csrc/trsv_grouped.h
LIST_MAX_MP, LIST_MAX_TERMS = 1536, 1 << 24      # host_sparse_setup.h, want_list

TWO_M = (129, 130, 191, 192, 255, 256)
BLOCKS = {"two": 2, "three": 3, "six": 6}
M_RANGE = {"two": (129, 256), "three": (257, 384), "six": (641, 768)}
# family -> (types its program must hold, types it must not hold)
MUST = {"two": ({"ZERO", "ADAT_LIST", "POTRF", "GROUP_DIAG_T", "GEMM_32_32_32", "GEMV_N"},
                {"GEMM_32_32_32_BATCHED", "GEMV_T", "SUB_PARTIALS", "TRSV_FWD", "TRSV_BWD", "ADAT_SPARSE", "ADAT_SPARSE_GLOBAL"}),
        "three": ({"ZERO", "ADAT_LIST", "POTRF", "TRSV_FWD", "TRSV_BWD"},
                  {"GROUP_DIAG_T", "GEMM_32_32_32_BATCHED", "GEMV_T", "SUB_PARTIALS", "ADAT_SPARSE", "ADAT_SPARSE_GLOBAL"}),
        "six": ({"ZERO", "ADAT_LIST", "POTRF", "GROUP_DIAG_T", "GEMM_32_32_32_BATCHED", "GEMV_N", "GEMV_T", "SUB_PARTIALS"},
                {"TRSV_FWD", "TRSV_BWD", "ADAT_SPARSE", "ADAT_SPARSE_GLOBAL"})}
DETECT_TOL = (0.5, 0.5)          # infeasibility_tol of the detect66 handles: what IO.primal_fire_case / dual_fire_case are built for


def group_size(nblk, ragged=True):
    """group_size of csrc/ipm_api.hip."""
    gsz = 0
    if nblk >= 2 * GS_MAX:
        if ragged or nblk % GS_MAX == 0:
            gsz = GS_MAX
    else:
        for p2 in (8, 4, 2):
            if nblk % p2 == 0:
                gsz = p2
                break
        if ragged and nblk > GS_MAX and gsz < 4:
            gsz = GS_MAX
    return gsz


def groups(family):
    """(gsz, nG) the family's handles must report."""
    nblk = BLOCKS[family]
    gsz = group_size(nblk)
    return gsz, (nblk // gsz if gsz else 0)


def base(family):
    return family.split("+")[0]


def shape(family, seed):
    """(m, n, density) of the family's LP of that seed."""
    fam = base(family)
    if fam == "two":
        m = TWO_M[seed % 6]
        density = 0.05 + 0.01 * (seed % 5)
    else:
        lo, hi = M_RANGE[fam]
        m = hi if seed % 8 == 7 else lo + (53 * seed) % 128
        density = 0.04 + 0.005 * (seed % 4) if fam == "three" else 0.02 + 0.005 * (seed % 3)
    n = m + 40 + (37 * seed) % 311
    if fam == "two" and seed % 13 == 6:
        n = 513
    return m, n, density


class WideLP:
    """One LP of a cell: A (csc_matrix), b, c and the state (x, y, s) a solve starts from."""

    def __init__(self, family, seed, case):
        self.family, self.seed = family, seed
        self.A = sparse.csc_matrix(case.A)
        self.b, self.c = case.b, case.c
        self.x, self.y, self.s = case.x, case.y, case.s
        self.m, self.n = case.m, case.n

    def state(self):
        return self.x, self.y, self.s


@functools.lru_cache(maxsize=None)
def case(family, seed):
    """The iteration_oracle.Case (dense A: keep only the few the oracle needs)."""
    m, n, density = shape(family, seed)
    out = IO.sparsify(IO.interior_case(m, n, False, seed), density, seed)
    if family.endswith("+primal"):
        out = IO.primal_fire_case(out)
    elif family.endswith("+dual"):
        out = IO.dual_fire_case(out)
    return out


case_uncached = case.__wrapped__


@functools.lru_cache(maxsize=None)
def lp(family, seed):
    """The WideLP, built once per process (the dense Case behind it is dropped unless case() holds it).  Treat it as read-only."""
    return WideLP(family, seed, case_uncached(family, seed))


def _spread(counts):
    """Families spread evenly over the batch order: member i of a family of c sits at (i + 1/2) / c of the way."""
    keys = sorted(((i + 0.5) / c, fam, i) for fam, c in counts for i in range(c))
    return [(fam, i) for _, fam, i in keys]


MIXED = (("two", 44), ("three", 14), ("six", 8))
CELLS = {
    "two66": [("two", s) for s in range(66)],
    "three66": [("three", s) for s in range(66)],
    "six66": [("six", s) for s in range(66)],
    "mixed66": _spread(MIXED),
    "detect66": [(("two", "two+primal", "two+dual")[s % 3], s) for s in range(66)],
    "sparse66": [("two", s) for s in range(66)],
    "cross64": [("two", s) for s in range(67)],
    "join70": [("two", s) for s in range(70)],
    "cap5": [("two", s) for s in range(5)],
}
ORACLE_POSITIONS = (0, 32, 63, 64)          # of two66: lane 0, the first lane of the upper half-wave, the last lane, the first LP of the split-off launch
CROSS_CAPS = (3, 1, 2)                      # cross64: iteration cap by position mod 3 -> 22 LPs leave first, then 22, then 23
JOINS = ((60, 10), (20, 46))                # join70: (LPs at the start, LPs added after the first step)


def cell(name):
    return [lp(fam, seed) for fam, seed in CELLS[name]]


def cross_cap(position):
    return CROSS_CAPS[position % 3]


def template(nb, substitution, detect=False):
    """A launch program of the shape of one iteration (type numbers), for the merge alone: residuals, list formation, nb x {potrf,
    panel, update}, then sweeps by `substitution` ("group" / "block") and the vector kernels."""
    pre = [LS["SPMV_CSR"], LS["SPMV_CSC_T"], LS["PREPARE_DETECT" if detect else "PREPARE"], LS["STOP_TEST_DETECT" if detect else "STOP_TEST"],
           LS["ZERO"], LS["ADAT_LIST"], LS["MAXDIAG"]]
    chol = []
    for k in range(nb):
        chol += [LS["POTRF"]] if k == nb - 1 else [LS["POTRF"], LS["GEMM_32_128_32"], LS["CHOL_UPDATE"]]
    if substitution == "group":
        inv = [LS["GROUP_DIAG_T"]] + 3 * [LS["GEMM_32_32_32_BATCHED"]]
        sweep = [LS["GEMV_N"]] * (nb - 1) + [LS["GEMV_N"]] + [LS["GEMV_T"], LS["SUB_PARTIALS"]] * (nb // 2 - 1)
    else:
        inv = []
        sweep = [LS["TRSV_FWD"]] * nb + [LS["TRSV_BWD"]] * nb
    solve = sweep + [LS["SPMV_CSC_T"], LS["DIRECTION"]]
    return pre + chol + inv + solve + [LS["MU_AFF"], LS["CORR_RHS"]] + solve + [LS["UPDATE"]]
