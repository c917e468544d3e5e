"""The cases of tests/test_gpu_late_large.py: one iteration against the oracle ABOVE eight 128-row blocks, where the dense path runs code
that no smaller shape reaches.  Shared with tests/test_late_large_cases_host.py (CPU).  Test infrastructure only: a helper module, not
a test.

Everything is tests/late_cases.py's: the builder late_case for the near-optimal states, evaluate_case (the oracle by
RefinementSolver, the float64 host restatement in three column orders, H, the spread, the dropped cells), the floors, MARGIN and
STABLE.  Nothing is redefined here.  The benign states are iteration_oracle.interior_case's, given a partition of all LOWER and
mu_target = 1 so that late_cases.permute carries them.  A is Gaussian, except in the dualdeg cases (DUALDEG_DENSITY below).

    case                                                        blocks  what only this shape reaches
    A 1100 x 1500: benign b; dualdeg 1e-8 b; dualdeg 1e-6       9       one group of 8 plus one leftover block step; forced two-level groups
    B 1536 x 2000 b dualdeg 1e-6                                12      three groups of 4: the cross-group partials at the smallest size
    C 2048 x 2300: benign; dualdeg 1e-8 b                       16      two 1024-row groups; fused by default (n <= 6 m), its last-group
                                                                        hand-off; streamed A^T pieces
    D 2200 x 2500: benign b; dualdeg 1e-8 b; dualdeg 1e-8       18      24 real rows in the last block; two groups plus two leftover steps;
                                                                        CS_WIDE at step 0 without look-ahead
    E late_cases.D300 and D1000 (evaluated there)               3, 8    the fused launch forced below its default size
    L CSC 1100 x 1500 dualdeg 1e-8, 5 % dense                   9       the lockstep twin of A: grouped sweeps + a leftover step, recorded
(b: half the columns bounded.)

Every near-optimal case is of the dualdeg family, because the host file holds every such case to one condition: the wrong rule
theta = x / (s + 1e-14) must push a cell over its bound, or the case is replaced.  A nondeg case (B, mu = 1e-6) and two primdeg cases
(A and D without bounds, mu = 1e-3) stood here first and could not meet it at any seed or density (largest error / bound 0.05 ..
0.16): with |B| <= m the direction does not depend on theta of the basic columns to first order.  Their shapes, mu (B) and
plain columns (A, D) are kept by the dualdeg cases that replaced them.
"""
from __future__ import annotations

import functools

import numpy as np

import iteration_oracle as IO
import late_cases as LC
from lockstep_wide_cases import group_size          # ipm_api.hip: group_size, restated there and held to the library's

SEED = LC.SEED
# name -> seed, where tests/test_late_large_cases_host.py forces another than SEED (late_cases.SEEDS' form).  B: with seed 3 the wrong
# theta exceeded its best cell by 2.7 x only, one step length; with seed 5 two independent cells by more than 30 x.
SEEDS = {"dense/1536x2000b/dualdeg/1e-06": 5}
BENIGN = "benign"
# The dualdeg cases have a sparse_pattern A of this density under the DENSE ingest (the dense kernels do not see the zeros).  With a
# Gaussian A their basis has a condition number near 1e4, H of the directions is 1e-6, and the wrong rule x / (s + 1e-14) stayed below
# every bound (largest error / bound 0.08, 0.26 and 0.2 at A, C, D): the host file's "the bounds mean something" asked for the
# replacement.  At 2 % it exceeds two independent cells of each (alpha_d 7 .. 11 x its bound, a second step length or sigma 2.2 .. 2.4 x).
DUALDEG_DENSITY = 0.02
SHAPES = {"A": (1100, 1500), "B": (1536, 2000), "C": (2048, 2300), "D": (2200, 2500)}
BLOCKS = {"A": 9, "B": 12, "C": 16, "D": 18}
LOCK_DENSITY = 0.05


def _name(letter, bounded, family, mu, kind="dense"):
    return LC.name_of(kind, *SHAPES[letter], bounded, family, mu)


A_BENIGN, A_DUAL, A_PLAIN = _name("A", True, BENIGN, 1.0), _name("A", True, "dualdeg", 1e-8), _name("A", False, "dualdeg", 1e-6)
B_DUAL = _name("B", True, "dualdeg", 1e-6)
C_BENIGN, C_DUAL = _name("C", False, BENIGN, 1.0), _name("C", True, "dualdeg", 1e-8)
D_BENIGN, D_DUAL, D_PLAIN = _name("D", True, BENIGN, 1.0), _name("D", True, "dualdeg", 1e-8), _name("D", False, "dualdeg", 1e-8)
LOCK_A = _name("A", False, "dualdeg", 1e-8, kind="lock")

LETTER = {A_BENIGN: "A", A_DUAL: "A", A_PLAIN: "A", B_DUAL: "B", C_BENIGN: "C", C_DUAL: "C", D_BENIGN: "D", D_DUAL: "D", D_PLAIN: "D"}
DENSE = list(LETTER)                                            # the cells A - D, in the order the GPU file runs them
NAMES = DENSE + [LOCK_A]
LATE = [nm for nm in NAMES if BENIGN not in nm]
E_CASES = LC.D300 + LC.D1000


def benign_case(m, n, bounded, seed):
    case = IO.interior_case(m, n, bounded, seed)
    case.part, case.mu_target = np.full(n, LC.LOWER), 1.0
    return case


def is_benign(name):
    return name.split("/")[2] == BENIGN


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name (late_cases.get for the cases of E), built once per process.  Read-only."""
    if name in LC.CASES:
        return LC.get(name)
    kind, shape, family, mu = name.split("/")
    bounded = shape.endswith("b")
    m, n = (int(v) for v in shape.rstrip("b").split("x"))
    seed = SEEDS.get(name, SEED)
    if family == BENIGN:
        return benign_case(m, n, bounded, seed)
    density = LOCK_DENSITY if kind == "lock" else DUALDEG_DENSITY if family == "dualdeg" else None
    return LC.late_case(m, n, float(mu), m + LC.FAMILIES[family][0], bounded, seed, density=density)


@functools.lru_cache(maxsize=None)
def evaluate(name):
    """late_cases.evaluate_case of the case, once per process (late_cases.evaluate for the cases of E).  Read-only."""
    return LC.evaluate(name) if name in LC.CASES else LC.evaluate_case(get(name))


def bound(name):
    return LC.bound_of(evaluate(name))


# ---------------------------------------------------------------------------------------------------------------------------
# the dense path's own rules, restated (tests/test_late_large_cases_host.py compares the table above with them, the GPU file
# compares them with schedule()).  group_size(nblk, ragged): blocks per explicit group inverse, 0: block steps throughout.
# ---------------------------------------------------------------------------------------------------------------------------
def groups_and_leftover(nblk, ragged=True):
    """(full groups, blocks left to block steps at the end) under group_size."""
    gsz = group_size(nblk, ragged)
    return (nblk // gsz, nblk % gsz) if gsz else (0, nblk)


def blocks_of(m):
    return (m + 127) // 128


def fused_by_default(m, n):
    """host_fused.h: ff_ok's size rule for a dense handle alone on its device: 16 .. 72 blocks, n <= 6 m (both padded: to 128 rows, the
    columns to what the handle reports; at the shapes here the padding decides nothing)."""
    return 16 <= blocks_of(m) <= 72 and n <= 6 * m
