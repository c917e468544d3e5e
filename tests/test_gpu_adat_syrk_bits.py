"""GPU test (-m gpu): adat_syrk_kernel (csrc/adat_syrk_f64.h), the dense formation B = A diag(d) A^T, pinned bit for bit.
tests/golden/adat_syrk_digests.json holds sha256 of IpmSolver.form_normal_matrix(d) for dense A from a seeded generator,
recorded on an MI355X with the build in which the kernel still carried its own copy of the stage loop (the commit before
csrc/mfma_stage_pipe.h).  A change to the stage schedule must not change a bit: the MFMA sequence of every accumulator stays.

Cases: what the stage loop can get wrong at its edges, as far as the handle's layout reaches them.  A handle pads n to a
multiple of 64 (make_layout, csrc/host_handle.h), so a launch has K/16 = 4, 8, 12, ... stages: one, two or three stages
cannot be reached through the API.  The shortest loop that can (4 stages), 8 and 12, n no multiple of 64, on one tile
(m = 128) and on six tiles with off-diagonal ones (m = 384); and split-K: with 36 stages the launch rule cuts K into four
chunks of 9, so chunks begin at stages 9 and 27 (the prologue fills the SECOND LDS buffer) and run an odd number of
stages (buffer parity at exit).  launch_path restates the launch rule and the test asserts the path each case names."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                              # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adat_syrk_digests.json")

# name -> (m, n, stages K/16, chunk begins)
CASES = {
    "128x61": (128, 61, 4, [0]),
    "128x100": (128, 100, 8, [0]),
    "128x190": (128, 190, 12, [0]),
    "384x61": (384, 61, 4, [0]),
    "384x100": (384, 100, 8, [0]),
    "384x190": (384, 190, 12, [0]),
    "128x570_splitk": (128, 570, 36, [0, 9, 18, 27]),
    "384x570_splitk": (384, 570, 36, [0, 9, 18, 27]),
}


def launch_path(m, n, slots=512):
    """(stages, chunk begins) of launch_adat_syrk for an m x n handle: make_layout's padding, then the split-K rule of the
    tiles beyond a multiple of `slots` (all of them here)."""
    mp, npad = -(-m // 128) * 128, -(-n // 64) * 64
    nt = mp // 128
    assert nt < 16                                  # (from 16 blocks on make_layout may pad the rows further)
    tiles, nk = nt * (nt + 1) // 2, npad // 16
    tail = tiles % slots
    if tail > 0 and nk >= 16:
        p = min(slots // tail, nk // 8)
        if p >= 2:
            per = -(-nk // p)
            return nk, list(range(0, nk, per))
    return nk, [0]


def normal_matrix(m, n):
    rng = np.random.default_rng(1000 * m + n)
    A = rng.standard_normal((m, n))
    d = 10.0 ** rng.uniform(-3, 3, n)
    with ipm.IpmSolver(A, np.zeros(m), np.zeros(n)) as sv:
        B = sv.form_normal_matrix(d)
    return A, d, B


def digest(B):
    return hashlib.sha256(np.ascontiguousarray(B, dtype=np.float64).tobytes()).hexdigest()


@pytest.mark.parametrize("case", sorted(CASES))
def test_formation_bits_are_the_recorded_ones(case):
    m, n, nk, begins = CASES[case]
    assert launch_path(m, n) == (nk, begins)
    if len(begins) > 1:
        assert any(b & 1 for b in begins) and (begins[1] - begins[0]) & 1
    with open(GOLDEN) as fh:
        want = json.load(fh)["digests"][case]
    A, d, B = normal_matrix(m, n)
    ref = (A * d) @ A.T
    assert float(np.max(np.abs(B - ref))) <= 1e-13 * float(np.max(np.abs(ref)))       # (a wrong fixture would not hide a wrong B)
    assert digest(B) == want
