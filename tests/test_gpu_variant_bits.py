"""GPU test (-m gpu): every problem class on every launch path computes, bit for bit, what the commit before the class-variant tables
computed (csrc/vector_ops.h X_VARIANTS, csrc/small_lp.h SMALL_ROWS; host_residuals.h).  The cells and their data are
tests/variant_bits_cases.py; the fixture tests/golden/variant_bits_parent.json was recorded from a build of that parent commit by
tools/record_variant_bits.py.  A row that drops or adds B, Q or F launches a kernel that ignores a term or reads another argument
group: the iterate differs from the first iteration on, and its digest with it.  The cells are feasible, so the tests of a D class
never fire and a D cell has the digest of its sibling without D: a D row that named the non-detecting kernel would pass here; those
rows are held by tests/test_step_dispatch_host.py and by the detection suites.

Like the ISA fixture test, this one compares the output of one compiler: it skips when hipcc is another one than the fixture's."""
import json
import os
import shutil
import subprocess

import pytest

import interiorpointmethod_amd as ipm
import variant_bits_cases as V

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variant_bits_parent.json")
PATHS = ("dense", "small", "batch", "lockstep", "large", "start")


@pytest.fixture(scope="module")
def parent():
    ref = json.load(open(FIXTURE))
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("hipcc is not available")
    if ref["compiler"] not in subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout:
        pytest.skip("the fixture was recorded with %r; this compiler is another one" % ref["compiler"])
    assert ref["seed"] == V.SEED
    return ref["cells"]


def test_the_fixture_holds_every_cell(parent):
    want = ["%s/%s" % (p, c) for p in ("dense", "small", "batch") for c in V.CLASSES]
    want += ["lockstep/%s/%d" % (c, k) for c in V.LOCKSTEP_CLASSES for k in (0, 1)] + ["large/" + c for c in V.LARGE_CLASSES]
    want += ["%s/%s" % (p, c) for p in ("start/dense", "start/small", "start-batch") for c in V.START_CLASSES]
    assert sorted(parent) == sorted(want)
    assert all(parent[k]["status"] == 1 for k in V.solved_cells(parent))
    assert all(parent["large/" + c]["iterations"] == V.LARGE_CAP for c in V.LARGE_CLASSES)


@pytest.mark.parametrize("path", PATHS)
def test_bits_are_the_parents(parent, path):
    got = V.cells(ipm, want=(path,))
    assert got
    for k in sorted(got):
        print(k, got[k])
    differ = {k: (got[k], parent[k]) for k in got if got[k] != parent[k]}
    assert not differ, differ
