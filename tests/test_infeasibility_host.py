"""Host side of the infeasibility detection (IPM_FLAG_DETECT_INFEASIBILITY): no GPU.

  * scipy's HiGHS confirms the verdict of every instance of tests/infeas_cases.py;
  * verify_certificate accepts the exact certificates of the constructions and rejects perturbed ones;
  * the row-order mappings (a reordered sparse handle, the general-form front end) on hand-built arrays;
  * the default kernels compile to exactly the ISA of the sources before the feature (fixture
    tests/golden/isa_default_kernels.json: sha256 of each kernel's instruction text, recorded from those sources with the
    compiler named there)."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import sparse
from scipy.optimize import linprog

import infeas_cases as IC
from interiorpointmethod_amd import general_form as G
from interiorpointmethod_amd import solver as S
from interiorpointmethod_amd.solver import verify_certificate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA_FIXTURE = os.path.join(ROOT, "tests", "golden", "isa_default_kernels.json")


def _linprog_status(P):
    A, b, c, ub = P["A"], P["b"], P["c"], P["ub"]
    bounds = [(0.0, None if ub is None or not np.isfinite(ub[j]) else float(ub[j])) for j in range(c.shape[0])]
    A = sparse.csr_matrix(A) if not sparse.issparse(A) else A
    return linprog(c, A_eq=A, b_eq=b, bounds=bounds, method="highs").status


@pytest.mark.parametrize("name", sorted(IC.all_instances(large=False)))
def test_highs_confirms_the_verdict(name):
    P = IC.all_instances()[name]()
    assert _linprog_status(P) == {"primal_infeasible": 2, "dual_infeasible": 3}[P["kind"]], name


def test_recorded_highs_verdicts_of_the_netlib_fixtures():
    """tests/golden/netlib_highs_status.json (what the GPU no-false-positive test trusts): HiGHS's status of each valid
    standard-form fixture, min c.x, A x = b, x >= 0.  Several are infeasible in that form (their general form has bounds that
    the fixture drops).  Re-checked here for the fixtures of up to 700 rows."""
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "netlib_highs_status.json")))
    assert ref["BOEING1"] == 2 and ref["AFIRO"] == 0
    for nm, st in sorted(ref.items()):
        A, b, c = IC.netlib(nm)
        if A.shape[0] <= 700:
            assert linprog(c, A_eq=A, b_eq=b, bounds=(0, None), method="highs").status == st, nm


def test_large_dense_instance_is_unbounded():
    """HiGHS needs minutes for the 2688 x 5376 instance; its construction proves it: a feasible point x0 > 0 and a ray d > 0 with
    A d = 0 and c.d = -1 (HiGHS confirms the same construction at 40 x 90 above)."""
    P = IC.large_dense()
    A, b, c, x0, d = P["A"], P["b"], P["c"], P["x0"], P["cert"]["x"]
    assert A.shape == (21 * 128, 42 * 128)
    assert x0.min() > 0 and np.abs(A @ x0 - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert d.min() > 0 and abs(c @ d + 1.0) <= 1e-12 and np.abs(A @ d).max() <= 1e-10
    assert verify_certificate(A, b, c, P["cert"]) <= 1e-10


@pytest.mark.parametrize("name", sorted(IC.all_instances()))
def test_verify_certificate_exact_and_perturbed(name):
    P = IC.all_instances()[name]()
    cert = P["cert"]
    A, b, c, ub = P["A"], P["b"], P["c"], P["ub"]
    assert verify_certificate(A, b, c, cert, ub=ub) <= 1e-9, name
    # perturbed: the normalised violation becomes visible (and a wrong sign is no certificate at all)
    if cert["kind"] == "primal_infeasible":
        y = cert["y"]
        assert verify_certificate(A, b, c, dict(cert, y=-y), ub=ub) == np.inf       # b.(-y) < 0: no certificate at all
        # push the tightest column of A^T y over zero through one of its rows
        As = sparse.csc_matrix(A)
        aty = np.asarray(As.T @ y).reshape(-1) - cert["z"]
        j = int(np.argmax(np.where(np.diff(As.indptr) > 0, aty, -np.inf)))
        i, a = As.indices[As.indptr[j]], As.data[As.indptr[j]]
        y2 = y.copy()
        y2[i] += np.sign(a) * (abs(aty[j]) + 1.0) / abs(a)
        assert verify_certificate(A, b, c, dict(cert, y=y2), ub=ub) > 1e-6, name
    else:
        x = cert["x"]
        rng = np.random.default_rng(0)
        noisy = dict(cert, x=x + 1e-2 * x.max() * rng.random(x.size))
        assert verify_certificate(A, b, c, noisy, ub=ub) > 1e-6, name
        assert verify_certificate(A, b, c, dict(cert, x=-x), ub=ub) == np.inf


def test_verify_certificate_needs_z_for_the_bounded_instance():
    P = IC.bounded_primal_infeasible()
    cert = P["cert"]
    assert verify_certificate(P["A"], P["b"], P["c"], cert, ub=P["ub"]) <= 1e-12
    # without z the same y is no certificate (b.y = |S| + 1 > 0 but A^T y = 1 on S: violation 1 / (|S| + 1))
    assert verify_certificate(P["A"], P["b"], P["c"], dict(cert, z=np.zeros_like(cert["z"])), ub=P["ub"]) >= 1.0 / 11 - 1e-12
    # and without the bounds there is none at all: the LP is feasible
    assert _linprog_status(dict(P, ub=None)) == 0


def test_verify_certificate_rejects_unknown_kinds():
    with pytest.raises(ValueError):
        verify_certificate(np.eye(2), np.ones(2), np.ones(2), dict(kind="optimal"))


def test_rows_out_of_a_reordered_handle():
    """A sparse handle whose rows the host reordered holds device row i = caller row perm[i]: the certificate's y goes back
    through _rows_out (what IpmSolver.certificate does) and is then a certificate of the caller's A."""
    P = IC.afiro_negative_sum_row()
    A, b, c = P["A"], P["b"], P["c"]
    perm = np.random.default_rng(5).permutation(A.shape[0])
    sv = S.IpmSolver.__new__(S.IpmSolver)
    sv._perm = perm
    y_dev = P["cert"]["y"][perm]                       # what the device holds in its row order
    y = sv._rows_out(y_dev)
    assert np.array_equal(y, P["cert"]["y"])
    assert verify_certificate(A, b, c, dict(P["cert"], y=y)) == 0.0
    # the device-order vector is a certificate of the permuted problem only
    Ap = sparse.csc_matrix(sparse.csr_matrix(A)[perm])
    assert verify_certificate(Ap, b[perm], c, dict(P["cert"], y=y_dev)) == 0.0
    assert np.array_equal(sv._rows_in(y), y_dev)


def test_general_form_row_order_and_native_columns():
    """get_Abc stacks inequality rows, then equality rows: a Farkas y of the general form in that order certifies the standard
    form new_interior_sparse solves; _ray_native maps native columns back onto the get_Abc columns."""
    # x1 + x2 <= 1 (ineq), x1 + x2 = 3 (eq), x >= 0: infeasible, y = (-1 on the inequality row, +1 on the equality row) / 2
    c = np.array([1.0, 1.0])
    Aineq, bineq = np.array([[1.0, 1.0]]), np.array([1.0])
    Aeq, beq = np.array([[1.0, 1.0]]), np.array([3.0])
    A, b, cs, offset = G.standard_form(c, Aeq=Aeq, beq=beq, Aineq=Aineq, bineq=bineq)
    assert A.shape == (2, 3) and offset == 0.0                # the slack column of the inequality row is appended
    y = np.array([-1.0, 1.0]) / 2.0
    assert verify_certificate(A, b, cs, dict(kind="primal_infeasible", y=y, z=None)) == 0.0
    assert verify_certificate(A, b, cs, dict(kind="primal_infeasible", y=y[::-1], z=None)) > 0.1
    # native form with a fixed variable: its column is removed on the host and restored as 0 by _ray_native
    F = G.native_form(np.array([1.0, -1.0, 0.0]), Aeq=np.array([[1.0, 0.0, 1.0]]), beq=np.array([1.0]),
                      lb=np.array([0.0, 0.0, 2.0]), ub=np.array([np.inf, np.inf, 2.0]))
    assert list(F.keep) == [0, 1] and list(F.fixed) == [2]
    ray = G._ray_native(F, np.array([0.0, 1.0]))
    assert np.array_equal(ray, [0.0, 1.0, 0.0])
    assert ray[:F.n].tolist() == [0.0, 1.0, 0.0]


def test_status_names_and_flag():
    from interiorpointmethod_amd import _lib
    assert S.STATUS_NAMES[5] == "primal_infeasible" and S.STATUS_NAMES[6] == "dual_infeasible"
    assert _lib.FLAG_DETECT_INFEASIBILITY == 32
    hdr = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    assert re.search(r"IPM_FLAG_DETECT_INFEASIBILITY\s*=\s*32", hdr)
    assert re.search(r"IPM_STATUS_PRIMAL_INFEASIBLE\s*=\s*5", hdr) and re.search(r"IPM_STATUS_DUAL_INFEASIBLE\s*=\s*6", hdr)
    src = open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "small_lp.h")).read()
    assert re.search(r"IPM_STATUS_NEEDS_SHIFT\s*=\s*4", src)           # the internal status stays clear of 5 and 6


def test_summarize_counts_the_verdicts():
    from interiorpointmethod_amd import batch
    rec = np.zeros((4, batch.NF))
    rec[:, 1] = [1, 5, 6, 6]
    s = batch.summarize(rec)
    assert (s["converged"], s["primal_infeasible"], s["dual_infeasible"]) == (1, 1, 2)


def test_lockstep_shard_takes_the_flag_explicitly():
    import inspect
    from interiorpointmethod_amd import batch
    assert "detect_infeasibility" in inspect.signature(batch.solve_shard_lockstep).parameters
    assert "detect_infeasibility" in inspect.signature(batch.solve_one).parameters


# ---------------------------------------------------------------------------------------------------- ISA of the default kernels
def kernel_isa(asm_text):
    """{kernel symbol: sha256 of its instruction text} of a device assembly file; block labels are renumbered per kernel
    (their global numbering shifts whenever another function is added) and comments are dropped."""
    out, cur, body = {}, None, []
    for line in asm_text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = hashlib.sha256("\n".join(body).encode()).hexdigest()
            cur = None
            continue
        t = line.split(";")[0].rstrip()
        if t.strip():
            body.append(re.sub(r"\.Ltmp\d+", ".Ltmp", re.sub(r"\.LBB\d+_", ".LBB_", t)))
    return out


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def test_default_kernels_compile_to_the_same_isa(tmp_path):
    ref = json.load(open(ISA_FIXTURE))
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not available")
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    if ref["compiler"] not in ver:
        pytest.skip("the fixture was recorded with %r; this compiler is another one" % ref["compiler"])
    asm = tmp_path / "ipm_api.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(asm),
                    os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "ipm_api.hip")], check=True, capture_output=True)
    now = kernel_isa(asm.read_text())
    for k in ref["must_include"]:
        assert k in ref["kernels"], k
    changed = [k for k, h in ref["kernels"].items() if now.get(k) != h]
    assert not changed, "default kernels whose ISA changed: %s" % changed
    # the new instantiations exist next to them
    for k in ("prepare_detect_kernel", "stop_test_detect_kernel", "small_lp_detect_kernel", "ls_prepare_detect", "ls_stop_test_detect",
              "certificate_kernel"):
        assert any(k in s for s in now), k
