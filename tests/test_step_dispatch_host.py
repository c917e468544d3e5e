"""Host tests (no GPU) of the class-variant tables (csrc/vector_ops.h X_VARIANTS, csrc/small_lp.h SMALL_ROWS / SMALL_START_ROWS),
read back through the debug entry ipm_debug_step_kernel: which kernel, or which lockstep twin type, serves each problem class at
each step.  The expectation below is written out from the launch ladders the tables replaced (B, D, Q, F: bounded, detect, quad,
free); nothing of it is read from the library.  The twin ids are those of the enum declarations in csrc/lockstep.h.

The last test holds the host units to the tables: outside them no class-variant kernel is named, so a later variant cannot grow a
ladder of its own beside them."""
import ctypes as C
import glob
import itertools
import os
import re

import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interiorpointmethod_amd", "csrc")

ERR_INVALID_ARG = -1                                    # include/ipm_hip.h: IPM_ERR_INVALID_ARG
STEPS = ("prepare", "stop_test", "scaling", "direction", "mu_aff", "corrector_rhs", "update", "small", "small_batch", "small_start",
         "small_start_batch", "start_primal", "start_dual", "start_shift", "start_primal_correct", "start_dual_correct")


def _enum(name, known=()):
    """{enumerator: value} of `enum name { ... }` in lockstep.h: a value is a number or an enumerator of `known`, then they count up."""
    txt = re.sub(r"//.*", "", open(os.path.join(CSRC, "lockstep.h")).read())
    body = re.search(r"enum %s \{(.*?)\};" % name, txt, re.S).group(1)
    out, nxt = dict(known), 0
    for item in (s.strip() for s in body.split(",")):
        if "=" in item:
            item, val = (s.strip() for s in item.split("="))
            nxt = int(val) if val.isdigit() else out[val]
        out[item] = nxt
        nxt += 1
    return out


LS = _enum("LsBndType", _enum("LsType"))      # (the bounded twins' ids continue LsType's: LS_PREPARE_BND = LS_NTYPES)

SMALL = {  # flags -> (id, single-LP kernel, batch kernel)
    "": (0, "small_lp", "small_lp_batch"), "B": (1, "small_lp_bounded", "small_lp_batch_bounded"),
    "D": (2, "small_lp_detect", "small_lp_batch_detect"), "BD": (3, "small_lp_bounded_detect", "small_lp_batch_bounded_detect"),
    "Q": (4, "small_qp", "small_lp_batch_quad"), "BQ": (5, "small_qp_bounded", "small_lp_batch_bounded_quad"),
    "QF": (6, "small_qp_free", "small_lp_batch_free_quad"), "BQF": (7, "small_qp_bounded_free", "small_lp_batch_bounded_free_quad"),
    "DQ": (8, "small_qp_detect", "small_lp_batch_quad_detect"), "BDQ": (9, "small_qp_bounded_detect", "small_lp_batch_bounded_quad_detect"),
    "DQF": (10, "small_qp_free_detect", "small_lp_batch_free_quad_detect"),
    "BDQF": (11, "small_qp_bounded_free_detect", "small_lp_batch_bounded_free_quad_detect"),
}


def twin(name):
    return name, LS[name]


def kern(name):
    return name + "_kernel", -1


def expected(step, B, D, Q, F):
    """(name, twin id or -1; for the small steps the row's id) of a legal class."""
    b = "_bounded" if B else ""
    bnd = "_BND" if B else ""
    if step == "prepare":
        if D and Q:
            return kern("prepare%s_%s_detect" % (b, "free" if F else "quad"))
        if F or Q:
            return kern("prepare%s_%s" % (b, "free" if F else "quad"))
        return twin("LS_PREPARE" + ("_DETECT" if D else "") + bnd)
    if step == "stop_test":
        if D and Q:
            return kern("stop_test%s_%s_detect" % (b, "free" if F else "quad"))
        if F:
            return kern("stop_test%s_free" % b)
        return twin("LS_STOP_TEST" + ("_DETECT" if D else "") + bnd)            # Q alone takes the LP's stop test
    if step == "scaling":
        return kern("scaling%s%s" % (b, "_free" if F else "_quad" if Q else ""))
    if step == "direction":
        return kern("direction%s_free" % b) if F else twin("LS_DIRECTION" + bnd)
    if step in ("mu_aff", "update"):
        if F or Q:
            return kern("%s%s_%s" % (step, b, "free" if F else "quad"))
        return twin("LS_" + step.upper() + bnd)
    if step == "corrector_rhs":
        return kern("corrector_rhs%s_free" % b) if F else twin("LS_CORR_RHS" + bnd)
    if step in ("small", "small_batch"):
        row = SMALL["".join(c for c, on in zip("BDQF", (B, D, Q, F)) if on)]
        return row[1 if step == "small" else 2] + "_kernel", row[0]
    if step in ("small_start", "small_start_batch"):
        return step + b + "_kernel", int(B)
    return kern(step + b)                                                      # the five start steps of the multi-kernel path


def ask(lib, step, B, D, Q, F):
    name = C.create_string_buffer(96)
    tw = C.c_int32(-99)
    rc = lib.ipm_debug_step_kernel(STEPS.index(step), int(B), int(D), int(Q), int(F), name, len(name), C.byref(tw))
    return rc, name.value.decode(), tw.value


def test_twin_ids_are_the_declared_ones():
    assert (LS["LS_PREPARE"], LS["LS_STOP_TEST"], LS["LS_DIRECTION"], LS["LS_UPDATE"], LS["LS_NTYPES"]) == (2, 3, 18, 21, 29)
    assert (LS["LS_PREPARE_BND"], LS["LS_UPDATE_BND"], LS["LS_NTYPES_ALL"]) == (29, 36, 37) and len(set(LS.values())) == len(LS) - 1


@pytest.mark.parametrize("step", STEPS)
def test_every_class_gets_the_kernel_the_ladders_chose(step):
    lib = ipm.load_library()
    seen = set()
    for B, D, Q, F in itertools.product((False, True), repeat=4):
        rc, name, tw = ask(lib, step, B, D, Q, F)
        if F and not Q:
            assert rc == ERR_INVALID_ARG, (step, B, D, Q, F)
            continue
        assert rc == _lib.IPM_OK, (step, B, D, Q, F)
        assert (name, tw) == expected(step, B, D, Q, F), (step, B, D, Q, F)
        seen.add(name)
    rows = {"prepare": 12, "stop_test": 10, "scaling": 6, "direction": 4, "mu_aff": 6, "corrector_rhs": 4, "update": 6, "small": 12,
            "small_batch": 12}.get(step, 2)
    assert len(seen) == rows


def test_bad_arguments_are_refused():
    lib = ipm.load_library()
    tw = C.c_int32(0)
    for step in (-1, len(STEPS)):
        assert lib.ipm_debug_step_kernel(step, 0, 0, 0, 0, None, 0, C.byref(tw)) == ERR_INVALID_ARG
    assert lib.ipm_debug_step_kernel(0, 0, 0, 0, 0, None, 8, C.byref(tw)) == ERR_INVALID_ARG
    assert lib.ipm_debug_step_kernel(0, 0, 0, 0, 0, None, 0, C.byref(tw)) == _lib.IPM_OK and tw.value == LS["LS_PREPARE"]


FAMILIES = ("prepare", "stop_test", "scaling", "direction", "mu_aff", "corrector_rhs", "update", "small_lp", "small_qp", "small_start",
            "start_primal", "start_dual", "start_shift", "start_primal_correct", "start_dual_correct")
VARIANT_KERNEL = re.compile(r"\b(?:%s)(?:_[a-z_]+)?_kernel\b" % "|".join(FAMILIES))


def test_the_pattern_knows_the_kernels():
    for name in ("prepare_kernel", "stop_test_bounded_free_detect_kernel", "small_lp_batch_quad_kernel", "small_qp_kernel", "update_bounded_kernel",
                 "start_primal_correct_bounded_kernel", "small_start_batch_bounded_kernel"):
        assert VARIANT_KERNEL.search("launch(%s, g)" % name), name
    for name in ("mcc_direction_kernel", "chol_update_kernel", "launch_chol_update", "set_params_kernel", "gemv_n_kernel"):
        assert not VARIANT_KERNEL.search(name), name


def test_host_units_name_no_class_variant_kernel():
    files = sorted(glob.glob(os.path.join(CSRC, "host_*.h"))) + [os.path.join(CSRC, "ipm_api.hip")]
    assert len(files) >= 10
    hits = []
    for path in files:
        for no, line in enumerate(open(path), 1):
            code = line.split("//")[0]
            hits += ["%s:%d: %s" % (os.path.basename(path), no, m) for m in VARIANT_KERNEL.findall(code)]
    assert not hits, "class-variant kernels named outside their tables:\n" + "\n".join(hits)
