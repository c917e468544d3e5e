#!/usr/bin/env python3
"""bench.py -- IPM iterations/sec of the HIP Newton/KKT path on the dense synthetic LP.

    python bench.py --gpus N --steps K --warmup W [--full]

One "step" = one full Mehrotra predictor-corrector iteration (stop
test, form A D^2 A^T, Cholesky, two solves, two ratio tests, update) on the BASELINE.json
config "dense synthetic LP m=4096 n=8192 fp64" (generator of SURVEY.md 8d, seed 0, start
x=s=1, y=0).  All inputs are resident in HBM before the timed region.  The iterate is reset
to the start point every 20 steps (3 tiny fill launches, inside the timed region) so that
any K stays on the pre-convergence trajectory (the LP converges in 24 iterations).

N > 1 (launched by torch.distributed.run, one rank per GPU): the single-LP dense path does
not shard ("replicas only"): every rank solves its own replica, no data-path
collective; value = N*K / max-over-ranks time  (weak scaling).

A plain run does only what the headline figure needs: it sets up, warms up, times the K steps, writes --dump-outputs
and prints the result line.  Everything else the benchmark measures or checks runs only with --full: the phase
breakdown (an untimed pass of its own), the objective check against the reference trajectory, the CPU baselines and
the Netlib legs (each of which --no-cpu-baseline / --no-netlib still turns off).

The LAST stdout line (rank 0) is ONE compact JSON object (< 2 KB: `compact_line`) with the contract keys plus `roofline`
and, with --full, `cpu_baseline` and the headline numbers of the Netlib legs; the full record (per-LP tables, notes) is
printed as an earlier line prefixed `BENCH_DETAIL ` and written to bench_detail.json.  The record carries `roofline` (the
dominant kernel, the fp64-MFMA A D^2 A^T contraction, timed with HIP events on the solver's stream inside the
timed region) and, with --full, `cpu_baseline` (the NumPy normal-equations oracle on the host cores,
bounded sample, rank 0 at N=1 only), `cpu_baseline_reference_algorithm` (one iteration of the
reference's OWN algorithm -- dense (m+2n) KKT matrix, two LAPACK gesv, main.py:13-21/185-244 --
restated by the oracle, same rank/N) and the second half of BASELINE.json's metric on this GPU:
`netlib_all` = Netlib LPs/s over ALL 73 valid benchmarks/ LPs (BASELINE.json configs[3]) and `netlib`
= the 26-LP parity set, each with its own `roofline`, `cpu_baseline` (one time-bounded oracle pass)
and a per-LP table carrying setup/solve/teardown seconds and the library's hidden recoveries
(`timeouts_recovered`, `serial_launches`).  `--workload netlib` runs a set sharded over the ranks
with the same keys (its `cpu_baseline` with --full as well).
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

M_DEFAULT, N_DEFAULT = 4096, 8192
RESET_EVERY = 20
PEAK_FP64_MFMA_TFLOPS = 78.6      # MI355X dense fp64 matrix peak


def kernel_source_sha(fused=False):
    """sha256 (first 16 hex) of the sources the dominant kernel is built from -- adat_syrk_kernel on the serial path,
    form_factor_kernel on the fused one: a PMC pass collected for another version of the kernel is refused
    (profiles/*_pmc_form_kernel*.json carries the kernel name and the sha it was collected with)."""
    import hashlib
    hsh = hashlib.sha256()
    for f in ("adat_syrk_f64.h", "gemm_nt_f64.h") + (("form_factor.h", "ff_schedule.h", "potrf_f64.h") if fused else ()):
        with open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", f), "rb") as fh:
            hsh.update(fh.read())
    return hsh.hexdigest()[:16]


def load_traffic(m, n, fused=False):
    """(traffic bytes per launch | None, note).  HBM-side bytes of the dominant kernel from the newest committed PMC
    pass (tools/pmc_form_kernel.py), accepted only for the same problem size AND the same kernel source."""
    import glob
    best, other = None, None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_form_kernel*.json"))):
        try:
            with open(f) as fh:
                d = json.load(fh)
        except Exception:
            continue
        if ("form_factor" in d.get("kernel", "")) != bool(fused):
            continue                            # a pass of the other path's kernel
        if tuple(d.get("shape", ())) == (m, n):
            best = (f, d)                       # newest pass collected at this problem size
        else:
            other = (f, d)
    if best is None:
        return None, ("no PMC pass committed" if other is None else
                      "no PMC pass for %d x %d (newest is %s for shape %s)" % (m, n, os.path.basename(other[0]), other[1].get("shape")))
    f, d = best
    if d.get("kernel_source_sha") != kernel_source_sha(fused):
        return None, "stale: %s was collected for kernel source %s, current is %s" % (
            os.path.basename(f), d.get("kernel_source_sha"), kernel_source_sha(fused))
    return d["derived"]["traffic_bytes_per_launch"], "from %s (rocprofv3 --pmc, separate passes)" % os.path.basename(f)


def _r(v, nd=6):
    """Round floats for the compact line (significant digits, not decimals)."""
    if isinstance(v, float):
        return float("%.*g" % (nd, v))
    if isinstance(v, (list, tuple)):
        return [_r(x, 4) for x in v]
    return v


def _pick(d, keys):
    return {k: _r(d[k]) for k in keys if d is not None and k in d}


def _short(s, n=160):
    s = str(s)
    return s if len(s) <= n else s[:n - 3] + "..."


COMPACT_LIMIT = 2048        # bytes: the driver keeps only a tail of stdout (~8 KB); the LAST line must fit it whole


def compact_line(out):
    """The ONE line the driver parses: the contract keys, `roofline`, `cpu_baseline` and the headline numbers of the
    Netlib legs -- nothing per LP and no prose.  Everything else goes to the detail record (`emit`)."""
    c = _pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                    "vs_baseline", "dtype", "data"))
    c["config"] = {"workload": _short(out.get("config", {}).get("workload", ""), 260)}
    rf = out.get("roofline") or {}
    c["roofline"] = _pick(rf, ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch",
                               "flops_per_launch", "avg_launch_ms"))
    if "kernel" in rf:
        c["roofline"]["kernel"] = _short(rf["kernel"], 40).split(" ")[0]
    if out.get("cpu_baseline"):
        c["cpu_baseline"] = _pick(out["cpu_baseline"], ("value", "unit", "cores", "kind"))
        c["cpu_baseline"]["sample"] = _short(out["cpu_baseline"].get("sample", ""), 60)
    if out.get("cpu_baseline_reference_algorithm"):
        c["cpu_baseline_reference_algorithm"] = _pick(out["cpu_baseline_reference_algorithm"], ("value", "unit", "cores"))
    for k in ("objective_check", "objective_checked"):
        if k in out:
            c[k] = _r(out[k], 13)
    if "whole_iteration" in out:
        c["whole_iteration"] = _pick(out["whole_iteration"], ("tflops", "frac_of_fp64_mfma_peak"))
    for key in ("netlib_all", "netlib"):
        nl = out.get(key)
        if not nl:
            continue
        e = _pick(nl, ("value", "unit", "wall_seconds", "wall_seconds_runs", "projected_makespan_8gpu_s", "slowest_lp"))
        sm = nl.get("summary") or {}
        e.update(_pick(sm, ("n", "converged", "total_iterations", "timeouts_recovered", "serial_launches")))
        e["roofline_frac"] = _r((nl.get("roofline") or {}).get("frac"))
        if nl.get("cpu_baseline"):
            e["cpu_baseline"] = _pick(nl["cpu_baseline"], ("value", "unit", "cores", "kind"))
        if nl.get("emulated_multi_gpu"):
            e["emulated_multi_gpu"] = _pick(nl["emulated_multi_gpu"], ("world", "wall_seconds", "value", "converged"))
        c[key] = e
    # the netlib workload's own line (bench.py --workload netlib) carries these at top level
    if "summary" in out:
        c["summary"] = _pick(out["summary"], ("n", "converged", "max_iter", "nan", "invalid", "errors", "total_iterations",
                                              "timeouts_recovered", "serial_launches"))
        c.update(_pick(out, ("wall_seconds", "projected_makespan_8gpu_s", "slowest_lp")))
    if "detail" in out:
        c["detail"] = out["detail"]
    line = json.dumps(c, separators=(",", ":"))
    if len(line) > COMPACT_LIMIT:                       # never happens with the keys above; keep the contract keys if it does
        for k in ("netlib", "netlib_all", "whole_iteration", "cpu_baseline_reference_algorithm"):
            c.pop(k, None)
            line = json.dumps(c, separators=(",", ":"))
            if len(line) <= COMPACT_LIMIT:
                break
    return line


def emit(out):
    """Write the full record (per-LP tables, notes) to bench_detail.json (under gpurun_out/ when that exists, so that it
    travels back from the GPU box) and print it as an EARLIER stdout line; the LAST stdout line is the compact one."""
    dd = os.path.join(ROOT, "gpurun_out")
    path = os.path.join(dd if os.path.isdir(dd) else ROOT, "bench_detail.json")
    try:
        with open(path, "w") as fh:
            json.dump(out, fh)
        out["detail"] = os.path.relpath(path, ROOT)
    except OSError:
        pass
    sys.stderr.flush()
    print("BENCH_DETAIL " + json.dumps(out))
    print(compact_line(out))
    sys.stdout.flush()


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """Write each array as d/<name>.npy in float64.  When the data exceed DUMP_MAX_BYTES in all (less 1 MB for the
    headers), every array is cut to the same share of its elements, a sample drawn with a fixed seed (flattened,
    positions sorted), so that two builds given the same arguments are compared element for element."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    budget = (DUMP_MAX_BYTES - (1 << 20)) // 8
    total = sum(a.size for a in arrays.values())
    for k, a in arrays.items():
        if total > budget:
            keep = max(1, a.size * budget // total)
            a = a.ravel()[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(d, k + ".npy"), a)


def makespan_fields(names, rec):
    """Scaling ceiling visible from one GPU: with the LPs spread over 8 GPUs the wall cannot go below the slowest single LP
    (seconds as measured here, under this run's contention)."""
    import numpy as np
    i = int(np.argmax(rec[:, 7]))
    return {"projected_makespan_8gpu_s": float(rec[i, 7]), "slowest_lp": names[int(rec[i, 0])]}


def emulated_multi_gpu(names, probs, flops, dev, world=8):
    """What `world` GPUs would do with this set, MEASURED on one: the static LPT shards of batch.run_batch (the partition every rank
    derives for itself) are solved one shard after the other on this GPU, each exactly as its rank would solve it (eight LPs in
    flight; a shard is too small for the lockstep batches); the slowest shard is the wall of the multi-GPU run -- the ranks share
    nothing but the final all-gather of 112-byte records.  (The dynamic schedule of a real run can only shorten it.)"""
    from interiorpointmethod_amd import batch
    costs = [batch.predicted_cost(p[0].shape[0], p[0].shape[1]) for p in probs]
    shards = batch.lpt_partition(costs, world)
    walls, conv, slowest = [], 0, None
    for ids in shards:
        if not ids:
            walls.append(0.0)
            continue
        sub = [probs[i] for i in ids]
        rec, el = run_netlib([names[i] for i in ids], sub, [flops[i] for i in ids], dev, workers=8)
        conv += int((rec[:, 1] == 1.0).sum())
        if el >= max(walls + [0.0]):
            j = int(rec[:, 7].argmax())
            slowest = names[ids[int(rec[j, 0])]]
        walls.append(float(el))
    wall = max(walls)
    return {"world": world, "wall_seconds": wall, "value": conv / wall if wall > 0 else 0.0, "unit": "LPs/s", "converged": conv,
            "shard_walls": walls, "slowest_lp_of_slowest_shard": slowest,
            "how": "the %d static LPT shards solved one after the other on ONE GPU, each as its rank would; wall = slowest shard" % world}


def _blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return int(max([p.get("num_threads", 1) for p in threadpool_info()] or [1]))
    except Exception:
        return int(os.cpu_count() or 1)


def cpu_baseline_reference_algorithm(A, b, c):
    """ONE iteration of the reference's own dense algorithm (assemble the (m+2n)^2 KKT matrix, two LAPACK gesv:
    main.py:13-21, 185-244) as restated by oracle.iterate(method="full"), from the start point, on the host."""
    from oracle import ipm_oracle as O
    import numpy as np
    m, n = A.shape
    x, y, s = O.initial_point(m, n, 0.0)
    t0 = time.perf_counter()
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        O.iterate(A, b, c, x, y, s, method="full")
    dt = time.perf_counter() - t0
    return {"value": 1.0 / dt, "unit": "iterations/s", "cores": _blas_threads(), "kind": "port",
            "sample": "1 iteration of oracle.iterate(method='full'): dense KKT matrix of order m+2n = %d, two LAPACK "
                      "gesv (the reference's algorithm, main.py:13-21/185-244), %.1f s; survey container (8 Xeon "
                      "cores, reference verbatim): 106.7 s/iteration at 4096x8192 (BASELINE.md 2.2)" % (m + 2 * n, dt)}


def cpu_baseline(A, b, c, budget_s=20.0, max_its=6):
    """Oracle (NumPy normal equations + LAPACK Cholesky) timed on the host: bounded sample."""
    import numpy as np
    from oracle import ipm_oracle as O
    m, n = A.shape
    x, y, s = O.initial_point(m, n, 0.0)
    t0 = time.perf_counter()
    its = 0
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        while its < max_its and (time.perf_counter() - t0) < budget_s:
            x, y, s, _ = O.iterate(A, b, c, x, y, s, method="normal")
            its += 1
    dt = time.perf_counter() - t0
    return {"value": its / dt, "unit": "iterations/s", "cores": _blas_threads(), "kind": "port",
            "sample": "%d iterations of oracle.iterate(method='normal') (NumPy (A*d)@A.T + LAPACK potrf: the SAME "
                      "normal-equations algorithm the GPU runs, not the reference's full-KKT LU -- that one is "
                      "cpu_baseline_reference_algorithm) on the same %dx%d LP from the start point, %.1f s, host has "
                      "%d logical CPUs" % (its, m, n, dt, os.cpu_count() or 0)}


def _dist_setup(local_rank, world, want_store=False):
    """(dist module or None, device index, device for the scalar reductions, store or None).  One rank per GPU over
    RCCL; the environment IPM_BENCH_BACKEND=gloo + IPM_BENCH_ONE_DEVICE=1 rehearses the multi-rank code path on a
    one-GPU box (every rank on device 0, CPU collectives).  want_store: a TCPStore (public API) for the
    self-scheduling counter of the batched mode, or None when it cannot be set up on every rank."""
    import torch
    force = bool(os.environ.get("IPM_BENCH_FORCE_DIST"))      # a process group of ONE rank: exercises the RCCL branch on one GPU
    if world <= 1 and not force:
        return None, local_rank, "cuda", None
    import torch.distributed as dist
    if world <= 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        world = 1
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    backend = os.environ.get("IPM_BENCH_BACKEND", "nccl")
    dev = 0 if os.environ.get("IPM_BENCH_ONE_DEVICE") else local_rank
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev))
        red = "cuda"
    else:
        dist.init_process_group(backend=backend)
        red = "cpu"
    store = None
    if want_store:
        from interiorpointmethod_amd import batch
        try:
            store = batch.make_store(dist.get_rank(), world, timeout_s=60)
        except Exception as e:          # port in use, ...: fall back to the static partition -- on EVERY rank
            print("bench: no scheduling store on rank %d (%s)" % (dist.get_rank(), e), file=sys.stderr)
        ok = torch.tensor([1 if store is not None else 0], dtype=torch.int32, device=red)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            store = None
    return dist, dev, red, store


PARITY_SET = ["AFIRO", "BANDM", "DEGEN2", "E226", "FIT1P", "GROW15", "GROW22", "GROW7", "KB2", "MAROS-R7", "SC105",
              "SC205", "SC50A", "SC50B", "SCSD1", "SCSD6", "SCSD8", "SCTAP1", "SCTAP2", "SCTAP3", "SHARE2B",
              "STOCFOR1", "STOCFOR2", "STOCFOR3", "TRUSS", "WOODW"]


PATHS = {}          # LP name -> "sparse" | "dense": the factorization path IpmSolver's rule picks (filled by load_netlib)
ORDER_INFO = {}     # LP name -> ipm_order_rows info (panel tree height, critical-path area) for the sparse-path LPs


def load_netlib(which, max_m=1 << 30):
    """(names, problems, algorithmic flops per iteration) of the committed Netlib fixtures.  which: "all" (73 valid
    benchmarks/ files), "parity" (the 26 the reference converges on), "general" (benchmarks_full through the
    general-form front end; conversion on the host, untimed)."""
    import glob
    import numpy as np
    from scipy import sparse
    from interiorpointmethod_amd.matio import load_npz_problem
    from interiorpointmethod_amd.solver import path_flops
    names, probs, flops = [], [], []

    def add(nm, A, b, c):
        # flops of one iteration as the device runs it: sparse contraction sum_j nnz_j^2; the Cholesky -- multifrontal
        # sparse factor: sum over columns of count^2; blocked dense factor: inside the tile envelope, m^3/3 when there is
        # none --; the four triangular sweeps (4 nnz(L) or 4 m^2); 12 nnz for the six SpMVs
        A = sparse.csc_matrix(A)
        names.append(nm); probs.append((A, b, c))
        path, f_chol, f_sweeps, info = path_flops(A, want_info=True)
        PATHS[nm] = path
        if path == "sparse":
            ORDER_INFO[nm] = info
        flops.append(float(np.sum(np.diff(A.indptr).astype(np.float64) ** 2)) + f_chol + f_sweeps + 12.0 * A.nnz)

    if which == "general":
        from interiorpointmethod_amd import general_form as G
        for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "general", "*.npz"))):
            z = np.load(f)

            def mat(prefix):
                if prefix + "_none" in z.files:
                    return None
                return sparse.csc_matrix((z[prefix + "_data"], z[prefix + "_indices"], z[prefix + "_indptr"]),
                                         shape=tuple(int(v) for v in z[prefix + "_shape"]))
            A, b, c, _ = G.standard_form(z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None,
                                         Aineq=mat("Aineq"), bineq=z["bineq"] if "bineq" in z.files else None,
                                         lb=z["lb"], ub=z["ub"])
            if A.shape[0] <= max_m:
                add(os.path.basename(f)[:-4], A, b, c)
        return names, probs, flops
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "netlib", "*.npz"))):
        nm = os.path.basename(f)[:-4]
        if which == "parity" and nm not in PARITY_SET:
            continue
        A, b, c, cTlb, valid = load_npz_problem(f)
        if valid and A.shape[0] <= max_m:
            add(nm, A, b, c)
    return names, probs, flops


def predicted_ms_per_iteration(name, m):
    """The fitted per-iteration latency models of DESIGN.md 4-S (solver.prefer_sparse_factor): sparse multifrontal factor
    0.061 ms per level of the panel tree + 3.5e-6 ms per (front rows)^2 along the critical path (floor 0.3 ms);
    dense-tile factor 0.1 ms + 0.08 ms per 128-row block; the fused single-workgroup kernel (m <= 128) 0.02 ms."""
    from interiorpointmethod_amd.solver import FUSED_SMALL_MAX_ROWS
    if m <= FUSED_SMALL_MAX_ROWS:
        return 0.02
    info = ORDER_INFO.get(name)
    if PATHS.get(name) == "sparse" and info:
        return max(0.3, -0.13 + 0.061 * info["panel_height"] + 3.5e-6 * info["path_area"])
    return 0.1 + 0.08 * ((m + 127) // 128)


def netlib_roofline(names, probs, flops, rec, elapsed, world):
    """Roofline view of a batched run.  Algorithmic flops of an LP = iterations x (sum_j nnz(A[:,j])^2 + Cholesky + sweeps
    + 12 nnz) (SURVEY 8d with the sparse contraction count; the Cholesky term as the device runs it, solver.path_flops).
    The suite is NOT flop bound: every iteration is a chain of dependent steps (pivot blocks / levels of the panel tree),
    so the prediction of the two fitted latency models (predicted_ms_per_iteration) is printed beside the MFMA fraction."""
    import numpy as np
    its = rec[:, 2]
    total = float(np.sum(its * np.array(flops)))
    ms_it = np.array([predicted_ms_per_iteration(nm, p[0].shape[0]) for nm, p in zip(names, probs)])
    per_lp_s = its * ms_it * 1e-3
    ach = total / elapsed / 1e12
    return {"bound": "mfma", "achieved": ach, "peak": PEAK_FP64_MFMA_TFLOPS * max(world, 1), "unit": "TFLOP/s",
            "frac": ach / (PEAK_FP64_MFMA_TFLOPS * max(world, 1)), "traffic": None,
            "flops_total": total, "iterations_total": int(its.sum()),
            "sparse_factor_lps": sorted(nm for nm in names if PATHS.get(nm) == "sparse"),
            "note": "sum over LPs of iterations x (sum_j nnz_j^2 + Cholesky flops [sparse multifrontal factor: sum over columns of "
                    "count^2; dense-tile factor: m^3/3, or inside the tile envelope] + sweeps [4 nnz(L) or 4 m^2] + 12 nnz) / "
                    "wall / (78.6 TFLOP/s x GPUs); the suite is bound by dependent steps (pivot chain / elimination-tree "
                    "levels), not by flops",
            "latency_floor": {"model": "iterations x fitted ms per iteration, one LP at a time with the look-ahead (DESIGN 4-S: "
                                       "sparse factor max(0.3, -0.13 + 0.061 panel-tree levels + 3.5e-6 critical-path area); "
                                       "dense-tile factor 0.1 + 0.08 per 128-row block; fused small-LP kernel 0.02)",
                              "chain_seconds_one_gpu": float(per_lp_s.sum()),
                              "largest_lp_predicted_seconds": float(per_lp_s.max()) if len(per_lp_s) else 0.0,
                              "largest_lp_predicted": names[int(np.argmax(per_lp_s))] if len(per_lp_s) else None,
                              "measured_wall_seconds": elapsed,
                              "largest_lp_seconds": float(rec[:, 7].max()),
                              "largest_lp": names[int(rec[int(np.argmax(rec[:, 7])), 0])]}}


def per_lp_table(names, rec):
    """Per-LP view of the gathered records: status, iterations, objective, wall seconds and its host-side split, and the
    library's hidden recoveries (batch.RECORD_FIELDS)."""
    return {names[int(r[0])]: {"status": int(r[1]), "it": int(r[2]), "obj": r[3], "s": round(r[7], 3),
                               "setup_s": round(r[11], 3), "solve_s": round(r[12], 3), "teardown_s": round(r[13], 3),
                               "timeouts_recovered": int(r[9]), "serial_launches": int(r[10])} for r in rec}


def netlib_cpu_baseline(names, probs, budget_s=20.0, tol_gap=None, max_iter=300):
    """The oracle (normal equations + guarded Cholesky, the algorithm the GPU runs) over a sample of the same set on the
    host, BOUNDED BY TIME: smallest LPs first; an LP is started only while its predicted cost (dense m x m Cholesky +
    formation per iteration at a few GFLOP/s effective, 60 iterations) fits what is left of the budget, and the loop
    ends at the budget.  One process, BLAS threads as configured.  Returns the per-LP seconds too, so that a subset (the
    parity set inside the full suite) can be reported from the same pass."""
    import numpy as np
    from oracle import ipm_oracle as O
    order = sorted(range(len(names)), key=lambda i: (probs[i][0].shape[0] * probs[i][0].shape[1], names[i]))
    done, per, skipped, t0 = [], {}, [], time.perf_counter()
    for i in order:
        left = budget_s - (time.perf_counter() - t0)
        if left <= 0:
            break
        A, b, c = probs[i]
        m, n = A.shape
        predicted = 60.0 * (m ** 3 / 3.0 + 2.0 * m * m * min(n, 50 * m) * 0.02) / 5e9      # crude: skip what cannot fit
        if predicted > left:
            skipped.append(names[i])
            continue
        t1 = time.perf_counter()
        with np.errstate(all="ignore"), warnings.catch_warnings():       # the oracle overflows on diverging LPs, as the reference does
            warnings.simplefilter("ignore")
            x, y, s, info = O.solve(A, b, c, tol=1e-8, y0=1.0, method="normal", max_iter=max_iter, tol_gap=tol_gap)
        per[names[i]] = (time.perf_counter() - t1, int(info["status"] == O.STATUS_OK))
        done.append(names[i])
    dt = time.perf_counter() - t0
    conv = sum(v[1] for v in per.values())
    return {"value": conv / dt if dt > 0 else 0.0, "unit": "LPs/s", "cores": _blas_threads(), "kind": "port",
            "sample": "oracle.solve(method='normal') smallest-first over the set within a %.0f s budget: %d LPs solved (%s ... %s), "
                      "%d converged, %.1f s, one process; not started (predicted beyond the budget): %d LPs; reference verbatim "
                      "loop in the survey container: 26 LPs in 603 s = 0.043 LPs/s per worker (BASELINE.md 2.4)" % (
                          budget_s, len(done), done[0] if done else "-", done[-1] if done else "-", conv, dt, len(skipped)),
            "sample_names": done, "seconds_per_lp": {k: round(v[0], 4) for k, v in per.items()},
            "converged_per_lp": {k: v[1] for k, v in per.items()}}


def cpu_baseline_subset(cb, subset):
    """The view of one netlib_cpu_baseline pass restricted to the LPs of `subset` (same timings, no second run)."""
    nm = [k for k in cb["sample_names"] if k in subset]
    dt = sum(cb["seconds_per_lp"][k] for k in nm)
    conv = sum(cb["converged_per_lp"][k] for k in nm)
    return {"value": conv / dt if dt > 0 else 0.0, "unit": "LPs/s", "cores": cb["cores"], "kind": "port",
            "sample": "the %d LPs of this set inside the time-bounded oracle pass over the full suite (netlib_all.cpu_baseline): "
                      "%d converged in %.1f s" % (len(nm), conv, dt), "sample_names": nm}


def lockstep_mode(lockstep=True, start="reference"):
    """run_batch's lockstep argument: IPM_LOCKSTEP=0 never, =1 always, unset: "auto" (batch.lockstep_wanted)."""
    env = os.environ.get("IPM_LOCKSTEP", "auto")
    if not lockstep or start != "reference" or env == "0":
        return False
    return True if env == "1" else "auto"


def run_netlib(names, probs, flops, dev, dist=None, red_dev="cuda", store=None, workers=2, schedule="dynamic",
               start="reference", regularize=0.0, general=False, lockstep=True):
    """Timed batched solve of the set -> (records, elapsed seconds incl. the gather, max over ranks)."""
    import torch
    from interiorpointmethod_amd import batch
    costs = [batch.predicted_cost(p[0].shape[0], p[0].shape[1]) for p in probs]
    order_mode = os.environ.get("IPM_BENCH_ORDER", "")
    if order_mode:                                   # experiment: where in the queue the sparse-factor LPs go
        for i, nm in enumerate(names):
            if PATHS.get(nm) == "sparse":
                costs[i] = 1e9 + costs[i] if order_mode == "sparse_first" else 1e-3 * costs[i]
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    rec, _ = batch.run_batch(probs, costs=costs, device=dev, dist=dist, store=store,
                             collective_at_world_one=bool(os.environ.get("IPM_BENCH_FORCE_DIST")),
                             gather_device=torch.device("cuda", dev) if (dist is not None and red_dev == "cuda") else None,
                             tol=1e-8, regularize=regularize, workers=workers, schedule=schedule, start=start,
                             lockstep=lockstep_mode(lockstep, start),
                             # the general-form driver's own settings: e3 = 1e-6, at most 999 iterations (main.py:1088-1127)
                             **(dict(max_iter=999, tol_gap=1e-6) if general else dict(max_iter=300)))
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    return rec, elapsed


def netlib_main(args):
    """Batched-LP mode (BASELINE.json configs[3]): the Netlib fixtures sharded over the ranks (self-scheduled from a
    shared counter, or a static LPT partition), a single RCCL all-gather of the statistics records at the end."""
    import numpy as np
    import torch
    from interiorpointmethod_amd import batch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist, dev, red_dev, store = _dist_setup(local_rank, world, want_store=(args.schedule == "dynamic"))
    names, probs, flops = load_netlib(args.netlib_set, args.max_m)
    general = args.netlib_set == "general"
    # warm-up: one small solve per rank (library load, first-launch costs) outside the timed region
    batch.solve_one(probs[names.index("AFIRO")] if "AFIRO" in names else probs[0], device=dev)
    if os.environ.get("IPM_DUMP_MAPS"):
        # diagnostic for a profiled run (tools/prof_suite.sh): the address map of this process after every library is
        # loaded, so that a raw stack trace of a fault under rocprofv3 can be symbolised afterwards
        with open("/proc/self/maps") as fi, open(os.environ["IPM_DUMP_MAPS"], "w") as fo:
            fo.write(fi.read())
    rec, elapsed = run_netlib(names, probs, flops, dev, dist=dist, red_dev=red_dev, store=store, workers=args.workers,
                              schedule=args.schedule, start=args.start, regularize=args.regularize, general=general)
    if rank == 0:
        if args.dump_outputs:
            by_lp = rec[np.argsort(rec[:, 0])]
            dump_outputs(args.dump_outputs, {"status": by_lp[:, 1], "iterations": by_lp[:, 2], "objective": by_lp[:, 3]})
        summ = batch.summarize(rec)
        sched = "one rank" if dist is None else ("self-scheduled from a shared counter (TCPStore)"
                                                 if (args.schedule == "dynamic" and store is not None) else "static LPT partition")
        if dist is not None:
            sched += ", records through dist.all_gather (backend %s, world %d)" % (dist.get_backend(), max(world, 1))
        out = {"metric": "Netlib LPs/sec (benchmarks_full/ general-form suite, batched, tol=1e-8, e3=1e-6, cap 999)"
                         if general else "Netlib LPs/sec (benchmarks/ suite, batched, tol=1e-8, cap 300)",
               "value": summ["converged"] / elapsed, "unit": "LPs/s", "n_gpus": max(world, 1), "steps": len(names),
               "warmup": 1, "ms_per_step": 1e3 * elapsed / max(len(names), 1), "higher_is_better": True,
               "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "netlib fixtures (tests/golden/netlib)",
               "config": {"workload": "Netlib %s set, %d LPs over %d GPU(s), %s; per GPU %s" % (
                   args.netlib_set, len(names), max(world, 1), sched,
                   "lockstep batches by size class (iteration k of the LPs of a class in the same launches), %d set-up threads" % max(1, args.workers)
                   if batch.lockstep_wanted(probs, max(world, 1), args.workers, lockstep_mode(True, args.start))
                   else "%d LP(s) in flight on separate streams" % max(1, args.workers))},
               "roofline": netlib_roofline(names, probs, flops, rec, elapsed, world),
               "summary": summ, "wall_seconds": elapsed, "regularize": args.regularize, "start_point": args.start,
               "per_lp": per_lp_table(names, rec)}
        if args.full and world == 1 and not args.no_cpu_baseline:
            cb = netlib_cpu_baseline(names, probs, tol_gap=1e-6 if general else None, max_iter=999 if general else 300)
            cb["gpu_seconds_same_sample"] = float(sum(r[7] for r in rec if names[int(r[0])] in cb["sample_names"]))
            out["cpu_baseline"] = cb
        out.update(makespan_fields(names, rec))
        emit(out)
    if dist is not None:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m", type=int, default=M_DEFAULT)
    ap.add_argument("--n", type=int, default=N_DEFAULT)
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps, measure and check everything else: dense = the phase breakdown, the "
                         "objective check, the CPU baselines and the Netlib legs; netlib = the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-netlib", action="store_true", help="dense workload, --full: skip the Netlib legs")
    ap.add_argument("--workload", default="dense", choices=["dense", "netlib"],
                    help="dense: IPM iterations/s on the synthetic LP (default, the headline metric); "
                         "netlib: LPs/s over the committed Netlib fixtures, sharded over the ranks")
    ap.add_argument("--netlib-set", default="all", choices=["all", "parity", "general"],
                    help="all 73 valid standard-form files, the 26 on which the reference converges, or the 72 general-form "
                         "files (benchmarks_full) through the general-form front end")
    ap.add_argument("--emulate-world", type=int, default=8, help="dense workload, --full: after the Netlib legs, also solve the static shards of this many ranks one after the other on this GPU (0 = skip)")
    ap.add_argument("--netlib-reps", type=int, default=3, help="dense workload, --full: runs of each Netlib leg (the median one is reported)")
    ap.add_argument("--max-m", type=int, default=1 << 30, help="netlib: skip LPs with more rows")
    ap.add_argument("--workers", type=int, default=8, help="netlib: LPs in flight per GPU, each on one stream (1 = strictly one at a time, with the look-ahead)")
    ap.add_argument("--schedule", default="dynamic", choices=["dynamic", "static"],
                    help="netlib, N > 1: pull LPs from a shared counter (rendezvous store) or static LPT partition")
    ap.add_argument("--start-point", dest="start", default="reference", choices=["reference", "mehrotra"],
                    help="netlib: start point; reference = x=s=y=1 (sparse_interior.py:193-200, parity mode), mehrotra = "
                         "Mehrotra's least-squares start (optional mode, not the reference's algorithm)")
    ap.add_argument("--regularize", type=float, default=0.0, help="netlib: Tikhonov shift (0 = reference-faithful)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy "
                         "(float64, at most 64 MB in all): dense = the iterate x, y, s and the step's statistics; "
                         "netlib = status, iterations and objective of every LP in suite order")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.workload == "netlib":
        return netlib_main(args)

    import numpy as np
    import torch
    import interiorpointmethod_amd as ipm
    from interiorpointmethod_amd.workloads import synthetic_lp, flops_per_iteration

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist, dev, red_dev, _ = _dist_setup(local_rank, world)
    ngpu = max(world, 1)
    if args.gpus != ngpu and rank == 0 and world > 1:
        print("warning: --gpus %d but WORLD_SIZE %d" % (args.gpus, world), file=sys.stderr)

    m, n = args.m, args.n
    A, b, c = synthetic_lp(m, n, seed=0)              # same LP on every rank (replicas)
    sv = ipm.IpmSolver(A, b, c, device=dev)

    def run(steps, profile=0):
        sv.set_profiling(profile)
        done, total_ms, st = 0, 0.0, None
        form_ms = factor_ms = tri_ms = other_ms = 0.0
        while done < steps:
            k = min(RESET_EVERY, steps - done)
            sv.init_state(0.0)
            st = sv.iterate(k)
            total_ms += st["solve_ms"]
            if profile:
                ph = sv.phase_ms()
                form_ms += ph["form"] * k; factor_ms += ph["factor"] * k
                tri_ms += ph["trisolve"] * k; other_ms += ph["other"] * k
            done += k
        return total_ms, (form_ms, factor_ms, tri_ms, other_ms), st

    run(args.warmup)
    fused = bool(sv.schedule().get("fused_factor"))       # the iteration ran the fused formation + factorization launch
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    dev_ms, phases, st = run(args.steps, profile=1)      # two event records per step around the dominant kernel
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if dist is not None:
        dist.barrier()
    elapsed = t1 - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs and rank == 0:
        # read back before the untimed passes below reset the iterate; solve_ms is a timing, not a result
        x, y, s = sv.get_state()
        dump_outputs(args.dump_outputs, dict({"x": x, "y": y, "s": s},
                                             **{k: v for k, v in st.items() if k != "solve_ms"}))

    KB = min(args.steps, RESET_EVERY)
    if args.full:
        # phase breakdown from a separate, untimed pass (nine event records per step cost ~1 %)
        _, phases_all, _ = run(KB, profile=2)
        torch.cuda.synchronize()

    if rank == 0:
        K = args.steps
        its_per_s = ngpu * K / elapsed
        form_ms = phases[0] / K
        nblk = (m + 127) // 128
        roles = fused and os.environ.get("IPM_FF_CHAIN_MODE", "1") != "0"
        if roles:
            # the dominant kernel is the ONE persistent launch that forms B = A D^2 A^T (m^2 n) and factors it (m^3 / 3): the pivot
            # chain and its small products are roles of the same launch
            flops_form = float(m) * m * n + float(m) ** 3 / 3.0
        elif fused:
            # chain_mode 0: the worker launch does the formation (m^2 n) AND the factorization's matrix work outside the pivot chain
            # (m^3 / 3 minus, per 128-row block, the diagonal block's own factorization and the chain's panel solve and tile
            # update: 128^3 (1/3 + 2 + 1) flop)
            flops_form = float(m) * m * n + float(m) ** 3 / 3.0 - nblk * 128.0 ** 3 * (1.0 / 3.0 + 3.0)
        else:
            flops_form = float(m) * m * n                       # lower-triangle SYRK, SURVEY 8(d)
        achieved = flops_form / (form_ms * 1e-3) / 1e12 if form_ms > 0 else 0.0
        traffic, traffic_src = load_traffic(m, n, fused)      # HBM-side bytes per launch: PMC pass collected separately
        out = {
            "metric": "IPM iterations/sec (m=%d,n=%d dense LP)" % (m, n),
            "value": its_per_s, "unit": "iterations/s", "n_gpus": ngpu, "steps": K, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / K, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "dense synthetic LP m=%d n=%d fp64, seed 0, start x=s=1 y=0 (%s); replicas per GPU" % (
                           m, n, {(4096, 8192): "BASELINE.json configs[1]", (16384, 32768): "BASELINE.json configs[4]"}.get(
                               (m, n), "not a BASELINE.json config: size sweep")),
                       "reset_every": RESET_EVERY},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_FP64_MFMA_TFLOPS,
                         "unit": "TFLOP/s", "frac": achieved / PEAK_FP64_MFMA_TFLOPS, "traffic": traffic,
                         "traffic_source": traffic_src,
                         "traffic_note": "L2<->fabric bytes per launch (2*FETCH_SIZE + WRITE_SIZE, gfx950 correction), null when "
                                         "the committed PMC pass was collected for another kernel source or size; algorithmic "
                                         "bytes 8mn + 4m^2 (+ 4m^2 for L when the launch also factors)",
                         "algorithmic_bytes_per_launch": 8.0 * m * n + 4.0 * m * m * (2.0 if fused else 1.0),
                         "kernel": ("form_factor_roles_kernel (ONE persistent launch of as many workgroups as CUs: B = A diag(d) A^T in 256x128 tile "
                                    "pairs, every update and panel solve of its Cholesky, and the pivot chain as roles of the launch; "
                                    "v_mfma_f64_16x16x4_f64)" if roles else
                                    "form_factor_kernel (persistent launch beside the pivot chain: B = A diag(d) A^T in 256x128 tile pairs + every "
                                    "trailing update and panel solve of the Cholesky outside the chain, v_mfma_f64_16x16x4_f64; 224 of 256 CUs)"
                                    if fused else "adat_syrk_kernel (B = A diag(d) A^T, lower 128x128 tiles, v_mfma_f64_16x16x4_f64)"),
                         "fused_formation_and_factorization": fused,
                         "flops_per_launch": flops_form, "avg_launch_ms": form_ms},
            "phases_ms_per_step": {"form": form_ms, "form_is": "the fused worker launch (formation + factorization beside the chain)" if fused else "the formation kernel",
                                   "device_total": dev_ms / K, "note": "form and device_total from the timed region"},
            "whole_iteration": {"flops_per_iteration": flops_per_iteration(m, n),
                                "tflops": flops_per_iteration(m, n) * its_per_s / ngpu / 1e12,
                                "frac_of_fp64_mfma_peak": flops_per_iteration(m, n) * its_per_s / ngpu / 1e12 / PEAK_FP64_MFMA_TFLOPS},
            "objective_after_last_block": st["objective"],
        }
        if args.full:
            out["phases_ms_per_step"].update(
                factor=phases_all[1] / KB, trisolve=phases_all[2] / KB, other=phases_all[3] / KB,
                note="form and device_total from the timed region; the rest from an untimed pass"
                + (" on the SERIAL path (formation then factorization, what profiling level 2 runs): its form + factor is what the fused launch replaces" if fused else ""))
            # guard against a fast-but-wrong kernel variant: the objective after the first min(steps, 20)
            # iterations from the start point (its own untimed pass when the last timed block was a partial one) is compared
            # at the default size with the REFERENCE's own trajectory (tests/golden/dense_syn_4096x8192.npz, generated by
            # importing the reference); at other sizes with the same iterations under the one-level factorization
            # (IPM_TWO_LEVEL=0, no overlapped formation) on a second handle
            kchk = min(args.steps, RESET_EVERY)
            if args.steps % RESET_EVERY == 0:
                obj_chk = st["objective"]
            else:
                sv.set_profiling(0)
                sv.init_state(0.0)
                obj_chk = sv.iterate(kchk)["objective"]
            fx = os.path.join(ROOT, "tests", "golden", "dense_syn_%dx%d.npz" % (m, n))
            if os.path.exists(fx):
                ref_obj = float(np.load(fx)["objective_after_iteration"][kchk - 1])
                ok = abs(obj_chk - ref_obj) <= 1e-6 * max(1.0, abs(ref_obj))
                out["objective_check_against"] = "reference trajectory, iteration %d: %.12e" % (kchk, ref_obj)
            else:
                sv.close()
                saved = {k: os.environ.get(k) for k in ("IPM_TWO_LEVEL", "IPM_FUSED_FACTOR")}
                os.environ["IPM_TWO_LEVEL"] = "0"; os.environ["IPM_FUSED_FACTOR"] = "0"
                sv1 = ipm.IpmSolver(A, b, c, device=dev)
                sv1.init_state(0.0)
                ref_obj = sv1.iterate(kchk)["objective"]
                sv1.close()
                for k, v in saved.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
                ok = abs(obj_chk - ref_obj) <= 1e-9 * max(1.0, abs(ref_obj))
                out["objective_check_against"] = "same %d iterations with IPM_TWO_LEVEL=0 IPM_FUSED_FACTOR=0: %.12e" % (kchk, ref_obj)
            out["objective_check"] = "ok" if ok else "MISMATCH"
            out["objective_checked"] = obj_chk
            if not ok:
                print("bench: objective after %d iterations is %.12e, expected %.12e" % (kchk, obj_chk, ref_obj), file=sys.stderr)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(A, b, c)
            if (m, n) == (M_DEFAULT, N_DEFAULT):
                out["cpu_baseline_reference_algorithm"] = cpu_baseline_reference_algorithm(A, b, c)
        if args.full and world == 1 and not args.no_netlib and (m, n) == (M_DEFAULT, N_DEFAULT):
            # second half of the headline metric on the same GPU, eight LPs in flight (one stream each):
            #   netlib_all = the metric's own config, BASELINE.json configs[3]: ALL 73 valid benchmarks/ LPs (the loop of
            #                script.py:147-173 over the suite);
            #   netlib     = the 26-LP parity set (the files on which the reference itself converges).
            sv.close()
            from interiorpointmethod_amd import batch
            names, probs, flops = load_netlib("all")
            batch.solve_one(probs[names.index("AFIRO")], device=dev)         # warm-up
            cb_all = None if args.no_cpu_baseline else netlib_cpu_baseline(names, probs)
            for key, label in (("netlib_all", "all 73 valid LPs of benchmarks/ (BASELINE.json configs[3])"),
                               ("netlib", "26-LP parity set of benchmarks/")):
                if key == "netlib":
                    keep = [i for i, nm in enumerate(names) if nm in PARITY_SET]
                    names, probs, flops = [names[i] for i in keep], [probs[i] for i in keep], [flops[i] for i in keep]
                # three runs, the MEDIAN one reported (all walls listed): the suite is ~1.5 s of host threads + four launch chains, and
                # one run in fifteen was seen 40 % slower than its neighbours on an otherwise idle box
                runs = sorted((run_netlib(names, probs, flops, dev, workers=8) for _ in range(max(1, args.netlib_reps))), key=lambda r: r[1])
                rec, el = runs[len(runs) // 2]
                summ = batch.summarize(rec)
                mode = ("lockstep batches by size class" if batch.lockstep_wanted(probs, 1, 8, lockstep_mode()) else "8 LPs in flight on separate streams")
                out[key] = {"metric": "Netlib LPs/sec (%s, tol=1e-8, cap 300, %s)" % (label, mode),
                            "value": summ["converged"] / el, "unit": "LPs/s", "n_gpus": 1, "wall_seconds": el,
                            "wall_seconds_runs": [float(r[1]) for r in runs],
                            "summary": summ, "roofline": netlib_roofline(names, probs, flops, rec, el, 1),
                            "per_lp": per_lp_table(names, rec)}
                if cb_all is not None:
                    cb = dict(cb_all) if key == "netlib_all" else cpu_baseline_subset(cb_all, set(names))
                    # the same LPs on the GPU (their share of the run above; eight LPs were in flight, so this is an upper bound)
                    cb["gpu_seconds_same_sample"] = float(sum(r[7] for r in rec if names[int(r[0])] in cb["sample_names"]))
                    out[key]["cpu_baseline"] = cb
                out[key].update(makespan_fields(names, rec))
                if key == "netlib_all":
                    full_set = (names, probs, flops)
            if args.emulate_world > 1:       # (after both timed legs: right behind the ~4 s of the shard runs the 0.2-s parity leg was measured at 124 instead of 146-164 LPs/s)
                out["netlib_all"]["emulated_multi_gpu"] = emulated_multi_gpu(*full_set, dev, args.emulate_world)
        emit(out)
    sv.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
