// host_residuals.h -- host side, unit 3: the products with A and the residual / stop-test launches.  Ahead of the factorization
// units because the factorization enqueues them on the residual stream under its chain-bound tail.
#pragma once
static void launch_gemv_n(ipm_handle* h, const double* v, double sa, double sb, const double* add, double* out,
                          hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    if (h->sparse) {
        const LsSpmv p{sparse_view(h), (int)h->mp, v, sa, sb, add, out, &h->sc->done};
        if (ls_push(h, LS_SPMV_CSR, (unsigned)((h->mp + 15) / 16), p)) return;
        hipLaunchKernelGGL(spmv_csr_kernel, dim3((unsigned)((h->mp + 15) / 16)), dim3(256), 0, st, sparse_view(h),
                           (int)h->mp, v, sa, sb, add, out, &h->sc->done);
        return;
    }
    hipLaunchKernelGGL(gemv_n_kernel, dim3((unsigned)(h->mp / 4)), dim3(256), 0, st, h->A, h->np, (int)h->mp,
                       (int)h->np, v, sa, sb, add, out, &h->sc->done);
}
static void launch_gemv_t(ipm_handle* h, const double* u, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    if (h->sparse) {
        const LsSpmvT p{sparse_view(h), (int)h->np, u, h->atp, &h->sc->done};
        if (ls_push(h, LS_SPMV_CSC_T, (unsigned)((h->np + 15) / 16), p)) return;
        hipLaunchKernelGGL(spmv_csc_t_kernel, dim3((unsigned)((h->np + 15) / 16)), dim3(256), 0, st, sparse_view(h),
                           (int)h->np, u, h->atp, &h->sc->done);
        return;
    }
    dim3 grid((unsigned)((h->np + 511) / 512), (unsigned)h->rc_chunks);
    hipLaunchKernelGGL(gemv_t_kernel, grid, dim3(256), 0, st, h->A, h->np, h->rows_per_chunk, (int)h->np, u,
                       h->atp, &h->sc->done);
}

// r_b, r_c, d, predictor v, stop test (and, with IPM_FLAG_DETECT_INFEASIBILITY, the infeasibility tests): the one launch site of the
// stop test of every multi-kernel path (dense, sparse envelope, sparse factor, fused formation + factorization, lockstep)
static int enqueue_residuals(ipm_handle* h, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    VecArgs a = vec_args(h);
    launch_gemv_n(h, h->x, 1.0, -1.0, h->b, h->rb, st);             // r_b = A x - b
    launch_gemv_t(h, h->y, st);                                     // A^T y (partials)
    if (h->bnd && h->detect) {
        hipLaunchKernelGGL(prepare_bounded_detect_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a, bnd_args(h));
        hipLaunchKernelGGL(stop_test_bounded_detect_kernel, dim3(1), dim3(64), 0, st, a, bnd_args(h), det_args(h));
    } else if (h->bnd) {                                            // (a bounded handle is never recorded: ls_eligible)
        hipLaunchKernelGGL(prepare_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a, bnd_args(h));
        hipLaunchKernelGGL(stop_test_bounded_kernel, dim3(1), dim3(64), 0, st, a, bnd_args(h));
    } else if (h->detect) {                                         // the infeasibility tests: their own lockstep twins
        const LsVecDet p{a, det_args(h)};
        if (!ls_push(h, LS_PREPARE_DETECT, (unsigned)h->vblk, p)) hipLaunchKernelGGL(prepare_detect_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a);
        if (!ls_push(h, LS_STOP_TEST_DETECT, 1u, p)) hipLaunchKernelGGL(stop_test_detect_kernel, dim3(1), dim3(64), 0, st, a, det_args(h));
    } else {
        if (!ls_push(h, LS_PREPARE, (unsigned)h->vblk, LsVecA{a, 0})) hipLaunchKernelGGL(prepare_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a);
        if (!ls_push(h, LS_STOP_TEST, 1u, LsVecA{a, 0})) hipLaunchKernelGGL(stop_test_kernel, dim3(1), dim3(64), 0, st, a);
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// Residual stream: everything of an iteration that needs (x, y, s) but not the factor -- r_b, r_c, the stop test and the
// predictor's right-hand side, three of the six passes over A -- runs on its own stream while the pivot chain of the
// factorization leaves most of the chip idle.  Called from inside enqueue_factor once the chain-bound tail begins (the
// head of the factorization is bound by its trailing updates, which these HBM passes would only slow down).
static int enqueue_residual_stream(ipm_handle* h, hipStream_t chain) {
    HIP_TRY(h, hipEventRecord(h->ev_mid, chain));
    HIP_TRY(h, hipStreamWaitEvent(h->stream3, h->ev_mid, 0));
    int rc = enqueue_residuals(h, h->stream3);
    if (rc) return rc;
    launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1, h->stream3);   // predictor rhs = -r_b - A (d*t)
    HIP_TRY(h, hipEventRecord(h->ev_res, h->stream3));
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}
static bool overlap_residuals(const ipm_handle* h) {
    return h->stream3 != nullptr && h->profiling < 2;          // (created for dense handles from 16 blocks on, ipm_create)
}
