// host_residuals.h -- host side, unit 3: the products with A and the residual / stop-test launches.  Ahead of the factorization
// units because the factorization enqueues them on the residual stream under its chain-bound tail.
#pragma once
static void launch_gemv_n(ipm_handle* h, const double* v, double sa, double sb, const double* add, double* out,
                          hipStream_t st = nullptr) {
    if (h->sparse) launch_twin<LS_SPMV_CSR>(h, (unsigned)((h->mp + 15) / 16), {sparse_view(h), (int)h->mp, v, sa, sb, add, out, solve_done(h)}, st);
    else launch_untwinned(h, gemv_n_kernel, dim3((unsigned)(h->mp / 4)), dim3(256), st, h->A, h->np, (int)h->mp, (int)h->np, v, sa, sb, add, out, solve_done(h));
}
// A^T u as partials [rc_chunks][np], into `part` (the handle's own, h->atp, unless the caller names another buffer of that shape)
static void launch_gemv_t(ipm_handle* h, const double* u, hipStream_t st = nullptr, double* part = nullptr) {
    if (!part) part = h->atp;
    if (h->sparse) launch_twin<LS_SPMV_CSC_T>(h, (unsigned)((h->np + 15) / 16), {sparse_view(h), (int)h->np, u, part, solve_done(h)}, st);
    else launch_untwinned(h, gemv_t_kernel, dim3((unsigned)((h->np + 511) / 512), (unsigned)h->rc_chunks), dim3(256), st, h->A, h->np, h->rows_per_chunk, (int)h->np, u, part, solve_done(h));
}
// The same pass (dense A) over the row chunks [chunk0, chunk1) only: gemv_t_kernel on the sub-range of A, u and the partials, so it
// writes exactly the partials the full launch writes for those chunks -- each chunk is one workgroup row's own sum, in the same
// order.  What cuts A^T dy into pieces that follow the backward sweep (host_iteration.h); never recorded.
static void launch_gemv_t_rows(ipm_handle* h, const double* u, int chunk0, int chunk1, hipStream_t st) {
    if (chunk1 <= chunk0) return;
    const int64_t r0 = (int64_t)chunk0 * h->rows_per_chunk;
    hipLaunchKernelGGL(gemv_t_kernel, dim3((unsigned)((h->np + 511) / 512), (unsigned)(chunk1 - chunk0)), dim3(256), 0, st ? st : h->stream,
                       h->A + r0 * h->np, h->np, h->rows_per_chunk, (int)h->np, u + r0, h->atp + (int64_t)chunk0 * h->np, &h->sc->done);
}

// The vector steps of the iteration, ONE launch function each: it holds the step's fork between the plain kernel, the detect
// kernel and their bounded forms.  All four have lockstep twins (T: the plain type, TB: its bounded twin, whose `single` is the
// *_bounded_kernel -- outside a recording a bounded handle enqueues what it always did; whether one may be recorded is ls_eligible's).
// A handle with a quadratic term (ipm_set_quadratic) runs the Quad instantiation of the four steps that have one (quad, quad_bounded:
// no twins -- a lockstep handle is refused the term); every other step is the LP's.
template <int T, int TB> static void launch_vec_step(ipm_handle* h, hipStream_t st = nullptr,
                                                     void (*quad)(VecArgs) = nullptr, void (*quad_bounded)(VecArgs, BndArgs) = nullptr) {
    if (h->quad && quad) {
        if (h->bnd) launch_untwinned(h, quad_bounded, dim3(h->vblk), dim3(VBLK), st, vec_args(h), bnd_args(h));
        else launch_untwinned(h, quad, dim3(h->vblk), dim3(VBLK), st, vec_args(h));
    } else if (h->bnd) launch_twin<TB>(h, (unsigned)h->vblk, {vec_args(h), 0, bnd_args(h)}, st);
    else launch_twin<T>(h, (unsigned)h->vblk, {vec_args(h), 0}, st);
}
// A handle with free columns (ipm_set_free_columns; it holds a quadratic term and is no lockstep handle: the setter and check_ready
// see to that) runs the Free instantiation of all seven steps.  An empty set enqueues what it always did.
// A detect handle reaches a quadratic term or free columns only with IPM_FLAG_DETECT_QUADRATIC (the setters): launch_prepare and
// launch_stop_test then pick the Detect instantiations of the Quad / Free kernels (quad_detect below), every other step is unchanged.
static bool free_step(ipm_handle* h, void (*plain)(VecArgs, FreeArgs), void (*bounded)(VecArgs, BndArgs, FreeArgs), hipStream_t st = nullptr, unsigned grid = 0) {
    if (!h->free_on) return false;
    const dim3 g(grid ? grid : (unsigned)h->vblk), b(grid ? 64 : VBLK);
    if (h->bnd) launch_untwinned(h, bounded, g, b, st, vec_args(h), bnd_args(h), free_args(h));
    else launch_untwinned(h, plain, g, b, st, vec_args(h), free_args(h));
    return true;
}
static bool quad_detect(const ipm_handle* h) { return h->detect && h->quad; }
static void launch_prepare(ipm_handle* h, hipStream_t st) {
    const double* g = h->quad_g;
    if (quad_detect(h)) {
        if (h->free_on && h->bnd) launch_untwinned(h, prepare_bounded_free_detect_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), bnd_args(h), g, free_args(h));
        else if (h->free_on) launch_untwinned(h, prepare_free_detect_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), g, free_args(h));
        else if (h->bnd) launch_untwinned(h, prepare_bounded_quad_detect_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), bnd_args(h), g);
        else launch_untwinned(h, prepare_quad_detect_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), g);
        return;
    }
    if (h->free_on && h->bnd) launch_untwinned(h, prepare_bounded_free_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), bnd_args(h), g, free_args(h));
    else if (h->free_on) launch_untwinned(h, prepare_free_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), g, free_args(h));
    else if (h->quad && h->bnd) launch_untwinned(h, prepare_bounded_quad_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), bnd_args(h), g);
    else if (h->quad) launch_untwinned(h, prepare_quad_kernel, dim3(h->vblk), dim3(VBLK), st, vec_args(h), g);
    else if (h->bnd && h->detect) launch_twin<LS_PREPARE_DETECT_BND>(h, (unsigned)h->vblk, {vec_args(h), bnd_args(h), det_args(h)}, st);
    else if (h->detect) launch_twin<LS_PREPARE_DETECT>(h, (unsigned)h->vblk, {vec_args(h), det_args(h)}, st);
    else launch_vec_step<LS_PREPARE, LS_PREPARE_BND>(h, st);
}
static void launch_stop_test(ipm_handle* h, hipStream_t st) {
    if (quad_detect(h)) {
        if (h->free_on && h->bnd) launch_untwinned(h, stop_test_bounded_free_detect_kernel, dim3(1u), dim3(64), st, vec_args(h), bnd_args(h), det_args(h), free_args(h));
        else if (h->free_on) launch_untwinned(h, stop_test_free_detect_kernel, dim3(1u), dim3(64), st, vec_args(h), det_args(h), free_args(h));
        else if (h->bnd) launch_untwinned(h, stop_test_bounded_quad_detect_kernel, dim3(1u), dim3(64), st, vec_args(h), bnd_args(h), det_args(h));
        else launch_untwinned(h, stop_test_quad_detect_kernel, dim3(1u), dim3(64), st, vec_args(h), det_args(h));
        return;
    }
    if (free_step(h, stop_test_free_kernel, stop_test_bounded_free_kernel, st, 1u)) return;
    if (h->bnd && h->detect) launch_twin<LS_STOP_TEST_DETECT_BND>(h, 1u, {vec_args(h), bnd_args(h), det_args(h)}, st);
    else if (h->bnd) launch_twin<LS_STOP_TEST_BND>(h, 1u, {vec_args(h), 0, bnd_args(h)}, st);
    else if (h->detect) launch_twin<LS_STOP_TEST_DETECT>(h, 1u, {vec_args(h), det_args(h)}, st);
    else launch_twin<LS_STOP_TEST>(h, 1u, {vec_args(h), 0}, st);
}
static void launch_scaling(ipm_handle* h) {      // (residual-stream iteration only, which is never recorded: no twin, nothing to refuse)
    const double* g = h->quad_g;
    if (h->free_on && h->bnd) hipLaunchKernelGGL(scaling_bounded_free_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, vec_args(h), bnd_args(h), g, free_args(h));
    else if (h->free_on) hipLaunchKernelGGL(scaling_free_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, vec_args(h), g, free_args(h));
    else if (h->quad && h->bnd) hipLaunchKernelGGL(scaling_bounded_quad_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, vec_args(h), bnd_args(h), g);
    else if (h->quad) hipLaunchKernelGGL(scaling_quad_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, vec_args(h), g);
    else if (h->bnd) hipLaunchKernelGGL(scaling_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, vec_args(h), bnd_args(h));
    else hipLaunchKernelGGL(scaling_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, vec_args(h));
}
static void launch_direction(ipm_handle* h, int corr) {
    if (h->free_on && h->bnd) launch_untwinned(h, direction_bounded_free_kernel, dim3(h->vblk), dim3(VBLK), nullptr, vec_args(h), corr, bnd_args(h), free_args(h));
    else if (h->free_on) launch_untwinned(h, direction_free_kernel, dim3(h->vblk), dim3(VBLK), nullptr, vec_args(h), corr, free_args(h));
    else if (h->bnd) launch_twin<LS_DIRECTION_BND>(h, (unsigned)h->vblk, {vec_args(h), corr, bnd_args(h)});
    else launch_twin<LS_DIRECTION>(h, (unsigned)h->vblk, {vec_args(h), corr});
}
// The three vector kernels of a centrality-corrector round (vector_ops.h: mcc_*).  No lockstep twins: ipm_set_centrality_correctors
// refuses a lockstep handle, and a program recorded with rounds pending would be cut like any other untwinned launch.
static void launch_mcc_target(ipm_handle* h, int first) {
    if (h->bnd) launch_untwinned(h, mcc_target_bounded_kernel, dim3(h->vblk), dim3(VBLK), nullptr, vec_args(h), mcc_vec_args(h), mcc_args(h, first), bnd_args(h), mcc_bnd_args(h));
    else launch_untwinned(h, mcc_target_kernel, dim3(h->vblk), dim3(VBLK), nullptr, vec_args(h), mcc_vec_args(h), mcc_args(h, first));
}
static void launch_mcc_direction(ipm_handle* h) {
    if (h->bnd) launch_untwinned(h, mcc_direction_bounded_kernel, dim3(h->vblk), dim3(VBLK), nullptr, mcc_vec_args(h), mcc_args(h, 0), mcc_bnd_args(h));
    else launch_untwinned(h, mcc_direction_kernel, dim3(h->vblk), dim3(VBLK), nullptr, mcc_vec_args(h), mcc_args(h, 0));
}
static void launch_mcc_accept(ipm_handle* h) {
    if (h->bnd) launch_untwinned(h, mcc_accept_bounded_kernel, dim3(h->vblk), dim3(VBLK), nullptr, vec_args(h), mcc_vec_args(h), mcc_args(h, 0), bnd_args(h), mcc_bnd_args(h));
    else launch_untwinned(h, mcc_accept_kernel, dim3(h->vblk), dim3(VBLK), nullptr, vec_args(h), mcc_vec_args(h), mcc_args(h, 0));
}
static void launch_mu_aff(ipm_handle* h) { if (!free_step(h, mu_aff_free_kernel, mu_aff_bounded_free_kernel)) launch_vec_step<LS_MU_AFF, LS_MU_AFF_BND>(h, nullptr, mu_aff_quad_kernel, mu_aff_bounded_quad_kernel); }
static void launch_corrector_rhs(ipm_handle* h) { if (!free_step(h, corrector_rhs_free_kernel, corrector_rhs_bounded_free_kernel)) launch_vec_step<LS_CORR_RHS, LS_CORR_RHS_BND>(h); }
static void launch_update(ipm_handle* h) { if (!free_step(h, update_free_kernel, update_bounded_free_kernel)) launch_vec_step<LS_UPDATE, LS_UPDATE_BND>(h, nullptr, update_quad_kernel, update_bounded_quad_kernel); }

// r_b, r_c, d, predictor v, stop test (and, with IPM_FLAG_DETECT_INFEASIBILITY, the infeasibility tests): the one launch site of the
// stop test of every multi-kernel path (dense, sparse envelope, sparse factor, fused formation + factorization, lockstep)
static int enqueue_residuals(ipm_handle* h, hipStream_t st = nullptr) {
    launch_gemv_n(h, h->x, 1.0, -1.0, h->b, h->rb, st);             // r_b = A x - b
    launch_gemv_t(h, h->y, st);                                     // A^T y (partials)
    launch_prepare(h, st);
    launch_stop_test(h, st);
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
// Is A^T dy streamed behind the backward sweeps (enqueue_normal_solve)?  Dense handles with a residual stream and grouped sweeps,
// on the fused and the serial factor path alike.  Its pieces sit behind device-polled gates, so the rule of every other polled
// hand-off holds: only while the handle polls and is alone on its device (polls_device; wants_polling is what may_poll takes the
// roll-back snapshot by), never after a recovered time-out (poll_fallback), never while a lockstep program is being recorded.
static bool stream_at_on(const ipm_handle* h) {
    return h->stream_at != 0 && overlap_residuals(h) && h->grouped_trsv && !h->sparse && polls_device(h) && !h->ls_rec;
}
