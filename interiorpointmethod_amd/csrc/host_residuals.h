// host_residuals.h -- host side, unit 3: the products with A, the launch tables of the vector steps (one per step, expanded from the
// variant lists next to the kernels: a launch is a look-up by the handle's class) and the residual / stop-test launches.  Ahead of
// the factorization units because the factorization enqueues them on the residual stream under its chain-bound tail.
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

// The vector steps of the iteration: one TABLE per step, expanded here from the list below the step's kernels (vector_ops.h:
// X_VARIANTS, X_FLAGS), and one look-up per launch.  A row is a lockstep twin type -- launched or recorded by launch_twin<T>, its
// argument struct built from (h, corr) -- or a kernel without a twin, its arguments bound by type (StepSrc): through launch_untwinned,
// which cuts a recording, or launched directly where the step is never recorded (scaling, the start).  No kernel and no argument
// list of a class variant is named in the host units; a new variant is one row per step it changes.
struct StepRow {
    unsigned serves;                       // the set of classes (bits masked with the step's flags) the row serves
    const char* name;                      // the kernel, or the twin type
    int twin;                              // LsType / LsBndType of a twin row, else -1
    void (*launch)(ipm_handle* h, int corr, unsigned grid, unsigned threads, hipStream_t st);
};
template <int T> static void row_twin(ipm_handle* h, int corr, unsigned grid, unsigned, hipStream_t st) { launch_twin<T>(h, grid, LsArgs<T>(h, corr), st); }
template <class... P> static void launch_untwinned_bound(ipm_handle* h, void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st, const StepSrc& s) {
    launch_untwinned(h, kernel, grid, block, st, Pick<P, StepSrc>::of(s)...);
}
template <auto K> static void row_untwinned(ipm_handle* h, int corr, unsigned grid, unsigned threads, hipStream_t st) { launch_untwinned_bound(h, K, dim3(grid), dim3(threads), st, StepSrc{h, corr}); }
template <auto K> static void row_direct(ipm_handle* h, int corr, unsigned grid, unsigned threads, hipStream_t st) { launch_bound(K, dim3(grid), dim3(threads), st ? st : h->stream, StepSrc{h, corr}); }
struct StepTable { const StepRow* rows; int n; unsigned flags; };
// the row that serves a class (null: none -- only for a class that is not legal)
constexpr const StepRow* step_row(const StepTable& t, unsigned bits) {
    for (int i = 0; i < t.n; ++i) if (t.rows[i].serves & V_AT(bits & t.flags)) return &t.rows[i];
    return nullptr;
}
constexpr bool step_table_ok(const StepTable& t) {          // every legal class is served by exactly one row
    for (unsigned c = 0; c <= V_ALL; ++c) {
        int n = 0;
        for (int i = 0; i < t.n; ++i) n += (t.rows[i].serves >> (c & t.flags)) & 1u;
        if (variant_legal(c) && n != 1) return false;
    }
    return true;
}
#define ROW_TWIN(SERVES, T) {SERVES, #T, T, row_twin<T>},
#define ROW_UNTWINNED(SERVES, K) {SERVES, #K, -1, row_untwinned<K>},
#define ROW_DIRECT(SERVES, K) {SERVES, #K, -1, row_direct<K>},
#define STEP_TABLE(NAME, VARIANTS, FLAGS, ROW_U)                                              \
    static constexpr StepRow NAME##_ROWS[] = {VARIANTS(ROW_U, ROW_TWIN)};                     \
    static constexpr StepTable NAME = {NAME##_ROWS, (int)(sizeof NAME##_ROWS / sizeof(StepRow)), FLAGS}; \
    static_assert(step_table_ok(NAME), #NAME ": a legal class without a row, or with two")
STEP_TABLE(STEP_PREPARE, PREPARE_VARIANTS, PREPARE_FLAGS, ROW_UNTWINNED);
STEP_TABLE(STEP_STOP_TEST, STOP_TEST_VARIANTS, STOP_TEST_FLAGS, ROW_UNTWINNED);
STEP_TABLE(STEP_SCALING, SCALING_VARIANTS, SCALING_FLAGS, ROW_DIRECT);
STEP_TABLE(STEP_DIRECTION, DIRECTION_VARIANTS, DIRECTION_FLAGS, ROW_UNTWINNED);
STEP_TABLE(STEP_MU_AFF, MU_AFF_VARIANTS, MU_AFF_FLAGS, ROW_UNTWINNED);
STEP_TABLE(STEP_CORRECTOR_RHS, CORRECTOR_RHS_VARIANTS, CORRECTOR_RHS_FLAGS, ROW_UNTWINNED);
STEP_TABLE(STEP_UPDATE, UPDATE_VARIANTS, UPDATE_FLAGS, ROW_UNTWINNED);
STEP_TABLE(STEP_START_PRIMAL, START_PRIMAL_VARIANTS, START_FLAGS, ROW_DIRECT);
STEP_TABLE(STEP_START_DUAL, START_DUAL_VARIANTS, START_FLAGS, ROW_DIRECT);
STEP_TABLE(STEP_START_SHIFT, START_SHIFT_VARIANTS, START_FLAGS, ROW_DIRECT);
STEP_TABLE(STEP_START_PRIMAL_CORRECT, START_PRIMAL_CORRECT_VARIANTS, START_FLAGS, ROW_DIRECT);
STEP_TABLE(STEP_START_DUAL_CORRECT, START_DUAL_CORRECT_VARIANTS, START_FLAGS, ROW_DIRECT);
// the launch of a step on a handle: the vector steps run h->vblk blocks of VBLK threads, the stop test one block of 64
static void launch_step(const StepTable& t, ipm_handle* h, hipStream_t st = nullptr, int corr = 0, unsigned grid = 0, unsigned threads = VBLK) {
    step_row(t, variant_bits(step_variant(h)))->launch(h, corr, grid ? grid : (unsigned)h->vblk, threads, st);
}
static void launch_prepare(ipm_handle* h, hipStream_t st) { launch_step(STEP_PREPARE, h, st); }
static void launch_stop_test(ipm_handle* h, hipStream_t st) { launch_step(STEP_STOP_TEST, h, st, 0, 1u, 64u); }
static void launch_scaling(ipm_handle* h) { launch_step(STEP_SCALING, h); }
static void launch_direction(ipm_handle* h, int corr) { launch_step(STEP_DIRECTION, h, nullptr, corr); }
static void launch_mu_aff(ipm_handle* h) { launch_step(STEP_MU_AFF, h); }
static void launch_corrector_rhs(ipm_handle* h) { launch_step(STEP_CORRECTOR_RHS, h); }
static void launch_update(ipm_handle* h) { launch_step(STEP_UPDATE, h); }
// The three vector kernels of a centrality-corrector round (vector_ops.h: mcc_*).  No lockstep twins: ipm_set_centrality_correctors
// refuses a lockstep handle, and a program recorded with rounds pending would be cut like any other untwinned launch.  They take two
// VecArgs and two BndArgs views, so a type does not identify the argument: their plain / bounded forks are written out.
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

// r_b, r_c, d, predictor v, stop test (and, with IPM_FLAG_DETECT_INFEASIBILITY, the infeasibility tests): the one launch site of the
// stop test of every multi-kernel path (dense, sparse envelope, sparse factor, fused formation + factorization, lockstep)
static int enqueue_residuals(ipm_handle* h, hipStream_t st = nullptr) {
    if (int rc_ = check_class(h, "enqueue_residuals")) return rc_;
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
