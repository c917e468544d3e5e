/*
 * ipm_hip.h -- C ABI of libipm_hip.so: the MI355X (gfx950) Newton/KKT hot path of a
 * Mehrotra predictor-corrector interior-point LP solver.
 *
 * Drop-in boundary for payakorn/InteriorPointMethod.  The reference has no FFI;
 * its seams are plain Python calls.  Each entry point below names
 * the reference code it replaces (paths relative to the reference repo root):
 *
 *   solver seam     interior_sparse   main.py:760-815   /  interior  main.py:707-757
 *   direction seam  direction_predicted_sparse(method="normal")  main.py:197,221-229
 *                   direction_corrected_sparse                  main.py:247-269
 *   linear seam     solve_linear                                 main.py:176-182
 *
 * Conventions: plain pointers and sizes only (no torch types).  All arithmetic is
 * IEEE fp64.  Every function returns an int status (IPM_OK == 0, < 0 error) and
 * never throws or aborts.  Buffers passed in are owned by the caller; device
 * scratch lives in a workspace that is either supplied by the caller (a device
 * pointer, e.g. the data_ptr() of a torch.uint8 tensor) or hipMalloc'ed by the
 * library when the caller passes NULL.  A handle is bound to one HIP device and
 * one stream, is not thread-safe; handles on distinct devices are independent.
 */
#ifndef IPM_HIP_H
#define IPM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPM_ABI_VERSION 4

/* return codes */
enum {
    IPM_OK = 0,
    IPM_ERR_INVALID_ARG = -1,
    IPM_ERR_HIP = -2,          /* a HIP runtime call failed; see ipm_last_error() */
    IPM_ERR_NO_DEVICE = -3,
    IPM_ERR_WORKSPACE = -4,    /* caller workspace too small / misaligned */
    IPM_ERR_STATE = -5,        /* call order violated (e.g. solve before set_A) */
    IPM_ERR_INVALID_INPUT = -6, /* non-finite entries in A, b or c (8 Netlib files) */
    IPM_ERR_SINGULAR = -7      /* ipm_lu_solve / ipm_lu_factor: an exactly zero pivot (info > 0) */
};

/* solver status written to ipm_stats.status (reference semantics in comments) */
enum {
    IPM_STATUS_RUNNING = 0,    /* stop test still true                     main.py:780 */
    IPM_STATUS_CONVERGED = 1,  /* check_optimality() returned False        main.py:162-173 */
    IPM_STATUS_MAX_ITER = 2,   /* k reached the cap (5000/50000)           main.py:725,780 */
    IPM_STATUS_NAN = 3,        /* non-finite iterate / residual            main.py:1141-1148 */
    /* (4 is taken by an internal status of the fused small-LP kernel) */
    /* With IPM_FLAG_DETECT_INFEASIBILITY only (ipm_get_certificate gives the certificate): */
    IPM_STATUS_PRIMAL_INFEASIBLE = 5,  /* a Farkas ray y, z of the dual was found: the LP has no feasible point */
    IPM_STATUS_DUAL_INFEASIBLE = 6     /* a ray x of the primal was found: the LP is unbounded (if feasible) */
};

/* ipm_options.flags */
enum {
    /* The Cholesky look-ahead hands work between its two streams through device counters polled inside kernels.
     * That is only safe while the handle's streams own their hardware queues: when several handles are driven
     * concurrently on one GPU (more streams than hardware queues), a polling kernel can sit in front of its own
     * producer in a shared queue.  The library protects itself: it counts the live handles per device and uses
     * stream events whenever more than one exists, and a poll that still times out (bounded spin) is not an error --
     * the affected call is rolled back and repeated with events, and the handle keeps events from then on
     * (ipm_get_schedule reports it).  This flag forces events from the start (slower per step, never polls). */
    IPM_FLAG_NO_DEVICE_POLLING = 1,
    /* ipm_solve switches the 1e-14 Tikhonov shift on by itself when the FIRST factorization of a solve had to guard
     * more than 5 % of its pivots (A has that many dependent rows: the QAP family of Netlib, 9-16 %; no other Netlib
     * file exceeds 2.7 %) and restarts the solve from its start state; the guard alone stalls there.
     * Reported in ipm_stats.auto_regularized.  This flag keeps the shift off. */
    IPM_FLAG_NO_AUTO_REGULARIZE = 2,
    /* One stream per handle: the blocked Cholesky runs without its look-ahead on a second stream (10-25 % slower for
     * a solve that has the GPU to itself).  For SEVERAL handles driven concurrently on one GPU this is the faster
     * setting by far: the HIP runtime maps streams onto four hardware queues, a mid-size LP keeps only a few CUs busy,
     * and four single-stream solves overlap almost perfectly (4 x DEGEN3: 1.15x the time of one) where two-stream
     * handles share queues and serialise (2.4x).  The batched mode of the Python host sets it. */
    IPM_FLAG_SINGLE_STREAM = 4,
    /* Sparse handles only: factor A D^2 A^T with the multifrontal SPARSE Cholesky (csrc/sparse_chol.h) instead of the
     * blocked dense one.  What scipy's spsolve does for the reference (SuperLU: fill-reducing order, symbolic
     * analysis, supernodal numeric factor; main.py:180, :226).  ipm_set_A_csc then analyses the pattern of A A^T in the
     * row order it is given -- pass the rows in the order ipm_order_rows returns -- and every factorization, forward and
     * backward substitution is ONE launch that walks the elimination tree.  It pays when the factor stays sparse
     * (STOCFOR3: 2.2e5 entries, tree height 36, against a chain of 131 dense 128-row blocks); ipm_order_rows reports
     * the numbers to decide with.  ipm_set_A_csc fails with IPM_ERR_INVALID_ARG when the structures exceed its caps. */
    IPM_FLAG_SPARSE_FACTOR = 8,
    /* The handle is created for ipm_solve_batch (the LOCKSTEP batch: iteration k of several LPs in the same launches): implies
     * IPM_FLAG_SINGLE_STREAM | IPM_FLAG_NO_DEVICE_POLLING and block-step triangular solves, so that every launch of its iteration has
     * a batched twin.  Such a handle still works with every other entry point (ipm_solve included: same arithmetic, one LP).
     * Who may join a batch: a handle with IPM_FLAG_DETECT_INFEASIBILITY, and -- only with IPM_FLAG_LOCKSTEP_BOUNDS -- one with finite
     * upper bounds.  Refused on such a handle whatever else is set: a quadratic term, free columns, centrality correctors, refinement
     * rounds, dense columns (none has batched twins). */
    IPM_FLAG_LOCKSTEP = 16,
    /* Detect infeasible and unbounded LPs.  At every stop test whose convergence test says "continue" (never
     * under ipm_iterate) the iterate (x, y, s, w, z) is tested, with beta = b^T y - u_U^T z_U and gamma = -c^T x:
     *   primal infeasible (status 5): beta > 0 and max_j max((A^T y - z)_j, 0) <= eps_p * beta;
     *     certificate y / beta, z / beta:  A^T y^ - z^ <= eps_p, z^ >= 0, b^T y^ - u^T z^ = 1;
     *   dual infeasible (status 6): gamma > 0 and max(||A x||_inf, max_{j in U} x_j) <= eps_d * gamma;
     *     certificate x / gamma:  x^ >= 0, ||A x^||_inf <= eps_d, x^_U <= eps_d, c^T x^ = -1.
     * eps_p = eps_d = 1e-8 unless ipm_set_infeasibility_tol says otherwise.  The tests only read what the iteration computes
     * anyway (five extra reductions per stop test); they change no iterate, so a flagged solve follows the unflagged one bit for
     * bit until it stops.  They certify what the infeasible-start iteration runs towards and do not guarantee detection: an LP
     * whose iterate overflows before its ray is clean still ends in IPM_STATUS_NAN.  Without the flag the kernels are
     * exactly those of a build without this feature.  A flagged handle may join the lockstep batch, next to unflagged ones. */
    IPM_FLAG_DETECT_INFEASIBILITY = 32,
    /* A handle that qualifies for the fused small path (sparse A of at most 128 rows, a product list of at most 2^22 terms) keeps
     * that path when it holds a quadratic term (ipm_set_quadratic): the whole loop of the QP runs in one launch of one workgroup
     * (the Quad variants of the small kernel), and the handle may join ipm_solve_small_batch next to LP handles.
     * Off by default: the small loop and the multi-kernel path sum in different orders, so their iterates agree to rounding, not bit
     * for bit.  The flag alone changes nothing: a flagged handle without a term (never set, or cleared with NULL / all zeros) runs
     * the LP kernels, bit for bit what an unflagged handle runs, and a handle that does not qualify for the small path ignores the
     * flag.  It lifts no refusal: a term with IPM_FLAG_DETECT_INFEASIBILITY (without IPM_FLAG_DETECT_QUADRATIC) or IPM_FLAG_LOCKSTEP, centrality correctors, refinement
     * rounds and dense columns on the small path are refused as without it. */
    IPM_FLAG_SMALL_QUADRATIC = 64,
    /* Bit 7 (value 128).  With IPM_FLAG_LOCKSTEP (ipm_create refuses it alone): a handle that holds finite upper bounds
     * (ipm_set_bounds) may join the lockstep batch -- ipm_batch_add and ipm_solve_batch accept it, next to unbounded and detecting
     * handles.  Its eight bounded vector steps run as batched kernels of their own types (csrc/lockstep.h: LsBndType), each the body of
     * the single-LP bounded kernel, so a joined bounded handle computes what ipm_solve computes on it alone, bit for bit, (w, z), the
     * history and the roll-back of the automatic Tikhonov restart included.  An opt-in: without the flag a bounded lockstep handle is
     * refused by the batch as before.  The flag alone changes nothing: a flagged handle without a finite bound is an ordinary lockstep
     * handle, bit for bit.  It lifts no other refusal of IPM_FLAG_LOCKSTEP. */
    IPM_FLAG_LOCKSTEP_BOUNDS = IPM_FLAG_SMALL_QUADRATIC << 1,
    /* Bit 8 (value 256).  With IPM_FLAG_SMALL_QUADRATIC (ipm_create refuses it alone: a free column needs the term, and the term
     * reaches the fused small path only with that flag): a handle that qualifies for the fused small path keeps it when it holds
     * free columns (ipm_set_free_columns) -- the whole loop of a factor-model QP of m + k <= 128 rows runs in one launch of one
     * workgroup (the two Free variants of the small kernel), and the handle may join ipm_solve_small_batch next to
     * every other handle of that path.  Both call orders: ipm_set_free_columns on a handle already on the small path is accepted,
     * and ipm_set_A_csc on a handle that holds a set may choose the path.  Every rule of ipm_set_free_columns holds unchanged
     * (g_j > 0, no finite bound, one pair left, no detection), and so do the refusals of the small path (centrality correctors,
     * refinement rounds, dense columns) and of Mehrotra's start (ipm_init_state_mehrotra; ipm_init_small_batch_mehrotra names the
     * handle's index).  Off by default: the small loop and the multi-kernel path sum in different orders.  The flag alone changes
     * nothing: a flagged handle without a set (never given, or cleared) runs the Quad or LP kernels, bit for bit what a handle
     * with IPM_FLAG_SMALL_QUADRATIC alone runs. */
    IPM_FLAG_SMALL_FREE = IPM_FLAG_LOCKSTEP_BOUNDS << 1,
    /* Bit 9 (value 512).  With IPM_FLAG_DETECT_INFEASIBILITY (ipm_create refuses it alone, and together with IPM_FLAG_LOCKSTEP: the
     * kernels have no batched twins): ipm_set_quadratic and ipm_set_free_columns accept the detecting handle, and its stop test
     * runs the two tests restated for a quadratic problem (U the bounded columns, Phi the free ones, g the diagonal):
     *   primal infeasible (status 5): beta = b^T y - u_U^T z_U > 0 and
     *       max( max_{j not in Phi} (A^T y - z)_j+ , max_{j in Phi} |(A^T y)_j| ) <= eps_p * beta   (a free column needs equality);
     *     certificate y / beta, z / beta as above.
     *   dual infeasible (status 6): gamma = -c^T x > 0, the LINEAR part of the objective only, and
     *       max( ||A x||_inf , max_{j in U} x_j , max_j g_j |x_j| ) <= eps_d * gamma;
     *     certificate x / gamma:  x^_j >= 0 off Phi, ||A x^||_inf, x^_U and g o x^ <= eps_d, c^T x^ = -1: a ray that avoids the curvature.
     * With g = 0 and no free column both are the tests above exactly.  The iteration is unchanged (a flagged solve follows the
     * unflagged quadratic one bit for bit until it stops); the tolerances are ipm_set_infeasibility_tol's; statuses, ipm_get_certificate
     * and its record are those above.  On an equilibrated handle the tests act on the scaled problem and the record's violation is
     * the SCALED problem's; the vectors of the certificate leave in the caller's units.  Every path a quadratic handle has is served:
     * multi-kernel (dense, sparse, residual stream) and, with IPM_FLAG_SMALL_QUADRATIC / IPM_FLAG_SMALL_FREE, the one-workgroup kernel
     * and ipm_solve_small_batch.  Detection is not guaranteed (an iterate that overflows first still ends in IPM_STATUS_NAN), and
     * curvature on ONE column of a ray does not bound a problem whose recession cone holds other rays: the loop then finds one of
     * those.  Without the flag every refusal stays as it was; the flag lifts no other refusal (lockstep, centrality correctors on a
     * quadratic handle, Mehrotra's start with free columns). */
    IPM_FLAG_DETECT_QUADRATIC = IPM_FLAG_SMALL_FREE << 1
};

typedef struct ipm_handle ipm_handle;

typedef struct ipm_options {
    double eta;              /* step damping, reference constant 0.91        main.py:607 */
    double pivot_guard_eps;  /* pivot <= eps*max diag(B) -> pivot_guard_big   */
    double pivot_guard_big;  /* replacement pivot, default 1e64 */
    int32_t check_every;     /* iterations enqueued between host status reads (>=1) */
    int32_t flags;           /* IPM_FLAG_*; 0 = defaults */
    int64_t sparse_nnz;      /* > 0: handle keeps A sparse (CSR+CSC on the device, no dense image) with at
                                most this many nonzeros; only ipm_set_A_csc may then supply A */
    double regularize;       /* Tikhonov shift: factor B + regularize*max diag(B)*I (0 = off, the default;
                                1e-12 makes the rank-deficient QAP family converge) */
} ipm_options;

/* per-solve statistics; norms use the reference's scaling (main.py:170-171).  With upper bounds set (ipm_set_bounds) the
 * fields describe the bounded system: rp_norm = ||(A x - b, x_U + w - u_U)||_2, rd_norm = ||A^T y + s - z - c||_2,
 * gap = x^T s + w^T z, mu = gap / (n + |U|), b_norm = ||(b, u_U)||_2 -- the norms the stop test of the folded problem
 * (one row x_j + t_j = u_j per bound) sees. */
typedef struct ipm_stats {
    int32_t status;          /* IPM_STATUS_* */
    int32_t iterations;      /* k: completed predictor-corrector steps */
    int32_t pivots_fixed;    /* total Cholesky pivots replaced by the guard */
    int32_t auto_regularized; /* 1: ipm_solve switched the Tikhonov shift on (IPM_FLAG_NO_AUTO_REGULARIZE) */
    double objective;        /* c^T x                                        main.py:815 */
    double rp_norm;          /* ||Ax-b||_2 */
    double rd_norm;          /* ||A^T y + s - c||_2 */
    double gap;              /* x^T s */
    double b_norm, c_norm;   /* ||b||_2, ||c||_2 */
    double mu, mu_aff, sigma;            /* last iteration           main.py:588-601 */
    double alpha_aff_p, alpha_aff_d;     /* predictor ratio tests    main.py:305-322 */
    double alpha_p, alpha_d;             /* damped step lengths      main.py:604-626 */
    double solve_ms;         /* device time of the last ipm_solve/ipm_iterate (HIP events) */
    double objective_last_finite; /* last finite c^T x seen by the stop test: what new_interior_sparse returns
                                     when the iterate goes NaN (main.py:1227-1233) */
} ipm_stats;

/* One record per completed iteration (the reference prints such a line: main.py:808-809, :1186).  objective, norms
 * and gap describe the iterate the iteration STARTED from (they come from its stop test), the step data what it did. */
typedef struct ipm_iter_record {
    int32_t k;               /* 0-based iteration index */
    int32_t pivots_fixed;    /* cumulative guarded pivots after this iteration's factorization */
    double objective, rp_norm, rd_norm, gap, mu, sigma;
    double alpha_aff_p, alpha_aff_d, alpha_p, alpha_d;
} ipm_iter_record;
#define IPM_HISTORY_CAPACITY 1024   /* ring: the most recent records are kept */

/* ---- library ---------------------------------------------------------------------- */
int ipm_abi_version(void);
int ipm_device_count(int* count);
void ipm_default_options(ipm_options* opts);

/* ---- handle ----------------------------------------------------------------------- */
/* Bytes of device workspace a handle for an m x n problem needs. */
int ipm_workspace_bytes(int64_t m, int64_t n, size_t* bytes);
/* Same for a handle created with ipm_options.sparse_nnz = nnz (A kept sparse). */
int ipm_workspace_bytes_csc(int64_t m, int64_t n, int64_t nnz, size_t* bytes);
/* Same from the options the handle will be created with (sparse_nnz, flags): a sparse handle with IPM_FLAG_SPARSE_FACTOR
 * factors with the multifrontal sparse Cholesky (what SuperLU does inside scipy's spsolve, main.py:180 / :226 of the
 * reference) and needs no dense m x m normal matrix in its workspace -- 2.2 GB less at STOCFOR3 (16675 rows).  The dense
 * entry points (ipm_form_normal_matrix, ipm_get_factor, ipm_solve_linear) still work on such a handle: the library
 * allocates the dense buffer itself on their first use.  A workspace sized by the two functions above is always
 * large enough as well. */
int ipm_workspace_bytes_opts(int64_t m, int64_t n, const ipm_options* opts, size_t* bytes);

/* workspace == NULL: the library allocates (and frees in ipm_destroy).
 * stream == NULL: the library creates its own stream on `device`. */
int ipm_create(int device, int64_t m, int64_t n, const ipm_options* opts,
               void* workspace, size_t workspace_bytes, void* stream, ipm_handle** out);
int ipm_destroy(ipm_handle* h);
const char* ipm_last_error(const ipm_handle* h);   /* also valid with h == NULL */

/* ---- problem data (replaces the arguments of interior_sparse, main.py:760) -------- */
/* Row-major m x n fp64 matrix with leading dimension ld (elements). is_device: the
 * pointer is device memory on the handle's device (copied device-to-device). */
int ipm_set_A_dense(ipm_handle* h, const double* A, int64_t ld, int is_device);
/* CSC triplets as scipy.sparse.csc_matrix holds them (sparse_interior.py:215); host memory.
 * Duplicate entries are summed (scipy's constructor semantics).  On a sparse handle A stays sparse
 * (SpMV + sparse formation of A D^2 A^T); on a dense handle it is scattered into the dense image.
 * A sparse handle also derives the 128-row-block ENVELOPE of A A^T from the structure of A in the row order
 * given: blocks below it are structurally zero in B and stay zero in the factor, and the blocked Cholesky
 * and the triangular solves skip them (exact; environment IPM_ENVELOPE=0 disables).  The row order that makes
 * the envelope small is the caller's choice -- the Python host applies reverse Cuthill-McKee to the pattern of
 * A A^T when that pays (SuperLU behind the reference's spsolve reorders too, main.py:180). */
int ipm_set_A_csc(ipm_handle* h, const int32_t* colptr, const int32_t* rowind,
                  const double* val, int64_t nnz);
int ipm_set_bc(ipm_handle* h, const double* b, const double* c);        /* host, length m / n */

/* ---- iterate (x, y, s) ------------------------------------------------------------- */
int ipm_set_state(ipm_handle* h, const double* x, const double* y, const double* s);  /* host */
int ipm_get_state(ipm_handle* h, double* x, double* y, double* s);                    /* host */
/* x = s = 1, y = y0: sparse_interior.py:193-200 (y0=1) / main.py:287-302 (y0=0); with bounds set also w = z = 1 on U */
int ipm_init_state(ipm_handle* h, double y0);
/* Mehrotra's starting point (SIAM J. Optim. 2 (1992) 575-601, section 7) computed ON THE DEVICE from the handle's own A, b, c (and u):
 * x = A^T (A A^T)^-1 b and y = (A A^T)^-1 A c, s = c - A^T y, shifted into the positive orthant and balanced; with bounds set also
 * (w, z): w = u - x and the reduced cost split into s = max(r, 0), z = max(-r, 0) on U, (x, w) and (s, z) shifted together and
 * balanced with x.s + w.z.  Not the reference's start: an optional mode that changes the trajectory.  A A^T is
 * factored with the handle's current guard and `regularize` settings exactly as ipm_normal_solve(h, NULL, ...) does; *pivots_fixed
 * (may be NULL) = its guarded pivots, i.e. the dependent rows of A.  No host arithmetic, no host copy of A; one stream
 * synchronisation at the end (plus ipm_normal_solve's retry after a recovered poll time-out).  Degenerate data (x.s + w.z not finite
 * or not positive, or a non-positive sum) gives the reference's start x = s = 1, y = 1, w = z = 1 on U, decided on the device.  y is
 * in the handle's row order, as ipm_get_state returns it.  Works on every handle kind (dense, sparse on the envelope factor,
 * IPM_FLAG_SPARSE_FACTOR, IPM_FLAG_LOCKSTEP before ipm_batch_add, the fused small path), bounded or not, and leaves the handle as
 * ipm_init_state does (the iteration count and the history restart with the next solve).  IPM_ERR_INVALID_ARG for a NULL handle,
 * IPM_ERR_STATE without A or without (b, c). */
int ipm_init_state_mehrotra(ipm_handle* h, int32_t* pivots_fixed);

/* ---- native upper bounds 0 <= x <= u ------------------------------------------------- */
/* u: host array of length n, +inf where x_j has no upper bound; u == NULL (or all +inf) removes the bounds, and the
 * handle then runs exactly the unbounded code.  NaN or negative entries: IPM_ERR_INVALID_INPUT.  The bounded set U
 * gets an upper slack w (x + w = u) and its dual z inside the Newton system: the normal matrix keeps order m
 * (DESIGN.md 4-B).  Sets w = z = 1 on U.  The bound vectors are allocated by the library on first use and freed by
 * ipm_destroy; the workspace size does not change.  Invalidates a pending predictor.  A handle with bounds joins
 * the lockstep batch only when it was created with IPM_FLAG_LOCKSTEP_BOUNDS (then with the arithmetic of ipm_solve on it alone,
 * (w, z) included); without that flag ipm_batch_add / ipm_solve_batch refuse it with IPM_ERR_INVALID_ARG. */
int ipm_set_bounds(ipm_handle* h, const double* u);
/* (w, z): host arrays of length n; entries outside U are ignored on set and read back as 0.  IPM_ERR_STATE without bounds. */
int ipm_set_bound_state(ipm_handle* h, const double* w, const double* z);
int ipm_get_bound_state(ipm_handle* h, double* w, double* z);

/* ---- separable convex QP: min c^T x + 1/2 x^T diag(g) x, g >= 0 -------- */
/* g: host array of length n; the call needs only n, so it may come before ipm_set_A_*.  g == NULL (or all zeros) removes the term,
 * and the handle then runs exactly the LP code.  NaN, Inf or negative entries: IPM_ERR_INVALID_INPUT, and the handle keeps what it
 * held.  The normal matrix stays A Theta A^T with Theta = (S/X + Z/W + G)^-1, so every factorization path serves the handle: dense
 * (the fused launch included), sparse on the envelope factor and with IPM_FLAG_SPARSE_FACTOR, bounded or not, with
 * ipm_set_refinement and with a dense-column split.  The dual residual is A^T y + s - z - c - g o x, the objective in ipm_stats
 * and the history is c^T x + 1/2 x^T diag(g) x, the stop test is unchanged, and the iteration takes ONE step length: alpha_p ==
 * alpha_d and alpha_aff_p == alpha_aff_d (the minimum of the pair) in ipm_stats and the history.  The vector is allocated by the
 * library on first use and freed by ipm_destroy; the workspace size does not change.  Invalidates a pending predictor.
 * The fused small-LP path is off unless IPM_FLAG_SMALL_QUADRATIC: without the flag ipm_set_A_csc does not choose it for a handle
 * that holds a term, and a nonzero g on a handle already on that path is IPM_ERR_INVALID_ARG (set the term before A); with the
 * flag the handle keeps the path in either order of the two calls and runs the Quad variants of the small kernel while it holds a
 * term.  Clearing is always accepted.
 * Refused with IPM_ERR_INVALID_ARG and a reason in ipm_last_error, never dropped: a nonzero g on an IPM_FLAG_LOCKSTEP handle (no
 * batched twins), on an IPM_FLAG_DETECT_INFEASIBILITY handle without IPM_FLAG_DETECT_QUADRATIC (the LP's tests do not fit a QP; that
 * flag adds the ones that do) and on a handle with
 * ipm_set_centrality_correctors(k > 0) (their accept rule compares step pairs); ipm_set_centrality_correctors(k > 0) refuses a
 * handle that holds a term.  ipm_init_state_mehrotra runs on such a handle and IGNORES g (the LP's start).
 * Scaled handle (ipm_equilibrate): g enters as g C^2 and leaves as g' / C^2, exact; an entry the factors push out of the normal
 * fp64 range is IPM_ERR_INVALID_INPUT, here and in ipm_equilibrate, which rescales a g already set; ipm_set_A_* return it to the
 * caller's units as they do u. */
int ipm_set_quadratic(ipm_handle* h, const double* g);
/* g (length n, the caller's units; zeros when no term is set) and the number of its positive entries; either may be NULL. */
int ipm_get_quadratic(ipm_handle* h, double* g, int64_t* nonzeros);

/* ---- free columns with curvature: what Q = diag(g) + F F^T needs -------- */
/* idx: `count` distinct column indices 0 .. n-1; count == 0 or idx == NULL clears the set, and the handle then runs exactly the
 * code it ran before.  A free column j carries no sign constraint: no s_j (stored and returned as exactly 0), no bound, no
 * complementarity pair; it needs g_j > 0 (ipm_set_quadratic), and its scaling is the constant 1 / g_j, so the normal matrix stays
 * A Theta A^T and every factorization path serves the handle: dense (the fused launch included), sparse on the envelope factor and
 * with IPM_FLAG_SPARSE_FACTOR, bounded or not (bounds on the OTHER columns), with ipm_set_refinement, with ipm_equilibrate (the
 * marks are scale-free) and with a dense-column split.  mu, mu_aff and sigma count n - count (+ |U|) pairs; the ratio tests skip the
 * free columns; their dual residual (A^T y - c - g o x)_j counts in rd_norm.  The call needs only n and may come before or after
 * ipm_set_A_*, ipm_set_quadratic and ipm_set_bounds.  With the reformulation t = F^T x (rows [F^T -I], t free, g_t = 1) a handle
 * solves min c^T x + 1/2 x^T (diag(g) + F F^T) x.
 * State: ipm_init_state writes x = 1 and s = 0 on the free columns; ipm_set_state stores s = 0 there whatever is passed (x may
 * have any sign or be 0); ipm_get_state returns 0.  Setting or changing the set on a handle that holds a state zeroes s on the new
 * free columns.  After CLEARING the set the former free columns still hold s = 0, which the barrier iteration cannot start from:
 * set a state anew (ipm_init_state / ipm_set_state) before the next iteration.
 * Refused with IPM_ERR_INVALID_ARG and a reason in ipm_last_error, in either order of the calls involved, never dropped: an index
 * out of range or given twice; a column with g_j = 0 (here when the term is set, by ipm_set_quadratic when the set came first,
 * and by ipm_iterate / ipm_solve / ipm_newton_direction when no term ever came); ipm_set_quadratic clearing the term or zeroing g_j
 * on a free column; a finite u_j on a free column (here, or by ipm_set_bounds); every column free (no pair left: mu would be 0/0);
 * an IPM_FLAG_LOCKSTEP handle, an IPM_FLAG_DETECT_INFEASIBILITY handle without IPM_FLAG_DETECT_QUADRATIC; a handle on the fused small path, IPM_FLAG_SMALL_QUADRATIC
 * included (set the columns before A: ipm_set_A_csc then takes the multi-kernel path) -- unless the handle was created with
 * IPM_FLAG_SMALL_FREE, which keeps it on that path in either call order; ipm_init_state_mehrotra on a handle with
 * free columns (its least-squares start is not restated for them).  Centrality correctors are refused as for every quadratic
 * handle.  The marks are np bytes allocated by the library on first use and freed by ipm_destroy.  Invalidates a pending predictor. */
int ipm_set_free_columns(ipm_handle* h, const int32_t* idx, int32_t count);
/* The set in the caller's order: *count receives its size, idx (capacity cap; may be NULL with cap == 0) the first cap indices. */
int ipm_get_free_columns(ipm_handle* h, int32_t* idx, int32_t cap, int32_t* count);

/* ---- LP free columns: free variables of a linear program, served natively -------- */
/* idx: `count` distinct column indices 0 .. n-1; count == 0 or idx == NULL clears the set, and the handle then enqueues exactly
 * what it enqueued before.  An LP free column j carries no sign constraint and no quadratic term: no s_j (stored and returned as
 * exactly 0), no bound, no complementarity pair.  Its curvature is borrowed: proximal-point primal regularisation of the free block
 * only (Altman and Gondzio 1999) -- at every iteration the free block of the objective carries 1/2 rho |x - x^k|^2 centred at the
 * iterate, whose gradient there is zero, so the residuals, the objective and the stop test are the true LP's, and only the Newton
 * matrix sees rho, as Theta_j = 1 / rho on the column.  rho is one positive finite number per handle, applied in the units of the
 * problem the handle iterates on (the scaled problem on an equilibrated handle); rho <= 0 selects IPM_FREE_LP_RHO_DEFAULT, a rho
 * that is not finite is IPM_ERR_INVALID_ARG.  The iteration keeps the LP's two step lengths; mu, mu_aff and sigma count
 * n - count (+ |U|) pairs; the ratio tests skip the columns; their dual residual (A^T y - c)_j counts in rd_norm.
 * Served: bounds on the other columns, dense A (the fused launch and the residual stream included), the envelope factor and
 * IPM_FLAG_SPARSE_FACTOR, ipm_set_refinement, ipm_equilibrate, the dense-column split, check_every / run-ahead,
 * ipm_newton_direction, and ipm_init_state_mehrotra (x_j the least-squares value, unshifted and uncorrected; s_j = 0; no term in
 * any minimum or sum of the start).
 * State: as for ipm_set_free_columns (x = 1, s = 0 from ipm_init_state; s stored and returned as 0; setting the set zeroes s there;
 * after clearing, set a state anew).
 * Refused with IPM_ERR_INVALID_ARG and a reason in ipm_last_error, in either order of the calls involved, never dropped: an index
 * out of range or given twice; a finite u_j on a marked column (here, or by ipm_set_bounds); every column free; a handle with a
 * quadratic term or an ipm_set_free_columns set (and those two setters on a handle with this set); an IPM_FLAG_LOCKSTEP handle;
 * an IPM_FLAG_DETECT_INFEASIBILITY handle; centrality correctors k > 0 (here, or by ipm_set_centrality_correctors); a handle
 * already on the fused small path (set the columns before A: ipm_set_A_csc then takes the multi-kernel path).
 * The marks are np bytes allocated by the library on first use and freed by ipm_destroy.  Invalidates a pending predictor. */
#define IPM_FREE_LP_RHO_DEFAULT 1e-8
int ipm_set_free_lp_columns(ipm_handle* h, const int32_t* idx, int32_t count, double rho);
/* The set in the caller's order and its rho (either pointer may be NULL): *count receives the size, idx the first cap indices. */
int ipm_get_free_lp_columns(ipm_handle* h, int32_t* idx, int32_t cap, int32_t* count, double* rho);
/* Test hook: a column vector of the iteration as the device holds it after the last ipm_newton_direction / ipm_iterate, n entries
 * in the HANDLE's units (a scaled handle's are not unscaled): which = 0 r_c, 1 d (the diagonal of Theta), 2 v, 3 q. */
int ipm_debug_get_column_vector(ipm_handle* h, int32_t which, double* out);

/* ---- equilibration: power-of-two Ruiz row / column scaling -------------- */
/* Scale the handle's LP on the device to R A C, R b, C c, u / C with diagonal R, C whose entries are exact powers of two, so that
 * scaling and unscaling introduce no rounding at all.  Rule (csrc/equilibrate.h): simultaneous Ruiz passes on |A| in the infinity
 * norm; a row or column whose largest magnitude in the current scaled matrix is v = f 2^e, f in [0.5, 1), has its factor
 * multiplied by 2^(-floor(e / 2)); empty rows and columns keep factor 1.  A pass changes nothing exactly when every non-empty row
 * and column maximum lies in [0.5, 2), so max_passes (0 .. 1024) is a cap, not a tuning knob: the cap runs on the device without
 * host synchronisation, passes behind the fixed point are no-ops.  A and every value table derived from it are rewritten once.
 * Requires A; b, c and u may be set before or after.  Off unless called: an unscaled handle runs exactly the code it ran before.
 * info (may be NULL): {passes that changed a factor, log2(max / min) of the non-empty row maxima before scaling, the same after,
 * log2(max / min) of the non-empty column maxima after}.  max_passes = 0, or data already at the fixed point: the handle stays
 * unscaled (info is still written).  IPM_ERR_STATE without A or on an already scaled handle.  Preconditions: finite data, and no
 * nonzero entry of A, b, c, u that the factors push into the subnormal range or to overflow -- checked on the device:
 * IPM_ERR_INVALID_INPUT, and the handle stays unscaled.  b, c or u that enter an already scaled handle meet the same precondition
 * on the way in: ipm_set_bc / ipm_set_bounds return IPM_ERR_INVALID_INPUT and keep what the handle held.
 * ONE BOUNDARY RULE from then on: data entering a scaled handle is scaled on the way in, data leaving it is unscaled on the way
 * out, all of it exact.  In: ipm_set_bc (R b, C c) and ipm_set_bounds (u / C), which recompute the norms; ipm_set_state (x / C,
 * y / R, s C); ipm_set_bound_state (w / C, z C).  Out: ipm_get_state (C x', R y', s' / C), ipm_get_bound_state (C w', z' / C),
 * ipm_newton_direction (C dx', R dy', ds' / C), ipm_get_certificate (y by R, x by C, z by 1 / C: a certificate of the caller's LP).
 * Everything else acts on the SCALED problem: the stop test and the infeasibility tests, the history, rp / rd / gap / mu and the
 * norms in ipm_stats, ipm_init_state and ipm_init_state_mehrotra (x = s = 1 etc. of the scaled LP), and the seams
 * ipm_form_normal_matrix, ipm_normal_solve and ipm_get_factor (A means R A C there).  The objective c'^T x' equals c^T x.  The
 * iterate must be set or initialised after this call (w = z = 1 on the bounded set are kept).  The batches need nothing: a scaled
 * handle is a handle with different data, scaled and unscaled ones mix freely, the unscale happens in the getters.
 * ipm_set_A_dense / ipm_set_A_csc make the handle unscaled again (its bounds return to the caller's units; b and c must be set
 * again); an A they reject leaves the scaled handle as it was.  The factors are the library's own allocation, freed by ipm_destroy; ipm_workspace_bytes* do not change. */
int ipm_equilibrate(ipm_handle* h, int32_t max_passes, double info[4]);
/* The factors: r (length m, the handle's row order) and c (length n), each may be NULL; all ones on an unscaled handle. */
int ipm_get_scaling(ipm_handle* h, double* r, double* c);

/* ---- direction seam (main.py:197 / :247) ------------------------------------------- */
/* corrector == 0: predictor direction at the current state (forms and factors A D^2 A^T).
 * corrector == 1: corrector direction; requires a preceding predictor call at the same
 * state (reuses its factor and affine direction).  Outputs are host arrays (may be NULL).
 * With bounds set these are the bounded (dx, dy, ds); dw = -(x + w - u) - dx and dz = -(r4 + z dw) / w on U follow
 * from them (r4 = w z for the predictor, w z + dw_aff dz_aff - sigma mu for the corrector). */
int ipm_newton_direction(ipm_handle* h, int corrector, double* dx, double* dy, double* ds,
                         ipm_stats* stats);

/* ---- solver seam ------------------------------------------------------------------- */
/* Run exactly n_steps predictor-corrector iterations from the current state.  The stop
 * test is evaluated (stats) but not acted on: this is the benchmark entry point.  The iteration count (and the
 * history) restarts at 0 with the first call after ipm_set_state / ipm_init_state and continues over further calls.  The residuals and the stop test
 * are evaluated once more after the last step, so objective / norms / gap in `stats` describe the state
 * ipm_get_state returns (step lengths, mu_aff and sigma are those of the last step taken). */
int ipm_iterate(ipm_handle* h, int32_t n_steps, ipm_stats* stats);
/* Loop of interior_sparse: stop test first, then one iteration, until the test fails or
 * max_iter iterations were taken.  tol_p/tol_d/tol_gap = e1/e2/e3 of main.py:772-774. */
int ipm_solve(ipm_handle* h, double tol_p, double tol_d, double tol_gap, int32_t max_iter,
              ipm_stats* stats);
/* The LOCKSTEP BATCH of the batched-LP mode (the driver loop of script.py:147-173 over independent LPs, on one GPU): ipm_solve for n
 * handles AT ONCE, iteration k of all of them in the same launches (csrc/lockstep.h).  Every handle must have been created with
 * IPM_FLAG_LOCKSTEP on the same device, hold a sparse A of more than 128 rows on the dense-tile factor (not IPM_FLAG_SPARSE_FACTOR)
 * and have A, b, c and a state set.  Handles with IPM_FLAG_DETECT_INFEASIBILITY, handles with finite upper bounds (ipm_set_bounds;
 * only with IPM_FLAG_LOCKSTEP_BOUNDS, IPM_ERR_INVALID_ARG without) and plain ones may be mixed freely.  Same arguments and per-handle semantics as ipm_solve (stop test, iteration cap, automatic
 * Tikhonov shift); stats[i] (may be NULL) describes handle i, with solve_ms the device time of the whole batch.  The arithmetic
 * of a handle is exactly that of ipm_solve on it alone: bit-identical iterates, for a bounded handle (w, z) included.  Launched on the first handle's stream. */
int ipm_solve_batch(ipm_handle** handles, int32_t n, double tol_p, double tol_d, double tol_gap, int32_t max_iter, ipm_stats* stats);
/* The same batch, incrementally: handles may JOIN between two steps (a host thread finishes an LP's set-up while the batch is already
 * running) and the caller learns which ones finished after every step (and can tear them down while the batch runs on).
 * ipm_batch_add: the handle (requirements as above) starts its solve from its current state, *index = its position in the batch.
 * ipm_batch_step: opt.check_every iterations of every active handle in lockstep; the indices of the handles that finished in this
 * step go to finished[0 .. *n_finished), *n_active = handles still running (0: nothing left to do).  `cap` is the capacity of
 * `finished`: every finished handle is reported exactly once, and the indices that do not fit stay queued in the batch -- the
 * following calls return them first, at most `cap` per call and oldest first, before or next to the handles that finish in those
 * calls, also when *n_active has reached 0 (such a call launches nothing).  A caller with cap < the number of handles therefore
 * calls until *n_active == 0 AND *n_finished == 0.  ipm_batch_stats: the statistics
 * of a finished handle.  A batch owns one stream; it is not thread-safe; the handles stay owned by the caller and must outlive their
 * part in the batch (destroy a handle only after ipm_batch_step reported it finished, or after ipm_batch_destroy). */
typedef struct ipm_batch ipm_batch;
int ipm_batch_create(int device, void* stream, ipm_batch** out);   /* stream: a hipStream_t of the caller (kept alive until ipm_batch_destroy), or NULL: the batch creates its own */
int ipm_batch_destroy(ipm_batch* b);
const char* ipm_batch_last_error(const ipm_batch* b);
int ipm_batch_add(ipm_batch* b, ipm_handle* h, double tol_p, double tol_d, double tol_gap, int32_t max_iter, int32_t* index);
int ipm_batch_step(ipm_batch* b, int32_t* finished, int32_t cap, int32_t* n_finished, int32_t* n_active);
int ipm_batch_stats(ipm_batch* b, int32_t index, ipm_stats* stats);
/* The SMALL-LP BATCH: ipm_solve for n handles of the fused single-workgroup path (sparse A of at most 128 rows, csrc/small_lp.h) in
 * ONE launch per kernel variant, one workgroup per LP -- a few hundred or thousand small LPs (scenario sweeps, parametric right-hand
 * sides, the AFIRO class of Netlib) fill the GPU's compute units where a loop of ipm_solve keeps one of them busy.  Every handle must be
 * served by that path (ipm_get_schedule out[9] == 1), live on the same device, have A, b, c and a state set and profiling off
 * (IPM_ERR_STATE otherwise); handles with upper bounds (ipm_set_bounds), with IPM_FLAG_DETECT_INFEASIBILITY and plain ones may be mixed
 * freely in one call, and so may handles that hold a quadratic term on this path (IPM_FLAG_SMALL_QUADRATIC, bounded or not), with
 * free columns on top (IPM_FLAG_SMALL_FREE, bounded or not), each of those four also with IPM_FLAG_DETECT_QUADRATIC (twelve kernel variants in all).  IPM_ERR_INVALID_ARG, with the offending index in ipm_last_error(NULL), for a NULL handle, a handle that is not on
 * the small path, a handle on another device and the same handle twice (two workgroups would race on one state); n < 0 or handles ==
 * NULL with n > 0 likewise; n == 0 returns IPM_OK and touches no device.  stream: a hipStream_t ON THE HANDLES' DEVICE the launches go to
 * (the caller's to guarantee: a stream does not tell its device), NULL = the first handle's stream; the handles may own any streams -- the batch stream waits (stream events) for each distinct one before the launch,
 * and the call returns with everything complete.  Same arguments and per-handle semantics as ipm_solve: stop test first, iteration
 * cap, and the automatic Tikhonov shift -- the handles whose first factorization asks for it (and only they) are launched a second
 * time with it, so a call is at most two rounds, each with one host synchronisation however large n is.  Afterwards ipm_get_state,
 * ipm_get_bound_state, ipm_get_history and ipm_get_certificate work on each handle as after ipm_solve.  stats (may be NULL): n records,
 * stats[i] describes handle i, with solve_ms the device time of the whole batch (as ipm_solve_batch).  The workgroups never
 * communicate and an LP's arithmetic is that of ipm_solve on it alone: bit-identical iterates, whatever the order of the handles. */
int ipm_solve_small_batch(ipm_handle** handles, int32_t n, double tol_p, double tol_d, double tol_gap, int32_t max_iter, void* stream,
                          ipm_stats* stats);
/* ipm_init_state_mehrotra for n handles of the fused small-LP path in ONE launch per variant (plain / bounded), one workgroup per LP.
 * Arguments are checked exactly as by ipm_solve_small_batch (NULL handle, not on the small path, other device, the same handle twice:
 * IPM_ERR_INVALID_ARG; n == 0: IPM_OK, no device touched), except that no state is needed (IPM_ERR_STATE without A or (b, c)) and that a
 * handle with free columns is refused as by ipm_init_state_mehrotra (IPM_ERR_INVALID_ARG naming its index, nothing launched); `stream`
 * has the same meaning and the same event waits on the handles' own streams apply.  pivots_fixed (may be NULL): n counts,
 * pivots_fixed[i] is handle i's.  The workgroups never communicate: each handle's (x, y, s[, w, z]) is bit-identical to
 * ipm_init_state_mehrotra on it alone, whatever the order of the handles.  One host synchronisation however large n is. */
int ipm_init_small_batch_mehrotra(ipm_handle** handles, int32_t n, void* stream, int32_t* pivots_fixed);
/* Tolerances of the infeasibility tests (IPM_FLAG_DETECT_INFEASIBILITY), each in (0, 1); default 1e-8 / 1e-8.  Takes effect
 * with the next solve (for the lockstep batch: with the next ipm_batch_add). */
int ipm_set_infeasibility_tol(ipm_handle* h, double eps_p, double eps_d);
/* The certificate of the last solve, which must have ended in IPM_STATUS_PRIMAL_INFEASIBLE or IPM_STATUS_DUAL_INFEASIBLE
 * (IPM_ERR_STATE otherwise).  Host arrays, each may be NULL: y (length m, in the handle's row order) and z (length n, 0 outside
 * the bounded set) = (y, z) / beta for status 5, zeros for 6; x (length n) = x / gamma for status 6, zeros for 5.
 * info (may be NULL): {kind (5 / 6), normalisation (beta / gamma), measured violation of the normalised certificate
 * (max (A^T y^ - z^)_+, or max(||A x^||_inf, max x^_U)), iteration k of the detection}. */
int ipm_get_certificate(ipm_handle* h, double* y, double* z, double* x, double info[4]);
/* Per-iteration records of the last ipm_solve / ipm_iterate, oldest first: min(iterations, IPM_HISTORY_CAPACITY,
 * capacity) records are written to `out` (host) and their number to *count. */
int ipm_get_history(ipm_handle* h, ipm_iter_record* out, int32_t capacity, int32_t* count);
/* How the handle schedules its factorization (tests and diagnostics): out[0] = 128-row blocks, out[1] = group size
 * of the two-level Cholesky (1 = one-level), out[2] = 1 when the 1024-row grouped triangular solves are used,
 * out[3] = 1 while cross-stream hand-offs poll device counters (0: stream events), out[4] / out[5] = bulk trailing
 * updates of the last factorization that signalled a counter / recorded an event, out[6] = 1 when the tile envelope
 * of a sparse handle is exploited, out[7] = live handles on this device, out[8] = poll time-outs recovered so far,
 * out[9] = 1 when the fused single-workgroup small-LP path serves this handle, out[10] = 1 when the last iteration ran the
 * FUSED formation + factorization (one persistent launch beside the pivot chain; dense handles of 20 .. 40 blocks with
 * n <= 3 m that have the device to themselves), out[11] = 1 while a sparse-factor handle runs one launch per level of its panel tree
 * (shared device) instead of one launch per sweep.  (ABI 4: twelve words; ABI 3 had ten.) */
int ipm_get_schedule(ipm_handle* h, int32_t out[12]);
/* The same record for callers that know about words added since (additive: ipm_get_schedule keeps its twelve): the first
 * min(capacity, 14) words are written, *count (optional) receives the number.  out[12] = 1 while A^T dy of the predictor and
 * the corrector is streamed behind the backward sweeps of the grouped solves (dense handles with a residual stream that poll the
 * device; IPM_STREAM_AT=0 and a recovered poll time-out switch it off).  out[13] = 128-row blocks per group of the grouped
 * triangular solves (8, 4 or 2; floor(blocks / out[13]) groups have explicit inverses), 0 without them. */
int ipm_get_schedule_words(ipm_handle* h, int32_t* out, int32_t capacity, int32_t* count);

/* Fill-reducing order of the ROWS of an m x n sparse A (CSC, host) for the Cholesky of A D^2 A^T: minimum degree on
 * the pattern of A A^T followed by the elimination-tree postorder.  Pure host code (no device is touched): the
 * reference gets the same service from SuperLU's COLAMD inside spsolve (main.py:180).  perm[new] = old, length m.
 * info (may be NULL, 8 doubles): [0] entries of the strict lower triangle of A A^T, [1] entries of the Cholesky factor in
 * this order (diagonal included), [2] multiply-adds of that factorization (sum over columns of count^2), [3] height of the
 * elimination tree in columns; of the panel tree the device would walk (the analysis ipm_set_A_csc runs): [4] its height in
 * panels, [5] the largest sum of (front rows)^2 along a root-to-leaf path, [6] panels, [7] rows of the widest front
 * ([4..7] zero when that analysis exceeds its caps).  Returns IPM_OK; IPM_ERR_WORKSPACE when the pattern or the ordering work exceeds the
 * built-in caps (A A^T close to dense: keep the dense path), perm is then the identity.
 * info[0] ON INPUT, honoured only together with info[1] = -1.0 (so that an uninitialised array cannot switch it on): the
 * milliseconds per iteration the caller expects from its alternative, the dense-tile path.  The elimination then gives up early (IPM_ERR_WORKSPACE) once a pivot's degree shows that the sparse factor cannot
 * beat that, and works within a budget scaled to it -- a caller that only wants the order when it pays (factor "auto" of the
 * Python host) saves 40 % of the host time the hopeless cases cost. */
int ipm_order_rows(int64_t m, int64_t n, const int32_t* colptr, const int32_t* rowind, int32_t* perm, double info[8]);
/* Structure of the sparse factor of a handle created with IPM_FLAG_SPARSE_FACTOR (IPM_ERR_STATE otherwise):
 * out[0] panels, [1] tasks, [2] panel-tree height, [3] widest front (rows), [4] entries of L stored, [5] entries of the
 * update matrices, [6] product-list terms of the formation, [7] launches that fell back to one workgroup after a
 * hand-off time-out. */
int ipm_get_factor_info(ipm_handle* h, int64_t out[8]);

/* ---- linear-solve seam (main.py:176-182) and kernel-level entry points ------------- */
/* Solve B z = rhs for a dense SYMMETRIC POSITIVE (SEMI)DEFINITE m x m host matrix by the blocked guarded Cholesky
 * (m = the handle's m; only the lower triangle is read).  The reference's solve_linear takes any square matrix
 * (LU); this seam is the normal-equations one, where the matrix is A D^2 A^T -- a general matrix is not accepted.
 * z may alias rhs.  pivots_fixed may be NULL. */
int ipm_solve_linear(ipm_handle* h, const double* B, int64_t ldb, const double* rhs, double* z,
                     int32_t* pivots_fixed);
/* The GENERAL-matrix seam (ipm_solve_linear above stays the SPD one): solve A X = B for any square n x n A by LU with partial
 * pivoting on the device (csrc/getrf_f64.h; LAPACK gesv, what the reference's np.linalg.solve does, main.py:178).  This is how the
 * reference's unreduced KKT system [[0, A^T, I], [A, 0, 0], [S, 0, X]] (main.py:13-21, zero diagonal block) is solved.  No handle:
 * the call allocates its own device memory and stream on `device` and frees both before it returns.  A (lda >= n), B and X
 * (nrhs columns, ldb / ldx >= nrhs) are row-major HOST arrays; X may alias B.  *info: 0, or j + 1 for the first exactly zero pivot
 * U[j][j] (then IPM_ERR_SINGULAR and X is not written).  NaN / Inf in A or B: IPM_ERR_INVALID_INPUT; bad sizes or leading
 * dimensions: IPM_ERR_INVALID_ARG; device memory not available: IPM_ERR_WORKSPACE.  Bitwise repeatable. */
int ipm_lu_solve(int device, int64_t n, const double* A, int64_t lda, int64_t nrhs, const double* B, int64_t ldb,
                 double* X, int64_t ldx, int64_t* info);
/* The factorization alone: P A = L U with the packed factors (unit L below the diagonal, U on and above it) written to host LU
 * (ldlu >= n) and the interchanges to ipiv (0-based: row i was swapped with row ipiv[i], in order; scipy.linalg.lu_factor's
 * convention).  info and errors as ipm_lu_solve; with IPM_ERR_SINGULAR the factors are still written. */
int ipm_lu_factor(int device, int64_t n, const double* A, int64_t lda, double* LU, int64_t ldlu, int32_t* ipiv,
                  int64_t* info);
/* Solve (A diag(d) A^T) z = rhs with the handle's own A: forms the normal matrix on the device (d on the host,
 * length n; NULL = all ones), factors it with the guarded blocked Cholesky (reuse_factor != 0: the factor of the
 * previous ipm_normal_solve / direction call is kept) and back-substitutes.  rhs, z: host, length m; z may alias
 * rhs.  Building block of start-point heuristics (x = A^T (A A^T)^-1 b, ...); the iterate is not touched. */
int ipm_normal_solve(ipm_handle* h, const double* d, const double* rhs, double* z, int reuse_factor,
                     int32_t* pivots_fixed);
/* Gondzio's multiple centrality correctors (Comput. Optim. Appl. 6 (1996) 137-156).  After Mehrotra's corrector
 * an iteration re-uses its factorization for up to k further rounds; a round is kept when it lengthens the step, and the first
 * rejected round ends the rounds of its iteration.  Off (k = 0) by default: the handle then runs exactly the iteration it ran
 * without this call.  k = 0 .. IPM_MAX_CORRECTORS, taking effect with the next iteration of ipm_solve / ipm_iterate
 * (ipm_newton_direction keeps returning Mehrotra's two directions).  IPM_ERR_INVALID_ARG, with the reason in ipm_last_error, for a NULL
 * handle or k out of range (both checked first, no device is touched), and with k > 0 for a handle on the fused small path (schedule
 * word 9: one workgroup holds the whole loop) and for a handle created with IPM_FLAG_LOCKSTEP (the rounds have no batched twins;
 * k = 0 is accepted on every handle).  A handle that ipm_set_A_csc puts on the small path AFTER k > 0 was set keeps k, and ipm_solve /
 * ipm_iterate / ipm_solve_small_batch refuse it (IPM_ERR_INVALID_ARG) until k is set to 0: the option is never dropped.  The
 * candidate vectors are the library's own allocation, made on first use and kept; the workspace sizes do not change.  With k = 0 the
 * library enqueues exactly what it enqueued before this call existed, also on a handle that ran with k > 0 earlier. */
#define IPM_MAX_CORRECTORS 8
int ipm_set_centrality_correctors(ipm_handle* h, int32_t k);
/* out = {k, rounds that did work, rounds accepted, iterations with at least one accepted round} of the last ipm_solve / ipm_iterate
 * sequence (the counts restart where the iteration count restarts). */
int ipm_get_corrector_info(ipm_handle* h, int64_t out[4]);
/* Iterative refinement of the normal-equations solves.  Every solve dy = B~^-1 t of the iteration (predictor,
 * corrector, centrality-corrector rounds) and of ipm_normal_solve uses the FACTORED matrix B~: guarded pivots, the Tikhonov shift and
 * the rounding of the Cholesky are in it.  With k > 0 up to k rounds follow each such solve on the device: r = t - A D^2 A^T dy from
 * the handle's own passes over A, rho = ||r||_2, then dy += B~^-1 r with the same factor.  The rounds of a solve end when rho is 0
 * or not finite, when rho did not halve against the round before (that correction stays), or when rho grew (that correction is
 * undone and counted as a revert).  The correction of the last round goes unverified: no residual is taken behind it.  The
 * decision lives on the device, the host does not synchronise, and the result does not depend on check_every.  D^2 is the handle's
 * current scaling vector (theta with bounds; the d of ipm_normal_solve, or with reuse_factor the one the handle holds).
 * ipm_init_state_mehrotra is not refined.  Off (k = 0) by default: the library then enqueues exactly what it enqueued before this call
 * existed, also on a handle that ran with k > 0 earlier.  k = 0 .. IPM_MAX_REFINE.  IPM_ERR_INVALID_ARG, with the reason in
 * ipm_last_error, for a NULL handle or k out of range (both checked first, no device is touched), and with k > 0 for a handle on the
 * fused small path and for a handle created with IPM_FLAG_LOCKSTEP (k = 0 is accepted on every handle).  A handle that goes onto the small path after k > 0 was set is refused by
 * ipm_solve / ipm_iterate / ipm_newton_direction / ipm_normal_solve until k is set to 0: the option is never dropped.  The vectors of
 * the rounds are the library's own allocation, made on first use and kept; the workspace sizes do not change. */
#define IPM_MAX_REFINE 4
int ipm_set_refinement(ipm_handle* h, int32_t k);
/* out = {k, solves refined, corrections applied, rounds ended because rho did not halve, reverts, rho_1/||t|| and the last kept
 * rho/||t|| of the most recent solve, the largest rho_1/||t||} of the last ipm_solve / ipm_iterate sequence (the counts restart where the
 * iteration count restarts), or of the last ipm_normal_solve or ipm_newton_direction call (each call's one solve: the counts restart
 * with it). */
int ipm_get_refinement_info(ipm_handle* h, double out[8]);
/* Test hook: one of the m-vectors of the last refined solve WITH its padding, to host `out`.  *count = padded length (rows
 * m .. *count - 1 are padding: zero); nothing is copied when out is NULL or capacity < *count.  which: 0 the kept right-hand side
 * t, 1 the residual r, 2 the correction delta (IPM_ERR_STATE on a handle that never ran a round), 3 the handle's dy (corrector,
 * ipm_normal_solve), 4 its predictor dy (tests/test_gpu_refine.py). */
int ipm_debug_get_refine_vector(ipm_handle* h, int32_t which, double* out, int64_t capacity, int64_t* count);
/* Dense columns split out of the sparse factor.  A column of A with many entries puts a full clique into A A^T and
 * the sparse factor fills up.  With the set DC of such columns named here (count <= IPM_MAX_DENSE_COLS distinct indices 0 .. n-1, in
 * any order), the NEXT ipm_set_A_csc builds the symbolic analysis, the product list of the formation and the sparse factor from A
 * without them, B_s = A_s D A_s^T = L L^T (pivot guard and Tikhonov shift apply to B_s as they do to B without a split), and every
 * factorization is followed by V = A_DC diag(sqrt(d_DC)), W = L^-1 V (one batched walk of the panel tree) and the Cholesky factor R
 * of S = I + W^T W; every solve B^-1 t then runs z = L^-1 t, z -= W S^-1 W^T z, L^-T z (Sherman-Morrison-Woodbury), for every caller
 * of a solve: the iteration with its corrector, centrality-corrector and refinement rounds, ipm_normal_solve, ipm_init_state_mehrotra,
 * bounded and infeasibility-detecting handles.  Products with A, residuals, A^T dy and the refinement residual keep the full A, which
 * is what stabilises the split: the bare formulas lose every digit of a whole solve near the optimum, where the rows that only basic
 * dense columns support leave B_s nearly singular.  So the library factors B_s + 1e-10 diag(V V^T) and runs at least two refinement
 * rounds (ipm_set_refinement's, against the full A D A^T) behind every refined solve of a split handle; ipm_set_refinement(h, k < 2)
 * on such a handle sets 2, and ipm_get_refinement_info reports it.  count = 0 clears the set (cols may be
 * NULL): the next ipm_set_A_csc builds the handle exactly as without this call.  A set given after ipm_set_A_csc waits for the next one.
 * IPM_ERR_INVALID_ARG, with the reason in ipm_last_error and the set the handle held kept, for: a NULL handle, count < 0 or
 * count > IPM_MAX_DENSE_COLS, and with count > 0 a handle without IPM_FLAG_SPARSE_FACTOR (or without sparse_nnz), a handle of
 * m <= 128 rows (the fused small path), a handle created with IPM_FLAG_LOCKSTEP, an index out of range or given twice.  A set whose
 * removal leaves a row of A empty is refused by ipm_set_A_csc (IPM_ERR_INVALID_ARG; the handle keeps the A it had).  Buffers are the
 * library's own allocation; the workspace sizes do not change.  Results are bitwise repeatable and do not depend on IPM_SP_MODE,
 * IPM_SP_GRID or IPM_SP_FUSE_FWD. */
#define IPM_MAX_DENSE_COLS 64
int ipm_set_dense_columns(ipm_handle* h, int32_t count, const int32_t* cols);
/* out[0] k, the dense columns of the split in place (0: none, and every other word is 0), [1] k padded to a multiple of 16, [2] row
 * chunks of the Gram and correction kernels, [3] entries of L stored with the split, [4] the same without it when known (the library
 * orders one of the two: 0; the Python host fills it in when it ordered both), [5] factorizations that built W and R, [6] corrections
 * applied, both since ipm_set_A_csc, [7] 0. */
int ipm_get_dense_split_info(ipm_handle* h, int64_t out[8]);
/* Test hook of the split (IPM_ERR_STATE without one): which = 0 V, 1 W (m x k, column-major, the handle's row order), 2 R (k x k,
 * row-major, zeros above the diagonal), 3 the column list (k values), as left by the last factorization; 4: L^-1 V computed again
 * by this call, one column at a time with the stock forward sweep of the sparse factor (what W must equal bit for bit).  *count = the number of
 * doubles; nothing is copied when out is NULL or capacity < *count (tests/test_gpu_dense_split.py). */
int ipm_debug_get_dense_split(ipm_handle* h, int32_t which, double* out, int64_t capacity, int64_t* count);
/* B = A diag(d) A^T (d on the host, length n); full symmetric m x m written to host B -- the FULL B also on a handle with a
 * dense-column split. */
int ipm_form_normal_matrix(ipm_handle* h, const double* d, double* B, int64_t ldb);
/* Cholesky factor of the handle's current normal matrix; lower triangle to host L.  On a handle with a dense-column split
 * (ipm_set_dense_columns) this is the factor of B_s + 1e-10 diag(V V^T), B_s = A_s D A_s^T the matrix without the dense columns, not of B. */
int ipm_get_factor(ipm_handle* h, double* L, int64_t ldl);
/* Timing of the device phases of the last ipm_iterate call, milliseconds per iteration:
 * out[0]=form A D^2 A^T, out[1]=factor, out[2]=triangular solves, out[3]=everything else.
 * enable = 1: only out[0] (two event records per iteration around the dominant kernel); enable = 2: all four
 * (nine records per iteration, ~1 % slower); 0: off. */
int ipm_set_profiling(ipm_handle* h, int enable);
/* Diagnostic builds only (environment IPM_POTRF_STAMPS=1 at ipm_create): s_memtime stamps of the first
 * diagonal-block factorization, 8 waves x 64 slots.  IPM_ERR_STATE otherwise. */
int ipm_debug_get_stamps(ipm_handle* h, long long* out);
/* Host only (no device is touched; tests): the ordered work list of the fused formation + factorization for `nblk` 128-row
 * blocks, `q` formation chunks per tile and `workers` workgroups (csrc/ff_schedule.h).  Up to `capacity` items of 8 bytes
 * {type, i, c, q, j0, j1, flags, seq} are written to `items`, their number to *count, the number of update items per lower
 * tile (row-major triangle, nblk (nblk + 1) / 2 entries) to tile_items, and the simulated {end of the factorization, end
 * of the formation} in microseconds to sim_us. */
/* Host only: the pieces A^T dy is cut into behind a backward sweep (csrc/host_factor_solve.h, at_piece_schedule) for a dense
 * handle of `nblk` 128-row blocks.  layout = {mp, gsz, rc_chunks, rows_per_chunk}; an entry that is 0 on input is replaced by what
 * ipm_create chooses for that block count.  One triple per sweep event, in sweep order: {first final row, chunk0, chunk1}; the
 * first min(capacity, events) triples are written, *count = events.  The last triple is the piece the main stream runs. */
int ipm_debug_at_pieces(int32_t nblk, int32_t layout[4], int32_t* pieces, int32_t capacity, int32_t* count);
/* Host only: the step plan of the dense blocked Cholesky (csrc/chol_plan.h, chol_step_plan) of a handle of `nblk` 128-row blocks and m
 * rows (m <= 0: all of them).  knobs = {look-ahead switch, device polling, two_level, group_steps, ss_small_blocks, shift in effect} as
 * the handle holds them (look-ahead still needs more than two blocks); env_last: the tile envelope (nblk entries) or NULL.
 * totals = {look-ahead, polling, group size, counter steps, event steps}; steps (capacity in records, written when >= nblk) receives one
 * record of IPM_CHOL_STEP_WORDS words per block step: {potrf panels, rows, rem, shape (0 narrow, 1 wide, 2 look-ahead), g0, gend, kcols,
 * window, crit_wait (0 none, 1 counter, 2 event), crit_count, crit_flag, poll_count, bulk (0 none, 1 counter, 2 event), bulk_count,
 * bulk_event}. */
#define IPM_CHOL_STEP_WORDS 15
int ipm_debug_chol_plan(int32_t nblk, int64_t m, const int32_t knobs[6], const int32_t* env_last, int32_t totals[5], int32_t* steps,
                        int32_t capacity);
/* Host only: the kernel that serves a problem class at a step, read from the library's variant tables (csrc/vector_ops.h,
 * csrc/small_lp.h; the class: bounded = ipm_set_bounds, detect = IPM_FLAG_DETECT_INFEASIBILITY, quad = ipm_set_quadratic, free_cols =
 * ipm_set_free_columns).  name_out (capacity bytes) receives the row's name: the kernel, or for a step that has a lockstep twin at
 * that class the twin's type (LS_*), whose id goes to *twin_type_out (-1: no twin).  For the IPM_STEP_SMALL* steps *twin_type_out is
 * the row's id instead: the variant (SMALL_*) or, for the two start steps, 0 plain / 1 bounded.  IPM_ERR_INVALID_ARG for free columns
 * without a quadratic term, which is no class. */
enum {
    IPM_STEP_PREPARE = 0, IPM_STEP_STOP_TEST, IPM_STEP_SCALING, IPM_STEP_DIRECTION, IPM_STEP_MU_AFF, IPM_STEP_CORRECTOR_RHS, IPM_STEP_UPDATE,
    IPM_STEP_SMALL, IPM_STEP_SMALL_BATCH, IPM_STEP_SMALL_START, IPM_STEP_SMALL_START_BATCH,
    IPM_STEP_START_PRIMAL, IPM_STEP_START_DUAL, IPM_STEP_START_SHIFT, IPM_STEP_START_PRIMAL_CORRECT, IPM_STEP_START_DUAL_CORRECT, IPM_STEP_COUNT
};
int ipm_debug_step_kernel(int32_t step, int32_t bounded, int32_t detect, int32_t quad, int32_t free_cols, char* name_out, int32_t capacity,
                          int32_t* twin_type_out);
/* The same with the fifth switch, free_lp = ipm_set_free_lp_columns: legal only without detect, quad and free_cols, and served by the
 * multi-kernel steps only (IPM_ERR_INVALID_ARG otherwise, the IPM_STEP_SMALL* steps included).  With free_lp = 0 it answers as
 * ipm_debug_step_kernel does. */
int ipm_debug_step_kernel_ex(int32_t step, int32_t bounded, int32_t detect, int32_t quad, int32_t free_cols, int32_t free_lp, char* name_out,
                             int32_t capacity, int32_t* twin_type_out);
/* Host only: the library's option-compatibility table (csrc/host_compat.h), read back.  The features a handle can hold;
 * the last two are option flags that only LIFT an exclusion, and IPM_FEATURE_MEHROTRA_START is an operation (ipm_init_state_mehrotra /
 * ipm_init_small_batch_mehrotra), never held. */
enum {
    IPM_FEATURE_BOUNDS = 0, IPM_FEATURE_QUADRATIC, IPM_FEATURE_FREE, IPM_FEATURE_FREE_LP, IPM_FEATURE_DETECT, IPM_FEATURE_DETECT_QP,
    IPM_FEATURE_CORRECTORS, IPM_FEATURE_REFINEMENT, IPM_FEATURE_DENSE_SPLIT, IPM_FEATURE_LOCKSTEP, IPM_FEATURE_LOCKSTEP_BOUNDS,
    IPM_FEATURE_SMALL_PATH, IPM_FEATURE_MEHROTRA_START, IPM_FEATURE_SMALL_QUADRATIC_FLAG, IPM_FEATURE_SMALL_FREE_FLAG, IPM_FEATURE_COUNT
};
/* Is switching feature a ON refused on a handle that holds feature b?  *excluded = 1 / 0; *lifted_by = the feature whose presence on
 * the handle removes the exclusion, -1 for none (also when *excluded = 0).  Either pointer may be NULL.  A row is symmetric unless the
 * table declares it one-directional.  IPM_ERR_INVALID_ARG for an id outside 0 .. IPM_FEATURE_COUNT - 1. */
int ipm_debug_compat(int32_t a, int32_t b, int32_t* excluded, int32_t* lifted_by);
int ipm_debug_ff_schedule(int32_t nblk, int32_t q, int32_t workers, unsigned char* items, int32_t capacity, int32_t* count,
                          int32_t* tile_items, double sim_us[2]);
int ipm_get_phase_ms(ipm_handle* h, double out[4]);
/* Test hook: inv(L_kk) of diagonal block k of the handle's current dense factor, 128 x 128 row-major (zeros above the diagonal), to
 * host `out`.  Rows of the block beyond the LP's row count are padding: the identity (tests/test_gpu_parity.py). */
int ipm_debug_get_block_inverse(ipm_handle* h, int32_t k, double* out);
/* Test hook: the explicit inverse of diagonal group g of the handle's current dense factor (grouped triangular solves: gsz blocks
 * of 128 rows per group, floor(blocks / gsz) groups), whole, (128 gsz) x (128 gsz) row-major, to host `out`: which = 0 X_g =
 * inv(L_gg) (zeros above the diagonal), which = 1 XT_g, its transpose.  IPM_ERR_STATE on a handle without group inverses.  The
 * environment switch IPM_GINV_REF=1 (read by ipm_create) makes the handle assemble them with three launches of the generic GEMM
 * kernel per level instead of two of their own engine: the same bits (tests/test_gpu_group_inverse.py). */
int ipm_debug_get_group_inverse(ipm_handle* h, int32_t g, int32_t which, double* out);
/* Diagnostic (environment IPM_FF_TRACE_ITEMS=1 at ipm_create; IPM_ERR_STATE otherwise): time line of the LAST fused formation +
 * factorization launch on the device-wide 100 MHz clock.  *count = words of the trace: 4 per work item {drawn, inputs ready,
 * done, worker} followed by 12 per 128-row block {potrf_diag: start, inputs ready, done, -; critical panel: same; critical
 * update: same}; out (capacity words) receives it when large enough; items (8 bytes each, may be NULL) the work list,
 * *nitems its length.  tools/ff_trace.py turns it into per-step stall tables. */
int ipm_debug_ff_trace(ipm_handle* h, long long* out, int64_t capacity, int64_t* count, unsigned char* items, int32_t* nitems);
/* Test hook (host only, no GPU): the schedule merge of the lockstep batch (csrc/lockstep_merge.h).  n launch programs, program i =
 * types_flat[off[i] .. off[i+1]) (kernel types); aligned != 0: progressive alignment (the product's merge), 0: the leader rule it
 * replaced.  out_steps (2 ints per step, capacity cap_steps steps): {type, member count}; out_members (2 ints per launch): {program,
 * position} in step order.  Returns the number of steps, -1 on bad arguments / too small a capacity. */
int ipm_debug_ls_merge(int32_t n, const int32_t* off, const int32_t* types_flat, int32_t max_group, int32_t aligned,
                       int32_t* out_steps, int32_t cap_steps, int32_t* out_members);
/* Test hook (host only, launches nothing): the merged schedule that the last ipm_batch_step of `b` launched, four words per step
 * in launch order: {kernel type (LsType or, for a bounded step, LsBndType of csrc/lockstep.h), members (handles served by the launch, at most 64), blocks (the packed
 * 1-D grid: the sum of the members' own grids), lds (dynamic LDS bytes: the largest among the members)}.  *count = the number of
 * steps (0 before the first step); IPM_ERR_INVALID_ARG, with *count set, when capacity (in words) < 4 * steps
 * (tests/test_gpu_lockstep_wide.py). */
int ipm_debug_batch_schedule(ipm_batch* b, int32_t* out, int32_t capacity, int32_t* count);
/* Test hooks of the guard bands (environment IPM_TEST_ALLOC_GUARD=<band bytes>[:<band byte>], read at every allocation and in every
 * ipm_workspace_bytes* call).  With the knob set every device allocation of the library lies between
 * two bands of that many bytes filled with the band byte (255 when none is given), and the workspace holds one band before its first
 * region, one between every two regions and one behind the last.  One record describes one band: of a pool block the band before it
 * (side 0) and the band behind it (side 1, which begins at the block's first byte past the size asked for); of the workspace the band
 * behind each region (side 1: it runs from the region's last byte asked for to the next region) and the one before the first (side 0).
 * tag: the region's name ("ws:nvec") or the allocating call site ("host_fused.h:71#12", #ordinal).  first_bad / bad_count: offset
 * of the first byte of the band that is not the band byte and the number of such bytes (-1 / 0 where the band is intact or was not
 * compared). */
typedef struct ipm_guard_band {
    char tag[96];
    uint64_t address;      /* device address of the band's first byte */
    uint64_t bytes;        /* of the band */
    uint64_t inner;        /* device address of the allocation or region the band guards */
    uint64_t inner_bytes;  /* as asked for */
    int32_t side;          /* 0: before, 1: behind */
    int32_t device;
    int32_t byte;          /* the band byte */
    int32_t ordinal;       /* of the allocation in the process */
    int64_t first_bad;
    int64_t bad_count;
} ipm_guard_band;
/* The live bands of handle h -- its workspace's and those of the pool blocks allocated on its stream -- or, with h = NULL, of the
 * process.  *count = their number; out (capacity records, may be NULL) receives the first `capacity`.  Launches and reads nothing. */
int ipm_debug_guard_list(ipm_handle* h, ipm_guard_band* out, int32_t capacity, int32_t* count);
/* Compares the same bands now: synchronises the device(s), copies every band to the host and compares there.  *count = the number of
 * DAMAGED bands; out receives the first `capacity` of them with first_bad / bad_count filled in.  Nothing is repaired. */
int ipm_debug_guard_check(ipm_handle* h, ipm_guard_band* out, int32_t capacity, int32_t* count);
/* Reads and clears the process-wide violation log: the damaged bands found when a guarded block was freed or a guarded handle
 * destroyed (both compare before they release).  *count = records in the log before the call. */
int ipm_debug_guard_log(ipm_guard_band* out, int32_t capacity, int32_t* count);
/* Host only: the regions of the workspace of an m x n handle under the knob in effect (opts as for ipm_workspace_bytes_opts, may be
 * NULL), in address order: tag, address = the region's OFFSET in the workspace, inner = the same, inner_bytes = bytes asked for, bytes =
 * the band behind it (0 with the knob unset).  *total = what ipm_workspace_bytes_opts reports, *band = the band width (0: unset). */
int ipm_debug_guard_layout(int64_t m, int64_t n, const ipm_options* opts, ipm_guard_band* out, int32_t capacity, int32_t* count, uint64_t* total,
                           uint64_t* band);
/* Host only: the comparison the check and the log use, on a host buffer: *first_bad = offset of the first of the `bytes` bytes at
 * `band` that differs from `byte` (-1: none), *bad_count = how many differ. */
int ipm_debug_guard_compare(const unsigned char* band, uint64_t bytes, int32_t byte, int64_t* first_bad, int64_t* bad_count);

#ifdef __cplusplus
}
#endif
#endif /* IPM_HIP_H */
