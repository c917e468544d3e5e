// iteration_rules.h -- the Mehrotra predictor-corrector iteration, stated once (gfx950): the device-resident state of a solve
// and the per-column and per-scalar rules of one iteration.  vector_ops.h (one kernel per step: the dense, sparse, fused-factor
// and lockstep paths) and small_lp.h (the whole loop in one workgroup) call these.
// Also here, for the same two callers: the per-column rules of Mehrotra's starting point on the device (start_*, further down).
//
// A rule works on column j, or on scalars that one thread holds.  It loads and stores that column's entries and adds the column's
// terms to the calling thread's own running sums and minima, in a fixed order; it never combines values of different threads.
// The calling path owns where the vectors live, how it obtains (A^T dy)_j (passed in as a value), every reduction across threads
// and the order of its additions.
// `Cols` is VecArgs or SmallLP: a rule uses the column pointers both name alike (x, s, rc, d, v, q, dxa, dsa, dx, ds).
// Bounded = native upper bounds (BndArgs), Detect = the infeasibility tests (DetArgs),
// Quad = a diagonal quadratic term in the objective (quad_*).
//
// Two rules are NOT here yet and are still written out in both files, to be kept identical by hand: the predictor column
// (prepare_kernel_body / residual_cols) and the stop decision (stop_test_kernel_body / the stop_test lambda).  Every shared
// spelling tried for them moved the register or scratch sizes of one side: prepare_kernel 50 -> 44..48 VGPRs,
// prepare_bounded_kernel 60 -> 68, stop_test_kernel 26 -> 22, small_lp_detect_kernel 80 -> 84 B of scratch,
// small_lp_bounded_detect_kernel 48 -> 0 B.
//
// Reference code the rules restate (paths in the reference repo):
//   residuals r_b, r_c, r3          main.py:66-73   (test_create_rhs_predicted)
//   stop test                       main.py:162-173 (check_optimality)
//   predictor rhs / recovery        main.py:223-228 (direction_predicted_sparse "normal")
//   ratio tests                     main.py:305-322 (predicted_stepsize), :604-626 (full_stepsize)
//   mu, mu_aff, sigma               main.py:588-601 (duality_gap)
//   corrector complementarity rhs   main.py:150-152 (create_rhs_corrected)
//   iterate update                  main.py:694-696 (corrected)
#pragma once
#include <hip/hip_runtime.h>

namespace ipm {

// device-resident scalar state of a solve
struct Scalars {
    double b_norm, c_norm;
    double rb_norm, rc_norm, gap, obj;
    double mu, mu_aff, sigma;
    double alpha_aff_p, alpha_aff_d, alpha_p, alpha_d;
    double maxdiag;
    double e1, e2, e3, eta;
    double obj_last_finite;      // last finite c^T x seen by the stop test (main.py:1227-1233 returns it on NaN)
    int done, status, k, max_iter, fixed, force, fixed_first;   // fixed_first: guarded pivots of the first factorization
    int done_f;                  // `done` as it stood when the iteration's formation began (scaling_kernel): what the formation and
                                 // factorization kernels of the overlapped path test, and the group inverses behind them, so that a
                                 // stop test that flips `done` while they are in flight (it runs on the residual stream) never leaves
                                 // B half factored or the factor with the inverses of the iterate before
};

// per-iteration record (include/ipm_hip.h: ipm_iter_record), written by record_iteration into a ring
struct IterRec {
    int k, fixed;
    double obj, rb, rc, gap, mu, sigma, aap, aad, ap, ad;
};
constexpr int HIST_CAP = 1024;

// Native upper bounds 0 <= x <= u: the bounded instantiations (Bounded = true) take these.  Every array is an
// n-vector; outside the bounded set U, u = +inf and w = z = dw = dz = 0, so the streams stay coalesced and no index gather is
// needed.  qz = r_4 / w of the current direction (the z-analogue of q).
struct BndArgs {
    const double* u;
    double *w, *z, *dwa, *dza, *dw, *dz, *qz;
    int nU;                        // |U|
};
__device__ __forceinline__ bool bnd_in(double u) { return u < 1.7976931348623157e308; }     // finite bound (u is never NaN)
// theta_j = 1 / (s/x + z/w) on U: the diagonal of D^2 (scaling_kernel and prepare_kernel write it concurrently: one expression)
__device__ __forceinline__ double bnd_theta(double x, double s, double w, double z) { return 1.0 / (s / x + z / w); }
// the number of complementarity pairs: mu = (x.s + w.z) / (n + |U|), and mu_aff alike
template <bool Bounded>
__device__ __forceinline__ double pair_count(int n, const BndArgs& bd) { return Bounded ? (double)(n + bd.nU) : (double)n; }

// Separable convex QP (ipm_set_quadratic): min c.x + 1/2 x.diag(g) x with g >= 0 (g = 0 outside its support and in
// the padding).  The Quad instantiations differ from the LP in four places, each stated here once:
//   dual residual  r_c = A^T y + s - z - c - g o x                    (quad_rc: the term taken off the LP's r_c)
//   scaling        d = x / (s + g x), on U: 1 / (s/x + z/w + g)       (scaling_kernel and prepare_kernel write it concurrently:
//                                                                      one expression each)
//   objective      sum_j (c_j + 1/2 g_j x_j) x_j                      (the P_CX partial; no new reduction)
//   ONE step       alpha = min(alpha_p, alpha_d) wherever the iteration holds a (primal, dual) pair: with unequal steps the dual
//                  residual would keep a term (alpha_d - alpha_p) g o dx that no later Newton step is aimed at
// With that d and that r_c the predictor's v, direction_column, corrector_column, the right-hand side -r_b - A v and the recovery
// keep the LP's formulas (eliminating ds = -(r_3 + s dx)/x from A^T dy + ds - dz - g o dx = -r_c only adds g to the diagonal).
// Both paths use them: the Quad kernels of vector_ops.h, and the Quad variants of the one-workgroup loop (small_lp.h,
// IPM_FLAG_SMALL_QUADRATIC), whose residual_cols applies the first three and whose loop applies the step rule to both pairs.
__device__ __forceinline__ double quad_rc(double rc_lp, double g, double x) { return rc_lp - g * x; }
__device__ __forceinline__ double quad_theta(double x, double s, double g) { return x / (s + g * x); }
__device__ __forceinline__ double quad_bnd_theta(double x, double s, double w, double z, double g) { return 1.0 / (s / x + z / w + g); }
__device__ __forceinline__ double quad_objective(double c, double g, double x) { return (c + 0.5 * g * x) * x; }
__device__ __forceinline__ double quad_step(double ap, double ad) { return fmin(ap, ad); }

// Free columns with curvature (ipm_set_free_columns): column j of a Quad handle with g_j > 0 that carries no sign
// constraint -- no s_j (stored as exactly 0), no bound (u_j = +inf), no complementarity pair.  What factor-model QPs need:
// Q = diag(g) + F F^T becomes t = F^T x with free t and 1/2 t.t in the diagonal.  The Free instantiations differ from the Quad
// ones in the rows below, each stated here once; the mark is an np-vector of bytes of the library's own (1 = free, 0 elsewhere and
// in the padding; constant during a solve), one more coalesced stream and no index gather:
//   dual residual  r_c = (A^T y)_j - c_j - g_j x_j                    (free_rc: quad_rc with s_j = 0)
//   scaling        d = 1 / g_j                                        (free_theta: finite, constant, exact; never x / (s + g x),
//                                                                      which is 0/0 at x_j = 0; scaling_kernel and prepare_kernel
//                                                                      write it concurrently: one expression)
//   predictor      q = 0, v = d r_c                                   (free_rhs_column; the corrector's column alike: no sigma mu)
//   objective      (c_j + 1/2 g_j x_j) x_j                            (quad_objective, unchanged)
//   recovery       dx = d w + v, ds = 0 (dw = dz = 0)                 (free_direction_column)
//   ratio tests    no contribution to minp or mind
//   mu, mu_aff, sigma: no term; the pair count is n - n_free (+ |U|)  (free_pair_count) in the stop test and the centring
//   update         x += alpha dx; s stays 0                           (free_update_column)
//   stop test      r_c of a free column counts in ||r_c||; it adds nothing to the gap
// Eliminating dx_j = (A^T dy + r_c)_j / g_j from row j of the Newton system, A^T dy - g dx = -r_c, puts 1/g_j on the diagonal of
// Theta: formation, every factorization path, the sweeps, refinement and the dense-column split read only d and serve it unchanged.
// The one step length of quad_step applies as to every quadratic handle.  A handle keeps at least one pair (n - n_free + |U| >= 1).
// Both paths use them: the Free kernels of vector_ops.h, and the Free variants of the one-workgroup loop (small_lp.h,
// IPM_FLAG_SMALL_FREE), whose column loops call the same helpers on the marked columns.
struct FreeArgs {
    const unsigned char* mark;     // [np] 1 on the free columns
    int nfree;
};
__device__ __forceinline__ bool free_in(const FreeArgs& fr, int j) { return fr.mark[j] != 0; }
__device__ __forceinline__ double free_rc(double aty, double c, double g, double x) { return quad_rc(aty - c, g, x); }
__device__ __forceinline__ double free_theta(double g) { return 1.0 / g; }
template <bool Bounded>
__device__ __forceinline__ double free_pair_count(int n, const BndArgs& bd, const FreeArgs& fr) { return pair_count<Bounded>(n - fr.nfree, bd); }
// q = 0, v = d r_c: the column of the predictor's and of the corrector's right-hand side (Bounded: qz = 0, the column is outside U)
template <bool Bounded, class Cols>
__device__ __forceinline__ void free_rhs_column(const Cols& a, const BndArgs& bd, int j, double dj, double rcj) {
    a.q[j] = 0.0;
    a.v[j] = dj * rcj;
    if constexpr (Bounded) bd.qz[j] = 0.0;
}
template <bool Bounded, class Cols>
__device__ __forceinline__ void free_direction_column(const Cols& a, int j, double w, double* DX, double* DS, double* DW, double* DZ) {
    DX[j] = a.d[j] * w + a.v[j];
    DS[j] = 0.0;
    if constexpr (Bounded) { DW[j] = 0.0; DZ[j] = 0.0; }
}
template <class Cols>
__device__ __forceinline__ void free_update_column(const Cols& a, int j, double ap) { a.x[j] += ap * a.dx[j]; }

// LP free columns (ipm_set_free_lp_columns): column j of an LP handle -- no quadratic term anywhere -- that carries no
// sign constraint.  It has no curvature of its own, so the Newton matrix borrows one: proximal-point primal regularisation of the
// free block only (Altman and Gondzio, Optim. Methods Softw. 11 (1999) 275-302).  At iteration k the free block of the objective
// carries 1/2 rho |x_Phi - x_Phi^k|^2, centred AT the iterate: its gradient there is zero, so r_c, the objective and the stop test
// are the true LP's; only the matrix sees rho, as Theta_j = 1 / rho.  Nothing is subtracted anywhere.  The rows that differ from
// an LP column, each stated once; the byte marks are FreeArgs, rho is the handle's one scalar (in the handle's units):
//   dual residual  r_c = (A^T y)_j - c_j                              (free_lp_rc: no s, no g x)
//   scaling        d = 1 / rho                                        (free_lp_theta: scaling_kernel and prepare_kernel write it
//                                                                      concurrently: one expression)
//   predictor      q = 0, v = d r_c                                   (free_rhs_column as it is; the corrector's column alike)
//   objective      c_j x_j
//   recovery       dx = d w + v, ds = 0 (dw = dz = 0)                 (free_direction_column as it is)
//   ratio tests, mu, mu_aff, sigma: no term; free_pair_count pairs
//   step lengths   the LP's two, alpha_p and alpha_d (never quad_step); x += alpha_p dx, s stays 0 (free_update_column)
//   stop test      r_c of the column counts in ||r_c||; nothing into the gap
// Row j of the Newton system is A^T dy - rho dx = -r_c: an inexact Newton step whose dual residual on the column after a step of
// length alpha_d is (1 - alpha_d) r_c + alpha_d rho dx_j, which vanishes with dx.
// The start (start_free_lp_*): x_j is the least-squares value, unshifted and uncorrected; s_j = 0; no term in a minimum or a sum.
struct FreeLpArgs {
    FreeArgs cols;                 // the marks and their count
    double rho;
};
__device__ __forceinline__ double free_lp_rc(double aty, double c) { return aty - c; }
__device__ __forceinline__ double free_lp_theta(double rho) { return 1.0 / rho; }

// Infeasibility tests of IPM_FLAG_DETECT_INFEASIBILITY, on the iterate of a stop test that said "continue":
//   primal infeasible: beta = b.y - u_U.z_U > 0 and max_j (A^T y - z)_j+ <= eps_p beta   (certificate y / beta, z / beta)
//   dual infeasible:   gamma = -c.x > 0 and max(||A x||_inf, max x_U) <= eps_d gamma      (certificate x / gamma)
// Maxima, not sums of squares: the iterate runs along a ray and |y| reaches 1e87 before the test fires.
//
// The same two tests of a quadratic handle (IPM_FLAG_DETECT_QUADRATIC), with U the native bounds, Phi the free columns
// and g the diagonal (0 where there is no term); with g = 0 and Phi empty they are the LP's tests exactly:
//   primal infeasible: beta as above and max( max_{j not in Phi} (A^T y - z)_j+ , max_{j in Phi} |(A^T y)_j| ) <= eps_p beta
//                      (detect_dual_free: a free column has no s that absorbs a reduced cost of either sign -- equality)
//   dual infeasible:   gamma = -c.x > 0 with c.x the LINEAR part only (the handle's objective carries 1/2 g x^2: detect_linear)
//                      and max(||A x||_inf, max x_U, max_j g_j |x_j|) <= eps_d gamma   (detect_curvature: the ray avoids the curvature)
// The iteration itself is unchanged: only what the stop test reads from the iterate differs.
__device__ __forceinline__ double detect_dual_free(double aty) { return fabs(aty); }
__device__ __forceinline__ double detect_linear(double c, double x) { return c * x; }
__device__ __forceinline__ double detect_curvature(double g, double x) { return g * fabs(x); }
struct DetArgs {
    double eps_p, eps_d;
    double* out;                   // [4]: kind (5 / 6), normalisation (beta / gamma), violation / normalisation, k at detection
};
constexpr int IPM_STATUS_PRIMAL_INFEASIBLE_ = 5, IPM_STATUS_DUAL_INFEASIBLE_ = 6;   // include/ipm_hip.h
// one thread; true (and done, status, dt.out set) when a test fires
__device__ __forceinline__ bool detect_fire(DetArgs dt, Scalars* sc, double beta, double vp, double gamma, double vd) {
    int kind = 0;
    double nrm = 0.0, viol = 0.0;
    if (beta > 0.0 && beta < 1.7e308 && vp <= dt.eps_p * beta) { kind = IPM_STATUS_PRIMAL_INFEASIBLE_; nrm = beta; viol = vp; }
    else if (gamma > 0.0 && gamma < 1.7e308 && vd <= dt.eps_d * gamma) { kind = IPM_STATUS_DUAL_INFEASIBLE_; nrm = gamma; viol = vd; }
    if (!kind) return false;
    dt.out[0] = (double)kind; dt.out[1] = nrm; dt.out[2] = viol / nrm; dt.out[3] = (double)sc->k;
    sc->status = kind;
    sc->done = 1;
    return true;
}

// start of a solve (force: no stop decision, ipm_iterate; reset: a new solve, not a continuation)
__device__ __forceinline__ void start_solve(Scalars* sc, double e1, double e2, double e3, double eta, int max_iter, int force, int reset) {
    sc->e1 = e1; sc->e2 = e2; sc->e3 = e3; sc->eta = eta;
    sc->max_iter = max_iter; sc->force = force;
    sc->done = 0; sc->done_f = 0; sc->status = 0;
    if (reset) { sc->k = 0; sc->fixed = 0; sc->fixed_first = 0; sc->obj_last_finite = __builtin_nan(""); }
}

// Direction recovery from w = (A^T dy)_j with the current q, v (main.py:227-228) and the ratio tests (main.py:305-322): this
// thread's running minima minp (over x, w) and mind (over s, z).  Bounded, on U: dw = -r_u - dx, dz = -(r4 + z dw)/w (qz = r4/w);
// dw = dz = 0 outside U.  (DX, DS, DW, DZ): the affine or the corrected direction.  xj, sj = x[j], s[j]: each path loads them on
// its own side of the product with A^T, and its register allocation depends on that.
template <bool Bounded, class Cols>
__device__ __forceinline__ void direction_column(const Cols& a, const BndArgs& bd, int j, double w, double* DX, double* DS, double* DW,
                                                 double* DZ, double xj, double sj, double& minp, double& mind) {
    const double dxj = a.d[j] * w + a.v[j];
    const double dsj = (-sj * dxj) / xj - a.q[j];
    DX[j] = dxj; DS[j] = dsj;
    if (dxj < 0.0) minp = fmin(minp, -xj / dxj);
    if (dsj < 0.0) mind = fmin(mind, -sj / dsj);
    if constexpr (Bounded) {
        const double uj = bd.u[j];
        double dwj = 0.0, dzj = 0.0;
        if (bnd_in(uj)) {
            const double wj = bd.w[j], zj = bd.z[j];
            dwj = -(xj + wj - uj) - dxj;
            dzj = (-zj * dwj) / wj - bd.qz[j];
            if (dwj < 0.0) minp = fmin(minp, -wj / dwj);
            if (dzj < 0.0) mind = fmin(mind, -zj / dzj);
        }
        DW[j] = dwj; DZ[j] = dzj;
    }
}

// column j's terms of (x + a_p dxa).(s + a_d dsa) and, Bounded, (w + a_p dwa).(z + a_d dza) (0 outside U), added to this thread's
// running sum in that order                                                        main.py:579-584, 598
template <bool Bounded, class Cols>
__device__ __forceinline__ void mu_aff_column(const Cols& a, const BndArgs& bd, int j, double ap, double ad, double& acc) {
    acc += (a.x[j] + ap * a.dxa[j]) * (a.s[j] + ad * a.dsa[j]);
    if constexpr (Bounded) acc += (bd.w[j] + ap * bd.dwa[j]) * (bd.z[j] + ad * bd.dza[j]);
}

// centring: mu_aff = (the reduced sum of mu_aff_column) / pairs ; sigma = (mu_aff / mu)^3          main.py:588-601
struct Centring { double mu_aff, sigma; };
template <bool Bounded>
__device__ __forceinline__ Centring centring(double sum, double mu, int n, const BndArgs& bd) {
    const double mu_aff = sum / pair_count<Bounded>(n, bd);
    const double r = mu_aff / mu;
    return {mu_aff, r * r * r};
}

// corrector column, sm = sigma mu: r3c = x s + dxa dsa - sm ; q = r3c/x ; v = d (r_c - q)             main.py:150-152
// Bounded, on U: r4c = w z + dwa dza - sm ; qz = r4c/w ; v = theta (r_c - q + (r4c - z r_u)/w)
// Two steps, so that a centrality corrector (below) re-enters at the second with its own complementarity terms: the terms, then
// q, qz, v from them into the arrays `a`, `bd` name.
template <class Cols>
__device__ __forceinline__ double corrector_r3(const Cols& a, int j, double xj, double sm) { return xj * a.s[j] + a.dxa[j] * a.dsa[j] - sm; }
__device__ __forceinline__ double corrector_r4(const BndArgs& bd, int j, double wj, double zj, double sm) { return wj * zj + bd.dwa[j] * bd.dza[j] - sm; }
template <class Cols>
__device__ __forceinline__ void corrector_rhs_plain(const Cols& a, int j, double qj) { a.v[j] = a.d[j] * (a.rc[j] - qj); }
template <class Cols>
__device__ __forceinline__ void corrector_rhs_bounded(const Cols& a, const BndArgs& bd, int j, double xj, double wj, double zj, double uj, double qj, double r4c) {
    bd.qz[j] = r4c / wj;
    a.v[j] = a.d[j] * (a.rc[j] - qj + (r4c - zj * (xj + wj - uj)) / wj);
}
template <bool Bounded, class Cols>
__device__ __forceinline__ void corrector_column(const Cols& a, const BndArgs& bd, int j, double sm) {
    const double xj = a.x[j];
    const double r3c = corrector_r3(a, j, xj, sm);
    const double qj = r3c / xj;
    a.q[j] = qj;
    if constexpr (Bounded) {
        const double uj = bd.u[j];
        if (bnd_in(uj)) {
            const double wj = bd.w[j], zj = bd.z[j];
            corrector_rhs_bounded(a, bd, j, xj, wj, zj, uj, qj, corrector_r4(bd, j, wj, zj, sm));
            return;
        }
    }
    corrector_rhs_plain(a, j, qj);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Gondzio's multiple centrality correctors (Comput. Optim. Appl. 6 (1996) 137-156): after Mehrotra's corrector the
// factor is used again for up to K rounds.  A round aims the complementarity products of a trial point a little beyond the step
// just found back into the box [beta_min, beta_max] sigma mu, solves for the direction with that target and keeps it when the
// step lengths grow by gamma delta in sum.
// The device-resident record of the rounds (the library's own allocation, beside the candidate vectors; the scalar record of the
// solve is not touched).  ap, ad: the step lengths of the direction a round starts from, left by its target kernel for its accept
// kernel.  rdone: the word the kernels of a round test in place of Scalars::done (done, or the chain of this iteration is dead: a
// round was rejected); rdead: a round of this iteration was rejected.  Tallies of the solve (ipm_get_corrector_info): rounds that
// did work, rounds accepted, iterations with an accepted round; hit: this iteration has one.
struct MccCtl {
    double ap, ad;
    int rdone, rdead, run, acc, iters, hit;
};
constexpr double MCC_DELTA = 0.1, MCC_GAMMA = 0.1, MCC_BETA_MIN = 0.1, MCC_BETA_MAX = 10.0;
__device__ __forceinline__ double mcc_trial_step(double alpha) { return fmin(1.0, alpha + MCC_DELTA); }
// the correction t of one complementarity product v = (x + a~_p dx)(s + a~_d ds): the projection onto the box minus v, bounded below
__device__ __forceinline__ double mcc_target(double v, double sm) {
    const double t = fmin(fmax(v, MCC_BETA_MIN * sm), MCC_BETA_MAX * sm) - v;
    return fmax(t, -MCC_BETA_MAX * sm);
}
// the candidate replaces the direction iff its step lengths gained gamma delta in sum; a NaN on either side rejects
__device__ __forceinline__ bool mcc_accept(double ap, double ad, double ahp, double ahd) { return ahp + ahd >= ap + ad + MCC_GAMMA * MCC_DELTA; }
// Column j of a round's right-hand side.  r3c (Bounded, on U: r4c): the complementarity terms of the direction the round starts from.
// `a`, `bd` name the current direction (dx, ds, dw, dz); `c`, `cb` are the same views with the CANDIDATE's q, v (qz) in place, which
// corrector_column's second step fills.  r3g (r4g) receive the candidate's terms r3c - t (r4c - t4; 0 outside U).
template <bool Bounded, class Cols>
__device__ __forceinline__ void mcc_rhs_column(const Cols& a, const BndArgs& bd, const Cols& c, const BndArgs& cb, int j, double tp, double td,
                                               double sm, double r3c, double r4c, double* r3g, double* r4g) {
    const double xj = a.x[j];
    const double r3 = r3c - mcc_target((xj + tp * a.dx[j]) * (a.s[j] + td * a.ds[j]), sm);
    const double qj = r3 / xj;
    r3g[j] = r3;
    c.q[j] = qj;
    if constexpr (Bounded) {
        const double uj = bd.u[j];
        if (bnd_in(uj)) {
            const double wj = bd.w[j], zj = bd.z[j];
            const double r4 = r4c - mcc_target((wj + tp * bd.dw[j]) * (zj + td * bd.dz[j]), sm);
            r4g[j] = r4;
            corrector_rhs_bounded(c, cb, j, xj, wj, zj, uj, qj, r4);
            return;
        }
        r4g[j] = 0.0;
    }
    corrector_rhs_plain(c, j, qj);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Iterative refinement of one normal-equations solve (ipm_set_refinement; restated in NumPy as tests/refine_oracle.py).
// The solve gave dy = B~^-1 t with the FACTORED matrix B~ (guarded pivots, Tikhonov shift, rounding of the blocked Cholesky) and
// a = A^T dy.  Up to k rounds correct it against the matrix-free operator A D^2 A^T.  Round j = 1 .. k:
//   1. r = t - A (d o a), rho_j = ||r||_2 (fixed-order reduction, bitwise repeatable);
//   2. rho_j is 0 or not finite: the rounds of this solve end;
//   3. j > 1 and rho_j > rho_{j-1}: (dy, a) are restored from the copy taken before the previous correction, a revert is
//      counted, the rounds end;
//   4. j > 1 and rho_j > rho_{j-1} / 2: the rounds end, the previous correction stays;
//   5. otherwise (dy, a) are copied aside, delta = B~^-1 r with the same factor and sweeps, dy += delta, a += A^T delta.
// The correction of the LAST round is never measured: no residual follows it.
// The decision of a round is this function, run by one thread (refine_decide_kernel) on the reduced sums of r^2 and t^2; it lives
// in the device-side record, so no host synchronisation takes part.  rdone: the word the products with A and the substitutions
// of a round test in place of Scalars::done (`outer_done`: the word the solve itself tests -- Scalars::done, or MccCtl::rdone inside
// a centrality-corrector round); action: what the round's apply kernel does.  Tallies (ipm_get_refinement_info): solves whose
// first round ran, corrections applied, rounds ended by rule 4, reverts, rho_1/||t|| and the last kept rho/||t|| of the most recent
// solve, the largest rho_1/||t|| of the sequence.
enum { REF_NONE = 0, REF_APPLY = 1, REF_RESTORE = 2 };
struct RefCtl {
    double rho_prev, first_rel, last_rel, max_rel;
    long long solves, applied, half, reverts;
    int rdone, action;
};
__device__ __forceinline__ void refine_decide(RefCtl* c, double r2, double t2, bool first, bool outer_done) {
    c->action = REF_NONE;
    if (first) {
        c->rdone = outer_done ? 1 : 0;
        if (outer_done) return;
        c->solves += 1;
    } else if (c->rdone) return;
    const double rho = sqrt(r2), tn = sqrt(t2);
    const double rel = rho > 0.0 ? rho / tn : rho;               // (rho = 0 with t = 0: 0, not 0/0)
    if (first) { c->first_rel = rel; c->max_rel = fmax(c->max_rel, rel); }
    if (!(rho > 0.0) || !(rho < 1.7976931348623157e308)) { c->last_rel = rel; c->rdone = 1; return; }                  // rule 2
    if (!first && rho > c->rho_prev) { c->reverts += 1; c->action = REF_RESTORE; c->rdone = 1; return; }              // rule 3
    if (!first && rho > 0.5 * c->rho_prev) { c->half += 1; c->last_rel = rel; c->rdone = 1; return; }                  // rule 4
    c->applied += 1; c->rho_prev = rho; c->last_rel = rel; c->action = REF_APPLY;                                     // rule 5
}

// damped step from the reduced ratio-test minimum (main.py:604-626) and the column update x += a_p dx ; s += a_d ds
// (Bounded: w += a_p dw ; z += a_d dz)  (main.py:694-696); y += a_d dy stays with the path, which knows where y lives
__device__ __forceinline__ double damped_step(double eta, double ratio_min) { return fmin(1.0, eta * ratio_min); }
template <bool Bounded, class Cols>
__device__ __forceinline__ void update_column(const Cols& a, const BndArgs& bd, int j, double ap, double ad) {
    a.x[j] += ap * a.dx[j];
    a.s[j] += ad * a.ds[j];
    if constexpr (Bounded) {
        bd.w[j] += ap * bd.dw[j];
        bd.z[j] += ad * bd.dz[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Mehrotra's starting point (SIAM J. Optim. 2 (1992) 575-601, section 7), the per-column rules of the device start
// (ipm_init_state_mehrotra): the least-squares x = A^T (A A^T)^-1 b and r = c - A^T (A A^T)^-1 A c come in as values, the calling path
// owns the solves, the products with A^T and every reduction.  Bounded, on U: w = u - x and r splits into s = max(r, 0), z = max(-r, 0);
// outside U, w = z = 0.  The arithmetic per column, and its order, is that of IpmSolver.mehrotra_start (handle.py).
//
// least-squares primal column: x (and w) as computed; this thread's running minimum over x and w_U
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_primal_column(const Cols& a, const BndArgs& bd, int j, double xj, double& mn) {
    a.x[j] = xj;
    mn = fmin(mn, xj);
    if constexpr (Bounded) {
        const double uj = bd.u[j];
        double wj = 0.0;
        if (bnd_in(uj)) { wj = uj - xj; mn = fmin(mn, wj); }
        bd.w[j] = wj;
    }
}
// least-squares dual column from the reduced cost r_j; this thread's running minimum over s and z_U
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_dual_column(const Cols& a, const BndArgs& bd, int j, double rj, double& mn) {
    double sj = rj;
    if constexpr (Bounded) {
        double zj = 0.0;
        if (bnd_in(bd.u[j])) { sj = fmax(rj, 0.0); zj = fmax(-rj, 0.0); mn = fmin(mn, zj); }
        bd.z[j] = zj;
    }
    a.s[j] = sj;
    mn = fmin(mn, sj);
}
// shift into the positive orthant from a reduced minimum: max(-1.5 min, 0)
__device__ __forceinline__ double start_shift(double mn) { return fmax(-1.5 * mn, 0.0); }
// x += dp, s += dd (on U: w += dp, z += dd); column j's terms of x.s + w.z, sum s + sum z_U and sum x + sum w_U
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_shift_column(const Cols& a, const BndArgs& bd, int j, double dp, double dd, double& xs, double& ss, double& sx) {
    const double xj = a.x[j] + dp, sj = a.s[j] + dd;
    a.x[j] = xj; a.s[j] = sj;
    xs += xj * sj; ss += sj; sx += xj;
    if constexpr (Bounded) {
        if (bnd_in(bd.u[j])) {
            const double wj = bd.w[j] + dp, zj = bd.z[j] + dd;
            bd.w[j] = wj; bd.z[j] = zj;
            xs += wj * zj; ss += zj; sx += wj;
        }
    }
}
// degenerate data (xs = (x.s + w.z) / 2 not finite or not positive, or a non-positive sum): the reference's start instead
__device__ __forceinline__ bool start_degenerate(double xs, double ss, double sx) { return !(fabs(xs) < 1.7e308 && ss > 0.0 && sx > 0.0 && xs > 0.0); }
// primal correction x += pc (on U: w += pc); column j's terms of sum x + sum w_U after it
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_primal_correct_column(const Cols& a, const BndArgs& bd, int j, double pc, double& sx) {
    const double xj = a.x[j] + pc;
    a.x[j] = xj; sx += xj;
    if constexpr (Bounded) {
        if (bnd_in(bd.u[j])) { const double wj = bd.w[j] + pc; bd.w[j] = wj; sx += wj; }
    }
}
// dual correction s += dc (on U: z += dc)
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_dual_correct_column(const Cols& a, const BndArgs& bd, int j, double dc) {
    a.s[j] += dc;
    if constexpr (Bounded) {
        if (bnd_in(bd.u[j])) bd.z[j] += dc;
    }
}
// the reference's start in column j, what ipm_init_state leaves: x = s = 1 (w = z = 1 on U, 0 outside)
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_reference_column(const Cols& a, const BndArgs& bd, int j) {
    a.x[j] = 1.0; a.s[j] = 1.0;
    if constexpr (Bounded) {
        const double o = bnd_in(bd.u[j]) ? 1.0 : 0.0;
        bd.w[j] = o; bd.z[j] = o;
    }
}

// The same five steps on an LP free column (FreeLpArgs above): the least-squares x as computed, s = 0 (w = z = 0: the column is
// outside U), and no term in any minimum or sum -- so the shift and both corrections pass it by.  On degenerate data the reference's
// start as ipm_init_state leaves it on such a handle: x = 1, s = 0.
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_free_lp_primal_column(const Cols& a, const BndArgs& bd, int j, double xj) {
    a.x[j] = xj;
    if constexpr (Bounded) bd.w[j] = 0.0;
}
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_free_lp_dual_column(const Cols& a, const BndArgs& bd, int j) {
    a.s[j] = 0.0;
    if constexpr (Bounded) bd.z[j] = 0.0;
}
template <bool Bounded, class Cols>
__device__ __forceinline__ void start_free_lp_reference_column(const Cols& a, const BndArgs& bd, int j) {
    a.x[j] = 1.0; a.s[j] = 0.0;
    if constexpr (Bounded) { bd.w[j] = 0.0; bd.z[j] = 0.0; }
}

// end of an iteration -- one thread: the IterRec of iteration k into the ring, the step lengths, k += 1.  mu, sigma and the affine
// step lengths come as values: the multi-kernel path reads them from *sc, where earlier kernels left them; the one-workgroup loop
// holds them in registers and stores mu_aff, sigma and the affine step lengths itself.
__device__ __forceinline__ void record_iteration(Scalars* sc, IterRec* hist, double mu, double sigma, double aap, double aad, double ap, double ad) {
    const int k = sc->k;
    IterRec r;
    r.k = k; r.fixed = sc->fixed; r.obj = sc->obj; r.rb = sc->rb_norm; r.rc = sc->rc_norm; r.gap = sc->gap;
    r.mu = mu; r.sigma = sigma; r.aap = aap; r.aad = aad; r.ap = ap; r.ad = ad;
    hist[k % HIST_CAP] = r;
    sc->alpha_p = ap; sc->alpha_d = ad; sc->k = k + 1;
}

}  // namespace ipm
