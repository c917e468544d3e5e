// small_lp.h -- the whole Mehrotra predictor-corrector LOOP of a small LP (m <= 128) in ONE launch of ONE
// workgroup (gfx950).  Replaces, for the AFIRO class of the Netlib set, the loop body of interior_sparse
// (main.py:780-807 of the reference repo) that the multi-kernel path runs as ~60 launch-bound kernels per
// iteration (AFIRO: 106 us per iteration, 93 iterations): here an iteration never leaves the compute unit.
//
//   * A stays sparse in HBM/L2 (CSR + CSC, as uploaded by ipm_set_A_csc); the n-vectors stay in global memory
//     (they are L2 resident: one workgroup, <= 100 KB); the m-vectors, the normal matrix B (16 nt x 16 nt, nt =
//     ceil(m/16)), its factor L and inv(L) live in LDS for the whole solve.
//   * B = A diag(d) A^T is evaluated from a PRODUCT LIST built once on the host: lower entry e = (i, k) is
//     sum_t coef[t] * d[col[t]] over the columns j that rows i and k share (coef = a_ij a_kj) -- a sparse
//     matrix-vector product with d, one thread per entry, no atomics, fixed order.
//   * The factorization is potrf_lds() -- the same guarded LDS Cholesky the blocked path runs on its 128 x 128
//     diagonal blocks -- on nt panels instead of 8; both triangular solves are matvecs with inv(L) in LDS.
//   * Reductions are wave shuffles + a fixed-order sum over the 8 waves: bitwise reproducible.
//
// The rules of the iteration are iteration_rules.h, shared with the multi-kernel path (vector_ops.h), except the predictor column
// (residual_cols) and the stop decision (stop_test), which restate prepare_kernel and stop_test_kernel of vector_ops.h: same
// mathematics, constants and stop test.  This file owns what this path does around the rules: A and the vectors
// as placed above, (A^T y)_j as a CSC dot product with y in LDS, the normal equations, and the reductions.  Their summation orders
// differ from the multi-kernel path's, so iterates agree to rounding, not bit for bit (tests compare both against the reference).
// residual_cols is the hand-kept second copy of the predictor column (iteration_rules.h): its Quad branches are kept in step with
// prepare_kernel_body<..., Quad> of vector_ops.h, its Free branch with prepare_kernel_body<..., Quad, Free>.
// Below the loop: Mehrotra's starting point of such an LP in one launch (small_start_body), single and batched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "potrf_f64.h"
#include "sparse_ops.h"
#include "vector_ops.h"

namespace ipm {

constexpr int SMALL_MAX_M = 128;
constexpr int IPM_STATUS_NEEDS_SHIFT = 4;      // internal: left after the first factorization, ipm_solve restarts

struct SmallLP {
    SparseA A;
    int m, n, nt;
    const int* bptr; const unsigned short* bi; const unsigned short* bk; const int* bcol; const double* bcoef; int nb;
    double *x, *y, *s;
    const double *b, *c;
    double *rc, *d, *v, *q, *dxa, *dsa, *dx, *ds;
    Scalars* sc;
    IterRec* hist;
    double eps, big, shift_rel;
    int max_steps;
    int auto_reg;
};

// sum / min of NV values over the 512 threads, fixed order; result in every thread.  `red` = 8 * NV doubles of LDS.
// FRESH_TID: the thread index is read behind an empty asm, so that nothing derived from it is hoisted out of the caller's loop
// (small_lp_body's Detect + Quad variants; see the note at `ctid` there).  false: the code it always was.
template <int NV, bool MIN, bool FRESH_TID = false>
__device__ __forceinline__ void block_reduce512(double (&v)[NV], double* red) {
    const int lane = thread_index<FRESH_TID>() & 63, wave = thread_index<FRESH_TID>() >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(v[q], off, 64);
            v[q] = MIN ? fmin(v[q], o) : v[q] + o;
        }
    }
    __syncthreads();                                   // red may still be read from the previous reduction
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) red[wave * NV + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double r = red[q];
#pragma unroll
        for (int w = 1; w < 8; ++w) r = MIN ? fmin(r, red[w * NV + q]) : r + red[w * NV + q];
        v[q] = r;
    }
}

// Bounded = true: native upper bounds (BndArgs) -- the same loop with the w / z terms folded into
// the same reductions (r_u^2 into ||r_b||^2, w.z into x.s, the w / z ratios into the step minima); no extra LDS.
// Detect = true: the infeasibility tests (detect_fire) in the stop test, from sums and maxima the residual passes
// gather on the side (b.y, u_U.z_U, max (A^T y - z)_+, max |A x|, max x_U).
// Quad = true: a diagonal quadratic term g (the handle's quad_g; IPM_FLAG_SMALL_QUADRATIC): r_c, d and the objective
// by the quad_* rules in residual_cols, and one step length (quad_step) wherever a (primal, dual) pair is held.  Everything else
// -- the formation from d, the factorization, both matvecs, the direction, the corrector and the stop test -- is the LP's.
// Free = true: free columns with curvature (FreeArgs; IPM_FLAG_SMALL_FREE): a marked column takes the free_* rules of
// iteration_rules.h in every column loop -- d = 1 / g, q = 0, v = d r_c, ds = 0, no ratio, no term of mu_aff -- and the pair count of
// the stop test and the centring is free_pair_count.  One more byte per column from global memory; no LDS, no reduction of its own.
// Detect with Quad (IPM_FLAG_DETECT_QUADRATIC; iteration_rules.h states the tests): residual_cols also gathers the linear
// c.x and max g|x| (and |A^T y| of a free column into the dual maximum), which ride in the two reductions the LP's tests make -- one
// more sum, one more maximum, the same LDS, no scratch memory (the note at `ctid` below says what that took).
template <bool Bounded, bool Detect = false, bool Quad = false, bool Free = false>
__device__ __forceinline__ void small_lp_body(SmallLP a, BndArgs bd, DetArgs dt = DetArgs{}, const double* g = nullptr, FreeArgs fr = FreeArgs{}) {
    static_assert(!Free || Quad, "a free column needs curvature: Free is only meaningful with Quad");
    __shared__ __attribute__((aligned(16))) double W[NB * WLD];
    __shared__ double dinv_s[NB];
    __shared__ double ys[NB], rbs[NB], t1s[NB], zs[NB], dys[NB];
    __shared__ double red[8 * 4];
    __shared__ double sh[8];                            // broadcast scalars
    __shared__ int go;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = a.m, n = a.n, nt = a.nt, mt = 16 * a.nt;
    const int row4 = tid >> 2, l4 = tid & 3;            // 4 lanes per row of A / of the triangular matvecs
    Scalars* sc = a.sc;

    if (tid < NB) {
        ys[tid] = tid < m ? a.y[tid] : 0.0;
        rbs[tid] = 0.0; t1s[tid] = 0.0; zs[tid] = 0.0; dys[tid] = 0.0;
    }
    __syncthreads();

    // The thread's indices as the loop body uses them.  In the Detect + Quad variants they are made opaque to the compiler at the top of
    // every iteration (an empty asm; potrf_lds and block_reduce512 do the same with their own copy, FRESH_TID), so that the per-thread
    // addresses and LDS offsets are formed where they are used: hoisted out of the loop, some fifty of them stayed live across the whole
    // iteration and the variants spilled 52 .. 68 VGPRs (204 .. 272 bytes of scratch per lane).  With this: none, 0 bytes.  In every
    // other variant they ARE tid, row4, l4 and the kernels are the code they were.
    int ctid = tid, crow4 = row4, cl4 = l4;
    double dby = 0.0, duz = 0.0, dmaty = 0.0, dmax = 0.0, dmxu = 0.0;      // Detect: this thread's share of the test quantities
    double dcxl = 0.0, dmgx = 0.0;                                         // Detect with Quad: of the linear c.x and of max g|x|
    // r_b = A x - b into rbs (4 lanes per row), returns this thread's share of ||r_b||^2
    auto residual_rows = [&]() {
        double rb2 = 0.0;
        if (crow4 < m) {
            const int pb = a.A.rowptr[crow4], pe = a.A.rowptr[crow4 + 1];
            double acc = 0.0;
            for (int p = pb + cl4; p < pe; p += 4) acc += a.A.rval[p] * a.x[a.A.colind[p]];
            acc += __shfl_xor(acc, 2, 4);
            acc += __shfl_xor(acc, 1, 4);
            const double r = acc - a.b[crow4];
            if (cl4 == 0) { rbs[crow4] = r; rb2 = r * r; }
            if constexpr (Detect) {
                if (cl4 == 0) { dby = a.b[crow4] * ys[crow4]; dmax = fabs(acc); }
            }
        }
        return rb2;
    };
    // r_c, d, q, v and the partial sums of ||r_c||^2, x.s, c.x  (Quad: the same column as prepare_kernel_body<..., Quad> of
    // vector_ops.h -- quad_rc, quad_theta / quad_bnd_theta, quad_objective; v keeps its formula with the new r_c and d)
    double ru2 = 0.0;                                   // bounded: this thread's share of ||r_u||^2 (residual_cols)
    double *DWp = nullptr, *DZp = nullptr;              // bounded: where direction() puts (dw, dz)
    auto residual_cols = [&](double& rc2, double& xs, double& cx) {
        for (int j = ctid; j < n; j += PD_THREADS) {
            const int pb = a.A.colptr[j], pe = a.A.colptr[j + 1];
            double w = 0.0;
            for (int p = pb; p < pe; ++p) w += a.A.cval[p] * ys[a.A.rowind[p]];
            const double xj = a.x[j], sj = a.s[j], cj = a.c[j];
            if constexpr (Free) {
                // the three kinds of column (free, on U, plain) choose values; the sums are updated once, straight-line, as below.
                // A free x_j may be 0 or negative: x_j s_j / x_j is formed on the other branch only.
                const double gj = g[j];
                double rcj, dj, r3 = 0.0, r4 = 0.0, ru_j2 = 0.0;
                double atyj = w;                                 // Detect: what the column gives the dual maximum ((A^T y - z)_j, free: |(A^T y)_j|)
                if (free_in(fr, j)) {
                    rcj = free_rc(w, cj, gj, xj); dj = free_theta(gj);
                    free_rhs_column<Bounded>(a, bd, j, dj, rcj);
                    if constexpr (Detect) atyj = detect_dual_free(w);
                } else {
                    r3 = xj * sj;
                    const double qj = r3 / xj;
                    rcj = quad_rc(w + sj - cj, gj, xj); dj = quad_theta(xj, sj, gj);
                    double vj = dj * (rcj - qj);
                    if constexpr (Bounded) {
                        const double uj = bd.u[j];
                        if (bnd_in(uj)) {
                            const double wj = bd.w[j], zj = bd.z[j];
                            const double ruj = xj + wj - uj;
                            rcj = quad_rc(w + sj - zj - cj, gj, xj); dj = quad_bnd_theta(xj, sj, wj, zj, gj); r4 = wj * zj; ru_j2 = ruj * ruj;
                            bd.qz[j] = r4 / wj;
                            vj = dj * (rcj - qj + (r4 - zj * ruj) / wj);
                            if constexpr (Detect) { duz += uj * zj; atyj = w - zj; dmxu = fmax(dmxu, xj); }
                        }
                    }
                    a.q[j] = qj; a.v[j] = vj;
                }
                a.rc[j] = rcj; a.d[j] = dj;
                rc2 += rcj * rcj; xs += r3; cx += quad_objective(cj, gj, xj);
                if constexpr (Bounded) { xs += r4; ru2 += ru_j2; }
                if constexpr (Detect) { dmaty = fmax(dmaty, atyj); dcxl += detect_linear(cj, xj); dmgx = fmax(dmgx, detect_curvature(gj, xj)); }
            } else if constexpr (Bounded && Detect && Quad) {
                // the Bounded branch below for a detecting quadratic handle: the same column, with the terms of the tests chosen inside
                // the branches and ALL accumulators updated once behind them (updated inside the branches, as the LP's detect variants
                // below do, duz / dmaty / dmxu were left in scratch memory: 24 bytes per lane)
                const double uj = bd.u[j], gj = g[j];
                double rcj = quad_rc(w + sj - cj, gj, xj), dj = quad_theta(xj, sj, gj), vj, r4 = 0.0, ru_j2 = 0.0;
                const double r3 = xj * sj, qj = r3 / xj;
                double atyj = w, uzj = 0.0, xuj = 0.0;
                if (bnd_in(uj)) {
                    const double wj = bd.w[j], zj = bd.z[j];
                    const double ruj = xj + wj - uj;
                    rcj = quad_rc(w + sj - zj - cj, gj, xj); dj = quad_bnd_theta(xj, sj, wj, zj, gj); r4 = wj * zj; ru_j2 = ruj * ruj;
                    bd.qz[j] = r4 / wj;
                    vj = dj * (rcj - qj + (r4 - zj * ruj) / wj);
                    uzj = uj * zj; atyj = w - zj; xuj = xj;
                } else {
                    vj = dj * (rcj - qj);
                }
                a.rc[j] = rcj; a.d[j] = dj; a.q[j] = qj; a.v[j] = vj;
                rc2 += rcj * rcj; xs += r3; xs += r4; cx += quad_objective(cj, gj, xj); ru2 += ru_j2;
                duz += uzj; dmaty = fmax(dmaty, atyj); dmxu = fmax(dmxu, xuj);
                dcxl += detect_linear(cj, xj); dmgx = fmax(dmgx, detect_curvature(gj, xj));
            } else if constexpr (Bounded) {
                // one straight-line update of the four sums for both kinds of column (with a `continue` per kind the
                // accumulators were left in scratch memory)
                const double uj = bd.u[j];
                double rcj = w + sj - cj, dj = xj / sj, vj, r4 = 0.0, ru_j2 = 0.0, gj = 0.0;
                if constexpr (Quad) { gj = g[j]; rcj = quad_rc(rcj, gj, xj); dj = quad_theta(xj, sj, gj); }
                const double r3 = xj * sj, qj = r3 / xj;
                if (bnd_in(uj)) {
                    const double wj = bd.w[j], zj = bd.z[j];
                    const double ruj = xj + wj - uj;
                    rcj = w + sj - zj - cj; dj = bnd_theta(xj, sj, wj, zj); r4 = wj * zj; ru_j2 = ruj * ruj;
                    if constexpr (Quad) { rcj = quad_rc(rcj, gj, xj); dj = quad_bnd_theta(xj, sj, wj, zj, gj); }
                    bd.qz[j] = r4 / wj;
                    vj = dj * (rcj - qj + (r4 - zj * ruj) / wj);
                    if constexpr (Detect) { duz += uj * zj; dmaty = fmax(dmaty, w - zj); dmxu = fmax(dmxu, xj); }
                } else {
                    vj = dj * (rcj - qj);
                    if constexpr (Detect) dmaty = fmax(dmaty, w);
                }
                a.rc[j] = rcj; a.d[j] = dj; a.q[j] = qj; a.v[j] = vj;
                rc2 += rcj * rcj; xs += r3; xs += r4; cx += Quad ? quad_objective(cj, gj, xj) : cj * xj; ru2 += ru_j2;
            } else if constexpr (Quad) {
                const double gj = g[j], rcj = quad_rc(w + sj - cj, gj, xj), dj = quad_theta(xj, sj, gj), r3 = xj * sj;
                a.rc[j] = rcj; a.d[j] = dj; a.q[j] = r3 / xj; a.v[j] = dj * (rcj - r3 / xj);
                rc2 += rcj * rcj; xs += r3; cx += quad_objective(cj, gj, xj);
                if constexpr (Detect) { dmaty = fmax(dmaty, w); dcxl += detect_linear(cj, xj); dmgx = fmax(dmgx, detect_curvature(gj, xj)); }
            } else {
                const double rcj = w + sj - cj, dj = xj / sj, r3 = xj * sj;
                a.rc[j] = rcj; a.d[j] = dj; a.q[j] = r3 / xj; a.v[j] = dj * (rcj - r3 / xj);
                rc2 += rcj * rcj; xs += r3; cx += cj * xj;
                if constexpr (Detect) dmaty = fmax(dmaty, w);
            }
        }
    };
    // stop test of check_optimality (main.py:162-173): thread 0, result in `go`
    // (Detect: ds = {b.y, u_U.z_U}, dm = {max (A^T y - z)_+, max |A x|, max x_U}, reduced over the workgroup; with Quad one more of each:
    //  ds[2] = the linear c.x, dm[3] = max g|x|, and the free columns' |A^T y| inside dm[0])
    auto stop_test = [&](double rb2, double rc2, double gap, double obj, const double* ds, const double* dm) {
        if (ctid == 0) {
            const double rb = sqrt(rb2), rcn = sqrt(rc2);
            sc->rb_norm = rb; sc->rc_norm = rcn; sc->gap = gap; sc->obj = obj;
            if (fabs(obj) < 1.7e308) sc->obj_last_finite = obj;
            double nmu = Bounded ? (double)(n + bd.nU) : (double)n;
            if constexpr (Free) nmu = free_pair_count<Bounded>(n, bd, fr);
            sc->mu = gap / nmu;
            sh[0] = gap / nmu;
            int cont_loop = 1;
            if (!sc->force) {
                const bool cont = (sc->e1 * (1.0 + sc->b_norm) < rb) || (sc->e2 * (1.0 + sc->c_norm) < rcn) || (sc->e3 < gap);
                if (!cont) {
                    const bool finite = (rb == rb) && (rcn == rcn) && (gap == gap) && (fabs(rb) < 1.7e308) &&
                                        (fabs(rcn) < 1.7e308) && (fabs(gap) < 1.7e308);
                    sc->status = finite ? 1 : 3; sc->done = 1; cont_loop = 0;
                } else if (Detect && !Quad && detect_fire(dt, sc, ds[0] - ds[1], dm[0], -obj, fmax(dm[1], dm[2]))) {
                    cont_loop = 0;
                } else if (Detect && Quad && detect_fire(dt, sc, ds[0] - ds[1], dm[0], -ds[2], fmax(fmax(dm[1], dm[2]), dm[3]))) {
                    cont_loop = 0;
                } else if (sc->k >= sc->max_iter) {
                    sc->status = 2; sc->done = 1; cont_loop = 0;
                }
            }
            go = cont_loop;
        }
    };
    // t1 = -r_b - A v ; z = inv(L) t1 ; dys = inv(L)^T z       (both matvecs with X = inv(L) from LDS)
    auto solve_normal = [&]() {
        if (crow4 < m) {
            const int pb = a.A.rowptr[crow4], pe = a.A.rowptr[crow4 + 1];
            double acc = 0.0;
            for (int p = pb + cl4; p < pe; p += 4) acc += a.A.rval[p] * a.v[a.A.colind[p]];
            acc += __shfl_xor(acc, 2, 4);
            acc += __shfl_xor(acc, 1, 4);
            if (cl4 == 0) t1s[crow4] = -rbs[crow4] - acc;
        }
        __syncthreads();
        if (crow4 < mt) {                                   // z_i = sum_{k <= i} X[i][k] t1_k,  X[i][k] at W[k*WLD + i + 1]
            double acc = 0.0;
            for (int k = cl4; k <= crow4; k += 4) acc += W[k * WLD + crow4 + 1] * t1s[k];
            acc += __shfl_xor(acc, 2, 4);
            acc += __shfl_xor(acc, 1, 4);
            if (cl4 == 0) zs[crow4] = acc;
        }
        __syncthreads();
        if (crow4 < mt) {                                   // dy_k = sum_{i >= k} X[i][k] z_i
            double acc = 0.0;
            for (int i = crow4 + cl4; i < mt; i += 4) acc += W[crow4 * WLD + i + 1] * zs[i];
            acc += __shfl_xor(acc, 2, 4);
            acc += __shfl_xor(acc, 1, 4);
            if (cl4 == 0) dys[crow4] = acc;
        }
        __syncthreads();
    };
    // direction_column over the columns with (A^T dy)_j from dys; this thread's ratio-test minima
    auto direction = [&](double* DX, double* DS, double& minp, double& mind) {
        for (int j = ctid; j < n; j += PD_THREADS) {
            const int pb = a.A.colptr[j], pe = a.A.colptr[j + 1];
            double w = 0.0;
            for (int p = pb; p < pe; ++p) w += a.A.cval[p] * dys[a.A.rowind[p]];
            const double xj = a.x[j], sj = a.s[j];
            if constexpr (Free) {
                if (free_in(fr, j)) free_direction_column<Bounded>(a, j, w, DX, DS, DWp, DZp);
                else direction_column<Bounded>(a, bd, j, w, DX, DS, DWp, DZp, xj, sj, minp, mind);
            } else direction_column<Bounded>(a, bd, j, w, DX, DS, DWp, DZp, xj, sj, minp, mind);
        }
    };

    int steps = 0;
    for (;;) {
        // ---------------------------------------------------------------- residuals + stop test
        if constexpr (Detect && Quad) asm volatile("" : "+v"(ctid), "+v"(crow4), "+v"(cl4));
        double r4[4] = {0.0, 0.0, 0.0, 0.0};               // ||r_b||^2, ||r_c||^2, x.s, c.x
        r4[0] = residual_rows();
        if constexpr (Bounded) ru2 = 0.0;
        residual_cols(r4[1], r4[2], r4[3]);
        if constexpr (Bounded) r4[0] += ru2;
        block_reduce512<4, false, Detect && Quad>(r4, red);
        constexpr int NS = (Detect && Quad) ? 3 : 2, NM = (Detect && Quad) ? 4 : 3;
        double ds[NS] = {}, dm[NM] = {};
        if constexpr (Detect) {
            ds[0] = dby; ds[1] = duz;
            if constexpr (Quad) ds[2] = dcxl;
            block_reduce512<NS, false, Detect && Quad>(ds, red);
            dm[0] = -dmaty; dm[1] = -dmax; dm[2] = -dmxu;                    // max = -min of the negated values
            if constexpr (Quad) dm[3] = -dmgx;
            block_reduce512<NM, true, Detect && Quad>(dm, red);
#pragma unroll
            for (int q = 0; q < NM; ++q) dm[q] = -dm[q];
            duz = 0.0; dmaty = 0.0; dmxu = 0.0;
            if constexpr (Quad) { dcxl = 0.0; dmgx = 0.0; }
        }
        stop_test(r4[0], r4[1], r4[2], r4[3], ds, dm);
        __syncthreads();
        if (!go || steps >= a.max_steps) break;
        const double mu = sh[0];

        // ---------------------------------------------------------------- B = A diag(d) A^T into W, guarded Cholesky
        for (int idx = ctid; idx < mt * WLD; idx += PD_THREADS) W[idx] = 0.0;
        __syncthreads();
        double mx[1] = {-1.7976931348623157e308};
        for (int e = ctid; e < a.nb; e += PD_THREADS) {
            const int i = a.bi[e], k = a.bk[e];
            double acc = 0.0;
            for (int t = a.bptr[e]; t < a.bptr[e + 1]; ++t) acc += a.bcoef[t] * a.d[a.bcol[t]];
            W[i * WLD + k] = acc;
            if (i != k && (i >> 4) == (k >> 4)) W[k * WLD + i] = acc;       // diagonal tiles are held symmetric
            if (i == k) mx[0] = (acc > mx[0]) ? acc : mx[0];                 // NaN never wins
        }
        if (ctid >= m && ctid < mt) W[ctid * WLD + ctid] = 1.0;                  // padding rows of the last tile
        {   // max over the TRUE rows (fmax would drop a NaN as well); -max of negated values = max
            double ng[1] = {-mx[0]};
            block_reduce512<1, true, Detect && Quad>(ng, red);
            mx[0] = -ng[0];
        }
        if (a.shift_rel != 0.0 && ctid < mt) W[ctid * WLD + ctid] += a.shift_rel * mx[0];
        __syncthreads();
        const int nfix = potrf_lds<false, NoEarlyWork, Detect && Quad>(W, dinv_s, nt, a.eps * mx[0], a.big, m, nullptr);
        if (ctid == 0) {
            sc->maxdiag = mx[0];
            const int fx = sc->fixed + nfix;
            sc->fixed = fx;
            int leave = 0;
            if (sc->k == 0) {
                sc->fixed_first = fx;
                if (a.auto_reg && (double)fx > 0.05 * (double)m) {          // > 5 % dependent rows: restart with the shift
                    sc->status = IPM_STATUS_NEEDS_SHIFT; sc->done = 1; leave = 1;
                }
            }
            go = !leave;
        }
        __syncthreads();
        if (!go) break;

        // ---------------------------------------------------------------- predictor
        solve_normal();
        double mn[2] = {1.0, 1.0};
        if constexpr (Bounded) { DWp = bd.dwa; DZp = bd.dza; }
        direction(a.dxa, a.dsa, mn[0], mn[1]);
        block_reduce512<2, true, Detect && Quad>(mn, red);
        double aap = mn[0], aad = mn[1];
        if constexpr (Quad) aap = aad = quad_step(aap, aad);                 // one step length
        double ma[1] = {0.0};
        for (int j = ctid; j < n; j += PD_THREADS) {
            if constexpr (Free) { if (!free_in(fr, j)) mu_aff_column<Bounded>(a, bd, j, aap, aad, ma[0]); }
            else mu_aff_column<Bounded>(a, bd, j, aap, aad, ma[0]);
        }
        block_reduce512<1, false, Detect && Quad>(ma, red);
        const Centring ct = centring<Bounded>(ma[0], mu, Free ? n - fr.nfree : n, bd);      // (Free: free_pair_count pairs)
        const double sm = ct.sigma * mu;
        // ---------------------------------------------------------------- corrector, same factor
        for (int j = ctid; j < n; j += PD_THREADS) {
            if constexpr (Free) {
                if (free_in(fr, j)) free_rhs_column<Bounded>(a, bd, j, a.d[j], a.rc[j]);
                else corrector_column<Bounded>(a, bd, j, sm);
            } else corrector_column<Bounded>(a, bd, j, sm);
        }
        __syncthreads();
        solve_normal();
        double mc[2] = {1.0, 1.0};
        if constexpr (Bounded) { DWp = bd.dw; DZp = bd.dz; }
        direction(a.dx, a.ds, mc[0], mc[1]);
        block_reduce512<2, true, Detect && Quad>(mc, red);
        // ---------------------------------------------------------------- damped step
        const double eta = sc->eta;
        double ap = damped_step(eta, mc[0]), ad = damped_step(eta, mc[1]);
        if constexpr (Quad) ap = ad = quad_step(ap, ad);
        for (int j = ctid; j < n; j += PD_THREADS) {
            if constexpr (Free) {
                if (free_in(fr, j)) free_update_column(a, j, ap);
                else update_column<Bounded>(a, bd, j, ap, ad);
            } else update_column<Bounded>(a, bd, j, ap, ad);
        }
        if (ctid < m) ys[ctid] += ad * dys[ctid];
        if (ctid == 0) {
            record_iteration(sc, a.hist, mu, ct.sigma, aap, aad, ap, ad);
            sc->mu_aff = ct.mu_aff; sc->sigma = ct.sigma; sc->alpha_aff_p = aap; sc->alpha_aff_d = aad;
        }
        ++steps;
        __syncthreads();
    }
    if (ctid < m) a.y[ctid] = ys[ctid];
}

__global__ __launch_bounds__(PD_THREADS) void small_lp_kernel(SmallLP a) { small_lp_body<false>(a, BndArgs{}); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_bounded_kernel(SmallLP a, BndArgs bd) { small_lp_body<true>(a, bd); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_detect_kernel(SmallLP a, DetArgs dt) { small_lp_body<false, true>(a, BndArgs{}, dt); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_bounded_detect_kernel(SmallLP a, BndArgs bd, DetArgs dt) { small_lp_body<true, true>(a, bd, dt); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_kernel(SmallLP a, const double* g) { small_lp_body<false, false, true>(a, BndArgs{}, DetArgs{}, g); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_bounded_kernel(SmallLP a, BndArgs bd, const double* g) { small_lp_body<true, false, true>(a, bd, DetArgs{}, g); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_free_kernel(SmallLP a, const double* g, FreeArgs fr) { small_lp_body<false, false, true, true>(a, BndArgs{}, DetArgs{}, g, fr); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_bounded_free_kernel(SmallLP a, BndArgs bd, const double* g, FreeArgs fr) { small_lp_body<true, false, true, true>(a, bd, DetArgs{}, g, fr); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_detect_kernel(SmallLP a, DetArgs dt, const double* g) { small_lp_body<false, true, true>(a, BndArgs{}, dt, g); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_bounded_detect_kernel(SmallLP a, BndArgs bd, DetArgs dt, const double* g) { small_lp_body<true, true, true>(a, bd, dt, g); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_free_detect_kernel(SmallLP a, DetArgs dt, const double* g, FreeArgs fr) { small_lp_body<false, true, true, true>(a, BndArgs{}, dt, g, fr); }
__global__ __launch_bounds__(PD_THREADS) void small_qp_bounded_free_detect_kernel(SmallLP a, BndArgs bd, DetArgs dt, const double* g, FreeArgs fr) { small_lp_body<true, true, true, true>(a, bd, dt, g, fr); }

// ------------------------------------------------------------------------------- batch of small LPs (ipm_solve_small_batch)
// One launch, one workgroup per LP: workgroup blockIdx.x reads item blockIdx.x of a table in device memory -- the arguments the
// single-LP kernel gets in its kernel-argument segment -- and runs the SAME body on it.  The workgroups never talk to each other
// (no atomics, no polling), so the dispatcher may run them in any order and in any number of rounds over the compute units; an LP's
// arithmetic is that of its one-at-a-time launch, bit for bit.  The body keeps ~133 KB of static LDS per instantiation, so the twelve
// variants stay twelve kernels: the host sorts the table by variant and launches one grid per variant present.
enum { SMALL_PLAIN = 0, SMALL_BOUNDED = 1, SMALL_DETECT = 2, SMALL_BOUNDED_DETECT = 3, SMALL_QUAD = 4, SMALL_BOUNDED_QUAD = 5, SMALL_FREE_QUAD = 6,
       SMALL_BOUNDED_FREE_QUAD = 7,
       // a detecting handle with a quadratic term (IPM_FLAG_DETECT_QUADRATIC): + 1 bounded, + 2 free columns
       SMALL_QUAD_DETECT = 8, SMALL_BOUNDED_QUAD_DETECT = 9, SMALL_FREE_QUAD_DETECT = 10, SMALL_BOUNDED_FREE_QUAD_DETECT = 11, SMALL_NVARIANTS = 12 };
struct SmallItem {
    SmallLP lp;
    BndArgs bd;
    DetArgs dt;
    const double* g;                                     // the quadratic diagonal of a SMALL_*QUAD item (the handle's quad_g), else NULL
    FreeArgs fr;                                         // the marks of a SMALL_*FREE_QUAD item (the handle's free_mark), else {NULL, 0}
    double eta;                                          // the handle's step damping (small_batch_params_kernel)
    int variant;                                         // SMALL_*
    int index;                                           // position of the handle in the caller's array (the gathered record goes there)
};

// the index is the workgroup's own: the loads are wave-uniform and the item ends up in scalar registers like kernel arguments do
template <bool Bounded, bool Detect, bool Quad = false, bool Free = false>
__device__ __forceinline__ void small_lp_batch_body(const SmallItem* __restrict__ items) {
    const SmallItem it = items[blockIdx.x];
    if constexpr (Free) small_lp_body<Bounded, Detect, Quad, true>(it.lp, it.bd, it.dt, it.g, it.fr);
    else small_lp_body<Bounded, Detect, Quad>(it.lp, it.bd, it.dt, it.g);
}
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<false, false>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_bounded_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<true, false>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_detect_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<false, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_bounded_detect_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<true, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_quad_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<false, false, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_bounded_quad_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<true, false, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_free_quad_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<false, false, true, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_bounded_free_quad_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<true, false, true, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_quad_detect_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<false, true, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_bounded_quad_detect_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<true, true, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_free_quad_detect_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<false, true, true, true>(items); }
__global__ __launch_bounds__(PD_THREADS) void small_lp_batch_bounded_free_quad_detect_kernel(const SmallItem* __restrict__ items) { small_lp_batch_body<true, true, true, true>(items); }

// The variant table of the one-workgroup path (host side; vector_ops.h says how a class is written): row SMALL_x serves the class
// `flags` with the single-LP kernel `one`, launched on a host item with its arguments bound by type, and the batch kernel `batch` on
// a device table of items.  The ids keep their values: a batch launches one grid per variant in id order.
template <> struct Pick<SmallLP, SmallItem> { static SmallLP of(const SmallItem& it) { return it.lp; } };
template <> struct Pick<BndArgs, SmallItem> { static BndArgs of(const SmallItem& it) { return it.bd; } };
template <> struct Pick<DetArgs, SmallItem> { static DetArgs of(const SmallItem& it) { return it.dt; } };
template <> struct Pick<const double*, SmallItem> { static const double* of(const SmallItem& it) { return it.g; } };
template <> struct Pick<FreeArgs, SmallItem> { static FreeArgs of(const SmallItem& it) { return it.fr; } };
struct SmallRow {
    int id; unsigned flags; const char *name, *batch_name;
    void (*one)(hipStream_t, const SmallItem&); void (*batch)(const SmallItem*);
};
template <auto K> static void small_one(hipStream_t st, const SmallItem& it) { launch_bound(K, dim3(1), dim3(PD_THREADS), st, it); }
#define SMALL_ROW(ID, FLAGS, ONE, BATCH) {ID, FLAGS, #ONE, #BATCH, small_one<ONE>, BATCH}
constexpr SmallRow SMALL_ROWS[] = {
    SMALL_ROW(SMALL_PLAIN, 0, small_lp_kernel, small_lp_batch_kernel),
    SMALL_ROW(SMALL_BOUNDED, V_B, small_lp_bounded_kernel, small_lp_batch_bounded_kernel),
    SMALL_ROW(SMALL_DETECT, V_D, small_lp_detect_kernel, small_lp_batch_detect_kernel),
    SMALL_ROW(SMALL_BOUNDED_DETECT, V_B | V_D, small_lp_bounded_detect_kernel, small_lp_batch_bounded_detect_kernel),
    SMALL_ROW(SMALL_QUAD, V_Q, small_qp_kernel, small_lp_batch_quad_kernel),
    SMALL_ROW(SMALL_BOUNDED_QUAD, V_B | V_Q, small_qp_bounded_kernel, small_lp_batch_bounded_quad_kernel),
    SMALL_ROW(SMALL_FREE_QUAD, V_Q | V_F, small_qp_free_kernel, small_lp_batch_free_quad_kernel),
    SMALL_ROW(SMALL_BOUNDED_FREE_QUAD, V_B | V_Q | V_F, small_qp_bounded_free_kernel, small_lp_batch_bounded_free_quad_kernel),
    SMALL_ROW(SMALL_QUAD_DETECT, V_D | V_Q, small_qp_detect_kernel, small_lp_batch_quad_detect_kernel),
    SMALL_ROW(SMALL_BOUNDED_QUAD_DETECT, V_B | V_D | V_Q, small_qp_bounded_detect_kernel, small_lp_batch_bounded_quad_detect_kernel),
    SMALL_ROW(SMALL_FREE_QUAD_DETECT, V_D | V_Q | V_F, small_qp_free_detect_kernel, small_lp_batch_free_quad_detect_kernel),
    SMALL_ROW(SMALL_BOUNDED_FREE_QUAD_DETECT, V_B | V_D | V_Q | V_F, small_qp_bounded_free_detect_kernel, small_lp_batch_bounded_free_quad_detect_kernel),
};
// the row of a class (its index in `rows` is its id), -1 for none
template <int N> constexpr int small_row_of(const SmallRow (&rows)[N], unsigned bits) {
    for (int i = 0; i < N; ++i) if (rows[i].flags == bits) return i;
    return -1;
}
// every row sits at its id, and every legal class has its row (flags are distinct: N legal classes, N rows)
template <int N> constexpr bool small_rows_ok(const SmallRow (&rows)[N], unsigned mask, int legal) {
    for (int i = 0; i < N; ++i) if (rows[i].id != i || !variant_legal(rows[i].flags) || (rows[i].flags & ~mask)) return false;
    int n = 0;
    for (unsigned c = 0; c <= mask; ++c) if ((c & ~mask) == 0 && variant_legal(c) && small_row_of(rows, c) >= 0) ++n;
    return n == N && N == legal;
}
// (the one-workgroup path serves no LP free set, V_L: ipm_set_free_lp_columns keeps such a handle on the multi-kernel path)
static_assert(small_rows_ok(SMALL_ROWS, V_ALL & ~V_L, SMALL_NVARIANTS), "SMALL_ROWS: one row per legal class, each at its SMALL_* id");

// start_solve(force = 0, reset = 1) for every item, as set_params_kernel does for one LP: one thread per item
__global__ __launch_bounds__(256) void small_batch_params_kernel(const SmallItem* __restrict__ items, int n, double e1, double e2, double e3, int max_iter) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    start_solve(items[i].lp.sc, e1, e2, e3, items[i].eta, max_iter, 0, 1);
}

// ------------------------------------------------------------------------------- Mehrotra's starting point (ipm_init_state_mehrotra)
// The start of a small LP in one launch of one workgroup: B = A A^T from the product list with d = 1 into the same
// LDS image W the loop uses, the same guarded potrf_lds, both solves as matvecs with inv(L) from LDS, (A^T u)_j and (A^T y)_j as CSC
// dot products with the m-vector in LDS, the shifts and the balance from block_reduce512.  The per-column rules are
// iteration_rules.h (start_*), shared with the multi-kernel path.  No LDS beyond what small_lp_body declares; the n-vectors stay in
// global memory and every thread keeps its own columns (j = tid, tid + 512, ...) from the first pass to the last, so the passes
// need no barrier between them beyond those of the reductions.  Leaves the guarded-pivot count in sc->fixed.
template <bool Bounded>
__device__ __forceinline__ void small_start_body(SmallLP a, BndArgs bd) {
    __shared__ __attribute__((aligned(16))) double W[NB * WLD];
    __shared__ double dinv_s[NB];
    __shared__ double ys[NB], t1s[NB], zs[NB];
    __shared__ double red[8 * 4];

    const int tid = threadIdx.x;
    const int m = a.m, n = a.n, nt = a.nt, mt = 16 * a.nt;
    const int row4 = tid >> 2, l4 = tid & 3;            // 4 lanes per row of A / of the triangular matvecs
    Scalars* sc = a.sc;

    // ---------------------------------------------------------------- B = A A^T into W, guarded Cholesky (as small_lp_body, d = 1)
    for (int idx = tid; idx < mt * WLD; idx += PD_THREADS) W[idx] = 0.0;
    __syncthreads();
    double mx[1] = {-1.7976931348623157e308};
    for (int e = tid; e < a.nb; e += PD_THREADS) {
        const int i = a.bi[e], k = a.bk[e];
        double acc = 0.0;
        for (int t = a.bptr[e]; t < a.bptr[e + 1]; ++t) acc += a.bcoef[t];
        W[i * WLD + k] = acc;
        if (i != k && (i >> 4) == (k >> 4)) W[k * WLD + i] = acc;
        if (i == k) mx[0] = (acc > mx[0]) ? acc : mx[0];
    }
    if (tid >= m && tid < mt) W[tid * WLD + tid] = 1.0;
    {
        double ng[1] = {-mx[0]};
        block_reduce512<1, true>(ng, red);
        mx[0] = -ng[0];
    }
    if (a.shift_rel != 0.0 && tid < mt) W[tid * WLD + tid] += a.shift_rel * mx[0];
    __syncthreads();
    const int nfix = potrf_lds<false>(W, dinv_s, nt, a.eps * mx[0], a.big, m, nullptr);
    if (tid == 0) { sc->maxdiag = mx[0]; sc->fixed = nfix; }

    // out = (L L^T)^-1 t1s with X = inv(L) from LDS (the two matvecs of small_lp_body's solve_normal)
    auto solve = [&](double* out) {
        __syncthreads();
        if (row4 < mt) {
            double acc = 0.0;
            for (int k = l4; k <= row4; k += 4) acc += W[k * WLD + row4 + 1] * t1s[k];
            acc += __shfl_xor(acc, 2, 4);
            acc += __shfl_xor(acc, 1, 4);
            if (l4 == 0) zs[row4] = acc;
        }
        __syncthreads();
        if (row4 < mt) {
            double acc = 0.0;
            for (int i = row4 + l4; i < mt; i += 4) acc += W[row4 * WLD + i + 1] * zs[i];
            acc += __shfl_xor(acc, 2, 4);
            acc += __shfl_xor(acc, 1, 4);
            if (l4 == 0) out[row4] = acc;
        }
        __syncthreads();
    };
    auto at_dot = [&](int j) {                            // (A^T ys)_j
        double w = 0.0;
        for (int p = a.A.colptr[j]; p < a.A.colptr[j + 1]; ++p) w += a.A.cval[p] * ys[a.A.rowind[p]];
        return w;
    };

    // ---------------------------------------------------------------- x = A^T (A A^T)^-1 b
    if (tid < NB) t1s[tid] = tid < m ? a.b[tid] : 0.0;
    solve(ys);
    double mn[2] = {__builtin_inf(), __builtin_inf()};
    for (int j = tid; j < n; j += PD_THREADS) start_primal_column<Bounded>(a, bd, j, at_dot(j), mn[0]);
    __syncthreads();                                      // ys is rewritten below
    // ---------------------------------------------------------------- y = (A A^T)^-1 A c ; r = c - A^T y
    if (tid < NB) t1s[tid] = 0.0;
    __syncthreads();
    if (row4 < m) {
        double acc = 0.0;
        for (int p = a.A.rowptr[row4] + l4; p < a.A.rowptr[row4 + 1]; p += 4) acc += a.A.rval[p] * a.c[a.A.colind[p]];
        acc += __shfl_xor(acc, 2, 4);
        acc += __shfl_xor(acc, 1, 4);
        if (l4 == 0) t1s[row4] = acc;
    }
    solve(ys);
    for (int j = tid; j < n; j += PD_THREADS) start_dual_column<Bounded>(a, bd, j, a.c[j] - at_dot(j), mn[1]);
    // ---------------------------------------------------------------- shifts, balance or fallback
    block_reduce512<2, true>(mn, red);
    const double dp = start_shift(mn[0]), dd = start_shift(mn[1]);
    double t3[3] = {0.0, 0.0, 0.0};                       // x.s + w.z, sum s + sum z_U, sum x + sum w_U
    for (int j = tid; j < n; j += PD_THREADS) start_shift_column<Bounded>(a, bd, j, dp, dd, t3[0], t3[1], t3[2]);
    block_reduce512<3, false>(t3, red);
    const double xs = 0.5 * t3[0];
    if (start_degenerate(xs, t3[1], t3[2])) {             // the same reduced values in every thread: all take this branch or none
        for (int j = tid; j < n; j += PD_THREADS) start_reference_column<Bounded>(a, bd, j);
        if (tid < m) a.y[tid] = 1.0;
        return;
    }
    const double pc = xs / t3[1];
    double sx[1] = {0.0};
    for (int j = tid; j < n; j += PD_THREADS) start_primal_correct_column<Bounded>(a, bd, j, pc, sx[0]);
    block_reduce512<1, false>(sx, red);
    const double dc = xs / sx[0];
    for (int j = tid; j < n; j += PD_THREADS) start_dual_correct_column<Bounded>(a, bd, j, dc);
    if (tid < m) a.y[tid] = ys[tid];
}
__global__ __launch_bounds__(PD_THREADS) void small_start_kernel(SmallLP a) { small_start_body<false>(a, BndArgs{}); }
__global__ __launch_bounds__(PD_THREADS) void small_start_bounded_kernel(SmallLP a, BndArgs bd) { small_start_body<true>(a, bd); }
__global__ __launch_bounds__(PD_THREADS) void small_start_batch_kernel(const SmallItem* __restrict__ items) { const SmallItem it = items[blockIdx.x]; small_start_body<false>(it.lp, it.bd); }
__global__ __launch_bounds__(PD_THREADS) void small_start_batch_bounded_kernel(const SmallItem* __restrict__ items) { const SmallItem it = items[blockIdx.x]; small_start_body<true>(it.lp, it.bd); }
// the start tells plain (row 0) from bounded (row 1) only: the tests of a Detect handle and the term play no part in it
constexpr SmallRow SMALL_START_ROWS[] = {
    SMALL_ROW(0, 0, small_start_kernel, small_start_batch_kernel),
    SMALL_ROW(1, V_B, small_start_bounded_kernel, small_start_batch_bounded_kernel),
};
static_assert(small_rows_ok(SMALL_START_ROWS, V_B, 2), "SMALL_START_ROWS: plain, bounded");

// every item's scalar record into ONE contiguous array (slot = the item's index): the host reads all statistics with one copy
__global__ __launch_bounds__(256) void small_batch_gather_kernel(const SmallItem* __restrict__ items, int n, Scalars* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[items[i].index] = *items[i].lp.sc;
}

}  // namespace ipm
