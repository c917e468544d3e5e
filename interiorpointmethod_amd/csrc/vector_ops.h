// vector_ops.h -- the HBM-bound part of one interior-point iteration (gfx950): dense GEMV
// passes over A and the fused elementwise/reduction kernels between them, one kernel per step.
//
// The state of a solve and the rules of the iteration that this path shares with the one-workgroup loop (small_lp.h) are in
// iteration_rules.h: direction recovery and ratio tests, mu_aff, centring, corrector column, damped step and update, iteration
// record, start of a solve.  The predictor column (prepare_kernel) and the stop decision (stop_test_kernel) are still written out
// here AND in small_lp.h (main.py:66-73, :162-173, :223-228 of the reference repo); iteration_rules.h says why.  Beyond that, this
// file owns what this path does around the rules: grid-stride loops over global memory, (A^T y)_j from the GEMV-T partials
// (col_sum), and the reductions.  All reductions are two-level with a fixed order (per-block partials, then every consumer
// re-sums the <= 64 partials in index order), so a solve is bitwise reproducible; no fp64
// atomics are used.  Scalars (norms, alpha, sigma, mu, stop flag) never leave the device
// inside an iteration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gemm_nt_f64.h"
#include "handoff.h"
#include "iteration_rules.h"

namespace ipm {

constexpr int VBLK = 256;        // threads per vector-kernel block
constexpr int MAXPART = 64;      // max blocks (= partials) of a vector kernel

// partial-sum slots (each MAXPART doubles)
enum { P_RC2 = 0, P_XS, P_CX, P_RB2, P_MINP_AFF, P_MIND_AFF, P_MUAFF, P_MINP, P_MIND, P_NSLOT };
// slots of the infeasibility tests (Detect instantiations only): b.y, u_U.z_U, max (A^T y - z)_+, max |A x|, max x_U
enum { P_BY = P_NSLOT, P_UZ, P_MATY, P_MAX, P_MXU, P_NSLOT_DETECT };
// two more of a quadratic handle's tests (Detect with Quad, IPM_FLAG_DETECT_QUADRATIC), behind every slot above: the LINEAR c.x (a sum:
// P_CX of such a handle carries 1/2 g x^2) and max_j g_j |x_j|.  The free columns' |(A^T y)_j| goes into P_MATY.
enum { P_CXL = P_NSLOT_DETECT, P_MGX, P_NSLOT_DETECT_QUAD };

__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = VBLK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double block_min(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = VBLK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmin(red[tid], red[tid + s]);   // fmin drops NaN like np.min never sees it
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double block_max(double v, double* red) { return -block_min(-v, red); }
__device__ __forceinline__ double sum_partials(const double* part, int slot, int nblk) {
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += part[slot * MAXPART + i];
    return s;
}
__device__ __forceinline__ double min_partials(const double* part, int slot, int nblk) {
    double s = 1.0;                                  // min(np.append(ratios, 1)), main.py:309
    for (int i = 0; i < nblk; ++i) s = fmin(s, part[slot * MAXPART + i]);
    return s;
}
__device__ __forceinline__ double max_partials(const double* part, int slot, int nblk) {
    double s = 0.0;                                  // the maxima are of non-negative quantities
    for (int i = 0; i < nblk; ++i) s = fmax(s, part[slot * MAXPART + i]);
    return s;
}

// ---------------------------------------------------------------------------------------
// GEMV, A row-major [mp][np] (zero padded).
// ---------------------------------------------------------------------------------------
// out[i] = sa * (A[i,:] . v) + sb * add[i]   -- one wave per row, 16 B per lane per step.
__device__ __forceinline__ void gemv_n_kernel_body(const double* __restrict__ A, int64_t lda, int mp,
                                                     int np, const double* __restrict__ v, double sa,
                                                     double sb, const double* __restrict__ add,
                                                     double* out, const int* done, const unsigned bx_, const unsigned gx_) {
    if (done && *done) return;
    const int lane = threadIdx.x & 63;
    const int row = bx_ * 4 + (threadIdx.x >> 6);
    if (row >= mp) return;
    const double* ar = A + (int64_t)row * lda;
    double acc0 = 0.0, acc1 = 0.0;
    for (int c = lane * 2; c < np; c += 128) {
        f64x2 a2 = *reinterpret_cast<const f64x2*>(ar + c);
        f64x2 v2 = *reinterpret_cast<const f64x2*>(v + c);
        acc0 += a2.x * v2.x;
        acc1 += a2.y * v2.y;
    }
    double s = acc0 + acc1;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[row] = sa * s + (add ? sb * add[row] : 0.0);
}
__global__ __launch_bounds__(256) void gemv_n_kernel(const double* __restrict__ A, int64_t lda, int mp,
                                                     int np, const double* __restrict__ v, double sa,
                                                     double sb, const double* __restrict__ add,
                                                     double* out, const int* done) { gemv_n_kernel_body(A, lda, mp, np, v, sa, sb, add, out, done, blockIdx.x, gridDim.x); }

// part[rc][c] = sum_{r in chunk rc} A[r][c] * u[r]  -- grid (ceil(np/512), RC); 2 columns/thread.
__device__ __forceinline__ void gemv_t_kernel_body(const double* __restrict__ A, int64_t lda, int rows_per_chunk,
                                                     int np, const double* __restrict__ u, double* part,
                                                     const int* done, const unsigned bx_, const unsigned by_) {
    if (done && *done) return;
    const int c = (bx_ * 256 + threadIdx.x) * 2;
    if (c >= np) return;
    const int r0 = by_ * rows_per_chunk;
    double a0 = 0.0, a1 = 0.0;
    const double* ap = A + (int64_t)r0 * lda + c;
#pragma unroll 8
    for (int r = 0; r < rows_per_chunk; ++r) {
        f64x2 a2 = *reinterpret_cast<const f64x2*>(ap + (int64_t)r * lda);
        double ur = u[r0 + r];
        a0 += a2.x * ur;
        a1 += a2.y * ur;
    }
    *reinterpret_cast<f64x2*>(part + (int64_t)by_ * np + c) = (f64x2){a0, a1};
}
__global__ __launch_bounds__(256) void gemv_t_kernel(const double* __restrict__ A, int64_t lda, int rows_per_chunk,
                                                     int np, const double* __restrict__ u, double* part,
                                                     const int* done) { gemv_t_kernel_body(A, lda, rows_per_chunk, np, u, part, done, blockIdx.x, blockIdx.y); }

// The same two kernels with a progress signal at their entry (handoff_signal_at_entry): the backward sweep of the grouped solve
// launches them where the kernel in front has made a range of rows of its result final, and the pieces of A^T dy that wait for
// those rows on the residual stream are released without an event or a launch of their own (host_factor_solve.h: SweepHook).
__global__ __launch_bounds__(256) void gemv_n_signal_kernel(const double* __restrict__ A, int64_t lda, int mp,
                                                            int np, const double* __restrict__ v, double sa,
                                                            double sb, const double* __restrict__ add,
                                                            double* out, const int* done, unsigned* progress, unsigned value) {
    handoff_signal_at_entry(progress, value);
    gemv_n_kernel_body(A, lda, mp, np, v, sa, sb, add, out, done, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(256) void gemv_t_signal_kernel(const double* __restrict__ A, int64_t lda, int rows_per_chunk,
                                                            int np, const double* __restrict__ u, double* part,
                                                            const int* done, unsigned* progress, unsigned value) {
    handoff_signal_at_entry(progress, value);
    gemv_t_kernel_body(A, lda, rows_per_chunk, np, u, part, done, blockIdx.x, blockIdx.y);
}

struct VecArgs {
    int m, n, np, rc_chunks;       // true sizes, padded n, number of gemv_t row chunks
    int nblk;                      // blocks of the vector kernels (<= MAXPART)
    const double* atp;             // gemv_t partials [rc_chunks][np]
    double *x, *y, *s;
    const double *b, *c;
    double *rb, *rc, *d, *v, *q;
    double *dxa, *dya, *dsa, *dx, *dy, *ds;
    double* part;                  // [P_NSLOT][MAXPART]
    Scalars* sc;
    IterRec* hist;                 // [HIST_CAP] ring of per-iteration records
};

// ------------------------------------------------------------------------------- class variants (host side)
// A handle's problem class is five switches, and every step of the iteration has one kernel per class it tells apart.  Which kernel
// serves which class is stated ONCE per step, in a table directly below the step's __global__ wrappers (here and in small_lp.h):
//     #define X_VARIANTS(U, T)  U(classes, kernel) ... T(classes, lockstep twin type) ...
// a row names its kernel once, says which classes it serves (V_AT(switches), or-ed where it serves several), and is either an untwinned
// kernel (U) or a lockstep twin type (T: lockstep.h, LsTwin<T>, which names the single-LP kernel).  X_FLAGS are the switches the step
// tells apart; the look-up masks the others off.  The host expands the lists into its launch tables (host_residuals.h), where a
// static_assert holds every table to "each legal class is served by exactly one row"; ipm_debug_step_kernel reads them back.
struct StepVariant {
    bool bounded, detect, quad, free;      // ipm_set_bounds, IPM_FLAG_DETECT_INFEASIBILITY, ipm_set_quadratic, ipm_set_free_columns
    bool free_lp = false;                  // ipm_set_free_lp_columns (the fifth switch, V_L)
};
enum : unsigned { V_B = 1, V_D = 2, V_Q = 4, V_F = 8, V_L = 16, V_ALL = 31 };
constexpr unsigned variant_bits(StepVariant v) {
    return (v.bounded ? V_B : 0u) | (v.detect ? V_D : 0u) | (v.quad ? V_Q : 0u) | (v.free ? V_F : 0u) | (v.free_lp ? V_L : 0u);
}
// THE legality rule of a class: a free column needs curvature, so free implies quad (check_ready and the small batch's own check
// refuse a handle in the other state before anything is launched); an LP free column borrows its curvature from the proximal term
// and lives on a plain or bounded LP handle only -- no quadratic term, no free columns with curvature, no infeasibility tests
// (the setters refuse every such pair in both orders of the calls)
constexpr bool variant_legal(unsigned bits) { return (!(bits & V_F) || (bits & V_Q)) && (!(bits & V_L) || !(bits & (V_D | V_Q | V_F))); }
#define V_AT(bits) (1u << (bits))         // the one class with exactly these switches (after the step's mask), as a set

// A kernel's arguments, bound by its parameter TYPES: Pick<P, Src>::of(src) is the argument of type P that a source of arguments
// holds (a handle at a step: host_handle.h, StepSrc; an item of the one-workgroup path: small_lp.h, SmallItem).  Each class-variant
// kernel's parameter list says which argument groups it takes, so no call site writes one out.
template <class P, class Src> struct Pick;
template <class Src, class... P> static void launch_bound(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st, const Src& src) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, Pick<P, Src>::of(src)...);
}

// sum over the row chunks of the GEMV-T partials, in chunk order (fixed order: bitwise reproducible).  Eight loads are in
// flight at a time: a plain loop waits for every load before it issues the next one (32 chunks = 32 L2 latencies, 13 us of
// direction_kernel's 13 us at n = 8192).
__device__ __forceinline__ double col_sum(const double* atp, int rc_chunks, int np, int j) {
    double s = 0.0;
    int r = 0;
    for (; r + 8 <= rc_chunks; r += 8) {
        double t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = atp[(int64_t)(r + q) * np + j];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += t[q];
    }
    for (; r < rc_chunks; ++r) s += atp[(int64_t)r * np + j];
    return s;
}

// r_c = A^T y + s - c ; d = x/s ; predictor v = d*(r_c - r3/x) ; partial ||r_c||^2, x.s, c.x, ||r_b||^2
// Bounded, on U: r_c -= z ; r_u = x + w - u ; d = theta ; v = theta (r_c - r3/x + (r4 - z r_u)/w) with r4 = w z ;
// r_u^2 joins ||r_b||^2 and w z joins x.s
// Detect (IPM_FLAG_DETECT_INFEASIBILITY): also the partials of the infeasibility tests (P_BY .. P_MXU) -- reads of what the
// pass holds anyway (A^T y from col_sum, A x = r_b + b), no extra pass over A
// Quad (ipm_set_quadratic; g: the np-vector of the diagonal): r_c, d and the objective by the quad_* rules, one more streamed vector
// (residual_cols of small_lp.h is the hand-kept second copy of this column, its Quad branches included: keep the two in step)
// Free (ipm_set_free_columns; fr: the byte marks and their count): a marked column by the free_* rules -- r_c without s, d = 1 / g,
// q = 0, v = d r_c, nothing into x.s -- one more streamed vector of bytes
// Detect with Quad (IPM_FLAG_DETECT_QUADRATIC; iteration_rules.h states the tests): two more partials, P_CXL and P_MGX, from c, g and x
// the column holds anyway, and |(A^T y)_j| of a free column into P_MATY -- still no extra pass over A
// FreeLp (ipm_set_free_lp_columns; fr: the marks, rho: the handle's proximal weight): a marked column by the free_lp_* rules -- r_c
// without s, d = 1 / rho, q = 0, v = d r_c, c x into the objective, nothing into x.s
template <bool Bounded = false, bool Detect = false, bool Quad = false, bool Free = false, bool FreeLp = false>
__device__ __forceinline__ void prepare_kernel_body(VecArgs a, const unsigned bx_, const unsigned gx_, BndArgs bd = BndArgs{}, const double* g = nullptr,
                                                    FreeArgs fr = FreeArgs{}, double rho = 0.0) {
    static_assert(!Free || Quad, "a free column needs curvature: Free is only meaningful with Quad");
    static_assert(!FreeLp || (!Detect && !Quad && !Free), "an LP free column lives on a plain or bounded LP handle");
    __shared__ double red[VBLK];
    const int gid = bx_ * VBLK + threadIdx.x, gsz = gx_ * VBLK;
    double rc2 = 0.0, xs = 0.0, cx = 0.0, rb2 = 0.0;
    double by = 0.0, uz = 0.0, maty = 0.0, max_ = 0.0, mxu = 0.0;      // Detect only
    double cxl = 0.0, mgx = 0.0;                                       // Detect with Quad only
    for (int j = gid; j < a.n; j += gsz) {
        double xj = a.x[j], sj = a.s[j];
        if constexpr (FreeLp) {
            if (free_in(fr, j)) {
                const double rcj = free_lp_rc(col_sum(a.atp, a.rc_chunks, a.np, j), a.c[j]);
                const double dj = free_lp_theta(rho);
                a.rc[j] = rcj;
                a.d[j] = dj;
                free_rhs_column<Bounded>(a, bd, j, dj, rcj);
                rc2 += rcj * rcj;
                cx += a.c[j] * xj;
                continue;
            }
        }
        if constexpr (Free) {
            if (free_in(fr, j)) {
                const double gj = g[j];
                const double atyj = col_sum(a.atp, a.rc_chunks, a.np, j);
                const double rcj = free_rc(atyj, a.c[j], gj, xj);
                const double dj = free_theta(gj);
                a.rc[j] = rcj;
                a.d[j] = dj;
                free_rhs_column<Bounded>(a, bd, j, dj, rcj);
                rc2 += rcj * rcj;
                cx += quad_objective(a.c[j], gj, xj);
                if constexpr (Detect) { maty = fmax(maty, detect_dual_free(atyj)); cxl += detect_linear(a.c[j], xj); mgx = fmax(mgx, detect_curvature(gj, xj)); }
                continue;
            }
        }
        if constexpr (Bounded) {
            const double uj = bd.u[j];
            if (bnd_in(uj)) {
                const double wj = bd.w[j], zj = bd.z[j];
                const double atyj = col_sum(a.atp, a.rc_chunks, a.np, j);
                double rcj = atyj + sj - zj - a.c[j];
                const double ruj = xj + wj - uj;
                double dj;
                if constexpr (Quad) { const double gj = g[j]; rcj = quad_rc(rcj, gj, xj); dj = quad_bnd_theta(xj, sj, wj, zj, gj); cx += quad_objective(a.c[j], gj, xj);
                                     if constexpr (Detect) { cxl += detect_linear(a.c[j], xj); mgx = fmax(mgx, detect_curvature(gj, xj)); } }
                else dj = bnd_theta(xj, sj, wj, zj);
                const double r3 = xj * sj, r4 = wj * zj;
                a.rc[j] = rcj;
                a.d[j] = dj;
                a.q[j] = r3 / xj;
                bd.qz[j] = r4 / wj;
                a.v[j] = dj * (rcj - r3 / xj + (r4 - zj * ruj) / wj);
                rc2 += rcj * rcj;
                xs += r3;
                xs += r4;
                if constexpr (!Quad) cx += a.c[j] * xj;
                rb2 += ruj * ruj;
                if constexpr (Detect) { uz += uj * zj; maty = fmax(maty, atyj - zj); mxu = fmax(mxu, xj); }
                continue;
            }
        }
        const double atyj = col_sum(a.atp, a.rc_chunks, a.np, j);
        double rcj = atyj + sj - a.c[j];
        double dj;
        if constexpr (Quad) { const double gj = g[j]; rcj = quad_rc(rcj, gj, xj); dj = quad_theta(xj, sj, gj); cx += quad_objective(a.c[j], gj, xj);
                             if constexpr (Detect) { cxl += detect_linear(a.c[j], xj); mgx = fmax(mgx, detect_curvature(gj, xj)); } }
        else dj = xj / sj;
        double r3 = xj * sj;
        a.rc[j] = rcj;
        a.d[j] = dj;
        a.q[j] = r3 / xj;
        a.v[j] = dj * (rcj - r3 / xj);
        rc2 += rcj * rcj;
        xs += r3;
        if constexpr (!Quad) cx += a.c[j] * xj;
        if constexpr (Detect) maty = fmax(maty, atyj);
    }
    for (int i = gid; i < a.m; i += gsz) {
        double r = a.rb[i]; rb2 += r * r;
        if constexpr (Detect) { const double bi = a.b[i]; by += bi * a.y[i]; max_ = fmax(max_, fabs(r + bi)); }
    }
    rc2 = block_sum(rc2, red); xs = block_sum(xs, red); cx = block_sum(cx, red); rb2 = block_sum(rb2, red);
    if constexpr (Detect) { by = block_sum(by, red); uz = block_sum(uz, red); maty = block_max(maty, red); max_ = block_max(max_, red); mxu = block_max(mxu, red); }
    if constexpr (Detect && Quad) { cxl = block_sum(cxl, red); mgx = block_max(mgx, red); }
    if (threadIdx.x == 0) {
        a.part[P_RC2 * MAXPART + bx_] = rc2;
        a.part[P_XS * MAXPART + bx_] = xs;
        a.part[P_CX * MAXPART + bx_] = cx;
        a.part[P_RB2 * MAXPART + bx_] = rb2;
        if constexpr (Detect) {
            a.part[P_BY * MAXPART + bx_] = by;
            a.part[P_UZ * MAXPART + bx_] = uz;
            a.part[P_MATY * MAXPART + bx_] = maty;
            a.part[P_MAX * MAXPART + bx_] = max_;
            a.part[P_MXU * MAXPART + bx_] = mxu;
        }
        if constexpr (Detect && Quad) {
            a.part[P_CXL * MAXPART + bx_] = cxl;
            a.part[P_MGX * MAXPART + bx_] = mgx;
        }
    }
}
__global__ __launch_bounds__(VBLK) void prepare_kernel(VecArgs a) { prepare_kernel_body(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void prepare_bounded_kernel(VecArgs a, BndArgs bd) { prepare_kernel_body<true>(a, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void prepare_detect_kernel(VecArgs a) { prepare_kernel_body<false, true>(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void prepare_bounded_detect_kernel(VecArgs a, BndArgs bd) { prepare_kernel_body<true, true>(a, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void prepare_quad_kernel(VecArgs a, const double* g) { prepare_kernel_body<false, false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, g); }
__global__ __launch_bounds__(VBLK) void prepare_bounded_quad_kernel(VecArgs a, BndArgs bd, const double* g) { prepare_kernel_body<true, false, true>(a, blockIdx.x, gridDim.x, bd, g); }
__global__ __launch_bounds__(VBLK) void prepare_free_kernel(VecArgs a, const double* g, FreeArgs fr) { prepare_kernel_body<false, false, true, true>(a, blockIdx.x, gridDim.x, BndArgs{}, g, fr); }
__global__ __launch_bounds__(VBLK) void prepare_bounded_free_kernel(VecArgs a, BndArgs bd, const double* g, FreeArgs fr) { prepare_kernel_body<true, false, true, true>(a, blockIdx.x, gridDim.x, bd, g, fr); }
__global__ __launch_bounds__(VBLK) void prepare_quad_detect_kernel(VecArgs a, const double* g) { prepare_kernel_body<false, true, true>(a, blockIdx.x, gridDim.x, BndArgs{}, g); }
__global__ __launch_bounds__(VBLK) void prepare_bounded_quad_detect_kernel(VecArgs a, BndArgs bd, const double* g) { prepare_kernel_body<true, true, true>(a, blockIdx.x, gridDim.x, bd, g); }
__global__ __launch_bounds__(VBLK) void prepare_free_detect_kernel(VecArgs a, const double* g, FreeArgs fr) { prepare_kernel_body<false, true, true, true>(a, blockIdx.x, gridDim.x, BndArgs{}, g, fr); }
__global__ __launch_bounds__(VBLK) void prepare_bounded_free_detect_kernel(VecArgs a, BndArgs bd, const double* g, FreeArgs fr) { prepare_kernel_body<true, true, true, true>(a, blockIdx.x, gridDim.x, bd, g, fr); }
__global__ __launch_bounds__(VBLK) void prepare_free_lp_kernel(VecArgs a, FreeLpArgs fl) { prepare_kernel_body<false, false, false, false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, nullptr, fl.cols, fl.rho); }
__global__ __launch_bounds__(VBLK) void prepare_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { prepare_kernel_body<true, false, false, false, true>(a, blockIdx.x, gridDim.x, bd, nullptr, fl.cols, fl.rho); }
constexpr unsigned PREPARE_FLAGS = V_ALL;
#define PREPARE_VARIANTS(U, T)                                                    \
    T(V_AT(0), LS_PREPARE)                                                        \
    T(V_AT(V_B), LS_PREPARE_BND)                                                  \
    T(V_AT(V_D), LS_PREPARE_DETECT)                                               \
    T(V_AT(V_B | V_D), LS_PREPARE_DETECT_BND)                                     \
    U(V_AT(V_Q), prepare_quad_kernel)                                             \
    U(V_AT(V_B | V_Q), prepare_bounded_quad_kernel)                               \
    U(V_AT(V_Q | V_F), prepare_free_kernel)                                       \
    U(V_AT(V_B | V_Q | V_F), prepare_bounded_free_kernel)                         \
    U(V_AT(V_D | V_Q), prepare_quad_detect_kernel)                                \
    U(V_AT(V_B | V_D | V_Q), prepare_bounded_quad_detect_kernel)                  \
    U(V_AT(V_D | V_Q | V_F), prepare_free_detect_kernel)                          \
    U(V_AT(V_B | V_D | V_Q | V_F), prepare_bounded_free_detect_kernel)            \
    U(V_AT(V_L), prepare_free_lp_kernel)                                          \
    U(V_AT(V_B | V_L), prepare_bounded_free_lp_kernel)

// d = x / s only (main.py:223): what the formation of A D^2 A^T needs; the full prepare_kernel follows on the residual
// stream while the factorization runs (host_iteration.h, enqueue_iteration).  Bounded: d = theta on U.  Quad: the quad_* scalings.
// Free: d = free_theta on the marked columns.  FreeLp: d = free_lp_theta there.
template <bool Bounded = false, bool Quad = false, bool Free = false, bool FreeLp = false>
__device__ __forceinline__ void scaling_kernel_body(VecArgs a, BndArgs bd = BndArgs{}, const double* g = nullptr, FreeArgs fr = FreeArgs{}, double rho = 0.0) {
    static_assert(!Free || Quad, "a free column needs curvature: Free is only meaningful with Quad");
    static_assert(!FreeLp || (!Quad && !Free), "an LP free column lives on a plain or bounded LP handle");
    if (blockIdx.x == 0 && threadIdx.x == 0) a.sc->done_f = a.sc->done;      // latch for this iteration's factorization
    if (a.sc->done) return;
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    for (int j = gid; j < a.n; j += gsz) {
        if constexpr (FreeLp) {
            if (free_in(fr, j)) { a.d[j] = free_lp_theta(rho); continue; }
        }
        if constexpr (Free) {
            if (free_in(fr, j)) { a.d[j] = free_theta(g[j]); continue; }
        }
        if constexpr (Bounded) {
            if (bnd_in(bd.u[j])) {
                if constexpr (Quad) a.d[j] = quad_bnd_theta(a.x[j], a.s[j], bd.w[j], bd.z[j], g[j]);
                else a.d[j] = bnd_theta(a.x[j], a.s[j], bd.w[j], bd.z[j]);
                continue;
            }
        }
        if constexpr (Quad) a.d[j] = quad_theta(a.x[j], a.s[j], g[j]);
        else a.d[j] = a.x[j] / a.s[j];
    }
}
__global__ __launch_bounds__(VBLK) void scaling_kernel(VecArgs a) { scaling_kernel_body(a); }
__global__ __launch_bounds__(VBLK) void scaling_bounded_kernel(VecArgs a, BndArgs bd) { scaling_kernel_body<true>(a, bd); }
__global__ __launch_bounds__(VBLK) void scaling_quad_kernel(VecArgs a, const double* g) { scaling_kernel_body<false, true>(a, BndArgs{}, g); }
__global__ __launch_bounds__(VBLK) void scaling_bounded_quad_kernel(VecArgs a, BndArgs bd, const double* g) { scaling_kernel_body<true, true>(a, bd, g); }
__global__ __launch_bounds__(VBLK) void scaling_free_kernel(VecArgs a, const double* g, FreeArgs fr) { scaling_kernel_body<false, true, true>(a, BndArgs{}, g, fr); }
__global__ __launch_bounds__(VBLK) void scaling_bounded_free_kernel(VecArgs a, BndArgs bd, const double* g, FreeArgs fr) { scaling_kernel_body<true, true, true>(a, bd, g, fr); }
__global__ __launch_bounds__(VBLK) void scaling_free_lp_kernel(VecArgs a, FreeLpArgs fl) { scaling_kernel_body<false, false, false, true>(a, BndArgs{}, nullptr, fl.cols, fl.rho); }
__global__ __launch_bounds__(VBLK) void scaling_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { scaling_kernel_body<true, false, false, true>(a, bd, nullptr, fl.cols, fl.rho); }
constexpr unsigned SCALING_FLAGS = V_B | V_Q | V_F | V_L;      // (residual-stream iteration only, which is never recorded: launched directly)
#define SCALING_VARIANTS(U, T)                                                    \
    U(V_AT(0), scaling_kernel)                                                    \
    U(V_AT(V_B), scaling_bounded_kernel)                                          \
    U(V_AT(V_Q), scaling_quad_kernel)                                             \
    U(V_AT(V_B | V_Q), scaling_bounded_quad_kernel)                               \
    U(V_AT(V_Q | V_F), scaling_free_kernel)                                       \
    U(V_AT(V_B | V_Q | V_F), scaling_bounded_free_kernel)                         \
    U(V_AT(V_L), scaling_free_lp_kernel)                                          \
    U(V_AT(V_B | V_L), scaling_bounded_free_lp_kernel)

// stop test of check_optimality (main.py:162-173) -- one thread.
// Bounded: ||r_b||^2 carries r_u^2 and the gap w.z (prepare_kernel), b_norm is ||(b, u_U)|| (ipm_set_bounds), mu divides by n + |U|.
// Detect: the infeasibility tests (detect_fire) where the convergence test says "continue", before the iteration cap.
// Free: mu divides by free_pair_count (the free columns put nothing into the gap; their r_c is in ||r_c||).
// Quad (meaningful with Detect only; IPM_FLAG_DETECT_QUADRATIC): gamma from the linear c.x (P_CXL), max g|x| (P_MGX) joins the dual violation.
template <bool Bounded = false, bool Detect = false, bool Free = false, bool Quad = false>
__device__ __forceinline__ void stop_test_kernel_body(VecArgs a, const unsigned bx_, const unsigned gx_, BndArgs bd = BndArgs{}, DetArgs dt = DetArgs{},
                                                      FreeArgs fr = FreeArgs{}) {
    static_assert(!Free || !Detect || Quad, "a free column needs curvature: Free is only meaningful with Quad");
    static_assert(!Quad || Detect, "the stop test reads the quadratic term through the infeasibility tests only");
    if (threadIdx.x != 0 || bx_ != 0) return;
    Scalars* sc = a.sc;
    if (sc->done) return;
    double rb = sqrt(sum_partials(a.part, P_RB2, a.nblk));
    double rc = sqrt(sum_partials(a.part, P_RC2, a.nblk));
    double gap = sum_partials(a.part, P_XS, a.nblk);
    sc->rb_norm = rb; sc->rc_norm = rc; sc->gap = gap;
    const double obj = sum_partials(a.part, P_CX, a.nblk);
    sc->obj = obj;
    if (fabs(obj) < 1.7e308) sc->obj_last_finite = obj;          // false for NaN and Inf
    if constexpr (Free) sc->mu = gap / free_pair_count<Bounded>(a.n, bd, fr);
    else if constexpr (Bounded) sc->mu = gap / (double)(a.n + bd.nU);
    else sc->mu = gap / (double)a.n;
    bool cont = (sc->e1 * (1.0 + sc->b_norm) < rb) || (sc->e2 * (1.0 + sc->c_norm) < rc) || (sc->e3 < gap);
    if (sc->force) return;
    if (!cont) {
        bool finite = (rb == rb) && (rc == rc) && (gap == gap) && (fabs(rb) < 1.7e308) && (fabs(rc) < 1.7e308) &&
                      (fabs(gap) < 1.7e308);
        sc->status = finite ? 1 : 3;
        sc->done = 1;
    } else if (Detect && !Quad && detect_fire(dt, sc, sum_partials(a.part, P_BY, a.nblk) - sum_partials(a.part, P_UZ, a.nblk),
                                              max_partials(a.part, P_MATY, a.nblk), -obj,
                                              fmax(max_partials(a.part, P_MAX, a.nblk), max_partials(a.part, P_MXU, a.nblk)))) {
    } else if (Detect && Quad && detect_fire(dt, sc, sum_partials(a.part, P_BY, a.nblk) - sum_partials(a.part, P_UZ, a.nblk),
                                             max_partials(a.part, P_MATY, a.nblk), -sum_partials(a.part, P_CXL, a.nblk),
                                             fmax(fmax(max_partials(a.part, P_MAX, a.nblk), max_partials(a.part, P_MXU, a.nblk)),
                                                  max_partials(a.part, P_MGX, a.nblk)))) {
    } else if (sc->k >= sc->max_iter) {
        sc->status = 2;
        sc->done = 1;
    }
}
__global__ void stop_test_kernel(VecArgs a) { stop_test_kernel_body(a, blockIdx.x, gridDim.x); }
__global__ void stop_test_bounded_kernel(VecArgs a, BndArgs bd) { stop_test_kernel_body<true>(a, blockIdx.x, gridDim.x, bd); }
__global__ void stop_test_detect_kernel(VecArgs a, DetArgs dt) { stop_test_kernel_body<false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, dt); }
__global__ void stop_test_bounded_detect_kernel(VecArgs a, BndArgs bd, DetArgs dt) { stop_test_kernel_body<true, true>(a, blockIdx.x, gridDim.x, bd, dt); }
__global__ void stop_test_free_kernel(VecArgs a, FreeArgs fr) { stop_test_kernel_body<false, false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, DetArgs{}, fr); }
__global__ void stop_test_bounded_free_kernel(VecArgs a, BndArgs bd, FreeArgs fr) { stop_test_kernel_body<true, false, true>(a, blockIdx.x, gridDim.x, bd, DetArgs{}, fr); }
__global__ void stop_test_quad_detect_kernel(VecArgs a, DetArgs dt) { stop_test_kernel_body<false, true, false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, dt); }
__global__ void stop_test_bounded_quad_detect_kernel(VecArgs a, BndArgs bd, DetArgs dt) { stop_test_kernel_body<true, true, false, true>(a, blockIdx.x, gridDim.x, bd, dt); }
__global__ void stop_test_free_detect_kernel(VecArgs a, DetArgs dt, FreeArgs fr) { stop_test_kernel_body<false, true, true, true>(a, blockIdx.x, gridDim.x, BndArgs{}, dt, fr); }
__global__ void stop_test_bounded_free_detect_kernel(VecArgs a, BndArgs bd, DetArgs dt, FreeArgs fr) { stop_test_kernel_body<true, true, true, true>(a, blockIdx.x, gridDim.x, bd, dt, fr); }
// (an LP free column changes the pair count and nothing else the stop test reads: the Free body, from the LP free set's marks)
__global__ void stop_test_free_lp_kernel(VecArgs a, FreeLpArgs fl) { stop_test_kernel_body<false, false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, DetArgs{}, fl.cols); }
__global__ void stop_test_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { stop_test_kernel_body<true, false, true>(a, blockIdx.x, gridDim.x, bd, DetArgs{}, fl.cols); }
// (the term alone changes nothing the stop test reads: without Detect a quadratic handle takes the LP's rows)
constexpr unsigned STOP_TEST_FLAGS = V_ALL;
#define STOP_TEST_VARIANTS(U, T)                                                  \
    T(V_AT(0) | V_AT(V_Q), LS_STOP_TEST)                                          \
    T(V_AT(V_B) | V_AT(V_B | V_Q), LS_STOP_TEST_BND)                              \
    T(V_AT(V_D), LS_STOP_TEST_DETECT)                                             \
    T(V_AT(V_B | V_D), LS_STOP_TEST_DETECT_BND)                                   \
    U(V_AT(V_Q | V_F), stop_test_free_kernel)                                     \
    U(V_AT(V_B | V_Q | V_F), stop_test_bounded_free_kernel)                       \
    U(V_AT(V_D | V_Q), stop_test_quad_detect_kernel)                              \
    U(V_AT(V_B | V_D | V_Q), stop_test_bounded_quad_detect_kernel)                \
    U(V_AT(V_D | V_Q | V_F), stop_test_free_detect_kernel)                        \
    U(V_AT(V_B | V_D | V_Q | V_F), stop_test_bounded_free_detect_kernel)          \
    U(V_AT(V_L), stop_test_free_lp_kernel)                                        \
    U(V_AT(V_B | V_L), stop_test_bounded_free_lp_kernel)

// The certificate of a detection (ipm_get_certificate): kind 5 -> (y / beta, z / beta), kind 6 -> x / gamma; the other parts 0.
// out = [x (n) | y (m) | z (n)]; z = nullptr without bounds.
__global__ __launch_bounds__(256) void certificate_kernel(const double* x, const double* y, const double* z, const double* det, int m, int n,
                                                          double* out) {
    const int gid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    const bool primal = det[0] == (double)IPM_STATUS_PRIMAL_INFEASIBLE_;
    const double sc = 1.0 / det[1];
    double *ox = out, *oy = out + n, *oz = out + n + m;
    for (int j = gid; j < n; j += gsz) {
        ox[j] = primal ? 0.0 : x[j] * sc;
        oz[j] = (primal && z) ? z[j] * sc : 0.0;
    }
    for (int i = gid; i < m; i += gsz) oy[i] = primal ? y[i] * sc : 0.0;
}

// direction_column + ratio test.  corr == 0: (dxa, dsa[, dwa, dza]) from dya with the predictor's q;
// corr == 1: (dx, ds[, dw, dz]) from dy with the corrector's q.
// Free: free_direction_column on the marked columns, which take no part in the ratio tests.
template <bool Bounded = false, bool Free = false>
__device__ __forceinline__ void direction_kernel_body(VecArgs a, int corr, const unsigned bx_, const unsigned gx_, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    if (a.sc->done) return;
    __shared__ double red[VBLK];
    const int gid = bx_ * VBLK + threadIdx.x, gsz = gx_ * VBLK;
    double* DX = corr ? a.dx : a.dxa;
    double* DS = corr ? a.ds : a.dsa;
    double mp_ = 1.0, md_ = 1.0;
    for (int j = gid; j < a.n; j += gsz) {
        const double xj = a.x[j], sj = a.s[j];
        const double w = col_sum(a.atp, a.rc_chunks, a.np, j);
        if constexpr (Free) {
            if (free_in(fr, j)) { free_direction_column<Bounded>(a, j, w, DX, DS, corr ? bd.dw : bd.dwa, corr ? bd.dz : bd.dza); continue; }
        }
        direction_column<Bounded>(a, bd, j, w, DX, DS, corr ? bd.dw : bd.dwa, corr ? bd.dz : bd.dza, xj, sj, mp_, md_);
    }
    mp_ = block_min(mp_, red); md_ = block_min(md_, red);
    if (threadIdx.x == 0) {
        a.part[(corr ? P_MINP : P_MINP_AFF) * MAXPART + bx_] = mp_;
        a.part[(corr ? P_MIND : P_MIND_AFF) * MAXPART + bx_] = md_;
    }
}
__global__ __launch_bounds__(VBLK) void direction_kernel(VecArgs a, int corr) { direction_kernel_body(a, corr, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void direction_bounded_kernel(VecArgs a, int corr, BndArgs bd) { direction_kernel_body<true>(a, corr, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void direction_free_kernel(VecArgs a, int corr, FreeArgs fr) { direction_kernel_body<false, true>(a, corr, blockIdx.x, gridDim.x, BndArgs{}, fr); }
__global__ __launch_bounds__(VBLK) void direction_bounded_free_kernel(VecArgs a, int corr, BndArgs bd, FreeArgs fr) { direction_kernel_body<true, true>(a, corr, blockIdx.x, gridDim.x, bd, fr); }
// (an LP free column's recovery is free_direction_column too: the Free body, from the LP free set's marks)
__global__ __launch_bounds__(VBLK) void direction_free_lp_kernel(VecArgs a, int corr, FreeLpArgs fl) { direction_kernel_body<false, true>(a, corr, blockIdx.x, gridDim.x, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void direction_bounded_free_lp_kernel(VecArgs a, int corr, BndArgs bd, FreeLpArgs fl) { direction_kernel_body<true, true>(a, corr, blockIdx.x, gridDim.x, bd, fl.cols); }
constexpr unsigned DIRECTION_FLAGS = V_B | V_F | V_L;
#define DIRECTION_VARIANTS(U, T)                                                  \
    T(V_AT(0), LS_DIRECTION)                                                      \
    T(V_AT(V_B), LS_DIRECTION_BND)                                                \
    U(V_AT(V_F), direction_free_kernel)                                           \
    U(V_AT(V_B | V_F), direction_bounded_free_kernel)                             \
    U(V_AT(V_L), direction_free_lp_kernel)                                        \
    U(V_AT(V_B | V_L), direction_bounded_free_lp_kernel)

// partial sums of mu_aff_column at the affine step lengths (Quad: at the one step quad_step makes of them, which the stats report)
// Free: no term of a marked column.  (An LP free column: Free without Quad -- the LP's two affine step lengths.)
template <bool Bounded = false, bool Quad = false, bool Free = false, bool FreeLp = false>
__device__ __forceinline__ void mu_aff_kernel_body(VecArgs a, const unsigned bx_, const unsigned gx_, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    static_assert(!Free || Quad, "a free column needs curvature: Free is only meaningful with Quad");
    static_assert(!FreeLp || (!Quad && !Free), "an LP free column lives on a plain or bounded LP handle");
    if (a.sc->done) return;
    __shared__ double red[VBLK];
    const int gid = bx_ * VBLK + threadIdx.x, gsz = gx_ * VBLK;
    double ap = min_partials(a.part, P_MINP_AFF, a.nblk);
    double ad = min_partials(a.part, P_MIND_AFF, a.nblk);
    if constexpr (Quad) ap = ad = quad_step(ap, ad);
    double acc = 0.0;
    for (int j = gid; j < a.n; j += gsz) {
        if constexpr (Free || FreeLp) {
            if (free_in(fr, j)) continue;
        }
        mu_aff_column<Bounded>(a, bd, j, ap, ad, acc);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) {
        a.part[P_MUAFF * MAXPART + bx_] = acc;
        if (bx_ == 0) { a.sc->alpha_aff_p = ap; a.sc->alpha_aff_d = ad; }
    }
}
__global__ __launch_bounds__(VBLK) void mu_aff_kernel(VecArgs a) { mu_aff_kernel_body(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void mu_aff_bounded_kernel(VecArgs a, BndArgs bd) { mu_aff_kernel_body<true>(a, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void mu_aff_quad_kernel(VecArgs a) { mu_aff_kernel_body<false, true>(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void mu_aff_bounded_quad_kernel(VecArgs a, BndArgs bd) { mu_aff_kernel_body<true, true>(a, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void mu_aff_free_kernel(VecArgs a, FreeArgs fr) { mu_aff_kernel_body<false, true, true>(a, blockIdx.x, gridDim.x, BndArgs{}, fr); }
__global__ __launch_bounds__(VBLK) void mu_aff_bounded_free_kernel(VecArgs a, BndArgs bd, FreeArgs fr) { mu_aff_kernel_body<true, true, true>(a, blockIdx.x, gridDim.x, bd, fr); }
__global__ __launch_bounds__(VBLK) void mu_aff_free_lp_kernel(VecArgs a, FreeLpArgs fl) { mu_aff_kernel_body<false, false, false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void mu_aff_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { mu_aff_kernel_body<true, false, false, true>(a, blockIdx.x, gridDim.x, bd, fl.cols); }
constexpr unsigned MU_AFF_FLAGS = V_B | V_Q | V_F | V_L;
#define MU_AFF_VARIANTS(U, T)                                                     \
    T(V_AT(0), LS_MU_AFF)                                                         \
    T(V_AT(V_B), LS_MU_AFF_BND)                                                   \
    U(V_AT(V_Q), mu_aff_quad_kernel)                                              \
    U(V_AT(V_B | V_Q), mu_aff_bounded_quad_kernel)                                \
    U(V_AT(V_Q | V_F), mu_aff_free_kernel)                                        \
    U(V_AT(V_B | V_Q | V_F), mu_aff_bounded_free_kernel)                          \
    U(V_AT(V_L), mu_aff_free_lp_kernel)                                           \
    U(V_AT(V_B | V_L), mu_aff_bounded_free_lp_kernel)

// centring from the re-summed partials of mu_aff_kernel, then corrector_column
// Free: the centring over free_pair_count pairs (centring with n - n_free columns), free_rhs_column on the marked columns.
template <bool Bounded = false, bool Free = false>
__device__ __forceinline__ void corrector_rhs_kernel_body(VecArgs a, const unsigned bx_, const unsigned gx_, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    if (a.sc->done) return;
    const int gid = bx_ * VBLK + threadIdx.x, gsz = gx_ * VBLK;
    const double mu = a.sc->mu;
    const Centring ct = centring<Bounded>(sum_partials(a.part, P_MUAFF, a.nblk), mu, Free ? a.n - fr.nfree : a.n, bd);
    const double sm = ct.sigma * mu;
    for (int j = gid; j < a.n; j += gsz) {
        if constexpr (Free) {
            if (free_in(fr, j)) { free_rhs_column<Bounded>(a, bd, j, a.d[j], a.rc[j]); continue; }
        }
        corrector_column<Bounded>(a, bd, j, sm);
    }
    if (gid == 0) { a.sc->mu_aff = ct.mu_aff; a.sc->sigma = ct.sigma; }
}
__global__ __launch_bounds__(VBLK) void corrector_rhs_kernel(VecArgs a) { corrector_rhs_kernel_body(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void corrector_rhs_bounded_kernel(VecArgs a, BndArgs bd) { corrector_rhs_kernel_body<true>(a, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void corrector_rhs_free_kernel(VecArgs a, FreeArgs fr) { corrector_rhs_kernel_body<false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, fr); }
__global__ __launch_bounds__(VBLK) void corrector_rhs_bounded_free_kernel(VecArgs a, BndArgs bd, FreeArgs fr) { corrector_rhs_kernel_body<true, true>(a, blockIdx.x, gridDim.x, bd, fr); }
// (an LP free column's corrector column is free_rhs_column over free_pair_count pairs too: the Free body, from the LP free set's marks)
__global__ __launch_bounds__(VBLK) void corrector_rhs_free_lp_kernel(VecArgs a, FreeLpArgs fl) { corrector_rhs_kernel_body<false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void corrector_rhs_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { corrector_rhs_kernel_body<true, true>(a, blockIdx.x, gridDim.x, bd, fl.cols); }
constexpr unsigned CORRECTOR_RHS_FLAGS = V_B | V_F | V_L;
#define CORRECTOR_RHS_VARIANTS(U, T)                                              \
    T(V_AT(0), LS_CORR_RHS)                                                       \
    T(V_AT(V_B), LS_CORR_RHS_BND)                                                 \
    U(V_AT(V_F), corrector_rhs_free_kernel)                                       \
    U(V_AT(V_B | V_F), corrector_rhs_bounded_free_kernel)                         \
    U(V_AT(V_L), corrector_rhs_free_lp_kernel)                                    \
    U(V_AT(V_B | V_L), corrector_rhs_bounded_free_lp_kernel)

// damped_step from the re-summed ratio-test minima (Quad: quad_step of the pair), update_column, y += a_d dy, record_iteration
// Free: free_update_column on the marked columns (s stays 0).  FreeLp: the same with the LP's own alpha_p (no quad_step).
template <bool Bounded = false, bool Quad = false, bool Free = false, bool FreeLp = false>
__device__ __forceinline__ void update_kernel_body(VecArgs a, const unsigned bx_, const unsigned gx_, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    static_assert(!Free || Quad, "a free column needs curvature: Free is only meaningful with Quad");
    static_assert(!FreeLp || (!Quad && !Free), "an LP free column lives on a plain or bounded LP handle");
    if (a.sc->done) return;
    const int gid = bx_ * VBLK + threadIdx.x, gsz = gx_ * VBLK;
    const double eta = a.sc->eta;
    double ap = damped_step(eta, min_partials(a.part, P_MINP, a.nblk));
    double ad = damped_step(eta, min_partials(a.part, P_MIND, a.nblk));
    if constexpr (Quad) ap = ad = quad_step(ap, ad);
    for (int j = gid; j < a.n; j += gsz) {
        if constexpr (Free || FreeLp) {
            if (free_in(fr, j)) { free_update_column(a, j, ap); continue; }
        }
        update_column<Bounded>(a, bd, j, ap, ad);
    }
    for (int i = gid; i < a.m; i += gsz) a.y[i] += ad * a.dy[i];
    if (gid == 0) {
        Scalars* sc = a.sc;
        if (sc->k == 0) sc->fixed_first = sc->fixed;
        record_iteration(sc, a.hist, sc->mu, sc->sigma, sc->alpha_aff_p, sc->alpha_aff_d, ap, ad);
    }
}
__global__ __launch_bounds__(VBLK) void update_kernel(VecArgs a) { update_kernel_body(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void update_bounded_kernel(VecArgs a, BndArgs bd) { update_kernel_body<true>(a, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void update_quad_kernel(VecArgs a) { update_kernel_body<false, true>(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(VBLK) void update_bounded_quad_kernel(VecArgs a, BndArgs bd) { update_kernel_body<true, true>(a, blockIdx.x, gridDim.x, bd); }
__global__ __launch_bounds__(VBLK) void update_free_kernel(VecArgs a, FreeArgs fr) { update_kernel_body<false, true, true>(a, blockIdx.x, gridDim.x, BndArgs{}, fr); }
__global__ __launch_bounds__(VBLK) void update_bounded_free_kernel(VecArgs a, BndArgs bd, FreeArgs fr) { update_kernel_body<true, true, true>(a, blockIdx.x, gridDim.x, bd, fr); }
__global__ __launch_bounds__(VBLK) void update_free_lp_kernel(VecArgs a, FreeLpArgs fl) { update_kernel_body<false, false, false, true>(a, blockIdx.x, gridDim.x, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void update_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { update_kernel_body<true, false, false, true>(a, blockIdx.x, gridDim.x, bd, fl.cols); }
constexpr unsigned UPDATE_FLAGS = V_B | V_Q | V_F | V_L;
#define UPDATE_VARIANTS(U, T)                                                     \
    T(V_AT(0), LS_UPDATE)                                                         \
    T(V_AT(V_B), LS_UPDATE_BND)                                                   \
    U(V_AT(V_Q), update_quad_kernel)                                              \
    U(V_AT(V_B | V_Q), update_bounded_quad_kernel)                                \
    U(V_AT(V_Q | V_F), update_free_kernel)                                        \
    U(V_AT(V_B | V_Q | V_F), update_bounded_free_kernel)                          \
    U(V_AT(V_L), update_free_lp_kernel)                                           \
    U(V_AT(V_B | V_L), update_bounded_free_lp_kernel)

// ---------------------------------------------------------------------------------------
// Centrality correctors (iteration_rules.h: mcc_*): the three vector kernels of one round, enqueued K times between
// the corrector's direction_kernel and update_kernel (host_iteration.h), never with K = 0.  Between the first two run the
// products with A and the solve with this iteration's factor, which test MccCtl::rdone in place of Scalars::done.
// `a`, `bd` are the handle's views; `c`, `cb` the same views with the candidate's q, v, dx, ds, dy (qz, dw, dz) in place.
// ---------------------------------------------------------------------------------------
struct MccArgs {
    double *r3, *r3g, *r4, *r4g;   // complementarity terms of the current direction (valid once a round was accepted) and of the candidate
    double* part;                  // [2][MAXPART]: the candidate's partial ratio-test minima (primal, dual)
    MccCtl* ctl;                   // the record of the rounds
    int first;                     // the iteration's first round
};

// target / right-hand side: alpha from the re-reduced minima as update_kernel takes it, the trial point, mcc_rhs_column.
// One thread opens the round: rdone for the kernels behind this one (they are whole launches later, so the word is never read in
// the launch that writes it; this kernel's own blocks decide from `done` and rdead, which earlier launches wrote), the step
// lengths for accept_kernel, the tally.  The first round revives the chain (rdead = 0) and so never reads rdead.
template <bool Bounded = false>
__device__ __forceinline__ void mcc_target_kernel_body(VecArgs a, VecArgs c, MccArgs g, BndArgs bd = BndArgs{}, BndArgs cb = BndArgs{}) {
    Scalars* sc = a.sc;
    MccCtl* ctl = g.ctl;
    const bool off = sc->done || (!g.first && ctl->rdead);
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (lead) {
        ctl->rdone = off ? 1 : 0;
        if (g.first) { ctl->rdead = 0; ctl->hit = 0; }
    }
    if (off) return;
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    const double eta = sc->eta;
    const double ap = damped_step(eta, min_partials(a.part, P_MINP, a.nblk));
    const double ad = damped_step(eta, min_partials(a.part, P_MIND, a.nblk));
    const double tp = mcc_trial_step(ap), td = mcc_trial_step(ad);
    const double sm = sc->sigma * sc->mu;                          // as corrector_rhs_kernel formed it
    for (int j = gid; j < a.n; j += gsz) {
        double r3c, r4c = 0.0;
        if (g.first) {                                             // Mehrotra's terms, as corrector_column computed them
            r3c = corrector_r3(a, j, a.x[j], sm);
            if constexpr (Bounded) { if (bnd_in(bd.u[j])) r4c = corrector_r4(bd, j, bd.w[j], bd.z[j], sm); }
        } else {
            r3c = g.r3[j];
            if constexpr (Bounded) r4c = g.r4[j];
        }
        mcc_rhs_column<Bounded>(a, bd, c, cb, j, tp, td, sm, r3c, r4c, g.r3g, g.r4g);
    }
    if (lead) { ctl->ap = ap; ctl->ad = ad; ctl->run += 1; }
}
__global__ __launch_bounds__(VBLK) void mcc_target_kernel(VecArgs a, VecArgs c, MccArgs g) { mcc_target_kernel_body(a, c, g); }
__global__ __launch_bounds__(VBLK) void mcc_target_bounded_kernel(VecArgs a, VecArgs c, MccArgs g, BndArgs bd, BndArgs cb) { mcc_target_kernel_body<true>(a, c, g, bd, cb); }

// candidate direction: direction_column on the candidate's arrays, its partial minima into slots of its own
template <bool Bounded = false>
__device__ __forceinline__ void mcc_direction_kernel_body(VecArgs c, MccArgs g, BndArgs cb = BndArgs{}) {
    if (g.ctl->rdone) return;
    __shared__ double red[VBLK];
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    double mp_ = 1.0, md_ = 1.0;
    for (int j = gid; j < c.n; j += gsz) {
        const double xj = c.x[j], sj = c.s[j];
        const double w = col_sum(c.atp, c.rc_chunks, c.np, j);
        direction_column<Bounded>(c, cb, j, w, c.dx, c.ds, cb.dw, cb.dz, xj, sj, mp_, md_);
    }
    mp_ = block_min(mp_, red); md_ = block_min(md_, red);
    if (threadIdx.x == 0) { g.part[blockIdx.x] = mp_; g.part[MAXPART + blockIdx.x] = md_; }
}
__global__ __launch_bounds__(VBLK) void mcc_direction_kernel(VecArgs c, MccArgs g) { mcc_direction_kernel_body(c, g); }
__global__ __launch_bounds__(VBLK) void mcc_direction_bounded_kernel(VecArgs c, MccArgs g, BndArgs cb) { mcc_direction_kernel_body<true>(c, g, cb); }

// accept: every block re-reduces the candidate's minima in the fixed order, holds them against the step lengths the target kernel
// left (the minima of the current direction, re-reduced there: reading them here again would race with the blocks that already
// replace them) and takes the same decision.  Accept: the block's columns of the candidate replace (dx, ds, dw, dz, q, qz, v) and the
// complementarity terms, its rows dy, its slot the partial minima.  Reject: the chain is dead for the rest of the iteration.
template <bool Bounded = false>
__device__ __forceinline__ void mcc_accept_kernel_body(VecArgs a, VecArgs c, MccArgs g, BndArgs bd = BndArgs{}, BndArgs cb = BndArgs{}) {
    MccCtl* ctl = g.ctl;
    if (ctl->rdone) return;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    const double eta = a.sc->eta;
    const double ahp = damped_step(eta, min_partials(g.part, 0, a.nblk));
    const double ahd = damped_step(eta, min_partials(g.part, 1, a.nblk));
    if (!mcc_accept(ctl->ap, ctl->ad, ahp, ahd)) {
        if (lead) ctl->rdead = 1;
        return;
    }
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    for (int j = gid; j < a.n; j += gsz) {
        a.dx[j] = c.dx[j]; a.ds[j] = c.ds[j]; a.q[j] = c.q[j]; a.v[j] = c.v[j]; g.r3[j] = g.r3g[j];
        if constexpr (Bounded) { bd.dw[j] = cb.dw[j]; bd.dz[j] = cb.dz[j]; bd.qz[j] = cb.qz[j]; g.r4[j] = g.r4g[j]; }
    }
    for (int i = gid; i < a.m; i += gsz) a.dy[i] = c.dy[i];
    if (threadIdx.x == 0) {
        a.part[P_MINP * MAXPART + blockIdx.x] = g.part[blockIdx.x];
        a.part[P_MIND * MAXPART + blockIdx.x] = g.part[MAXPART + blockIdx.x];
    }
    if (lead) {
        ctl->acc += 1;
        if (!ctl->hit) { ctl->hit = 1; ctl->iters += 1; }
    }
}
__global__ __launch_bounds__(VBLK) void mcc_accept_kernel(VecArgs a, VecArgs c, MccArgs g) { mcc_accept_kernel_body(a, c, g); }
__global__ __launch_bounds__(VBLK) void mcc_accept_bounded_kernel(VecArgs a, VecArgs c, MccArgs g, BndArgs bd, BndArgs cb) { mcc_accept_kernel_body<true>(a, c, g, bd, cb); }

// ---------------------------------------------------------------------------------------
// Mehrotra's starting point on the device (ipm_init_state_mehrotra): the column work between the two solves with
// A A^T and after them.  The rules are iteration_rules.h (start_*); the reductions are the two-level fixed-order ones of this file.
// Entries beyond n (and rows beyond m) are never written: they keep the zeros ipm_init_state leaves there.
// ---------------------------------------------------------------------------------------
enum { PS_MIN_P = 0, PS_MIN_D, PS_XS, PS_SS, PS_SX, PS_SX2 };      // partial slots of the start (the iteration's slots are free then)

__device__ __forceinline__ double start_min_partials(const double* part, int slot, int nblk) {
    double s = __builtin_inf();
    for (int i = 0; i < nblk; ++i) s = fmin(s, part[slot * MAXPART + i]);
    return s;
}
struct StartSums { double xs, ss, sx; };      // (x.s + w.z) / 2, sum s + sum z_U, sum x + sum w_U after the shifts
__device__ __forceinline__ StartSums start_sums(const double* part, int nblk) {
    return {0.5 * sum_partials(part, PS_XS, nblk), sum_partials(part, PS_SS, nblk), sum_partials(part, PS_SX, nblk)};
}

// finishes the A^T partials in col_sum's order.  Dual = false: x = A^T u (Bounded: w = u - x on U) and the partial minima of (x, w_U);
// Dual = true: r = c - A^T y, s = r (Bounded, on U: s = max(r, 0), z = max(-r, 0)), the partial minima of (s, z_U), and y = dy
// FreeLp: a marked column by the start_free_lp_* rules (no term in the minimum)
template <bool Bounded, bool Dual, bool FreeLp = false>
__device__ __forceinline__ void start_ls_kernel_body(VecArgs a, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    __shared__ double red[VBLK];
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    double mn = __builtin_inf();
    for (int j = gid; j < a.n; j += gsz) {
        const double t = col_sum(a.atp, a.rc_chunks, a.np, j);
        if constexpr (FreeLp) {
            if (free_in(fr, j)) {
                if constexpr (Dual) start_free_lp_dual_column<Bounded>(a, bd, j);
                else start_free_lp_primal_column<Bounded>(a, bd, j, t);
                continue;
            }
        }
        if constexpr (Dual) start_dual_column<Bounded>(a, bd, j, a.c[j] - t, mn);
        else start_primal_column<Bounded>(a, bd, j, t, mn);
    }
    if constexpr (Dual) for (int i = gid; i < a.m; i += gsz) a.y[i] = a.dy[i];
    mn = block_min(mn, red);
    if (threadIdx.x == 0) a.part[(Dual ? PS_MIN_D : PS_MIN_P) * MAXPART + blockIdx.x] = mn;
}
__global__ __launch_bounds__(VBLK) void start_primal_kernel(VecArgs a) { start_ls_kernel_body<false, false>(a); }
__global__ __launch_bounds__(VBLK) void start_primal_bounded_kernel(VecArgs a, BndArgs bd) { start_ls_kernel_body<true, false>(a, bd); }
__global__ __launch_bounds__(VBLK) void start_dual_kernel(VecArgs a) { start_ls_kernel_body<false, true>(a); }
__global__ __launch_bounds__(VBLK) void start_dual_bounded_kernel(VecArgs a, BndArgs bd) { start_ls_kernel_body<true, true>(a, bd); }
__global__ __launch_bounds__(VBLK) void start_primal_free_lp_kernel(VecArgs a, FreeLpArgs fl) { start_ls_kernel_body<false, false, true>(a, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void start_primal_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { start_ls_kernel_body<true, false, true>(a, bd, fl.cols); }
__global__ __launch_bounds__(VBLK) void start_dual_free_lp_kernel(VecArgs a, FreeLpArgs fl) { start_ls_kernel_body<false, true, true>(a, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void start_dual_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { start_ls_kernel_body<true, true, true>(a, bd, fl.cols); }

// scalar phase 1: the shifts from the re-reduced minima, applied; partial sums of x.s + w.z, sum s + sum z_U, sum x + sum w_U
template <bool Bounded, bool FreeLp = false>
__device__ __forceinline__ void start_shift_kernel_body(VecArgs a, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    __shared__ double red[VBLK];
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    const double dp = start_shift(start_min_partials(a.part, PS_MIN_P, a.nblk));
    const double dd = start_shift(start_min_partials(a.part, PS_MIN_D, a.nblk));
    double xs = 0.0, ss = 0.0, sx = 0.0;
    for (int j = gid; j < a.n; j += gsz) {
        if constexpr (FreeLp) {
            if (free_in(fr, j)) continue;
        }
        start_shift_column<Bounded>(a, bd, j, dp, dd, xs, ss, sx);
    }
    xs = block_sum(xs, red); ss = block_sum(ss, red); sx = block_sum(sx, red);
    if (threadIdx.x == 0) {
        a.part[PS_XS * MAXPART + blockIdx.x] = xs;
        a.part[PS_SS * MAXPART + blockIdx.x] = ss;
        a.part[PS_SX * MAXPART + blockIdx.x] = sx;
    }
}
__global__ __launch_bounds__(VBLK) void start_shift_kernel(VecArgs a) { start_shift_kernel_body<false>(a); }
__global__ __launch_bounds__(VBLK) void start_shift_bounded_kernel(VecArgs a, BndArgs bd) { start_shift_kernel_body<true>(a, bd); }
__global__ __launch_bounds__(VBLK) void start_shift_free_lp_kernel(VecArgs a, FreeLpArgs fl) { start_shift_kernel_body<false, true>(a, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void start_shift_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { start_shift_kernel_body<true, true>(a, bd, fl.cols); }

// scalar phase 2: degenerate data -> the reference's start (x = s = 1, y = 1, w = z = 1 on U) and nothing else; otherwise the
// primal correction x += xs / ss and the partial sums of sum x + sum w_U after it
template <bool Bounded, bool FreeLp = false>
__device__ __forceinline__ void start_primal_correct_kernel_body(VecArgs a, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    __shared__ double red[VBLK];
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    const StartSums t = start_sums(a.part, a.nblk);
    if (start_degenerate(t.xs, t.ss, t.sx)) {                     // (the same decision in every thread of every block: all leave)
        for (int j = gid; j < a.n; j += gsz) {
            if constexpr (FreeLp) {
                if (free_in(fr, j)) { start_free_lp_reference_column<Bounded>(a, bd, j); continue; }
            }
            start_reference_column<Bounded>(a, bd, j);
        }
        for (int i = gid; i < a.m; i += gsz) a.y[i] = 1.0;
        return;
    }
    const double pc = t.xs / t.ss;
    double sx = 0.0;
    for (int j = gid; j < a.n; j += gsz) {
        if constexpr (FreeLp) {
            if (free_in(fr, j)) continue;
        }
        start_primal_correct_column<Bounded>(a, bd, j, pc, sx);
    }
    sx = block_sum(sx, red);
    if (threadIdx.x == 0) a.part[PS_SX2 * MAXPART + blockIdx.x] = sx;
}
__global__ __launch_bounds__(VBLK) void start_primal_correct_kernel(VecArgs a) { start_primal_correct_kernel_body<false>(a); }
__global__ __launch_bounds__(VBLK) void start_primal_correct_bounded_kernel(VecArgs a, BndArgs bd) { start_primal_correct_kernel_body<true>(a, bd); }
__global__ __launch_bounds__(VBLK) void start_primal_correct_free_lp_kernel(VecArgs a, FreeLpArgs fl) { start_primal_correct_kernel_body<false, true>(a, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void start_primal_correct_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { start_primal_correct_kernel_body<true, true>(a, bd, fl.cols); }

// scalar phase 3: the dual correction s += xs / (sum x + sum w_U); nothing on degenerate data (phase 2 wrote the reference's start)
template <bool Bounded, bool FreeLp = false>
__device__ __forceinline__ void start_dual_correct_kernel_body(VecArgs a, BndArgs bd = BndArgs{}, FreeArgs fr = FreeArgs{}) {
    const int gid = blockIdx.x * VBLK + threadIdx.x, gsz = gridDim.x * VBLK;
    const StartSums t = start_sums(a.part, a.nblk);
    if (start_degenerate(t.xs, t.ss, t.sx)) return;
    const double dc = t.xs / sum_partials(a.part, PS_SX2, a.nblk);
    for (int j = gid; j < a.n; j += gsz) {
        if constexpr (FreeLp) {
            if (free_in(fr, j)) continue;
        }
        start_dual_correct_column<Bounded>(a, bd, j, dc);
    }
}
__global__ __launch_bounds__(VBLK) void start_dual_correct_kernel(VecArgs a) { start_dual_correct_kernel_body<false>(a); }
__global__ __launch_bounds__(VBLK) void start_dual_correct_bounded_kernel(VecArgs a, BndArgs bd) { start_dual_correct_kernel_body<true>(a, bd); }
__global__ __launch_bounds__(VBLK) void start_dual_correct_free_lp_kernel(VecArgs a, FreeLpArgs fl) { start_dual_correct_kernel_body<false, true>(a, BndArgs{}, fl.cols); }
__global__ __launch_bounds__(VBLK) void start_dual_correct_bounded_free_lp_kernel(VecArgs a, BndArgs bd, FreeLpArgs fl) { start_dual_correct_kernel_body<true, true>(a, bd, fl.cols); }
// The five steps of the start tell plain from bounded, and an LP free set from none (launched directly: the start is never part of
// a recorded program).
constexpr unsigned START_FLAGS = V_B | V_L;
#define START_PRIMAL_VARIANTS(U, T) U(V_AT(0), start_primal_kernel) U(V_AT(V_B), start_primal_bounded_kernel) \
    U(V_AT(V_L), start_primal_free_lp_kernel) U(V_AT(V_B | V_L), start_primal_bounded_free_lp_kernel)
#define START_DUAL_VARIANTS(U, T) U(V_AT(0), start_dual_kernel) U(V_AT(V_B), start_dual_bounded_kernel) \
    U(V_AT(V_L), start_dual_free_lp_kernel) U(V_AT(V_B | V_L), start_dual_bounded_free_lp_kernel)
#define START_SHIFT_VARIANTS(U, T) U(V_AT(0), start_shift_kernel) U(V_AT(V_B), start_shift_bounded_kernel) \
    U(V_AT(V_L), start_shift_free_lp_kernel) U(V_AT(V_B | V_L), start_shift_bounded_free_lp_kernel)
#define START_PRIMAL_CORRECT_VARIANTS(U, T) U(V_AT(0), start_primal_correct_kernel) U(V_AT(V_B), start_primal_correct_bounded_kernel) \
    U(V_AT(V_L), start_primal_correct_free_lp_kernel) U(V_AT(V_B | V_L), start_primal_correct_bounded_free_lp_kernel)
#define START_DUAL_CORRECT_VARIANTS(U, T) U(V_AT(0), start_dual_correct_kernel) U(V_AT(V_B), start_dual_correct_bounded_kernel) \
    U(V_AT(V_L), start_dual_correct_free_lp_kernel) U(V_AT(V_B | V_L), start_dual_correct_bounded_free_lp_kernel)

// out[i] = value for i < n (fill)
__global__ void fill_kernel(double* out, int n, double value) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = value;
}

// ||v||_2 of a short vector -> *out (single block)
__global__ __launch_bounds__(VBLK) void norm2_kernel(const double* v, int n, double* out) {
    __shared__ double red[VBLK];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += VBLK) acc += v[i] * v[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) *out = sqrt(acc);
}

// ||(b, u_U)||_2 -> *out (single block): b_norm of the bounded stop test
__global__ __launch_bounds__(VBLK) void bnd_norm2_kernel(const double* b, int m, const double* u, int n, double* out) {
    __shared__ double red[VBLK];
    double acc = 0.0;
    for (int i = threadIdx.x; i < m; i += VBLK) acc += b[i] * b[i];
    for (int j = threadIdx.x; j < n; j += VBLK) { const double uj = u[j]; if (bnd_in(uj)) acc += uj * uj; }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) *out = sqrt(acc);
}

// w = z = value on U, 0 outside (mask_only: keep w, z on U and zero them outside)
__global__ void bnd_fill_kernel(const double* u, double* w, double* z, int n, double value, int mask_only) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (!bnd_in(u[j])) { w[j] = 0.0; z[j] = 0.0; }
    else if (!mask_only) { w[j] = value; z[j] = value; }
}

// s = 0 on the free columns (every seam that writes a state: ipm_init_state, ipm_set_state, ipm_set_free_columns; the LP free set of
// ipm_set_free_lp_columns alike, from its own marks)
__global__ void free_zero_s_kernel(const unsigned char* mark, double* s, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n && mark[j]) s[j] = 0.0;
}

}  // namespace ipm
