// getrf_f64.h -- blocked right-looking LU with partial pivoting, P A = L U, for a dense row-major fp64 matrix on gfx950,
// and the substitution (getrs) that uses it.  The general-matrix seam of the library (ipm_lu_solve / ipm_lu_factor): what
// np.linalg.solve (LAPACK gesv) does for the reference's solve_linear (main.py:176-182) and its unreduced KKT direction
// (main.py:185-212), whose matrix [[0, A^T, I], [A, 0, 0], [S, 0, X]] has a zero diagonal block and needs pivoting.
//
// The matrix is padded to a multiple of the panel width NB with identity rows and columns (their entries in the real
// columns are zero and stay zero, so a padded row is never a pivot of a real column).  Per NB-column panel at column k:
//   lu_panel_step_kernel  x (NB + 1)   one launch per column: apply the pivot found by the previous launch (row swap inside
//                                      the panel), scale, rank-1 update of the panel's remaining columns, and the argmax of
//                                      the next column.  Every workgroup writes its (|a|, row) maximum; the LAST workgroup to
//                                      finish (arrival ticket, no waiting) reduces them and stages the two rows the next
//                                      launch swaps.  Ties go to the smaller row index, so the pivot does not depend on the
//                                      order anything ran in (bitwise repeatable, LAPACK idamax's choice on exact ties).
//   lu_laswp_kernel                    the panel's NB interchanges on every column left and right of it, one launch
//   lu_trsm_kernel                     U12 = inv(L11) A12 (unit lower L11 in LDS), written in place AND transposed into the
//                                      strip `ut` (NB doubles per column, K contiguous) for the NT GEMM
//   gemm_nt (gemm_nt_f64.h)            A22 -= L21 U12 on the fp64 MFMA: P = L21 (K = NB contiguous in the rows of A), Q = ut
// An exactly zero pivot does not stop the factorization (LAPACK info > 0): the column is left unscaled and the first such
// column is recorded in LuState::info.
//
// Substitution: lu_gather_kernel applies P to the right-hand sides (the permutation is composed on the host from the
// interchanges), then one lu_trsv_step_kernel per NB-row block and sweep: every workgroup solves the diagonal block (in LDS,
// redundantly) and updates its share of the rows below (forward, unit L) or above (backward, U) with it; workgroup 0 stores the
// block's solution.  The solved block goes to a second array, so no launch reads what it writes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gemm_nt_f64.h"

namespace ipm {

constexpr int LU_MAX_GRID = 1024;      // workgroups of a panel step (their argmax partials live in LuState)
constexpr int LU_RC = 8;               // right-hand sides per workgroup of a substitution step
constexpr int LU_TRSV_ROWS = 64;       // rows of the off-diagonal update per substitution workgroup

struct LuState {
    int piv;                  // pivot row of the column the next panel step eliminates
    int info;                 // 0, or 1 + the first column with an exactly zero pivot
    unsigned ticket;          // arrival counter of the running panel step (the last arriver resets it)
    int pad_;
    double pivval;            // a[piv][col] (signed)
    double urow[128];         // panel row `piv` before the swap: becomes row `col`
    double orow[128];         // panel row `col` before the swap: becomes row `piv`
    double pval[LU_MAX_GRID]; // per-workgroup argmax partials
    int pidx[LU_MAX_GRID];
};

// (|v|, row) total order: larger magnitude first, then the smaller row
__device__ __forceinline__ bool lu_better(double v, int r, double bv, int br) {
    return v > bv || (v == bv && r < br);
}

// Panel step j of the panel at column k (j = -1: argmax of the panel's first column only).  Rows > k + j are
// updated; waves own rows round-robin.  Lane c holds panel columns c (and c + 64 when NB = 128).
template <int NB>
__global__ __launch_bounds__(256) void lu_panel_step_kernel(double* __restrict__ a, int64_t lda, int n, int np, int k, int j,
                                                            LuState* st, int* __restrict__ ipiv) {
    constexpr int H = NB / 64;                  // columns per lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = gridDim.x * 4, gw = blockIdx.x * 4 + wave;
    const int jj = j + 1;                       // column whose argmax this launch computes (NB: none)
    const int rfirst = k + j + 1;
    double u[H];
    double pv = 0.0;
    int p = -1;
    if (j >= 0) {
        p = st->piv; pv = st->pivval;
#pragma unroll
        for (int h = 0; h < H; ++h) u[h] = st->urow[lane + 64 * h];
        if (blockIdx.x == 0 && wave == 0) {     // row k + j <- the pivot row (nobody else reads row k + j in this launch)
            double* dst = a + (int64_t)(k + j) * lda + k;
#pragma unroll
            for (int h = 0; h < H; ++h) dst[lane + 64 * h] = u[h];
        }
    }
    double bv = -1.0;
    int br = 0x7fffffff;
    // RB rows per wave per pass, all loads issued before any store (the rows are independent; one row at a time leaves a
    // wave with a single HBM round trip in flight)
    constexpr int RB = 4;
    for (int r0 = rfirst + gw; r0 < np; r0 += RB * W) {
        double v[RB][H];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int r = r0 + q * W;
            const double* row = a + (int64_t)r * lda + k;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int c = lane + 64 * h;
                // row p receives the old row k + j (staged, since row k + j is rewritten)
                v[q][h] = (r >= np) ? 0.0 : (r == p) ? st->orow[c] : ((c >= j) ? row[c] : 0.0);
            }
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int r = r0 + q * W;
            if (r >= np) break;
            if (j >= 0) {
                const double aj = __shfl(v[q][j / 64], j & 63);
                if (pv != 0.0) {
                    const double l = aj / pv;
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        const int c = lane + 64 * h;
                        if (c == j) v[q][h] = l;
                        else if (c > j) v[q][h] = fma(-l, u[h], v[q][h]);
                    }
                }
                double* row = a + (int64_t)r * lda + k;
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int c = lane + 64 * h;
                    if (r == p || c >= j) row[c] = v[q][h];
                }
            }
            if (jj < NB) {
#pragma unroll
                for (int h = 0; h < H; ++h)
                    if (lane + 64 * h == jj && lu_better(fabs(v[q][h]), r, bv, br)) { bv = fabs(v[q][h]); br = r; }
            }
        }
    }
    if (jj >= NB) return;
    // ---- argmax of column jj: the lane holding it -> LDS -> workgroup partial -> last workgroup
    __shared__ double sv[4];
    __shared__ int si[4];
    __shared__ bool last;
    const int owner = jj & 63;
    if (lane == owner) { sv[wave] = bv; si[wave] = br; }
    __threadfence();                             // every wave's row stores are out before the ticket below
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = sv[0]; int bi = si[0];
        for (int w = 1; w < 4; ++w) if (lu_better(sv[w], si[w], b, bi)) { b = sv[w]; bi = si[w]; }
        st->pval[blockIdx.x] = b; st->pidx[blockIdx.x] = bi;
        __threadfence();                         // the partial before the ticket
        const unsigned t = atomicAdd(&st->ticket, 1u);
        last = (t == gridDim.x - 1);
    }
    __syncthreads();
    if (!last) return;
    __threadfence();                             // acquire: every other workgroup's stores are visible
    const int col = k + jj;
    {   // the workgroups' partials: strided per thread, then a tree in LDS (the order is total, so the result is unique)
        __shared__ double rv[256];
        __shared__ int ri[256];
        double b = -1.0; int bi = 0x7fffffff;
        for (int g = threadIdx.x; g < (int)gridDim.x; g += blockDim.x) {
            const double pvv = __hip_atomic_load(&st->pval[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int pii = __hip_atomic_load(&st->pidx[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lu_better(pvv, pii, b, bi)) { b = pvv; bi = pii; }
        }
        rv[threadIdx.x] = b; ri[threadIdx.x] = bi;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o && lu_better(rv[threadIdx.x + o], ri[threadIdx.x + o], rv[threadIdx.x], ri[threadIdx.x])) {
                rv[threadIdx.x] = rv[threadIdx.x + o]; ri[threadIdx.x] = ri[threadIdx.x + o];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            b = rv[0]; bi = ri[0];
            if (!(b > 0.0)) {                    // exactly zero column: no interchange (idamax picks the first row)
                bi = col;
                if (col < n && st->info == 0) st->info = col + 1;
            }
            st->piv = bi;
            ipiv[col] = bi;
            st->ticket = 0u;
            si[0] = bi;
        }
    }
    __syncthreads();
    const int pr = si[0];
    for (int c = threadIdx.x; c < NB; c += blockDim.x) {
        const double vu = __hip_atomic_load(&a[(int64_t)pr * lda + k + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double vo = __hip_atomic_load(&a[(int64_t)col * lda + k + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        st->urow[c] = vu;
        st->orow[c] = vo;
        if (c == jj) st->pivval = vu;
    }
}

// The panel's NB interchanges (rows k + i <-> ipiv[k + i], in order) on every column outside [k, k + NB): one thread per column.
template <int NB>
__global__ __launch_bounds__(256) void lu_laswp_kernel(double* __restrict__ a, int64_t lda, int np, int k, const int* __restrict__ ipiv) {
    __shared__ int pv[NB];
    for (int i = threadIdx.x; i < NB; i += blockDim.x) pv[i] = ipiv[k + i];
    __syncthreads();
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= np - NB) return;
    const int c = idx < k ? idx : idx + NB;
    for (int i = 0; i < NB; ++i) {
        const int p = pv[i];
        if (p != k + i) {
            double* x = a + (int64_t)(k + i) * lda + c;
            double* y = a + (int64_t)p * lda + c;
            const double t = *x; *x = *y; *y = t;
        }
    }
}

// U12 = inv(L11) A12 for the columns right of the panel, one thread per column, in 32-row chunks (registers); L11 (unit
// lower) in LDS.  The result is stored in place and transposed into ut (row c = column c of U12, NB doubles).
template <int NB>
__global__ __launch_bounds__(128) void lu_trsm_kernel(double* __restrict__ a, int64_t lda, int np, int k, double* __restrict__ ut) {
    extern __shared__ double L11[];              // [NB][NB]
    for (int e = threadIdx.x; e < NB * NB; e += blockDim.x) {
        const int r = e / NB, c = e % NB;
        L11[e] = a[(int64_t)(k + r) * lda + k + c];
    }
    __syncthreads();
    const int c = k + NB + blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= np) return;
    double* col = a + (int64_t)k * lda + c;
    double* out = ut + (int64_t)c * NB;
    constexpr int CH = 32;
    for (int c0 = 0; c0 < NB; c0 += CH) {
        double x[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) x[i] = col[(int64_t)(c0 + i) * lda];
        for (int t = 0; t < c0; ++t) {           // earlier chunks (final, in out[])
            const double v = out[t];
#pragma unroll
            for (int i = 0; i < CH; ++i) x[i] = fma(-L11[(c0 + i) * NB + t], v, x[i]);
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
#pragma unroll
            for (int t = 0; t < i; ++t) x[i] = fma(-L11[(c0 + i) * NB + c0 + t], x[t], x[i]);
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) { col[(int64_t)(c0 + i) * lda] = x[i]; out[c0 + i] = x[i]; }
    }
}

// Identity on the padding (rows and columns n .. np of an np x np image whose padding is zero) and a finiteness check of
// the first n x n entries (bad != 0 afterwards when any is NaN or Inf).
__global__ __launch_bounds__(256) void lu_prepare_kernel(double* __restrict__ a, int64_t lda, int n, int np, int* bad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)np * np) return;
    const int r = (int)(e / np), c = (int)(e % np);
    double* p = a + (int64_t)r * lda + c;
    if (r < n && c < n) { if (!isfinite(*p)) atomicOr(bad, 1); }
    else if (r == c) *p = 1.0;
}

// Finiteness of an n x nr block (ld = nr).
__global__ __launch_bounds__(256) void lu_check_kernel(const double* __restrict__ v, int64_t count, int* bad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count && !isfinite(v[e])) atomicOr(bad, 1);
}

// y[i][q] = b[perm[i]][q] (row-major, nr right-hand sides)
__global__ __launch_bounds__(256) void lu_gather_kernel(const double* __restrict__ b, double* __restrict__ y, const int* __restrict__ perm, int np, int nr) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)np * nr) return;
    const int i = (int)(e / nr), q = (int)(e % nr);
    y[e] = b[(int64_t)perm[i] * nr + q];
}

// One block step of a substitution sweep with the packed factor `a`.  Block rows [b0, b0 + NB).
//   forward  (UPPER = false): z_b = inv(unit L_bb) y_b  -> out;   y[r] -= L[r, b] z_b for r >= b0 + NB
//   backward (UPPER = true):  x_b = inv(U_bb) y_b       -> out;   y[r] -= U[r, b] x_b for r <  b0
// grid (1 + row workgroups, ceil(nr / LU_RC)); dynamic LDS: NB*NB + NB*LU_RC doubles.
template <int NB, bool UPPER>
__global__ __launch_bounds__(256) void lu_trsv_step_kernel(const double* __restrict__ a, int64_t lda, int np, int b0,
                                                           double* __restrict__ y, double* __restrict__ out, int nr) {
    extern __shared__ double lds[];
    double* D = lds;                             // [NB][NB] diagonal block
    double* ys = lds + NB * NB;                  // [NB][LU_RC]
    const int q0 = blockIdx.y * LU_RC;
    const int nq = min(LU_RC, nr - q0);
    for (int e = threadIdx.x; e < NB * NB; e += blockDim.x) D[e] = a[(int64_t)(b0 + e / NB) * lda + b0 + e % NB];
    for (int e = threadIdx.x; e < NB * LU_RC; e += blockDim.x) {
        const int r = e / LU_RC, q = e % LU_RC;
        ys[e] = q < nq ? y[(int64_t)(b0 + r) * nr + q0 + q] : 0.0;
    }
    __syncthreads();
    // column-oriented solve: thread t owns entries (r, q) = (t / LU_RC + 32 e, t % LU_RC)
    const int q = threadIdx.x % LU_RC, rb = threadIdx.x / LU_RC;
    constexpr int RS = 256 / LU_RC;              // 32 rows per pass
    for (int s = 0; s < NB; ++s) {
        const int i = UPPER ? NB - 1 - s : s;
        if (UPPER) {
            if (rb == 0) ys[i * LU_RC + q] /= D[i * NB + i];
            __syncthreads();
        }
        const double xi = ys[i * LU_RC + q];
        for (int r = rb; r < NB; r += RS)
            if (UPPER ? r < i : r > i) ys[r * LU_RC + q] = fma(-D[r * NB + i], xi, ys[r * LU_RC + q]);
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        for (int e = threadIdx.x; e < NB * LU_RC; e += blockDim.x) {
            const int r = e / LU_RC, qq = e % LU_RC;
            if (qq < nq) out[(int64_t)(b0 + r) * nr + q0 + qq] = ys[e];
        }
        return;
    }
    // off-diagonal update: one wave per row, lanes over the block's columns, fixed butterfly reduction
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rbase = UPPER ? (blockIdx.x - 1) * LU_TRSV_ROWS : b0 + NB + (blockIdx.x - 1) * LU_TRSV_ROWS;
    const int rend = UPPER ? b0 : np;
    for (int rr = wave; rr < LU_TRSV_ROWS; rr += 4) {
        const int r = rbase + rr;
        if (r >= rend) break;
        double lv[NB / 64];
#pragma unroll
        for (int h = 0; h < NB / 64; ++h) lv[h] = a[(int64_t)r * lda + b0 + lane + 64 * h];
        for (int qq = 0; qq < nq; ++qq) {
            double s = 0.0;
#pragma unroll
            for (int h = 0; h < NB / 64; ++h) s = fma(lv[h], ys[(lane + 64 * h) * LU_RC + qq], s);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) y[(int64_t)r * nr + q0 + qq] -= s;
        }
    }
}

}  // namespace ipm
