// dense_split.h -- dense columns split out of the sparse normal-matrix factor (gfx950); DESIGN.md 4-D.
//
// A few columns of A with many entries each put a full clique into A A^T and the multifrontal factor of sparse_chol.h fills up.
// With the set DC of those columns (k <= DS_MAX_COLS) taken out,  B = A D A^T = B_s + V V^T,  B_s = A_s D_s A_s^T = L L^T the
// sparse factor as before and V = A_DC diag(sqrt(d_DC)) (m x k, dense).  Sherman-Morrison-Woodbury in its factored form:
//     W = L^-1 V,   S = I_k + W^T W = R R^T,   B^-1 t = L^-T (z - W S^-1 W^T z),  z = L^-1 t.
// S has every eigenvalue >= 1: its Cholesky needs no guard.  A factorization adds: scatter (V), one batched forward sweep (W),
// Gram (partials of W^T W on the matrix cores), Schur factor (R).  A solve adds two launches between its sweeps: the partials of
// W^T z, then the k x k solve and z -= W v.
//
// Determinism: V and W are column-major m x k (leading dimension m).  The rows are cut into CHUNKS whose size depends on m alone
// (ds_chunk_rows); one workgroup owns a chunk, writes its partial, and whoever needs the sum adds the partials in chunk order.  No
// atomics on data, no flags, nothing spins; no result depends on a grid size, on IPM_SP_GRID, IPM_SP_MODE or IPM_SP_THREADS.
// Column j of W is bitwise what sp_fwd_kernel gives for column j of V alone (ds_fwd_kernel is its level form, the column on
// blockIdx.y, each column with its own slice of update vectors; k = 1 runs sp_fwd_kernel itself).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gemm_nt_f64.h"
#include "sparse_chol.h"

namespace ipm {

constexpr int DS_MAX_COLS = 64;          // IPM_MAX_DENSE_COLS
// The sparse part is factored as B_s + DS_DIAG_REL diag(V V^T), and every solve of a split handle is followed by at least
// DS_MIN_REFINE refinement rounds against the full A D A^T (refine_ops.h), which take that term out again.  Why: near the optimum
// the rows that only BASIC dense columns support leave B_s with pivots the size of the vanishing d, ||W||^2 passes 1 / eps and
// z - W S^-1 W^T z cancels every digit (the formulas in NumPy float64 lose the LP the same way).  With the term, ||W||^2 stays
// below 1 / DS_DIAG_REL on those rows and a round contracts by about DS_DIAG_REL (DESIGN.md 4-D has the measurements).
constexpr double DS_DIAG_REL = 1e-10;
constexpr int DS_MIN_REFINE = 2;
constexpr int DS_THREADS = 256;
constexpr int DS_ROWS = 64;              // rows of W a Gram workgroup stages in LDS at a time (16 MFMA k-steps)
constexpr int DS_LDT = DS_ROWS + 2;      // LDS stride of a staged column: 2 mod 4, the fragment reads fall on distinct bank pairs (gemm_nt_f64.h)
constexpr int DS_LDS = DS_MAX_COLS + 1;  // LDS row stride of the k x k matrices S and R (odd: a column walk hits distinct banks)

// rows per chunk: a function of m only -- 256 up to 65536 rows, then as many as keep the chunks at 256
__host__ __device__ __forceinline__ int ds_chunk_rows(long long m) { return m <= 65536 ? 256 : 256 * (int)((m + 65535) / 65536); }

struct DsSplit {
    int k, kp, m, nchunk, rows;          // columns, k padded to a multiple of 16, rows of A, row chunks, rows per chunk
    const int* cols;                     // [k] the dense columns of A
    double* V;                           // [m x k] column-major
    double* W;                           // [m x k] column-major
    double* uvec;                        // [k][uvlen] update vectors of the batched forward sweep
    long long uvlen;
    double* gpart;                       // [nchunk][kp x kp] partials of W^T W (lower 16 x 16 tiles)
    double* R;                           // [kp x kp] row-major, lower: Cholesky factor of I + W^T W (identity on the padding)
    double* upart;                       // [nchunk][kp] partials of W^T z
};

// ------------------------------------------------------------------------------------------------------------ V
// One workgroup per dense column: V(:, j) = 0, then the entries of the column times sqrt(d) (rows are distinct in a canonical CSC).
__global__ __launch_bounds__(DS_THREADS) void ds_scatter_kernel(const int* __restrict__ colptr, const int* __restrict__ rowind,
                                                                const double* __restrict__ cval, const double* __restrict__ d, DsSplit s,
                                                                const int* done) {
    if (done && *done) return;
    const int j = blockIdx.x, tid = threadIdx.x;
    if (j >= s.k) return;
    const int col = s.cols[j];
    double* v = s.V + (long long)j * s.m;
    for (int i = tid; i < s.m; i += DS_THREADS) v[i] = 0.0;
    __syncthreads();
    const double sd = sqrt(d[col]);
    for (int q = colptr[col] + tid; q < colptr[col + 1]; q += DS_THREADS) {
        const int i = rowind[q];
        if (i >= 0 && i < s.m) v[i] = cval[q] * sd;
    }
}

// ------------------------------------------------------------------------------------------------------------ W = L^-1 V
// The level form of sp_fwd_kernel with the right-hand-side column on blockIdx.y: ONE walk of the panel tree for all k columns (one
// launch per level; the kernel boundary is the hand-off).  Statement for statement the arithmetic of sp_fwd_kernel.
template <int NT>
__global__ __launch_bounds__(NT) void ds_fwd_kernel(SpFactor f, DsSplit s, int rmax, const SpRec* __restrict__ recs, int lvl_count) {
    if (f.done && *f.done) return;
    extern __shared__ __attribute__((aligned(16))) double fv[];
    double* D = fv + rmax;
    const int tid = threadIdx.x;
    const int col = blockIdx.y;
    if (col >= s.k) return;
    const double* rhs = s.V + (long long)col * s.m;
    double* z = s.W + (long long)col * s.m;
    double* uvec = s.uvec + (long long)col * s.uvlen;
    for (int tn = (int)blockIdx.x; tn < lvl_count; tn += (int)gridDim.x) {
        const SpRec& rc = recs[tn];
        const int r = rc.r, w = rc.w, nchild = rc.nchild;
        __syncthreads();
        const double* Lp = f.L + rc.lptr;
        double* uv = uvec + rc.rowptr;
        for (int a = tid; a < r; a += NT) fv[a] = a < w ? rhs[rc.c0 + a] : 0.0;
        for (int idx = tid; idx < w * w; idx += NT) D[idx] = Lp[idx];
        double cu[SPC_MAXCH];
        int cr[SPC_MAXCH];
#pragma unroll
        for (int t = 0; t < SPC_MAXCH; ++t) {
            cr[t] = -1; cu[t] = 0.0;
            if (t < nchild) {
                const int pc = rc.ch[t].pc;
                if (tid < pc) { cu[t] = *(uvec + rc.ch[t].relptr + tid); cr[t] = f.crel[rc.ch[t].relptr + tid]; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < SPC_MAXCH; ++t) {
            if (t < nchild) {
                if (cr[t] >= 0) fv[cr[t]] += cu[t];
                const int pc = rc.ch[t].pc;
                if (pc > NT) {
                    const double* uc = uvec + rc.ch[t].relptr;
                    const int* rel = f.crel + rc.ch[t].relptr;
                    for (int i = NT + tid; i < pc; i += NT) fv[rel[i]] += uc[i];
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
        }
        if (tid < 64 && w > 0) {                          // w x w lower triangular solve in the registers of wave 0 (w <= 32)
            const int ln = tid < w ? tid : 0;
            double fa = fv[ln];
            const double di = f.dinv[rc.c0 + ln];
            for (int c = 0; c < w; ++c) {
                const double zc = readlane_f64(fa, c) * readlane_f64(di, c);
                if (tid == c) fa = zc;
                else if (tid > c && tid < w) fa -= D[tid * w + c] * zc;
            }
            if (tid < w) fv[tid] = fa;
        }
        __syncthreads();
        for (int a = tid; a < r; a += NT) {
            if (a < w) { z[rc.c0 + a] = fv[a]; }
            else {
                const double* row = Lp + (long long)a * w;
                double dot = 0.0;
                for (int c = 0; c < w; ++c) dot += row[c] * fv[c];
                uv[a] = fv[a] - dot;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ W^T W
// One workgroup per row chunk: DS_ROWS rows of all kp columns are staged in LDS (coalesced along the columns of W, zeros beyond
// row m, the chunk and column k), then wave I owns the 16 x 16 tiles (I, J <= I) of the partial and runs v_mfma_f64_16x16x4_f64 over
// the staged rows, four at a time in ascending order.  Lane maps: gemm_nt_f64.h.
__global__ __launch_bounds__(DS_THREADS) void ds_gram_kernel(DsSplit s, const int* done) {
    if (done && *done) return;
    __shared__ double T[DS_MAX_COLS * DS_LDT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int nT = s.kp >> 4;
    const int row0 = (int)blockIdx.x * s.rows, row1 = min(s.m, row0 + s.rows);
    f64x4 acc[4];
#pragma unroll
    for (int J = 0; J < 4; ++J) acc[J] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int rb = row0; rb < row1; rb += DS_ROWS) {
        __syncthreads();
        for (int idx = tid; idx < s.kp * DS_ROWS; idx += DS_THREADS) {
            const int c = idx / DS_ROWS, rr = idx - c * DS_ROWS, row = rb + rr;
            T[c * DS_LDT + rr] = (c < s.k && row < row1) ? s.W[(long long)c * s.m + row] : 0.0;
        }
        __syncthreads();
        if (wv < nT) {
            const double* pa = T + (16 * wv + fr) * DS_LDT + fk;
            for (int st = 0; st < DS_ROWS / 4; ++st) {
                const double a = pa[4 * st];
#pragma unroll
                for (int J = 0; J < 4; ++J) {
                    if (J <= wv) {
                        const double b = T[(16 * J + fr) * DS_LDT + fk + 4 * st];
                        acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[J], 0, 0, 0);
                    }
                }
            }
        }
    }
    // accumulator register q of lane l: G(16 I + (l >> 4) + 4 q, 16 J + (l & 15))
    double* out = s.gpart + (long long)blockIdx.x * s.kp * s.kp;
    if (wv < nT) {
#pragma unroll
        for (int J = 0; J < 4; ++J) {
            if (J <= wv) {
#pragma unroll
                for (int q = 0; q < 4; ++q) out[(16 * wv + fk + 4 * q) * s.kp + 16 * J + fr] = acc[J][q];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ R R^T = I + W^T W
// One workgroup: the partials summed in chunk order, + I, right-looking Cholesky of the k x k matrix in LDS, R to memory.
__global__ __launch_bounds__(DS_THREADS) void ds_schur_kernel(DsSplit s, const int* done) {
    if (done && *done) return;
    __shared__ double S[DS_MAX_COLS * DS_LDS];
    const int tid = threadIdx.x, k = s.k, kp = s.kp;
    for (int idx = tid; idx < k * k; idx += DS_THREADS) {
        const int i = idx / k, j = idx - i * k;
        if (j > i) continue;
        double sum = 0.0;
        for (int c = 0; c < s.nchunk; ++c) sum += s.gpart[(long long)c * kp * kp + i * kp + j];
        S[i * DS_LDS + j] = i == j ? sum + 1.0 : sum;
    }
    for (int c = 0; c < k; ++c) {
        __syncthreads();
        const double root = sqrt(S[c * DS_LDS + c]);
        __syncthreads();
        for (int i = c + tid; i < k; i += DS_THREADS) S[i * DS_LDS + c] = i == c ? root : S[i * DS_LDS + c] / root;
        __syncthreads();
        const int q = k - c - 1;
        for (int idx = tid; idx < q * q; idx += DS_THREADS) {
            const int i = c + 1 + idx / q, j = c + 1 + idx % q;
            if (j <= i) S[i * DS_LDS + j] -= S[i * DS_LDS + c] * S[j * DS_LDS + c];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < kp * kp; idx += DS_THREADS) {
        const int i = idx / kp, j = idx - i * kp;
        s.R[idx] = (i < k && j <= i) ? S[i * DS_LDS + j] : (i == j ? 1.0 : 0.0);
    }
}

// ------------------------------------------------------------------------------------------------------------ z -= W S^-1 W^T z
// Step 1, one workgroup per row chunk: upart[chunk][j] = sum over the chunk's rows of W(row, j) z(row).  Wave w takes the columns
// w, w + 4, ...; a lane sums its rows in ascending order, the 64 lane sums meet in a fixed butterfly.
__global__ __launch_bounds__(DS_THREADS) void ds_wtz_kernel(DsSplit s, const double* __restrict__ z, const int* done) {
    if (done && *done) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row0 = (int)blockIdx.x * s.rows, row1 = min(s.m, row0 + s.rows);
    double* out = s.upart + (long long)blockIdx.x * s.kp;
    for (int j = wv; j < s.kp; j += DS_THREADS / 64) {
        double acc = 0.0;
        if (j < s.k) {
            const double* w = s.W + (long long)j * s.m;
            for (int row = row0 + lane; row < row1; row += 64) acc += w[row] * z[row];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) out[j] = acc;
    }
}

// Step 2, one workgroup per row chunk: u = the partials in chunk order, R R^T v = u in the registers of wave 0 (every workgroup
// solves the same k x k system and gets the same bits: k <= 64 makes that cheaper than another launch), z -= W v on the chunk's rows
// with the columns in ascending order.
__global__ __launch_bounds__(DS_THREADS) void ds_apply_kernel(DsSplit s, double* z, const int* done) {
    if (done && *done) return;
    __shared__ double Rs[DS_MAX_COLS * DS_LDS];
    __shared__ double u[DS_MAX_COLS];
    const int tid = threadIdx.x, k = s.k, kp = s.kp;
    for (int idx = tid; idx < k * k; idx += DS_THREADS) {
        const int i = idx / k, j = idx - i * k;
        if (j <= i) Rs[i * DS_LDS + j] = s.R[i * kp + j];
    }
    if (tid < k) {
        double sum = 0.0;
        for (int c = 0; c < s.nchunk; ++c) sum += s.upart[(long long)c * kp + tid];
        u[tid] = sum;
    }
    __syncthreads();
    if (tid < 64) {
        double ui = tid < k ? u[tid] : 0.0;
        for (int c = 0; c < k; ++c) {                     // R y = u
            const double yc = readlane_f64(ui, c) / Rs[c * DS_LDS + c];
            if (tid == c) ui = yc;
            else if (tid > c && tid < k) ui -= Rs[tid * DS_LDS + c] * yc;
        }
        for (int c = k - 1; c >= 0; --c) {                // R^T v = y
            const double vc = readlane_f64(ui, c) / Rs[c * DS_LDS + c];
            if (tid == c) ui = vc;
            else if (tid < c) ui -= Rs[c * DS_LDS + tid] * vc;
        }
        if (tid < k) u[tid] = ui;
    }
    __syncthreads();
    const int row0 = (int)blockIdx.x * s.rows, row1 = min(s.m, row0 + s.rows);
    for (int row = row0 + tid; row < row1; row += DS_THREADS) {
        double acc = 0.0;
        for (int j = 0; j < k; ++j) acc += s.W[(long long)j * s.m + row] * u[j];
        z[row] -= acc;
    }
}

}  // namespace ipm
