// equilibrate.h -- power-of-two Ruiz equilibration of the LP on the device: the rule, the abs-max reductions of the
// current scaled matrix, the factor update and the kernels that rewrite A and every value table derived from it ONCE.
//
// THE RULE (stated here once; tests/equilibrate_oracle.py restates it in NumPy): a row or column whose largest magnitude of
// r_i |a_ij| c_j is v > 0, v = f 2^e with f in [0.5, 1) (frexp), has its factor multiplied by 2^(-floor(e / 2)); v = 0 (an empty or
// padding line) leaves it alone.  All rows and all columns are updated from the SAME maxima (simultaneous passes).  A pass changes
// nothing exactly when every non-empty maximum lies in [0.5, 2): the fixed point.  The factors are kept as integer exponents, so
// a scaled entry is ldexp(a_ij, er_i + ec_j): no rounding anywhere, and no intermediate product that could leave the range.
// Preconditions: finite data, and no nonzero entry of A, b, c, u that the final factors push out of the normal range -- checked on
// the device (the reductions flag it), never assumed.  The max reductions are order independent (deterministic by construction);
// the only atomics are integer ORs on flag words.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "sparse_chol.h"      // SpNode (eq_spf_apply_kernel)

namespace ipm {

constexpr int EQ_EXP_LIMIT = 900;      // |exponent| of a factor beyond which the scaling is refused
constexpr int EQ_MAX_PASSES = 1024;    // cap of the cap (one flag word per pass)
constexpr int EQ_COL_CHUNKS = 64;      // row chunks of the dense column maxima (two-level reduction, as gemv_t's partials)

// exponent added to a line's factor for the maximum v > 0 (finite)
__host__ __device__ __forceinline__ int ruiz_shift(double v) { int e; (void)frexp(v, &e); return -(e >> 1); }
// a nonzero finite entry whose scaled image left the normal range
__device__ __forceinline__ bool eq_bad(double a, double sa) {
    return a != 0.0 && fabs(a) <= 1.7976931348623157e308 && !(fabs(sa) >= 2.2250738585072014e-308 && fabs(sa) <= 1.7976931348623157e308);
}

// Sparse A, rows (CSR) and columns (CSC) alike: 16 lanes per line, out[line] = max_p |val[p]| 2^(e_own[line] + e_other[ind[p]]).
// live (may be null): the previous pass's `changed` word -- 0 means the fixed point was reached, the maxima on file still hold.
__global__ __launch_bounds__(256) void eq_sparse_max_kernel(const int* __restrict__ ptr, const int* __restrict__ ind, const double* __restrict__ val,
                                                            int nline, const int* __restrict__ e_own, const int* __restrict__ e_other,
                                                            double* __restrict__ out, const int* live, int* err) {
    if (live && *live == 0) return;
    const int line = blockIdx.x * 16 + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
    double mx = 0.0;
    bool bad = false;
    if (line < nline) {
        const int eo = e_own[line], pe = ptr[line + 1];
        for (int p = ptr[line] + l16; p < pe; p += 16) {
            const double a = fabs(val[p]), sa = ldexp(a, eo + e_other[ind[p]]);
            bad |= eq_bad(a, sa);
            mx = fmax(mx, sa);
        }
    }
    for (int o = 8; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 16));
    if (line < nline && l16 == 0) out[line] = mx;
    if (bad) atomicOr(err, 1);
}

// Dense A (row-major mp x np, np a multiple of 64): one workgroup per row, 16-byte loads.
__global__ __launch_bounds__(256) void eq_dense_rowmax_kernel(const double* __restrict__ A, int np, const int* __restrict__ er, const int* __restrict__ ec,
                                                              double* __restrict__ rowmax, const int* live, int* err) {
    if (live && *live == 0) return;
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x, e = er[i];
    const double2* row = (const double2*)(A + (size_t)i * np);
    const int2* ec2 = (const int2*)ec;
    double mx = 0.0;
    bool bad = false;
    for (int j2 = tid; j2 < np / 2; j2 += 256) {
        const double2 a = row[j2];
        const int2 c = ec2[j2];
        const double a0 = fabs(a.x), a1 = fabs(a.y), s0 = ldexp(a0, e + c.x), s1 = ldexp(a1, e + c.y);
        bad |= eq_bad(a0, s0) | eq_bad(a1, s1);
        mx = fmax(mx, fmax(s0, s1));
    }
    red[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) rowmax[i] = red[0];
    if (bad) atomicOr(err, 1);
}

// Column maxima of dense A, level 1: grid (column pairs / 128, row chunks); a thread owns two adjacent columns (16-byte loads,
// consecutive threads consecutive addresses) and walks the rows of its chunk.  part[chunk][j]; level 2 below.
__global__ __launch_bounds__(128) void eq_dense_colpart_kernel(const double* __restrict__ A, int m, int np, int rows_per_chunk, const int* __restrict__ er,
                                                               const int* __restrict__ ec, double* __restrict__ part, const int* live) {
    if (live && *live == 0) return;
    const int j2 = blockIdx.x * 128 + threadIdx.x;
    if (j2 >= np / 2) return;
    const int i0 = blockIdx.y * rows_per_chunk, i1 = min(i0 + rows_per_chunk, m);
    const int2 c = ((const int2*)ec)[j2];
    double m0 = 0.0, m1 = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double2 a = ((const double2*)(A + (size_t)i * np))[j2];
        const int e = er[i];
        m0 = fmax(m0, ldexp(fabs(a.x), e + c.x));
        m1 = fmax(m1, ldexp(fabs(a.y), e + c.y));
    }
    ((double2*)(part + (size_t)blockIdx.y * np))[j2] = make_double2(m0, m1);
}
__global__ __launch_bounds__(256) void eq_colmax_combine_kernel(const double* __restrict__ part, int np, int chunks, double* __restrict__ colmax, const int* live) {
    if (live && *live == 0) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    double mx = 0.0;
    for (int k = 0; k < chunks; ++k) mx = fmax(mx, part[(size_t)k * np + j]);
    colmax[j] = mx;
}

// One pass of the rule on the exponents of R and C.  changed: this pass's flag word; live: the previous pass's (null for the first).
__global__ __launch_bounds__(256) void eq_factor_kernel(const double* __restrict__ rowmax, int m, int* __restrict__ er, const double* __restrict__ colmax, int n,
                                                        int* __restrict__ ec, const int* live, int* changed, int* err) {
    if (live && *live == 0) return;
    const int g = blockIdx.x * 256 + threadIdx.x;
    bool ch = false, bad = false;
    if (g < m) {
        const double v = rowmax[g];
        if (v > 0.0 && v <= 1.7976931348623157e308) {
            const int sh = ruiz_shift(v);
            if (sh) { const int e = er[g] + sh; er[g] = e; ch = true; bad |= e > EQ_EXP_LIMIT || e < -EQ_EXP_LIMIT; }
        }
    }
    if (g < n) {
        const double v = colmax[g];
        if (v > 0.0 && v <= 1.7976931348623157e308) {
            const int sh = ruiz_shift(v);
            if (sh) { const int e = ec[g] + sh; ec[g] = e; ch = true; bad |= e > EQ_EXP_LIMIT || e < -EQ_EXP_LIMIT; }
        }
    }
    if (ch) atomicOr(changed, 1);
    if (bad) atomicOr(err, 1);
}

// {largest, smallest positive} entry of v[0 .. n) -> out[0], out[1] (0, 0 when no entry is positive); single workgroup
__global__ __launch_bounds__(256) void eq_spread_kernel(const double* __restrict__ v, int n, double* out) {
    __shared__ double rmx[256], rmn[256];
    const int tid = threadIdx.x;
    double mx = 0.0, mn = 1.7976931348623157e308;
    for (int i = tid; i < n; i += 256) {
        const double a = v[i];
        if (a > 0.0) { mx = fmax(mx, a); mn = fmin(mn, a); }
    }
    rmx[tid] = mx; rmn[tid] = mn;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { rmx[tid] = fmax(rmx[tid], rmx[tid + s]); rmn[tid] = fmin(rmn[tid], rmn[tid + s]); }
        __syncthreads();
    }
    if (tid == 0) { out[0] = rmx[0]; out[1] = rmx[0] > 0.0 ? rmn[0] : 0.0; }
}

// v[i] <- v[i] 2^(sign e[i]) (b <- R b, c <- C c, u <- u / C: +inf stays +inf); check != 0: flag only, write nothing
__global__ __launch_bounds__(256) void eq_vec_kernel(double* __restrict__ v, const int* __restrict__ e, int n, int sign, int check, int* err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = v[i], sa = ldexp(a, sign * e[i]);
    if (check) { if (eq_bad(a, sa)) atomicOr(err, 1); }
    else v[i] = sa;
}

// ---- the rewrite of A, once
__global__ __launch_bounds__(256) void eq_sparse_apply_kernel(const int* __restrict__ ptr, const int* __restrict__ ind, double* __restrict__ val, int nline,
                                                              const int* __restrict__ e_own, const int* __restrict__ e_other) {
    const int line = blockIdx.x * 16 + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
    if (line >= nline) return;
    const int eo = e_own[line], pe = ptr[line + 1];
    for (int p = ptr[line] + l16; p < pe; p += 16) val[p] = ldexp(val[p], eo + e_other[ind[p]]);
}
__global__ __launch_bounds__(256) void eq_dense_apply_kernel(double* __restrict__ A, int np, const int* __restrict__ er, const int* __restrict__ ec) {
    const int i = blockIdx.x, j2 = blockIdx.y * 256 + threadIdx.x;
    if (j2 >= np / 2) return;
    double2* row = (double2*)(A + (size_t)i * np);
    const int e = er[i];
    const int2 c = ((const int2*)ec)[j2];
    double2 a = row[j2];
    a.x = ldexp(a.x, e + c.x); a.y = ldexp(a.y, e + c.y);
    row[j2] = a;
}
// Product lists of ipm_set_A_csc (host_sparse_setup.h): entry e = (bi[e], bk[e]) of B with the terms bptr[e] .. bptr[e + 1) over the
// columns bcol[t].  coef_k == null: the small path, coef[t] = a_ij a_kj scales by r_i r_k c_j^2; else the list path, coef[t] = a_ij
// by r_i c_j and coef_k[t] = a_kj by r_k c_j.  (The product of two exactly scaled entries is the exactly scaled product.)
template <class Idx>
__global__ __launch_bounds__(256) void eq_list_apply_kernel(const int* __restrict__ bptr, const Idx* __restrict__ bi, const Idx* __restrict__ bk, const int* __restrict__ bcol,
                                                            double* __restrict__ coef, double* __restrict__ coef_k, int nb, const int* __restrict__ er,
                                                            const int* __restrict__ ec) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nb) return;
    const int ei = er[bi[e]], ek = er[bk[e]];
    for (int t = bptr[e]; t < bptr[e + 1]; ++t) {
        const int cj = ec[bcol[t]];
        if (coef_k) { coef[t] = ldexp(coef[t], ei + cj); coef_k[t] = ldexp(coef_k[t], ek + cj); }
        else coef[t] = ldexp(coef[t], ei + ek + 2 * cj);
    }
}
// Product list of the sparse factor (build_sparse_factor): slot lptr[J] + a w + b of panel J is entry (rows[rowptr[J] + a], c0 + b) of
// B, its terms fptr[slot] .. fptr[slot + 1) hold a_ij a_kj over the columns fcol[t].  One workgroup per panel.
__global__ __launch_bounds__(256) void eq_spf_apply_kernel(const SpNode* __restrict__ node, const int* __restrict__ rows, const int* __restrict__ fptr,
                                                           const int* __restrict__ fcol, double* __restrict__ fcoef, const int* __restrict__ er,
                                                           const int* __restrict__ ec) {
    const SpNode nd = node[blockIdx.x];
    const long long slots = (long long)nd.r * nd.w;
    for (long long q = threadIdx.x; q < slots; q += 256) {
        const int a = (int)(q / nd.w), b = (int)(q % nd.w);
        const int eik = er[rows[nd.rowptr + a]] + er[nd.c0 + b];
        const long long slot = nd.lptr + q;
        for (int t = fptr[slot]; t < fptr[slot + 1]; ++t) fcoef[t] = ldexp(fcoef[t], eik + 2 * ec[fcol[t]]);
    }
}

}  // namespace ipm
