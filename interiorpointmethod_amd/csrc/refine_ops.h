// refine_ops.h -- the kernels of the iterative refinement of a normal-equations solve (gfx950; the rule: iteration_rules.h,
// refine_decide; the launch sequence: host_iteration.h, enqueue_refine).  One round is
//   residual (dense or CSR)  ->  decide  ->  [the handle's substitution sweeps and its A^T pass, unchanged kernels]  ->  apply.
// The residual kernels are products with A whose input column is formed on the fly, z_j = d_j * sum_c atp[c][j] (the A^T dy
// partials in chunk order, col_sum), so d o (A^T dy) is never written out.  Every reduction has a fixed order: a solve with
// refinement is bitwise repeatable.  A kernel of a round that follows the end of the rounds returns at entry (RefCtl::rdone).
#pragma once
#include "sparse_ops.h"
#include "vector_ops.h"

namespace ipm {

constexpr int REF_ROWS = 16;        // rows of A per workgroup of a residual kernel (= one pair of partial sums)
constexpr int REF_TILE = 512;       // columns of z staged in LDS at a time (dense)

// the right-hand side of a solve, kept aside before the sweeps consume it
__global__ __launch_bounds__(256) void refine_keep_kernel(const double* __restrict__ t, double* keep, int mp, const int* done) {
    if (done && *done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < mp) keep[i] = t[i];
}

// does the residual kernel of a round run?  The first round asks the word of the solve, the later ones the record.
__device__ __forceinline__ bool refine_round_off(const int* done, const RefCtl* ctl, int first) { return first ? (done && *done) : ctl->rdone != 0; }

// r = t - A z and this workgroup's sums of r^2 and t^2 (part[2 bx], part[2 bx + 1]); A row-major [mp][np], zero padded.
// 16 rows per workgroup, four per wave; z is staged 512 columns at a time, so the partials of A^T dy are summed once per
// workgroup and tile, not once per row.  Rows m .. mp-1 (padding) get r = 0.  grid = mp / 16.
__global__ __launch_bounds__(256) void refine_residual_dense_kernel(const double* __restrict__ A, int64_t lda, int m, int mp, int n, int np,
                                                                    const double* __restrict__ d, const double* __restrict__ atp, int rc_chunks,
                                                                    const double* __restrict__ t, double* r, double* part,
                                                                    const int* done, const RefCtl* ctl, int first) {
    if (refine_round_off(done, ctl, first)) return;
    __shared__ double zs[REF_TILE];
    __shared__ double red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * REF_ROWS + wave * 4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < np; c0 += REF_TILE) {
        __syncthreads();                                       // (the tile before has been read)
        for (int jj = tid; jj < REF_TILE; jj += 256) {
            const int j = c0 + jj;
            zs[jj] = j < n ? d[j] * col_sum(atp, rc_chunks, np, j) : 0.0;
        }
        __syncthreads();
        for (int cc = lane * 2; cc < REF_TILE && c0 + cc < np; cc += 128) {
            const double z0 = zs[cc], z1 = zs[cc + 1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = row0 + q;
                if (row < m) {
                    const f64x2 a2 = *reinterpret_cast<const f64x2*>(A + (int64_t)row * lda + c0 + cc);
                    acc[q] += a2.x * z0;
                    acc[q] += a2.y * z1;
                }
            }
        }
    }
    double rr = 0.0, tt = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double s = acc[q];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const int row = row0 + q;
        if (lane == 0 && row < mp) {
            const double ti = row < m ? t[row] : 0.0;
            const double ri = row < m ? ti - s : 0.0;
            r[row] = ri;
            rr += ri * ri;
            tt += ti * ti;
        }
    }
    if (lane == 0) { red[0][wave] = rr; red[1][wave] = tt; }
    __syncthreads();
    if (tid == 0) {
        part[2 * blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        part[2 * blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// The same for a sparse handle (CSR): 16 lanes per row, 16 rows per workgroup, fixed-order tree reduction.  grid = mp / 16.
__global__ __launch_bounds__(256) void refine_residual_csr_kernel(SparseA A, int mp, int np, const double* __restrict__ d,
                                                                  const double* __restrict__ atp, int rc_chunks, const double* __restrict__ t,
                                                                  double* r, double* part, const int* done, const RefCtl* ctl, int first) {
    if (refine_round_off(done, ctl, first)) return;
    __shared__ double red[2][REF_ROWS];
    const int l16 = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int row = blockIdx.x * REF_ROWS + rl;
    double s = 0.0;
    if (row < A.m) {
        const int pb = A.rowptr[row], pe = A.rowptr[row + 1];
        for (int p = pb + l16; p < pe; p += 16) {
            const int j = A.colind[p];
            s += A.rval[p] * (d[j] * col_sum(atp, rc_chunks, np, j));
        }
    }
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    if (l16 == 0) {
        const double ti = row < A.m ? t[row] : 0.0;
        const double ri = row < A.m ? ti - s : 0.0;
        if (row < mp) r[row] = ri;
        red[0][rl] = ri * ri;
        red[1][rl] = ti * ti;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double rr = 0.0, tt = 0.0;
        for (int q = 0; q < REF_ROWS; ++q) { rr += red[0][q]; tt += red[1][q]; }
        part[2 * blockIdx.x] = rr;
        part[2 * blockIdx.x + 1] = tt;
    }
}

// One workgroup: the sums of the npart pairs in a fixed order (thread i takes the pairs i, i + 256, ... in turn, then the tree of
// block_sum), then refine_decide by one thread.  A round that does not run leaves stale partials; refine_decide does not look at
// them then.
__global__ __launch_bounds__(VBLK) void refine_decide_kernel(const double* __restrict__ part, int npart, RefCtl* ctl, const int* done, int first) {
    __shared__ double red[VBLK];
    double rr = 0.0, tt = 0.0;
    for (int i = threadIdx.x; i < npart; i += VBLK) { rr += part[2 * i]; tt += part[2 * i + 1]; }
    rr = block_sum(rr, red);
    tt = block_sum(tt, red);
    if (threadIdx.x == 0) refine_decide(ctl, rr, tt, first != 0, done && *done);
}

// What a round does to (dy, a): REF_APPLY -- copy them aside, dy += delta, and fold the fresh partials of A^T delta into the
// partials of A^T dy chunk by chunk (their readers sum the chunks exactly as before); REF_RESTORE -- put the copies back;
// REF_NONE -- nothing.  Only the true rows move: the padding of dy stays as it is (zero).  na = rc_chunks * np.
__global__ __launch_bounds__(VBLK) void refine_apply_kernel(const RefCtl* ctl, int m, int64_t na, const double* __restrict__ delta,
                                                           const double* __restrict__ atd, double* dy, double* atp, double* dy_keep, double* atp_keep) {
    const int action = ctl->action;
    if (action == REF_NONE) return;
    const int64_t gid = (int64_t)blockIdx.x * VBLK + threadIdx.x, gsz = (int64_t)gridDim.x * VBLK;
    if (action == REF_APPLY) {
        for (int64_t i = gid; i < m; i += gsz) { const double v = dy[i]; dy_keep[i] = v; dy[i] = v + delta[i]; }
        for (int64_t k = gid; k < na; k += gsz) { const double v = atp[k]; atp_keep[k] = v; atp[k] = v + atd[k]; }
    } else {
        for (int64_t i = gid; i < m; i += gsz) dy[i] = dy_keep[i];
        for (int64_t k = gid; k < na; k += gsz) atp[k] = atp_keep[k];
    }
}

}  // namespace ipm
