// ginv_gemm_f64.h -- the products of the group inverses (trsv_grouped.h, enqueue_group_inverses), as a latency-oriented engine.
//
// One level of the recursive doubling is, per pair of hs x hs diagonal blocks,
//     S = XT11 * L21^T ;   X21 = -X22 * S^T ;   XT12 = -S * X22^T
// at hs = 128, 256, 512: products of at most 0.27 GFLOP that sit, for the last group, on the path between two factorizations.
// gemm_nt_body (gemm_nt_f64.h) runs them latency bound: the global loads of a stage are issued one stage ahead, and with one MFMA
// per wave and k-step there is nothing to hide a memory round trip behind, so every one of the K / 32 stages costs one.  Here
//   * the global loads of GI_DEPTH stages are in flight at once (a ring of register stages, statically indexed: the K loop is
//     unrolled, K / 32 = 4, 8 or 16 stages), so a product costs about K / (32 GI_DEPTH) round trips instead of K / 32;
//   * the launch of X21 also produces XT12: both read the same rows of X22 and S, and the MFMA operand layouts of the two roles
//     coincide (A operand lane l: row l & 15, k l >> 4; B operand lane l: the same), so the fragment a workgroup reads for
//     X21 = -X22 * S^T serves XT12 = -S * X22^T with the operands swapped.  Two launches per level instead of three.
// Every bit is the one gemm_nt_f64_kernel<32, 32, 32, 2, 2, false> produces: per accumulator the same v_mfma_f64_16x16x4_f64
// sequence over k = 0, 4, 8, ... with the same operand values in the same roles (XT12's accumulator has S as its A operand, as
// in the three-launch form), then acc *= alpha, beta = 0.  Nothing is skipped: the zero triangles of XT11 and X22 are multiplied.
// LDS layout and bank argument are those of gemm_nt_f64.h (rows of 32 + 2 doubles).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_nt_f64.h"

namespace ipm {

constexpr int GI_BM = 32, GI_BK = 32;   // 32 x 32 tile, 2 x 2 waves, one 16 x 16 accumulator per wave and product
constexpr int GI_DEPTH = 8;             // stages of global loads in flight: 4 f64x2 per thread and stage, 128 VGPRs in all

// C[i][j] = alpha * sum_k P[i][k] Q[j][k]  (M = N = K = hs); DUAL: also CT[j][i] = alpha * sum_k Q[j][k] P[i][k] with Q's rows as
// the A operand.  Batched over blockIdx.y (pairs: strides sP, sQ, sC, sCT) and blockIdx.z (groups: sP2, ...).
struct GinvGemm {
    const double* P; int64_t ldp, sP, sP2;
    const double* Q; int64_t ldq, sQ, sQ2;
    double* C; int64_t ldc, sC, sC2;
    double* CT; int64_t ldct, sCT, sCT2;        // DUAL only
    int hs;
    double alpha;
    const int* done;                            // device flag: the kernel is a no-op when *done != 0 (may be null)
};

template <int NK, bool DUAL>
__global__ __launch_bounds__(256, 1) void ginv_gemm_kernel(GinvGemm g) {
    if (g.done && *g.done) return;
    constexpr int BM = GI_BM, BK = GI_BK, NT = 256;
    constexpr int LDT = BK + 2;                 // padded LDS row (doubles)
    constexpr int CH = BK / 2;                  // 16-byte chunks per tile row
    constexpr int RSTEP = NT / CH;              // rows one pass of the workgroup covers
    constexpr int PL = (BM * CH) / NT;          // chunks per thread and operand tile
    constexpr int D = GI_DEPTH < NK ? GI_DEPTH : NK;
    static_assert((BM * CH) % NT == 0, "tile/threads mismatch");
    __shared__ __attribute__((aligned(16))) double lds[4 * BM * LDT];
    double* Ps = lds;                           // [2][BM][LDT]
    double* Qs = lds + 2 * BM * LDT;            // [2][BM][LDT]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // (tiles row-major over blockIdx.x; a 2-D patch of tiles per XCD was measured and changed no kernel's time)
    const int ntn = g.hs / BM;
    const int ti = (int)blockIdx.x / ntn, tj = (int)blockIdx.x % ntn;
    const int row0 = ti * BM, col0 = tj * BM;
    const int64_t by = blockIdx.y, bz = blockIdx.z;
    const int ch0 = tid % CH, r0t = tid / CH;
    const double* Pg = g.P + by * g.sP + bz * g.sP2 + (int64_t)(row0 + r0t) * g.ldp + ch0 * 2;
    const double* Qg = g.Q + by * g.sQ + bz * g.sQ2 + (int64_t)(col0 + r0t) * g.ldq + ch0 * 2;

    f64x2 pr[D][PL], qr[D][PL];                 // the ring: slot s holds stage t with t % D == s
    auto load_stage = [&](int t) {
#pragma unroll
        for (int i = 0; i < PL; ++i) qr[t % D][i] = *reinterpret_cast<const f64x2*>(Qg + (int64_t)(i * RSTEP) * g.ldq + t * BK);
#pragma unroll
        for (int i = 0; i < PL; ++i) pr[t % D][i] = *reinterpret_cast<const f64x2*>(Pg + (int64_t)(i * RSTEP) * g.ldp + t * BK);
    };
    auto store_stage = [&](int t) {
        const int buf = t & 1;
#pragma unroll
        for (int i = 0; i < PL; ++i) *reinterpret_cast<f64x2*>(Qs + (buf * BM + r0t + i * RSTEP) * LDT + ch0 * 2) = qr[t % D][i];
#pragma unroll
        for (int i = 0; i < PL; ++i) *reinterpret_cast<f64x2*>(Ps + (buf * BM + r0t + i * RSTEP) * LDT + ch0 * 2) = pr[t % D][i];
    };

#pragma unroll
    for (int t = 0; t < D; ++t) load_stage(t);
    if (g.done && *g.done) return;              // the latch once more, behind the first loads: nothing is stored yet
    store_stage(0);
    if (D < NK) load_stage(D);
    __syncthreads();

    f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0}, acct = acc;
    const int fr = lane & 15, fk = lane >> 4;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
        const int buf = kt & 1;
        const double* pa = Ps + (buf * BM + wm * 16 + fr) * LDT + fk;
        const double* qb = Qs + (buf * BM + wn * 16 + fr) * LDT + fk;
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const double a = pa[kk * 4], b = qb[kk * 4];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            if (DUAL) acct = __builtin_amdgcn_mfma_f64_16x16x4f64(b, a, acct, 0, 0, 0);
        }
        if (kt + 1 < NK) {
            store_stage(kt + 1);                                 // the other buffer: its readers passed the last barrier
            if (kt + 1 + D < NK) load_stage(kt + 1 + D);         // into the slot just emptied
        }
        __syncthreads();
    }

    // accumulator register q of lane l is D[row = (l >> 4) + 4 q][col = l & 15]
    acc *= g.alpha;
    double* c = g.C + by * g.sC + bz * g.sC2 + (int64_t)(row0 + wm * 16 + fk) * g.ldc + col0 + wn * 16 + fr;
#pragma unroll
    for (int q = 0; q < 4; ++q) c[(int64_t)(4 * q) * g.ldc] = acc[q];
    if (DUAL) {
        acct *= g.alpha;
        double* ct = g.CT + by * g.sCT + bz * g.sCT2 + (int64_t)(col0 + wn * 16 + fk) * g.ldct + row0 + wm * 16 + fr;
#pragma unroll
        for (int q = 0; q < 4; ++q) ct[(int64_t)(4 * q) * g.ldct] = acct[q];
    }
}

// hs = 128, 256 or 512 (the levels of a group of at most 8 blocks); np pairs, nG groups
template <bool DUAL>
inline hipError_t launch_ginv_gemm(const GinvGemm& g, int np, int nG, hipStream_t stream) {
    const int nt = g.hs / GI_BM;
    const dim3 grid((unsigned)(nt * nt), (unsigned)np, (unsigned)nG), block(256);
    switch (g.hs / GI_BK) {
        case 4: hipLaunchKernelGGL((ginv_gemm_kernel<4, DUAL>), grid, block, 0, stream, g); break;
        case 8: hipLaunchKernelGGL((ginv_gemm_kernel<8, DUAL>), grid, block, 0, stream, g); break;
        case 16: hipLaunchKernelGGL((ginv_gemm_kernel<16, DUAL>), grid, block, 0, stream, g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ipm
