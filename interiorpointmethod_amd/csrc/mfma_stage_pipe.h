// mfma_stage_pipe.h -- the software-pipelined stage schedule of the fp64 MFMA (v_mfma_f64_16x16x4_f64) GEMM-NT kernels for
// gfx950, stated once.  adat_syrk_kernel (adat_syrk_f64.h) and chol_update_kernel / ls_chol_update (chol_update_f64.h) ARE
// this loop with their own loads, LDS stores and fragment reads.  ff_gemm_pair and ff_gemm_pipe (form_factor.h) follow the
// same schedule on copies of their own -- see the end of this comment.
//
// A wave holds NI x NJ MFMA tiles in `acc`; a stage is KS k-steps of 4 columns (BK = 4 KS) of both operands in one of two
// LDS buffers (stage s in buffer s & 1).  Against the plain double-buffered loop (gemm_nt_f64_kernel, ff_gemm: read the
// fragments, wait, multiply; store the next stage; barrier) the schedule of one stage differs in two things:
//
//   * Fragment reads are software pipelined one k-step ahead through two register sets: the ds_reads of k-step kk + 1 are
//     issued before the NI x NJ MFMAs of k-step kk, so no LDS latency is exposed inside a stage.  The generic kernel reads
//     all fragments of two k-steps, waits, multiplies (two exposed LDS round trips per BK = 16 stage).
//   * The stage barrier sits BEFORE the last k-step instead of after it: the next stage's operands (their global loads
//     were issued a whole stage earlier) are written to the other LDS buffer between the MFMA rows of k-step KS - 2 -- the
//     waits for the loads sit behind NJ MFMAs each instead of in front of all of them --, the barrier follows, and the
//     loads of stage s + 2 and the first fragments of stage s + 1 go out in front of the MFMAs of k-step KS - 1, whose
//     fragments are in registers already: the MFMA stream of a wave continues across the stage boundary.
//
// Every __builtin_amdgcn_sched_barrier(0) below pins that order against the compiler's scheduler; the throughput rests on
// their placement (0.87 - 0.90 of the fp64 MFMA peak standalone: adat_syrk_f64.h).  The MFMA sequence per
// accumulator is k-step by k-step, stage by stage: results are bit-identical to the plain loop.
//
// An engine supplies what differs, as callables:
//   issue_loads(s)              global loads of stage s into the engine's staging registers
//   store_stage(buf)            the staging registers -> LDS buffer `buf`, the whole stage (prologue)
//   store_behind_row(buf, i)    the slice of them that goes behind MFMA row i of k-step KS - 2 (all i < NI: the whole stage)
//   read_frags(a, b, buf, kk)   fragments of k-step kk of buffer `buf` into a[NI] (rows of P) and b[NJ] (rows of Q)
//
// The engines of the fused launch (form_factor.h) are NOT on this template.  They add a second form of the last k-step (MFMA
// row 0 first, loads and fragment reads between the rows, no branch in the loop) and waves that only stage; both were written
// into this template and the result compiled.  form_factor_roles_kernel_mfma_first, the launch that runs, sits at 256 VGPRs,
// and its register allocation did not survive either engine going through the template: 4 -> 19 spilled VGPRs with
// ff_gemm_pair on it, 4 -> 2 with ff_gemm_pipe alone, spill code inside the stage loops moving in both cases
// (profiles/stage_pipe_isa_parent_vs_this.txt).  A changed loop is not a refactor, so they keep their copies until that
// kernel has register headroom.
#pragma once
#include <hip/hip_runtime.h>
#include "gemm_nt_f64.h"

namespace ipm {

// acc += P Q^T over stages [s_begin, s_end), s_begin < s_end.  Every wave of the workgroup calls it (stage barriers).
template <int KS, int NI, int NJ, class IssueLoads, class StoreStage, class StoreBehindRow, class ReadFrags>
__device__ __forceinline__ void mfma_stage_pipe(const int s_begin, const int s_end, f64x4 (&acc)[NI][NJ], const IssueLoads& issue_loads,
                                                const StoreStage& store_stage, const StoreBehindRow& store_behind_row,
                                                const ReadFrags& read_frags_into) {
    static_assert(KS >= 4 && KS % 2 == 0, "k-step kk uses fragment set kk & 1; the last two k-steps are peeled");
    double fa[2][NI], fb[2][NJ];                                // two fragment register sets
    auto read_frags = [&](int set, int buf, int kk) { read_frags_into(fa[set], fb[set], buf, kk); };
    auto mfma_row = [&](int set, int i) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[set][i], fb[set][j], acc[i][j], 0, 0, 0);
    };
    auto mfma_all = [&](int set) {
#pragma unroll
        for (int i = 0; i < NI; ++i) mfma_row(set, i);
    };

    // ---- prologue: stage s_begin into LDS, loads of stage s_begin + 1 in flight, first fragments in set 0
    issue_loads(s_begin);
    store_stage(s_begin & 1);
    __syncthreads();
    if (s_begin + 1 < s_end) issue_loads(s_begin + 1);
    read_frags(0, s_begin & 1, 0);

    for (int s = s_begin; s < s_end; ++s) {
        const int buf = s & 1;
        const bool more = s + 1 < s_end;
#pragma unroll
        for (int kk = 0; kk < KS - 2; ++kk) {                   // k-steps 0 .. KS-3: prefetch kk + 1, multiply kk
            read_frags((kk + 1) & 1, buf, kk + 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_all(kk & 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        read_frags(1, buf, KS - 1);                             // fragments of the last k-step, before the barrier
        __builtin_amdgcn_sched_barrier(0);
        // k-step KS-2, with the next stage's operands written to the other LDS buffer between its MFMA rows
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            mfma_row(0, i);
            if (more) store_behind_row(buf ^ 1, i);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                        // writes of stage s+1 visible; reads of stage s issued
        if (s + 2 < s_end) issue_loads(s + 2);
        if (more) read_frags(0, buf ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mfma_all(1);                                            // k-step KS-1
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace ipm
