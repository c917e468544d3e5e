// lockstep.h -- the LOCKSTEP BATCH of the batched-LP mode (gfx950): iteration k of SEVERAL independent LPs in the SAME launches.
//
// Why.  A Netlib-size LP is a chain of ~100 small dependent launches per interior-point iteration (reference loop:
// main.py:780-807; the driver loop being batched: script.py:147-173).  Solving several LPs at once from several streams does
// not overlap more than FOUR of those chains: HIP multiplexes the streams onto four hardware queues, two streams of one queue
// serialise, and more queues are slower (profiles/r04_netlib_*_rejected.txt) -- the 73-LP suite is bound at (sum of the chains) / 4.
// What raises the concurrency is not more chains but kernels that serve several LPs per launch: the grids of the LPs of a step
// are packed back to back into ONE 1-D grid, the arguments of every LP's launch come from a device table (LsRec), and a block
// finds its LP with one wave-wide load of the start offsets + a ballot (LS_ENTER below) -- no surplus blocks, whatever the size
// mix.  The launch count of a batch iteration is then that of its LONGEST program, not the sum.
//
// How.  Nothing about an LP's arithmetic changes: the handle's own launch sequence (enqueue_iteration, single-stream path) is
// RECORDED once -- every launch site is one launch_twin<T> call (host_handle.h; the types: LsTwin<T> below), which records (kernel
// type, grid, argument struct) instead of launching -- and the records of all LPs are merged, each LP's order preserved, into global steps of one kernel type each (host_lockstep.h: ls_merge).  The device
// code of a step is the body of the kernel the handle would have launched (X_kernel_body, shared with the one-LP kernels), so a
// lockstep solve is BIT-IDENTICAL to the same handle solved alone (tests/test_gpu_lockstep.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

#include "chol_update_f64.h"
#include "gemm_nt_f64.h"
#include "potrf_f64.h"
#include "sparse_ops.h"
#include "trsv_grouped.h"
#include "vector_ops.h"

struct ipm_handle;      // (include/ipm_hip.h; defined in host_handle.h)

namespace ipm {

enum LsType {
    LS_SPMV_CSR = 0, LS_SPMV_CSC_T, LS_PREPARE, LS_STOP_TEST, LS_ZERO, LS_ADAT_LIST, LS_ADAT_SPARSE, LS_ADAT_SPARSE_GLOBAL, LS_MAXDIAG,
    LS_POTRF, LS_GEMM_32_128_32, LS_GEMM_64_64_16, LS_GEMM_64_128_16, LS_GEMM_128_128_16, LS_GEMM_32_32_32, LS_CHOL_UPDATE, LS_TRSV_FWD, LS_TRSV_BWD,
    LS_DIRECTION, LS_MU_AFF, LS_CORR_RHS, LS_UPDATE, LS_GEMV_N, LS_GEMV_T, LS_SUB_PARTIALS, LS_GROUP_DIAG_T, LS_GEMM_32_32_32_BATCHED,
    LS_PREPARE_DETECT, LS_STOP_TEST_DETECT, LS_NTYPES
};

// The bounded twins (IPM_FLAG_LOCKSTEP_BOUNDS): the eight bounded vector steps of the single-stream iteration, types of their own so
// that the wrappers above them and every single-LP kernel compile to what they compiled to before.  Their ids continue LsType's --
// which is why LsTwin, ls_kernel, record_twin and launch_twin are keyed on int: a value past LS_NTYPES is no LsType.
enum LsBndType {
    LS_PREPARE_BND = LS_NTYPES, LS_PREPARE_DETECT_BND, LS_STOP_TEST_BND, LS_STOP_TEST_DETECT_BND, LS_DIRECTION_BND, LS_MU_AFF_BND, LS_CORR_RHS_BND,
    LS_UPDATE_BND, LS_NTYPES_ALL
};

constexpr int LS_ARG_BYTES = 304;
constexpr int LS_MAX_GROUP = 64;              // LPs per launch: the block -> LP look-up is one wave-wide load + ballot
struct LsRec {                                // one LP's share of one global step
    unsigned gridx;                           // blocks of this LP's launch
    unsigned lds;                             // dynamic LDS bytes of this LP's launch (adat_sparse_kernel only)
    unsigned start;                           // first block of this LP inside the step's 1-D grid (the grids are packed back to back:
                                              // a 2-D grid of max-gridx x LPs would dispatch tens of thousands of blocks that leave at once)
    unsigned pad_;
    alignas(8) unsigned char args[LS_ARG_BYTES];
};

// (the four of the vector steps are filled from a handle at a step, corr = the direction step's: the constructors, host_handle.h)
struct LsVecA { VecArgs a; int corr; LsVecA(ipm_handle* h, int corr); };
struct LsVecDet { VecArgs a; DetArgs dt; LsVecDet(ipm_handle* h, int corr); };             // the infeasibility tests of a handle with IPM_FLAG_DETECT_INFEASIBILITY
struct LsVecBnd { VecArgs a; int corr; BndArgs bd; LsVecBnd(ipm_handle* h, int corr); };   // a handle with native upper bounds (ipm_set_bounds) ...
struct LsVecBndDet { VecArgs a; BndArgs bd; DetArgs dt; LsVecBndDet(ipm_handle* h, int corr); };   // ... and with the infeasibility tests
struct LsSpmv { SparseA A; int mp; const double* v; double sa, sb; const double* add; double* out; const int* done; };
struct LsSpmvT { SparseA A; int np; const double* u; double* w; const int* done; };
struct LsZero { double* p; int64_t n; const int* done; };
struct LsAdatList { const int *bptr, *bi, *bk, *bcol; const double *bai, *bak; int nb; const double* d; double* B; int64_t ldb; int m, mp; const int* done; };
struct LsAdatSp { SparseA A; const double* d; double* B; int64_t ldb; int mp; const int* done; };
struct LsGemvN { const double* A; int64_t lda; int mp, np; const double* v; double sa, sb; const double* add; double* out; const int* done; };
struct LsGemvT { const double* A; int64_t lda; int rows_per_chunk, np; const double* u; double* part; const int* done; unsigned gx; };   // gx: blocks per row chunk
struct LsSubPart { double* z; const double* part; int np, rc; const int* done; };
struct LsGroupDiagT { const double* invD; double* XT; double* X; int b0, GS; const int* done; };
struct LsMaxdiag { const double* B; int64_t ld; int n; double* out; const int* done; };

// block -> (LP, block of that LP's launch): the LPs' first blocks are ascending; every wave looks its own block up
#define LS_ENTER(ARGT)                                                                                                  \
    const unsigned lane_ = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));                          \
    const unsigned s_ = lane_ < count ? recs[lane_].start : 0xffffffffu;                                                \
    const int lp_ = __popcll(__ballot(s_ <= blockIdx.x)) - 1;                                                           \
    const LsRec& r_ = recs[lp_];                                                                                        \
    const unsigned bx = blockIdx.x - r_.start;                                                                          \
    const ARGT& p = *reinterpret_cast<const ARGT*>(r_.args)

// ONE DECLARATION PER TYPE, next to its ls_* wrapper kernel: LsTwin<T> = the argument struct, the block dimension and `single`, the
// launch of the single-LP kernel from that struct with the field list the wrapper passes to X_kernel_body.  launch_twin<T> (host
// side) records the struct or calls `single`; ls_launch takes wrapper and block dimension from here.  The GEMM types state `is`
// instead -- the launcher instantiation they record: launch_gemm_nt / launch_chol_update hand their struct to ls_gemm_hook.
template <int T> struct LsTwin;
template <int T> using LsArgs = typename LsTwin<T>::Args;
template <class A, unsigned THREADS> struct LsTwinOf {
    static_assert(sizeof(A) <= LS_ARG_BYTES && std::is_trivially_copyable<A>::value, "LsRec::args");
    using Args = A;
    static constexpr unsigned threads = THREADS;
    static dim3 block() { return dim3(THREADS); }
};
// `single` of a type whose single-LP kernel has the 1-D grid of the record
#define LS_SINGLE(KERNEL, ...)                                                                                          \
    static void single(const Args& p, unsigned grid, unsigned lds, hipStream_t st) { hipLaunchKernelGGL(KERNEL, dim3(grid), block(), lds, st, __VA_ARGS__); }
// head of the wrapper kernel of type T (optional: the second argument of __launch_bounds__), bound to the type for ls_launch
using LsKernel = void (*)(const LsRec*, unsigned);
template <int T> inline constexpr LsKernel ls_kernel = nullptr;
#define LS_KERNEL(T, NAME, ...)                                                                                         \
    __global__ __launch_bounds__(LsTwin<T>::threads, ##__VA_ARGS__) void NAME(const LsRec* recs, const unsigned count); \
    template <> inline constexpr LsKernel ls_kernel<T> = NAME;                                                          \
    __global__ __launch_bounds__(LsTwin<T>::threads, ##__VA_ARGS__) void NAME(const LsRec* recs, const unsigned count)

template <> struct LsTwin<LS_SPMV_CSR> : LsTwinOf<LsSpmv, 256> { LS_SINGLE(spmv_csr_kernel, p.A, p.mp, p.v, p.sa, p.sb, p.add, p.out, p.done) };
LS_KERNEL(LS_SPMV_CSR, ls_spmv_csr) { LS_ENTER(LsArgs<LS_SPMV_CSR>); spmv_csr_kernel_body(p.A, p.mp, p.v, p.sa, p.sb, p.add, p.out, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_SPMV_CSC_T> : LsTwinOf<LsSpmvT, 256> { LS_SINGLE(spmv_csc_t_kernel, p.A, p.np, p.u, p.w, p.done) };
LS_KERNEL(LS_SPMV_CSC_T, ls_spmv_csc_t) { LS_ENTER(LsArgs<LS_SPMV_CSC_T>); spmv_csc_t_kernel_body(p.A, p.np, p.u, p.w, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_PREPARE> : LsTwinOf<LsVecA, VBLK> { LS_SINGLE(prepare_kernel, p.a) };
LS_KERNEL(LS_PREPARE, ls_prepare) { LS_ENTER(LsArgs<LS_PREPARE>); prepare_kernel_body(p.a, bx, r_.gridx); }
template <> struct LsTwin<LS_STOP_TEST> : LsTwinOf<LsVecA, 64> { LS_SINGLE(stop_test_kernel, p.a) };
LS_KERNEL(LS_STOP_TEST, ls_stop_test) { LS_ENTER(LsArgs<LS_STOP_TEST>); stop_test_kernel_body(p.a, bx, r_.gridx); }
template <> struct LsTwin<LS_PREPARE_DETECT> : LsTwinOf<LsVecDet, VBLK> { LS_SINGLE(prepare_detect_kernel, p.a) };
LS_KERNEL(LS_PREPARE_DETECT, ls_prepare_detect) { LS_ENTER(LsArgs<LS_PREPARE_DETECT>); prepare_kernel_body<false, true>(p.a, bx, r_.gridx); }
template <> struct LsTwin<LS_STOP_TEST_DETECT> : LsTwinOf<LsVecDet, 64> { LS_SINGLE(stop_test_detect_kernel, p.a, p.dt) };
LS_KERNEL(LS_STOP_TEST_DETECT, ls_stop_test_detect) { LS_ENTER(LsArgs<LS_STOP_TEST_DETECT>); stop_test_kernel_body<false, true>(p.a, bx, r_.gridx, BndArgs{}, p.dt); }
template <> struct LsTwin<LS_ZERO> : LsTwinOf<LsZero, 256> { LS_SINGLE(zero_unless_done_kernel, p.p, p.n, p.done) };
LS_KERNEL(LS_ZERO, ls_zero) { LS_ENTER(LsArgs<LS_ZERO>); zero_unless_done_kernel_body(p.p, p.n, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_ADAT_LIST> : LsTwinOf<LsAdatList, 256> { LS_SINGLE(adat_list_kernel, p.bptr, p.bi, p.bk, p.bcol, p.bai, p.bak, p.nb, p.d, p.B, p.ldb, p.m, p.mp, p.done) };
LS_KERNEL(LS_ADAT_LIST, ls_adat_list) {
    LS_ENTER(LsArgs<LS_ADAT_LIST>);
    adat_list_kernel_body(p.bptr, p.bi, p.bk, p.bcol, p.bai, p.bak, p.nb, p.d, p.B, p.ldb, p.m, p.mp, p.done, bx, r_.gridx);
}
// (the one type with dynamic LDS: `lds` of the launch site, the largest among the LPs of a step in ls_launch)
template <> struct LsTwin<LS_ADAT_SPARSE> : LsTwinOf<LsAdatSp, 256> { LS_SINGLE(adat_sparse_kernel, p.A, p.d, p.B, p.ldb, p.mp, p.done) };
LS_KERNEL(LS_ADAT_SPARSE, ls_adat_sparse) { LS_ENTER(LsArgs<LS_ADAT_SPARSE>); adat_sparse_kernel_body(p.A, p.d, p.B, p.ldb, p.mp, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_ADAT_SPARSE_GLOBAL> : LsTwinOf<LsAdatSp, 256> { LS_SINGLE(adat_sparse_global_kernel, p.A, p.d, p.B, p.ldb, p.mp, p.done) };
LS_KERNEL(LS_ADAT_SPARSE_GLOBAL, ls_adat_sparse_global) { LS_ENTER(LsArgs<LS_ADAT_SPARSE_GLOBAL>); adat_sparse_global_kernel_body(p.A, p.d, p.B, p.ldb, p.mp, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_MAXDIAG> : LsTwinOf<LsMaxdiag, 256> { LS_SINGLE(maxdiag_kernel, p.B, p.ld, p.n, p.out, p.done) };
LS_KERNEL(LS_MAXDIAG, ls_maxdiag) { LS_ENTER(LsArgs<LS_MAXDIAG>); maxdiag_kernel_body(p.B, p.ld, p.n, p.out, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_POTRF> : LsTwinOf<PotrfDiag, PD_THREADS> { LS_SINGLE(potrf_diag_kernel<false>, p) };
LS_KERNEL(LS_POTRF, ls_potrf) {
    LS_ENTER(LsArgs<LS_POTRF>);
    if (p.done && *p.done) return;                           // (no signal word on this path: a lockstep handle never polls)
    __shared__ __attribute__((aligned(16))) double W[NB * WLD];
    __shared__ double dinv_s[NB];
    potrf_diag_body<false>(p, W, dinv_s);
}
template <int BM, int BN, int BK, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN) / 2 < 2 ? 1 : 2) void ls_gemm(const LsRec* recs, const unsigned count) {
    LS_ENTER(GemmNT);
    if (p.done && *p.done) return;
    __shared__ __attribute__((aligned(16))) double lds[2 * (BM + BN) * (BK + 2)];
    gemm_nt_body<BM, BN, BK, WM, WN, false>(p, (int)bx, 0, 0, lds);
}
template <int BM_, int BN_, int BK_, int WM_, int WN_> struct LsGemmTwin : LsTwinOf<GemmNT, 64 * WM_ * WN_> {
    static constexpr bool is(int bm, int bn, int bk, int wm, int wn) { return bm == BM_ && bn == BN_ && bk == BK_ && wm == WM_ && wn == WN_; }   // the instantiation of launch_gemm_nt this type records
};
#define LS_GEMM_TWIN(T, ...)                                                                                            \
    template <> struct LsTwin<T> : LsGemmTwin<__VA_ARGS__> {};                                                          \
    template <> inline constexpr LsKernel ls_kernel<T> = ls_gemm<__VA_ARGS__>;
LS_GEMM_TWIN(LS_GEMM_32_128_32, 32, 128, 32, 1, 8)
LS_GEMM_TWIN(LS_GEMM_64_64_16, 64, 64, 16, 2, 2)
LS_GEMM_TWIN(LS_GEMM_64_128_16, 64, 128, 16, 2, 2)
LS_GEMM_TWIN(LS_GEMM_128_128_16, 128, 128, 16, 2, 2)
LS_GEMM_TWIN(LS_GEMM_32_32_32, 32, 32, 32, 2, 2)
template <> struct LsTwin<LS_CHOL_UPDATE> : LsTwinOf<GemmNT, 256> { static constexpr bool is(int bm, int, int, int, int) { return bm == -1; } };      // (what launch_chol_update hands to the hook)
LS_KERNEL(LS_CHOL_UPDATE, ls_chol_update, 2) { LS_ENTER(LsArgs<LS_CHOL_UPDATE>); chol_update_kernel_body(p, bx, r_.gridx); }
template <> struct LsTwin<LS_TRSV_FWD> : LsTwinOf<TrsvStep, 256> { LS_SINGLE(trsv_fwd_step_kernel, p) };
LS_KERNEL(LS_TRSV_FWD, ls_trsv_fwd) { LS_ENTER(LsArgs<LS_TRSV_FWD>); trsv_fwd_step_kernel_body(p, bx, r_.gridx); }
template <> struct LsTwin<LS_TRSV_BWD> : LsTwinOf<TrsvStep, 256> { LS_SINGLE(trsv_bwd_step_kernel, p) };
LS_KERNEL(LS_TRSV_BWD, ls_trsv_bwd) { LS_ENTER(LsArgs<LS_TRSV_BWD>); trsv_bwd_step_kernel_body(p, bx, r_.gridx); }
template <> struct LsTwin<LS_DIRECTION> : LsTwinOf<LsVecA, VBLK> { LS_SINGLE(direction_kernel, p.a, p.corr) };
LS_KERNEL(LS_DIRECTION, ls_direction) { LS_ENTER(LsArgs<LS_DIRECTION>); direction_kernel_body(p.a, p.corr, bx, r_.gridx); }
template <> struct LsTwin<LS_MU_AFF> : LsTwinOf<LsVecA, VBLK> { LS_SINGLE(mu_aff_kernel, p.a) };
LS_KERNEL(LS_MU_AFF, ls_mu_aff) { LS_ENTER(LsArgs<LS_MU_AFF>); mu_aff_kernel_body(p.a, bx, r_.gridx); }
template <> struct LsTwin<LS_CORR_RHS> : LsTwinOf<LsVecA, VBLK> { LS_SINGLE(corrector_rhs_kernel, p.a) };
LS_KERNEL(LS_CORR_RHS, ls_corr_rhs) { LS_ENTER(LsArgs<LS_CORR_RHS>); corrector_rhs_kernel_body(p.a, bx, r_.gridx); }
template <> struct LsTwin<LS_UPDATE> : LsTwinOf<LsVecA, VBLK> { LS_SINGLE(update_kernel, p.a) };
LS_KERNEL(LS_UPDATE, ls_update) { LS_ENTER(LsArgs<LS_UPDATE>); update_kernel_body(p.a, bx, r_.gridx); }
// the bounded twins: the Bounded instantiation of the same bodies, `single` = the *_bounded*_kernel of vector_ops.h
template <> struct LsTwin<LS_PREPARE_BND> : LsTwinOf<LsVecBnd, VBLK> { LS_SINGLE(prepare_bounded_kernel, p.a, p.bd) };
LS_KERNEL(LS_PREPARE_BND, ls_prepare_bnd) { LS_ENTER(LsArgs<LS_PREPARE_BND>); prepare_kernel_body<true>(p.a, bx, r_.gridx, p.bd); }
template <> struct LsTwin<LS_PREPARE_DETECT_BND> : LsTwinOf<LsVecBndDet, VBLK> { LS_SINGLE(prepare_bounded_detect_kernel, p.a, p.bd) };
LS_KERNEL(LS_PREPARE_DETECT_BND, ls_prepare_detect_bnd) { LS_ENTER(LsArgs<LS_PREPARE_DETECT_BND>); prepare_kernel_body<true, true>(p.a, bx, r_.gridx, p.bd); }
template <> struct LsTwin<LS_STOP_TEST_BND> : LsTwinOf<LsVecBnd, 64> { LS_SINGLE(stop_test_bounded_kernel, p.a, p.bd) };
LS_KERNEL(LS_STOP_TEST_BND, ls_stop_test_bnd) { LS_ENTER(LsArgs<LS_STOP_TEST_BND>); stop_test_kernel_body<true>(p.a, bx, r_.gridx, p.bd); }
template <> struct LsTwin<LS_STOP_TEST_DETECT_BND> : LsTwinOf<LsVecBndDet, 64> { LS_SINGLE(stop_test_bounded_detect_kernel, p.a, p.bd, p.dt) };
LS_KERNEL(LS_STOP_TEST_DETECT_BND, ls_stop_test_detect_bnd) { LS_ENTER(LsArgs<LS_STOP_TEST_DETECT_BND>); stop_test_kernel_body<true, true>(p.a, bx, r_.gridx, p.bd, p.dt); }
template <> struct LsTwin<LS_DIRECTION_BND> : LsTwinOf<LsVecBnd, VBLK> { LS_SINGLE(direction_bounded_kernel, p.a, p.corr, p.bd) };
LS_KERNEL(LS_DIRECTION_BND, ls_direction_bnd) { LS_ENTER(LsArgs<LS_DIRECTION_BND>); direction_kernel_body<true>(p.a, p.corr, bx, r_.gridx, p.bd); }
template <> struct LsTwin<LS_MU_AFF_BND> : LsTwinOf<LsVecBnd, VBLK> { LS_SINGLE(mu_aff_bounded_kernel, p.a, p.bd) };
LS_KERNEL(LS_MU_AFF_BND, ls_mu_aff_bnd) { LS_ENTER(LsArgs<LS_MU_AFF_BND>); mu_aff_kernel_body<true>(p.a, bx, r_.gridx, p.bd); }
template <> struct LsTwin<LS_CORR_RHS_BND> : LsTwinOf<LsVecBnd, VBLK> { LS_SINGLE(corrector_rhs_bounded_kernel, p.a, p.bd) };
LS_KERNEL(LS_CORR_RHS_BND, ls_corr_rhs_bnd) { LS_ENTER(LsArgs<LS_CORR_RHS_BND>); corrector_rhs_kernel_body<true>(p.a, bx, r_.gridx, p.bd); }
template <> struct LsTwin<LS_UPDATE_BND> : LsTwinOf<LsVecBnd, VBLK> { LS_SINGLE(update_bounded_kernel, p.a, p.bd) };
LS_KERNEL(LS_UPDATE_BND, ls_update_bnd) { LS_ENTER(LsArgs<LS_UPDATE_BND>); update_kernel_body<true>(p.a, bx, r_.gridx, p.bd); }

template <> struct LsTwin<LS_GEMV_N> : LsTwinOf<LsGemvN, 256> { LS_SINGLE(gemv_n_kernel, p.A, p.lda, p.mp, p.np, p.v, p.sa, p.sb, p.add, p.out, p.done) };
LS_KERNEL(LS_GEMV_N, ls_gemv_n) { LS_ENTER(LsArgs<LS_GEMV_N>); gemv_n_kernel_body(p.A, p.lda, p.mp, p.np, p.v, p.sa, p.sb, p.add, p.out, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_GEMV_T> : LsTwinOf<LsGemvT, 256> {      // single-LP grid (gx, row chunks), packed as gx * chunks
    static void single(const Args& p, unsigned grid, unsigned, hipStream_t st) {
        hipLaunchKernelGGL(gemv_t_kernel, dim3(p.gx, grid / p.gx), block(), 0, st, p.A, p.lda, p.rows_per_chunk, p.np, p.u, p.part, p.done);
    }
};
LS_KERNEL(LS_GEMV_T, ls_gemv_t) { LS_ENTER(LsArgs<LS_GEMV_T>); gemv_t_kernel_body(p.A, p.lda, p.rows_per_chunk, p.np, p.u, p.part, p.done, bx % p.gx, bx / p.gx); }
template <> struct LsTwin<LS_SUB_PARTIALS> : LsTwinOf<LsSubPart, 256> { LS_SINGLE(sub_partials_kernel, p.z, p.part, p.np, p.rc, p.done) };
LS_KERNEL(LS_SUB_PARTIALS, ls_sub_partials) { LS_ENTER(LsArgs<LS_SUB_PARTIALS>); sub_partials_kernel_body(p.z, p.part, p.np, p.rc, p.done, bx, r_.gridx); }
template <> struct LsTwin<LS_GROUP_DIAG_T> : LsTwinOf<LsGroupDiagT, 32 * 8> {      // block (32, 8); single-LP grid (4, 4, blocks), packed as 16 * blocks
    static dim3 block() { return dim3(32, 8); }
    static void single(const Args& p, unsigned grid, unsigned, hipStream_t st) {
        hipLaunchKernelGGL(group_diag_transpose_kernel, dim3(4, 4, grid / 16), block(), 0, st, p.invD, p.XT, p.X, p.b0, p.GS, p.done);
    }
};
LS_KERNEL(LS_GROUP_DIAG_T, ls_group_diag_t) {
    LS_ENTER(LsArgs<LS_GROUP_DIAG_T>);
    group_diag_transpose_kernel_body(p.invD, p.XT, p.X, p.b0, p.GS, p.done, bx & 3u, (bx >> 2) & 3u, bx >> 4);
}
// the batched form of the NT contraction (group inverses: blockIdx.y = pair, blockIdx.z = group), its 3-D grid packed
template <> struct LsTwin<LS_GEMM_32_32_32_BATCHED> : LsGemmTwin<32, 32, 32, 2, 2> {};
LS_KERNEL(LS_GEMM_32_32_32_BATCHED, ls_gemm_32_batched, 2) {
    LS_ENTER(LsArgs<LS_GEMM_32_32_32_BATCHED>);
    if (p.done && *p.done) return;
    __shared__ __attribute__((aligned(16))) double lds[2 * (32 + 32) * (32 + 2)];
    const unsigned gx = (unsigned)p.n_direct;
    gemm_nt_body<32, 32, 32, 2, 2, false>(p, (int)(bx % gx), (int)((bx / gx) % (unsigned)p.batch), (int)(bx / (gx * (unsigned)p.batch)), lds);
}

// launch one global step: `count` (<= LS_MAX_GROUP) LPs, `blocks` = the sum of their grids, `lds` = the largest dynamic LDS among them
template <int... T> inline hipError_t ls_launch_in(std::integer_sequence<int, T...>, int type, const LsRec* d_recs, unsigned count, unsigned blocks, unsigned lds, hipStream_t st) {
    static const struct { LsKernel kernel; dim3 block; } step[] = {{ls_kernel<T>, LsTwin<T>::block()}...};
    if (type < 0 || type >= LS_NTYPES_ALL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(step[type].kernel, dim3(blocks), step[type].block, lds, st, d_recs, count);
    return hipGetLastError();
}
inline hipError_t ls_launch(int type, const LsRec* d_recs, unsigned count, unsigned blocks, unsigned lds, hipStream_t st) {
    return ls_launch_in(std::make_integer_sequence<int, LS_NTYPES_ALL>{}, type, d_recs, count, blocks, lds, st);
}

}  // namespace ipm
