// ipm_api.hip -- C ABI of libipm_hip.so (see include/ipm_hip.h), the ONE translation unit of the library: it includes the
// kernel headers, then the host-side units (host_*.h) in dependency order, and holds ipm_create / ipm_destroy, the data
// setters and getters, bounds, certificate, history / schedule and the dense seams.
//
// One iteration (reference loop main.py:780-807) is a fixed sequence of
// launches on one HIP stream.  All scalars stay on the device; the host reads one small
// pinned record every `check_every` iterations.  Kernels of an iteration that follows a
// satisfied stop test are no-ops (they test Scalars::done first), so running ahead of the
// host check never changes the result.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <functional>
#include <vector>

#include "../../include/ipm_hip.h"
#include "gemm_nt_f64.h"
#include "adat_syrk_f64.h"
#include "chol_update_f64.h"
#include "potrf_f64.h"
#include "sparse_ops.h"
#include "trsv_grouped.h"
#include "ginv_gemm_f64.h"
#include "getrf_f64.h"
#include "small_lp.h"
#include "sparse_chol.h"
#include "sparse_symbolic.h"
#include "dense_split.h"
#include "vector_ops.h"
#include "refine_ops.h"
#include "form_factor.h"
#include "lockstep.h"
#include "lockstep_merge.h"
#include "chol_plan.h"
#include "equilibrate.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <chrono>
#include <limits>
#include <utility>

using namespace ipm;

#include "host_handle.h"
#include "host_compat.h"
#include "host_equilibrate.h"
#include "host_sparse_setup.h"
#include "host_residuals.h"
#include "host_factor_solve.h"
#include "host_fused.h"
#include "host_iteration.h"
#include "host_lockstep.h"
#include "host_lu.h"
#include "host_small_batch.h"

// ------------------------------------------------------------------------------- library
extern "C" int ipm_abi_version(void) { return IPM_ABI_VERSION; }

extern "C" int ipm_device_count(int* count) {
    if (!count) return fail(nullptr, IPM_ERR_INVALID_ARG, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail(nullptr, IPM_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = c;
    return IPM_OK;
}

extern "C" void ipm_default_options(ipm_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->eta = 0.91;
    o->pivot_guard_eps = 1e-30;
    o->pivot_guard_big = 1e64;
    o->check_every = 4;
}

extern "C" const char* ipm_last_error(const ipm_handle* h) { return h ? h->err : g_err; }

extern "C" int ipm_workspace_bytes(int64_t m, int64_t n, size_t* bytes) {
    if (!bytes || m <= 0 || n <= 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "bad arguments to ipm_workspace_bytes");
    *bytes = make_layout(m, n).total;
    return IPM_OK;
}

extern "C" int ipm_workspace_bytes_csc(int64_t m, int64_t n, int64_t nnz, size_t* bytes) {
    if (!bytes || m <= 0 || n <= 0 || nnz <= 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "bad arguments to ipm_workspace_bytes_csc");
    *bytes = make_layout(m, n, nnz).total;
    return IPM_OK;
}

extern "C" int ipm_workspace_bytes_opts(int64_t m, int64_t n, const ipm_options* opts, size_t* bytes) {
    if (!bytes || m <= 0 || n <= 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "bad arguments to ipm_workspace_bytes_opts");
    const int64_t nnz = opts && opts->sparse_nnz > 0 ? opts->sparse_nnz : 0;
    *bytes = make_layout(m, n, nnz, layout_no_dense(m, nnz, opts ? opts->flags : 0u)).total;
    return IPM_OK;
}

// ------------------------------------------------------------------------------- handle
// Guard bands of the workspace (IPM_TEST_ALLOC_GUARD, host_handle.h): the band behind every region -- from the last byte the region
// asked for to the next region, so the rounding to 256 is band too -- and the one before the first, filled on the handle's stream and
// entered in the registry under the handle.
static hipError_t guard_workspace(ipm_handle* h, const Layout& L) {
    char* base = (char*)h->ws;
    hipError_t e = hipMemsetAsync(base, L.band_byte, L.reg[0].off, h->stream);
    for (int r = 0; r < L.nreg && e == hipSuccess; ++r) {
        const size_t from = L.reg[r].off + L.reg[r].bytes, to = r + 1 < L.nreg ? L.reg[r + 1].off : L.total;
        e = hipMemsetAsync(base + from, L.band_byte, to - from, h->stream);
    }
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_guard_mutex);
    const int ordinal = g_guard_ordinal++;
    guard_register(h, h->stream, L.reg[0].name, 0, base, L.reg[0].off, base + L.reg[0].off, L.reg[0].bytes, h->device, L.band_byte, ordinal);
    for (int r = 0; r < L.nreg; ++r) {
        const size_t from = L.reg[r].off + L.reg[r].bytes, to = r + 1 < L.nreg ? L.reg[r + 1].off : L.total;
        guard_register(h, h->stream, L.reg[r].name, 1, base + from, to - from, base + L.reg[r].off, L.reg[r].bytes, h->device, L.band_byte, ordinal);
    }
    h->guarded = true;
    return hipSuccess;
}

// Every IPM_* switch ipm_create reads; what follows from them and the option flags (a flag overrides its switch) is decided in
// ipm_create.  Read at their own stage: IPM_SP_* (build_sparse_factor), IPM_FF_PROF / IPM_FF_TRACE_ITEMS (ff_build), IPM_LU_NB, ff_schedule.h,
// IPM_TEST_ALLOC_FILL, IPM_TEST_ALLOC_GUARD (at every allocation and in every make_layout: alloc_fill, alloc_guard, host_handle.h).
static void read_env_switches(ipm_handle* h) {
    if (const char* e = getenv("IPM_TEST_SPIN_LIMIT")) h->spin_limit = (unsigned)std::max(1, atoi(e));
    if (const char* e = getenv("IPM_ENVELOPE")) h->envelope = atoi(e);
    if (const char* e = getenv("IPM_LOOKAHEAD")) h->lookahead = atoi(e);
    if (const char* e = getenv("IPM_GROUPED_TRSV")) h->grouped_trsv = atoi(e);
    if (getenv("IPM_LS_BLOCK_STEPS")) h->ls_block_steps = true;
    if (const char* e = getenv("IPM_RAGGED_GROUPS")) h->ragged_groups = atoi(e) != 0;
    if (const char* e = getenv("IPM_FLAG_SYNC")) h->flag_sync = atoi(e);
    if (const char* e = getenv("IPM_BULK_VARIANT")) h->bulk_variant = atoi(e);
    if (const char* e = getenv("IPM_TWO_LEVEL")) h->two_level = atoi(e);
    if (const char* e = getenv("IPM_GROUP_STEPS")) h->group_steps = atoi(e);
    if (const char* e = getenv("IPM_FUSED_SMALL")) h->fused_small = atoi(e);
    if (const char* e = getenv("IPM_LIST_FORM")) h->list_form_opt = atoi(e);
    if (getenv("IPM_POTRF_STAMPS")) h->potrf_stamps = true;
    if (const char* e = getenv("IPM_FUSED_FACTOR")) { if (!strcmp(e, "force")) { h->ff_enabled = 1; h->ff_min_nblk = 3; h->ff_forced = true; } else h->ff_enabled = atoi(e); }
    if (const char* e = getenv("IPM_FF_MAX_NBLK")) h->ff_max_nblk = atoi(e);
    if (const char* e = getenv("IPM_FF_CHAIN_MODE")) h->ff_chain_mode0 = atoi(e) == 0;
    if (const char* e = getenv("IPM_FF_REF_ENGINE")) h->ff_ref_engine = atoi(e) != 0;
    if (const char* e = getenv("IPM_GINV_REF")) h->ginv_ref = atoi(e) != 0;
    if (const char* e = getenv("IPM_FF_Q"))h->ff_q = std::max(1, std::min(16, atoi(e)));
    if (const char* e = getenv("IPM_STREAM_AT")) h->stream_at = atoi(e);
}

// Group size of the grouped triangular solves (0: none).
// RAGGED groups (round 3): the block count need not be a multiple of the group size -- floor(nblk / gsz) full groups get
// their explicit inverses, the blocks left over at the end are substituted block by block (enqueue_potrs_grouped).  From
// 16 blocks on always groups of 8 (19 blocks: 2 groups + 3 steps, 28 launches per iteration's four sweeps + 10 for the
// inverses instead of 76); 9 .. 15 blocks: the largest of 8 / 4 that divides, else 8 + leftover; below 9 as before.
static int group_size(int nblk, bool ragged) {
    int gsz = 0;
    if (nblk >= 2 * GS_MAX) { if (ragged || nblk % GS_MAX == 0) gsz = GS_MAX; }
    else {
        for (int p2 = GS_MAX; p2 >= 2; p2 /= 2) if (nblk % p2 == 0) { gsz = p2; break; }
        if (ragged && nblk > GS_MAX && gsz < 4) gsz = GS_MAX;
    }
    return gsz;
}

extern "C" int ipm_create(int device, int64_t m, int64_t n, const ipm_options* opts, void* workspace,
                          size_t workspace_bytes, void* stream, ipm_handle** out) {
    if (!out) return fail(nullptr, IPM_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (m <= 0 || n <= 0 || m > (1 << 20) || n > (1 << 24)) return fail(nullptr, IPM_ERR_INVALID_ARG, "bad problem size %lld x %lld", (long long)m, (long long)n);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, IPM_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(nullptr, IPM_ERR_INVALID_ARG, "device %d out of range (%d visible)", device, ndev);
    static_assert(IPM_FLAG_LOCKSTEP_BOUNDS == 128, "the bit the Python host states (_lib.FLAG_LOCKSTEP_BOUNDS)");
    if (opts && (opts->flags & IPM_FLAG_LOCKSTEP_BOUNDS) && !(opts->flags & IPM_FLAG_LOCKSTEP))
        return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_create: IPM_FLAG_LOCKSTEP_BOUNDS without IPM_FLAG_LOCKSTEP (it opts a lockstep handle into the bounded twins, nothing else)");
    static_assert(IPM_FLAG_SMALL_FREE == 256, "the bit the Python host states (_lib.FLAG_SMALL_FREE)");
    if (opts && (opts->flags & IPM_FLAG_SMALL_FREE) && !(opts->flags & IPM_FLAG_SMALL_QUADRATIC))
        return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_create: IPM_FLAG_SMALL_FREE without IPM_FLAG_SMALL_QUADRATIC (a free column needs a quadratic term, and the term reaches the fused small path only with that flag)");
    static_assert(IPM_FLAG_DETECT_QUADRATIC == 512, "the bit the Python host states (_lib.FLAG_DETECT_QUADRATIC)");
    if (opts && (opts->flags & IPM_FLAG_DETECT_QUADRATIC) && !(opts->flags & IPM_FLAG_DETECT_INFEASIBILITY))
        return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_create: IPM_FLAG_DETECT_QUADRATIC without IPM_FLAG_DETECT_INFEASIBILITY (it opts a detecting handle into the tests of a quadratic problem, nothing else)");
    if (opts && (opts->flags & IPM_FLAG_DETECT_QUADRATIC) && (opts->flags & IPM_FLAG_LOCKSTEP))
        return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_create: IPM_FLAG_DETECT_QUADRATIC with IPM_FLAG_LOCKSTEP %s", compat_row(IPM_FEATURE_DETECT_QP, IPM_FEATURE_LOCKSTEP)->a_on);
    ipm_handle* h = new ipm_handle();
    h->device = device;
    if (opts) h->opt = *opts; else ipm_default_options(&h->opt);
    if (h->opt.check_every < 1) h->opt.check_every = 1;
    if (!(h->opt.eta > 0.0)) h->opt.eta = 0.91;
    if (!(h->opt.pivot_guard_big > 0.0)) h->opt.pivot_guard_big = 1e64;
    if (!(h->opt.regularize >= 0.0)) h->opt.regularize = 0.0;
    h->shift_rel = h->opt.regularize;
    read_env_switches(h);
    if (h->opt.sparse_nnz < 0) h->opt.sparse_nnz = 0;
    h->sparse = h->opt.sparse_nnz > 0;
    h->nnz_cap = h->opt.sparse_nnz;
    h->no_dense = layout_no_dense(m, h->opt.sparse_nnz, h->opt.flags);
    Layout L = make_layout(m, n, h->opt.sparse_nnz, h->no_dense);
    h->m = m; h->n = n; h->mp = L.mp; h->np = L.np; h->nblk = L.nblk;
    h->rc_chunks = L.rc_chunks; h->rows_per_chunk = L.rows_per_chunk; h->vblk = L.vblk;
    h->ws_bytes = L.total;
#define CREATE_TRY(call)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            int rc_ = fail(nullptr, IPM_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
            ipm_destroy(h);                                                                    \
            return rc_;                                                                        \
        }                                                                                      \
    } while (0)
    CREATE_TRY(hipSetDevice(device));
    if (stream) { h->stream = (hipStream_t)stream; }
    else { CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
    if (workspace) {
        if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) {
            int rc_ = fail(nullptr, IPM_ERR_WORKSPACE, "workspace too small or not 256-byte aligned (%zu < %zu)", workspace_bytes, L.total);
            ipm_destroy(h);
            return rc_;
        }
        h->ws = workspace;
    } else {
        CREATE_TRY(hipMalloc(&h->ws, L.total));
        h->own_ws = true;
    }
    char* base = (char*)h->ws;
    CREATE_TRY(alloc_fill(base, L.total, h->stream));      // test knob IPM_TEST_ALLOC_FILL (host_handle.h): before the uploads and the zeroing below
    h->A = (double*)(base + L.off_A);
    h->B = h->no_dense ? nullptr : (double*)(base + L.off_B);
    h->invD = h->no_dense ? nullptr : (double*)(base + L.off_inv);
    double* nv = (double*)(base + L.off_nvec);
    h->x = nv; h->s = nv + L.np; h->c = nv + 2 * L.np; h->rc = nv + 3 * L.np; h->d = nv + 4 * L.np;
    h->v = nv + 5 * L.np; h->q = nv + 6 * L.np; h->dxa = nv + 7 * L.np; h->dsa = nv + 8 * L.np;
    h->dx = nv + 9 * L.np; h->ds = nv + 10 * L.np;
    double* mv = (double*)(base + L.off_mvec);
    h->y = mv; h->b = mv + L.mp; h->rb = mv + 2 * L.mp; h->t1 = mv + 3 * L.mp; h->t2 = mv + 4 * L.mp;
    h->dya = mv + 5 * L.mp; h->dy = mv + 6 * L.mp;
    h->atp = (double*)(base + L.off_atp);
    h->part = (double*)(base + L.off_part);
    h->det = (double*)(base + L.off_det);
    h->sc = (Scalars*)(base + L.off_sc);
    h->fixed = (int*)(base + L.off_fixed);
    h->hist = (IterRec*)(base + L.off_hist);
    h->snap = (double*)(base + L.off_snap);
    h->slab = h->no_dense ? nullptr : (double*)(base + L.off_slab);
    h->d_tile_order = (int*)(base + L.off_order);
    {   // lower tiles enumerated super-block by super-block (8 x 8 tiles): the ~64 workgroups an XCD runs
        // at once then share 8 + 8 operand panels in that XCD's L2 instead of 1 + 64
        std::vector<int> order;
        const int nT = L.nblk, PB = 8;
        order.reserve((size_t)nT * (nT + 1) / 2);
        for (int I = 0; I * PB < nT; ++I)
            for (int J = 0; J <= I; ++J)
                for (int ti = I * PB; ti < nT && ti < (I + 1) * PB; ++ti)
                    for (int tj = J * PB; tj <= ti && tj < (J + 1) * PB; ++tj) order.push_back((ti << 16) | tj);
        CREATE_TRY(hipMemcpyAsync(h->d_tile_order, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice, h->stream));
        CREATE_TRY(hipStreamSynchronize(h->stream));
    }
    h->d_rowptr = (int*)(base + L.off_rowptr); h->d_colptr = (int*)(base + L.off_colptr);
    h->d_colind = (int*)(base + L.off_colind); h->d_rowind = (int*)(base + L.off_rowind);
    h->d_rval = (double*)(base + L.off_rval); h->d_cval = (double*)(base + L.off_cval);
    {   // test knob (see handoff.h): spin bound of the device-side hand-offs; set in every case, so that a later handle restores the default
        CREATE_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(ipm_spin_limit), &h->spin_limit, sizeof h->spin_limit, 0, hipMemcpyHostToDevice, h->stream));
        CREATE_TRY(hipStreamSynchronize(h->stream));
    }
    // zero everything except A and B (padding entries of every vector must stay 0)
    CREATE_TRY(hipMemsetAsync(base + L.off_inv, 0, L.off_slab - L.off_inv, h->stream));
    // test knob IPM_TEST_ALLOC_GUARD (host_handle.h): the bands are filled BEHIND that range memset, which runs across those between
    // inv and slab, and behind every upload above (none reaches a band: each writes the bytes its region asked for)
    if (L.band) CREATE_TRY(guard_workspace(h, L));
    {
        std::lock_guard<std::mutex> lock(g_hsc_mutex);
        if (!g_hsc_pool.empty()) { h->h_sc = g_hsc_pool.back(); g_hsc_pool.pop_back(); }
    }
    if (!h->h_sc) CREATE_TRY(hipHostMalloc((void**)&h->h_sc, sizeof(Scalars), hipHostMallocDefault));
    memset(h->h_sc, 0, sizeof(Scalars));
    CREATE_TRY(hipEventCreate(&h->ev0));
    CREATE_TRY(hipEventCreate(&h->ev1));
    h->detect = (h->opt.flags & IPM_FLAG_DETECT_INFEASIBILITY) != 0;
    h->detect_qp = (h->opt.flags & IPM_FLAG_DETECT_QUADRATIC) != 0;
    if (h->opt.flags & IPM_FLAG_LOCKSTEP) { h->lockstep = 1; h->opt.flags |= IPM_FLAG_SINGLE_STREAM | IPM_FLAG_NO_DEVICE_POLLING; }
    if (h->opt.flags & IPM_FLAG_SINGLE_STREAM) h->lookahead = 0;
    if (h->lockstep && h->ls_block_steps) h->grouped_trsv = 0;      // (A/B: block-step substitutions in the lockstep batch)
    if (h->lockstep) h->ss_small_blocks = 1 << 20;      // ONE panel / update kernel shape at every step: step k of all LPs of a batch then shares its launches
    if (h->no_dense) h->grouped_trsv = 0;      // the sparse factor has its own sweeps; a dense entry point on such a handle solves block by block
    h->gsz = h->grouped_trsv ? group_size(h->nblk, h->ragged_groups) : 0;      // (IPM_RAGGED_GROUPS=0 restores the old rule)
    if (h->gsz > 0) {
        const size_t nG = (size_t)h->nblk / h->gsz, GR = (size_t)h->gsz * 128;
        CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->gXT, sizeof(double) * nG * GR * GR));
        CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->gX, sizeof(double) * nG * GR * GR));
        CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->gS, sizeof(double) * nG * (GR / 2) * (GR / 2)));
        CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->gPart, sizeof(double) * 16 * (size_t)h->mp));
        // (stream-ordered: a plain hipMemset runs on the NULL stream, which the handle's non-blocking streams do not
        //  wait for -- it could land after the first group inverses were written and zero them)
        CREATE_TRY(hipMemsetAsync(h->gXT, 0, sizeof(double) * nG * GR * GR, h->stream));     // blocks below the block diagonal stay zero
        CREATE_TRY(hipMemsetAsync(h->gX, 0, sizeof(double) * nG * GR * GR, h->stream));      // blocks above the block diagonal stay zero
    } else {
        h->grouped_trsv = 0;
    }
    CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->d_flags, sizeof(unsigned) * (2 * (size_t)h->nblk + 4)));
    CREATE_TRY(hipMemsetAsync(h->d_flags, 0, sizeof(unsigned) * (2 * (size_t)h->nblk + 4), h->stream));
    CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->d_bulk_done, sizeof(unsigned) * (2 * (size_t)h->nblk + 4)));   // [0,nblk) bulk, [nblk,2nblk) crit
    CREATE_TRY(hipMemsetAsync(h->d_bulk_done, 0, sizeof(unsigned) * (2 * (size_t)h->nblk + 4), h->stream));
    if (h->opt.flags & IPM_FLAG_NO_DEVICE_POLLING) h->flag_sync = 0;
    if (h->potrf_stamps) { CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->stamp_buf, 8 * 64 * sizeof(long long))); CREATE_TRY(hipMemsetAsync(h->stamp_buf, 0, 8 * 64 * sizeof(long long), h->stream)); }
    if (lookahead_wanted(h->lookahead, h->nblk))           // (a single-stream handle creates no second stream: see stream3 below)
        CREATE_TRY(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    CREATE_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    // The residual stream exists only where it is used (dense handles from 16 blocks on): the HIP runtime maps streams onto a
    // handful of hardware queues in creation order, and an idle third stream per handle pushes the streams of the NEXT handle
    // onto queues that this handle's chain already occupies (two concurrent solves then serialise: tools/concurrency_probe.py)
    if (!h->sparse && h->lookahead != 0 && h->nblk >= 16)
        CREATE_TRY(hipStreamCreateWithFlags(&h->stream3, hipStreamNonBlocking));
    CREATE_TRY(hipEventCreateWithFlags(&h->ev_mid, hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&h->ev_res, hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&h->ev_grp, hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&h->ev_last, hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&h->ev_at, hipEventDisableTiming));
    if (h->ff_chain_mode0) {
        // 0 asked for the chain as three launches per step beside 224 workers: that structure met a recovered hand-off time-out and
        // has been removed.  Whoever asks for it by name is told so, not given another structure silently.
        int rc_ = fail(nullptr, IPM_ERR_INVALID_ARG, "IPM_FF_CHAIN_MODE=0 is not supported (that structure of the fused launch was removed)");
        ipm_destroy(h);
        return rc_;
    }
    h->ev_crit.assign(h->nblk, nullptr); h->ev_bulk.assign(h->nblk, nullptr);
    for (int k = 0; k < h->nblk; ++k) {
        CREATE_TRY(hipEventCreateWithFlags(&h->ev_crit[k], hipEventDisableTiming));
        CREATE_TRY(hipEventCreateWithFlags(&h->ev_bulk[k], hipEventDisableTiming));
    }
    if (h->sparse && h->mp <= SP_LDS_MAX_MP && device < MAX_DEVICES && !g_attr_set[device].load(std::memory_order_acquire)) {
        CREATE_TRY(hipFuncSetAttribute((const void*)adat_sparse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS_MAX_MP * 8));
        g_attr_set[device].store(true, std::memory_order_release);      // idempotent: a concurrent second call is harmless
    }
    hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 5000, 0, 1);
    CREATE_TRY(hipGetLastError());
    CREATE_TRY(hipStreamSynchronize(h->stream));
#undef CREATE_TRY
    if (device < MAX_DEVICES) { g_live[device].fetch_add(1, std::memory_order_acq_rel); h->counted = true; }
    *out = h;
    return IPM_OK;
}

extern "C" int ipm_destroy(ipm_handle* h) {
    if (!h) return IPM_OK;
    (void)hipSetDevice(h->device);
    if (h->ff_prof) ff_dump_profile(h);
    if (h->counted) g_live[h->device].fetch_sub(1, std::memory_order_acq_rel);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    for (auto& v : {&h->ev_crit, &h->ev_bulk})
        for (hipEvent_t e : *v) if (e) (void)hipEventDestroy(e);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->stream3) { (void)hipStreamSynchronize(h->stream3); (void)hipStreamDestroy(h->stream3); }
    if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
    if (h->ev_res) (void)hipEventDestroy(h->ev_res);
    if (h->ev_grp) (void)hipEventDestroy(h->ev_grp);
    if (h->ev_last) (void)hipEventDestroy(h->ev_last);
    if (h->ev_at) (void)hipEventDestroy(h->ev_at);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->h_sc) { std::lock_guard<std::mutex> lock(g_hsc_mutex); g_hsc_pool.push_back(h->h_sc); h->h_sc = nullptr; }
    if (h->guarded) {                                          // every stream is idle: compare the workspace's bands, log the damage
        const ipm_handle* self = h;
        guard_release([self](const GuardRec& r) { return r.owner == self; });
    }
    for (void* p : {(void*)h->stamp_buf, (void*)h->d_flags, (void*)h->d_bulk_done, (void*)h->B_own, (void*)h->invD_own, (void*)h->bnd_mem, (void*)h->quad_g, (void*)h->free_set.mark, (void*)h->free_lp_set.mark, (void*)h->mcc.mem, (void*)h->ref.mem, (void*)h->cert_mem, (void*)h->gXT, (void*)h->gX, (void*)h->gS, (void*)h->gPart})
        dev_free(h->device, h->stream, p);
    ff_release(h);
    free_sparse_factor(h);
    for (void* p : {(void*)h->sm_bptr, (void*)h->sm_bcol, (void*)h->sm_bi, (void*)h->sm_bk, (void*)h->sm_bcoef, (void*)h->ls_bi, (void*)h->ls_bk, (void*)h->ls_bak})
        dev_free(h->device, h->stream, p);
    if (h->own_ws && h->ws) (void)hipFree(h->ws);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return IPM_OK;
}

// ------------------------------------------------------------------------------- data
static bool all_finite(const double* p, int64_t rows, int64_t cols, int64_t ld) {
    for (int64_t i = 0; i < rows; ++i)
        for (int64_t j = 0; j < cols; ++j)
            if (!isfinite(p[i * ld + j])) return false;
    return true;
}

extern "C" int ipm_set_A_dense(ipm_handle* h, const double* A, int64_t ld, int is_device) {
    if (!h || !A || ld < h->n) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_A_dense: bad arguments");
    if (h->sparse) return fail(h, IPM_ERR_STATE, "ipm_set_A_dense: the handle was created for a sparse A (sparse_nnz > 0)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!is_device && !all_finite(A, h->m, h->n, ld)) return fail(h, IPM_ERR_INVALID_INPUT, "A has non-finite entries");
    if (int rc_ = eq_reset(h)) return rc_;
    HIP_TRY(h, hipMemsetAsync(h->A, 0, sizeof(double) * h->mp * h->np, h->stream));
    HIP_TRY(h, hipMemcpy2DAsync(h->A, sizeof(double) * h->np, A, sizeof(double) * ld, sizeof(double) * h->n, h->m,
                                is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->haveA = true; h->predictor_valid = false;
    return IPM_OK;
}

extern "C" int ipm_set_bc(ipm_handle* h, const double* b, const double* c) {
    if (!h || !b || !c) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_bc: bad arguments");
    if (!all_finite(b, 1, h->m, h->m) || !all_finite(c, 1, h->n, h->n)) return fail(h, IPM_ERR_INVALID_INPUT, "b or c has non-finite entries");
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<double> bs, cs;                                  // scaled handle: R b, C c (host_equilibrate.h)
    const double *b0 = b, *c0 = c;
    b = eq_in(h, bs, b, h->eq_r, false); c = eq_in(h, cs, c, h->eq_c, false);
    if (!eq_in_range(h, b0, b, (size_t)h->m) || !eq_in_range(h, c0, c, (size_t)h->n))
        return fail(h, IPM_ERR_INVALID_INPUT, "ipm_set_bc: the handle's scaling would push an entry of b or c out of the normal fp64 range");
    HIP_TRY(h, hipMemcpyAsync(h->b, b, sizeof(double) * h->m, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->c, c, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    enqueue_bc_norms(h);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->haveBC = true; h->predictor_valid = false;
    return IPM_OK;
}

// free columns (of either set) hold no s: every seam that writes a state zeroes it there
static int enqueue_free_zero_s(ipm_handle* h) {
    const ColumnSet& cs = h->free_set.on ? h->free_set : h->free_lp_set;      // (never both: host_compat.h refuses the pair)
    if (!cs.on) return IPM_OK;
    hipLaunchKernelGGL(free_zero_s_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, (const unsigned char*)cs.mark, h->s, (int)h->n);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

extern "C" int ipm_set_state(ipm_handle* h, const double* x, const double* y, const double* s) {
    if (!h || !x || !y || !s) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_state: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<double> xs, ys, ss;                              // scaled handle: x / C, y / R, s C
    x = eq_in(h, xs, x, h->eq_c, true); y = eq_in(h, ys, y, h->eq_r, true); s = eq_in(h, ss, s, h->eq_c, false);
    HIP_TRY(h, hipMemcpyAsync(h->x, x, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->y, y, sizeof(double) * h->m, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->s, s, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    if (int rc_ = enqueue_free_zero_s(h)) return rc_;              // free columns: s = 0, whatever was passed
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    mark_fresh_state(h);
    return IPM_OK;
}

extern "C" int ipm_get_state(ipm_handle* h, double* x, double* y, double* s) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_state: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    if (x) HIP_TRY(h, hipMemcpyAsync(x, h->x, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    if (y) HIP_TRY(h, hipMemcpyAsync(y, h->y, sizeof(double) * h->m, hipMemcpyDeviceToHost, h->stream));
    if (s) HIP_TRY(h, hipMemcpyAsync(s, h->s, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    eq_out(h, x, h->eq_c, false); eq_out(h, y, h->eq_r, false); eq_out(h, s, h->eq_c, true);      // scaled handle: C x', R y', s' / C
    return IPM_OK;
}

// Native upper bounds x_j <= u_j.  The bound vectors are the library's own allocation, made on first use and
// kept (a later ipm_set_bounds(h, NULL) only switches the bounded kernels off); the workspace is not involved.
extern "C" int ipm_set_bounds(ipm_handle* h, const double* u) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_bounds: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    int nU = 0;
    if (u) {
        for (int64_t j = 0; j < h->n; ++j) {
            const double v = u[j];
            if (!(v >= 0.0)) return fail(h, IPM_ERR_INVALID_INPUT, "ipm_set_bounds: u[%lld] = %g (bounds must be >= 0, +inf for none)", (long long)j, v);
            if (v < std::numeric_limits<double>::infinity()) {
                if (int rc_ = column_conflict(h, "ipm_set_bounds", IPM_FEATURE_BOUNDS, j, v)) return rc_;
                ++nU;
            }
        }
    }
    h->predictor_valid = false;
    if (nU == 0) {                                             // NULL or all +inf: the unbounded code, exactly
        h->bnd = false; h->bnd_nU = 0; h->bnd_finite.clear();
        if (h->haveBC) hipLaunchKernelGGL(norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->b, (int)h->m, &h->sc->b_norm);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return IPM_OK;
    }
    const size_t np = (size_t)h->np;
    if (!h->bnd_mem) {
        if (dev_malloc(h->device, h->stream, (void**)&h->bnd_mem, sizeof(double) * BND_VECS * np) != hipSuccess)
            return fail(h, IPM_ERR_HIP, "ipm_set_bounds: %d x %lld doubles could not be allocated", BND_VECS, (long long)np);
        HIP_TRY(h, hipMemsetAsync(h->bnd_mem, 0, sizeof(double) * BND_VECS * np, h->stream));
    }
    std::vector<double> uu(np, std::numeric_limits<double>::infinity());     // padding columns: unbounded
    std::copy(u, u + h->n, uu.begin());
    eq_out(h, uu.data(), h->eq_c, true);                        // scaled handle: u / C (+inf stays +inf)
    if (!eq_in_range(h, u, uu.data(), (size_t)h->n))
        return fail(h, IPM_ERR_INVALID_INPUT, "ipm_set_bounds: the handle's scaling would push a bound out of the normal fp64 range");
    HIP_TRY(h, hipMemcpyAsync(h->bnd_mem, uu.data(), sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
    h->bnd = true; h->bnd_nU = nU;
    h->bnd_finite.assign((size_t)h->n, 0);
    for (int64_t j = 0; j < h->n; ++j) h->bnd_finite[(size_t)j] = u[j] < std::numeric_limits<double>::infinity();
    const BndArgs bd = bnd_args(h);
    hipLaunchKernelGGL(bnd_fill_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, bd.u, bd.w, bd.z, (int)np, 1.0, 0);
    if (h->haveBC) hipLaunchKernelGGL(bnd_norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->b, (int)h->m, bd.u, (int)h->n, &h->sc->b_norm);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return IPM_OK;
}

// Separable convex QP: the diagonal g of the objective's quadratic term.  The vector is the library's own
// allocation, made on first use and kept (clearing only switches the Quad kernels off); the workspace is not involved.  The whole
// np-vector is written, so the padding is zero before any kernel reads it.
extern "C" int ipm_set_quadratic(ipm_handle* h, const double* g) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_quadratic: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    int64_t nnz = 0;
    if (g) {
        for (int64_t j = 0; j < h->n; ++j) {
            const double v = g[j];
            if (!(v >= 0.0) || !(v < std::numeric_limits<double>::infinity()))
                return fail(h, IPM_ERR_INVALID_INPUT, "ipm_set_quadratic: g[%lld] = %g (the diagonal must be finite and >= 0)", (long long)j, v);
            if (v > 0.0) ++nnz;
        }
    }
    for (int c : h->free_set.cols)
        if (int rc_ = column_conflict(h, "ipm_set_quadratic", IPM_FEATURE_QUADRATIC, c, g ? g[c] : 0.0)) return rc_;
    if (nnz == 0) {                                            // NULL or all zeros: the LP code, exactly
        h->quad = false; h->quad_nnz = 0; h->predictor_valid = false; h->quad_pos.clear();
        return IPM_OK;
    }
    if (int rc_ = compat_refuse(h, "ipm_set_quadratic", IPM_FEATURE_QUADRATIC)) return rc_;
    const size_t np = (size_t)h->np;
    std::vector<double> gg(np, 0.0);
    std::copy(g, g + h->n, gg.begin());
    if (h->scaled) {                                           // scaled handle: g C^2 (host_equilibrate.h), exact
        for (int64_t j = 0; j < h->n; ++j) gg[(size_t)j] = gg[(size_t)j] * h->eq_c[(size_t)j] * h->eq_c[(size_t)j];
        if (!eq_in_range(h, g, gg.data(), (size_t)h->n))
            return fail(h, IPM_ERR_INVALID_INPUT, "ipm_set_quadratic: the handle's scaling would push an entry of g out of the normal fp64 range");
    }
    if (!h->quad_g && dev_malloc(h->device, h->stream, (void**)&h->quad_g, sizeof(double) * np) != hipSuccess)
        return fail(h, IPM_ERR_HIP, "ipm_set_quadratic: %lld doubles could not be allocated", (long long)np);
    HIP_TRY(h, hipMemcpyAsync(h->quad_g, gg.data(), sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->quad = true; h->quad_nnz = nnz; h->predictor_valid = false;
    h->quad_pos.assign((size_t)h->n, 0);
    for (int64_t j = 0; j < h->n; ++j) h->quad_pos[(size_t)j] = g[j] > 0.0;
    return IPM_OK;
}

extern "C" int ipm_get_quadratic(ipm_handle* h, double* g, int64_t* nonzeros) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_quadratic: NULL handle");
    if (nonzeros) *nonzeros = h->quad ? h->quad_nnz : 0;
    if (!g) return IPM_OK;
    if (!h->quad) { std::fill(g, g + h->n, 0.0); return IPM_OK; }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(g, h->quad_g, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    eq_out(h, g, h->eq_c, true); eq_out(h, g, h->eq_c, true);      // scaled handle: g' / C^2
    return IPM_OK;
}

// The two column sets: free columns with curvature and LP free columns (columns without a quadratic
// term and without a sign constraint, served by proximal-point regularisation of the free block; iteration_rules.h: free_lp_*).  ONE
// setter body: `feature` names the set and its row of the compatibility table, rho (the LP set's extra; null for the other) is checked
// and stored with it.  The marks are the library's own allocation of np bytes, made on first use and kept (clearing only switches the
// set's kernels off); the whole vector is written, so the padding is zero before any kernel reads it.
static int set_column_set(ipm_handle* h, ColumnSet ipm_handle::*which, int feature, const char* who, const int32_t* idx, int32_t count, const double* rho_in = nullptr) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (count < 0) return fail(h, IPM_ERR_INVALID_ARG, "%s: count = %d", who, (int)count);
    ColumnSet& cs = h->*which;
    if (count == 0 || !idx) {                                  // cleared: the code without the set, exactly
        cs.cols.clear(); cs.host.clear(); cs.on = false; h->predictor_valid = false;
        return IPM_OK;
    }
    double rho = rho_in ? *rho_in : 0.0;
    if (!std::isfinite(rho)) return fail(h, IPM_ERR_INVALID_ARG, "%s: rho = %g is not finite", who, rho);
    if (!(rho > 0.0)) rho = IPM_FREE_LP_RHO_DEFAULT;
    if (int rc_ = compat_refuse(h, who, feature)) return rc_;
    std::vector<char> seen((size_t)h->n, 0);
    for (int32_t t = 0; t < count; ++t) {
        const int32_t j = idx[t];
        if (j < 0 || j >= h->n) return fail(h, IPM_ERR_INVALID_ARG, "%s: column index %d out of range", who, (int)j);
        if (seen[(size_t)j]) return fail(h, IPM_ERR_INVALID_ARG, "%s: column index %d is duplicated", who, (int)j);
        seen[(size_t)j] = 1;
        if (int rc_ = column_conflict(h, who, feature, j)) return rc_;
    }
    if ((int64_t)count >= h->n) return fail(h, IPM_ERR_INVALID_ARG, "%s: all %d columns free leaves no complementarity pair (mu would be 0/0)", who, (int)count);
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t np = (size_t)h->np;
    if (!cs.mark && dev_malloc(h->device, h->stream, (void**)&cs.mark, np) != hipSuccess)
        return fail(h, IPM_ERR_HIP, "%s: %lld bytes could not be allocated", who, (long long)np);
    std::vector<unsigned char> mk(np, 0);
    for (int32_t t = 0; t < count; ++t) mk[(size_t)idx[t]] = 1;
    HIP_TRY(h, hipMemcpyAsync(cs.mark, mk.data(), np, hipMemcpyHostToDevice, h->stream));
    cs.cols.assign(idx, idx + count); cs.host.swap(seen); cs.on = true; h->predictor_valid = false;
    if (rho_in) h->free_lp_rho = rho;
    if (int rc_ = enqueue_free_zero_s(h)) return rc_;              // a state the handle holds loses s on the new free columns
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return IPM_OK;
}
static int get_column_set(ipm_handle* h, ColumnSet ipm_handle::*which, const char* who, int32_t* idx, int32_t cap, int32_t* count) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (cap < 0 || (cap > 0 && !idx)) return fail(h, IPM_ERR_INVALID_ARG, "%s: bad arguments", who);
    const ColumnSet& cs = h->*which;
    const int32_t k = (int32_t)cs.cols.size();
    if (count) *count = k;
    for (int32_t t = 0; t < k && t < cap; ++t) idx[t] = cs.cols[(size_t)t];
    return IPM_OK;
}

extern "C" int ipm_set_free_columns(ipm_handle* h, const int32_t* idx, int32_t count) {
    return set_column_set(h, &ipm_handle::free_set, IPM_FEATURE_FREE, "ipm_set_free_columns", idx, count);
}
extern "C" int ipm_get_free_columns(ipm_handle* h, int32_t* idx, int32_t cap, int32_t* count) {
    return get_column_set(h, &ipm_handle::free_set, "ipm_get_free_columns", idx, cap, count);
}
extern "C" int ipm_set_free_lp_columns(ipm_handle* h, const int32_t* idx, int32_t count, double rho) {
    return set_column_set(h, &ipm_handle::free_lp_set, IPM_FEATURE_FREE_LP, "ipm_set_free_lp_columns", idx, count, &rho);
}
extern "C" int ipm_get_free_lp_columns(ipm_handle* h, int32_t* idx, int32_t cap, int32_t* count, double* rho) {
    const int rc = get_column_set(h, &ipm_handle::free_lp_set, "ipm_get_free_lp_columns", idx, cap, count);
    if (!rc && rho) *rho = h->free_lp_rho;
    return rc;
}

// test hook: a column vector of the iteration as the device holds it (the handle's units: no unscaling), n entries
extern "C" int ipm_debug_get_column_vector(ipm_handle* h, int32_t which, double* out) {
    if (!h || !out || which < 0 || which > 3) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_get_column_vector: bad arguments");
    const double* src[4] = {h->rc, h->d, h->v, h->q};
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, src[which], sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return IPM_OK;
}

extern "C" int ipm_set_bound_state(ipm_handle* h, const double* w, const double* z) {
    if (!h || !w || !z) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_bound_state: bad arguments");
    if (!h->bnd) return fail(h, IPM_ERR_STATE, "ipm_set_bound_state: no finite bound is set (ipm_set_bounds)");
    HIP_TRY(h, hipSetDevice(h->device));
    const BndArgs bd = bnd_args(h);
    std::vector<double> wsc, zsc;                                // scaled handle: w / C, z C
    w = eq_in(h, wsc, w, h->eq_c, true); z = eq_in(h, zsc, z, h->eq_c, false);
    HIP_TRY(h, hipMemcpyAsync(bd.w, w, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(bd.z, z, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(bnd_fill_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, bd.u, bd.w, bd.z, (int)h->n, 0.0, 1);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->predictor_valid = false; h->fresh_state = true;
    return IPM_OK;
}

extern "C" int ipm_get_bound_state(ipm_handle* h, double* w, double* z) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_bound_state: NULL handle");
    if (!h->bnd) return fail(h, IPM_ERR_STATE, "ipm_get_bound_state: no finite bound is set (ipm_set_bounds)");
    HIP_TRY(h, hipSetDevice(h->device));
    const BndArgs bd = bnd_args(h);
    if (w) HIP_TRY(h, hipMemcpyAsync(w, bd.w, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    if (z) HIP_TRY(h, hipMemcpyAsync(z, bd.z, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    eq_out(h, w, h->eq_c, false); eq_out(h, z, h->eq_c, true);      // scaled handle: C w', z' / C
    return IPM_OK;
}

static int enqueue_init_state(ipm_handle* h, double y0) {
    int gn = (int)((h->n + 255) / 256), gm = (int)((h->m + 255) / 256);
    hipLaunchKernelGGL(fill_kernel, dim3(gn), dim3(256), 0, h->stream, h->x, (int)h->n, 1.0);
    hipLaunchKernelGGL(fill_kernel, dim3(gn), dim3(256), 0, h->stream, h->s, (int)h->n, 1.0);
    hipLaunchKernelGGL(fill_kernel, dim3(gm), dim3(256), 0, h->stream, h->y, (int)h->m, y0);
    if (h->bnd) {                                                   // w = z = 1 on U (0 outside)
        const BndArgs bd = bnd_args(h);
        hipLaunchKernelGGL(bnd_fill_kernel, dim3(gn), dim3(256), 0, h->stream, bd.u, bd.w, bd.z, (int)h->n, 1.0, 0);
    }
    HIP_TRY(h, hipGetLastError());
    return enqueue_free_zero_s(h);                                  // free columns: x = 1 like every column, s = 0
}

extern "C" int ipm_init_state(ipm_handle* h, double y0) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_init_state: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = enqueue_init_state(h, y0);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    mark_fresh_state(h);
    return IPM_OK;
}

// diagnostic: copy the s_memtime stamps of the first diagonal-block factorization (8 waves x 64 slots)
extern "C" int ipm_debug_get_stamps(ipm_handle* h, long long* out) {
    if (!h || !out || !h->stamp_buf) return fail(h, IPM_ERR_STATE, "stamps not enabled (IPM_POTRF_STAMPS=1)");
    HIP_TRY(h, hipMemcpyAsync(out, h->stamp_buf, 8 * 64 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return IPM_OK;
}

extern "C" int ipm_set_profiling(ipm_handle* h, int enable) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_profiling: NULL handle");
    h->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return IPM_OK;
}
extern "C" int ipm_get_phase_ms(ipm_handle* h, double out[4]) {
    if (!h || !out) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_phase_ms: bad arguments");
    for (int i = 0; i < 4; ++i) out[i] = h->phase_ms[i];
    return IPM_OK;
}

// ------------------------------------------------------------------------------- infeasibility detection
extern "C" int ipm_set_infeasibility_tol(ipm_handle* h, double eps_p, double eps_d) {
    if (!h || !(eps_p > 0.0) || !(eps_d > 0.0) || !(eps_p < 1.0) || !(eps_d < 1.0))
        return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_infeasibility_tol: tolerances must lie in (0, 1)");
    h->det_eps_p = eps_p; h->det_eps_d = eps_d;
    return IPM_OK;
}

extern "C" int ipm_get_certificate(ipm_handle* h, double* y, double* z, double* x, double info[4]) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_certificate: NULL handle");
    const int status = h->h_sc ? h->h_sc->status : 0;
    if (status != IPM_STATUS_PRIMAL_INFEASIBLE && status != IPM_STATUS_DUAL_INFEASIBLE)
        return fail(h, IPM_ERR_STATE, "ipm_get_certificate: the last solve ended in status %d, not in an infeasibility detection (5 / 6)", status);
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    if (!h->cert_mem) HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->cert_mem, sizeof(double) * (2 * n + m)));
    const unsigned grid = (unsigned)std::min<size_t>((std::max(n, m) + 255) / 256, 256);
    hipLaunchKernelGGL(certificate_kernel, dim3(grid), dim3(256), 0, h->stream, h->x, h->y, h->bnd ? bnd_args(h).z : nullptr, h->det,
                       (int)m, (int)n, h->cert_mem);
    HIP_TRY(h, hipGetLastError());
    double rec[4];
    HIP_TRY(h, hipMemcpyAsync(rec, h->det, sizeof rec, hipMemcpyDeviceToHost, h->stream));
    if (x) HIP_TRY(h, hipMemcpyAsync(x, h->cert_mem, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (y) HIP_TRY(h, hipMemcpyAsync(y, h->cert_mem + n, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream));
    if (z) HIP_TRY(h, hipMemcpyAsync(z, h->cert_mem + n + m, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    eq_out(h, x, h->eq_c, false); eq_out(h, y, h->eq_r, false); eq_out(h, z, h->eq_c, true);      // scaled handle: a certificate of the caller's LP
    if (info) for (int i = 0; i < 4; ++i) info[i] = rec[i];
    return IPM_OK;
}

extern "C" int ipm_get_history(ipm_handle* h, ipm_iter_record* out, int32_t capacity, int32_t* count) {
    if (!h || !count || capacity < 0 || (capacity > 0 && !out)) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_history: bad arguments");
    static_assert(sizeof(ipm_iter_record) == sizeof(IterRec), "history record layout");
    HIP_TRY(h, hipSetDevice(h->device));
    int k = 0;
    HIP_TRY(h, hipMemcpyAsync(&k, &h->sc->k, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int nrec = std::min(std::min(k, HIST_CAP), (int)capacity);
    if (nrec > 0) {
        std::vector<IterRec> ring(HIST_CAP);
        HIP_TRY(h, hipMemcpyAsync(ring.data(), h->hist, sizeof(IterRec) * HIST_CAP, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < nrec; ++i) memcpy(&out[i], &ring[(size_t)(k - nrec + i) % HIST_CAP], sizeof(IterRec));
    }
    *count = nrec;
    return IPM_OK;
}

static const int SCHEDULE_WORDS = 14;
extern "C" int ipm_get_schedule_words(ipm_handle* h, int32_t* out, int32_t capacity, int32_t* count) {
    if (!h || !out || capacity < 0) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_schedule_words: bad arguments");
    const int live = live_on_device(h);
    int32_t w[SCHEDULE_WORDS];
    w[0] = h->nblk; w[1] = h->last_gs; w[2] = h->grouped_trsv;
    w[3] = (may_poll(h) && live <= 1) ? 1 : 0;
    w[4] = h->n_counter_steps; w[5] = h->n_event_steps; w[6] = h->use_env ? 1 : 0; w[7] = live;
    w[8] = h->timeouts_recovered; w[9] = h->small ? 1 : 0;
    w[10] = h->ff_last ? 1 : 0; w[11] = (h->spf && sp_level(h)) ? 1 : 0;
    w[12] = stream_at_on(h) ? 1 : 0;
    w[13] = h->grouped_trsv ? h->gsz : 0;
    const int n = std::min<int>(capacity, SCHEDULE_WORDS);
    memcpy(out, w, sizeof(int32_t) * (size_t)n);
    if (count) *count = n;
    return IPM_OK;
}
extern "C" int ipm_get_schedule(ipm_handle* h, int32_t out[12]) {
    if (!h || !out) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_schedule: bad arguments");
    return ipm_get_schedule_words(h, out, 12, nullptr);
}

extern "C" int ipm_debug_at_pieces(int32_t nblk, int32_t layout[4], int32_t* pieces, int32_t capacity, int32_t* count) {
    if (nblk < 1 || nblk > (1 << 13) || !layout || !count) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_debug_at_pieces: bad arguments");
    const Layout L = make_layout((int64_t)nblk * NB, 64);
    if (layout[0] <= 0) layout[0] = (int32_t)L.mp;
    if (layout[1] <= 0) layout[1] = group_size(nblk, true);
    if (layout[2] <= 0) layout[2] = L.rc_chunks;
    if (layout[3] <= 0) layout[3] = L.rows_per_chunk;
    const std::vector<AtPiece> ev = at_piece_schedule(layout[0], layout[1], nblk, layout[2], layout[3]);
    *count = (int32_t)ev.size();
    if (pieces) for (size_t e = 0; e < ev.size() && (int64_t)e < capacity; ++e) { pieces[3 * e] = ev[e].first_row; pieces[3 * e + 1] = ev[e].chunk0; pieces[3 * e + 2] = ev[e].chunk1; }
    return IPM_OK;
}

extern "C" int ipm_debug_chol_plan(int32_t nblk, int64_t m, const int32_t knobs[6], const int32_t* env_last, int32_t totals[5], int32_t* steps,
                                   int32_t capacity) {
    if (nblk < 1 || nblk > (1 << 13) || !knobs || !totals) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_debug_chol_plan: bad arguments");
    static_assert(CHOL_STEP_WORDS == IPM_CHOL_STEP_WORDS && sizeof(CholStep) == sizeof(int32_t) * IPM_CHOL_STEP_WORDS, "plan record layout");
    const int64_t mp = (int64_t)nblk * NB;
    const bool la = lookahead_wanted(knobs[0], nblk);
    const CholPlan p = chol_step_plan(nblk, m > 0 && m <= mp ? m : mp, mp, la, la && knobs[1] != 0, knobs[2], knobs[3], knobs[4], knobs[5] != 0, env_last);
    totals[0] = p.lookahead; totals[1] = p.polling; totals[2] = p.gs; totals[3] = p.n_counter_steps; totals[4] = p.n_event_steps;
    if (steps && capacity >= nblk) memcpy(steps, p.steps.data(), sizeof(CholStep) * (size_t)nblk);
    return IPM_OK;
}

// The variant tables, read back (host only; tests/test_step_dispatch_host.py, tests/test_free_lp_host.py): the row that serves a
// class at a step.  ipm_debug_step_kernel is the four-switch entry, ipm_debug_step_kernel_ex adds the fifth (LP free columns).
static int debug_step_kernel(const char* who, int32_t step, unsigned bits, char* name_out, int32_t capacity, int32_t* twin_type_out);
extern "C" int ipm_debug_step_kernel(int32_t step, int32_t bounded, int32_t detect, int32_t quad, int32_t free_cols, char* name_out, int32_t capacity,
                                     int32_t* twin_type_out) {
    return debug_step_kernel("ipm_debug_step_kernel", step, variant_bits(StepVariant{bounded != 0, detect != 0, quad != 0, free_cols != 0}), name_out, capacity, twin_type_out);
}
extern "C" int ipm_debug_step_kernel_ex(int32_t step, int32_t bounded, int32_t detect, int32_t quad, int32_t free_cols, int32_t free_lp, char* name_out,
                                        int32_t capacity, int32_t* twin_type_out) {
    return debug_step_kernel("ipm_debug_step_kernel_ex", step, variant_bits(StepVariant{bounded != 0, detect != 0, quad != 0, free_cols != 0, free_lp != 0}), name_out, capacity, twin_type_out);
}
// The compatibility table, read back (host only; tests/test_compat_table_host.py, tests/test_gpu_compat_orders.py).
extern "C" int ipm_debug_compat(int32_t a, int32_t b, int32_t* excluded, int32_t* lifted_by) {
    if (a < 0 || a >= IPM_FEATURE_COUNT || b < 0 || b >= IPM_FEATURE_COUNT) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_debug_compat: feature id outside 0 .. %d", IPM_FEATURE_COUNT - 1);
    const CompatRow* r = compat_row(a, b);
    if (excluded) *excluded = r != nullptr;
    if (lifted_by) *lifted_by = r ? r->lifted_by : -1;
    return IPM_OK;
}
// The guard bands, read back (IPM_TEST_ALLOC_GUARD, host_handle.h; tests/test_alloc_guard_host.py, tests/test_gpu_alloc_guard.py).
// A handle's bands: its workspace's and those of the pool blocks allocated on its stream.
static std::vector<ipm_guard_band> guard_snapshot(const ipm_handle* h) {
    std::vector<ipm_guard_band> v;
    std::lock_guard<std::mutex> lock(g_guard_mutex);
    for (const GuardRec& r : g_guard_live)
        if (!h || r.owner == h || (!r.owner && r.stream == h->stream && r.b.device == h->device)) v.push_back(r.b);
    std::sort(v.begin(), v.end(), [](const ipm_guard_band& a, const ipm_guard_band& b) { return a.ordinal != b.ordinal ? a.ordinal < b.ordinal : a.address < b.address; });
    return v;
}
static int guard_copy_out(const std::vector<ipm_guard_band>& v, ipm_guard_band* out, int32_t capacity, int32_t* count) {
    for (size_t i = 0; out && i < v.size() && (int64_t)i < capacity; ++i) out[i] = v[i];
    *count = (int32_t)v.size();
    return IPM_OK;
}
extern "C" int ipm_debug_guard_list(ipm_handle* h, ipm_guard_band* out, int32_t capacity, int32_t* count) {
    if (!count || capacity < 0) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_guard_list: bad arguments");
    return guard_copy_out(guard_snapshot(h), out, capacity, count);
}
extern "C" int ipm_debug_guard_check(ipm_handle* h, ipm_guard_band* out, int32_t capacity, int32_t* count) {
    if (!count || capacity < 0) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_guard_check: bad arguments");
    std::vector<ipm_guard_band> v = guard_snapshot(h), bad;
    bool synced[MAX_DEVICES] = {};
    for (ipm_guard_band& b : v) {
        if (b.device >= 0 && b.device < MAX_DEVICES && !synced[b.device]) {      // every stream of the device: nothing is still writing
            HIP_TRY(h, hipSetDevice(b.device));
            HIP_TRY(h, hipDeviceSynchronize());
            synced[b.device] = true;
        }
        guard_check_band(b);
        if (b.bad_count != 0) bad.push_back(b);
    }
    return guard_copy_out(bad, out, capacity, count);
}
extern "C" int ipm_debug_guard_log(ipm_guard_band* out, int32_t capacity, int32_t* count) {
    if (!count || capacity < 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_debug_guard_log: bad arguments");
    std::vector<ipm_guard_band> v;
    { std::lock_guard<std::mutex> lock(g_guard_mutex); v.swap(g_guard_log); }
    return guard_copy_out(v, out, capacity, count);
}
extern "C" int ipm_debug_guard_layout(int64_t m, int64_t n, const ipm_options* opts, ipm_guard_band* out, int32_t capacity, int32_t* count,
                                      uint64_t* total, uint64_t* band) {
    if (!count || capacity < 0 || m <= 0 || n <= 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_debug_guard_layout: bad arguments");
    const int64_t nnz = opts && opts->sparse_nnz > 0 ? opts->sparse_nnz : 0;
    const Layout L = make_layout(m, n, nnz, layout_no_dense(m, nnz, opts ? opts->flags : 0u));
    std::vector<ipm_guard_band> v((size_t)L.nreg);
    for (int r = 0; r < L.nreg; ++r) {
        ipm_guard_band& b = v[(size_t)r];
        memset(&b, 0, sizeof b);
        snprintf(b.tag, sizeof b.tag, "%s", L.reg[r].name);
        const size_t from = L.reg[r].off + L.reg[r].bytes, to = r + 1 < L.nreg ? L.reg[r + 1].off : L.total;
        b.address = b.inner = L.reg[r].off; b.inner_bytes = L.reg[r].bytes; b.bytes = L.band ? to - from : 0;
        b.side = 1; b.device = -1; b.byte = L.band_byte; b.ordinal = r; b.first_bad = -1;
    }
    if (total) *total = L.total;
    if (band) *band = L.band;
    return guard_copy_out(v, out, capacity, count);
}
extern "C" int ipm_debug_guard_compare(const unsigned char* band, uint64_t bytes, int32_t byte, int64_t* first_bad, int64_t* bad_count) {
    if (!band || !first_bad || !bad_count || byte < 0 || byte > 255) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_debug_guard_compare: bad arguments");
    guard_compare(band, (size_t)bytes, byte, first_bad, bad_count);
    return IPM_OK;
}
static int debug_step_kernel(const char* who, int32_t step, unsigned bits, char* name_out, int32_t capacity, int32_t* twin_type_out) {
    static const StepTable* const steps[] = {&STEP_PREPARE, &STEP_STOP_TEST, &STEP_SCALING, &STEP_DIRECTION, &STEP_MU_AFF, &STEP_CORRECTOR_RHS, &STEP_UPDATE};
    static const StepTable* const starts[] = {&STEP_START_PRIMAL, &STEP_START_DUAL, &STEP_START_SHIFT, &STEP_START_PRIMAL_CORRECT, &STEP_START_DUAL_CORRECT};
    static_assert(sizeof steps / sizeof *steps == IPM_STEP_SMALL && IPM_STEP_START_PRIMAL + sizeof starts / sizeof *starts == IPM_STEP_COUNT, "the step ids of ipm_hip.h");
    if (step < 0 || step >= IPM_STEP_COUNT || capacity < 0 || (capacity > 0 && !name_out)) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: bad arguments", who);
    if (!variant_legal(bits & ~V_L)) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: free columns without a quadratic term are no class (a free column needs g > 0)", who);
    if (!variant_legal(bits)) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: LP free columns beside a quadratic term, free columns with curvature or the infeasibility tests are no class", who);
    if ((bits & V_L) && step >= IPM_STEP_SMALL && step < IPM_STEP_START_PRIMAL) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: the one-workgroup path serves no LP free columns", who);
    const char* name;
    int id;
    if (step >= IPM_STEP_SMALL && step < IPM_STEP_START_PRIMAL) {          // the one-workgroup path: the row's id is its SMALL_* value / bounded
        const bool start = step >= IPM_STEP_SMALL_START, batch = step == IPM_STEP_SMALL_BATCH || step == IPM_STEP_SMALL_START_BATCH;
        id = start ? small_row_of(SMALL_START_ROWS, bits & V_B) : small_row_of(SMALL_ROWS, bits);
        const SmallRow& row = start ? SMALL_START_ROWS[id] : SMALL_ROWS[id];
        name = batch ? row.batch_name : row.name;
    } else {
        const StepRow* row = step_row(step < IPM_STEP_SMALL ? *steps[step] : *starts[step - IPM_STEP_START_PRIMAL], bits);
        name = row->name; id = row->twin;
    }
    if (capacity > 0) snprintf(name_out, (size_t)capacity, "%s", name);
    if (twin_type_out) *twin_type_out = id;
    return IPM_OK;
}

// ------------------------------------------------------------------------------- kernel-level entry points
extern "C" int ipm_form_normal_matrix(ipm_handle* h, const double* d, double* B, int64_t ldb) {
    if (!h || !d || !B || ldb < h->m) return fail(h, IPM_ERR_INVALID_ARG, "ipm_form_normal_matrix: bad arguments");
    if (!h->haveA) return fail(h, IPM_ERR_STATE, "ipm_form_normal_matrix: A not set");
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, 0);
    HIP_TRY(h, hipMemcpyAsync(h->d, d, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    int rc = enqueue_form(h, h->d, /*dense_image=*/true);
    if (rc) return rc;
    std::vector<double> tmp((size_t)h->mp * h->mp);
    HIP_TRY(h, hipMemcpyAsync(tmp.data(), h->B, sizeof(double) * h->mp * h->mp, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // tiles strictly above the block diagonal are not computed: mirror from the lower triangle
    for (int64_t i = 0; i < h->m; ++i)
        for (int64_t j = 0; j < h->m; ++j)
            B[i * ldb + j] = (j <= i) ? tmp[i * h->mp + j] : tmp[j * h->mp + i];
    h->predictor_valid = false;
    return IPM_OK;
}

extern "C" int ipm_normal_solve(ipm_handle* h, const double* d, const double* rhs, double* z, int reuse_factor,
                                int32_t* pivots_fixed) {
    if (!h || !rhs || !z) return fail(h, IPM_ERR_INVALID_ARG, "ipm_normal_solve: bad arguments");
    if (!h->haveA) return fail(h, IPM_ERR_STATE, "ipm_normal_solve: A not set");
    int rc = rounds_check_path(h, h->ref, "ipm_normal_solve");
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    for (int attempt = 0;; ++attempt) {                     // second pass only after a recovered poll time-out
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, 1);
        if (!reuse_factor) {
            if (d) {
                HIP_TRY(h, hipMemcpyAsync(h->d, d, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
            } else {
                hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->d, (int)h->n, 1.0);
            }
            if ((rc = enqueue_form(h, h->d))) return rc;
            if ((rc = enqueue_factor(h))) return rc;
            if ((rc = enqueue_group_inverses(h))) return rc;
        }
        HIP_TRY(h, hipMemsetAsync(h->t1, 0, sizeof(double) * h->mp, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->t1, rhs, sizeof(double) * h->m, hipMemcpyHostToDevice, h->stream));
        if ((rc = rounds_start(h, h->ref, true))) return rc;
        // refinement against A diag(h->d) A^T: only its rounds need A^T z (h->atp is free here)
        if ((rc = enqueue_normal_solve(h, h->t1, h->dy, h->ref.k > 0 ? h->atp : nullptr, /*refine=*/true))) return rc;
        bool tmo = false;
        if ((rc = read_scalars(h, &tmo))) return rc;
        if (!tmo) break;
        if (attempt || reuse_factor) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
        poll_fallback(h);
    }
    HIP_TRY(h, hipMemcpyAsync(z, h->dy, sizeof(double) * h->m, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (pivots_fixed) *pivots_fixed = h->h_sc->fixed;
    h->predictor_valid = false;
    return IPM_OK;
}

extern "C" int ipm_get_factor(ipm_handle* h, double* L, int64_t ldl) {
    if (!h || !L || ldl < h->m) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_factor: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc_ = ensure_dense_B(h)) return rc_;
    if (h->spf) {                       // dense image of the sparse factor (the dense B buffer is free in this mode)
        HIP_TRY(h, hipMemsetAsync(h->B, 0, sizeof(double) * h->mp * h->mp, h->stream));
        hipLaunchKernelGGL(sp_expand_kernel, dim3((unsigned)h->spF.nsn), dim3(256), 0, h->stream, h->spF, h->B, (long long)h->mp);
        HIP_TRY(h, hipGetLastError());
    }
    std::vector<double> tmp((size_t)h->mp * h->mp);
    HIP_TRY(h, hipMemcpyAsync(tmp.data(), h->B, sizeof(double) * h->mp * h->mp, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < h->m; ++i)
        for (int64_t j = 0; j < h->m; ++j) L[i * ldl + j] = (j <= i) ? tmp[i * h->mp + j] : 0.0;
    return IPM_OK;
}

extern "C" int ipm_solve_linear(ipm_handle* h, const double* B, int64_t ldb, const double* rhs, double* z, int32_t* pivots_fixed) {
    if (!h || !B || !rhs || !z || ldb < h->m) return fail(h, IPM_ERR_INVALID_ARG, "ipm_solve_linear: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc_ = ensure_dense_B(h)) return rc_;
    const int64_t m = h->m, mp = h->mp;
    std::vector<double> img((size_t)mp * mp, 0.0);
    for (int64_t i = 0; i < mp; ++i) {
        if (i < m) memcpy(&img[(size_t)i * mp], B + i * ldb, sizeof(double) * m);
        else img[(size_t)i * mp + i] = 1.0;
    }
    const bool saved_env = h->use_env;
    h->use_env = false;                                   // an arbitrary dense B: no structure to exploit
    struct SpOff { ipm_handle* h; ~SpOff() { h->spf_off = false; } } sp_off{h};
    h->spf_off = true;                                    // ... and not the sparse factor of the handle's own A
    int rc = IPM_OK;
    for (int attempt = 0;; ++attempt) {                   // second pass only after a recovered poll time-out
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, 1);
        hipError_t e = hipMemcpyAsync(h->B, img.data(), sizeof(double) * mp * mp, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(h->t1, 0, sizeof(double) * mp, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h->t1, rhs, sizeof(double) * m, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) { h->use_env = saved_env; return fail(h, IPM_ERR_HIP, "ipm_solve_linear: upload failed: %s", hipGetErrorString(e)); }
        rc = enqueue_factor(h);
        if (!rc) rc = enqueue_group_inverses(h);
        if (!rc) rc = enqueue_potrs(h, h->t1, h->dy);
        bool tmo = false;
        if (!rc) rc = read_scalars(h, &tmo);
        if (rc || !tmo) break;
        if (attempt) { rc = fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events"); break; }
        poll_fallback(h);
    }
    h->use_env = saved_env;
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(z, h->dy, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (pivots_fixed) *pivots_fixed = h->h_sc->fixed;
    h->predictor_valid = false;
    return IPM_OK;
}
