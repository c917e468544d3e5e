// ipm_api.hip -- C ABI of libipm_hip.so (see include/ipm_hip.h): handle, workspace layout
// in HBM, and the per-iteration launch sequence of the Mehrotra predictor-corrector step.
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
#include <vector>

#include "../../include/ipm_hip.h"
#include "gemm_nt_f64.h"
#include "adat_syrk_f64.h"
#include "chol_update_f64.h"
#include "potrf_f64.h"
#include "sparse_ops.h"
#include "trsv_grouped.h"
#include "getrf_f64.h"
#include "small_lp.h"
#include "sparse_chol.h"
#include "sparse_symbolic.h"
#include "vector_ops.h"
#include "form_factor.h"
#include "lockstep.h"
#include "lockstep_merge.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <chrono>
#include <limits>
#include <utility>

using namespace ipm;

static thread_local char g_err[512] = "";

// Live handles per device.  The device-polled hand-offs of the Cholesky look-ahead are only safe while ONE handle
// drives the GPU (its two streams then sit on hardware queues of their own); with more than one live handle on a
// device every factorization uses stream events instead (enqueue_factor).  Counted at create / destroy.
static const int MAX_DEVICES = 64;
static std::atomic<int> g_live[MAX_DEVICES];
static std::atomic<bool> g_attr_set[MAX_DEVICES];      // per-device function attributes (dynamic LDS of adat_sparse)

struct ipm_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream2 = nullptr;            // bulk stream of the Cholesky look-ahead
    hipStream_t stream3 = nullptr;            // residual stream: r_b, r_c, stop test and the predictor rhs under the factorization
    hipEvent_t ev_mid = nullptr, ev_res = nullptr, ev_grp = nullptr, ev_last = nullptr;
    std::vector<hipEvent_t> ev_crit, ev_bulk;
    hipEvent_t ev_fork = nullptr;
    int lookahead = 1;
    int grouped_trsv = 1;                 // group inverses + GEMV solves (trsv_grouped.h); IPM_GROUPED_TRSV=0 disables
    int gsz = 0;                          // 128-blocks per group: 8 from 16 blocks on (ragged: leftover blocks are solved step by step), else the largest of 8/4/2 dividing nblk
    double *gXT = nullptr, *gX = nullptr, *gS = nullptr, *gPart = nullptr;   // own allocation
    unsigned* d_bulk_done = nullptr;      // [nblk] workgroup-completion counters of the bulk trailing updates
    bool no_dense = false;                // B / invD / slab are not in the workspace (layout_no_dense); B_own, invD_own once ensure_dense_B ran
    double* B_own = nullptr; double* invD_own = nullptr;
    int group_steps = 0;                  // > 0: forced group size of the two-level schedule
    int two_level = 1;                    // group the Cholesky steps: K = 128*gs trailing updates (IPM_TWO_LEVEL=0 disables)
    int bulk_variant = 0;                 // 0: chol_update_kernel (adat_syrk schedule, round 3); 7: the generic kernel of rounds 1-2 (bit-identical, tested)
    int ss_small_blocks = 16;             // single-stream handles: trailing blocks up to which the narrow-tile panel / update kernels are used (73-LP suite, 8 in flight:
                                          // 12.4 / 13.5 / 14.1 / 14.5 / 14.4 LPs/s for 0 / 4 / 8 / 16 / 64 blocks)
    int flag_sync = 1;                    // main stream polls d_bulk_done instead of waiting on a stream event
    int last_gs = 1, n_counter_steps = 0, n_event_steps = 0, timeouts_recovered = 0;   // ipm_get_schedule
    bool counted = false;                 // this handle is in g_live
    // fused single-workgroup path for small sparse LPs (small_lp.h): product list of B's lower entries, own allocation
    bool small = false;
    int fused_small = 1;                  // IPM_FUSED_SMALL=0: always the multi-kernel path
    bool list_form = false;               // sparse handle, 128 < m, <= 1536 padded rows: B from the product list (adat_list_kernel)
    int list_form_opt = 1;                // IPM_LIST_FORM=0: one workgroup per row of B (adat_sparse_kernel)
    int *ls_bi = nullptr, *ls_bk = nullptr;
    double* ls_bak = nullptr;             // list path: sm_bcoef holds a_ij, ls_bak a_kj (the products are formed on the device)
    int sm_nb = 0;
    int *sm_bptr = nullptr, *sm_bcol = nullptr;
    unsigned short *sm_bi = nullptr, *sm_bk = nullptr;
    double* sm_bcoef = nullptr;
    // multifrontal sparse Cholesky (sparse_chol.h), IPM_FLAG_SPARSE_FACTOR: structures built by ipm_set_A_csc, own allocations
    bool spf = false;                     // the sparse factor serves this handle
    bool spf_off = false;                 // set around calls that factor a caller's dense matrix (ipm_solve_linear)
    bool sp_serial = false;               // after a hand-off time-out: one workgroup per launch (never waits)
    SpFactor spF;                         // device view
    std::vector<void*> sp_allocs;
    int *sp_fptr = nullptr, *sp_fcol = nullptr;
    double* sp_fcoef = nullptr;
    long long* sp_diagpos = nullptr;
    long long sp_nslot = 0, sp_nu = 0, sp_terms = 0;
    int sp_height = 0, sp_rmax = 0, sp_grid = 1, sp_serial_launches = 0, sp_nvirtual = 0;
    size_t sp_lds_chol = 0, sp_lds_solve = 0;
    int sp_fv_off = 0;                    // doubles of sp_chol_kernel's dynamic LDS in front of the forward substitution's r-vector
    int sp_fuse_fwd = 1;                  // the predictor's forward substitution rides on the factorization (IPM_SP_FUSE_FWD=0: own sweep)
    const double* sp_fwd_fused = nullptr; // right-hand side whose forward substitution the last factorization carried (z in t2)
    int sp_lds_doubles = 16, sp_threads = 256;
    int sp_level_mode = 0;                // 1 (IPM_SP_MODE=level): one launch per level of the panel tree, no in-kernel hand-offs; -1 (=task): one
                                          // launch per sweep even when the device is shared; 0: sp_level() decides
    std::vector<int> sp_lvlptr;           // [levels + 1] into the level-ordered records
    SpRec* sp_rec_level = nullptr;
    unsigned sp_epoch = 0;
    double shift_rel = 0.0;               // Tikhonov shift in effect (opt.regularize, or 1e-14 switched on by ipm_solve)
    int auto_reg = 0;                     // 1: the shift was switched on automatically
    unsigned* d_flags = nullptr;          // [2*nblk] hand-off flags + 1 timeout word (own allocation)
    int64_t m = 0, n = 0, mp = 0, np = 0;
    int nblk = 0, rc_chunks = 0, rows_per_chunk = 0, vblk = 0;
    ipm_options opt;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    bool own_ws = false;
    // device arrays (all inside the workspace)
    double *A = nullptr, *B = nullptr, *invD = nullptr;
    double *x = nullptr, *s = nullptr, *c = nullptr, *rc = nullptr, *d = nullptr, *v = nullptr, *q = nullptr;
    double *dxa = nullptr, *dsa = nullptr, *dx = nullptr, *ds = nullptr;
    double *y = nullptr, *b = nullptr, *rb = nullptr, *t1 = nullptr, *t2 = nullptr, *dya = nullptr, *dy = nullptr;
    double *atp = nullptr, *part = nullptr, *slab = nullptr;
    // fused formation + factorization (form_factor.h): dense handles of FF_MIN_NBLK .. FF_MAX_NBLK blocks that have the device to
    // themselves run ONE persistent worker launch beside the pivot chain instead of formation followed by factorization
    int ff_enabled = 1;                   // IPM_FUSED_FACTOR=0 disables, =force also below FF_MIN_NBLK blocks (tests)
    // Where the fused launch is the default.  Measured on MI355X, it/s fused / serial (tools/ff_sizes.sh, profiles/r04_ff_sizes_fused_vs_serial.txt;
    // n = 2m unless noted): 1536: 903 / 941 -- 2048: 684 / 640 -- 2560: 514 / 439 -- 3072: 422 / 302 -- 3584: 335 / 242 -- 4096: 259 / 208 --
    // 5120: 150 / 113 -- 6144: 93.3 / 79.6 -- 8192: 41.8 / 40.0 -- 10240: 22.3 / 22.4 -- 4096 x 4608: 358 / 267 -- 4096 x 16384: 152 / 137 --
    // 4096 x 32768: 85.5 / 87.1 (the formation dominates there and the serial kernel forms faster).  So: 16 .. 72 blocks while n <= 6 m.
    // IPM_FF_MAX_NBLK / IPM_FUSED_FACTOR=force|0 override.
    int ff_min_nblk = 16, ff_max_nblk = 72;
    bool ff_forced = false;
    bool ff_ref_engine = false;           // IPM_FF_REF_ENGINE=1: form_factor_roles_kernel (the engines' previous stage schedule), the reference of tests/test_gpu_ff_engines.py
    int ff_q = 4;                         // formation chunks per tile (IPM_FF_Q)
    int ff_workers = 0;                   // WORKER workgroups of the persistent launch (set by ff_build from the CU count, no switch)
    int* d_ff_tile_items = nullptr;       // [tile_items | tile_q]
    int ff_qmax = 16;                     // slab capacity per tile (the first block rows are formed in more, shorter chunks)
    bool ff_built = false, ff_last = false;
    FFSchedule ff_sched;
    FFItem* d_ff_items = nullptr;         // the work list in ticket order
    unsigned* d_ff_flags = nullptr;       // ticket[16] | reserved[8] | dbg[8] | fcount[ntile] | tprog[ntile] | lfinal[nblk] | dready[nblk] | potrfdone[nblk]
    size_t ff_flag_words = 0;
    double* ff_slab = nullptr;            // [ntile][Q][128*128]
    long long* ff_trace = nullptr;        // IPM_FF_TRACE_ITEMS=1: [nitems][4] per-item time line + [nblk][12] chain kernels (ipm_debug_ff_trace)
    long long* ff_prof = nullptr;         // IPM_FF_PROF=1: [workers][16] cycle profile of the persistent launch (accumulates)
    const int* fdone = nullptr;           // `done` word the formation / factorization kernels test (null: Scalars::done; the overlapped
                                          // path points it at the per-iteration latch Scalars::done_f)
    // Tile envelope (skyline) of A A^T for sparse handles, from the structure of A in the caller's row order:
    // env_last[k] = last 128-row block with a structural nonzero at or left of column block k (monotone).  Blocks
    // below it are exactly zero in B and stay zero in L, so the panel solves, trailing updates and triangular
    // solves skip them.  The Python host reorders the rows (reverse Cuthill-McKee) to make the envelope small.
    std::vector<int> env_last, env_first;     // env_first[i] = first column block with env_last >= i
    bool use_env = false;
    int envelope = 1;                         // IPM_ENVELOPE=0 disables
    bool sparse = false;                 // A kept as CSR + CSC on the device
    int64_t nnz_cap = 0, nnz = 0;
    int* d_tile_order = nullptr;         // 2-D patch order of the lower 128x128 tiles of B (L2 reuse)
    int *d_rowptr = nullptr, *d_colind = nullptr, *d_colptr = nullptr, *d_rowind = nullptr;
    double *d_rval = nullptr, *d_cval = nullptr;
    long long* stamp_buf = nullptr;       // diagnostic only (IPM_POTRF_STAMPS=1)
    unsigned* ff_potrfdone = nullptr;     // fused launch: the chain's hand-off words of the launch enqueued last (one per block)
    Scalars* sc = nullptr;
    IterRec* hist = nullptr;              // [HIST_CAP] per-iteration records (ring)
    double* snap = nullptr;               // roll-back copy of (x, y, s) + Scalars (poll time-out / auto-regularize restart)
    // native upper bounds (ipm_set_bounds): own allocation of BND_VECS n-vectors, made on first use
    bool bnd = false;                     // a finite bound is set: the bounded kernel instantiations run
    int bnd_nU = 0;                       // |U|
    double* bnd_mem = nullptr;            // u | w | z | dwa | dza | dw | dz | qz | roll-back w | roll-back z
    // infeasibility detection (IPM_FLAG_DETECT_INFEASIBILITY): the Detect kernel instantiations run
    bool detect = false;
    double det_eps_p = 1e-8, det_eps_d = 1e-8;   // ipm_set_infeasibility_tol
    double* det = nullptr;                // [4] record of the last detection (workspace): kind, normalisation, violation, k
    double* cert_mem = nullptr;           // x | y | z of ipm_get_certificate (own allocation, made on first use)
    int* fixed = nullptr;
    Scalars* h_sc = nullptr;          // pinned host mirror
    bool haveA = false, haveBC = false, haveState = false, predictor_valid = false;
    bool fresh_state = true;              // the iterate was (re)set: the next ipm_iterate counts its steps from k = 0
    int profiling = 0;                    // 0 off, 1 events around the A D^2 A^T kernel only, 2 every phase
    double phase_ms[4] = {0, 0, 0, 0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // lockstep batch (lockstep.h, ipm_solve_batch): while non-null, every launch site of the single-stream iteration path RECORDS
    // (kernel type, grid, arguments) here instead of launching
    std::vector<struct LsLaunch>* ls_rec = nullptr;
    bool ls_cut = false;                  // a launch without a lockstep twin was met while recording
    int lockstep = 0;                     // IPM_FLAG_LOCKSTEP: created for ipm_solve_batch (block-step substitutions: every launch of the iteration is recordable)
    char err[512] = "";
};
struct LsLaunch { int type; LsRec rec; };
template <class A> static bool ls_push(ipm_handle* h, int type, unsigned gridx, const A& a, unsigned lds = 0) {
    if (!h->ls_rec) return false;
    static_assert(sizeof(A) <= LS_ARG_BYTES, "LsRec::args too small");
    LsLaunch L;
    memset(&L, 0, sizeof L);
    L.type = type; L.rec.gridx = gridx; L.rec.lds = lds;
    memcpy(L.rec.args, &a, sizeof(A));
    h->ls_rec->push_back(L);
    return true;
}

static int fail(ipm_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof g_err, "%s", buf);
    if (h) snprintf(h->err, sizeof h->err, "%s", buf);
    return code;
}

#define HIP_TRY(h, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((h), IPM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                  \
    } while (0)

static inline int64_t round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }

// Device memory the handle owns besides its workspace.  STREAM-ORDERED (hipMallocAsync / hipFreeAsync on the handle's
// stream, pool kept for reuse): a plain hipFree synchronises the whole device, and with several LPs in flight every one
// of a handle's ~30 frees waited for the other LPs' queued iterations -- measured in the 73-LP suite: STOCFOR3 0.46 s of
// solve and 1.14 s of teardown, SIERRA 0.12 s and 1.19 s.
static std::atomic<int> g_pool_state[64];       // per device: 0 unknown, 1 stream-ordered allocation available, 2 not
static hipMemPool_t g_pool[64];                 // the library's OWN pool per device (never the device's default pool: its
                                                // attributes belong to the host application)
static std::mutex g_pool_mutex;
static bool async_alloc_ok(int device) {
    if (device < 0 || device >= 64) return false;
    int st = g_pool_state[device].load(std::memory_order_acquire);
    if (st == 0) {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        st = g_pool_state[device].load(std::memory_order_acquire);
        if (st != 0) return st == 1;
        int supported = 0;
        if (hipDeviceGetAttribute(&supported, hipDeviceAttributeMemoryPoolsSupported, device) == hipSuccess && supported) {
            hipMemPoolProps props;
            memset(&props, 0, sizeof props);
            props.allocType = hipMemAllocationTypePinned;
            props.handleTypes = hipMemHandleTypeNone;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = device;
            hipMemPool_t pool = nullptr;
            if (hipMemPoolCreate(&pool, &props) == hipSuccess && pool) {
                // freed blocks stay in the pool up to this many bytes, so the next handle reuses them (the sparse factor of
                // one LP is ~20 blocks); beyond it they go back to the device at the next synchronisation point instead of
                // staying resident for the life of the process
                uint64_t keep = (uint64_t)2 << 30;
                (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
                g_pool[device] = pool;
                st = 1;
            }
        }
        if (st == 0) st = 2;
        g_pool_state[device].store(st, std::memory_order_release);
    }
    return st == 1;
}
static hipError_t dev_malloc(int device, hipStream_t stream, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (async_alloc_ok(device)) return hipMallocFromPoolAsync(p, bytes, g_pool[device], stream);
    return hipMalloc(p, bytes);
}
static void dev_free(int device, hipStream_t stream, void* p) {
    if (!p) return;
    if (async_alloc_ok(device)) (void)hipFreeAsync(p, stream); else (void)hipFree(p);
}
// pinned host mirrors of the scalar record are recycled, never freed (hipHostFree synchronises too)
static std::mutex g_hsc_mutex;
static std::vector<Scalars*> g_hsc_pool;

static GemmNT gemm_defaults() {
    GemmNT g;
    memset(&g, 0, sizeof g);
    g.alpha = 1.0; g.unit_diag_from = -1; g.batch = 1; g.batch2 = 1;
    return g;
}

// ------------------------------------------------------------------------------- layout
struct Layout {
    int64_t mp, np;
    int nblk, rc_chunks, rows_per_chunk, vblk;
    size_t off_A, off_B, off_inv, off_nvec, off_mvec, off_atp, off_part, off_det, off_sc, off_fixed, off_hist, off_snap, off_slab, total;
    size_t off_rowptr, off_colind, off_rval, off_colptr, off_rowind, off_cval, off_order;
};
static const int N_NVEC = 11;   // x s c rc d v q dxa dsa dx ds
static const int N_MVEC = 7;    // y b rb t1 t2 dya dy

// no_dense: the handle factors with the sparse multifrontal Cholesky (IPM_FLAG_SPARSE_FACTOR on a sparse handle beyond the fused
// small-LP size) -- B, inv(L_kk) and the split-K slab are not part of the workspace; ensure_dense_B allocates them if a
// dense entry point (ipm_form_normal_matrix, ipm_get_factor, ipm_solve_linear) is ever called on such a handle.
static bool layout_no_dense(int64_t m, int64_t sparse_nnz, unsigned flags) { return sparse_nnz > 0 && (flags & IPM_FLAG_SPARSE_FACTOR) && m > 128; }
static Layout make_layout(int64_t m, int64_t n, int64_t sparse_nnz = 0, bool no_dense = false) {
    Layout L;
    L.mp = round_up(m, NB);
    {   // the grouped triangular solves (trsv_grouped.h) need whole 1024-row groups: pad a little further when that
        // costs at most 1/8 more blocks (identity rows are cheap; 4 x nblk dependent launches per iteration are not)
        const int64_t nb = L.mp / NB, nb8 = round_up(nb, 8);
        if (nb >= 16 && (nb8 - nb) * 8 <= nb) L.mp = nb8 * NB;
    }
    L.np = round_up(n, 64);
    L.nblk = (int)(L.mp / NB);
    int64_t c64 = L.mp / 64;
    L.rc_chunks = (int)(c64 <= 32 ? c64 : 32);          // <= 32 row chunks of A^T u partials (mp/64 must divide evenly)
    while (L.mp % L.rc_chunks) --L.rc_chunks;
    L.rows_per_chunk = (int)(L.mp / L.rc_chunks);
    while ((int64_t)L.rc_chunks * L.rows_per_chunk < L.mp) ++L.rows_per_chunk;   // (exact by construction)
    int64_t mx = m > n ? m : n;
    int64_t vb = (mx + VBLK - 1) / VBLK;          // one element per thread until MAXPART blocks
    L.vblk = (int)(vb < 1 ? 1 : (vb > MAXPART ? MAXPART : vb));
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    if (sparse_nnz > 0) { L.rc_chunks = 1; L.rows_per_chunk = (int)L.mp; }
    L.off_A = take(sparse_nnz > 0 ? 0 : sizeof(double) * L.mp * L.np);
    L.off_B = take(no_dense ? 0 : sizeof(double) * L.mp * L.mp);
    L.off_inv = take(no_dense ? 0 : sizeof(double) * L.nblk * NB * NB);
    L.off_nvec = take(sizeof(double) * L.np * N_NVEC);
    L.off_mvec = take(sizeof(double) * L.mp * N_MVEC);
    L.off_atp = take(sizeof(double) * L.rc_chunks * L.np);
    L.off_part = take(sizeof(double) * P_NSLOT_DETECT * MAXPART);     // (the slots of the infeasibility tests included)
    L.off_det = take(sizeof(double) * 4);
    L.off_sc = take(sizeof(Scalars));
    L.off_fixed = take(256);
    L.off_hist = take(sizeof(IterRec) * HIST_CAP);
    L.off_snap = take(sizeof(double) * (2 * L.np + L.mp) + sizeof(Scalars));
    L.off_slab = take(no_dense ? 0 : sizeof(double) * (size_t)kSlabTiles * 128 * 128);   // split-K partial tiles (64 MB)
    L.off_order = take(sizeof(int) * ((size_t)L.nblk * (L.nblk + 1) / 2));
    L.off_rowptr = take(sparse_nnz > 0 ? sizeof(int) * (m + 1) : 0);
    L.off_colptr = take(sparse_nnz > 0 ? sizeof(int) * (n + 1) : 0);
    L.off_colind = take(sparse_nnz > 0 ? sizeof(int) * sparse_nnz : 0);
    L.off_rowind = take(sparse_nnz > 0 ? sizeof(int) * sparse_nnz : 0);
    L.off_rval = take(sparse_nnz > 0 ? sizeof(double) * sparse_nnz : 0);
    L.off_cval = take(sparse_nnz > 0 ? sizeof(double) * sparse_nnz : 0);
    L.total = off;
    return L;
}

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
__global__ void set_params_kernel(Scalars* sc, double e1, double e2, double e3, double eta, int max_iter,
                                  int force, int reset) {
    sc->e1 = e1; sc->e2 = e2; sc->e3 = e3; sc->eta = eta;
    sc->max_iter = max_iter; sc->force = force;
    sc->done = 0; sc->done_f = 0; sc->status = 0;
    if (reset) { sc->k = 0; sc->fixed = 0; sc->fixed_first = 0; sc->obj_last_finite = __builtin_nan(""); }
}

static void free_sparse_factor(ipm_handle* h);
static void ff_release(ipm_handle* h);
extern "C" int ipm_create(int device, int64_t m, int64_t n, const ipm_options* opts, void* workspace,
                          size_t workspace_bytes, void* stream, ipm_handle** out) {
    if (!out) return fail(nullptr, IPM_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (m <= 0 || n <= 0 || m > (1 << 20) || n > (1 << 24)) return fail(nullptr, IPM_ERR_INVALID_ARG, "bad problem size %lld x %lld", (long long)m, (long long)n);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, IPM_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(nullptr, IPM_ERR_INVALID_ARG, "device %d out of range (%d visible)", device, ndev);
    ipm_handle* h = new ipm_handle();
    h->device = device;
    if (opts) h->opt = *opts; else ipm_default_options(&h->opt);
    if (h->opt.check_every < 1) h->opt.check_every = 1;
    if (!(h->opt.eta > 0.0)) h->opt.eta = 0.91;
    if (!(h->opt.pivot_guard_big > 0.0)) h->opt.pivot_guard_big = 1e64;
    if (!(h->opt.regularize >= 0.0)) h->opt.regularize = 0.0;
    h->shift_rel = h->opt.regularize;
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
    {   // test knob (see gemm_nt_f64.h): spin bound of the device-side hand-offs; set in every case, so that a later handle restores the default
        unsigned lim = 1u << 22;
        if (const char* e = getenv("IPM_TEST_SPIN_LIMIT")) lim = (unsigned)std::max(1, atoi(e));
        CREATE_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(ipm_spin_limit), &lim, sizeof lim, 0, hipMemcpyHostToDevice, h->stream));
        CREATE_TRY(hipStreamSynchronize(h->stream));
    }
    if (const char* e = getenv("IPM_ENVELOPE")) h->envelope = atoi(e);
    // zero everything except A and B (padding entries of every vector must stay 0)
    CREATE_TRY(hipMemsetAsync(base + L.off_inv, 0, L.off_slab - L.off_inv, h->stream));
    {
        std::lock_guard<std::mutex> lock(g_hsc_mutex);
        if (!g_hsc_pool.empty()) { h->h_sc = g_hsc_pool.back(); g_hsc_pool.pop_back(); }
    }
    if (!h->h_sc) CREATE_TRY(hipHostMalloc((void**)&h->h_sc, sizeof(Scalars), hipHostMallocDefault));
    memset(h->h_sc, 0, sizeof(Scalars));
    CREATE_TRY(hipEventCreate(&h->ev0));
    CREATE_TRY(hipEventCreate(&h->ev1));
    if (const char* e = getenv("IPM_LOOKAHEAD")) h->lookahead = atoi(e);
    h->detect = (h->opt.flags & IPM_FLAG_DETECT_INFEASIBILITY) != 0;
    if (h->opt.flags & IPM_FLAG_LOCKSTEP) { h->lockstep = 1; h->opt.flags |= IPM_FLAG_SINGLE_STREAM | IPM_FLAG_NO_DEVICE_POLLING; }
    if (h->opt.flags & IPM_FLAG_SINGLE_STREAM) h->lookahead = 0;
    if (const char* e = getenv("IPM_GROUPED_TRSV")) h->grouped_trsv = atoi(e);
    if (h->lockstep && getenv("IPM_LS_BLOCK_STEPS")) h->grouped_trsv = 0;      // (A/B: block-step substitutions in the lockstep batch)
    if (h->lockstep) h->ss_small_blocks = 1 << 20;      // ONE panel / update kernel shape at every step: step k of all LPs of a batch then shares its launches
    if (h->no_dense) h->grouped_trsv = 0;      // the sparse factor has its own sweeps; a dense entry point on such a handle solves block by block
    h->gsz = 0;
    if (h->grouped_trsv) {
        // RAGGED groups (round 3): the block count need not be a multiple of the group size -- floor(nblk / gsz) full groups get
        // their explicit inverses, the blocks left over at the end are substituted block by block (enqueue_potrs_grouped).  From
        // 16 blocks on always groups of 8 (19 blocks: 2 groups + 3 steps, 28 launches per iteration's four sweeps + 10 for the
        // inverses instead of 76); 9 .. 15 blocks: the largest of 8 / 4 that divides, else 8 + leftover; below 9 as before.
        const bool ragged = !(getenv("IPM_RAGGED_GROUPS") && atoi(getenv("IPM_RAGGED_GROUPS")) == 0);
        if (h->nblk >= 2 * GS_MAX) { if (ragged || h->nblk % GS_MAX == 0) h->gsz = GS_MAX; }
        else {
            for (int p2 = GS_MAX; p2 >= 2; p2 /= 2) if (h->nblk % p2 == 0) { h->gsz = p2; break; }
            if (ragged && h->nblk > GS_MAX && h->gsz < 4) h->gsz = GS_MAX;
        }
    }
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
    if (const char* e = getenv("IPM_FLAG_SYNC")) h->flag_sync = atoi(e);
    if (h->opt.flags & IPM_FLAG_NO_DEVICE_POLLING) h->flag_sync = 0;
    if (const char* e = getenv("IPM_BULK_VARIANT")) h->bulk_variant = atoi(e);
    if (const char* e = getenv("IPM_TWO_LEVEL")) h->two_level = atoi(e);
    if (const char* e = getenv("IPM_GROUP_STEPS")) h->group_steps = atoi(e);
    if (const char* e = getenv("IPM_FUSED_SMALL")) h->fused_small = atoi(e);
    if (const char* e = getenv("IPM_LIST_FORM")) h->list_form_opt = atoi(e);
    if (getenv("IPM_POTRF_STAMPS")) { CREATE_TRY(dev_malloc(device, h->stream, (void**)&h->stamp_buf, 8 * 64 * sizeof(long long))); CREATE_TRY(hipMemsetAsync(h->stamp_buf, 0, 8 * 64 * sizeof(long long), h->stream)); }
    if (h->lookahead != 0 && h->nblk > 2)                  // (a single-stream handle creates no second stream: see stream3 below)
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
    if (const char* e = getenv("IPM_FUSED_FACTOR")) { if (!strcmp(e, "force")) { h->ff_enabled = 1; h->ff_min_nblk = 3; h->ff_forced = true; } else h->ff_enabled = atoi(e); }
    if (const char* e = getenv("IPM_FF_MAX_NBLK")) h->ff_max_nblk = atoi(e);
    if (const char* e = getenv("IPM_FF_CHAIN_MODE")) {
        // 0 asked for the chain as three launches per step beside 224 workers: that structure met a recovered hand-off time-out and
        // has been removed.  Whoever asks for it by name is told so, not given another structure silently.
        if (atoi(e) == 0) {
            int rc_ = fail(nullptr, IPM_ERR_INVALID_ARG, "IPM_FF_CHAIN_MODE=0 is not supported (that structure of the fused launch was removed)");
            ipm_destroy(h);
            return rc_;
        }
    }
    if (const char* e = getenv("IPM_FF_REF_ENGINE")) h->ff_ref_engine = atoi(e) != 0;
    if (const char* e = getenv("IPM_FF_Q")) h->ff_q = std::max(1, std::min(16, atoi(e)));
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
    if (h->ff_prof) {          // diagnostic: where the workers' cycles went (sum over the handle's fused launches)
        (void)hipDeviceSynchronize();
        std::vector<long long> P(16 * ((size_t)h->ff_workers + 1));
        (void)hipMemcpy(P.data(), h->ff_prof, sizeof(long long) * P.size(), hipMemcpyDeviceToHost);
        double tot[16] = {0};
        for (int w = 0; w <= h->ff_workers; ++w) for (int k = 0; k < 16; ++k) tot[k] += (double)P[(size_t)w * 16 + k];
        static const char* nm[] = {"ticket", "F gemm", "F store+publish", "T wait", "T gemm", "T base+combine", "panel wait", "panel gemm", "T store+publish"};
        double sum = 0; for (int k = 0; k < 9; ++k) sum += tot[k];
        fprintf(stderr, "[ff prof] %d workers, F items %.0f, T items %.0f, cycles per worker in the launches %.3g (sum of phases %.3g)\n", h->ff_workers, tot[FFP_NF], tot[FFP_NT], tot[FFP_TOTAL] / h->ff_workers, sum / h->ff_workers);
        for (int k = 0; k < 9; ++k) fprintf(stderr, "   %-18s %6.2f %%\n", nm[k], 100.0 * tot[k] / sum);
    }
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
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->h_sc) { std::lock_guard<std::mutex> lock(g_hsc_mutex); g_hsc_pool.push_back(h->h_sc); h->h_sc = nullptr; }
    for (void* p : {(void*)h->stamp_buf, (void*)h->d_flags, (void*)h->d_bulk_done, (void*)h->B_own, (void*)h->invD_own, (void*)h->bnd_mem, (void*)h->cert_mem, (void*)h->gXT, (void*)h->gX, (void*)h->gS, (void*)h->gPart})
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
    HIP_TRY(h, hipMemsetAsync(h->A, 0, sizeof(double) * h->mp * h->np, h->stream));
    HIP_TRY(h, hipMemcpy2DAsync(h->A, sizeof(double) * h->np, A, sizeof(double) * ld, sizeof(double) * h->n, h->m,
                                is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->haveA = true; h->predictor_valid = false;
    return IPM_OK;
}

// ------------------------------------------------------------------------------- sparse factor (IPM_FLAG_SPARSE_FACTOR)
static void free_sparse_factor(ipm_handle* h) {
    for (void* p : h->sp_allocs) dev_free(h->device, h->stream, p);
    h->sp_allocs.clear();
    h->spf = false;
}

template <class T>
static int sp_upload(ipm_handle* h, const std::vector<T>& v, T** out, size_t min_count = 1) {
    const size_t cnt = std::max(v.size(), min_count);
    void* d = nullptr;
    HIP_TRY(h, dev_malloc(h->device, h->stream, &d, sizeof(T) * cnt));
    h->sp_allocs.push_back(d);
    if (!v.empty()) HIP_TRY(h, hipMemcpyAsync(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, h->stream));
    *out = (T*)d;
    return IPM_OK;
}
template <class T>
static int sp_alloc_zero(ipm_handle* h, size_t count, T** out) {
    void* d = nullptr;
    if (count < 1) count = 1;
    HIP_TRY(h, dev_malloc(h->device, h->stream, &d, sizeof(T) * count));
    h->sp_allocs.push_back(d);
    HIP_TRY(h, hipMemsetAsync(d, 0, sizeof(T) * count, h->stream));
    *out = (T*)d;
    return IPM_OK;
}

// ipm_order_rows analyses the LP in the order it returns; the caller then permutes the rows and calls ipm_set_A_csc, which needs
// the same analysis: a few entries are kept (matched by the exact canonical CSC pattern of the permuted matrix, taken once).
struct SymCacheEntry { int m = 0, n = 0; double relax = 1.0; std::vector<int> cp, ri; sym::Supernodes S; };
static std::mutex g_sym_mutex;
static std::deque<SymCacheEntry> g_sym_cache;
static bool sym_cache_take(int m, int n, const std::vector<int>& cp, const std::vector<int>& ri, double relax, sym::Supernodes& S) {
    std::lock_guard<std::mutex> lock(g_sym_mutex);
    for (auto it = g_sym_cache.begin(); it != g_sym_cache.end(); ++it)
        if (it->m == m && it->n == n && it->relax == relax && it->cp.size() == cp.size() && it->ri.size() == ri.size() &&
            std::equal(cp.begin(), cp.end(), it->cp.begin()) && std::equal(ri.begin(), ri.end(), it->ri.begin())) {
            S = std::move(it->S);
            g_sym_cache.erase(it);
            return true;
        }
    return false;
}

// Symbolic analysis of A A^T in the given row order, task partition, product lists of the formation; everything the three
// kernels of sparse_chol.h index with goes to the device once.  cp/ri/cv: canonical CSC of A; rp/ci/rv: its CSR.
static int build_sparse_factor(ipm_handle* h, const std::vector<int>& cp, const std::vector<int>& ri, const std::vector<double>& cv,
                               const std::vector<int>& rp, const std::vector<int>& ci, const std::vector<double>& rv) {
    free_sparse_factor(h);
    const int m = (int)h->m, n = (int)h->n;
    sym::Supernodes S;
    double relax = 1.0;
    if (!sym_cache_take(m, n, cp, ri, relax, S)) {          // not ordered through ipm_order_rows just before: analyse here
        sym::Pattern P;
        if (!sym::normal_pattern(m, n, cp.data(), ri.data(), (int64_t)1.5e8, P))
            return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: the pattern of A A^T exceeds 1.5e8 entries (use the dense path)");
        const int arc = sym::analyse(P, SPC_WCAP, SPC_PANEL, S, (int64_t)2.5e8, relax);
        if (arc) return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: the factor structures exceed 2.5e8 entries (use the dense path)");
    }
    if (S.rmax > SPC_PANEL || S.panel_max > SPC_PANEL) return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: a front of %d rows exceeds the panel budget", S.rmax);
    const int nsn = S.nsn;
    // ---- tasks: whole subtrees below a work threshold, chains of the remaining (top) panels
    std::vector<double> sub((size_t)nsn, 0.0);
    double total = 0.0;
    for (int J = 0; J < nsn; ++J) {
        const double r = (double)(S.rowptr[(size_t)J + 1] - S.rowptr[J]);
        const double cst = 1.0 + r * r / 1024.0 + 0.5 * (S.childptr[(size_t)J + 1] - S.childptr[J]);
        sub[J] += cst;
        total += cst;
        if (S.parent[J] >= 0) sub[S.parent[J]] += sub[J];
    }
    // (every task costs one draw from ONE atomic counter, every workgroup one more: a few hundred of each keep that queue
    //  off the critical path -- measured: 2048 workgroups drawing 3000 tasks spend 0.2 ms per sweep on the counter alone)
    // one-wave workgroups (four times the panels in flight) are an option, not the default: measured 35 % SLOWER at STOCFOR3
    // (fronts of <= 56 rows): a panel is instruction-latency bound and 256 threads share its loops
    const int threads = SPC_THREADS;      // (one-wave workgroups, four times the panels in flight, were measured 35 % slower at STOCFOR3)
    double div = 1536.0;
    const double T = std::max(8.0, total / div);
    std::vector<int> taskof((size_t)nsn, -1), topkids((size_t)nsn, 0);
    for (int J = 0; J < nsn; ++J) if (sub[J] > T && S.parent[J] >= 0) topkids[S.parent[J]]++;
    int ntask = 0;
    for (int J = nsn - 1; J >= 0; --J) {
        const int pj = S.parent[J];
        const bool low = !(sub[J] > T);
        if (low) taskof[J] = (pj >= 0 && !(sub[pj] > T)) ? taskof[pj] : ntask++;
        else taskof[J] = (pj >= 0 && topkids[pj] == 1) ? taskof[pj] : ntask++;       // (the parent of a top panel is a top panel)
    }
    // tasks in ascending order of their top panel: ids were handed out top-down, so reverse them
    for (int J = 0; J < nsn; ++J) taskof[J] = ntask - 1 - taskof[J];
    std::vector<int> taskptr((size_t)ntask + 1, 0), tasknode((size_t)nsn);
    for (int J = 0; J < nsn; ++J) taskptr[(size_t)taskof[J] + 1]++;
    for (int t = 0; t < ntask; ++t) taskptr[(size_t)t + 1] += taskptr[t];
    { std::vector<int> nx(taskptr.begin(), taskptr.end() - 1); for (int J = 0; J < nsn; ++J) tasknode[(size_t)nx[taskof[J]]++] = J; }
    for (int t = 0; t + 1 < ntask; ++t)              // the order the deadlock argument rests on
        if (tasknode[(size_t)taskptr[t + 1] - 1] >= tasknode[(size_t)taskptr[t + 2] - 1])
            return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: internal error (task order)");
    std::vector<SpNode> nodes((size_t)nsn);
    for (int J = 0; J < nsn; ++J) {
        SpNode& nd = nodes[J];
        memset(&nd, 0, sizeof nd);
        nd.c0 = S.c0[J]; nd.w = S.w[J];
        nd.r = (int)(S.rowptr[(size_t)J + 1] - S.rowptr[J]);
        nd.nchild = S.childptr[(size_t)J + 1] - S.childptr[J]; nd.child0 = S.childptr[J];
        nd.parent = S.parent[J];
        nd.publish = (nd.parent >= 0 && taskof[nd.parent] != taskof[J]) ? 1 : 0;
        for (int t = S.childptr[J]; t < S.childptr[(size_t)J + 1]; ++t) if (taskof[S.child[(size_t)t]] != taskof[J]) nd.wait_children = 1;
        nd.rowptr = S.rowptr[J]; nd.lptr = S.lptr[J]; nd.uptr = S.uptr[J];
    }
    if (S.max_children > SPC_MAXCH) return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: internal error (fan-in)");
    std::vector<SpRec> recs((size_t)nsn);
    for (int tn = 0; tn < nsn; ++tn) {
        const int J = tasknode[(size_t)tn];
        const SpNode& nd = nodes[J];
        SpRec& rc = recs[(size_t)tn];
        memset(&rc, 0, sizeof rc);
        rc.J = J; rc.c0 = nd.c0; rc.w = nd.w; rc.r = nd.r; rc.nchild = nd.nchild; rc.parent = nd.parent;
        rc.wait_children = nd.wait_children; rc.publish = nd.publish;
        rc.rowptr = nd.rowptr; rc.lptr = nd.lptr; rc.uptr = nd.uptr;
        for (int t = 0; t < nd.nchild; ++t) {
            const int K = S.child[(size_t)(nd.child0 + t)];
            SpChild& c = rc.ch[t];
            c.uptr = nodes[K].uptr; c.relptr = nodes[K].rowptr + nodes[K].w; c.pc = nodes[K].r - nodes[K].w; c.K = K;
            c.ext = taskof[K] != taskof[J] ? 1 : 0;
        }
    }
    // level-ordered copy of the records (level = 1 + the highest level among the children): LEVEL mode launches one kernel per level
    std::vector<int> lvl((size_t)nsn, 1), lvlptr;
    int nlev = 0;
    for (int J = 0; J < nsn; ++J) { if (S.parent[J] >= 0) lvl[S.parent[J]] = std::max(lvl[S.parent[J]], lvl[J] + 1); nlev = std::max(nlev, lvl[J]); }
    std::vector<SpRec> recs_level((size_t)nsn);
    {
        std::vector<int> pos_of((size_t)nsn);
        for (int tn = 0; tn < nsn; ++tn) pos_of[(size_t)tasknode[(size_t)tn]] = tn;
        lvlptr.assign((size_t)nlev + 1, 0);
        for (int J = 0; J < nsn; ++J) lvlptr[(size_t)lvl[J]]++;
        for (int l = 0; l < nlev; ++l) lvlptr[(size_t)l + 1] += lvlptr[(size_t)l];
        std::vector<int> nx(lvlptr.begin(), lvlptr.end() - 1);
        for (int J = 0; J < nsn; ++J) recs_level[(size_t)nx[(size_t)lvl[J] - 1]++] = recs[(size_t)pos_of[(size_t)J]];
    }
    h->sp_lvlptr = lvlptr;
    // ---- product lists: slot e of the panel values <- sum_t fcoef[t] d[fcol[t]]
    const int64_t nslot = S.lptr[nsn];
    std::vector<int> fptr((size_t)nslot + 1, 0), fcol;
    std::vector<double> fcoef;
    {
        size_t terms = 0;
        for (int j = 0; j < n; ++j) { const size_t c = (size_t)(cp[j + 1] - cp[j]); terms += c * (c + 1) / 2; }
        if (terms > ((size_t)1 << 30)) return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: %zu products in A D^2 A^T (use the dense path)", terms);
        fcol.resize(terms); fcoef.resize(terms);
        std::vector<int> where((size_t)m, -1);
        // pass 1: counts per slot, pass 2: fill (columns ascending within a slot)
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<int> nx;
            if (pass == 1) {
                for (int64_t e = 0; e < nslot; ++e) fptr[(size_t)e + 1] += fptr[(size_t)e];
                nx.assign(fptr.begin(), fptr.end() - 1);
            }
            for (int J = 0; J < nsn; ++J) {
                const int64_t r0 = S.rowptr[J];
                const int r = nodes[J].r, w = nodes[J].w, c0 = nodes[J].c0;
                for (int a = 0; a < r; ++a) where[S.rows[(size_t)(r0 + a)]] = a;
                for (int b = 0; b < w; ++b) {
                    const int k = c0 + b;
                    for (int p = rp[k]; p < rp[k + 1]; ++p) {                    // columns of A ascending
                        const int j = ci[p];
                        const double akj = rv[p];
                        for (int q = cp[j]; q < cp[j + 1]; ++q) {
                            const int i = ri[q];
                            if (i < k) continue;
                            const int a = where[i];
                            if (a < 0) return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: internal error (entry outside the front)");
                            const int64_t e = S.lptr[J] + (int64_t)a * w + b;
                            if (pass == 0) fptr[(size_t)e + 1]++;
                            else { const int t = nx[(size_t)e]++; fcol[(size_t)t] = j; fcoef[(size_t)t] = cv[q] * akj; }
                        }
                    }
                }
                for (int a = 0; a < r; ++a) where[S.rows[(size_t)(r0 + a)]] = -1;
            }
        }
        h->sp_terms = (long long)terms;
    }
    // ---- upload
    SpFactor& F = h->spF;
    memset(&F, 0, sizeof F);
    F.nsn = nsn; F.ntask = ntask; F.m = m;
    int rc;
    SpNode* d_node = nullptr; int *d_rows = nullptr, *d_child = nullptr, *d_crel = nullptr, *d_taskptr = nullptr, *d_tasknode = nullptr, *d_taskof = nullptr;
    SpRec* d_rec = nullptr;
    if ((rc = sp_upload(h, recs, &d_rec))) return rc;
    F.rec = d_rec;
    if ((rc = sp_upload(h, recs_level, &h->sp_rec_level))) return rc;
    h->sp_level_mode = 0;             // IPM_SP_MODE=level: always one launch per level; =task: never (A/B under contention); unset: sp_level()
    if (const char* e = getenv("IPM_SP_MODE")) h->sp_level_mode = !strcmp(e, "level") ? 1 : (!strcmp(e, "task") ? -1 : 0);
    if ((rc = sp_upload(h, nodes, &d_node))) return rc;
    if ((rc = sp_upload(h, S.rows, &d_rows))) return rc;
    if ((rc = sp_upload(h, S.child, &d_child))) return rc;
    if ((rc = sp_upload(h, S.crel, &d_crel))) return rc;
    if ((rc = sp_upload(h, taskptr, &d_taskptr))) return rc;
    if ((rc = sp_upload(h, tasknode, &d_tasknode))) return rc;
    if ((rc = sp_upload(h, taskof, &d_taskof))) return rc;
    if ((rc = sp_upload(h, fptr, &h->sp_fptr))) return rc;
    if ((rc = sp_upload(h, fcol, &h->sp_fcol))) return rc;
    if ((rc = sp_upload(h, fcoef, &h->sp_fcoef))) return rc;
    { std::vector<long long> dp(S.diagpos.begin(), S.diagpos.end()); if ((rc = sp_upload(h, dp, &h->sp_diagpos))) return rc; }
    F.node = d_node; F.rows = d_rows; F.child = d_child; F.crel = d_crel; F.taskptr = d_taskptr; F.tasknode = d_tasknode; F.taskof = d_taskof;
    if ((rc = sp_alloc_zero(h, (size_t)nslot, &F.L))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)S.uptr[nsn], &F.U))) return rc;
    if ((rc = sp_alloc_zero(h, S.rows.size(), &F.uvec))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)m, &F.dinv))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)3 * nsn, &F.flag))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)8, &F.ctr))) return rc;
    F.timeout = h->d_flags + 2 * (size_t)h->nblk;
    F.done = &h->sc->done;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->sp_nslot = nslot; h->sp_nu = S.uptr[nsn]; h->sp_height = S.height; h->sp_rmax = S.rmax; h->sp_nvirtual = S.nvirtual;
    h->sp_lds_doubles = (int)std::max<int64_t>(std::max<int64_t>(16, S.panel_max), std::min<int64_t>((int64_t)S.rmax * S.rmax, SPC_FRONT));
    {   // LDS of the factorization kernel: the largest panel image with its padded row stride (sparse_chol.h: sp_chol_lds_need)
        long long need = 16;
        for (int J = 0; J < nsn; ++J) need = std::max(need, sp_chol_lds_need((int)(S.rowptr[(size_t)J + 1] - S.rowptr[(size_t)J]), S.w[(size_t)J], h->sp_lds_doubles));
        h->sp_fv_off = (int)need;
        h->sp_lds_chol = sizeof(double) * ((size_t)need + (size_t)std::max(16, S.rmax));      // + the r-vector of the fused forward substitution
        if (const char* e = getenv("IPM_SP_FUSE_FWD")) h->sp_fuse_fwd = atoi(e);
    }
    h->sp_lds_solve = sizeof(double) * ((size_t)std::max(16, S.rmax) + SPC_WCAP * SPC_WCAP);
    h->sp_threads = threads;
    if (h->sp_lds_solve > 48 * 1024 || h->sp_lds_chol > 48 * 1024) {
        // fronts beyond ~5000 rows: the forward sweep's update vector + diagonal block pass the default dynamic-LDS limit
        const int cap = 96 * 1024;
        if (h->sp_lds_solve > (size_t)cap || h->sp_lds_chol > (size_t)cap) return fail(h, IPM_ERR_INVALID_ARG, "sparse factor: a front of %d rows exceeds the LDS budget of the sweeps", S.rmax);
        HIP_TRY(h, hipFuncSetAttribute((const void*)sp_fwd_kernel<SPC_THREADS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        HIP_TRY(h, hipFuncSetAttribute((const void*)sp_chol_kernel<SPC_THREADS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
    }
    // Fence-free hand-off (write-through stores + sc1 loads) is OPT-IN (IPM_SP_SC1=1): it passes every test and is 8-12 % faster
    // per sweep at STOCFOR3 (0.358 / 0.182 / 0.141 -> 0.328 / 0.161 / 0.132 ms), but this kernel runs several workgroups per CU,
    // outside the configurations that form is documented for; the release / acquire pair is the default.
    {   // workgroups the chip holds at once: LDS- or wave-limited (32 waves per CU)
        const size_t lds = std::max(h->sp_lds_chol, h->sp_lds_solve) + 512;
        const int wave_cap = threads == 64 ? 16 : 8;
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((size_t)wave_cap, (size_t)(160 * 1024) / lds));
        h->sp_grid = std::max(1, std::min(ntask, 256 * per_cu));
    }
    if (const char* e = getenv("IPM_SP_GRID")) h->sp_grid = std::max(1, std::min(ntask, atoi(e)));
    h->sp_epoch = 0; h->sp_serial = false;
    h->spf = true;
    return IPM_OK;
}

extern "C" int ipm_order_rows(int64_t m, int64_t n, const int32_t* colptr, const int32_t* rowind, int32_t* perm, double info[8]) {
    if (m <= 0 || n <= 0 || !colptr || !rowind || !perm || m > (1 << 24)) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_order_rows: bad arguments");
    for (int64_t i = 0; i < m; ++i) perm[i] = (int32_t)i;
    // info[0] on input (optional, > 0, with info[1] = -1 as the marker): the ms per iteration the caller's alternative (the dense-tile path) is predicted to take.
    // The elimination then stops early (IPM_ERR_WORKSPACE, as for a pattern that fills to dense) at the first pivot whose degree d
    // shows that the sparse factor cannot win: the fronts on the way from that pivot to the root have d, d - 32, d - 64 ... rows,
    // i.e. at least d^3 / 96 row^2 on the critical path at 3.5e-6 ms each (the fit of DESIGN 4-S), and a 10 % gain is asked for.
    // The work budget of the elimination shrinks with it: on the 73 Netlib files every LP that ends on the sparse factor is ordered
    // within 1.2e7 units of work (CZPROB), while the ones that fill up burn the full 6e7 (0.1 - 0.27 s of host time each) before
    // they give up -- 2e7 + 4e6 per ms of the alternative keeps a 2x margin for an LP of a millisecond per iteration and the full
    // budget for STOCFOR3-sized ones (10 ms).
    int degree_cap = 0;
    int64_t work_budget = (int64_t)6e7;
    if (info && info[1] == -1.0 && info[0] > 0.0 && info[0] < 1e6) {      // explicit opt-in (info[1] = -1): an uninitialised info array must not trigger it
        degree_cap = std::max(64, (int)std::cbrt(info[0] * 96.0 / 3.5e-6 / 1.1));
        work_budget = std::min<int64_t>(work_budget, (int64_t)(2e7 + 4e6 * info[0]));
    }
    if (info) for (int k = 0; k < 8; ++k) info[k] = 0.0;
    if (colptr[0] != 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_order_rows: colptr[0] != 0");
    for (int64_t j = 0; j < n; ++j) {
        if (colptr[j + 1] < colptr[j]) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_order_rows: colptr not monotone");
        for (int32_t p = colptr[j]; p < colptr[j + 1]; ++p)
            if (rowind[p] < 0 || rowind[p] >= m) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_order_rows: row index %d out of range", rowind[p]);
    }
    std::vector<int> pv;
    sym::OrderInfo oi;
    sym::Pattern P;                    // pattern of A A^T in the final order: formed once per LP, reused by the analysis below
    if (sym::order_rows((int)m, (int)n, colptr, rowind, pv, oi, (int64_t)6e7, &P, degree_cap, work_budget)) return fail(nullptr, IPM_ERR_WORKSPACE, "ipm_order_rows: A A^T is too dense for the sparse factor");
    for (int64_t i = 0; i < m; ++i) perm[i] = pv[(size_t)i];
    if (info) {
        info[0] = (double)oi.nnz_pattern; info[1] = (double)oi.nnz_factor; info[2] = oi.flops; info[3] = (double)oi.height;
        // the panel tree the device would walk (the analysis ipm_set_A_csc needs for the rows in this order): what a cost model
        // needs.  Kept for that call (sym_cache): the caller permutes the rows and hands the matrix over next.
        sym::Supernodes S;
        double relax = 1.0;
            if ((int64_t)P.idx.size() <= (int64_t)1.5e8 && sym::analyse(P, SPC_WCAP, SPC_PANEL, S, (int64_t)2.5e8, relax) == 0) {
            double area = 0.0; int levels = 0;
            sym::critical_path(S, area, levels);
            info[4] = (double)S.height; info[5] = area; info[6] = (double)S.nsn; info[7] = (double)S.rmax;
            SymCacheEntry e;
            e.m = (int)m; e.n = (int)n; e.relax = relax;
            std::vector<int> pos((size_t)m);
            for (int64_t k = 0; k < m; ++k) pos[(size_t)pv[(size_t)k]] = (int)k;
            e.cp.assign(colptr, colptr + n + 1);
            e.ri.resize((size_t)colptr[n]);
            for (int64_t j = 0; j < n; ++j) {
                for (int32_t q = colptr[j]; q < colptr[j + 1]; ++q) e.ri[(size_t)q] = pos[(size_t)rowind[q]];
                std::sort(e.ri.begin() + colptr[j], e.ri.begin() + colptr[j + 1]);
            }
            e.S = std::move(S);
            std::lock_guard<std::mutex> lock(g_sym_mutex);
            if (g_sym_cache.size() >= 8) g_sym_cache.pop_front();
            g_sym_cache.push_back(std::move(e));
        }
    }
    return IPM_OK;
}

extern "C" int ipm_get_factor_info(ipm_handle* h, int64_t out[8]) {
    if (!h || !out) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_factor_info: bad arguments");
    if (!h->spf) return fail(h, IPM_ERR_STATE, "ipm_get_factor_info: the handle has no sparse factor (IPM_FLAG_SPARSE_FACTOR)");
    out[0] = h->spF.nsn; out[1] = h->spF.ntask; out[2] = h->sp_height; out[3] = h->sp_rmax; out[4] = h->sp_nslot; out[5] = h->sp_nu;
    out[6] = h->sp_terms; out[7] = h->sp_serial_launches;
    return IPM_OK;
}

extern "C" int ipm_set_A_csc(ipm_handle* h, const int32_t* colptr, const int32_t* rowind, const double* val, int64_t nnz) {
    if (!h || !colptr || (nnz > 0 && (!rowind || !val)) || nnz < 0) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_A_csc: bad arguments");
    if (colptr[0] != 0 || colptr[h->n] != nnz) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_A_csc: colptr does not span nnz");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->sparse) {
        // canonical CSC (rows sorted, duplicates summed) and its CSR transpose, built on the host
        std::vector<int> cp(h->n + 1, 0), ri; std::vector<double> cv;
        ri.reserve((size_t)nnz); cv.reserve((size_t)nnz);
        std::vector<std::pair<int, double>> col;
        for (int64_t j = 0; j < h->n; ++j) {
            if (colptr[j + 1] < colptr[j]) return fail(h, IPM_ERR_INVALID_ARG, "colptr not monotone");
            col.clear();
            for (int32_t p = colptr[j]; p < colptr[j + 1]; ++p) {
                if (rowind[p] < 0 || rowind[p] >= h->m) return fail(h, IPM_ERR_INVALID_ARG, "row index %d out of range", rowind[p]);
                if (!isfinite(val[p])) return fail(h, IPM_ERR_INVALID_INPUT, "A has non-finite entries");
                col.emplace_back(rowind[p], val[p]);
            }
            std::stable_sort(col.begin(), col.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
            for (size_t q = 0; q < col.size(); ++q) {
                if (!ri.empty() && (int64_t)ri.size() > cp[j] && ri.back() == col[q].first) cv.back() += col[q].second;
                else { ri.push_back(col[q].first); cv.push_back(col[q].second); }
            }
            cp[j + 1] = (int)ri.size();
        }
        const int64_t nz = (int64_t)ri.size();
        if (nz > h->nnz_cap) return fail(h, IPM_ERR_INVALID_ARG, "nnz %lld exceeds the handle's sparse_nnz %lld", (long long)nz, (long long)h->nnz_cap);
        std::vector<int> rp(h->m + 1, 0), ci((size_t)nz); std::vector<double> rv((size_t)nz);
        for (int64_t q = 0; q < nz; ++q) rp[ri[q] + 1]++;
        for (int64_t i = 0; i < h->m; ++i) rp[i + 1] += rp[i];
        { std::vector<int> next(rp.begin(), rp.end() - 1);
          for (int64_t j = 0; j < h->n; ++j)
              for (int q = cp[j]; q < cp[j + 1]; ++q) { int dst = next[ri[q]]++; ci[dst] = (int)j; rv[dst] = cv[q]; } }
        HIP_TRY(h, hipMemcpyAsync(h->d_colptr, cp.data(), sizeof(int) * (h->n + 1), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_rowptr, rp.data(), sizeof(int) * (h->m + 1), hipMemcpyHostToDevice, h->stream));
        if (nz > 0) {
            HIP_TRY(h, hipMemcpyAsync(h->d_rowind, ri.data(), sizeof(int) * nz, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(h->d_cval, cv.data(), sizeof(double) * nz, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(h->d_colind, ci.data(), sizeof(int) * nz, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(h->d_rval, rv.data(), sizeof(double) * nz, hipMemcpyHostToDevice, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        {   // tile envelope of A A^T: B(i,k) != 0 structurally iff some column of A has rows in blocks i and k
            std::vector<int> last(h->nblk);
            for (int k = 0; k < h->nblk; ++k) last[k] = k;
            for (int64_t j = 0; j < h->n; ++j) {
                if (cp[j + 1] == cp[j]) continue;
                const int top = ri[cp[j + 1] - 1] / NB;                 // rows are sorted within a column
                for (int q = cp[j]; q < cp[j + 1]; ++q) { int kb = ri[q] / NB; if (last[kb] < top) last[kb] = top; }
            }
            for (int k = 1; k < h->nblk; ++k) if (last[k] < last[k - 1]) last[k] = last[k - 1];
            std::vector<int> first(h->nblk);
            for (int i = 0, c = 0; i < h->nblk; ++i) { while (last[c] < i) ++c; first[i] = c; }
            double work = 0.0, dense = 0.0;
            for (int k = 0; k < h->nblk; ++k) { double w = last[k] - k, d = h->nblk - 1 - k; work += w * w; dense += d * d; }
            h->env_last = last; h->env_first = first;
            h->use_env = h->envelope != 0 && work < 0.8 * dense;         // only when it actually removes work
        }
        h->nnz = nz; h->haveA = true; h->predictor_valid = false;
        h->small = false; h->list_form = false;
        {
            // Product list: lower entry (i, k) of B = A diag(d) A^T is sum_t coef[t] d[col[t]] over the columns that rows
            // i and k share (coef = a_ij a_kj) -- a sparse matrix-vector product with d.  Entries ordered by (i, k), terms
            // by column: a fixed summation order.  Used by the fused small-LP kernel (m <= 128) and, for sparse handles up
            // to 1536 padded rows, by adat_list_kernel (one thread per entry instead of one workgroup per row of B walking
            // its nonzeros one dependent load at a time).
            size_t terms = 0;
            for (int64_t j = 0; j < h->n; ++j) { const size_t c = (size_t)(cp[j + 1] - cp[j]); terms += c * (c + 1) / 2; }
            const bool want_small = h->fused_small && h->m <= SMALL_MAX_M && terms <= ((size_t)1 << 22);
            // (measured, ms per iteration list / row-owner: SHELL (8 blocks) 0.778 / 0.810, DEGEN3 (12) 1.13 / 1.12, PILOT87 (30)
            //  2.44 / 2.38: the zero fill of B eats the gain from 16 blocks on)
            const bool want_list = h->list_form_opt && h->m > SMALL_MAX_M && h->mp <= 1536 && terms <= ((size_t)1 << 24);
            if (want_small || want_list) {
                const int M = (int)h->m;
                std::vector<int> bptr(1, 0), bi, bk, mark((size_t)M, -1), cntk((size_t)M, 0), startk((size_t)M, 0), touched;
                // list path: entries up to the end of row i's 16 x 16 diagonal tile (potrf_diag reads those tiles whole), each
                // computed from its own row's point of view -- exactly the values, products and order of adat_sparse_kernel
                const int hi_mask = want_small ? 0 : 15;
                std::vector<int> bcol;
                std::vector<double> bai, bak;
                bcol.reserve(terms + 16 * (size_t)M); bai.reserve(terms + 16 * (size_t)M); bak.reserve(terms + 16 * (size_t)M);
                for (int i = 0; i < M; ++i) {
                    const int hi = std::min(i | hi_mask, M - 1);
                    touched.clear();
                    mark[i] = i; cntk[i] = 0; touched.push_back(i);                       // the diagonal entry always exists
                    for (int p = rp[i]; p < rp[i + 1]; ++p) {
                        const int j = ci[p];
                        for (int q = cp[j]; q < cp[j + 1] && ri[q] <= hi; ++q) {           // rows sorted within a column
                            const int k = ri[q];
                            if (mark[k] != i) { mark[k] = i; cntk[k] = 0; touched.push_back(k); }
                            ++cntk[k];
                        }
                    }
                    std::sort(touched.begin(), touched.end());
                    for (int k : touched) {
                        startk[k] = bptr.back();
                        bi.push_back(i); bk.push_back(k);
                        bptr.push_back(bptr.back() + cntk[k]);
                    }
                    bcol.resize((size_t)bptr.back()); bai.resize((size_t)bptr.back()); bak.resize((size_t)bptr.back());
                    for (int p = rp[i]; p < rp[i + 1]; ++p) {                              // columns ascending within the row
                        const int j = ci[p];
                        const double aij = rv[p];
                        for (int q = cp[j]; q < cp[j + 1] && ri[q] <= hi; ++q) {
                            const int t = startk[ri[q]]++;
                            bcol[t] = j; bai[t] = aij; bak[t] = cv[q];
                        }
                    }
                }
                if (bcol.empty()) { bcol.push_back(0); bai.push_back(0.0); bak.push_back(0.0); }
                std::vector<double> bcoef(bcol.size());
                for (size_t t = 0; t < bcol.size(); ++t) bcoef[t] = bai[t] * bak[t];
                for (void** p : {(void**)&h->sm_bptr, (void**)&h->sm_bcol, (void**)&h->sm_bi, (void**)&h->sm_bk, (void**)&h->sm_bcoef,
                                 (void**)&h->ls_bi, (void**)&h->ls_bk, (void**)&h->ls_bak})
                    if (*p) { dev_free(h->device, h->stream, *p); *p = nullptr; }
                h->sm_nb = (int)bi.size();
                const size_t nt_ = bcol.size();
                HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->sm_bptr, sizeof(int) * bptr.size()));
                HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->sm_bcol, sizeof(int) * nt_));
                HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->sm_bcoef, sizeof(double) * nt_));
                HIP_TRY(h, hipMemcpyAsync(h->sm_bptr, bptr.data(), sizeof(int) * bptr.size(), hipMemcpyHostToDevice, h->stream));
                HIP_TRY(h, hipMemcpyAsync(h->sm_bcol, bcol.data(), sizeof(int) * nt_, hipMemcpyHostToDevice, h->stream));
                HIP_TRY(h, hipMemcpyAsync(h->sm_bcoef, want_small ? bcoef.data() : bai.data(), sizeof(double) * nt_, hipMemcpyHostToDevice, h->stream));
                if (want_small) {
                    std::vector<unsigned short> si(bi.begin(), bi.end()), sk(bk.begin(), bk.end());
                    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->sm_bi, sizeof(unsigned short) * si.size()));
                    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->sm_bk, sizeof(unsigned short) * sk.size()));
                    HIP_TRY(h, hipMemcpyAsync(h->sm_bi, si.data(), sizeof(unsigned short) * si.size(), hipMemcpyHostToDevice, h->stream));
                    HIP_TRY(h, hipMemcpyAsync(h->sm_bk, sk.data(), sizeof(unsigned short) * sk.size(), hipMemcpyHostToDevice, h->stream));
                    h->small = true;
                } else {
                    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->ls_bi, sizeof(int) * bi.size()));
                    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->ls_bk, sizeof(int) * bk.size()));
                    HIP_TRY(h, hipMemcpyAsync(h->ls_bi, bi.data(), sizeof(int) * bi.size(), hipMemcpyHostToDevice, h->stream));
                    HIP_TRY(h, hipMemcpyAsync(h->ls_bk, bk.data(), sizeof(int) * bk.size(), hipMemcpyHostToDevice, h->stream));
                    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->ls_bak, sizeof(double) * nt_));
                    HIP_TRY(h, hipMemcpyAsync(h->ls_bak, bak.data(), sizeof(double) * nt_, hipMemcpyHostToDevice, h->stream));
                    h->list_form = true;
                }
                // (stream-ordered copies + one sync: the library issues NO legacy-stream operation -- another host thread may
                //  be capturing a graph on a blocking stream, which a NULL-stream copy would illegally depend on)
                HIP_TRY(h, hipStreamSynchronize(h->stream));
            }
        }
        if ((h->opt.flags & IPM_FLAG_SPARSE_FACTOR) && !h->small) {      // (m <= 128: the fused single-workgroup kernel serves the LP)
            int rc = build_sparse_factor(h, cp, ri, cv, rp, ci, rv);
            if (rc) { h->haveA = false; return rc; }
        }
        return IPM_OK;
    }
    // dense row-major image of A (scattered on the host, one upload)
    double* img = (double*)calloc((size_t)h->mp * h->np, sizeof(double));
    if (!img) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_A_csc: host allocation of %lld x %lld failed", (long long)h->mp, (long long)h->np);
    for (int64_t j = 0; j < h->n; ++j) {
        if (colptr[j + 1] < colptr[j]) { free(img); return fail(h, IPM_ERR_INVALID_ARG, "colptr not monotone"); }
        for (int32_t p = colptr[j]; p < colptr[j + 1]; ++p) {
            int32_t i = rowind[p];
            if (i < 0 || i >= h->m) { free(img); return fail(h, IPM_ERR_INVALID_ARG, "row index %d out of range", i); }
            if (!isfinite(val[p])) { free(img); return fail(h, IPM_ERR_INVALID_INPUT, "A has non-finite entries"); }
            img[(int64_t)i * h->np + j] += val[p];      // duplicates sum, as scipy's csc constructor does
        }
    }
    hipError_t e = hipMemcpyAsync(h->A, img, sizeof(double) * h->mp * h->np, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(img);
    if (e != hipSuccess) return fail(h, IPM_ERR_HIP, "upload of A failed: %s", hipGetErrorString(e));
    h->haveA = true; h->predictor_valid = false;
    return IPM_OK;
}

// native upper bounds: views into the BND_VECS n-vectors of ipm_set_bounds
static const int BND_VECS = 10;
static BndArgs bnd_args(ipm_handle* h) {
    const size_t np = (size_t)h->np;
    double* p = h->bnd_mem;
    BndArgs b;
    b.u = p; b.w = p + np; b.z = p + 2 * np; b.dwa = p + 3 * np; b.dza = p + 4 * np; b.dw = p + 5 * np; b.dz = p + 6 * np;
    b.qz = p + 7 * np; b.nU = h->bnd_nU;
    return b;
}

extern "C" int ipm_set_bc(ipm_handle* h, const double* b, const double* c) {
    if (!h || !b || !c) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_bc: bad arguments");
    if (!all_finite(b, 1, h->m, h->m) || !all_finite(c, 1, h->n, h->n)) return fail(h, IPM_ERR_INVALID_INPUT, "b or c has non-finite entries");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->b, b, sizeof(double) * h->m, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->c, c, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    if (h->bnd) hipLaunchKernelGGL(bnd_norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->b, (int)h->m, bnd_args(h).u, (int)h->n, &h->sc->b_norm);
    else hipLaunchKernelGGL(norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->b, (int)h->m, &h->sc->b_norm);
    hipLaunchKernelGGL(norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->c, (int)h->n, &h->sc->c_norm);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->haveBC = true; h->predictor_valid = false;
    return IPM_OK;
}

extern "C" int ipm_set_state(ipm_handle* h, const double* x, const double* y, const double* s) {
    if (!h || !x || !y || !s) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_state: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->x, x, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->y, y, sizeof(double) * h->m, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->s, s, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->haveState = true; h->predictor_valid = false; h->fresh_state = true;
    h->h_sc->status = 0;                                       // (a certificate describes the iterate of its detection only)
    return IPM_OK;
}

extern "C" int ipm_get_state(ipm_handle* h, double* x, double* y, double* s) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_state: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    if (x) HIP_TRY(h, hipMemcpyAsync(x, h->x, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    if (y) HIP_TRY(h, hipMemcpyAsync(y, h->y, sizeof(double) * h->m, hipMemcpyDeviceToHost, h->stream));
    if (s) HIP_TRY(h, hipMemcpyAsync(s, h->s, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
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
            if (v < std::numeric_limits<double>::infinity()) ++nU;
        }
    }
    h->predictor_valid = false;
    if (nU == 0) {                                             // NULL or all +inf: the unbounded code, exactly
        h->bnd = false; h->bnd_nU = 0;
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
    HIP_TRY(h, hipMemcpyAsync(h->bnd_mem, uu.data(), sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
    h->bnd = true; h->bnd_nU = nU;
    const BndArgs bd = bnd_args(h);
    hipLaunchKernelGGL(bnd_fill_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, bd.u, bd.w, bd.z, (int)np, 1.0, 0);
    if (h->haveBC) hipLaunchKernelGGL(bnd_norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->b, (int)h->m, bd.u, (int)h->n, &h->sc->b_norm);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return IPM_OK;
}

extern "C" int ipm_set_bound_state(ipm_handle* h, const double* w, const double* z) {
    if (!h || !w || !z) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_bound_state: bad arguments");
    if (!h->bnd) return fail(h, IPM_ERR_STATE, "ipm_set_bound_state: no finite bound is set (ipm_set_bounds)");
    HIP_TRY(h, hipSetDevice(h->device));
    const BndArgs bd = bnd_args(h);
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
    return IPM_OK;
}

extern "C" int ipm_init_state(ipm_handle* h, double y0) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_init_state: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = enqueue_init_state(h, y0);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->haveState = true; h->predictor_valid = false; h->fresh_state = true;
    h->h_sc->status = 0;                                       // (a certificate describes the iterate of its detection only)
    return IPM_OK;
}

// ------------------------------------------------------------------------------- launch sequence
static VecArgs vec_args(ipm_handle* h) {
    VecArgs a;
    a.m = (int)h->m; a.n = (int)h->n; a.np = (int)h->np; a.rc_chunks = h->rc_chunks; a.nblk = h->vblk;
    a.atp = h->atp; a.x = h->x; a.y = h->y; a.s = h->s; a.b = h->b; a.c = h->c;
    a.rb = h->rb; a.rc = h->rc; a.d = h->d; a.v = h->v; a.q = h->q;
    a.dxa = h->dxa; a.dya = h->dya; a.dsa = h->dsa; a.dx = h->dx; a.dy = h->dy; a.ds = h->ds;
    a.part = h->part; a.sc = h->sc; a.hist = h->hist;
    return a;
}

static SparseA sparse_view(const ipm_handle* h) {
    SparseA A;
    A.rowptr = h->d_rowptr; A.colind = h->d_colind; A.rval = h->d_rval;
    A.colptr = h->d_colptr; A.rowind = h->d_rowind; A.cval = h->d_cval;
    A.m = (int)h->m; A.n = (int)h->n;
    return A;
}

static void launch_gemv_n(ipm_handle* h, const double* v, double sa, double sb, const double* add, double* out,
                          hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    if (h->sparse) {
        const LsSpmv p{sparse_view(h), (int)h->mp, v, sa, sb, add, out, &h->sc->done};
        if (ls_push(h, LS_SPMV_CSR, (unsigned)((h->mp + 15) / 16), p)) return;
        hipLaunchKernelGGL(spmv_csr_kernel, dim3((unsigned)((h->mp + 15) / 16)), dim3(256), 0, st, sparse_view(h),
                           (int)h->mp, v, sa, sb, add, out, &h->sc->done);
        return;
    }
    hipLaunchKernelGGL(gemv_n_kernel, dim3((unsigned)(h->mp / 4)), dim3(256), 0, st, h->A, h->np, (int)h->mp,
                       (int)h->np, v, sa, sb, add, out, &h->sc->done);
}
static void launch_gemv_t(ipm_handle* h, const double* u, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    if (h->sparse) {
        const LsSpmvT p{sparse_view(h), (int)h->np, u, h->atp, &h->sc->done};
        if (ls_push(h, LS_SPMV_CSC_T, (unsigned)((h->np + 15) / 16), p)) return;
        hipLaunchKernelGGL(spmv_csc_t_kernel, dim3((unsigned)((h->np + 15) / 16)), dim3(256), 0, st, sparse_view(h),
                           (int)h->np, u, h->atp, &h->sc->done);
        return;
    }
    dim3 grid((unsigned)((h->np + 511) / 512), (unsigned)h->rc_chunks);
    hipLaunchKernelGGL(gemv_t_kernel, grid, dim3(256), 0, st, h->A, h->np, h->rows_per_chunk, (int)h->np, u,
                       h->atp, &h->sc->done);
}

static DetArgs det_args(const ipm_handle* h) { return DetArgs{h->det_eps_p, h->det_eps_d, h->det}; }

// r_b, r_c, d, predictor v, stop test (and, with IPM_FLAG_DETECT_INFEASIBILITY, the infeasibility tests): the one launch site of the
// stop test of every multi-kernel path (dense, sparse envelope, sparse factor, fused formation + factorization, lockstep)
static int enqueue_residuals(ipm_handle* h, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    VecArgs a = vec_args(h);
    launch_gemv_n(h, h->x, 1.0, -1.0, h->b, h->rb, st);             // r_b = A x - b
    launch_gemv_t(h, h->y, st);                                     // A^T y (partials)
    if (h->bnd && h->detect) {
        hipLaunchKernelGGL(prepare_bounded_detect_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a, bnd_args(h));
        hipLaunchKernelGGL(stop_test_bounded_detect_kernel, dim3(1), dim3(64), 0, st, a, bnd_args(h), det_args(h));
    } else if (h->bnd) {                                            // (a bounded handle is never recorded: ls_eligible)
        hipLaunchKernelGGL(prepare_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a, bnd_args(h));
        hipLaunchKernelGGL(stop_test_bounded_kernel, dim3(1), dim3(64), 0, st, a, bnd_args(h));
    } else if (h->detect) {                                         // the infeasibility tests: their own lockstep twins
        const LsVecDet p{a, det_args(h)};
        if (!ls_push(h, LS_PREPARE_DETECT, (unsigned)h->vblk, p)) hipLaunchKernelGGL(prepare_detect_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a);
        if (!ls_push(h, LS_STOP_TEST_DETECT, 1u, p)) hipLaunchKernelGGL(stop_test_detect_kernel, dim3(1), dim3(64), 0, st, a, det_args(h));
    } else {
        if (!ls_push(h, LS_PREPARE, (unsigned)h->vblk, LsVecA{a, 0})) hipLaunchKernelGGL(prepare_kernel, dim3(h->vblk), dim3(VBLK), 0, st, a);
        if (!ls_push(h, LS_STOP_TEST, 1u, LsVecA{a, 0})) hipLaunchKernelGGL(stop_test_kernel, dim3(1), dim3(64), 0, st, a);
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// Residual stream: everything of an iteration that needs (x, y, s) but not the factor -- r_b, r_c, the stop test and the
// predictor's right-hand side, three of the six passes over A -- runs on its own stream while the pivot chain of the
// factorization leaves most of the chip idle.  Called from inside enqueue_factor once the chain-bound tail begins (the
// head of the factorization is bound by its trailing updates, which these HBM passes would only slow down).
static int enqueue_residual_stream(ipm_handle* h, hipStream_t chain) {
    HIP_TRY(h, hipEventRecord(h->ev_mid, chain));
    HIP_TRY(h, hipStreamWaitEvent(h->stream3, h->ev_mid, 0));
    int rc = enqueue_residuals(h, h->stream3);
    if (rc) return rc;
    launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1, h->stream3);   // predictor rhs = -r_b - A (d*t)
    HIP_TRY(h, hipEventRecord(h->ev_res, h->stream3));
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}
static bool overlap_residuals(const ipm_handle* h) {
    return h->stream3 != nullptr && h->profiling < 2;          // (created for dense handles from 16 blocks on, ipm_create)
}

static inline bool sp_on(const ipm_handle* h) { return h->spf && !h->spf_off; }
// Sparse factor: one launch per LEVEL of the panel tree (the kernel boundary is the hand-off, nothing spins) instead of one
// launch per sweep with flag hand-offs between tasks.  Chosen by IPM_SP_MODE=level, and automatically wherever the handle
// shares the device -- IPM_FLAG_NO_DEVICE_POLLING (batched mode) or more than one live handle: spinning consumers next to
// other LPs' kernels are what turned STOCFOR3's 0.10 s into 1.4-1.7 s in a shared run, and the level form measured equal
// under contention (73-LP suite 3.11-3.15 s vs 3.20-3.32 s).  Same arithmetic, bit-identical results.  Mirrors the `alone`
// rule of the dense look-ahead (enqueue_factor).
static inline bool sp_level(const ipm_handle* h) {
    if (h->sp_serial || h->sp_level_mode < 0) return false;
    if (h->sp_level_mode > 0 || (h->opt.flags & IPM_FLAG_NO_DEVICE_POLLING)) return true;
    return h->device < MAX_DEVICES && g_live[h->device].load(std::memory_order_acquire) > 1;
}
static inline unsigned sp_launch_grid(ipm_handle* h) {
    if (h->sp_serial) { ++h->sp_serial_launches; return 1u; }
    return (unsigned)h->sp_grid;
}

// B = A diag(d) A^T (lower tiles), unit diagonal on padding rows
// Dense B and inv(L_kk) for a handle whose workspace carries none (layout_no_dense): allocated on first use by a dense entry
// point, stream-ordered, freed in ipm_destroy.  A no-op everywhere else.
static int ensure_dense_B(ipm_handle* h) {
    if (h->B && h->invD) return IPM_OK;
    if (!h->no_dense) return fail(h, IPM_ERR_STATE, "handle has no dense normal-matrix buffer");
    if ((!h->B_own && dev_malloc(h->device, h->stream, (void**)&h->B_own, sizeof(double) * (size_t)h->mp * h->mp) != hipSuccess) ||
        (!h->invD_own && dev_malloc(h->device, h->stream, (void**)&h->invD_own, sizeof(double) * (size_t)h->nblk * NB * NB) != hipSuccess))
        return fail(h, IPM_ERR_HIP, "dense normal-matrix buffer (%lld x %lld doubles) could not be allocated", (long long)h->mp, (long long)h->mp);   // (what was allocated stays owned: freed in ipm_destroy, reused by a later call)
    HIP_TRY(h, hipMemsetAsync(h->invD_own, 0, sizeof(double) * (size_t)h->nblk * NB * NB, h->stream));
    h->B = h->B_own; h->invD = h->invD_own;
    return IPM_OK;
}

static int enqueue_form(ipm_handle* h, const double* d, bool dense_image = false) {
    if (sp_on(h) && !dense_image) {
        // the entries of B go straight into the panels of the sparse factor (one thread per slot, fixed term order)
        hipLaunchKernelGGL(sp_form_kernel, dim3((unsigned)((h->sp_nslot + 255) / 256)), dim3(256), 0, h->stream, h->sp_fptr, h->sp_fcol,
                           h->sp_fcoef, h->sp_nslot, d, h->spF.L, &h->sc->maxdiag, &h->sc->done);
        hipLaunchKernelGGL(sp_maxdiag_kernel, dim3((unsigned)((h->m + 255) / 256)), dim3(256), 0, h->stream, h->spF.L, h->sp_diagpos, (int)h->m, &h->sc->maxdiag,
                           &h->sc->done);
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    if (int rc_ = ensure_dense_B(h)) return rc_;
    if (h->sparse && h->list_form) {
        const int64_t nB = h->mp * h->mp;                       // even (mp is a multiple of 128)
        const unsigned zgrid = (unsigned)std::min<int64_t>((nB / 2 + 255) / 256, 4096);
        if (!ls_push(h, LS_ZERO, zgrid, LsZero{h->B, nB, &h->sc->done}))
            hipLaunchKernelGGL(zero_unless_done_kernel, dim3(zgrid), dim3(256), 0, h->stream, h->B, nB, &h->sc->done);
        const int work = h->sm_nb + (int)(h->mp - h->m);
        const LsAdatList pl{h->sm_bptr, h->ls_bi, h->ls_bk, h->sm_bcol, h->sm_bcoef, h->ls_bak, h->sm_nb, d, h->B, h->mp, (int)h->m, (int)h->mp, &h->sc->done};
        if (!ls_push(h, LS_ADAT_LIST, (unsigned)((work + 255) / 256), pl))
            hipLaunchKernelGGL(adat_list_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, h->stream, h->sm_bptr, h->ls_bi, h->ls_bk,
                               h->sm_bcol, h->sm_bcoef, h->ls_bak, h->sm_nb, d, h->B, h->mp, (int)h->m, (int)h->mp, &h->sc->done);
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    if (h->sparse) {
        const LsAdatSp ps{sparse_view(h), d, h->B, h->mp, (int)h->mp, &h->sc->done};
        if (h->mp <= SP_LDS_MAX_MP) {          // dynamic-LDS attribute set per device in ipm_create
            if (!ls_push(h, LS_ADAT_SPARSE, (unsigned)h->mp, ps, (unsigned)(h->mp * sizeof(double))))
                hipLaunchKernelGGL(adat_sparse_kernel, dim3((unsigned)h->mp), dim3(256), (size_t)h->mp * sizeof(double), h->stream,
                                   sparse_view(h), d, h->B, h->mp, (int)h->mp, &h->sc->done);
        } else if (!ls_push(h, LS_ADAT_SPARSE_GLOBAL, (unsigned)h->mp, ps)) {
            hipLaunchKernelGGL(adat_sparse_global_kernel, dim3((unsigned)h->mp), dim3(256), 0, h->stream, sparse_view(h), d,
                               h->B, h->mp, (int)h->mp, &h->sc->done);
        }
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    GemmNT g = gemm_defaults();
    g.batch = 1; g.sP = g.sQ = g.sC = 0; g.batch2 = 1; g.sP2 = g.sQ2 = g.sC2 = 0;
    g.tile_order = h->d_tile_order;
    g.P = h->A; g.ldp = h->np; g.Q = h->A; g.ldq = h->np; g.w = d;
    g.C = h->B; g.ldc = h->mp; g.M = (int)h->mp; g.N = (int)h->mp; g.K = (int)h->np;
    g.alpha = 1.0; g.beta = 0.0; g.lower = 1; g.unit_diag_from = (int)h->m; g.done = h->fdone ? h->fdone : &h->sc->done;
    // the dedicated software-pipelined kernel (adat_syrk_f64.h; the generic gemm_nt kernel it replaced in round 2 computes the same bits)
    HIP_TRY(h, launch_adat_syrk(h->A, h->np, d, h->B, h->mp, (int)h->mp, (int)h->np, (int)h->m, h->fdone ? h->fdone : &h->sc->done,
                                h->d_tile_order, h->stream, h->slab, 512));
    return IPM_OK;
}

// blocked guarded Cholesky of B in place (lower), right-looking with one step of look-ahead:
//   main stream : potrf_diag(k) -> [wait bulk(k-1)] -> panel rows of block k+1 -> update of tile (k+1,k+1)
//   bulk stream : [wait diag(k)] panel rows >= k+2 -> [wait crit(k)] rest of the trailing update
// so the serial diagonal-block factorization of step k+1 overlaps the bulk update of step k.
static int enqueue_group_inverses(ipm_handle* h, int g0, int g1, hipStream_t st);
// sp_fwd_rhs (sparse factor only): right-hand side whose forward substitution rides on the factorization (z -> h->t2); the next
// enqueue_potrs of that right-hand side then runs the backward sweep only (h->sp_fwd_fused).
// 16-wide panels of diagonal block k that hold rows of the LP (the rest of the block is padding: unit diagonal): potrf_diag
// factors only those -- the last real block of an LP whose row count is no multiple of 128, and the blocks the layout pads with
static inline int potrf_panels(const ipm_handle* h, int k) {
    if (h->shift_rel != 0.0) return NB / 16;              // (the Tikhonov shift touches every diagonal entry: keep the full block)
    const int64_t real = h->m - (int64_t)k * NB;
    return real >= NB ? NB / 16 : (int)std::max<int64_t>(1, (real + 15) / 16);
}

static int enqueue_factor(ipm_handle* h, bool use_env = false, int mid_step = -1, int ginv_step = -1, const double* sp_fwd_rhs = nullptr) {
    if (sp_on(h)) {                     // multifrontal sparse Cholesky: one launch walks the elimination tree
        if (!h->sp_fuse_fwd) sp_fwd_rhs = nullptr;
        h->sp_fwd_fused = sp_fwd_rhs;
#define SP_LAUNCH_CHOL(NT, SC, GRID, RECS, COUNT)                                                                                  \
    hipLaunchKernelGGL((sp_chol_kernel<NT, SC>), dim3(GRID), dim3(NT), h->sp_lds_chol, h->stream, h->spF, ep, &h->sc->maxdiag,       \
                       h->opt.pivot_guard_eps, h->opt.pivot_guard_big, h->shift_rel, &h->sc->fixed, h->sp_lds_doubles, RECS, COUNT,    \
                       sp_fwd_rhs, h->t2, h->sp_fv_off)
#define SP_CHOL(GRID, RECS, COUNT)                                                                                                   \
    do {                                                                                                                             \
        SP_LAUNCH_CHOL(SPC_THREADS, false, GRID, RECS, COUNT);                                                                       \
    } while (0)
        const unsigned ep = ++h->sp_epoch;
        if (sp_level(h)) {
            // one launch per level of the panel tree, leaves first: the kernel boundary is the hand-off (~5 us against ~8-20 us
            // for a flag hand-off inside one launch), nothing spins, and concurrent handles interleave at launch granularity
            for (size_t l = 0; l + 1 < h->sp_lvlptr.size(); ++l) {
                const int cnt = h->sp_lvlptr[l + 1] - h->sp_lvlptr[l];
                SP_CHOL((unsigned)std::min(cnt, h->sp_grid), h->sp_rec_level + h->sp_lvlptr[l], cnt);
            }
        } else {
            SP_CHOL(sp_launch_grid(h), h->spF.rec, 0);
        }
#undef SP_CHOL
#undef SP_LAUNCH_CHOL
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    if (int rc_ = ensure_dense_B(h)) return rc_;
    const int* done = h->fdone ? h->fdone : &h->sc->done;
    use_env = use_env && h->use_env;
    // threshold scale = max diag over the TRUE rows only (padding rows carry a unit diagonal)
    if (!ls_push(h, LS_MAXDIAG, 1u, LsMaxdiag{h->B, h->mp, (int)h->m, &h->sc->maxdiag, done}))
        hipLaunchKernelGGL(maxdiag_kernel, dim3(1), dim3(256), 0, h->stream, h->B, h->mp, (int)h->m, &h->sc->maxdiag, done);
    const bool la = h->lookahead != 0 && h->nblk > 2 && h->stream2 != nullptr;
    // group size of the two-level schedule.  Measured (factor, ms): 16384 x 32768: 39.7 / 34.9 / 33.4 / 32.9 / 32.5 for groups
    // of 1 / 2 / 3 / 4 / 6; 8192 x 16384: 7.87 / 7.46 / 7.34 / 7.34 for 1 / 2 / 3 / 4; but 4096 x 8192: 2.21 -> 2.36 with groups
    // of 2 (half of its steps are bound by the pivot chain, which grouping lengthens): on from 48 blocks.
    // IPM_TWO_LEVEL=0 disables, IPM_GROUP_STEPS=n forces a group size (>= 8 blocks).
    int gs = 1;
    if (la && !use_env && h->two_level != 0) {
        if (h->group_steps > 0) gs = h->nblk >= 8 ? h->group_steps : 1;
        else if (h->nblk >= 96) gs = 4;
        else if (h->nblk >= 48) gs = 3;
    }
    // Group table: uniform groups of gs block columns (from 48 blocks on; one-level below that -- pairing only the head of the
    // factorization was measured and does not pay below 48 blocks either: 2.158 / 2.157 / 2.182 / 2.213 ms for 0 / 4 / 8 / 16 paired steps)
    std::vector<int> grp_lo(h->nblk), grp_hi(h->nblk);
    for (int k = 0; k < h->nblk; ++k) {
        if (gs > 1) { grp_lo[k] = (k / gs) * gs; grp_hi[k] = std::min(grp_lo[k] + gs, h->nblk); }
        else { grp_lo[k] = k; grp_hi[k] = k + 1; }
    }
    h->last_gs = gs;
    hipStream_t sm = h->stream, sb = la ? h->stream2 : h->stream;
    // device-polled hand-offs only while this is the one live handle on the device (see g_live)
    const bool alone = h->device >= MAX_DEVICES || g_live[h->device].load(std::memory_order_acquire) <= 1;
    const bool fs = la && h->flag_sync != 0 && alone;
    h->n_counter_steps = 0; h->n_event_steps = 0;
    std::vector<unsigned> bulk_wgs(h->nblk, 0u);          // workgroups of the bulk update of each step
    if (la) {
        if (fs) HIP_TRY(h, hipMemsetAsync(h->d_bulk_done, 0, sizeof(unsigned) * 2 * (size_t)h->nblk, sm));
        HIP_TRY(h, hipEventRecord(h->ev_fork, sm));
        HIP_TRY(h, hipStreamWaitEvent(sb, h->ev_fork, 0));
    }
    for (int k = 0; k < h->nblk; ++k) {
        PotrfDiag pd;
        pd.Bkk = h->B + (int64_t)k * NB * (h->mp + 1); pd.ld = h->mp;
        pd.inv = h->invD + (int64_t)k * NB * NB;
        pd.maxdiag = &h->sc->maxdiag; pd.eps = h->opt.pivot_guard_eps; pd.big = h->opt.pivot_guard_big; pd.shift_rel = h->shift_rel;
        pd.fixed = &h->sc->fixed; pd.done = done; pd.stamps = nullptr;
        pd.wait_on = nullptr; pd.wait_count = 0; pd.signal = nullptr; pd.timeout = nullptr; pd.dbg = nullptr; pd.dbg_tag = 0;
        pd.trace = nullptr;
        pd.nt = potrf_panels(h, k);
        pd.rows = (int)(h->m - (int64_t)k * NB);
        if (h->stamp_buf && k == 0) {
            pd.stamps = h->stamp_buf;
            if (getenv("IPM_POTRF_SKIP")) pd.dbg_tag = (unsigned)atoi(getenv("IPM_POTRF_SKIP"));
            hipLaunchKernelGGL(potrf_diag_kernel<true>, dim3(1), dim3(PD_THREADS), 0, sm, pd);
        } else if (!ls_push(h, LS_POTRF, 1u, pd)) {
            hipLaunchKernelGGL(potrf_diag_kernel<false>, dim3(1), dim3(PD_THREADS), 0, sm, pd);
        }
        if (k == ginv_step) {
            // blocks 0 .. k are final (the diagonal block k was just factored, every panel block left of it in these rows is
            // ordered before it through the look-ahead hand-offs): the inverses of the complete 1024-row groups go to the
            // residual stream, only the last group's is left for after the factorization
            HIP_TRY(h, hipEventRecord(h->ev_grp, sm));
            HIP_TRY(h, hipStreamWaitEvent(h->stream3, h->ev_grp, 0));
            int rc_ = enqueue_group_inverses(h, 0, (k + 1) / h->gsz, h->stream3);
            if (rc_) return rc_;
        }
        if (k == mid_step) { int rc_ = enqueue_residual_stream(h, sm); if (rc_) return rc_; }
        int rem = (int)(h->mp - (int64_t)(k + 1) * NB);
        if (rem <= 0) break;
        if (use_env) {                                              // rows below the envelope are zero and stay zero
            rem = std::min(rem, (h->env_last[k] - k) * NB);
            if (rem <= 0) {                                         // nothing below the diagonal block in this column
                if (la) HIP_TRY(h, hipEventRecord(h->ev_bulk[k], sb));
                continue;
            }
        }
        double* panel = h->B + (int64_t)(k + 1) * NB * h->mp + (int64_t)k * NB;
        GemmNT t = gemm_defaults();                                 // L_ik = B_ik inv(L_kk)^T, in place
        t.tile_order = nullptr; t.batch = 1; t.sP = t.sQ = t.sC = 0; t.batch2 = 1; t.sP2 = t.sQ2 = t.sC2 = 0;
        t.P = panel; t.ldp = h->mp; t.Q = pd.inv; t.ldq = NB; t.w = nullptr;
        t.C = panel; t.ldc = h->mp; t.M = rem; t.N = NB; t.K = NB;
        t.alpha = 1.0; t.beta = 0.0; t.lower = 0; t.unit_diag_from = -1; t.done = done;
        GemmNT u = gemm_defaults();                                 // B_ij -= L_ik L_jk^T
        u.tile_order = nullptr; u.batch = 1; u.sP = u.sQ = u.sC = 0; u.batch2 = 1; u.sP2 = u.sQ2 = u.sC2 = 0;
        u.P = panel; u.ldp = h->mp; u.Q = panel; u.ldq = h->mp; u.w = nullptr;
        u.C = h->B + (int64_t)(k + 1) * NB * (h->mp + 1); u.ldc = h->mp; u.M = rem; u.N = rem; u.K = NB;
        u.alpha = -1.0; u.beta = 1.0; u.lower = 1; u.unit_diag_from = -1; u.done = done;
        if (!la) {
            // one stream (batched mode, small handles): panel and update are BOTH on the dependent chain of the step.  With few
            // trailing blocks the chip is empty anyway: narrower tiles (32-row panel strips on 8 waves / 64 x 64 update tiles) are
            // latency-shorter kernels -- ss_small_blocks = trailing blocks up to which they are used (IPM_SS_SMALL_TILES)
            if (rem <= h->ss_small_blocks * NB) {
                HIP_TRY(h, (launch_gemm_nt<32, 128, 32, 1, 8>(t, sm)));
                HIP_TRY(h, (launch_gemm_nt<64, 64, 16, 2, 2>(u, sm)));
                continue;
            }
            HIP_TRY(h, (launch_gemm_nt<64, 128, 16, 2, 2>(t, sm)));
            if (h->bulk_variant == 7) HIP_TRY(h, (launch_gemm_nt<128, 128, 16, 2, 2>(u, sm)));
            else HIP_TRY(h, launch_chol_update(u, sm));
            continue;
        }
        // one event per step on the main stream (after the critical panel rows): every extra record / wait
        // costs the pivot chain ~6-12 us of command-processor time (profiles/, trace of a step)
        GemmNT tc = t; tc.M = NB;                                   // critical panel rows: block row k+1
        if (k >= 1) {     // the previous bulk update either signalled a counter (small grids) or recorded an event
            if (bulk_wgs[k - 1] > 0) { tc.wait_on = h->d_bulk_done + (k - 1); tc.wait_count = bulk_wgs[k - 1]; tc.timeout = h->d_flags + 2 * (size_t)h->nblk; }
            else HIP_TRY(h, hipStreamWaitEvent(sm, h->ev_bulk[k - 1], 0));
        }
        // bulk side: the (small) panel launch of the bulk stream polls the completion counter of the critical
        // panel launch instead of a stream event, unless it is large enough to crowd the CUs while it spins
        const int tb_wgs = (rem - NB) / 64;
        // SAFETY: a polling launch holds LDS on every CU it lands on; potrf_diag needs a CU with 133 KB free and
        // sits upstream of the signal, so a wide poller deadlocks the chain until its spin bound expires
        // (observed at m = 16384 with 254 pollers).  Only launches that leave most CUs untouched may poll.
        const bool crit_flag = fs && rem > NB && tb_wgs <= 64;
        if (crit_flag) tc.signal = h->d_bulk_done + h->nblk + k;
        // NOTE the panel solve is IN PLACE (C = P): a workgroup must own whole rows, i.e. BN == N == 128.  Tiles narrower
        // than the panel (tried: 16 workgroups of 32 x 32) race -- one workgroup overwrites columns another still reads.
        HIP_TRY(h, (launch_gemm_nt<32, 128, 32, 1, 8>(tc, sm)));     // 8 waves, BK=32: 4 stages
        if (!crit_flag) HIP_TRY(h, hipEventRecord(h->ev_crit[k], sm));
        // Two-level blocking (dense handles): the steps come in groups of `gs` block columns.  A step updates only the
        // remaining columns of its group (a window of K = 128 tiles) and DEFERS the rest of its trailing update; the last
        // step of the group applies all of them at once with K = 128 gs -- the group's panels are adjacent block columns
        // of L, i.e. one k-contiguous operand -- so the trailing matrix, whose read-modify-write is what bounds a
        // K = 128 update (16 flop/byte), is streamed once per group instead of once per step.
        const int g0 = grp_lo[k], gend = grp_hi[k];                  // group = block columns [g0, gend)
        const bool grouped = gend - g0 > 1;
        const bool grp_inner = grouped && k + 1 < gend;             // not the last column of its group: window only
        const bool grp_last = grouped && !grp_inner;
        if (grp_last && k > g0) {                                   // operands: block columns g0..k, rows >= k+1
            u.P = panel - (int64_t)(k - g0) * NB; u.Q = u.P; u.K = (k - g0 + 1) * NB;
        }
        GemmNT uc = u; uc.M = NB; uc.N = NB;                        // critical tile (k+1,k+1)
        HIP_TRY(h, (launch_gemm_nt<32, 32, 32, 2, 2>(uc, sm)));      // 10 sub-tiles of 32x32
        if (!crit_flag) HIP_TRY(h, hipStreamWaitEvent(sb, h->ev_crit[k], 0));
        if (rem > NB) {
            GemmNT tb = t; tb.C = panel + (int64_t)NB * h->mp; tb.P = tb.C; tb.M = rem - NB;
            if (crit_flag) { tb.wait_on = h->d_bulk_done + h->nblk + k; tb.wait_count = NB / 32; tb.timeout = h->d_flags + 2 * (size_t)h->nblk; }   // workgroups of the critical panel launch
            HIP_TRY(h, (launch_gemm_nt<64, 128, 16, 2, 2>(tb, sb)));
            GemmNT ub = u;
            const int nt = rem / NB;
            if (grp_inner) {
                // window: tiles (i, j), i >= k+2, k+1 <= j < gend:  B(i,j) -= L(i,k) L(j,k)^T as ONE rectangular GEMM.
                // Inside the group it also touches a few tiles above the diagonal (i < j), which nobody reads.
                const int wn = gend - (k + 1);
                ub.P = panel + (int64_t)NB * h->mp; ub.Q = panel;
                ub.C = h->B + (int64_t)(k + 2) * NB * h->mp + (int64_t)(k + 1) * NB;
                ub.M = rem - NB; ub.N = std::min(wn * NB, rem); ub.lower = 0;
                if (fs) { bulk_wgs[k] = (unsigned)((ub.M / NB) * (ub.N / NB)); ub.signal = h->d_bulk_done + k; ++h->n_counter_steps; }
                else ++h->n_event_steps;
                if (h->bulk_variant == 7) HIP_TRY(h, (launch_gemm_nt<128, 128, 16, 2, 2>(ub, sb)));
                else HIP_TRY(h, launch_chol_update(ub, sb));
                HIP_TRY(h, hipEventRecord(h->ev_bulk[k], sb));
                continue;
            }
            const int ub_wgs = nt * (nt + 1) / 2 - 1;
            // the per-workgroup release (L2 write-back) of the counter protocol only pays in the latency-bound
            // regime; a throughput-bound update (thousands of tiles: 16k: 40 -> 50 ms) keeps the stream event
            if (fs && ub_wgs <= 1024) {
                bulk_wgs[k] = (unsigned)ub_wgs;
                ub.signal = h->d_bulk_done + k;
                ++h->n_counter_steps;
            } else ++h->n_event_steps;
            if (h->bulk_variant == 7) HIP_TRY(h, (launch_gemm_nt<128, 128, 16, 2, 2>(ub, sb, nullptr, 512, /*skip_first=*/1)));   // the generic kernel (rounds 1-2)
            else HIP_TRY(h, launch_chol_update(ub, sb, /*skip_first=*/1));
        }
        HIP_TRY(h, hipEventRecord(h->ev_bulk[k], sb));
    }
    if (la) HIP_TRY(h, hipStreamWaitEvent(sm, h->ev_bulk[h->nblk - 2], 0));
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// ------------------------------------------------------------------------------- fused formation + factorization
// Can this iteration run the fused path?  (mirrors the `fs` rule of enqueue_factor: device-polled hand-offs need the
// device to themselves; a recovered poll time-out clears flag_sync and with it this path, for good)
static bool ff_ok(const ipm_handle* h) {
    if (!h->ff_enabled || h->sparse || h->lookahead == 0 || h->stream2 == nullptr || h->flag_sync == 0) return false;
    if (h->nblk < h->ff_min_nblk || h->nblk > std::min(h->ff_max_nblk, FF_MAX_NBLK) || h->np % FF_PBK) return false;
    if (!h->ff_forced && h->np > 6 * h->mp) return false;
    return h->device >= MAX_DEVICES || g_live[h->device].load(std::memory_order_acquire) <= 1;
}

// schedule + device buffers, once per handle
static int ff_build(ipm_handle* h) {
    if (h->ff_built) return IPM_OK;
    {
        // the work list, its calibration and the one-workgroup-per-CU launch are those of a whole MI355X (gfx950, 256 CUs): on any other
        // device (another part, a partition) the handle keeps the serial path unless the fused one is forced (IPM_FUSED_FACTOR=force)
        hipDeviceProp_t prop;
        HIP_TRY(h, hipGetDeviceProperties(&prop, h->device));
        if (!h->ff_forced && (strncmp(prop.gcnArchName, "gfx950", 6) != 0 || prop.multiProcessorCount != 256))
            return fail(h, IPM_ERR_STATE, "fused factor: built for a 256-CU gfx950 device (this one: %s, %d CUs)", prop.gcnArchName, prop.multiProcessorCount);
    }
    if (h->ff_workers <= 0) {
        hipDeviceProp_t prop;
        HIP_TRY(h, hipGetDeviceProperties(&prop, h->device));
        // ONE launch of as many workgroups as there are CUs (dealt evenly whatever the dispatcher's rotation); the chain and the four
        // strips of its critical products are roles of that launch, everybody else works
        h->ff_workers = std::max(8, prop.multiProcessorCount - 1 - FF_CRIT_WGS);
    }
    const int nstages = (int)(h->np / FF_PBK);               // BK = 16 stages of the pair engine
    const int Q = std::max(1, std::min(h->ff_q, nstages));
    h->ff_q = Q;
    FFModel M;
    M.nstages = nstages;
    ff_build_schedule(h->nblk, Q, h->ff_workers, M, h->ff_sched, std::max(Q, std::min(16, nstages)));
    h->ff_qmax = 1;                                           // slab capacity per tile = the most chunks any tile is formed in
    for (int q_ : h->ff_sched.tile_q) h->ff_qmax = std::max(h->ff_qmax, q_);
    if (nstages > 65535) return fail(h, IPM_ERR_INVALID_ARG, "fused factor: %d formation stages exceed the 16-bit stage range of a work item", nstages);
    const size_t ntile = (size_t)h->nblk * (h->nblk + 1) / 2;
    {   // every tile complete?  (an incomplete list would be an internal error of the scheduler, never a reason to hang a GPU)
        std::vector<int> fcnt(ntile, 0), base(ntile, 0), applied(ntile, 0), paneled(ntile, 0);
        for (const FFItem& it : h->ff_sched.items) {
            const size_t t = (size_t)ff_tile(it.i, it.c);
            if (it.type == FF_D) continue;
            if (it.type == FF_F) {
                if (it.c <= it.i) fcnt[t]++;
                if (it.i + 1 < h->nblk) fcnt[(size_t)ff_tile(it.i + 1, it.c)]++;
                continue;
            }
            if (it.t.j0 != applied[t]) return fail(h, IPM_ERR_INVALID_ARG, "fused factor: internal error (column order of tile %d,%d)", it.i, it.c);
            applied[t] = it.t.j1;
            if (it.t.flags & FF_ADD_BASE) base[t]++;
            if (it.t.flags & FF_PANEL) paneled[t]++;
        }
        for (int i = 0; i < h->nblk; ++i)
            for (int c = 0; c <= i; ++c) {
                const size_t t = (size_t)ff_tile(i, c);
                if (fcnt[t] != h->ff_sched.tile_q[t] || base[t] != 1 || applied[t] != ff_limit(i, c) || paneled[t] != (ff_needs_panel(i, c) ? 1 : 0))
                    return fail(h, IPM_ERR_INVALID_ARG, "fused factor: internal error (tile %d,%d incomplete in the work list)", i, c);
            }
    }
    const size_t nit = h->ff_sched.items.size();
    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->d_ff_items, sizeof(FFItem) * nit));
    HIP_TRY(h, hipMemcpyAsync(h->d_ff_items, h->ff_sched.items.data(), sizeof(FFItem) * nit, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->d_ff_tile_items, sizeof(int) * 2 * ntile));
    HIP_TRY(h, hipMemcpyAsync(h->d_ff_tile_items, h->ff_sched.tile_items.data(), sizeof(int) * ntile, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_ff_tile_items + ntile, h->ff_sched.tile_q.data(), sizeof(int) * ntile, hipMemcpyHostToDevice, h->stream));
    h->ff_flag_words = 32 + 2 * ntile + 3 * (size_t)h->nblk;
    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->d_ff_flags, sizeof(unsigned) * 2 * h->ff_flag_words));     // live words + diagnostic snapshot
    HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->ff_slab, sizeof(double) * ntile * (size_t)h->ff_qmax * 128 * 128));
    if (getenv("IPM_FF_PROF")) {
        HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->ff_prof, sizeof(long long) * 16 * ((size_t)h->ff_workers + 1)));
        HIP_TRY(h, hipMemsetAsync(h->ff_prof, 0, sizeof(long long) * 16 * ((size_t)h->ff_workers + 1), h->stream));
    }
    if (getenv("IPM_FF_TRACE_ITEMS")) {
        const size_t words = 4 * nit + 12 * (size_t)h->nblk;
        HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&h->ff_trace, sizeof(long long) * words));
        HIP_TRY(h, hipMemsetAsync(h->ff_trace, 0, sizeof(long long) * words, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->ff_built = true;
    return IPM_OK;
}

// ff_ok and the schedule + buffers are there.  A failure of ff_build (an allocation, an internal check) is not an error of the
// solve: what was allocated is freed, the handle stops using the fused launch and the iteration runs formation then factorization.
static void ff_release(ipm_handle* h) {
    for (void** p : {(void**)&h->d_ff_items, (void**)&h->d_ff_flags, (void**)&h->ff_slab, (void**)&h->ff_prof, (void**)&h->ff_trace,
                     (void**)&h->d_ff_tile_items}) { dev_free(h->device, h->stream, *p); *p = nullptr; }
    h->ff_built = false;
}
static bool ff_use(ipm_handle* h) {
    if (!ff_ok(h)) return false;
    if (h->ff_built) return true;
    if (ff_build(h) == IPM_OK) return true;
    ff_release(h);
    h->ff_enabled = 0;
    (void)hipGetLastError();
    return false;
}

// The one persistent launch on the main stream: the pivot chain (one workgroup), the four strips of its critical products and the
// workers (formation chunks, max diag(B), every update / panel solve outside the chain) are roles of it, coupled through device
// counters only.  Behind it, on the residual stream, a gate on the chain's progress and what may run from that step on.
// `ev` (optional): ev[1] / ev[2] bracket the launch.
static int enqueue_form_factor(ipm_handle* h, hipEvent_t* ev, int mid_step, int ginv_step) {
    if (!h->ff_built) return fail(h, IPM_ERR_STATE, "fused factor: schedule not built");
    const int nblk = h->nblk;
    const size_t ntile = (size_t)nblk * (nblk + 1) / 2;
    const int* done = h->fdone ? h->fdone : &h->sc->done;
    hipStream_t sw = h->stream;
    unsigned* F = h->d_ff_flags;                               // (layout at the field: tools/ff_debug.py decodes by offset)
    unsigned *ticket = F, *dbg = F + 24, *fcount = F + 32, *tprog = fcount + ntile, *lfinal = tprog + ntile, *dready = lfinal + nblk,
             *potrfdone = dready + nblk;
    unsigned* timeout = h->d_flags + 2 * (size_t)nblk;
    h->ff_potrfdone = potrfdone;                               // (the gate of the last group's inverses polls its last word: enqueue_iteration)
    HIP_TRY(h, hipMemsetAsync(F, 0, sizeof(unsigned) * h->ff_flag_words, sw));
    HIP_TRY(h, hipEventRecord(h->ev_fork, sw));
    long long* ctrace = h->ff_trace ? h->ff_trace + 4 * h->ff_sched.items.size() : nullptr;
    // the pivot chain and its two small products are ROLES of the launch (claimed by arrival); max diag(B) comes from the FF_D
    // items at the head of the work list
    FFRoles roles;
    memset(&roles, 0, sizeof roles);
    FFChain& c = roles.chain;
    c.B = h->B; c.ldb = h->mp; c.invD = h->invD;
    c.maxbits = (const unsigned long long*)(F + 8); c.dcount = F + 10; c.maxdiag_out = &h->sc->maxdiag;
    c.dready = dready; c.potrfdone = potrfdone; c.timeout = timeout; c.dbg = dbg; c.trace = ctrace;
    c.eps = h->opt.pivot_guard_eps; c.big = h->opt.pivot_guard_big; c.shift_rel = h->shift_rel;
    c.fixed = &h->sc->fixed; c.done = done; c.nblk = nblk; c.m = (int)h->m;
    FFCrit& cc = roles.crit;
    cc.B = h->B; cc.ldb = h->mp; cc.invD = h->invD; cc.tprog = tprog; cc.tile_items = h->d_ff_tile_items;
    cc.potrfdone = potrfdone; cc.lfinal = lfinal; cc.dready = dready; cc.timeout = timeout; cc.dbg = dbg; cc.trace = ctrace;
    cc.done = done; cc.nblk = nblk;
    roles.role = F + 3;
    FFArgs a;
    memset(&a, 0, sizeof a);
    a.A = h->A; a.lda = h->np; a.d = h->d; a.B = h->B; a.ldb = h->mp; a.invD = h->invD; a.slab = h->ff_slab;
    a.items = h->d_ff_items; a.nitems = (int)h->ff_sched.items.size();
    a.ticket = ticket; a.fcount = fcount; a.tprog = tprog; a.lfinal = lfinal; a.dready = dready; a.potrfdone = potrfdone;
    a.timeout = timeout; a.dbg = dbg; a.done = done;
    { static const bool dbg_on = getenv("IPM_FF_DEBUG") != nullptr; a.dbg_words = dbg_on ? (unsigned)h->ff_flag_words : 0u; }
    a.trace = h->ff_trace;
    a.prof = h->ff_prof;
    a.tile_q = h->d_ff_tile_items + ntile;
    a.maxbits = (unsigned long long*)(F + 8); a.dcount = F + 10;
    a.nblk = nblk; a.Q = h->ff_qmax; a.nstages = (int)(h->np / FF_PBK); a.m = (int)h->m;
    if (ev) HIP_TRY(h, hipEventRecord(ev[1], sw));
    {
        const dim3 grid((unsigned)h->ff_workers + 1u + (unsigned)FF_CRIT_WGS);
        const bool instr = a.prof || a.trace;
        if (h->ff_ref_engine) {
            if (instr) hipLaunchKernelGGL((form_factor_roles_kernel<true>), grid, dim3(FF_THREADS), 0, sw, a, roles);
            else hipLaunchKernelGGL((form_factor_roles_kernel<false>), grid, dim3(FF_THREADS), 0, sw, a, roles);
        } else if (instr) {
            hipLaunchKernelGGL((form_factor_roles_kernel_mfma_first<true>), grid, dim3(FF_THREADS), 0, sw, a, roles);
        } else {
            hipLaunchKernelGGL((form_factor_roles_kernel_mfma_first<false>), grid, dim3(FF_THREADS), 0, sw, a, roles);
        }
    }
    if (ev) HIP_TRY(h, hipEventRecord(ev[2], sw));
    HIP_TRY(h, hipGetLastError());
    h->n_counter_steps = nblk; h->n_event_steps = 0; h->last_gs = 1;
    // Everything the residual stream does -- the inverses of the complete 1024-row groups, r_b, r_c, the stop test, the
    // predictor's right-hand side -- sits behind a GATE that opens when the chain has factored block `gate_step`: no stream
    // event can mark a point inside the persistent launch, and every CU is taken until the workers leave, which they do from
    // about that step on (all items drawn).  Enqueued after the launch; ev_res joins it into the main stream as before.
    const int gate_step = ginv_step >= 0 ? ginv_step : mid_step;
    if (gate_step >= 0) {
        HIP_TRY(h, hipStreamWaitEvent(h->stream3, h->ev_fork, 0));            // (the hand-off words are zeroed)
        hipLaunchKernelGGL(ff_gate_kernel, dim3(1), dim3(64), 0, h->stream3, potrfdone + gate_step, 1u, timeout, done);
        if (ginv_step >= 0) { int rc_ = enqueue_group_inverses(h, 0, (ginv_step + 1) / h->gsz, h->stream3); if (rc_) return rc_; }
        if (mid_step >= 0) {
            int rc_ = enqueue_residuals(h, h->stream3);
            if (rc_) return rc_;
            launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1, h->stream3);   // predictor rhs = -r_b - A (d*t)
            HIP_TRY(h, hipEventRecord(h->ev_res, h->stream3));
        }
    }
    HIP_TRY(h, hipGetLastError());
    h->ff_last = true;
    return IPM_OK;
}

extern "C" int ipm_debug_ff_schedule(int32_t nblk, int32_t q, int32_t workers, unsigned char* items, int32_t capacity, int32_t* count,
                                     int32_t* tile_items, double sim_us[2]) {
    if (nblk < 1 || nblk > FF_MAX_NBLK || q < 1 || q > 16 || workers < 1 || !count) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_debug_ff_schedule: bad arguments");
    static_assert(sizeof(FFItem) == 8, "work item layout");
    FFSchedule S;
    if (const char* e = getenv("IPM_FF_CHAIN_MODE")) if (atoi(e) == 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "IPM_FF_CHAIN_MODE=0 is not supported (that structure of the fused launch was removed)");     // as ipm_create
    FFModel M;
    M.nstages = 512;                                          // K = 8192 (the headline size's formation), BK = 16 stages
    ff_build_schedule(nblk, q, workers, M, S, std::max(q, 16));
    *count = (int32_t)S.items.size();
    if (items) memcpy(items, S.items.data(), sizeof(FFItem) * std::min<size_t>(S.items.size(), (size_t)std::max(0, capacity)));
    if (tile_items) for (size_t t = 0; t < S.tile_items.size(); ++t) tile_items[t] = S.tile_items[t];
    if (sim_us) { sim_us[0] = S.makespan_us; sim_us[1] = S.form_end_us; }
    return IPM_OK;
}

extern "C" int ipm_debug_get_block_inverse(ipm_handle* h, int32_t k, double* out) {
    if (!h || !out || k < 0 || k >= h->nblk) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_get_block_inverse: bad arguments");
    if (!h->invD) return fail(h, IPM_ERR_STATE, "the handle holds no dense factor");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, h->invD + (int64_t)k * NB * NB, sizeof(double) * NB * NB, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return IPM_OK;
}

extern "C" int ipm_debug_ff_trace(ipm_handle* h, long long* out, int64_t capacity, int64_t* count, unsigned char* items, int32_t* nitems) {
    if (!h || !count) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_ff_trace: bad arguments");
    if (!h->ff_trace || !h->ff_built) return fail(h, IPM_ERR_STATE, "no item trace (IPM_FF_TRACE_ITEMS=1 at ipm_create, fused path)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nit = h->ff_sched.items.size(), words = 4 * nit + 12 * (size_t)h->nblk;
    *count = (int64_t)words;
    if (nitems) *nitems = (int32_t)nit;
    if (out && capacity >= (int64_t)words) {
        HIP_TRY(h, hipMemcpyAsync(out, h->ff_trace, sizeof(long long) * words, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (items) memcpy(items, h->ff_sched.items.data(), sizeof(FFItem) * nit);
    return IPM_OK;
}

// X_g, XT_g = inv of every 1024 x 1024 diagonal group of the factor and its transpose (trsv_grouped.h):
// recursive doubling 128 -> 256 -> 512 -> 1024, three GEMMs per level batched over (pairs in a group,
// groups).  After enqueue_factor, on the main stream.
static int enqueue_group_inverses(ipm_handle* h, int g0 = 0, int g1 = -1, hipStream_t st = nullptr) {
    if (sp_on(h)) return IPM_OK;
    if (!h->grouped_trsv) return IPM_OK;
    const int GS = h->gsz;
    const int64_t GR = (int64_t)GS * 128;
    if (g1 < 0) g1 = h->nblk / GS;
    if (!st) st = h->stream;
    const int nG = g1 - g0;                               // groups [g0, g1)
    if (nG <= 0) return IPM_OK;
    const int* done = &h->sc->done;
    if (!ls_push(h, LS_GROUP_DIAG_T, 16u * (unsigned)(nG * GS), LsGroupDiagT{h->invD, h->gXT, h->gX, g0 * GS, GS, done}))
        hipLaunchKernelGGL(group_diag_transpose_kernel, dim3(4, 4, nG * GS), dim3(32, 8), 0, st, h->invD, h->gXT, h->gX, g0 * GS, GS, done);
    const int64_t gXs = GR * GR, gL = GR * (h->mp + 1), gSs = (GR / 2) * (GR / 2);   // group strides in X/XT, L, S
    double* gXT = h->gXT + g0 * gXs; double* gX = h->gX + g0 * gXs; double* gS = h->gS + g0 * gSs;
    const double* Lg = h->B + g0 * gL;
    for (int hs = 128; hs < GR; hs *= 2) {
        const int np = (int)(GR / (2 * hs));              // pairs per group
        GemmNT t = gemm_defaults();
        t.tile_order = nullptr; t.w = nullptr; t.done = done; t.lower = 0; t.unit_diag_from = -1;
        t.M = hs; t.N = hs; t.K = hs; t.beta = 0.0; t.batch = np; t.batch2 = nG;
        const int64_t pX = (int64_t)2 * hs * (GR + 1);                                 // pair strides in X, XT
        const int64_t pL = (int64_t)2 * hs * (h->mp + 1);
        const int64_t pS = (int64_t)hs * hs;
        GemmNT a = t;                                     // S = XT11 * L21^T
        a.P = gXT; a.ldp = GR; a.sP = pX; a.sP2 = gXs;
        a.Q = Lg + (int64_t)hs * h->mp; a.ldq = h->mp; a.sQ = pL; a.sQ2 = gL;
        a.C = gS; a.ldc = hs; a.sC = pS; a.sC2 = gSs; a.alpha = 1.0;
        HIP_TRY(h, (launch_gemm_nt<32, 32, 32, 2, 2>(a, st)));      // 32 x 32 tiles (4x the workgroups of 64 x 64: 0.17 -> 0.12 ms)
        GemmNT b = t;                                     // X21 = -X22 * S^T
        b.P = gX + (int64_t)hs * GR + hs; b.ldp = GR; b.sP = pX; b.sP2 = gXs;
        b.Q = gS; b.ldq = hs; b.sQ = pS; b.sQ2 = gSs;
        b.C = gX + (int64_t)hs * GR; b.ldc = GR; b.sC = pX; b.sC2 = gXs; b.alpha = -1.0;
        HIP_TRY(h, (launch_gemm_nt<32, 32, 32, 2, 2>(b, st)));
        GemmNT c = t;                                     // XT12 = -S * X22^T
        c.P = gS; c.ldp = hs; c.sP = pS; c.sP2 = gSs;
        c.Q = gX + (int64_t)hs * GR + hs; c.ldq = GR; c.sQ = pX; c.sQ2 = gXs;
        c.C = gXT + hs; c.ldc = GR; c.sC = pX; c.sC2 = gXs; c.alpha = -1.0;
        HIP_TRY(h, (launch_gemm_nt<32, 32, 32, 2, 2>(c, st)));
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

static void launch_dense_gemv_n(ipm_handle* h, const double* A, int64_t lda, int rows, int cols, const double* v, double sa,
                                double sb, const double* add, double* out) {
    if (ls_push(h, LS_GEMV_N, (unsigned)((rows + 3) / 4), LsGemvN{A, lda, rows, cols, v, sa, sb, add, out, &h->sc->done})) return;
    hipLaunchKernelGGL(gemv_n_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, h->stream, A, lda, rows, cols, v, sa, sb,
                       add, out, &h->sc->done);
}

// out = B^{-1} r with the 1024-row group inverses: 4 group steps per sweep at m = 4096
// wait_last (optional): event after which the LAST group's inverse is available; the forward sweep over the earlier groups
// does not need it and runs ahead of the wait
static int enqueue_potrs_grouped(ipm_handle* h, double* r, double* out, hipEvent_t wait_last = nullptr) {
    const int GS = h->gsz;
    const int GR = GS * 128;
    const int nG = h->nblk / GS;
    const int* done = &h->sc->done;
    double* z = h->t2;
    for (int g = 0; g < nG; ++g) {                                        // forward: L z = r
        if (wait_last && g == nG - 1) HIP_TRY(h, hipStreamWaitEvent(h->stream, wait_last, 0));
        launch_dense_gemv_n(h, h->gX + (int64_t)g * GR * GR, GR, GR, GR, r + (int64_t)g * GR, 1.0, 0.0, nullptr, z + (int64_t)g * GR);
        int below = (int)(h->mp - (int64_t)(g + 1) * GR);
        if (h->use_env) below = std::min(below, (int)((int64_t)(h->env_last[(g + 1) * GS - 1] + 1) * NB - (int64_t)(g + 1) * GR));
        if (below > 0) {
            double* rb = r + (int64_t)(g + 1) * GR;
            launch_dense_gemv_n(h, h->B + (int64_t)(g + 1) * GR * h->mp + (int64_t)g * GR, h->mp, below, GR, z + (int64_t)g * GR, -1.0, 1.0,
                                rb, rb);
        }
    }
    // blocks behind the last full group (ragged groups): one launch per block step, as without groups
    const int k_left = nG * GS;
    if (k_left < h->nblk) {
        TrsvStep a;
        a.L = h->B; a.ld = h->mp; a.inv = h->invD; a.done = done;
        a.r = r; a.z = z; a.j0 = 0;
        for (int k = k_left; k < h->nblk; ++k) {
            a.k = k;
            const int nb = h->use_env ? h->env_last[k] - k + 1 : h->nblk - k;
            if (!ls_push(h, LS_TRSV_FWD, (unsigned)nb, a)) hipLaunchKernelGGL(trsv_fwd_step_kernel, dim3(nb), dim3(256), 0, h->stream, a);
        }
        a.r = z; a.z = out;
        for (int k = h->nblk - 1; k >= k_left; --k) {
            a.k = k;
            a.j0 = h->use_env ? h->env_first[k] : 0;
            if (!ls_push(h, LS_TRSV_BWD, (unsigned)(k - a.j0 + 1), a)) hipLaunchKernelGGL(trsv_bwd_step_kernel, dim3(k - a.j0 + 1), dim3(256), 0, h->stream, a);
        }
    }
    for (int g = nG - 1; g >= 0; --g) {                                   // backward: L^T w = z
        launch_dense_gemv_n(h, h->gXT + (int64_t)g * GR * GR, GR, GR, GR, z + (int64_t)g * GR, 1.0, 0.0, nullptr, out + (int64_t)g * GR);
        int left = g * GR;
        const int c0 = h->use_env ? std::min(left, h->env_first[g * GS] * NB) : 0;   // columns left of c0 are zero in these rows
        left -= c0;
        if (left > 0) {
            dim3 grid((unsigned)((left + 511) / 512), 16);
            if (!ls_push(h, LS_GEMV_T, grid.x * 16u, LsGemvT{h->B + (int64_t)g * GR * h->mp + c0, h->mp, GR / 16, left, out + (int64_t)g * GR, h->gPart, done, grid.x}))
                hipLaunchKernelGGL(gemv_t_kernel, grid, dim3(256), 0, h->stream, h->B + (int64_t)g * GR * h->mp + c0, h->mp, GR / 16, left,
                                   out + (int64_t)g * GR, h->gPart, done);
            if (!ls_push(h, LS_SUB_PARTIALS, (unsigned)((left + 255) / 256), LsSubPart{z + c0, h->gPart, left, 16, done}))
                hipLaunchKernelGGL(sub_partials_kernel, dim3((unsigned)((left + 255) / 256)), dim3(256), 0, h->stream, z + c0, h->gPart, left, 16, done);
        }
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// out = B^{-1} r  (r is consumed; uses t2 as the intermediate)
static int enqueue_potrs(ipm_handle* h, double* r, double* out, hipEvent_t wait_last = nullptr) {
    if (sp_on(h)) {                     // forward and backward sweep over the elimination tree, one launch each
        const int rm = std::max(16, h->sp_rmax);
#define SP_LAUNCH_FWD(NT, SC, GRID, RECS, COUNT) \
    hipLaunchKernelGGL((sp_fwd_kernel<NT, SC>), dim3(GRID), dim3(NT), h->sp_lds_solve, h->stream, h->spF, ep, r, h->t2, rm, RECS, COUNT)
#define SP_LAUNCH_BWD(NT, SC, GRID, RECS, COUNT) \
    hipLaunchKernelGGL((sp_bwd_kernel<NT, SC>), dim3(GRID), dim3(NT), 0, h->stream, h->spF, ep, h->t2, out, RECS, COUNT)
#define SP_SWEEP(WHICH, GRID, RECS, COUNT)                                                                                            \
    do {                                                                                                                             \
        WHICH(SPC_THREADS, false, GRID, RECS, COUNT);                                                                                \
    } while (0)
        unsigned ep = ++h->sp_epoch;
        const size_t nlev = h->sp_lvlptr.size() > 0 ? h->sp_lvlptr.size() - 1 : 0;
        const bool fwd_done = h->sp_fwd_fused != nullptr && h->sp_fwd_fused == r;       // the factorization carried L z = r already (z in t2)
        h->sp_fwd_fused = nullptr;
        if (sp_level(h)) {
            for (size_t l = 0; l < nlev && !fwd_done; ++l) {
                const int cnt = h->sp_lvlptr[l + 1] - h->sp_lvlptr[l];
                SP_SWEEP(SP_LAUNCH_FWD, (unsigned)std::min(cnt, h->sp_grid), h->sp_rec_level + h->sp_lvlptr[l], cnt);
            }
            for (size_t l = nlev; l-- > 0;) {
                const int cnt = h->sp_lvlptr[l + 1] - h->sp_lvlptr[l];
                SP_SWEEP(SP_LAUNCH_BWD, (unsigned)std::min(cnt, h->sp_grid), h->sp_rec_level + h->sp_lvlptr[l], cnt);
            }
        } else {
            if (!fwd_done) SP_SWEEP(SP_LAUNCH_FWD, sp_launch_grid(h), h->spF.rec, 0);
            ep = ++h->sp_epoch;
            SP_SWEEP(SP_LAUNCH_BWD, sp_launch_grid(h), h->spF.rec, 0);
        }
#undef SP_SWEEP
#undef SP_LAUNCH_FWD
#undef SP_LAUNCH_BWD
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    if (h->grouped_trsv) return enqueue_potrs_grouped(h, r, out, wait_last);
    if (wait_last) HIP_TRY(h, hipStreamWaitEvent(h->stream, wait_last, 0));
    TrsvStep a;
    a.L = h->B; a.ld = h->mp; a.inv = h->invD; a.done = &h->sc->done;
    a.r = r; a.z = h->t2;
    a.j0 = 0;
    for (int k = 0; k < h->nblk; ++k) {
        a.k = k;
        const int nb = h->use_env ? h->env_last[k] - k + 1 : h->nblk - k;
        if (!ls_push(h, LS_TRSV_FWD, (unsigned)nb, a)) hipLaunchKernelGGL(trsv_fwd_step_kernel, dim3(nb), dim3(256), 0, h->stream, a);
    }
    a.r = h->t2; a.z = out;
    for (int k = h->nblk - 1; k >= 0; --k) {
        a.k = k;
        a.j0 = h->use_env ? h->env_first[k] : 0;
        if (!ls_push(h, LS_TRSV_BWD, (unsigned)(k - a.j0 + 1), a)) hipLaunchKernelGGL(trsv_bwd_step_kernel, dim3(k - a.j0 + 1), dim3(256), 0, h->stream, a);
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

static int enqueue_predictor(ipm_handle* h, hipEvent_t* ev, bool have_rhs = false, hipEvent_t wait_last = nullptr) {
    VecArgs a = vec_args(h);
    if (!have_rhs) launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1);   // rhs = -r_b - A (d*t)
    if (ev) HIP_TRY(h, hipEventRecord(ev[0], h->stream));
    int rc = enqueue_potrs(h, h->t1, h->dya, wait_last);
    if (rc) return rc;
    if (ev) HIP_TRY(h, hipEventRecord(ev[1], h->stream));
    launch_gemv_t(h, h->dya);
    if (h->bnd) hipLaunchKernelGGL(direction_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, 0, bnd_args(h));
    else if (!ls_push(h, LS_DIRECTION, (unsigned)h->vblk, LsVecA{a, 0})) hipLaunchKernelGGL(direction_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, 0);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

static int enqueue_corrector(ipm_handle* h, hipEvent_t* ev) {
    VecArgs a = vec_args(h);
    if (h->bnd) {
        hipLaunchKernelGGL(mu_aff_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, bnd_args(h));
        hipLaunchKernelGGL(corrector_rhs_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, bnd_args(h));
    } else {
        if (!ls_push(h, LS_MU_AFF, (unsigned)h->vblk, LsVecA{a, 0})) hipLaunchKernelGGL(mu_aff_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a);
        if (!ls_push(h, LS_CORR_RHS, (unsigned)h->vblk, LsVecA{a, 0})) hipLaunchKernelGGL(corrector_rhs_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a);
    }
    launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1);
    if (ev) HIP_TRY(h, hipEventRecord(ev[0], h->stream));
    int rc = enqueue_potrs(h, h->t1, h->dy);
    if (rc) return rc;
    if (ev) HIP_TRY(h, hipEventRecord(ev[1], h->stream));
    launch_gemv_t(h, h->dy);
    if (h->bnd) hipLaunchKernelGGL(direction_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, 1, bnd_args(h));
    else if (!ls_push(h, LS_DIRECTION, (unsigned)h->vblk, LsVecA{a, 1})) hipLaunchKernelGGL(direction_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, 1);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

static int enqueue_update(ipm_handle* h) {
    VecArgs a = vec_args(h);
    if (h->bnd) hipLaunchKernelGGL(update_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, bnd_args(h));
    else if (!ls_push(h, LS_UPDATE, (unsigned)h->vblk, LsVecA{a, 0})) hipLaunchKernelGGL(update_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// events per profiled iteration: 0 start, 1 before form, 2 after form, 3 after factor,
// 4/5 around predictor solve, 6/7 around corrector solve, 8 end
static const int EV_PER_IT = 9;

static int enqueue_iteration(ipm_handle* h, hipEvent_t* ev) {
    int rc;
    const bool all = ev && h->profiling >= 2;            // each event record costs the stream ~6 us: level 1 keeps two
    if (overlap_residuals(h)) {
        // d = x/s -> formation -> factorization, with the residuals, the stop test and the predictor rhs on the residual
        // stream under the chain-bound tail of the factorization
        VecArgs a = vec_args(h);
        if (h->bnd) hipLaunchKernelGGL(scaling_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, bnd_args(h));
        else hipLaunchKernelGGL(scaling_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a);
        const bool fused = ff_use(h);                        // evaluated ONCE per iteration (the live-handle count can change under it)
        if (ev && !fused) HIP_TRY(h, hipEventRecord(ev[1], h->stream));
        // the stop test of THIS iterate runs on the residual stream while the factorization is in flight: formation and
        // factorization test the latch scaling_kernel took (Scalars::done_f), so they either run whole or not at all and
        // after a converged solve B / invD hold the complete factor of the final iterate (ipm_get_factor, pivots_fixed)
        struct Latch { ipm_handle* h; ~Latch() { h->fdone = nullptr; } } latch{h};
        h->fdone = &h->sc->done_f;
        h->ff_last = false;
        if (!fused) {
            if ((rc = enqueue_form(h, h->d))) return rc;
            if (ev) HIP_TRY(h, hipEventRecord(ev[2], h->stream));
        }
        // start late in the chain-bound tail: the three passes need ~0.2 ms, six steps of the chain.  Measured at 32 blocks
        // (it/s for a start at step 0 / 4 / 12 / 20 / 26 / 30): 199.5 / 199.6 / 200.6 / 201.0 / 203.1 / 200.5
        const int rstep = h->nblk * 13 / 16;
        const int nG = h->grouped_trsv ? h->nblk / h->gsz : 0;
        const int gstep = (nG >= 2 && (nG - 1) * h->gsz - 1 < rstep) ? (nG - 1) * h->gsz - 1 : -1;
        if (fused) { if ((rc = enqueue_form_factor(h, ev, rstep, gstep))) return rc; }
        else if ((rc = enqueue_factor(h, true, rstep, gstep))) return rc;
        h->fdone = nullptr;
        if (gstep >= 0) {
            // the last group's inverse (nine dependent launches, ~80 us) goes to the residual stream as well: the forward
            // sweep of the predictor over the earlier groups runs beside it and only its last step waits
            if (h->ff_last && h->ff_potrfdone) {
                // fused launch: the residual stream does not wait for an EVENT behind the launch (in the kernel trace both streams
                // then resumed 45 us after the launch's last wave: two streams waiting for each other's events) but for the chain's
                // last hand-off word, like the gate of the earlier groups: behind it the whole factor is released at agent scope
                // (every worker's writes through the tile counters the chain acquired), and every kernel of a stream starts with an
                // acquire.  The last group's inverse now starts 2 us after the launch ends, the main stream's sweep 11 us
                // (profiles/r04_dense_iteration_timeline*.txt): 261.3 -> 262.4 it/s.
                hipLaunchKernelGGL(ff_gate_kernel, dim3(1), dim3(64), 0, h->stream3, h->ff_potrfdone + (h->nblk - 1), 1u, h->d_flags + 2 * (size_t)h->nblk, &h->sc->done);
            } else {
                HIP_TRY(h, hipEventRecord(h->ev_grp, h->stream));
                HIP_TRY(h, hipStreamWaitEvent(h->stream3, h->ev_grp, 0));
            }
            if ((rc = enqueue_group_inverses(h, nG - 1, nG, h->stream3))) return rc;
            HIP_TRY(h, hipEventRecord(h->ev_last, h->stream3));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_res, 0));
            if ((rc = enqueue_predictor(h, nullptr, /*have_rhs=*/true, h->ev_last))) return rc;
        } else {
            if ((rc = enqueue_group_inverses(h, 0, nG, nullptr))) return rc;
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_res, 0));
            if ((rc = enqueue_predictor(h, nullptr, /*have_rhs=*/true))) return rc;
        }
        if ((rc = enqueue_corrector(h, nullptr))) return rc;
        if ((rc = enqueue_update(h))) return rc;
        return IPM_OK;
    }
    if (all) HIP_TRY(h, hipEventRecord(ev[0], h->stream));
    if ((rc = enqueue_residuals(h))) return rc;
    h->ff_last = false;
    bool have_rhs = false;
    if (h->profiling < 2 && ff_use(h)) {
        // (handles below 16 blocks have no residual stream: the fused launch is used here only when IPM_FUSED_FACTOR=force
        //  lowers the block limit -- the tests' way to run the fused kernels at small sizes)
        if ((rc = enqueue_form_factor(h, ev, -1, -1))) return rc;
    } else {
        if (ev) HIP_TRY(h, hipEventRecord(ev[1], h->stream));
        if ((rc = enqueue_form(h, h->d))) return rc;
        if (ev) HIP_TRY(h, hipEventRecord(ev[2], h->stream));
        if (sp_on(h) && h->sp_fuse_fwd) {
            // sparse factor: the predictor's right-hand side does not depend on the factor -- form it first and let its forward
            // substitution ride on the factorization (four walks of the elimination tree per iteration instead of five)
            launch_gemv_n(h, h->v, -1.0, -1.0, h->rb, h->t1);   // rhs = -r_b - A (d*t)
            have_rhs = true;
            if ((rc = enqueue_factor(h, true, -1, -1, h->t1))) return rc;
        } else if ((rc = enqueue_factor(h, true))) return rc;
    }
    if ((rc = enqueue_group_inverses(h))) return rc;
    if (all) HIP_TRY(h, hipEventRecord(ev[3], h->stream));
    if ((rc = enqueue_predictor(h, all ? ev + 4 : nullptr, have_rhs))) return rc;
    if ((rc = enqueue_corrector(h, all ? ev + 6 : nullptr))) return rc;
    if ((rc = enqueue_update(h))) return rc;
    if (all) HIP_TRY(h, hipEventRecord(ev[8], h->stream));
    return IPM_OK;
}

// Host copy of the scalar record (one sync).  *timed_out (optional) receives the poll time-out word of the
// device-side hand-offs and the word is cleared; without it a time-out is an error.
static int read_scalars(ipm_handle* h, bool* timed_out = nullptr) {
    unsigned tmo = 0;
    unsigned* word = h->d_flags + 2 * (size_t)h->nblk;
    HIP_TRY(h, hipMemcpyAsync(h->h_sc, h->sc, sizeof(Scalars), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&tmo, word, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (tmo) {
        if (h->stream2) HIP_TRY(h, hipStreamSynchronize(h->stream2));               // the bulk stream may still be draining
        if (h->ff_built && h->ff_last && getenv("IPM_FF_DEBUG")) {
            // diagnostic: where did the fused launch stop?  (hand-off words of the LAST factorization of the call)
            std::vector<unsigned> F(h->ff_flag_words);
            (void)hipMemcpy(F.data(), h->d_ff_flags, sizeof(unsigned) * F.size(), hipMemcpyDeviceToHost);
            if (F[24] && F[26] < 6) {           // a worker wait gave up first: show the snapshot it took instead of the final state
                std::vector<unsigned> S(h->ff_flag_words);
                (void)hipMemcpy(S.data(), h->d_ff_flags + h->ff_flag_words, sizeof(unsigned) * S.size(), hipMemcpyDeviceToHost);
                for (size_t w = 0; w < F.size(); ++w) if (w < 24 || w >= 32) F[w] = S[w];
                fprintf(stderr, "[ff debug] (snapshot taken by the first wait that gave up)\n");
            }
            const int nb = h->nblk; const size_t nt = (size_t)nb * (nb + 1) / 2;
            const unsigned *fc = F.data() + 32, *tp = fc + nt, *lf = tp + nt, *dr = lf + nb, *pd = dr + nb;
            fprintf(stderr, "[ff debug] ticket %u of %zu items; first worker wait that gave up: count %u item %u kind %u target %u seen %u\n", F[0],
                    h->ff_sched.items.size(), F[24], F[25], F[26], F[27], F[28]);
            if (F[24] && F[26] < 6 && F[25] < h->ff_sched.items.size()) {
                const FFItem& it = h->ff_sched.items[F[25]];
                fprintf(stderr, "  that item: T(%d,%d)[%d,%d) flags %d seq %d\n", it.i, it.c, it.t.j0, it.t.j1, it.t.flags, it.t.seq);
            }
            fprintf(stderr, "  potrfdone:");
            for (int k = 0; k < nb; ++k) fprintf(stderr, " %u", pd[k]);
            fprintf(stderr, "\n  dready:");
            for (int k = 0; k < nb; ++k) fprintf(stderr, " %u", dr[k]);
            fprintf(stderr, "\n  lfinal:");
            for (int k = 0; k < nb; ++k) fprintf(stderr, " %u", lf[k]);
            fprintf(stderr, "\n  incomplete tiles (i,c: fcount/expected tprog/expected):");
            int shown = 0;
            for (int i = 0; i < nb; ++i)
                for (int c = 0; c <= i; ++c) {
                    const size_t t = (size_t)ff_tile(i, c);
                    // (a tile's chunk count is its own: IPM_FF_Q_LAST forms the last block rows in other counts than ff_q)
                    if ((fc[t] != (unsigned)h->ff_sched.tile_q[t] || tp[t] != (unsigned)h->ff_sched.tile_items[t]) && shown++ < 24)
                        fprintf(stderr, " (%d,%d: %u/%d %u/%d)", i, c, fc[t], h->ff_sched.tile_q[t], tp[t], h->ff_sched.tile_items[t]);
                }
            fprintf(stderr, "\n");
        }
        HIP_TRY(h, hipMemsetAsync(word, 0, sizeof(unsigned), h->stream));
        if (!timed_out) return fail(h, IPM_ERR_HIP, "a device-side hand-off poll timed out (persistent solve)");
    }
    if (timed_out) *timed_out = tmo != 0;
    return IPM_OK;
}

// A poll time-out means a consumer gave up waiting and computed on stale tiles: the results of the call are
// garbage but nothing hung.  Policy: never surface it -- switch this handle to stream events for good, undo the
// call's effect on the iterate (callers restore their snapshot) and run it again.
static void poll_fallback(ipm_handle* h) {
    if (h->spf) h->sp_serial = true;          // sparse factor: one workgroup per launch from now on (it never waits)
    if (h->ff_last) h->ff_enabled = 0;        // the fused launch timed out: serial formation + factorization from now on, look-ahead kept
    else h->flag_sync = 0;
    ++h->timeouts_recovered;
}

// (x, y, s, Scalars) <-> roll-back buffer, one launch
__global__ __launch_bounds__(256) void snapshot_kernel(double* x, double* y, double* s, Scalars* sc, double* snap, int np,
                                                       int mp, int restore) {
    const int gid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    double *sx = snap, *ss = snap + np, *sy = snap + 2 * (size_t)np;
    Scalars* ssc = (Scalars*)(snap + 2 * (size_t)np + mp);
    if (restore) {
        for (int j = gid; j < np; j += gsz) { x[j] = sx[j]; s[j] = ss[j]; }
        for (int i = gid; i < mp; i += gsz) y[i] = sy[i];
        if (gid == 0) *sc = *ssc;
    } else {
        for (int j = gid; j < np; j += gsz) { sx[j] = x[j]; ss[j] = s[j]; }
        for (int i = gid; i < mp; i += gsz) sy[i] = y[i];
        if (gid == 0) *ssc = *sc;
    }
}
__global__ __launch_bounds__(256) void snapshot_bounds_kernel(double* w, double* z, double* sw, double* sz, int np, int restore) {
    const int gid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    for (int j = gid; j < np; j += gsz) {
        if (restore) { w[j] = sw[j]; z[j] = sz[j]; }
        else { sw[j] = w[j]; sz[j] = z[j]; }
    }
}
static int enqueue_snapshot(ipm_handle* h, int restore, hipStream_t st = nullptr) {
    const int64_t mx = h->np > h->mp ? h->np : h->mp;
    const unsigned grid = (unsigned)std::min<int64_t>((mx + 255) / 256, 256);
    hipLaunchKernelGGL(snapshot_kernel, dim3(grid), dim3(256), 0, st ? st : h->stream, h->x, h->y, h->s, h->sc, h->snap, (int)h->np,
                       (int)h->mp, restore);
    if (h->bnd) {                                              // (w, z) <-> their roll-back copies behind the bound vectors
        const BndArgs b = bnd_args(h);
        double* sw = h->bnd_mem + 8 * (size_t)h->np;
        hipLaunchKernelGGL(snapshot_bounds_kernel, dim3(grid), dim3(256), 0, st ? st : h->stream, b.w, b.z, sw, sw + h->np, (int)h->np, restore);
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}
// can the next factorization time out at all?  (mirrors the `fs` rule of enqueue_factor)
static bool may_poll(const ipm_handle* h) { return (h->spf && !h->sp_serial && !sp_level(h)) || h->lookahead != 0 && h->nblk > 2 && h->stream2 != nullptr && h->flag_sync != 0; }

static void fill_stats(ipm_handle* h, ipm_stats* st, double ms) {
    if (!st) return;
    const Scalars& s = *h->h_sc;
    memset(st, 0, sizeof *st);
    st->status = s.status; st->iterations = s.k; st->pivots_fixed = s.fixed; st->auto_regularized = h->auto_reg;
    st->objective_last_finite = s.obj_last_finite;
    st->objective = s.obj; st->rp_norm = s.rb_norm; st->rd_norm = s.rc_norm; st->gap = s.gap;
    st->b_norm = s.b_norm; st->c_norm = s.c_norm; st->mu = s.mu; st->mu_aff = s.mu_aff; st->sigma = s.sigma;
    st->alpha_aff_p = s.alpha_aff_p; st->alpha_aff_d = s.alpha_aff_d; st->alpha_p = s.alpha_p; st->alpha_d = s.alpha_d;
    st->solve_ms = ms;
}

static int check_ready(ipm_handle* h, const char* who) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (!h->haveA || !h->haveBC || !h->haveState) return fail(h, IPM_ERR_STATE, "%s: A, (b,c) and a state must be set first", who);
    return IPM_OK;
}

// ------------------------------------------------------------------------------- seams
extern "C" int ipm_newton_direction(ipm_handle* h, int corrector, double* dx, double* dy, double* ds, ipm_stats* stats) {
    int rc = check_ready(h, "ipm_newton_direction");
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!corrector) {
        for (int attempt = 0;; ++attempt) {                 // second pass only after a recovered poll time-out
            hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, 0);
            if ((rc = enqueue_residuals(h))) return rc;
            if ((rc = enqueue_form(h, h->d))) return rc;
            if ((rc = enqueue_factor(h, true))) return rc;
            if ((rc = enqueue_group_inverses(h))) return rc;
            if ((rc = enqueue_predictor(h, nullptr))) return rc;
            VecArgs a = vec_args(h);
            if (h->bnd) hipLaunchKernelGGL(mu_aff_bounded_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a, bnd_args(h));
            else hipLaunchKernelGGL(mu_aff_kernel, dim3(h->vblk), dim3(VBLK), 0, h->stream, a);   // alpha_aff for stats
            bool tmo = false;
            if ((rc = read_scalars(h, &tmo))) return rc;
            if (!tmo) break;
            if (attempt) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
            poll_fallback(h);
        }
        h->predictor_valid = true;
        if (dx) HIP_TRY(h, hipMemcpyAsync(dx, h->dxa, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        if (dy) HIP_TRY(h, hipMemcpyAsync(dy, h->dya, sizeof(double) * h->m, hipMemcpyDeviceToHost, h->stream));
        if (ds) HIP_TRY(h, hipMemcpyAsync(ds, h->dsa, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    } else {
        if (!h->predictor_valid) return fail(h, IPM_ERR_STATE, "corrector requested without a predictor at this state");
        if ((rc = enqueue_corrector(h, nullptr))) return rc;
        // alpha_p/alpha_d for stats without moving the iterate: recompute in a 1-thread kernel? they are
        // written by update_kernel only; expose the raw ratio minima through sigma/mu_aff and leave alpha to
        // ipm_iterate.  (The step lengths are checked end-to-end by the iterate tests.)
        if (dx) HIP_TRY(h, hipMemcpyAsync(dx, h->dx, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        if (dy) HIP_TRY(h, hipMemcpyAsync(dy, h->dy, sizeof(double) * h->m, hipMemcpyDeviceToHost, h->stream));
        if (ds) HIP_TRY(h, hipMemcpyAsync(ds, h->ds, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    }
    if (corrector && (rc = read_scalars(h))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    fill_stats(h, stats, 0.0);
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

// whole loop of a small sparse LP in one launch of one workgroup (small_lp.h)
static int enqueue_small(ipm_handle* h, int max_steps, int auto_reg) {
    SmallLP a;
    a.A = sparse_view(h); a.m = (int)h->m; a.n = (int)h->n; a.nt = (int)((h->m + 15) / 16);
    a.bptr = h->sm_bptr; a.bi = h->sm_bi; a.bk = h->sm_bk; a.bcol = h->sm_bcol; a.bcoef = h->sm_bcoef; a.nb = h->sm_nb;
    a.x = h->x; a.y = h->y; a.s = h->s; a.b = h->b; a.c = h->c;
    a.rc = h->rc; a.d = h->d; a.v = h->v; a.q = h->q; a.dxa = h->dxa; a.dsa = h->dsa; a.dx = h->dx; a.ds = h->ds;
    a.sc = h->sc; a.hist = h->hist;
    a.eps = h->opt.pivot_guard_eps; a.big = h->opt.pivot_guard_big; a.shift_rel = h->shift_rel;
    a.max_steps = max_steps; a.auto_reg = auto_reg;
    if (h->bnd && h->detect) hipLaunchKernelGGL(small_lp_bounded_detect_kernel, dim3(1), dim3(PD_THREADS), 0, h->stream, a, bnd_args(h), det_args(h));
    else if (h->bnd) hipLaunchKernelGGL(small_lp_bounded_kernel, dim3(1), dim3(PD_THREADS), 0, h->stream, a, bnd_args(h));
    else if (h->detect) hipLaunchKernelGGL(small_lp_detect_kernel, dim3(1), dim3(PD_THREADS), 0, h->stream, a, det_args(h));
    else hipLaunchKernelGGL(small_lp_kernel, dim3(1), dim3(PD_THREADS), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

extern "C" int ipm_iterate(ipm_handle* h, int32_t n_steps, ipm_stats* stats) {
    int rc = check_ready(h, "ipm_iterate");
    if (rc) return rc;
    if (n_steps < 0) return fail(h, IPM_ERR_INVALID_ARG, "n_steps < 0");
    HIP_TRY(h, hipSetDevice(h->device));
    h->predictor_valid = false;
    std::vector<hipEvent_t> evs;
    struct EvGuard {                                   // destroyed on every return path
        std::vector<hipEvent_t>& v;
        ~EvGuard() { for (auto& e : v) if (e) (void)hipEventDestroy(e); }
    } guard{evs};
    if (h->profiling) {
        evs.assign((size_t)EV_PER_IT * n_steps, nullptr);
        for (auto& e : evs) HIP_TRY(h, hipEventCreate(&e));
    }
    float ms = 0.f;
    const int reset_k = h->fresh_state ? 1 : 0;      // iteration count and history restart with a newly set iterate
    h->fresh_state = false;
    if (h->small && !h->profiling) {
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, reset_k);
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        if ((rc = enqueue_small(h, n_steps, 0))) return rc;
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        if ((rc = read_scalars(h))) return rc;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        fill_stats(h, stats, ms);
        return IPM_OK;
    }
    for (int attempt = 0;; ++attempt) {
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1,
                           attempt == 0 ? reset_k : 0);
        const bool guard_poll = may_poll(h) && n_steps > 0;
        if (guard_poll && (rc = enqueue_snapshot(h, 0))) return rc;
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        for (int it = 0; it < n_steps; ++it)
            if ((rc = enqueue_iteration(h, h->profiling ? &evs[(size_t)it * EV_PER_IT] : nullptr))) return rc;
        // residuals + stop test of the state just reached: the statistics describe what ipm_get_state returns
        if ((rc = enqueue_residuals(h))) return rc;
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        bool tmo = false;
        if ((rc = read_scalars(h, &tmo))) return rc;
        if (!tmo) break;
        // (at most two recoveries per call: the fused launch falls back to formation + look-ahead factorization, which still polls
        //  device counters, and that one to stream events)
        if (attempt >= 2 || !guard_poll) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
        poll_fallback(h);
        if ((rc = enqueue_snapshot(h, 1))) return rc;
    }
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (h->profiling && n_steps > 0) {
        double ph[4] = {0, 0, 0, 0};
        for (int it = 0; it < n_steps; ++it) {
            hipEvent_t* e = &evs[(size_t)it * EV_PER_IT];
            float f = 0.f, total = 0.f;
            (void)hipEventElapsedTime(&f, e[1], e[2]); ph[0] += f;
            if (h->profiling < 2) continue;
            (void)hipEventElapsedTime(&f, e[2], e[3]); ph[1] += f;
            float s1 = 0.f, s2 = 0.f;
            (void)hipEventElapsedTime(&s1, e[4], e[5]); (void)hipEventElapsedTime(&s2, e[6], e[7]); ph[2] += s1 + s2;
            (void)hipEventElapsedTime(&total, e[0], e[8]);
            float f12 = 0.f, f23 = 0.f;
            (void)hipEventElapsedTime(&f12, e[1], e[2]); (void)hipEventElapsedTime(&f23, e[2], e[3]);
            ph[3] += total - f12 - f23 - s1 - s2;
        }
        for (int i = 0; i < 4; ++i) h->phase_ms[i] = ph[i] / n_steps;
    }
    fill_stats(h, stats, ms);
    return IPM_OK;
}

extern "C" int ipm_solve(ipm_handle* h, double tol_p, double tol_d, double tol_gap, int32_t max_iter, ipm_stats* stats) {
    int rc = check_ready(h, "ipm_solve");
    if (rc) return rc;
    if (max_iter < 0) return fail(h, IPM_ERR_INVALID_ARG, "max_iter < 0");
    HIP_TRY(h, hipSetDevice(h->device));
    h->predictor_valid = false; h->fresh_state = false;
    if (h->auto_reg) { h->auto_reg = 0; h->shift_rel = h->opt.regularize; }      // decided per solve
    hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, tol_p, tol_d, tol_gap, h->opt.eta, max_iter, 0, 1);
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    const int chunk = h->opt.check_every;
    const bool may_auto = h->opt.regularize == 0.0 && !(h->opt.flags & IPM_FLAG_NO_AUTO_REGULARIZE);
    if (h->small) {
        // one launch runs the loop to its end; a second one only when the first factorization asked for the shift
        // (the kernel leaves before it touches the iterate, so there is nothing to roll back)
        if ((rc = enqueue_small(h, 1 << 30, may_auto ? 1 : 0))) return rc;
        if ((rc = read_scalars(h))) return rc;
        if (h->h_sc->status == IPM_STATUS_NEEDS_SHIFT) {
            h->shift_rel = 1e-14; h->auto_reg = 1;
            hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, tol_p, tol_d, tol_gap, h->opt.eta, max_iter, 0, 1);
            if ((rc = enqueue_small(h, 1 << 30, 0))) return rc;
            if ((rc = read_scalars(h))) return rc;
        }
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        HIP_TRY(h, hipEventSynchronize(h->ev1));
        float ms_ = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms_, h->ev0, h->ev1));
        fill_stats(h, stats, ms_);
        return IPM_OK;
    }
    bool first = true;
    int recovered = 0;
    for (;;) {
        // roll-back point: the first chunk (auto-regularize restart) and every chunk that can hit a poll time-out
        const bool snap = first || may_poll(h);
        if (snap && (rc = enqueue_snapshot(h, 0))) return rc;
        for (int i = 0; i < chunk; ++i)
            if ((rc = enqueue_iteration(h, nullptr))) return rc;
        bool tmo = false;
        if ((rc = read_scalars(h, &tmo))) return rc;
        if (tmo) {
            if (!snap || ++recovered > 2) return fail(h, IPM_ERR_HIP, "hand-off time-out persists with stream events");
            poll_fallback(h);
            if ((rc = enqueue_snapshot(h, 1))) return rc;
            continue;                                          // same chunk again, with stream events
        }
        if (first && may_auto && h->h_sc->k > 0 && (double)h->h_sc->fixed_first > 0.05 * (double)h->m) {
            // A has > 5 % dependent rows (QAP family): the guard alone stalls the loop.  Restart
            // this solve from its start state with the 1e-14 Tikhonov shift.  No other Netlib file crosses 2.7 %, so
            // every solve that does not take this branch is bit-identical to one with the flag off.
            h->shift_rel = 1e-14; h->auto_reg = 1;
            if ((rc = enqueue_snapshot(h, 1))) return rc;
            first = false;
            continue;
        }
        first = false;
        if (h->h_sc->done) break;
    }
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    fill_stats(h, stats, ms);
    return IPM_OK;
}


// ------------------------------------------------------------------------------- lockstep batch (lockstep.h)
static void ls_gemm_hook(void* ctx, int bm, int bn, int bk, int wm, int wn, const GemmNT& g, int grid) {
    ipm_handle* h = (ipm_handle*)ctx;
    int type = -1;
    if (bm == -1) type = LS_CHOL_UPDATE;
    else if (bm == 32 && bn == 128 && bk == 32 && wm == 1 && wn == 8) type = LS_GEMM_32_128_32;
    else if (bm == 64 && bn == 64 && bk == 16) type = LS_GEMM_64_64_16;
    else if (bm == 64 && bn == 128 && bk == 16) type = LS_GEMM_64_128_16;
    else if (bm == 128 && bn == 128 && bk == 16 && wm == 2 && wn == 2) type = LS_GEMM_128_128_16;
    else if (bm == 32 && bn == 32 && bk == 32) type = LS_GEMM_32_32_32;
    if (g.batch > 1 || g.batch2 > 1) {                       // the group inverses' batched products: 3-D grid packed into the LP's block range
        if (type != LS_GEMM_32_32_32) { h->ls_cut = true; return; }
        ls_push(h, LS_GEMM_32_32_32_BATCHED, (unsigned)grid * (unsigned)g.batch * (unsigned)g.batch2, g);
        return;
    }
    if (type < 0 || g.wait_on || g.signal) { h->ls_cut = true; return; }      // not recordable: ls_record_program reports it
    ls_push(h, type, (unsigned)grid, g);
}
static bool ls_eligible(const ipm_handle* h) {
    return h->lockstep && !h->bnd && h->sparse && !h->small && !h->spf && h->lookahead == 0 && h->stream2 == nullptr && h->B && h->invD &&
           h->haveA && h->haveBC && h->haveState;
}
// the launch sequence of ONE iteration of the handle, recorded (nothing is launched)
static int ls_record_program(ipm_handle* h, std::vector<LsLaunch>& prog) {
    prog.clear();
    GemmRecorder rec{ls_gemm_hook, h};
    h->ls_rec = &prog; h->ls_cut = false;
    g_gemm_recorder = &rec;
    const int rc = enqueue_iteration(h, nullptr);
    g_gemm_recorder = nullptr;
    const bool cut = h->ls_cut;
    h->ls_rec = nullptr;
    if (rc) return rc;
    if (cut || prog.empty()) return fail(h, IPM_ERR_STATE, "ipm_solve_batch: the handle's iteration holds a launch without a lockstep twin");
    return IPM_OK;
}
struct LsStep { int type; unsigned count, blocks, lds; size_t offset; };      // `count` records from `offset` on; blocks = sum of their grids
// Merge the programs (each LP's order preserved) into global steps of one kernel type (lockstep_merge.h: progressive alignment;
// IPM_LS_MERGE=leader selects the first version for the A/B).
static void ls_merge(const std::vector<const std::vector<LsLaunch>*>& progs, std::vector<LsStep>& steps, std::vector<LsRec>& recs) {
    steps.clear(); recs.clear();
    std::vector<std::vector<int>> types(progs.size());
    for (size_t i = 0; i < progs.size(); ++i) { types[i].reserve(progs[i]->size()); for (const LsLaunch& L : *progs[i]) types[i].push_back(L.type); }
    static const bool leader = getenv("IPM_LS_MERGE") && !strcmp(getenv("IPM_LS_MERGE"), "leader");
    std::vector<LsPlanStep> plan;
    if (leader) ls_merge_leader(types, LS_MAX_GROUP, plan); else ls_merge_aligned(types, LS_MAX_GROUP, plan);
    for (const LsPlanStep& ps : plan) {
        LsStep st;
        st.type = ps.type; st.count = 0; st.blocks = 0; st.lds = 0; st.offset = recs.size();
        for (const auto& mb : ps.members) {
            const LsLaunch& L = (*progs[(size_t)mb.first])[(size_t)mb.second];
            LsRec r = L.rec;
            r.start = st.blocks;
            recs.push_back(r);
            st.count++; st.blocks += L.rec.gridx; st.lds = std::max(st.lds, L.rec.lds);
        }
        steps.push_back(st);
    }
}
// Test hook (CPU): the merge alone.  n programs, program i = types[off[i] .. off[i+1]); aligned != 0: the progressive alignment,
// 0: the leader rule.  out_steps (capacity cap_steps) receives {type, members} per step, out_members (capacity = total launches)
// {program, position} per member in step order.  Returns the step count, or -1 when a capacity is too small.
extern "C" int ipm_debug_ls_merge(int32_t n, const int32_t* off, const int32_t* types_flat, int32_t max_group, int32_t aligned,
                                  int32_t* out_steps, int32_t cap_steps, int32_t* out_members) {
    if (n < 0 || !off || (n > 0 && !types_flat) || max_group < 1) return -1;
    std::vector<std::vector<int>> types((size_t)n);
    for (int i = 0; i < n; ++i) types[(size_t)i].assign(types_flat + off[i], types_flat + off[i + 1]);
    std::vector<LsPlanStep> plan;
    if (aligned) ls_merge_aligned(types, max_group, plan); else ls_merge_leader(types, max_group, plan);
    if ((int64_t)plan.size() > cap_steps) return -1;
    size_t w = 0;
    for (size_t s = 0; s < plan.size(); ++s) {
        out_steps[2 * s] = plan[s].type; out_steps[2 * s + 1] = (int32_t)plan[s].members.size();
        for (const auto& mb : plan[s].members) { out_members[2 * w] = mb.first; out_members[2 * w + 1] = mb.second; ++w; }
    }
    return (int)plan.size();
}

struct ipm_batch {
    int device = 0;
    hipStream_t S = nullptr;
    bool own_stream = true;                            // S was created here (ipm_batch_create without a stream)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<ipm_handle*> hs;                       // in the order they were added
    std::vector<std::vector<LsLaunch>> prog;
    std::vector<char> first, finished;
    std::vector<int> active;
    std::vector<LsStep> steps;
    std::vector<LsRec> recs;
    LsRec* d_recs = nullptr;
    size_t d_cap = 0;
    bool dirty = true, started = false;
    int chunk = 1;
    double t_merge = 0, t_enqueue = 0, t_wait = 0;     // IPM_LS_DEBUG: host seconds merging schedules, enqueueing launches, waiting for the chunk
    long n_launch = 0, n_merge = 0;
    char err[512] = "";
};
static int bfail(ipm_batch* b, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof g_err, "%s", buf);
    if (b) snprintf(b->err, sizeof b->err, "%s", buf);
    return code;
}
#define B_TRY(b, call)                                                                                                        \
    do {                                                                                                                      \
        hipError_t e_ = (call);                                                                                               \
        if (e_ != hipSuccess) return bfail((b), IPM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

extern "C" int ipm_batch_create(int device, void* stream, ipm_batch** out) {
    if (!out) return bfail(nullptr, IPM_ERR_INVALID_ARG, "ipm_batch_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return bfail(nullptr, IPM_ERR_NO_DEVICE, "ipm_batch_create: device %d not visible", device);
    ipm_batch* b = new ipm_batch();
    b->device = device;
    hipError_t e = hipSetDevice(device);
    if (stream) { b->S = (hipStream_t)stream; b->own_stream = false; }          // the caller's stream (kept alive by the caller)
    else if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->S, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&b->ev0);
    if (e == hipSuccess) e = hipEventCreate(&b->ev1);
    static std::atomic<bool> attr_set[MAX_DEVICES];
    if (e == hipSuccess && device < MAX_DEVICES && !attr_set[device].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute((const void*)ls_adat_sparse, hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS_MAX_MP * 8);
        attr_set[device].store(true, std::memory_order_release);
    }
    if (e != hipSuccess) { const int rc = bfail(nullptr, IPM_ERR_HIP, "ipm_batch_create: %s", hipGetErrorString(e)); if (b->S && b->own_stream) (void)hipStreamDestroy(b->S); delete b; return rc; }
    *out = b;
    return IPM_OK;
}
extern "C" int ipm_batch_destroy(ipm_batch* b) {
    if (!b) return IPM_OK;
    (void)hipSetDevice(b->device);
    if (b->S) (void)hipStreamSynchronize(b->S);
    if (getenv("IPM_LS_DEBUG"))
        fprintf(stderr, "[lockstep] batch of %zu LPs: %ld launches, host %.3f s enqueueing (%.1f us per launch) + %.3f s waiting for the chunks + %.3f s in %ld schedule merges\n",
                b->hs.size(), b->n_launch, b->t_enqueue, b->n_launch ? 1e6 * b->t_enqueue / (double)b->n_launch : 0.0, b->t_wait, b->t_merge, b->n_merge);
    if (b->d_recs) dev_free(b->device, b->S, b->d_recs);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->S) { (void)hipStreamSynchronize(b->S); if (b->own_stream) (void)hipStreamDestroy(b->S); }
    delete b;
    return IPM_OK;
}
extern "C" const char* ipm_batch_last_error(const ipm_batch* b) { return b ? b->err : g_err; }

// A handle joins the batch (at any time between two ipm_batch_step calls): its solve starts from its current state with these
// tolerances, exactly as ipm_solve would start it.  *index = its position in the batch (what ipm_batch_step reports).
extern "C" int ipm_batch_add(ipm_batch* b, ipm_handle* h, double tol_p, double tol_d, double tol_gap, int32_t max_iter, int32_t* index) {
    if (!b || !h || max_iter < 0) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_batch_add: bad arguments");
    if (h->device != b->device) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_batch_add: the handle lives on device %d, the batch on %d", h->device, b->device);
    if (h->bnd) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_batch_add: a handle with upper bounds (ipm_set_bounds) has no lockstep twin");
    if (!ls_eligible(h)) return bfail(b, IPM_ERR_STATE, "ipm_batch_add: not a lockstep handle (IPM_FLAG_LOCKSTEP, sparse A, more than 128 rows, dense-tile factor, A / b / c / state set)");
    B_TRY(b, hipSetDevice(b->device));
    if (h->stream != b->S) B_TRY(b, hipStreamSynchronize(h->stream));      // everything the handle did on its own stream is complete
    h->predictor_valid = false; h->fresh_state = false;
    if (h->auto_reg) { h->auto_reg = 0; h->shift_rel = h->opt.regularize; }
    if (!b->started) { B_TRY(b, hipEventRecord(b->ev0, b->S)); b->started = true; }
    hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, b->S, h->sc, tol_p, tol_d, tol_gap, h->opt.eta, max_iter, 0, 1);
    int rc = enqueue_snapshot(h, 0, b->S);                     // roll-back point of the automatic Tikhonov shift (first chunk)
    if (rc) return bfail(b, rc, "%s", h->err);
    std::vector<LsLaunch> pr;
    if ((rc = ls_record_program(h, pr))) return bfail(b, rc, "%s", h->err);
    const int idx = (int)b->hs.size();
    b->hs.push_back(h); b->prog.push_back(std::move(pr)); b->first.push_back(1); b->finished.push_back(0);
    b->active.push_back(idx);
    b->chunk = std::max(b->chunk, (int)h->opt.check_every);
    b->dirty = true;
    if (index) *index = idx;
    return IPM_OK;
}

// One chunk (check_every iterations) of every active handle in lockstep, then the stop flags are read: the indices of the
// handles that finished in this chunk go to finished[0 .. *n_finished) (capacity cap), *n_active = handles still running.
extern "C" int ipm_batch_step(ipm_batch* b, int32_t* finished, int32_t cap, int32_t* n_finished, int32_t* n_active) {
    if (!b || !n_finished || (cap > 0 && !finished)) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_batch_step: bad arguments");
    *n_finished = 0;
    if (n_active) *n_active = (int32_t)b->active.size();
    if (b->active.empty()) return IPM_OK;
    B_TRY(b, hipSetDevice(b->device));
    hipStream_t S = b->S;
    const auto t_in = std::chrono::steady_clock::now();
    auto secs = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
    if (b->dirty) {
        std::vector<const std::vector<LsLaunch>*> ps;
        for (int i : b->active) ps.push_back(&b->prog[(size_t)i]);
        ls_merge(ps, b->steps, b->recs);
        B_TRY(b, hipStreamSynchronize(S));                   // (the table of the previous schedule may still be read)
        if (b->recs.size() > b->d_cap) {
            if (b->d_recs) dev_free(b->device, S, b->d_recs);
            b->d_recs = nullptr; b->d_cap = b->recs.size() + b->recs.size() / 2;
            B_TRY(b, dev_malloc(b->device, S, (void**)&b->d_recs, sizeof(LsRec) * b->d_cap));
        }
        B_TRY(b, hipMemcpyAsync(b->d_recs, b->recs.data(), sizeof(LsRec) * b->recs.size(), hipMemcpyHostToDevice, S));
        B_TRY(b, hipStreamSynchronize(S));                   // (`recs` is reused)
        b->dirty = false;
        b->t_merge += secs(t_in); b->n_merge++;
        if (getenv("IPM_LS_DEBUG")) {
            size_t longest = 0; int cnt[LS_NTYPES] = {0};
            for (int i : b->active) longest = std::max(longest, b->prog[(size_t)i].size());
            for (const LsStep& st : b->steps) cnt[st.type]++;
            fprintf(stderr, "[lockstep] %zu LPs active, longest program %zu launches, merged schedule %zu steps (%zu records); steps by type:", b->active.size(), longest, b->steps.size(), b->recs.size());
            for (int t = 0; t < LS_NTYPES; ++t) if (cnt[t]) fprintf(stderr, " %d:%d", t, cnt[t]);
            fprintf(stderr, "\n");
        }
    }
    const auto t_mid = std::chrono::steady_clock::now();
    static const bool ls_prof = getenv("IPM_LS_PROF") != nullptr;      // diagnostic: a synchronisation after every launch, wall time per kernel type
    if (ls_prof) {
        static double tot[LS_NTYPES]; static long cnt[LS_NTYPES]; static long calls = 0;
        for (int c = 0; c < b->chunk; ++c)
            for (const LsStep& st : b->steps) {
                const auto t0 = std::chrono::steady_clock::now();
                B_TRY(b, ls_launch(st.type, b->d_recs + st.offset, st.count, st.blocks, st.lds, S));
                B_TRY(b, hipStreamSynchronize(S));
                tot[st.type] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); cnt[st.type]++;
            }
        if (++calls % 25 == 0) {
            fprintf(stderr, "[lockstep prof] %zu active, %zu steps; us per launch (launches) by type:", b->active.size(), b->steps.size());
            for (int t = 0; t < LS_NTYPES; ++t) if (cnt[t]) fprintf(stderr, " %d:%.1f(%ld)", t, 1e6 * tot[t] / cnt[t], cnt[t]);
            fprintf(stderr, "\n");
            for (int t = 0; t < LS_NTYPES; ++t) { tot[t] = 0; cnt[t] = 0; }
        }
    } else
    for (int c = 0; c < b->chunk; ++c)
        for (const LsStep& st : b->steps) B_TRY(b, ls_launch(st.type, b->d_recs + st.offset, st.count, st.blocks, st.lds, S));
    for (int i : b->active) B_TRY(b, hipMemcpyAsync(b->hs[(size_t)i]->h_sc, b->hs[(size_t)i]->sc, sizeof(Scalars), hipMemcpyDeviceToHost, S));
    b->t_enqueue += secs(t_mid); b->n_launch += (long)b->chunk * (long)b->steps.size();
    const auto t_w = std::chrono::steady_clock::now();
    B_TRY(b, hipStreamSynchronize(S));
    b->t_wait += secs(t_w);
    if (getenv("IPM_LS_DEBUG") && atoi(getenv("IPM_LS_DEBUG")) >= 2) {
        size_t longest = 0, lead = 0;
        for (int i : b->active) if (b->prog[(size_t)i].size() > longest) { longest = b->prog[(size_t)i].size(); lead = (size_t)i; }
        static const auto t_proc = std::chrono::steady_clock::now();      // (first chunk of the process = 0)
        fprintf(stderr, "[lockstep chunk] t=%.3f s batch %p: %zu active, %zu steps (longest program %zu: %d rows), %.3f ms per iteration\n", secs(t_proc), (void*)b,
                b->active.size(), b->steps.size(), longest, (int)b->hs[lead]->m, 1e3 * secs(t_mid) / b->chunk);
    }
    std::vector<int> keep;
    for (int i : b->active) {
        ipm_handle* h = b->hs[(size_t)i];
        const bool may_auto = h->opt.regularize == 0.0 && !(h->opt.flags & IPM_FLAG_NO_AUTO_REGULARIZE);
        if (b->first[(size_t)i] && may_auto && h->h_sc->k > 0 && (double)h->h_sc->fixed_first > 0.05 * (double)h->m) {
            // > 5 % dependent rows (QAP family): restart this LP from its start state with the 1e-14 Tikhonov shift (as ipm_solve does)
            h->shift_rel = 1e-14; h->auto_reg = 1;
            int rc = enqueue_snapshot(h, 1, S);
            if (!rc) rc = ls_record_program(h, b->prog[(size_t)i]);
            if (rc) return bfail(b, rc, "%s", h->err);
            b->first[(size_t)i] = 0; b->dirty = true;
            keep.push_back(i);
            continue;
        }
        b->first[(size_t)i] = 0;
        if (h->h_sc->done) {
            b->dirty = true; b->finished[(size_t)i] = 1;
            if (*n_finished < cap) finished[(*n_finished)++] = i;
            continue;
        }
        keep.push_back(i);
    }
    b->active.swap(keep);
    if (n_active) *n_active = (int32_t)b->active.size();
    return IPM_OK;
}
extern "C" int ipm_batch_stats(ipm_batch* b, int32_t index, ipm_stats* stats) {
    if (!b || index < 0 || index >= (int32_t)b->hs.size() || !stats) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_batch_stats: bad arguments");
    float ms = 0.f;
    if (b->started) {
        (void)hipSetDevice(b->device);
        if (hipEventRecord(b->ev1, b->S) == hipSuccess && hipEventSynchronize(b->ev1) == hipSuccess) (void)hipEventElapsedTime(&ms, b->ev0, b->ev1);
    }
    fill_stats(b->hs[(size_t)index], stats, ms);             // (the handle's host mirror of the scalars was read by the step that saw it finish)
    return IPM_OK;
}

extern "C" int ipm_solve_batch(ipm_handle** hs, int32_t n, double tol_p, double tol_d, double tol_gap, int32_t max_iter, ipm_stats* stats) {
    if (!hs || n <= 0 || max_iter < 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_batch: bad arguments");
    for (int i = 0; i < n; ++i) if (!hs[i]) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_batch: NULL handle");
    for (int i = 0; i < n; ++i)
        if (hs[i]->bnd) return fail(hs[i], IPM_ERR_INVALID_ARG, "ipm_solve_batch: handle %d has upper bounds (ipm_set_bounds): no lockstep twin", i);
    ipm_batch* b = nullptr;
    int rc = ipm_batch_create(hs[0]->device, nullptr, &b);
    if (rc) return rc;
    struct Guard { ipm_batch* b; ~Guard() { ipm_batch_destroy(b); } } guard{b};
    for (int i = 0; i < n && !rc; ++i) { rc = ipm_batch_add(b, hs[i], tol_p, tol_d, tol_gap, max_iter, nullptr); if (rc) snprintf(hs[i]->err, sizeof hs[i]->err, "%s", b->err); }
    int32_t nfin = 0, nact = n;
    std::vector<int32_t> fin((size_t)n);
    while (!rc && nact > 0) rc = ipm_batch_step(b, fin.data(), n, &nfin, &nact);
    if (rc) { snprintf(hs[0]->err, sizeof hs[0]->err, "%s", b->err); return rc; }
    if (stats) for (int i = 0; i < n; ++i) ipm_batch_stats(b, i, &stats[i]);
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

extern "C" int ipm_get_schedule(ipm_handle* h, int32_t out[12]) {
    if (!h || !out) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_schedule: bad arguments");
    const int live = h->device < MAX_DEVICES ? g_live[h->device].load(std::memory_order_acquire) : 1;
    out[0] = h->nblk; out[1] = h->last_gs; out[2] = h->grouped_trsv;
    out[3] = (may_poll(h) && live <= 1) ? 1 : 0;
    out[4] = h->n_counter_steps; out[5] = h->n_event_steps; out[6] = h->use_env ? 1 : 0; out[7] = live;
    out[8] = h->timeouts_recovered; out[9] = h->small ? 1 : 0;
    out[10] = h->ff_last ? 1 : 0; out[11] = (h->spf && sp_level(h)) ? 1 : 0;
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
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    for (int attempt = 0;; ++attempt) {                     // second pass only after a recovered poll time-out
        hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(1), 0, h->stream, h->sc, 1e-8, 1e-8, 1e-8, h->opt.eta, 1 << 30, 1, 1);
        if (!reuse_factor) {
            if (d) {
                HIP_TRY(h, hipMemcpyAsync(h->d, d, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
            } else {
                hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->d, (int)h->n, 1.0);
            }
            if ((rc = enqueue_form(h, h->d))) return rc;
            if ((rc = enqueue_factor(h, true))) return rc;
            if ((rc = enqueue_group_inverses(h))) return rc;
        }
        HIP_TRY(h, hipMemsetAsync(h->t1, 0, sizeof(double) * h->mp, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->t1, rhs, sizeof(double) * h->m, hipMemcpyHostToDevice, h->stream));
        if ((rc = enqueue_potrs(h, h->t1, h->dy))) return rc;
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

// ------------------------------------------------------------------------------- general square systems (getrf_f64.h)
// No handle: the call owns a stream and its device memory and releases both before it returns.
namespace {
struct LuRun {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    ~LuRun() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : allocs) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int alloc(void** p, size_t bytes, const char* what) {
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(nullptr, IPM_ERR_WORKSPACE, "lu: cannot allocate %zu bytes of device memory for %s: %s", bytes, what, hipGetErrorString(e));
        }
        allocs.push_back(*p);
        return IPM_OK;
    }
};
}  // namespace

#define LU_TRY(call)                                                                                                   \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) return fail(nullptr, IPM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Panel width.  Measured on MI355X (LU section; profiles/r05_lu_20480_kernel_stats.txt): kernel time at n = 20480
// 734 ms with 64 against 775 ms with 128 (the wider panel's trailing update is faster, 133 vs 158 ms, its panel steps slower,
// 576 vs 524 ms), wall time at n = 8192 0.173 vs 0.194 s.  64 is the default; IPM_LU_NB=128 selects the other.
static int lu_nb() {
    const char* e = getenv("IPM_LU_NB");
    return (e && atoi(e) == 128) ? 128 : 64;
}

template <int NB>
static int lu_factor_device(LuRun& R, double* a, int64_t np, int n, LuState* st, int* ipiv, double* ut) {
    // The dynamic-LDS limits of this width's kernels, once per device.  Under the mutex, so no thread launches them before the
    // thread that sets the attributes has finished (an exchange-first flag let a second thread through early); a failed
    // attempt leaves the flag clear for the next call.
    static std::mutex attr_mu;
    static bool attr_set[MAX_DEVICES];
    {
        std::lock_guard<std::mutex> lk(attr_mu);
        if (!attr_set[R.device]) {
            LU_TRY(hipFuncSetAttribute((const void*)lu_trsm_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, NB * NB * 8));
            LU_TRY(hipFuncSetAttribute((const void*)lu_trsv_step_kernel<NB, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (NB * NB + NB * LU_RC) * 8));
            LU_TRY(hipFuncSetAttribute((const void*)lu_trsv_step_kernel<NB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (NB * NB + NB * LU_RC) * 8));
            attr_set[R.device] = true;
        }
    }
    const int npi = (int)np;
    for (int k = 0; k < npi; k += NB) {
        for (int j = -1; j < NB; ++j) {
            const int rows = npi - (k + j + 1);
            int g = (rows + 63) / 64;                 // 16 rows per wave
            g = g < 1 ? 1 : (g > LU_MAX_GRID ? LU_MAX_GRID : g);
            hipLaunchKernelGGL(lu_panel_step_kernel<NB>, dim3(g), dim3(256), 0, R.stream, a, np, n, npi, k, j, st, ipiv);
        }
        if (npi > NB)
            hipLaunchKernelGGL(lu_laswp_kernel<NB>, dim3((unsigned)((npi - NB + 255) / 256)), dim3(256), 0, R.stream, a, np, npi, k, ipiv);
        const int rest = npi - k - NB;
        if (rest > 0) {
            hipLaunchKernelGGL(lu_trsm_kernel<NB>, dim3((unsigned)((rest + 127) / 128)), dim3(128), NB * NB * 8, R.stream, a, np, npi, k, ut);
            GemmNT g;
            memset(&g, 0, sizeof g);
            g.P = a + (int64_t)(k + NB) * np + k; g.ldp = np;
            g.Q = ut + (int64_t)(k + NB) * NB; g.ldq = NB;
            g.C = a + (int64_t)(k + NB) * np + k + NB; g.ldc = np;
            g.M = rest; g.N = rest; g.K = NB;
            g.alpha = -1.0; g.beta = 1.0;
            g.unit_diag_from = -1;
            g.batch = 1; g.batch2 = 1;
            if (NB == 128) LU_TRY((launch_gemm_nt<128, 128, 16, 2, 2>(g, R.stream)));
            else LU_TRY((launch_gemm_nt<64, 64, 16, 2, 2>(g, R.stream)));
        }
        LU_TRY(hipGetLastError());
    }
    return IPM_OK;
}

// Upload A (n x n, lda) into a padded np x np device image, factor it.  On return ipiv_h holds the np interchanges and *info the
// LAPACK info; a, ipiv stay on the device for the substitution.
static int lu_run_factor(LuRun& R, int nb, int64_t n, const double* A, int64_t lda, double** a_out, int** ipiv_out,
                         std::vector<int>& ipiv_h, int64_t* info) {
    const int64_t np = round_up(n, nb);
    double* a = nullptr; double* ut = nullptr; LuState* st = nullptr; int* ipiv = nullptr; int* bad = nullptr;
    if (int rc = R.alloc((void**)&a, sizeof(double) * np * np, "the matrix")) return rc;
    if (int rc = R.alloc((void**)&ut, sizeof(double) * np * nb, "the U strip")) return rc;
    if (int rc = R.alloc((void**)&st, sizeof(LuState), "the panel state")) return rc;
    if (int rc = R.alloc((void**)&ipiv, sizeof(int) * np, "the pivots")) return rc;
    if (int rc = R.alloc((void**)&bad, sizeof(int), "a flag")) return rc;
    LU_TRY(hipMemsetAsync(a, 0, sizeof(double) * np * np, R.stream));
    LU_TRY(hipMemsetAsync(st, 0, sizeof(LuState), R.stream));
    LU_TRY(hipMemsetAsync(bad, 0, sizeof(int), R.stream));
    LU_TRY(hipMemcpy2DAsync(a, sizeof(double) * np, A, sizeof(double) * lda, sizeof(double) * n, n, hipMemcpyHostToDevice, R.stream));
    hipLaunchKernelGGL(lu_prepare_kernel, dim3((unsigned)((np * np + 255) / 256)), dim3(256), 0, R.stream, a, np, (int)n, (int)np, bad);
    LU_TRY(hipGetLastError());
    int h_bad = 0;
    LU_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, R.stream));
    LU_TRY(hipStreamSynchronize(R.stream));
    if (h_bad) return fail(nullptr, IPM_ERR_INVALID_INPUT, "lu: the matrix has NaN or Inf entries");
    int rc = nb == 64 ? lu_factor_device<64>(R, a, np, (int)n, st, ipiv, ut) : lu_factor_device<128>(R, a, np, (int)n, st, ipiv, ut);
    if (rc) return rc;
    ipiv_h.assign((size_t)np, 0);
    int h_info = 0;
    LU_TRY(hipMemcpyAsync(ipiv_h.data(), ipiv, sizeof(int) * np, hipMemcpyDeviceToHost, R.stream));
    LU_TRY(hipMemcpyAsync(&h_info, (char*)st + offsetof(LuState, info), sizeof(int), hipMemcpyDeviceToHost, R.stream));
    LU_TRY(hipStreamSynchronize(R.stream));
    *info = h_info;
    *a_out = a; *ipiv_out = ipiv;
    return IPM_OK;
}

static int lu_begin(LuRun& R, int device, const char* who) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return fail(nullptr, IPM_ERR_NO_DEVICE, "%s: no HIP device", who); }
    if (device < 0 || device >= count || device >= MAX_DEVICES) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: no device %d", who, device);
    R.device = device;
    LU_TRY(hipSetDevice(device));
    LU_TRY(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
    return IPM_OK;
}

extern "C" int ipm_lu_factor(int device, int64_t n, const double* A, int64_t lda, double* LU, int64_t ldlu, int32_t* ipiv,
                             int64_t* info) {
    if (n < 1 || n > (1 << 30) / 2 || !A || !LU || !ipiv || !info || lda < n || ldlu < n)
        return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_lu_factor: bad arguments");
    LuRun R;
    if (int rc = lu_begin(R, device, "ipm_lu_factor")) return rc;
    const int nb = lu_nb();
    double* a = nullptr; int* dpiv = nullptr;
    std::vector<int> piv;
    if (int rc = lu_run_factor(R, nb, n, A, lda, &a, &dpiv, piv, info)) return rc;
    const int64_t np = round_up(n, nb);
    LU_TRY(hipMemcpy2DAsync(LU, sizeof(double) * ldlu, a, sizeof(double) * np, sizeof(double) * n, n, hipMemcpyDeviceToHost, R.stream));
    LU_TRY(hipStreamSynchronize(R.stream));
    for (int64_t i = 0; i < n; ++i) ipiv[i] = piv[i];
    if (*info > 0) return fail(nullptr, IPM_ERR_SINGULAR, "ipm_lu_factor: U[%lld][%lld] is exactly zero: the matrix is singular",
                               (long long)(*info - 1), (long long)(*info - 1));
    return IPM_OK;
}

extern "C" int ipm_lu_solve(int device, int64_t n, const double* A, int64_t lda, int64_t nrhs, const double* B, int64_t ldb,
                            double* X, int64_t ldx, int64_t* info) {
    if (n < 1 || n > (1 << 30) / 2 || nrhs < 1 || nrhs > (1 << 20) || !A || !B || !X || !info || lda < n || ldb < nrhs || ldx < nrhs)
        return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_lu_solve: bad arguments");
    LuRun R;
    if (int rc = lu_begin(R, device, "ipm_lu_solve")) return rc;
    const int nb = lu_nb();
    const int64_t np = round_up(n, nb);
    const int nr = (int)nrhs;
    double *bd = nullptr, *y = nullptr, *z = nullptr;
    int *perm = nullptr, *bad = nullptr;
    if (int rc = R.alloc((void**)&bd, sizeof(double) * np * nr, "the right-hand sides")) return rc;
    if (int rc = R.alloc((void**)&y, sizeof(double) * np * nr, "the right-hand sides")) return rc;
    if (int rc = R.alloc((void**)&z, sizeof(double) * np * nr, "the right-hand sides")) return rc;
    if (int rc = R.alloc((void**)&perm, sizeof(int) * np, "the permutation")) return rc;
    if (int rc = R.alloc((void**)&bad, sizeof(int), "a flag")) return rc;
    // B first (X may alias it, and the factorization's failure paths must not have consumed it)
    LU_TRY(hipMemsetAsync(bd, 0, sizeof(double) * np * nr, R.stream));
    LU_TRY(hipMemsetAsync(bad, 0, sizeof(int), R.stream));
    LU_TRY(hipMemcpy2DAsync(bd, sizeof(double) * nr, B, sizeof(double) * ldb, sizeof(double) * nr, n, hipMemcpyHostToDevice, R.stream));
    hipLaunchKernelGGL(lu_check_kernel, dim3((unsigned)((n * nr + 255) / 256)), dim3(256), 0, R.stream, bd, n * nr, bad);
    LU_TRY(hipGetLastError());
    int h_bad = 0;
    LU_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, R.stream));
    LU_TRY(hipStreamSynchronize(R.stream));
    if (h_bad) return fail(nullptr, IPM_ERR_INVALID_INPUT, "ipm_lu_solve: the right-hand side has NaN or Inf entries");
    double* a = nullptr; int* dpiv = nullptr;
    std::vector<int> piv;
    if (int rc = lu_run_factor(R, nb, n, A, lda, &a, &dpiv, piv, info)) return rc;
    if (*info > 0) return fail(nullptr, IPM_ERR_SINGULAR, "ipm_lu_solve: U[%lld][%lld] is exactly zero: the matrix is singular",
                               (long long)(*info - 1), (long long)(*info - 1));
    // P as a gather: apply the interchanges, in order, to the identity
    std::vector<int> pm((size_t)np);
    for (int64_t i = 0; i < np; ++i) pm[i] = (int)i;
    for (int64_t i = 0; i < np; ++i) std::swap(pm[i], pm[piv[i]]);
    LU_TRY(hipMemcpyAsync(perm, pm.data(), sizeof(int) * np, hipMemcpyHostToDevice, R.stream));
    hipLaunchKernelGGL(lu_gather_kernel, dim3((unsigned)((np * nr + 255) / 256)), dim3(256), 0, R.stream, bd, y, perm, (int)np, nr);
    const unsigned gq = (unsigned)((nr + LU_RC - 1) / LU_RC);
    const size_t lds = (size_t)(nb * nb + nb * LU_RC) * 8;
    const int nblk = (int)(np / nb);
    for (int b = 0; b < nblk; ++b) {                          // forward: y -> z (unit L)
        const int b0 = b * nb;
        const unsigned gx = 1 + (unsigned)((np - b0 - nb + LU_TRSV_ROWS - 1) / LU_TRSV_ROWS);
        if (nb == 64) hipLaunchKernelGGL((lu_trsv_step_kernel<64, false>), dim3(gx, gq), dim3(256), lds, R.stream, a, np, (int)np, b0, y, z, nr);
        else hipLaunchKernelGGL((lu_trsv_step_kernel<128, false>), dim3(gx, gq), dim3(256), lds, R.stream, a, np, (int)np, b0, y, z, nr);
    }
    for (int b = nblk - 1; b >= 0; --b) {                     // backward: z -> y (U)
        const int b0 = b * nb;
        const unsigned gx = 1 + (unsigned)((b0 + LU_TRSV_ROWS - 1) / LU_TRSV_ROWS);
        if (nb == 64) hipLaunchKernelGGL((lu_trsv_step_kernel<64, true>), dim3(gx, gq), dim3(256), lds, R.stream, a, np, (int)np, b0, z, y, nr);
        else hipLaunchKernelGGL((lu_trsv_step_kernel<128, true>), dim3(gx, gq), dim3(256), lds, R.stream, a, np, (int)np, b0, z, y, nr);
    }
    LU_TRY(hipGetLastError());
    LU_TRY(hipMemcpy2DAsync(X, sizeof(double) * ldx, y, sizeof(double) * nr, sizeof(double) * nr, n, hipMemcpyDeviceToHost, R.stream));
    LU_TRY(hipStreamSynchronize(R.stream));
    return IPM_OK;
}
