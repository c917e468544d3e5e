// host_handle.h -- host side of libipm_hip.so, unit 1: the handle, the scheduling predicates every launch site shares, error
// reporting, the stream-ordered memory pool, the workspace layout and the argument views of the handle's device arrays.
// Single translation unit: included by ipm_api.hip after the kernel headers, `static` functions only.
#pragma once
static thread_local char g_err[512] = "";

// Live handles per device.  The device-polled hand-offs of the Cholesky look-ahead are only safe while ONE handle
// drives the GPU (its two streams then sit on hardware queues of their own); with more than one live handle on a
// device every factorization uses stream events instead (polls_device is an input of the step plan, chol_plan.h).  Counted at create / destroy.
static const int MAX_DEVICES = 64;
static std::atomic<int> g_live[MAX_DEVICES];
static std::atomic<bool> g_attr_set[MAX_DEVICES];      // per-device function attributes (dynamic LDS of adat_sparse)

// A round feature (centrality correctors, iterative refinement): k rounds set by the caller, device memory of its own made on first
// use, and at the END of that memory a control record the kernels keep (tallies, the rounds' `done` word) with its roll-back copy
// CTL_DOUBLES, the room of one record, behind it.  RoundsKind is what differs between the features besides where their vectors lie:
// the words of the messages, the range of k and the size formula.  The operations are in host_iteration.h (rounds_*).
struct ipm_handle;
struct RoundsKind { const char *noun, *none, *setter; int feature, kmax; size_t (*doubles)(const ipm_handle*); };      // (feature: its IPM_FEATURE_* of host_compat.h)
template <class Ctl, int CTL_DOUBLES> struct Rounds {
    static_assert(sizeof(Ctl) <= sizeof(double) * CTL_DOUBLES, "the record outgrew its slot");
    const RoundsKind* kind;
    int k = 0;
    double* mem = nullptr;
    Ctl host = Ctl{};                     // host copy of the record, read back with the scalar record (read_scalars)
    Ctl* ctl_copy(const ipm_handle* h) const { return (Ctl*)((double*)ctl(h) + CTL_DOUBLES); }
    Ctl* ctl(const ipm_handle* h) const { return (Ctl*)(mem + kind->doubles(h) - 2 * CTL_DOUBLES); }
};
static const int MCC_CTL_DOUBLES = 8, REF_CTL_DOUBLES = 16;
static size_t mcc_doubles(const ipm_handle* h), ref_doubles(const ipm_handle* h);      // (beside the views, below)
static const RoundsKind MCC_KIND{"centrality correctors", "no rounds", "ipm_set_centrality_correctors", IPM_FEATURE_CORRECTORS, IPM_MAX_CORRECTORS, mcc_doubles};
static const RoundsKind REF_KIND{"refinement rounds", "none", "ipm_set_refinement", IPM_FEATURE_REFINEMENT, IPM_MAX_REFINE, ref_doubles};

// A set of columns the caller marks (free columns with curvature, LP free columns): own allocation of np bytes, made on first use and kept.
struct ColumnSet {
    bool on = false;                      // the set is not empty: its kernel instantiations run
    std::vector<int> cols;                // the set, in the caller's order
    std::vector<char> host;               // host: column j is in the set (empty without a set), what the per-column checks read
    unsigned char* mark = nullptr;        // 1 on the set's columns, 0 elsewhere and in the padding (written whole); scale-free and
                                          // constant during a solve, so neither the equilibration nor the roll-back snapshot touch it
    bool has(int64_t j) const { return on && host[(size_t)j] != 0; }
};

struct ipm_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream2 = nullptr;            // bulk stream of the Cholesky look-ahead
    hipStream_t stream3 = nullptr;            // residual stream: r_b, r_c, stop test and the predictor rhs under the factorization
    hipEvent_t ev_mid = nullptr, ev_res = nullptr, ev_grp = nullptr, ev_last = nullptr;
    // A^T dy streamed behind the backward sweeps (host_iteration.h): on until a hand-off time-out or IPM_STREAM_AT=0;
    // at_epoch counts the sweep events signalled so far (the progress word, at_progress_word, holds the last one: monotone, never
    // cleared; it would wrap after 2^32 events, some 7e8 iterations of one handle); ev_at joins the residual stream's pieces into the
    // main stream
    int stream_at = 1;
    unsigned at_epoch = 0;
    hipEvent_t ev_at = nullptr;
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
    long long sp_nslot = 0, sp_nu = 0, sp_terms = 0, sp_uvlen = 0;      // (sp_uvlen: doubles of the forward sweep's update vectors)
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
    // dense columns split out of the sparse factor (ipm_set_dense_columns, dense_split.h)
    std::vector<int> ds_cols;             // the set asked for, in the caller's order; ipm_set_A_csc builds the split from it
    bool ds_on = false;                   // the sparse factor in place is that of A without those columns: W and R follow every factorization
    DsSplit dsp;                          // device view (own allocations, freed with the sparse factor's)
    long long ds_factorizations = 0, ds_corrections = 0;
    double shift_rel = 0.0;               // Tikhonov shift in effect (opt.regularize, or 1e-14 switched on by ipm_solve)
    int auto_reg = 0;                     // 1: the shift was switched on automatically
    unsigned* d_flags = nullptr;          // [2*nblk] hand-off flags + 1 timeout word + 1 progress word of the streamed A^T dy (own allocation)
    int64_t m = 0, n = 0, mp = 0, np = 0;
    int nblk = 0, rc_chunks = 0, rows_per_chunk = 0, vblk = 0;
    ipm_options opt;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    bool own_ws = false;
    bool guarded = false;                 // the workspace carries guard bands (IPM_TEST_ALLOC_GUARD at ipm_create), entered in the registry
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
    bool ginv_ref = false;                // IPM_GINV_REF=1: the group inverses as three launches of the generic kernel per level, the reference of tests/test_gpu_group_inverse.py
    bool ff_ref_engine = false;           // IPM_FF_REF_ENGINE=1: form_factor_roles_kernel (the engines' previous stage schedule), the reference of tests/test_gpu_ff_engines.py
    int ff_q = 4;                         // formation chunks per tile (IPM_FF_Q)
    int ff_workers = 0;                   // WORKER workgroups of the persistent launch (set by ff_build from the CU count, no switch)
    int* d_ff_tile_items = nullptr;       // [tile_items | tile_q]
    int ff_qmax = 16;                     // slab capacity per tile (the first block rows are formed in more, shorter chunks)
    bool ff_built = false, ff_last = false;
    FFSchedule ff_sched;
    FFItem* d_ff_items = nullptr;         // the work list in ticket order
    unsigned* d_ff_flags = nullptr;       // the hand-off words (layout: FFWords, ff_schedule.h) + as many again for the diagnostic snapshot
    size_t ff_flag_words = 0;             // FFWords::count
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
    // separable convex QP (ipm_set_quadratic): own allocation of one np-vector, made on first use
    bool quad = false;                    // a positive entry is set: the Quad kernel instantiations run
    int64_t quad_nnz = 0;                 // positive entries of g
    double* quad_g = nullptr;             // g in the handle's units (g C^2 on a scaled handle), zero in the padding; constant during a
                                          // solve, so the roll-back snapshot carries nothing of it
    std::vector<char> quad_pos;           // host: g_j > 0 (empty without a term), what the free-column checks read
    std::vector<char> bnd_finite;         // host: u_j finite (empty without a finite bound), for the same checks
    // free columns with curvature (ipm_set_free_columns) and LP free columns (ipm_set_free_lp_columns, DESIGN.md 4-W:
    // never together with a quadratic term or the first set)
    ColumnSet free_set, free_lp_set;
    double free_lp_rho = 1e-8;            // the proximal weight, in the handle's units (IPM_FREE_LP_RHO_DEFAULT)
    // centrality correctors (ipm_set_centrality_correctors): up to mcc.k rounds per iteration re-use its factor
    Rounds<MccCtl, MCC_CTL_DOUBLES> mcc{&MCC_KIND};   // mem: q v dx ds r3 r3g | qz dw dz r4 r4g (n-vectors) | dy (m-vector) | partial minima [2][MAXPART] | record | its copy
    // iterative refinement of the normal-equations solves (ipm_set_refinement): up to ref.k rounds behind every solve
    // of the iteration and of ipm_normal_solve
    Rounds<RefCtl, REF_CTL_DOUBLES> ref{&REF_KIND};   // mem: t r delta dy-copy (m-vectors) | atp-copy, A^T delta partials [rc_chunks][np] | partial sums [2][mp/16] | record | its copy
    const int* sdone = nullptr;           // the word the products with A and the substitutions test in place of Scalars::done (solve_done, SolveWord)
    // infeasibility detection (IPM_FLAG_DETECT_INFEASIBILITY): the Detect kernel instantiations run
    bool detect = false;
    bool detect_qp = false;               // IPM_FLAG_DETECT_QUADRATIC on top: the setters of a quadratic term / of free columns accept the handle
    double det_eps_p = 1e-8, det_eps_d = 1e-8;   // ipm_set_infeasibility_tol
    double* det = nullptr;                // [4] record of the last detection (workspace): kind, normalisation, violation, k
    double* cert_mem = nullptr;           // x | y | z of ipm_get_certificate (own allocation, made on first use)
    // power-of-two equilibration (ipm_equilibrate): the device holds the SCALED problem; the factors live here, on the
    // host, where the boundary rule applies them (host_equilibrate.h)
    bool scaled = false;
    std::vector<double> eq_r, eq_c;       // R (length m, the handle's row order), C (length n)
    int* fixed = nullptr;
    Scalars* h_sc = nullptr;          // pinned host mirror
    bool haveA = false, haveBC = false, haveState = false, predictor_valid = false;
    bool fresh_state = true;              // the iterate was (re)set: the next ipm_iterate counts its steps from k = 0
    int profiling = 0;                    // 0 off, 1 events around the A D^2 A^T kernel only, 2 every phase
    double phase_ms[4] = {0, 0, 0, 0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // lockstep batch (lockstep.h, ipm_solve_batch): while non-null, launch_twin (below) RECORDS here instead of launching
    std::vector<struct LsLaunch>* ls_rec = nullptr;
    bool ls_cut = false;                  // a launch without a lockstep twin was met while recording
    int lockstep = 0;                     // IPM_FLAG_LOCKSTEP: created for ipm_solve_batch (block-step substitutions: every launch of the iteration is recordable)
    // switches ipm_create acts on once (read_env_switches)
    unsigned spin_limit = 1u << 22;       // IPM_TEST_SPIN_LIMIT: spin bound of the device-side hand-offs (test knob, see handoff.h)
    bool ragged_groups = true;            // IPM_RAGGED_GROUPS=0: group inverses only where the group size divides the block count
    bool ls_block_steps = false, potrf_stamps = false, ff_chain_mode0 = false;   // IPM_LS_BLOCK_STEPS (A/B: block-step substitutions in the lockstep
                                          // batch), IPM_POTRF_STAMPS (allocate stamp_buf), IPM_FF_CHAIN_MODE=0 was asked for (refused by ipm_create)
    char err[512] = "";
};
struct LsLaunch { int type; LsRec rec; };
// A launch site of the iteration names its kernel type and fills ONE argument struct (lockstep.h: LsTwin<T>): the launch is recorded
// while a program is being recorded (record_twin: also the GEMM launchers' way in, ls_gemm_hook), else the single-LP kernel runs.
template <int T> static void record_twin(ipm_handle* h, unsigned gridx, const LsArgs<T>& a, unsigned lds = 0) {
    LsLaunch L{};
    L.type = T; L.rec.gridx = gridx; L.rec.lds = lds;
    memcpy(L.rec.args, &a, sizeof a);
    h->ls_rec->push_back(L);
}
template <int T> static void launch_twin(ipm_handle* h, unsigned grid, const LsArgs<T>& a, hipStream_t st = nullptr, unsigned lds = 0) {
    if (h->ls_rec) record_twin<T>(h, grid, a, lds);
    else LsTwin<T>::single(a, grid, lds, st ? st : h->stream);
}
// A launch WITHOUT a twin that shares an if / else chain with recorded sites: while recording nothing is launched and the program
// is marked cut, so that ls_record_program refuses the handle instead of keeping a program with a hole.
template <class... P, class... Q> static void launch_untwinned(ipm_handle* h, void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st, const Q&... args) {
    if (h->ls_rec) h->ls_cut = true;
    else hipLaunchKernelGGL(kernel, grid, block, 0, st ? st : h->stream, args...);
}

// the message goes to the thread's record and to `err` (char[512] of a handle or a batch, may be null); returns `code`
static int vfail(char* err, int code, const char* fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    snprintf(g_err, sizeof g_err, "%s", buf);
    if (err) snprintf(err, 512, "%s", buf);
    return code;
}
static int fail(ipm_handle* h, int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); code = vfail(h ? h->err : nullptr, code, fmt, ap); va_end(ap); return code; }

#define HIP_TRY(h, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((h), IPM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                  \
    } while (0)

static inline int64_t round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }

// ------------------------------------------------------------------------------- scheduling rules, each stated once
static inline int live_on_device(const ipm_handle* h) { return h->device < MAX_DEVICES ? g_live[h->device].load(std::memory_order_acquire) : 1; }
static inline bool alone_on_device(const ipm_handle* h) { return live_on_device(h) <= 1; }      // device-polled hand-offs are allowed (see g_live)
static inline bool lookahead_wanted(int lookahead, int nblk) { return lookahead != 0 && nblk > 2; }      // (ipm_create makes the bulk stream then)
static inline bool lookahead_on(const ipm_handle* h) { return lookahead_wanted(h->lookahead, h->nblk) && h->stream2 != nullptr; }
// wants_polling: the handle ASKS for device-polled hand-offs in the look-ahead; polls_device: a launch enqueued now gets them.
// may_poll (host_iteration.h) decides about the roll-back snapshot with wants_polling, WITHOUT alone_on_device: the live-handle
// count can change between the snapshot and the launch, so the snapshot rule is deliberately the conservative superset of the
// launch rule -- a launch that polls always has a snapshot to roll back to.
static inline bool wants_polling(const ipm_handle* h) { return lookahead_on(h) && h->flag_sync != 0; }
static inline bool polls_device(const ipm_handle* h) { return wants_polling(h) && alone_on_device(h); }
static inline unsigned* timeout_word(const ipm_handle* h) { return h->d_flags + 2 * (size_t)h->nblk; }      // time-out word of the device-side hand-offs
static inline unsigned* at_progress_word(const ipm_handle* h) { return timeout_word(h) + 1; }               // progress word of the streamed A^T dy (d_flags has four spare words)
static inline const int* solve_done(const ipm_handle* h) { return h->sdone ? h->sdone : &h->sc->done; }       // `done` word the products with A and the substitutions test
// sets that word for a scope: the previous one comes back on every return path
struct SolveWord {
    ipm_handle* const h; const int* const prev;
    SolveWord(ipm_handle* h_, const int* w) : h(h_), prev(h_->sdone) { h->sdone = w; }
    ~SolveWord() { h->sdone = prev; }
    SolveWord(const SolveWord&) = delete;
};
static inline const int* factor_done(const ipm_handle* h) { return h->fdone ? h->fdone : &h->sc->done; }    // `done` word formation / factorization test

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
// Test knob IPM_TEST_ALLOC_FILL=<byte 0..255>: every device allocation of the library (and the workspace, ipm_create) is filled with
// that byte on the stream it is first used on, BEFORE any write of the library's own -- so that a result which depends on what the memory
// held before shows (0xFF: NaN as doubles, -1 as indices; tests/test_gpu_residue.py).  Read at each allocation, so that a test can
// switch it between two handles of one process.  Unset: -1, and nothing is enqueued.
static int alloc_fill_byte() {
    const char* e = getenv("IPM_TEST_ALLOC_FILL");
    if (!e || !*e) return -1;
    const int v = atoi(e);
    return v < 0 || v > 255 ? -1 : v;
}
static hipError_t alloc_fill(void* p, size_t bytes, hipStream_t stream) {
    const int v = alloc_fill_byte();
    return v < 0 ? hipSuccess : hipMemsetAsync(p, v, bytes, stream);
}
// Test knob IPM_TEST_ALLOC_GUARD=<band bytes, a multiple of 256>[:<band byte 0..255, default 255>]: every device allocation of the
// library gets a band of that many bytes on each side, filled with the band byte, and the workspace one band before its first region,
// between every two regions and behind the last (make_layout) -- so that a kernel that writes outside the memory it was given shows
// (tests/test_gpu_alloc_guard.py).  Read at each allocation and by every make_layout, like IPM_TEST_ALLOC_FILL; anything
// malformed (text, a negative or zero width, no multiple of 256, a byte outside 0..255) is the knob unset.  Unset: band 0 -- no extra
// byte, no launch, no synchronisation, no registry entry.  Host code only: the comparison is done on the host, there is no kernel.
struct GuardKnob { size_t band = 0; int byte = 255; };
static GuardKnob alloc_guard() {
    GuardKnob g;
    const char* e = getenv("IPM_TEST_ALLOC_GUARD");
    if (!e || !*e) return g;
    char* end = nullptr;
    const long long w = strtoll(e, &end, 10);
    if (end == e || w <= 0 || w % 256 || w > (1ll << 30)) return g;
    long b = 255;
    if (*end == ':') { const char* t = end + 1; b = strtol(t, &end, 10); if (end == t || b < 0 || b > 255) return g; }
    if (*end) return g;
    g.band = (size_t)w; g.byte = (int)b;
    return g;
}
// The process-wide registry of live bands and the log of the damage found when a guarded block was released.  owner: the handle whose
// workspace the band lies in (null for a pool block, which is told apart by the stream it was allocated on).
struct GuardRec { ipm_guard_band b; const void* owner; hipStream_t stream; };
static std::mutex g_guard_mutex;
static std::vector<GuardRec> g_guard_live;
static std::vector<ipm_guard_band> g_guard_log;
static std::atomic<int> g_guard_count{0};       // live records: 0 lets every release return at once
static int g_guard_ordinal = 0;
static void guard_compare(const unsigned char* p, size_t bytes, int byte, int64_t* first_bad, int64_t* bad_count) {
    int64_t first = -1, cnt = 0;
    for (size_t i = 0; i < bytes; ++i)
        if (p[i] != (unsigned char)byte) { if (first < 0) first = (int64_t)i; ++cnt; }
    *first_bad = first; *bad_count = cnt;
}
static void guard_register(const void* owner, hipStream_t stream, const char* tag, int side, const void* addr, size_t bytes, const void* inner,
                           size_t inner_bytes, int device, int byte, int ordinal) {
    GuardRec r{};
    snprintf(r.b.tag, sizeof r.b.tag, "%s", tag);
    r.b.address = (uint64_t)(uintptr_t)addr; r.b.bytes = bytes; r.b.inner = (uint64_t)(uintptr_t)inner; r.b.inner_bytes = inner_bytes;
    r.b.side = side; r.b.device = device; r.b.byte = byte; r.b.ordinal = ordinal; r.b.first_bad = -1; r.b.bad_count = 0;
    r.owner = owner; r.stream = stream;
    g_guard_live.push_back(r);
    g_guard_count.fetch_add(1, std::memory_order_release);
}
// copies the band to the host and compares there (the caller has synchronised whatever may still write); false: a copy failed
static bool guard_check_band(ipm_guard_band& b) {
    std::vector<unsigned char> host((size_t)b.bytes);
    if (hipSetDevice(b.device) != hipSuccess || hipMemcpy(host.data(), (const void*)(uintptr_t)b.address, (size_t)b.bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        b.first_bad = 0; b.bad_count = -1;           // unreadable counts as damaged
        return false;
    }
    guard_compare(host.data(), (size_t)b.bytes, b.byte, &b.first_bad, &b.bad_count);
    return true;
}
// Takes the records `match` selects out of the registry, compares their bands and appends the damaged ones to the log.
template <class Match> static void guard_release(Match match) {
    std::vector<GuardRec> mine;
    {
        std::lock_guard<std::mutex> lock(g_guard_mutex);
        for (size_t i = 0; i < g_guard_live.size();)
            if (match(g_guard_live[i])) { mine.push_back(g_guard_live[i]); g_guard_live[i] = g_guard_live.back(); g_guard_live.pop_back(); g_guard_count.fetch_sub(1, std::memory_order_release); }
            else ++i;
    }
    for (GuardRec& r : mine) {
        guard_check_band(r.b);
        if (r.b.bad_count != 0) { std::lock_guard<std::mutex> lock(g_guard_mutex); g_guard_log.push_back(r.b); }
    }
}
// The ONE allocation and the one release behind dev_malloc / dev_free and LuRun (host_lu.h); pool: from the library's stream-ordered
// pool, else hipMalloc / hipFree.  The pointer handed out stays 256-byte aligned (the band is a multiple of 256).
static hipError_t guarded_alloc(int device, hipStream_t stream, void** p, size_t bytes, bool pool, const char* file, int line) {
    const GuardKnob g = alloc_guard();
    hipError_t e = pool ? hipMallocFromPoolAsync(p, bytes + 2 * g.band, g_pool[device], stream) : hipMalloc(p, bytes + 2 * g.band);
    if (e != hipSuccess || g.band == 0) return e;
    char* outer = (char*)*p;
    char* inner = outer + g.band;
    *p = inner;
    if ((e = hipMemsetAsync(outer, g.byte, g.band, stream)) != hipSuccess || (e = hipMemsetAsync(inner + bytes, g.byte, g.band, stream)) != hipSuccess) {
        if (pool) (void)hipFreeAsync(outer, stream); else (void)hipFree(outer);
        *p = nullptr;
        return e;
    }
    const char* base = strrchr(file, '/');
    char tag[96];
    std::lock_guard<std::mutex> lock(g_guard_mutex);
    const int ordinal = g_guard_ordinal++;
    snprintf(tag, sizeof tag, "%s:%d#%d", base ? base + 1 : file, line, ordinal);
    guard_register(nullptr, stream, tag, 0, outer, g.band, inner, bytes, device, g.byte, ordinal);
    guard_register(nullptr, stream, tag, 1, inner + bytes, g.band, inner, bytes, device, g.byte, ordinal);
    return hipSuccess;
}
static void guarded_free(hipStream_t stream, void* p, bool pool) {
    if (!p) return;
    if (g_guard_count.load(std::memory_order_acquire) > 0) {           // (a block allocated with the knob unset is in no record)
        void* outer = nullptr;
        {
            std::lock_guard<std::mutex> lock(g_guard_mutex);
            for (const GuardRec& r : g_guard_live)
                if (!r.owner && r.b.side == 0 && r.b.inner == (uint64_t)(uintptr_t)p) outer = (void*)(uintptr_t)r.b.address;
        }
        if (outer) {
            (void)hipStreamSynchronize(stream);
            guard_release([p](const GuardRec& r) { return !r.owner && r.b.inner == (uint64_t)(uintptr_t)p; });
            p = outer;
        }
    }
    if (pool) (void)hipFreeAsync(p, stream); else (void)hipFree(p);
}
static hipError_t dev_malloc(int device, hipStream_t stream, void** p, size_t bytes, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    if (bytes == 0) bytes = 16;
    const hipError_t e = guarded_alloc(device, stream, p, bytes, async_alloc_ok(device), file, line);
    return e != hipSuccess ? e : alloc_fill(*p, bytes, stream);
}
static void dev_free(int device, hipStream_t stream, void* p) {
    if (!p) return;
    guarded_free(stream, p, async_alloc_ok(device));
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
    // the regions in address order, and the guard band between them (IPM_TEST_ALLOC_GUARD; 0 when unset: the regions lie back to back)
    struct Region { const char* name; size_t off, bytes; };
    static const int MAX_REGIONS = 24;
    Region reg[MAX_REGIONS];
    int nreg;
    size_t band;
    int band_byte;
};
static const int N_NVEC = 11;   // x s c rc d v q dxa dsa dx ds
static const int N_MVEC = 7;    // y b rb t1 t2 dya dy

// no_dense: the handle factors with the sparse multifrontal Cholesky (IPM_FLAG_SPARSE_FACTOR on a sparse handle beyond the fused
// small-LP size) -- B, inv(L_kk) and the split-K slab are not part of the workspace; ensure_dense_B allocates them if a
// dense entry point (ipm_form_normal_matrix, ipm_get_factor, ipm_solve_linear) is ever called on such a handle.
static bool layout_no_dense(int64_t m, int64_t sparse_nnz, unsigned flags) { return sparse_nnz > 0 && (flags & IPM_FLAG_SPARSE_FACTOR) && m > 128; }
static Layout make_layout(int64_t m, int64_t n, int64_t sparse_nnz = 0, bool no_dense = false, const GuardKnob guard = alloc_guard()) {
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
    L.band = guard.band; L.band_byte = guard.byte; L.nreg = 0;
    size_t off = L.band;                          // a band before the first region, one behind every region
    auto take = [&](const char* name, size_t bytes) { size_t o = off; L.reg[L.nreg++] = Layout::Region{name, o, bytes}; off += (bytes + 255) / 256 * 256 + L.band; return o; };
    if (sparse_nnz > 0) { L.rc_chunks = 1; L.rows_per_chunk = (int)L.mp; }
    L.off_A = take("ws:A", sparse_nnz > 0 ? 0 : sizeof(double) * L.mp * L.np);
    L.off_B = take("ws:B", no_dense ? 0 : sizeof(double) * L.mp * L.mp);
    L.off_inv = take("ws:inv", no_dense ? 0 : sizeof(double) * L.nblk * NB * NB);
    L.off_nvec = take("ws:nvec", sizeof(double) * L.np * N_NVEC);
    L.off_mvec = take("ws:mvec", sizeof(double) * L.mp * N_MVEC);
    L.off_atp = take("ws:atp", sizeof(double) * L.rc_chunks * L.np);
    L.off_part = take("ws:part", sizeof(double) * P_NSLOT_DETECT_QUAD * MAXPART);     // (the slots of the infeasibility tests included, a quadratic handle's two too)
    L.off_det = take("ws:det", sizeof(double) * 4);
    L.off_sc = take("ws:sc", sizeof(Scalars));
    L.off_fixed = take("ws:fixed", 256);
    L.off_hist = take("ws:hist", sizeof(IterRec) * HIST_CAP);
    L.off_snap = take("ws:snap", sizeof(double) * (2 * L.np + L.mp) + sizeof(Scalars));
    L.off_slab = take("ws:slab", no_dense ? 0 : sizeof(double) * (size_t)kSlabTiles * 128 * 128);   // split-K partial tiles (64 MB)
    L.off_order = take("ws:order", sizeof(int) * ((size_t)L.nblk * (L.nblk + 1) / 2));
    L.off_rowptr = take("ws:rowptr", sparse_nnz > 0 ? sizeof(int) * (m + 1) : 0);
    L.off_colptr = take("ws:colptr", sparse_nnz > 0 ? sizeof(int) * (n + 1) : 0);
    L.off_colind = take("ws:colind", sparse_nnz > 0 ? sizeof(int) * sparse_nnz : 0);
    L.off_rowind = take("ws:rowind", sparse_nnz > 0 ? sizeof(int) * sparse_nnz : 0);
    L.off_rval = take("ws:rval", sparse_nnz > 0 ? sizeof(double) * sparse_nnz : 0);
    L.off_cval = take("ws:cval", sparse_nnz > 0 ? sizeof(double) * sparse_nnz : 0);
    L.total = off;
    return L;
}

__global__ void set_params_kernel(Scalars* sc, double e1, double e2, double e3, double eta, int max_iter,
                                  int force, int reset) { start_solve(sc, e1, e2, e3, eta, max_iter, force, reset); }

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

static FreeArgs free_args(const ipm_handle* h) { return FreeArgs{h->free_set.mark, (int)h->free_set.cols.size()}; }
static FreeLpArgs free_lp_args(const ipm_handle* h) { return FreeLpArgs{FreeArgs{h->free_lp_set.mark, (int)h->free_lp_set.cols.size()}, h->free_lp_rho}; }

// centrality correctors: views into mcc.mem.  mcc_vec_args / mcc_bnd_args are the handle's views with the candidate's arrays in place.
static const int MCC_NVECS = 11;
static size_t mcc_doubles(const ipm_handle* h) { return (size_t)MCC_NVECS * h->np + (size_t)h->mp + 2 * MAXPART + 2 * MCC_CTL_DOUBLES; }
static VecArgs mcc_vec_args(ipm_handle* h) {
    const size_t np = (size_t)h->np;
    double* p = h->mcc.mem;
    VecArgs c = vec_args(h);
    c.q = p; c.v = p + np; c.dx = p + 2 * np; c.ds = p + 3 * np; c.dy = p + MCC_NVECS * np;
    return c;
}
static BndArgs mcc_bnd_args(ipm_handle* h) {
    const size_t np = (size_t)h->np;
    double* p = h->mcc.mem;
    BndArgs b = bnd_args(h);
    b.qz = p + 6 * np; b.dw = p + 7 * np; b.dz = p + 8 * np;
    return b;
}
static MccArgs mcc_args(ipm_handle* h, int first) {
    const size_t np = (size_t)h->np;
    double* p = h->mcc.mem;
    MccArgs g;
    g.r3 = p + 4 * np; g.r3g = p + 5 * np; g.r4 = p + 9 * np; g.r4g = p + 10 * np;
    g.part = p + MCC_NVECS * np + (size_t)h->mp; g.ctl = h->mcc.ctl(h); g.first = first;
    return g;
}

// iterative refinement: views into ref.mem
struct RefViews { double *t, *r, *delta, *dy_keep, *atp_keep, *atd, *part; RefCtl* ctl; };
static size_t ref_na(const ipm_handle* h) { return (size_t)h->rc_chunks * h->np; }
static size_t ref_doubles(const ipm_handle* h) { return 4 * (size_t)h->mp + 2 * ref_na(h) + 2 * (size_t)(h->mp / REF_ROWS) + 2 * REF_CTL_DOUBLES; }
static RefViews ref_views(const ipm_handle* h) {
    const size_t mp = (size_t)h->mp, na = ref_na(h);
    double* p = h->ref.mem;
    RefViews v;
    v.t = p; v.r = p + mp; v.delta = p + 2 * mp; v.dy_keep = p + 3 * mp; v.atp_keep = p + 4 * mp; v.atd = v.atp_keep + na;
    v.part = v.atd + na; v.ctl = h->ref.ctl(h);
    return v;
}

static DetArgs det_args(const ipm_handle* h) { return DetArgs{h->det_eps_p, h->det_eps_d, h->det}; }

// ------------------------------------------------------------------------------- the handle's problem class and its arguments
// The ONE place that reads the five class switches of a handle in order to choose a kernel (vector_ops.h: StepVariant and the
// variant tables; the legality rule free => quad is variant_legal, which check_ready and the small batch's own check enforce before
// a launch).  Every other reader of these fields keeps data in step with them: the setters, equilibration, the roll-back copies
// of (w, z), the refusals.
static StepVariant step_variant(const ipm_handle* h) { return StepVariant{h->bnd, h->detect, h->quad, h->free_set.on, h->free_lp_set.on}; }
// ... and the guard in front of every table look-up (the iteration's and the small path's entries call it before their first launch):
// a handle whose class is not legal has no row, and an entry point that forgot check_ready gets an error, not a null row.
static int check_class(ipm_handle* h, const char* who) {
    const unsigned bits = variant_bits(step_variant(h));
    if (variant_legal(bits)) return IPM_OK;
    if (bits & V_L) return fail(h, IPM_ERR_STATE, "%s: LP free columns beside a quadratic term, free columns with curvature or the infeasibility tests: no kernel serves that class", who);
    return fail(h, IPM_ERR_STATE, "%s: free columns without a quadratic term: no kernel serves that class", who);
}

// A handle at a step, as a source of kernel arguments (vector_ops.h: Pick): each argument group by its type, int = the step's corr.
struct StepSrc { ipm_handle* h; int corr; };
template <> struct Pick<VecArgs, StepSrc> { static VecArgs of(const StepSrc& s) { return vec_args(s.h); } };
template <> struct Pick<BndArgs, StepSrc> { static BndArgs of(const StepSrc& s) { return bnd_args(s.h); } };
template <> struct Pick<DetArgs, StepSrc> { static DetArgs of(const StepSrc& s) { return det_args(s.h); } };
template <> struct Pick<const double*, StepSrc> { static const double* of(const StepSrc& s) { return s.h->quad_g; } };
template <> struct Pick<FreeArgs, StepSrc> { static FreeArgs of(const StepSrc& s) { return free_args(s.h); } };
template <> struct Pick<FreeLpArgs, StepSrc> { static FreeLpArgs of(const StepSrc& s) { return free_lp_args(s.h); } };
template <> struct Pick<int, StepSrc> { static int of(const StepSrc& s) { return s.corr; } };
// ... and the argument structs of the vector steps' lockstep twins (lockstep.h)
inline LsVecA::LsVecA(ipm_handle* h, int corr_) : a(vec_args(h)), corr(corr_) {}
inline LsVecDet::LsVecDet(ipm_handle* h, int) : a(vec_args(h)), dt(det_args(h)) {}
inline LsVecBnd::LsVecBnd(ipm_handle* h, int corr_) : a(vec_args(h)), corr(corr_), bd(bnd_args(h)) {}
inline LsVecBndDet::LsVecBndDet(ipm_handle* h, int) : a(vec_args(h)), bd(bnd_args(h)), dt(det_args(h)) {}
