// host_factor_solve.h -- host side, unit 4: formation of B = A D A^T, the launches of the dense blocked Cholesky (its look-ahead
// schedule is the step plan of chol_plan.h), of the sparse factor, the group inverses and the triangular sweeps.
#pragma once
static inline bool sp_on(const ipm_handle* h) { return h->spf && !h->spf_off; }
// Sparse factor: one launch per LEVEL of the panel tree (the kernel boundary is the hand-off, nothing spins) instead of one
// launch per sweep with flag hand-offs between tasks.  Chosen by IPM_SP_MODE=level, and automatically wherever the handle
// shares the device -- IPM_FLAG_NO_DEVICE_POLLING (batched mode) or more than one live handle: spinning consumers next to
// other LPs' kernels are what turned STOCFOR3's 0.10 s into 1.4-1.7 s in a shared run, and the level form measured equal
// under contention (73-LP suite 3.11-3.15 s vs 3.20-3.32 s).  Same arithmetic, bit-identical results.
static inline bool sp_level(const ipm_handle* h) {
    if (h->sp_serial || h->sp_level_mode < 0) return false;
    if (h->sp_level_mode > 0 || (h->opt.flags & IPM_FLAG_NO_DEVICE_POLLING)) return true;
    return !alone_on_device(h);
}
static inline unsigned sp_launch_grid(ipm_handle* h) {
    if (h->sp_serial) { ++h->sp_serial_launches; return 1u; }
    return (unsigned)h->sp_grid;
}
// The launches of one walk of the panel tree, launch(grid, recs, count).  by_level: one launch per level, leaves or root first,
// of min(level's records, sp_grid) workgroups -- the kernel boundary is the hand-off (~5 us against ~8-20 us for a flag hand-off
// inside one launch), nothing spins, concurrent handles interleave at launch granularity.  Else (task mode) one launch over all records.
template <class Launch>
static void sp_walk(ipm_handle* h, bool by_level, bool leaves_first, Launch launch) {
    if (!by_level) { launch(sp_launch_grid(h), h->spF.rec, 0); return; }
    const size_t nlev = h->sp_lvlptr.empty() ? 0 : h->sp_lvlptr.size() - 1;
    for (size_t i = 0; i < nlev; ++i) {
        const size_t l = leaves_first ? i : nlev - 1 - i;
        const int cnt = h->sp_lvlptr[l + 1] - h->sp_lvlptr[l];
        launch((unsigned)std::min(cnt, h->sp_grid), h->sp_rec_level + h->sp_lvlptr[l], cnt);
    }
}

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

// B = A diag(d) A^T (lower tiles), unit diagonal on padding rows
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
        launch_twin<LS_ZERO>(h, zgrid, {h->B, nB, &h->sc->done});
        const int work = h->sm_nb + (int)(h->mp - h->m);
        launch_twin<LS_ADAT_LIST>(h, (unsigned)((work + 255) / 256), {h->sm_bptr, h->ls_bi, h->ls_bk, h->sm_bcol, h->sm_bcoef, h->ls_bak, h->sm_nb, d, h->B, h->mp, (int)h->m, (int)h->mp, &h->sc->done});
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    if (h->sparse) {
        const LsAdatSp ps{sparse_view(h), d, h->B, h->mp, (int)h->mp, &h->sc->done};
        if (h->mp <= SP_LDS_MAX_MP) launch_twin<LS_ADAT_SPARSE>(h, (unsigned)h->mp, ps, nullptr, (unsigned)(h->mp * sizeof(double)));   // dynamic-LDS attribute set per device in ipm_create
        else launch_twin<LS_ADAT_SPARSE_GLOBAL>(h, (unsigned)h->mp, ps);
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    // the dedicated software-pipelined kernel (adat_syrk_f64.h; the generic gemm_nt kernel it replaced in round 2 computes the same bits)
    HIP_TRY(h, launch_adat_syrk(h->A, h->np, d, h->B, h->mp, (int)h->mp, (int)h->np, (int)h->m, factor_done(h),
                                h->d_tile_order, h->stream, h->slab, 512));
    return IPM_OK;
}

// X_g, XT_g = inv of every 1024 x 1024 diagonal group of the factor and its transpose (trsv_grouped.h):
// recursive doubling 128 -> 256 -> 512 -> 1024, batched over (pairs in a group, groups): per level one launch for S and one
// that produces X21 and XT12 together (ginv_gemm_f64.h).  The three-launch form on the generic kernel computes the same bits;
// it is what a lockstep program records (its kernels have twins) and what IPM_GINV_REF=1 selects, the reference of
// tests/test_gpu_group_inverse.py.  After enqueue_factor, on the main stream.
static int enqueue_group_inverses(ipm_handle* h, int g0 = 0, int g1 = -1, hipStream_t st = nullptr) {
    if (sp_on(h)) return IPM_OK;
    if (!h->grouped_trsv) return IPM_OK;
    const int GS = h->gsz;
    const int64_t GR = (int64_t)GS * 128;
    if (g1 < 0) g1 = h->nblk / GS;
    if (!st) st = h->stream;
    const int nG = g1 - g0;                               // groups [g0, g1)
    if (nG <= 0) return IPM_OK;
    const int* done = factor_done(h);                     // (the inverses belong to the factor: whole or not at all, like it)
    launch_twin<LS_GROUP_DIAG_T>(h, 16u * (unsigned)(nG * GS), {h->invD, h->gXT, h->gX, g0 * GS, GS, done}, st);
    const int64_t gXs = GR * GR, gL = GR * (h->mp + 1), gSs = (GR / 2) * (GR / 2);   // group strides in X/XT, L, S
    double* gXT = h->gXT + g0 * gXs; double* gX = h->gX + g0 * gXs; double* gS = h->gS + g0 * gSs;
    const double* Lg = h->B + g0 * gL;
    const bool three_launches = h->ginv_ref || g_gemm_recorder;
    for (int hs = 128; hs < GR; hs *= 2) {
        const int np = (int)(GR / (2 * hs));              // pairs per group
        const int64_t pX = (int64_t)2 * hs * (GR + 1);                                 // pair strides in X, XT
        const int64_t pL = (int64_t)2 * hs * (h->mp + 1);
        const int64_t pS = (int64_t)hs * hs;
        if (!three_launches) {
            GinvGemm a{};                                 // S = XT11 * L21^T
            a.hs = hs; a.alpha = 1.0; a.done = done;
            a.P = gXT; a.ldp = GR; a.sP = pX; a.sP2 = gXs;
            a.Q = Lg + (int64_t)hs * h->mp; a.ldq = h->mp; a.sQ = pL; a.sQ2 = gL;
            a.C = gS; a.ldc = hs; a.sC = pS; a.sC2 = gSs;
            HIP_TRY(h, launch_ginv_gemm<false>(a, np, nG, st));
            GinvGemm b{};                                 // X21 = -X22 * S^T and XT12 = -S * X22^T
            b.hs = hs; b.alpha = -1.0; b.done = done;
            b.P = gX + (int64_t)hs * GR + hs; b.ldp = GR; b.sP = pX; b.sP2 = gXs;
            b.Q = gS; b.ldq = hs; b.sQ = pS; b.sQ2 = gSs;
            b.C = gX + (int64_t)hs * GR; b.ldc = GR; b.sC = pX; b.sC2 = gXs;
            b.CT = gXT + hs; b.ldct = GR; b.sCT = pX; b.sCT2 = gXs;
            HIP_TRY(h, launch_ginv_gemm<true>(b, np, nG, st));
            continue;
        }
        GemmNT t = gemm_defaults();
        t.done = done;
        t.M = hs; t.N = hs; t.K = hs; t.batch = np; t.batch2 = nG;
        GemmNT a = t;                                    // S = XT11 * L21^T
        a.P = gXT; a.ldp = GR; a.sP = pX; a.sP2 = gXs;
        a.Q = Lg + (int64_t)hs * h->mp; a.ldq = h->mp; a.sQ = pL; a.sQ2 = gL;
        a.C = gS; a.ldc = hs; a.sC = pS; a.sC2 = gSs;
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

// Dense-column split behind a factorization of B_s (dense_split.h): V from the handle's CSC copy of the dense columns
// and the d the formation used (h->d at every call site), W = L^-1 V in ONE walk of the panel tree -- always the level form, one
// launch per level whatever IPM_SP_MODE says: nothing spins, so the time-out machinery has nothing to cover -- then the Gram
// partials and the Schur factor R.  k = 1: the walk runs sp_fwd_kernel itself on the split's update vectors.
static int enqueue_dense_split_factor(ipm_handle* h) {
    const DsSplit& s = h->dsp;
    const int* done = h->spF.done;
    hipLaunchKernelGGL(ds_scatter_kernel, dim3((unsigned)s.k), dim3(DS_THREADS), 0, h->stream, h->d_colptr, h->d_rowind, h->d_cval, h->d, s, done);
    const int rm = std::max(16, h->sp_rmax);
    SpFactor F = h->spF;
    F.uvec = s.uvec;
    sp_walk(h, /*by_level=*/true, /*leaves_first=*/true, [&](unsigned grid, const SpRec* recs, int count) {
        if (s.k == 1) hipLaunchKernelGGL((sp_fwd_kernel<SPC_THREADS>), dim3(grid), dim3(SPC_THREADS), h->sp_lds_solve, h->stream, F, 0u, s.V, s.W, rm, recs, count);
        else hipLaunchKernelGGL((ds_fwd_kernel<SPC_THREADS>), dim3(grid, (unsigned)s.k), dim3(SPC_THREADS), h->sp_lds_solve, h->stream, F, s, rm, recs, count);
    });
    hipLaunchKernelGGL(ds_gram_kernel, dim3((unsigned)s.nchunk), dim3(DS_THREADS), 0, h->stream, s, done);
    hipLaunchKernelGGL(ds_schur_kernel, dim3(1), dim3(DS_THREADS), 0, h->stream, s, done);
    ++h->ds_factorizations;
    return IPM_OK;
}
// The correction of a solve between its sweeps: z -= W (R R^T)^-1 W^T z on z = L^-1 t.
static void enqueue_dense_split_correction(ipm_handle* h, double* z) {
    const DsSplit& s = h->dsp;
    hipLaunchKernelGGL(ds_wtz_kernel, dim3((unsigned)s.nchunk), dim3(DS_THREADS), 0, h->stream, s, z, solve_done(h));
    hipLaunchKernelGGL(ds_apply_kernel, dim3((unsigned)s.nchunk), dim3(DS_THREADS), 0, h->stream, s, z, solve_done(h));
    ++h->ds_corrections;
}

// Multifrontal sparse Cholesky: one launch walks the elimination tree.
// sp_fwd_rhs: right-hand side whose forward substitution rides on the factorization (z -> h->t2); the next enqueue_potrs of that
// right-hand side then runs the backward sweep only (h->sp_fwd_fused).
static int enqueue_sparse_factor(ipm_handle* h, const double* sp_fwd_rhs) {
    if (!h->sp_fuse_fwd) sp_fwd_rhs = nullptr;
    h->sp_fwd_fused = sp_fwd_rhs;
    const unsigned ep = ++h->sp_epoch;
    sp_walk(h, sp_level(h), /*leaves_first=*/true, [&](unsigned grid, const SpRec* recs, int count) {
        hipLaunchKernelGGL((sp_chol_kernel<SPC_THREADS>), dim3(grid), dim3(SPC_THREADS), h->sp_lds_chol, h->stream, h->spF, ep,
                           &h->sc->maxdiag, h->opt.pivot_guard_eps, h->opt.pivot_guard_big, h->shift_rel, &h->sc->fixed,
                           h->sp_lds_doubles, recs, count, sp_fwd_rhs, h->t2, h->sp_fv_off);
    });
    if (h->ds_on) { if (int rc_ = enqueue_dense_split_factor(h)) return rc_; }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// "Which kernel runs the trailing update", stated once: chol_update_kernel, or the generic kernel of rounds 1-2 (IPM_BULK_VARIANT=7)
static hipError_t launch_trailing_update(const ipm_handle* h, const GemmNT& g, hipStream_t stream, int skip_first) {
    if (h->bulk_variant == 7) return launch_gemm_nt<128, 128, 16, 2, 2>(g, stream, nullptr, 512, skip_first);
    return launch_chol_update(g, stream, skip_first);
}

// blocked guarded Cholesky of B in place (lower).  The schedule -- groups, envelope clip, step shapes, which hand-off is a counter
// and which an event, every polled count -- is chol_step_plan (chol_plan.h); this function walks the plan, fills the
// argument structs from a step's record and launches.  mid_step / ginv_step: block steps at which the caller's residual stream
// and the inverses of the complete groups start (host_iteration.h); they are hooks of the call site, not schedule.
// sp_fwd_rhs: see enqueue_sparse_factor (sparse factor only).
static int enqueue_factor(ipm_handle* h, int mid_step = -1, int ginv_step = -1, const double* sp_fwd_rhs = nullptr) {
    if (sp_on(h)) return enqueue_sparse_factor(h, sp_fwd_rhs);
    if (int rc_ = ensure_dense_B(h)) return rc_;
    const int* done = factor_done(h);
    // threshold scale = max diag over the TRUE rows only (padding rows carry a unit diagonal)
    launch_twin<LS_MAXDIAG>(h, 1u, {h->B, h->mp, (int)h->m, &h->sc->maxdiag, done});
    const CholPlan plan = chol_step_plan(h->nblk, h->m, h->mp, lookahead_on(h), polls_device(h), h->two_level, h->group_steps,
                                         h->ss_small_blocks, h->shift_rel != 0.0, h->use_env ? h->env_last.data() : nullptr);
    h->last_gs = plan.gs; h->n_counter_steps = plan.n_counter_steps; h->n_event_steps = plan.n_event_steps;
    hipStream_t sm = h->stream, sb = plan.lookahead ? h->stream2 : h->stream;
    unsigned* const bulk_done = h->d_bulk_done;                     // counters: [k] bulk update of step k, [nblk + k] its critical panel
    if (plan.polling) HIP_TRY(h, hipMemsetAsync(bulk_done, 0, sizeof(unsigned) * 2 * (size_t)h->nblk, sm));
    if (plan.lookahead) {
        HIP_TRY(h, hipEventRecord(h->ev_fork, sm));
        HIP_TRY(h, hipStreamWaitEvent(sb, h->ev_fork, 0));
    }
    for (int k = 0; k < h->nblk; ++k) {
        const CholStep& s = plan.steps[k];
        PotrfDiag pd;
        pd.Bkk = h->B + (int64_t)k * NB * (h->mp + 1); pd.ld = h->mp;
        pd.inv = h->invD + (int64_t)k * NB * NB;
        pd.maxdiag = &h->sc->maxdiag; pd.eps = h->opt.pivot_guard_eps; pd.big = h->opt.pivot_guard_big; pd.shift_rel = h->shift_rel;
        pd.fixed = &h->sc->fixed; pd.done = done; pd.stamps = nullptr;
        pd.wait_on = nullptr; pd.wait_count = 0; pd.signal = nullptr; pd.timeout = nullptr; pd.dbg = nullptr; pd.dbg_tag = 0;
        pd.trace = nullptr;
        pd.nt = s.potrf_panels;
        pd.rows = s.rows;
        if (h->stamp_buf && k == 0) {                               // (IPM_POTRF_STAMPS: the stamping instantiation has no twin)
            pd.stamps = h->stamp_buf;
            if (getenv("IPM_POTRF_SKIP")) pd.dbg_tag = (unsigned)atoi(getenv("IPM_POTRF_SKIP"));
            launch_untwinned(h, potrf_diag_kernel<true>, dim3(1), dim3(PD_THREADS), sm, pd);
        } else launch_twin<LS_POTRF>(h, 1u, pd, sm);
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
        if (s.rem <= 0) {                                           // the last block column, or nothing below the diagonal block in this one
            if (s.bulk_event) HIP_TRY(h, hipEventRecord(h->ev_bulk[k], sb));
            continue;
        }
        double* panel = h->B + (int64_t)(k + 1) * NB * h->mp + (int64_t)k * NB;
        GemmNT t = gemm_defaults();                                 // L_ik = B_ik inv(L_kk)^T, in place
        t.P = panel; t.ldp = h->mp; t.Q = pd.inv; t.ldq = NB;
        t.C = panel; t.ldc = h->mp; t.M = s.rem; t.N = NB; t.K = NB;
        t.lower = 0; t.done = done;
        GemmNT u = gemm_defaults();                                 // B_ij -= L_ik L_jk^T: block columns k-kcols+1 .. k of L, rows >= k+1
        u.P = panel - (int64_t)(s.kcols - 1) * NB; u.ldp = h->mp; u.Q = u.P; u.ldq = h->mp;
        u.C = h->B + (int64_t)(k + 1) * NB * (h->mp + 1); u.ldc = h->mp; u.M = s.rem; u.N = s.rem; u.K = s.kcols * NB;
        u.alpha = -1.0; u.beta = 1.0; u.lower = 1; u.done = done;
        if (s.shape == CS_NARROW) {
            HIP_TRY(h, (launch_gemm_nt<32, 128, 32, 1, 8>(t, sm)));
            HIP_TRY(h, (launch_gemm_nt<64, 64, 16, 2, 2>(u, sm)));
        } else if (s.shape == CS_WIDE) {
            HIP_TRY(h, (launch_gemm_nt<64, 128, 16, 2, 2>(t, sm)));
            HIP_TRY(h, launch_trailing_update(h, u, sm, 0));
        } else {
            // one event per step on the main stream (after the critical panel rows): every extra record / wait
            // costs the pivot chain ~6-12 us of command-processor time (profiles/, trace of a step)
            GemmNT tc = t; tc.M = NB;                               // critical panel rows: block row k+1
            if (s.crit_wait == CH_COUNTER) { tc.wait_on = bulk_done + (k - 1); tc.wait_count = (unsigned)s.crit_count; tc.timeout = timeout_word(h); }
            else if (s.crit_wait == CH_EVENT) HIP_TRY(h, hipStreamWaitEvent(sm, h->ev_bulk[k - 1], 0));
            if (s.crit_flag) tc.signal = bulk_done + h->nblk + k;
            // NOTE the panel solve is IN PLACE (C = P): a workgroup must own whole rows, i.e. BN == N == 128.  Tiles narrower
            // than the panel (tried: 16 workgroups of 32 x 32) race -- one workgroup overwrites columns another still reads.
            HIP_TRY(h, (launch_gemm_nt<32, 128, 32, 1, 8>(tc, sm)));     // 8 waves, BK=32: 4 stages
            if (!s.crit_flag) HIP_TRY(h, hipEventRecord(h->ev_crit[k], sm));
            GemmNT uc = u; uc.M = NB; uc.N = NB;                    // critical tile (k+1,k+1)
            HIP_TRY(h, (launch_gemm_nt<32, 32, 32, 2, 2>(uc, sm)));      // 10 sub-tiles of 32x32
            if (!s.crit_flag) HIP_TRY(h, hipStreamWaitEvent(sb, h->ev_crit[k], 0));
            if (s.bulk != CH_NONE) {
                GemmNT tb = t; tb.C = panel + (int64_t)NB * h->mp; tb.P = tb.C; tb.M = s.rem - NB;
                if (s.crit_flag) { tb.wait_on = bulk_done + h->nblk + k; tb.wait_count = (unsigned)s.poll_count; tb.timeout = timeout_word(h); }
                HIP_TRY(h, (launch_gemm_nt<64, 128, 16, 2, 2>(tb, sb)));
                GemmNT ub = u;
                if (s.window) {                                     // tiles (i, j), i >= k+2, k+1 <= j < k+1+window, as one rectangular GEMM
                    ub.P = tb.C; ub.Q = panel;
                    ub.C = h->B + (int64_t)(k + 2) * NB * h->mp + (int64_t)(k + 1) * NB;
                    ub.M = s.rem - NB; ub.N = s.window * NB; ub.lower = 0;
                }
                if (s.bulk == CH_COUNTER) ub.signal = bulk_done + k;
                HIP_TRY(h, launch_trailing_update(h, ub, sb, /*skip_first=*/s.window ? 0 : 1));
            }
        }
        if (s.bulk_event) HIP_TRY(h, hipEventRecord(h->ev_bulk[k], sb));
    }
    if (plan.lookahead) HIP_TRY(h, hipStreamWaitEvent(sm, h->ev_bulk[h->nblk - 2], 0));
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// signal (optional): the launch is the signalling entry point and stores `value` to that progress word at its entry (SweepHook below)
static void launch_dense_gemv_n(ipm_handle* h, const double* A, int64_t lda, int rows, int cols, const double* v, double sa,
                                double sb, const double* add, double* out, unsigned* signal = nullptr, unsigned value = 0) {
    if (signal) hipLaunchKernelGGL(gemv_n_signal_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, h->stream, A, lda, rows, cols, v, sa, sb, add, out, solve_done(h), signal, value);
    else launch_twin<LS_GEMV_N>(h, (unsigned)((rows + 3) / 4), {A, lda, rows, cols, v, sa, sb, add, out, solve_done(h)});
}

// Block-step substitution over the blocks [k0, nblk), one launch per block step: forward sweep L z = r, then the backward sweep
// L^T out = z inside the envelope.  k0 = 0 is the whole solve; k0 > 0 the blocks behind the last full group (ragged groups).
static void enqueue_block_steps(ipm_handle* h, int k0, double* r, double* z, double* out) {
    TrsvStep a;
    a.L = h->B; a.ld = h->mp; a.inv = h->invD; a.done = solve_done(h);
    a.r = r; a.z = z; a.j0 = 0;
    for (int k = k0; k < h->nblk; ++k) {
        a.k = k;
        const int nb = h->use_env ? h->env_last[k] - k + 1 : h->nblk - k;
        launch_twin<LS_TRSV_FWD>(h, (unsigned)nb, a);
    }
    a.r = z; a.z = out;
    for (int k = h->nblk - 1; k >= k0; --k) {
        a.k = k;
        a.j0 = h->use_env ? h->env_first[k] : 0;
        launch_twin<LS_TRSV_BWD>(h, (unsigned)(k - a.j0 + 1), a);
    }
}

// The backward sweep of the grouped solve makes `out` final from its last row upwards, in EVENTS: first the block steps behind the
// last full group (ragged block counts: rows >= nG * GR), then the groups nG-1 .. 0 (rows >= g * GR), each with its diagonal
// gemv_n.  A pass over A that reads `out` by row chunks (gemv_t_kernel: chunk `by` = rows by * rows_per_chunk ...) can follow the
// events: a chunk is computable once ALL its rows lie at or above the event's first final row, so a chunk that straddles a
// boundary goes with the later event.  One entry per event, in sweep order: the first final row and the row chunks [chunk0, chunk1)
// that become computable (empty where a chunk is taller than what the event adds).  The chunks of the LAST event (row 0) are what
// is left when the sweep has ended.  Empty result: the chunks do not tile the rows (no caller then cuts the pass).
struct AtPiece { int first_row, chunk0, chunk1; };
static std::vector<AtPiece> at_piece_schedule(int64_t mp, int gsz, int nblk, int rc_chunks, int rows_per_chunk) {
    std::vector<AtPiece> ev;
    if (gsz <= 0 || nblk < gsz || rc_chunks <= 0 || rows_per_chunk <= 0 || (int64_t)rc_chunks * rows_per_chunk != mp || mp != (int64_t)nblk * NB) return ev;
    const int nG = nblk / gsz;
    const int64_t GR = (int64_t)gsz * NB;
    int hi = rc_chunks;
    auto event = [&](int64_t first) {
        const int lo = (int)std::min<int64_t>(hi, (first + rows_per_chunk - 1) / rows_per_chunk);
        ev.push_back({(int)first, lo, hi});
        hi = lo;
    };
    if (nblk > nG * gsz) event(nG * GR);
    for (int g = nG - 1; g >= 0; --g) event(g * GR);
    return ev;
}
// What a caller that follows the events hands to the sweep.  Event e (index into at_piece_schedule) is SIGNALLED by the kernel that
// follows its last kernel in the stream -- the sweep's gemv_t behind a group's diagonal gemv_n, the next diagonal gemv_n behind the
// block steps -- which is launched as the signalling entry point and stores base + e + 1 to `word` at its entry
// (handoff_signal_at_entry: no event record and no launch on the sweep's stream).  released(e) is called once that kernel is
// enqueued: whatever the caller enqueues to wait for the word is then BEHIND its releaser in enqueue order, the rule that keeps a
// device-side wait from deadlocking however streams map to hardware queues.  The last event is not signalled and not reported:
// the sweep has ended, its rows are the caller's to use in stream order.
struct SweepHook {
    unsigned* word;
    unsigned base;
    std::function<void(int)> released;
};

// out = B^{-1} r with the 1024-row group inverses: 4 group steps per sweep at m = 4096
// wait_last (optional): event after which the LAST group's inverse is available; the forward sweep over the earlier groups
// does not need it and runs ahead of the wait
static int enqueue_potrs_grouped(ipm_handle* h, double* r, double* out, hipEvent_t wait_last = nullptr, const SweepHook* hook = nullptr) {
    const int GS = h->gsz;
    const int GR = GS * 128;
    const int nG = h->nblk / GS;
    const int* done = solve_done(h);
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
    enqueue_block_steps(h, nG * GS, r, z, out);
    int e = 0;                                                            // next sweep event (at_piece_schedule)
    bool pending = hook && h->nblk > nG * GS;                             // event e is complete and the next kernel has to signal it
    for (int g = nG - 1; g >= 0; --g) {                                   // backward: L^T w = z
        launch_dense_gemv_n(h, h->gXT + (int64_t)g * GR * GR, GR, GR, GR, z + (int64_t)g * GR, 1.0, 0.0, nullptr, out + (int64_t)g * GR,
                            pending ? hook->word : nullptr, pending ? hook->base + (unsigned)e + 1u : 0u);
        if (pending) { hook->released(e); ++e; pending = false; }
        int left = g * GR;
        const int c0 = h->use_env ? std::min(left, h->env_first[g * GS] * NB) : 0;   // columns left of c0 are zero in these rows
        left -= c0;
        if (left > 0) {
            const unsigned gx = (unsigned)((left + 511) / 512);      // blocks per row chunk, 16 row chunks
            const LsArgs<LS_GEMV_T> t{h->B + (int64_t)g * GR * h->mp + c0, h->mp, GR / 16, left, out + (int64_t)g * GR, h->gPart, done, gx};
            if (hook) {                                              // group g's rows are final: this kernel signals it
                hipLaunchKernelGGL(gemv_t_signal_kernel, dim3(gx, 16u), dim3(256), 0, h->stream, t.A, t.lda, t.rows_per_chunk, t.np, t.u, t.part, t.done,
                                   hook->word, hook->base + (unsigned)e + 1u);
                hook->released(e); ++e;
            } else launch_twin<LS_GEMV_T>(h, gx * 16u, t);
            launch_twin<LS_SUB_PARTIALS>(h, (unsigned)((left + 255) / 256), {z + c0, h->gPart, left, 16, done});
        } else if (hook && g > 0) pending = true;                    // (envelope: nothing left of the group) the next diagonal gemv_n signals
    }
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}

// out = B^{-1} r  (r is consumed; uses t2 as the intermediate)
static int enqueue_potrs(ipm_handle* h, double* r, double* out, hipEvent_t wait_last = nullptr, const SweepHook* hook = nullptr) {
    if (sp_on(h)) {                     // forward and backward sweep over the elimination tree, one launch each
        const int rm = std::max(16, h->sp_rmax);
        unsigned ep = ++h->sp_epoch;
        const bool fwd_done = h->sp_fwd_fused != nullptr && h->sp_fwd_fused == r;       // the factorization carried L z = r already (z in t2)
        h->sp_fwd_fused = nullptr;
        const bool by_level = sp_level(h);                  // (evaluated once for both sweeps)
        SpFactor F = h->spF;                                // the sweeps test the word of whoever asks for the solve (solve_done)
        F.done = solve_done(h);
        if (!fwd_done) sp_walk(h, by_level, /*leaves_first=*/true, [&](unsigned grid, const SpRec* recs, int count) {
            hipLaunchKernelGGL((sp_fwd_kernel<SPC_THREADS>), dim3(grid), dim3(SPC_THREADS), h->sp_lds_solve, h->stream, F, ep, r, h->t2, rm, recs, count);
        });
        if (h->ds_on) enqueue_dense_split_correction(h, h->t2);      // (also behind a forward sweep that rode on the factorization)
        if (!by_level) ep = ++h->sp_epoch;                   // the level-mode sweeps share one epoch, task mode takes one per sweep
        sp_walk(h, by_level, /*leaves_first=*/false, [&](unsigned grid, const SpRec* recs, int count) {
            hipLaunchKernelGGL((sp_bwd_kernel<SPC_THREADS>), dim3(grid), dim3(SPC_THREADS), 0, h->stream, F, ep, h->t2, out, recs, count);
        });
        HIP_TRY(h, hipGetLastError());
        return IPM_OK;
    }
    if (h->grouped_trsv) return enqueue_potrs_grouped(h, r, out, wait_last, hook);      // (a hook is given to grouped sweeps only: stream_at_on)
    if (wait_last) HIP_TRY(h, hipStreamWaitEvent(h->stream, wait_last, 0));
    enqueue_block_steps(h, 0, r, h->t2, out);
    HIP_TRY(h, hipGetLastError());
    return IPM_OK;
}
