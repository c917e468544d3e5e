// host_fused.h -- host side, unit 5: the fused formation + factorization launch (form_factor.h, ff_schedule.h): selection rule,
// schedule + buffers, the launch itself, its debug exports and diagnostic dumps.
#pragma once
// ------------------------------------------------------------------------------- fused formation + factorization
// Can this iteration run the fused path?  (its hand-offs are device-polled: polls_device; a recovered poll time-out clears
// flag_sync and with it this path, for good; ff_min_nblk is 3 at least, so the size rule implies lookahead_on's nblk > 2)
static bool ff_ok(const ipm_handle* h) {
    if (!h->ff_enabled || h->sparse || !polls_device(h)) return false;
    if (h->nblk < h->ff_min_nblk || h->nblk > std::min(h->ff_max_nblk, FF_MAX_NBLK) || h->np % FF_PBK) return false;
    return h->ff_forced || h->np <= 6 * h->mp;
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
    h->ff_flag_words = FFWords(h->nblk).count;
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
    const int* done = factor_done(h);
    hipStream_t sw = h->stream;
    unsigned* F = h->d_ff_flags;
    const FFWords W(nblk);
    unsigned *ticket = F + W.ticket, *dbg = F + W.dbg, *fcount = F + W.fcount, *tprog = F + W.tprog, *lfinal = F + W.lfinal,
             *dready = F + W.dready, *potrfdone = F + W.potrfdone;
    unsigned* timeout = timeout_word(h);
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
    c.maxbits = (const unsigned long long*)(F + W.maxbits); c.dcount = F + W.dcount; c.maxdiag_out = &h->sc->maxdiag;
    c.dready = dready; c.potrfdone = potrfdone; c.timeout = timeout; c.dbg = dbg; c.trace = ctrace;
    c.eps = h->opt.pivot_guard_eps; c.big = h->opt.pivot_guard_big; c.shift_rel = h->shift_rel;
    c.fixed = &h->sc->fixed; c.done = done; c.nblk = nblk; c.m = (int)h->m;
    FFCrit& cc = roles.crit;
    cc.B = h->B; cc.ldb = h->mp; cc.invD = h->invD; cc.tprog = tprog; cc.tile_items = h->d_ff_tile_items;
    cc.potrfdone = potrfdone; cc.lfinal = lfinal; cc.dready = dready; cc.timeout = timeout; cc.dbg = dbg; cc.trace = ctrace;
    cc.done = done; cc.nblk = nblk;
    roles.role = F + W.role;
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
    a.maxbits = (unsigned long long*)(F + W.maxbits); a.dcount = F + W.dcount;
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

extern "C" int ipm_debug_get_group_inverse(ipm_handle* h, int32_t g, int32_t which, double* out) {
    if (!h || !out || which < 0 || which > 1) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_get_group_inverse: bad arguments");
    if (!h->grouped_trsv || !h->gX || !h->gXT) return fail(h, IPM_ERR_STATE, "the handle holds no group inverses");
    if (g < 0 || g >= h->nblk / h->gsz) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_get_group_inverse: no such group");
    const size_t GR = (size_t)h->gsz * 128;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, (which ? h->gXT : h->gX) + (size_t)g * GR * GR, sizeof(double) * GR * GR, hipMemcpyDeviceToHost, h->stream));
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

// IPM_FF_PROF=1: where the workers' cycles went (sum over the handle's fused launches); called from ipm_destroy
static void ff_dump_profile(ipm_handle* h) {
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

// IPM_FF_DEBUG after a hand-off time-out (read_scalars): where did the fused launch stop?  (hand-off words of the call's LAST factorization)
static void ff_dump_handoffs(ipm_handle* h) {
    std::vector<unsigned> F(h->ff_flag_words);
    (void)hipMemcpy(F.data(), h->d_ff_flags, sizeof(unsigned) * F.size(), hipMemcpyDeviceToHost);
    const int nb = h->nblk;
    const FFWords W(nb);
    const unsigned* rec = F.data() + W.dbg;                    // the record of the first wait that gave up (handoff.h)
    const bool worker = rec[HD_COUNT] && rec[HD_KIND] < HK_ROLES;
    if (worker) {                       // a worker wait gave up first: show the snapshot it took instead of the final state
        std::vector<unsigned> S(h->ff_flag_words);
        (void)hipMemcpy(S.data(), h->d_ff_flags + h->ff_flag_words, sizeof(unsigned) * S.size(), hipMemcpyDeviceToHost);
        for (size_t w = 0; w < F.size(); ++w) if (w < W.dbg || w >= W.dbg_end) F[w] = S[w];
        fprintf(stderr, "[ff debug] (snapshot taken by the first wait that gave up)\n");
    }
    const unsigned *fc = F.data() + W.fcount, *tp = F.data() + W.tprog, *lf = F.data() + W.lfinal, *dr = F.data() + W.dready, *pd = F.data() + W.potrfdone;
    fprintf(stderr, "[ff debug] ticket %u of %zu items; first worker wait that gave up: count %u item %u kind %u target %u seen %u\n", F[W.ticket],
            h->ff_sched.items.size(), rec[HD_COUNT], rec[HD_TAG], rec[HD_KIND], rec[HD_TARGET], rec[HD_SEEN]);
    if (worker && rec[HD_TAG] < h->ff_sched.items.size()) {
        const FFItem& it = h->ff_sched.items[rec[HD_TAG]];
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
