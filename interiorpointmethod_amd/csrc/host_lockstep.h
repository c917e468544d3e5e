// host_lockstep.h -- host side, unit 7: the lockstep batch (lockstep.h, lockstep_merge.h): recording of a handle's iteration,
// the merge into global steps, ipm_batch_* and ipm_solve_batch.
#pragma once
// ------------------------------------------------------------------------------- lockstep batch (lockstep.h)
// the GEMM launchers' way into a recording: the type is the one whose declared tile shape (lockstep.h) is the launcher's instantiation
template <int... T> static bool ls_record_gemm(ipm_handle* h, int bm, int bn, int bk, int wm, int wn, const GemmNT& g, unsigned grid) {
    return ((LsTwin<T>::is(bm, bn, bk, wm, wn) && (record_twin<T>(h, grid, g), true)) || ...);
}
static void ls_gemm_hook(void* ctx, int bm, int bn, int bk, int wm, int wn, const GemmNT& g, int grid) {
    ipm_handle* h = (ipm_handle*)ctx;
    bool ok;
    if (g.batch > 1 || g.batch2 > 1)                         // the group inverses' batched products: 3-D grid packed into the LP's block range
        ok = ls_record_gemm<LS_GEMM_32_32_32_BATCHED>(h, bm, bn, bk, wm, wn, g, (unsigned)grid * (unsigned)g.batch * (unsigned)g.batch2);
    else                                                     // (a device-polled hand-off has no twin)
        ok = !g.wait_on && !g.signal && ls_record_gemm<LS_CHOL_UPDATE, LS_GEMM_32_128_32, LS_GEMM_64_64_16, LS_GEMM_64_128_16, LS_GEMM_128_128_16, LS_GEMM_32_32_32>(h, bm, bn, bk, wm, wn, g, (unsigned)grid);
    if (!ok) h->ls_cut = true;                               // not recordable: ls_record_program reports it
}
// (a handle with finite upper bounds only with IPM_FLAG_LOCKSTEP_BOUNDS, the opt-in to the bounded twins)
static bool ls_bounds_ok(const ipm_handle* h) { return !compat_blocker(h, IPM_FEATURE_LOCKSTEP, nullptr, IPM_FEATURE_BOUNDS); }      // (host_compat.h: lifted by IPM_FLAG_LOCKSTEP_BOUNDS)
static bool ls_eligible(const ipm_handle* h) {
    return h->lockstep && ls_bounds_ok(h) && h->sparse && !h->small && !h->spf && h->lookahead == 0 && h->stream2 == nullptr && h->B && h->invD &&
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
    std::vector<int> unreported;                       // finished, not yet handed to the caller (ipm_batch_step: cap was too small), oldest first
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
static int bfail(ipm_batch* b, int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); code = vfail(b ? b->err : nullptr, code, fmt, ap); va_end(ap); return code; }
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
    if (!ls_bounds_ok(h)) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_batch_add: a handle with upper bounds (ipm_set_bounds) has no lockstep twin");
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
// EVERY finished handle is reported exactly once: those that did not fit into `cap` stay queued (b->unreported) and lead the
// list of the following calls, at most `cap` per call, also when nothing is active any more.
static void ls_report_finished(ipm_batch* b, int32_t* finished, int32_t cap, int32_t* n_finished) {
    size_t k = 0;
    while (k < b->unreported.size() && *n_finished < cap) finished[(*n_finished)++] = b->unreported[k++];
    b->unreported.erase(b->unreported.begin(), b->unreported.begin() + (long)k);
}
extern "C" int ipm_batch_step(ipm_batch* b, int32_t* finished, int32_t cap, int32_t* n_finished, int32_t* n_active) {
    if (!b || !n_finished || (cap > 0 && !finished)) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_batch_step: bad arguments");
    *n_finished = 0;
    if (n_active) *n_active = (int32_t)b->active.size();
    if (b->active.empty()) { ls_report_finished(b, finished, cap, n_finished); return IPM_OK; }
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
            size_t longest = 0; int cnt[LS_NTYPES_ALL] = {0};
            for (int i : b->active) longest = std::max(longest, b->prog[(size_t)i].size());
            for (const LsStep& st : b->steps) cnt[st.type]++;
            fprintf(stderr, "[lockstep] %zu LPs active, longest program %zu launches, merged schedule %zu steps (%zu records); steps by type:", b->active.size(), longest, b->steps.size(), b->recs.size());
            for (int t = 0; t < LS_NTYPES_ALL; ++t) if (cnt[t]) fprintf(stderr, " %d:%d", t, cnt[t]);
            fprintf(stderr, "\n");
        }
    }
    const auto t_mid = std::chrono::steady_clock::now();
    static const bool ls_prof = getenv("IPM_LS_PROF") != nullptr;      // diagnostic: a synchronisation after every launch, wall time per kernel type
    static double tot[LS_NTYPES_ALL]; static long cnt[LS_NTYPES_ALL]; static long calls = 0;
    for (int c = 0; c < b->chunk; ++c)
        for (const LsStep& st : b->steps) {
            const auto t0 = ls_prof ? std::chrono::steady_clock::now() : t_mid;
            B_TRY(b, ls_launch(st.type, b->d_recs + st.offset, st.count, st.blocks, st.lds, S));
            if (!ls_prof) continue;
            B_TRY(b, hipStreamSynchronize(S));
            tot[st.type] += secs(t0); cnt[st.type]++;
        }
    if (ls_prof && ++calls % 25 == 0) {
        fprintf(stderr, "[lockstep prof] %zu active, %zu steps; us per launch (launches) by type:", b->active.size(), b->steps.size());
        for (int t = 0; t < LS_NTYPES_ALL; ++t) if (cnt[t]) fprintf(stderr, " %d:%.1f(%ld)", t, 1e6 * tot[t] / cnt[t], cnt[t]);
        fprintf(stderr, "\n");
        for (int t = 0; t < LS_NTYPES_ALL; ++t) { tot[t] = 0; cnt[t] = 0; }
    }
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
            b->unreported.push_back(i);
            continue;
        }
        keep.push_back(i);
    }
    b->active.swap(keep);
    ls_report_finished(b, finished, cap, n_finished);
    if (n_active) *n_active = (int32_t)b->active.size();
    return IPM_OK;
}
// Test hook (host only, nothing is launched): the merged schedule the last ipm_batch_step launched, {type, members, blocks, lds}
// per step, copied from b->steps.  *count = steps; IPM_ERR_INVALID_ARG (with *count set) when capacity < 4 * steps.
extern "C" int ipm_debug_batch_schedule(ipm_batch* b, int32_t* out, int32_t capacity, int32_t* count) {
    if (!b || !count || (capacity > 0 && !out) || capacity < 0) return bfail(b, IPM_ERR_INVALID_ARG, "ipm_debug_batch_schedule: bad arguments");
    *count = (int32_t)b->steps.size();
    if ((int64_t)capacity < 4 * (int64_t)b->steps.size())
        return bfail(b, IPM_ERR_INVALID_ARG, "ipm_debug_batch_schedule: capacity %d < 4 x %zu steps", (int)capacity, b->steps.size());
    for (size_t s = 0; s < b->steps.size(); ++s) {
        const LsStep& st = b->steps[s];
        out[4 * s] = st.type; out[4 * s + 1] = (int32_t)st.count; out[4 * s + 2] = (int32_t)st.blocks; out[4 * s + 3] = (int32_t)st.lds;
    }
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
    for (int i = 0; i < n; ++i)          // (ls_bounds_ok, in the table's words)
        if (int rc_ = compat_refuse(hs[i], "ipm_solve_batch", IPM_FEATURE_LOCKSTEP, i, /*to_handle=*/true, IPM_FEATURE_BOUNDS)) return rc_;
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
