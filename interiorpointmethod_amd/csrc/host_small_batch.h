// host_small_batch.h -- host side, unit 9: ipm_solve_small_batch and ipm_init_small_batch_mehrotra, many small LPs (fused single-workgroup path, small_lp.h) in one
// launch per kernel variant, one workgroup per LP.
#pragma once
// ------------------------------------------------------------------------------- batch of small LPs (small_lp.h)
// Dispatch order: by variant (one grid each), inside a variant by estimated cost per iteration, largest first, so that the long LPs
// start first and the tail of the grid is short.  The estimate is the entry count of the product list times the panel count:
// for a dense B that is (16 nt)^2 / 2 * nt, the scale of the Cholesky's flops, and for a sparse one it follows the formation.
// (The iteration counts are not predictable.)  Ties go to the caller's order; no result depends on any of this.
static double small_cost(const ipm_handle* h) { return (double)h->sm_nb * (double)((h->m + 15) / 16); }

// one round: parameters, one grid per variant present, gather, ONE copy to the host and ONE synchronisation
static int small_batch_round(ipm_handle* h0, ipm_handle** hs, const std::vector<int>& members, bool first, double tol_p, double tol_d, double tol_gap,
                             int max_iter, hipStream_t S, SmallItem* d_items, Scalars* d_sc, std::vector<SmallItem>& items, Scalars* h_sc) {
    const int cnt = (int)members.size();
    std::vector<int> order(members);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        const int va = small_variant(hs[a]), vb = small_variant(hs[b]);
        if (va != vb) return va < vb;
        return small_cost(hs[a]) > small_cost(hs[b]);
    });
    items.resize((size_t)cnt);
    int count[SMALL_NVARIANTS] = {};
    for (int p = 0; p < cnt; ++p) {
        ipm_handle* h = hs[order[(size_t)p]];
        if (int rc_ = check_class(h, "ipm_solve_small_batch")) return rc_;
        const bool may_auto = h->opt.regularize == 0.0 && !(h->opt.flags & IPM_FLAG_NO_AUTO_REGULARIZE);
        items[(size_t)p] = small_item(h, p, 1 << 30, first && may_auto ? 1 : 0);
        count[items[(size_t)p].variant]++;
    }
    HIP_TRY(h0, hipMemcpyAsync(d_items, items.data(), sizeof(SmallItem) * (size_t)cnt, hipMemcpyHostToDevice, S));
    const unsigned g256 = (unsigned)((cnt + 255) / 256);
    hipLaunchKernelGGL(small_batch_params_kernel, dim3(g256), dim3(256), 0, S, d_items, cnt, tol_p, tol_d, tol_gap, max_iter);
    int off = 0;
    for (int v = 0; v < SMALL_NVARIANTS; ++v) {
        if (!count[v]) continue;
        launch_small(SMALL_ROWS[v], S, nullptr, d_items + off, (unsigned)count[v]);
        off += count[v];
    }
    hipLaunchKernelGGL(small_batch_gather_kernel, dim3(g256), dim3(256), 0, S, d_items, cnt, d_sc);
    HIP_TRY(h0, hipGetLastError());
    HIP_TRY(h0, hipMemcpyAsync(h_sc, d_sc, sizeof(Scalars) * (size_t)cnt, hipMemcpyDeviceToHost, S));
    HIP_TRY(h0, hipStreamSynchronize(S));
    for (int p = 0; p < cnt; ++p) *hs[order[(size_t)p]]->h_sc = h_sc[p];
    return IPM_OK;
}

template <class R> static int small_batch_check_rounds(const char* who, int i, const R& r) {      // a round feature with k > 0
    return r.k > 0 ? fail(nullptr, IPM_ERR_INVALID_ARG, "%s: handle %d has %d %s set; the small-LP kernel runs %s", who, i, r.k, r.kind->noun, r.kind->none) : IPM_OK;
}
// the argument rules both batch entries share: n, the array, and per handle NULL / not on the small path / another device / twice
static int small_batch_check_handles(const char* who, ipm_handle** hs, int32_t n) {
    if (n < 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: n = %d < 0", who, (int)n);
    if (n == 0) return IPM_OK;
    if (!hs) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: handles is NULL (n = %d)", who, (int)n);
    for (int i = 0; i < n; ++i) {
        ipm_handle* h = hs[i];
        if (!h) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: handle %d is NULL", who, i);
        if (!h->small) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: handle %d is not on the fused small-LP path (sparse A of at most %d rows; ipm_get_schedule out[9])", who, i, SMALL_MAX_M);
        int rc;
        if ((rc = small_batch_check_rounds(who, i, h->mcc)) || (rc = small_batch_check_rounds(who, i, h->ref))) return rc;
        if (h->device != hs[0]->device) return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: handle %d lives on device %d, handle 0 on device %d", who, i, h->device, hs[0]->device);
    }
    {   // the same handle twice: two workgroups would race on one state
        std::vector<std::pair<const ipm_handle*, int>> seen((size_t)n);
        for (int i = 0; i < n; ++i) seen[(size_t)i] = {hs[i], i};
        std::sort(seen.begin(), seen.end());
        for (int i = 1; i < n; ++i)
            if (seen[(size_t)i].first == seen[(size_t)i - 1].first)
                return fail(nullptr, IPM_ERR_INVALID_ARG, "%s: handle %d is the same handle as handle %d", who, seen[(size_t)i].second, seen[(size_t)i - 1].second);
    }
    return IPM_OK;
}
// whatever the handles did on their own streams is complete before the batch touches them: one event per distinct stream
static int small_batch_wait_streams(ipm_handle** hs, int32_t n, hipStream_t S) {
    ipm_handle* h0 = hs[0];
    std::vector<hipStream_t> waited;
    for (int i = 0; i < n; ++i) {
        ipm_handle* h = hs[i];
        if (h->stream == S || std::find(waited.begin(), waited.end(), h->stream) != waited.end()) continue;
        HIP_TRY(h0, hipEventRecord(h->ev_fork, h->stream));
        HIP_TRY(h0, hipStreamWaitEvent(S, h->ev_fork, 0));
        waited.push_back(h->stream);
    }
    return IPM_OK;
}
struct SmallBatchMem {                                       // the item table and the gathered records of a batch call, released on every return path
    int device; hipStream_t S; SmallItem* items = nullptr; Scalars* sc = nullptr;
    ~SmallBatchMem() { dev_free(device, S, items); dev_free(device, S, sc); }
};

extern "C" int ipm_solve_small_batch(ipm_handle** hs, int32_t n, double tol_p, double tol_d, double tol_gap, int32_t max_iter, void* stream,
                                     ipm_stats* stats) {
    if (int rc_ = small_batch_check_handles("ipm_solve_small_batch", hs, n)) return rc_;
    if (n == 0) return IPM_OK;                               // nothing to do: no device is touched
    if (max_iter < 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: max_iter < 0");
    for (int i = 0; i < n; ++i) {
        ipm_handle* h = hs[i];
        if (!h->haveA || !h->haveBC || !h->haveState) return fail(nullptr, IPM_ERR_STATE, "ipm_solve_small_batch: handle %d: A, (b,c) and a state must be set first", i);
        if (h->profiling) return fail(nullptr, IPM_ERR_STATE, "ipm_solve_small_batch: handle %d has profiling on (ipm_set_profiling)", i);
        if (const int c = free_without_term(h); c >= 0)          // (check_ready's rule of the single solve)
            return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: handle %d: column %d %s", i, c, FREE_NEEDS_TERM);
    }
    ipm_handle* h0 = hs[0];
    HIP_TRY(h0, hipSetDevice(h0->device));
    hipStream_t S = stream ? (hipStream_t)stream : h0->stream;
    if (int rc_ = small_batch_wait_streams(hs, n, S)) return rc_;
    for (int i = 0; i < n; ++i) {                            // as ipm_solve starts a solve
        ipm_handle* h = hs[i];
        h->predictor_valid = false; h->fresh_state = false;
        if (h->auto_reg) { h->auto_reg = 0; h->shift_rel = h->opt.regularize; }
    }
    SmallBatchMem mem{h0->device, S};
    HIP_TRY(h0, dev_malloc(h0->device, S, (void**)&mem.items, sizeof(SmallItem) * (size_t)n));
    HIP_TRY(h0, dev_malloc(h0->device, S, (void**)&mem.sc, sizeof(Scalars) * (size_t)n));
    std::vector<SmallItem> items;
    std::vector<Scalars> host_sc((size_t)n);
    std::vector<int> members((size_t)n);
    for (int i = 0; i < n; ++i) members[(size_t)i] = i;
    HIP_TRY(h0, hipEventRecord(h0->ev0, S));
    int rc = small_batch_round(h0, hs, members, true, tol_p, tol_d, tol_gap, max_iter, S, mem.items, mem.sc, items, host_sc.data());
    if (rc) return rc;
    // the automatic Tikhonov shift of ipm_solve: the LPs whose first factorization asked for it left before they touched their iterate;
    // they alone run a second time, with the shift.  At most two rounds per call.
    members.clear();
    for (int i = 0; i < n; ++i)
        if (hs[i]->h_sc->status == IPM_STATUS_NEEDS_SHIFT) { hs[i]->shift_rel = 1e-14; hs[i]->auto_reg = 1; members.push_back(i); }
    if (!members.empty() && (rc = small_batch_round(h0, hs, members, false, tol_p, tol_d, tol_gap, max_iter, S, mem.items, mem.sc, items, host_sc.data()))) return rc;
    HIP_TRY(h0, hipEventRecord(h0->ev1, S));
    HIP_TRY(h0, hipEventSynchronize(h0->ev1));
    float ms = 0.f;
    HIP_TRY(h0, hipEventElapsedTime(&ms, h0->ev0, h0->ev1));
    if (stats) for (int i = 0; i < n; ++i) fill_stats(hs[i], &stats[i], ms);
    return IPM_OK;
}

// Mehrotra's starting point for n handles of the small path in one launch per variant (plain / bounded), one workgroup per LP: the
// batch form of ipm_init_state_mehrotra, with one copy of the scalar records to the host and one synchronisation.
extern "C" int ipm_init_small_batch_mehrotra(ipm_handle** hs, int32_t n, void* stream, int32_t* pivots_fixed) {
    if (int rc_ = small_batch_check_handles("ipm_init_small_batch_mehrotra", hs, n)) return rc_;
    if (n == 0) return IPM_OK;                               // nothing to do: no device is touched
    for (int i = 0; i < n; ++i)
        if (!hs[i]->haveA || !hs[i]->haveBC) return fail(nullptr, IPM_ERR_STATE, "ipm_init_small_batch_mehrotra: handle %d: A and (b,c) must be set first", i);
    for (int i = 0; i < n; ++i)              // as ipm_init_state_mehrotra refuses one such handle, before anything is launched
        if (int rc_ = compat_refuse(hs[i], "ipm_init_small_batch_mehrotra", IPM_FEATURE_MEHROTRA_START, i, /*to_handle=*/false)) return rc_;
    ipm_handle* h0 = hs[0];
    HIP_TRY(h0, hipSetDevice(h0->device));
    hipStream_t S = stream ? (hipStream_t)stream : h0->stream;
    if (int rc_ = small_batch_wait_streams(hs, n, S)) return rc_;
    SmallBatchMem mem{h0->device, S};
    HIP_TRY(h0, dev_malloc(h0->device, S, (void**)&mem.items, sizeof(SmallItem) * (size_t)n));
    HIP_TRY(h0, dev_malloc(h0->device, S, (void**)&mem.sc, sizeof(Scalars) * (size_t)n));
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {      // plain first, inside a variant the long LPs first (small_cost)
        const bool ba = step_variant(hs[a]).bounded, bb = step_variant(hs[b]).bounded;
        if (ba != bb) return !ba;
        return small_cost(hs[a]) > small_cost(hs[b]);
    });
    std::vector<SmallItem> items((size_t)n);
    int nplain = 0;
    for (int p = 0; p < n; ++p) {
        items[(size_t)p] = small_item(hs[order[(size_t)p]], p, 0, 0);
        if (!step_variant(hs[order[(size_t)p]]).bounded) ++nplain;
    }
    HIP_TRY(h0, hipMemcpyAsync(mem.items, items.data(), sizeof(SmallItem) * (size_t)n, hipMemcpyHostToDevice, S));
    const unsigned g256 = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(small_batch_params_kernel, dim3(g256), dim3(256), 0, S, mem.items, (int)n, 1e-8, 1e-8, 1e-8, 1 << 30);
    if (nplain) launch_small(SMALL_START_ROWS[0], S, nullptr, mem.items, (unsigned)nplain);
    if (n - nplain) launch_small(SMALL_START_ROWS[1], S, nullptr, mem.items + nplain, (unsigned)(n - nplain));
    hipLaunchKernelGGL(small_batch_gather_kernel, dim3(g256), dim3(256), 0, S, mem.items, (int)n, mem.sc);
    HIP_TRY(h0, hipGetLastError());
    std::vector<Scalars> host_sc((size_t)n);
    HIP_TRY(h0, hipMemcpyAsync(host_sc.data(), mem.sc, sizeof(Scalars) * (size_t)n, hipMemcpyDeviceToHost, S));
    HIP_TRY(h0, hipStreamSynchronize(S));
    for (int p = 0; p < n; ++p) {
        ipm_handle* h = hs[order[(size_t)p]];
        *h->h_sc = host_sc[(size_t)p];
        if (pivots_fixed) pivots_fixed[order[(size_t)p]] = h->h_sc->fixed;
        mark_fresh_state(h);
    }
    return IPM_OK;
}
