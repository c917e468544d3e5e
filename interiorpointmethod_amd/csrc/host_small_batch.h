// host_small_batch.h -- host side, unit 9: ipm_solve_small_batch, many small LPs (fused single-workgroup path, small_lp.h) in one
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
    int count[SMALL_NVARIANTS] = {0, 0, 0, 0};
    for (int p = 0; p < cnt; ++p) {
        ipm_handle* h = hs[order[(size_t)p]];
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
        launch_small(v, S, nullptr, d_items + off, (unsigned)count[v]);
        off += count[v];
    }
    hipLaunchKernelGGL(small_batch_gather_kernel, dim3(g256), dim3(256), 0, S, d_items, cnt, d_sc);
    HIP_TRY(h0, hipGetLastError());
    HIP_TRY(h0, hipMemcpyAsync(h_sc, d_sc, sizeof(Scalars) * (size_t)cnt, hipMemcpyDeviceToHost, S));
    HIP_TRY(h0, hipStreamSynchronize(S));
    for (int p = 0; p < cnt; ++p) *hs[order[(size_t)p]]->h_sc = h_sc[p];
    return IPM_OK;
}

extern "C" int ipm_solve_small_batch(ipm_handle** hs, int32_t n, double tol_p, double tol_d, double tol_gap, int32_t max_iter, void* stream,
                                     ipm_stats* stats) {
    if (n < 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: n = %d < 0", (int)n);
    if (n == 0) return IPM_OK;                               // nothing to do: no device is touched
    if (!hs) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: handles is NULL (n = %d)", (int)n);
    if (max_iter < 0) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: max_iter < 0");
    for (int i = 0; i < n; ++i) {
        ipm_handle* h = hs[i];
        if (!h) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: handle %d is NULL", i);
        if (!h->small) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: handle %d is not on the fused small-LP path (sparse A of at most %d rows; ipm_get_schedule out[9])", i, SMALL_MAX_M);
        if (h->device != hs[0]->device) return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: handle %d lives on device %d, handle 0 on device %d", i, h->device, hs[0]->device);
    }
    {   // the same handle twice: two workgroups would race on one state
        std::vector<std::pair<const ipm_handle*, int>> seen((size_t)n);
        for (int i = 0; i < n; ++i) seen[(size_t)i] = {hs[i], i};
        std::sort(seen.begin(), seen.end());
        for (int i = 1; i < n; ++i)
            if (seen[(size_t)i].first == seen[(size_t)i - 1].first)
                return fail(nullptr, IPM_ERR_INVALID_ARG, "ipm_solve_small_batch: handle %d is the same handle as handle %d", seen[(size_t)i].second, seen[(size_t)i - 1].second);
    }
    for (int i = 0; i < n; ++i) {
        ipm_handle* h = hs[i];
        if (!h->haveA || !h->haveBC || !h->haveState) return fail(nullptr, IPM_ERR_STATE, "ipm_solve_small_batch: handle %d: A, (b,c) and a state must be set first", i);
        if (h->profiling) return fail(nullptr, IPM_ERR_STATE, "ipm_solve_small_batch: handle %d has profiling on (ipm_set_profiling)", i);
    }
    ipm_handle* h0 = hs[0];
    HIP_TRY(h0, hipSetDevice(h0->device));
    hipStream_t S = stream ? (hipStream_t)stream : h0->stream;
    {   // whatever the handles did on their own streams is complete before the batch touches them: one event per distinct stream
        std::vector<hipStream_t> waited;
        for (int i = 0; i < n; ++i) {
            ipm_handle* h = hs[i];
            if (h->stream == S || std::find(waited.begin(), waited.end(), h->stream) != waited.end()) continue;
            HIP_TRY(h0, hipEventRecord(h->ev_fork, h->stream));
            HIP_TRY(h0, hipStreamWaitEvent(S, h->ev_fork, 0));
            waited.push_back(h->stream);
        }
    }
    for (int i = 0; i < n; ++i) {                            // as ipm_solve starts a solve
        ipm_handle* h = hs[i];
        h->predictor_valid = false; h->fresh_state = false;
        if (h->auto_reg) { h->auto_reg = 0; h->shift_rel = h->opt.regularize; }
    }
    struct Mem {                                             // released on every return path
        int device; hipStream_t S; SmallItem* items = nullptr; Scalars* sc = nullptr;
        ~Mem() { dev_free(device, S, items); dev_free(device, S, sc); }
    } mem{h0->device, S};
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
