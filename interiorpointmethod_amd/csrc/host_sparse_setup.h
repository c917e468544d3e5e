// host_sparse_setup.h -- host side, unit 2: set-up of the multifrontal sparse Cholesky (IPM_FLAG_SPARSE_FACTOR): the symbolic cache,
// panel tables and uploads (build_sparse_factor), the row order (ipm_order_rows) and the CSC ingest (ipm_set_A_csc).
#pragma once
// ------------------------------------------------------------------------------- sparse factor (IPM_FLAG_SPARSE_FACTOR)
static void free_sparse_factor(ipm_handle* h) {
    for (void* p : h->sp_allocs) dev_free(h->device, h->stream, p);
    h->sp_allocs.clear();
    h->spf = false;
    h->ds_on = false;
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
// diag_extra (dense-column split only): per row, further terms (column, coefficient) of its DIAGONAL entry, appended to the slot's list.
typedef std::vector<std::vector<std::pair<int, double>>> SpDiagExtra;
static int build_sparse_factor(ipm_handle* h, const std::vector<int>& cp, const std::vector<int>& ri, const std::vector<double>& cv,
                               const std::vector<int>& rp, const std::vector<int>& ci, const std::vector<double>& rv,
                               const SpDiagExtra* diag_extra = nullptr) {
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
        if (diag_extra) for (const auto& row : *diag_extra) terms += row.size();
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
                    if (diag_extra) {                                            // (row k is row b of its own panel: own columns come first)
                        const int64_t e = S.lptr[J] + (int64_t)b * w + b;
                        for (const auto& term : (*diag_extra)[(size_t)k]) {
                            if (pass == 0) fptr[(size_t)e + 1]++;
                            else { const int t = nx[(size_t)e]++; fcol[(size_t)t] = term.first; fcoef[(size_t)t] = term.second; }
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
    F.timeout = timeout_word(h);
    F.done = &h->sc->done;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->sp_uvlen = (long long)S.rows.size();
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
        HIP_TRY(h, hipFuncSetAttribute((const void*)sp_fwd_kernel<SPC_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        HIP_TRY(h, hipFuncSetAttribute((const void*)ds_fwd_kernel<SPC_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        HIP_TRY(h, hipFuncSetAttribute((const void*)sp_chol_kernel<SPC_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
    }
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

// ------------------------------------------------------------------------------- dense columns (dense_split.h)
// The buffers of the split behind a sparse factor that build_sparse_factor made from A WITHOUT the columns h->ds_cols: the handle's
// own stream-ordered allocations, freed with the factor's (the workspace sizes do not change).
static int build_dense_split(ipm_handle* h) {
    DsSplit& s = h->dsp;
    memset(&s, 0, sizeof s);
    s.k = (int)h->ds_cols.size(); s.kp = (s.k + 15) / 16 * 16; s.m = (int)h->m;
    s.rows = ds_chunk_rows(h->m); s.nchunk = (int)((h->m + s.rows - 1) / s.rows);
    s.uvlen = h->sp_uvlen;
    int rc;
    int* d_cols = nullptr;
    if ((rc = sp_upload(h, h->ds_cols, &d_cols))) return rc;
    s.cols = d_cols;
    if ((rc = sp_alloc_zero(h, (size_t)s.m * s.k, &s.V))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)s.m * s.k, &s.W))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)s.uvlen * s.k, &s.uvec))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)s.nchunk * s.kp * s.kp, &s.gpart))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)s.kp * s.kp, &s.R))) return rc;
    if ((rc = sp_alloc_zero(h, (size_t)s.nchunk * s.kp, &s.upart))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->ds_factorizations = 0; h->ds_corrections = 0;
    h->ds_on = true;
    return IPM_OK;
}

extern "C" int ipm_set_dense_columns(ipm_handle* h, int32_t count, const int32_t* cols) {
    if (!h || count < 0 || (count > 0 && !cols)) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_dense_columns: bad arguments");
    if (count == 0) { h->ds_cols.clear(); return IPM_OK; }
    if (count > IPM_MAX_DENSE_COLS) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_dense_columns: %d columns exceed IPM_MAX_DENSE_COLS = %d", (int)count, IPM_MAX_DENSE_COLS);
    if (!h->sparse || !(h->opt.flags & IPM_FLAG_SPARSE_FACTOR)) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_dense_columns: the handle has no sparse factor (IPM_FLAG_SPARSE_FACTOR on a sparse handle)");
    if (h->m <= SMALL_MAX_M) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_dense_columns: a handle of m <= %d rows runs the fused small path, which has no split", SMALL_MAX_M);
    if (int rc_ = compat_refuse(h, "ipm_set_dense_columns", IPM_FEATURE_DENSE_SPLIT)) return rc_;
    std::vector<char> seen((size_t)h->n, 0);
    for (int32_t t = 0; t < count; ++t) {
        if (cols[t] < 0 || cols[t] >= h->n) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_dense_columns: column index %d out of range", (int)cols[t]);
        if (seen[(size_t)cols[t]]) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_dense_columns: column index %d is duplicated", (int)cols[t]);
        seen[(size_t)cols[t]] = 1;
    }
    h->ds_cols.assign(cols, cols + count);
    return IPM_OK;
}

extern "C" int ipm_get_dense_split_info(ipm_handle* h, int64_t out[8]) {
    if (!h || !out) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_dense_split_info: bad arguments");
    for (int t = 0; t < 8; ++t) out[t] = 0;
    if (!h->ds_on) return IPM_OK;
    out[0] = h->dsp.k; out[1] = h->dsp.kp; out[2] = h->dsp.nchunk; out[3] = h->sp_nslot;
    out[5] = h->ds_factorizations; out[6] = h->ds_corrections;
    return IPM_OK;
}

extern "C" int ipm_debug_get_dense_split(ipm_handle* h, int32_t which, double* out, int64_t capacity, int64_t* count) {
    if (!h || !count || which < 0 || which > 4) return fail(h, IPM_ERR_INVALID_ARG, "ipm_debug_get_dense_split: bad arguments");
    if (!h->ds_on) return fail(h, IPM_ERR_STATE, "ipm_debug_get_dense_split: the handle has no dense-column split");
    const DsSplit& s = h->dsp;
    const int64_t k = s.k;
    *count = (which < 2 || which == 4) ? (int64_t)s.m * k : which == 2 ? k * k : k;
    if (!out || capacity < *count) return IPM_OK;
    if (which == 3) { for (int64_t t = 0; t < k; ++t) out[t] = (double)h->ds_cols[(size_t)t]; return IPM_OK; }
    HIP_TRY(h, hipSetDevice(h->device));
    if (which == 4) {           // L^-1 V again, one column at a time with the stock sp_fwd_kernel (level form), into a buffer of its own
        double* tmp = nullptr;
        HIP_TRY(h, dev_malloc(h->device, h->stream, (void**)&tmp, sizeof(double) * (size_t)*count));
        SpFactor F = h->spF;
        F.uvec = s.uvec;        // (column 0's slice as scratch: the next factorization rewrites it)
        F.done = nullptr;
        const int rm = std::max(16, h->sp_rmax);
        const size_t nlev = h->sp_lvlptr.empty() ? 0 : h->sp_lvlptr.size() - 1;
        for (int64_t j = 0; j < k; ++j)
            for (size_t l = 0; l < nlev; ++l) {
                const int cnt = h->sp_lvlptr[l + 1] - h->sp_lvlptr[l];
                hipLaunchKernelGGL((sp_fwd_kernel<SPC_THREADS>), dim3((unsigned)std::min(cnt, h->sp_grid)), dim3(SPC_THREADS), h->sp_lds_solve, h->stream, F, 0u,
                                   s.V + j * s.m, tmp + j * s.m, rm, h->sp_rec_level + h->sp_lvlptr[l], cnt);
            }
        hipError_t e = hipMemcpyAsync(out, tmp, sizeof(double) * (size_t)*count, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        dev_free(h->device, h->stream, tmp);
        if (e != hipSuccess) return fail(h, IPM_ERR_HIP, "ipm_debug_get_dense_split: %s", hipGetErrorString(e));
        return IPM_OK;
    }
    if (which < 2) {
        HIP_TRY(h, hipMemcpyAsync(out, which == 0 ? s.V : s.W, sizeof(double) * (size_t)*count, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return IPM_OK;
    }
    std::vector<double> R((size_t)s.kp * s.kp);
    HIP_TRY(h, hipMemcpyAsync(R.data(), s.R, sizeof(double) * R.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < k; ++i) for (int64_t j = 0; j < k; ++j) out[i * k + j] = R[(size_t)(i * s.kp + j)];
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
        const bool split = !h->ds_cols.empty() && (h->opt.flags & IPM_FLAG_SPARSE_FACTOR);      // (ipm_set_dense_columns refused m <= 128)
        std::vector<char> is_dense;
        if (split) {            // A without the dense columns must keep every row: B_s would be singular by structure
            is_dense.assign((size_t)h->n, 0);
            for (int j : h->ds_cols) is_dense[(size_t)j] = 1;
            std::vector<int> left((size_t)h->m, 0);
            for (int64_t j = 0; j < h->n; ++j) if (!is_dense[(size_t)j]) for (int q = cp[j]; q < cp[j + 1]; ++q) left[(size_t)ri[q]]++;
            for (int64_t i = 0; i < h->m; ++i)
                if (!left[(size_t)i]) return fail(h, IPM_ERR_INVALID_ARG, "ipm_set_A_csc: taking the dense columns out empties row %lld of A (ipm_set_dense_columns)", (long long)i);
        }
        if (nz > h->nnz_cap) return fail(h, IPM_ERR_INVALID_ARG, "nnz %lld exceeds the handle's sparse_nnz %lld", (long long)nz, (long long)h->nnz_cap);
        if (int rc_ = eq_reset(h)) return rc_;               // a valid new A: the handle is unscaled again (host_equilibrate.h)
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
            // (the small path's rows of the compatibility table, host_compat.h: a handle that holds a quadratic term takes the path only with
            //  IPM_FLAG_SMALL_QUADRATIC, one that holds free columns only with IPM_FLAG_SMALL_FREE on top, one with an LP free set never)
            const bool want_small = h->fused_small && h->m <= SMALL_MAX_M && terms <= ((size_t)1 << 22) && !compat_blocker(h, IPM_FEATURE_SMALL_PATH);
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
            int rc;
            if (split) {
                // A_s: the same n columns with the dense ones emptied, so that the product list indexes the full d; everything
                // else (products with A, residuals, A^T dy, the refinement residual) keeps the full A uploaded above
                // B_s also takes DS_DIAG_REL times the DIAGONAL of the dense columns' own term V V^T (dense_split.h): near the optimum
                // the rows that only basic dense columns support would leave B_s with pivots the size of the vanishing d
                std::vector<int> cps(cp.size(), 0), ris, rps(rp.size(), 0), cis; std::vector<double> cvs, rvs;
                SpDiagExtra extra((size_t)h->m);
                for (int64_t i = 0; i < h->m; ++i)
                    for (int q = rp[i]; q < rp[i + 1]; ++q) if (is_dense[(size_t)ci[q]]) extra[(size_t)i].emplace_back(ci[q], DS_DIAG_REL * rv[q] * rv[q]);
                for (int64_t j = 0; j < h->n; ++j) {
                    if (!is_dense[(size_t)j]) for (int q = cp[j]; q < cp[j + 1]; ++q) { ris.push_back(ri[q]); cvs.push_back(cv[q]); }
                    cps[(size_t)j + 1] = (int)ris.size();
                }
                for (int64_t i = 0; i < h->m; ++i) {
                    for (int q = rp[i]; q < rp[i + 1]; ++q) if (!is_dense[(size_t)ci[q]]) { cis.push_back(ci[q]); rvs.push_back(rv[q]); }
                    rps[(size_t)i + 1] = (int)cis.size();
                }
                rc = build_sparse_factor(h, cps, ris, cvs, rps, cis, rvs, &extra);
                if (!rc) rc = build_dense_split(h);
                if (!rc && h->ref.k < DS_MIN_REFINE) h->ref.k = DS_MIN_REFINE;      // the split's own refinement rounds
            } else rc = build_sparse_factor(h, cp, ri, cv, rp, ci, rv);
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
    if (int rc_ = eq_reset(h)) { free(img); return rc_; }      // a valid new A: the handle is unscaled again (host_equilibrate.h)
    hipError_t e = hipMemcpyAsync(h->A, img, sizeof(double) * h->mp * h->np, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(img);
    if (e != hipSuccess) return fail(h, IPM_ERR_HIP, "upload of A failed: %s", hipGetErrorString(e));
    h->haveA = true; h->predictor_valid = false;
    return IPM_OK;
}
