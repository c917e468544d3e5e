// host_equilibrate.h -- host side, unit 1b: ipm_equilibrate / ipm_get_scaling (kernels and the rule: equilibrate.h)
// and THE BOUNDARY RULE of a scaled handle, stated once: data entering the handle is scaled on the way in, data leaving it is
// unscaled on the way out (eq_in / eq_out).  Every factor is a power of two, so both directions are exact, and they are applied on
// the host to arrays that are on the host anyway; the device only ever sees the scaled problem.
#pragma once

// v (length f.size()) times (or over) the factors -> tmp; returns tmp.data().  Unscaled handle: v itself.
static const double* eq_in(const ipm_handle* h, std::vector<double>& tmp, const double* v, const std::vector<double>& f, bool divide) {
    if (!h->scaled || !v) return v;
    tmp.resize(f.size());
    for (size_t i = 0; i < f.size(); ++i) tmp[i] = divide ? v[i] / f[i] : v[i] * f[i];
    return tmp.data();
}
static void eq_out(const ipm_handle* h, double* v, const std::vector<double>& f, bool divide) {
    if (!h->scaled || !v) return;
    for (size_t i = 0; i < f.size(); ++i) v[i] = divide ? v[i] / f[i] : v[i] * f[i];
}

// The device check of ipm_equilibrate covers the data present at that call; data entering a scaled handle LATER meets the same
// precondition here: no nonzero finite entry whose scaled image leaves the normal fp64 range (+inf, a missing bound, stays +inf).
static bool eq_in_range(const ipm_handle* h, const double* v, const double* scaled, size_t n) {
    if (!h->scaled || v == scaled) return true;
    for (size_t i = 0; i < n; ++i)
        if (v[i] != 0.0 && std::isfinite(v[i]) && !std::isnormal(scaled[i])) return false;
    return true;
}

// b_norm / c_norm of the handle's current (b, c, u), stated once: ipm_set_bc and ipm_equilibrate both enqueue exactly this
static void enqueue_bc_norms(ipm_handle* h) {
    if (h->bnd) hipLaunchKernelGGL(bnd_norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->b, (int)h->m, bnd_args(h).u, (int)h->n, &h->sc->b_norm);
    else hipLaunchKernelGGL(norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->b, (int)h->m, &h->sc->b_norm);
    hipLaunchKernelGGL(norm2_kernel, dim3(1), dim3(VBLK), 0, h->stream, h->c, (int)h->n, &h->sc->c_norm);
}

// A new A has arrived and passed its validation (ipm_set_A_dense / ipm_set_A_csc call this just before they touch the device copy
// of A, so a rejected A leaves the scaled handle as it was): the handle is unscaled again.  The bounds it holds go back to the
// caller's units (exact), and so does its quadratic term (g' = g C^2); b and c must be set again.
static int eq_reset(ipm_handle* h) {
    if (!h->scaled) return IPM_OK;
    if (h->quad) {
        std::vector<double> g((size_t)h->n);
        HIP_TRY(h, hipMemcpyAsync(g.data(), h->quad_g, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t j = 0; j < g.size(); ++j) g[j] = g[j] / h->eq_c[j] / h->eq_c[j];
        HIP_TRY(h, hipMemcpyAsync(h->quad_g, g.data(), sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (h->bnd) {
        std::vector<double> u((size_t)h->n);
        HIP_TRY(h, hipMemcpyAsync(u.data(), h->bnd_mem, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t j = 0; j < u.size(); ++j) u[j] *= h->eq_c[j];
        HIP_TRY(h, hipMemcpyAsync(h->bnd_mem, u.data(), sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->scaled = false; h->eq_r.clear(); h->eq_c.clear();
    h->haveBC = false; h->haveState = false;
    return IPM_OK;
}

static double eq_log2_spread(const double* mxmn) { return mxmn[0] > 0.0 && mxmn[1] > 0.0 ? log2(mxmn[0]) - log2(mxmn[1]) : 0.0; }

extern "C" int ipm_equilibrate(ipm_handle* h, int32_t max_passes, double info[4]) {
    if (!h || max_passes < 0 || max_passes > EQ_MAX_PASSES) return fail(h, IPM_ERR_INVALID_ARG, "ipm_equilibrate: bad arguments (0 <= max_passes <= %d)", EQ_MAX_PASSES);
    if (!h->haveA) return fail(h, IPM_ERR_STATE, "ipm_equilibrate: A not set");
    if (h->scaled) return fail(h, IPM_ERR_STATE, "ipm_equilibrate: the handle is already scaled");
    HIP_TRY(h, hipSetDevice(h->device));
    const int m = (int)h->m, n = (int)h->n, np = (int)h->np, mp = (int)h->mp, cap = max_passes;
    const int chunks = h->sparse ? 0 : (int)std::min<int64_t>(EQ_COL_CHUNKS, (m + 63) / 64);
    const int rows_per_chunk = chunks ? (m + chunks - 1) / chunks : 0;
    // temporary device memory of this call: doubles rowmax | colmax | spread[6] | part, then ints er | ec | changed[cap + 1] | err[cap + 3]
    const size_t nd = (size_t)mp + np + 8 + (size_t)chunks * np, ni = (size_t)mp + np + 2 * (size_t)cap + 8;
    double* dmem = nullptr;
    if (dev_malloc(h->device, h->stream, (void**)&dmem, sizeof(double) * nd + sizeof(int) * ni) != hipSuccess)
        return fail(h, IPM_ERR_HIP, "ipm_equilibrate: %zu bytes of scratch could not be allocated", sizeof(double) * nd + sizeof(int) * ni);
    struct Free { ipm_handle* h; void* p; ~Free() { dev_free(h->device, h->stream, p); } } free_dmem{h, dmem};
    double *rowmax = dmem, *colmax = dmem + mp, *spread = colmax + np, *part = spread + 8;
    int *er = (int*)(dmem + nd), *ec = er + mp, *changed = ec + np, *err_max = changed + cap + 1, *err_misc = err_max + cap + 1;
    HIP_TRY(h, hipMemsetAsync(dmem, 0, sizeof(double) * nd + sizeof(int) * ni, h->stream));
    const SparseA S = sparse_view(h);
    auto maxima = [&](const int* live, int* err) {
        if (h->sparse) {
            hipLaunchKernelGGL(eq_sparse_max_kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, h->stream, S.rowptr, S.colind, S.rval, m, er, ec, rowmax, live, err);
            hipLaunchKernelGGL(eq_sparse_max_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, h->stream, S.colptr, S.rowind, S.cval, n, ec, er, colmax, live, err);
        } else {
            hipLaunchKernelGGL(eq_dense_rowmax_kernel, dim3((unsigned)m), dim3(256), 0, h->stream, h->A, np, er, ec, rowmax, live, err);
            hipLaunchKernelGGL(eq_dense_colpart_kernel, dim3((unsigned)((np / 2 + 127) / 128), (unsigned)chunks), dim3(128), 0, h->stream, h->A, m, np, rows_per_chunk, er, ec, part, live);
            hipLaunchKernelGGL(eq_colmax_combine_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, part, np, chunks, colmax, live);
        }
    };
    // the cap runs on the device without a host synchronisation: a pass behind the fixed point returns at its first instruction
    maxima(nullptr, err_max);
    hipLaunchKernelGGL(eq_spread_kernel, dim3(1), dim3(256), 0, h->stream, rowmax, m, spread);
    const unsigned gf = (unsigned)((std::max(m, n) + 255) / 256);
    for (int p = 0; p < cap; ++p) {
        hipLaunchKernelGGL(eq_factor_kernel, dim3(gf), dim3(256), 0, h->stream, rowmax, m, er, colmax, n, ec, p ? changed + p - 1 : nullptr, changed + p, err_misc);
        maxima(changed + p, err_max + p + 1);
    }
    hipLaunchKernelGGL(eq_spread_kernel, dim3(1), dim3(256), 0, h->stream, rowmax, m, spread + 2);
    hipLaunchKernelGGL(eq_spread_kernel, dim3(1), dim3(256), 0, h->stream, colmax, n, spread + 4);
    if (h->haveBC) {
        hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, h->b, er, m, 1, 1, err_misc);
        hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->c, ec, n, 1, 1, err_misc);
    }
    if (h->bnd) hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->bnd_mem, ec, n, -1, 1, err_misc);
    if (h->quad) hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->quad_g, ec, n, 2, 1, err_misc);      // g <- g C^2
    HIP_TRY(h, hipGetLastError());
    std::vector<int> flags(2 * (size_t)cap + 8);
    double sp[6];
    HIP_TRY(h, hipMemcpyAsync(flags.data(), changed, sizeof(int) * flags.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(sp, spread, sizeof sp, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int passes = 0;
    while (passes < cap && flags[(size_t)passes]) ++passes;
    const int* f_err_max = flags.data() + cap + 1;
    const int f_err_misc = flags[2 * (size_t)cap + 2];
    if (info) { info[0] = passes; info[1] = eq_log2_spread(sp); info[2] = eq_log2_spread(sp + 2); info[3] = eq_log2_spread(sp + 4); }
    if (passes == 0) return IPM_OK;                      // cap 0, or the data sit at the fixed point already: nothing to rewrite
    if (f_err_max[passes] || f_err_misc)                 // (the maxima of launch `passes` are those of the final factors)
        return fail(h, IPM_ERR_INVALID_INPUT, "ipm_equilibrate: a factor would push an entry of A, b, c, u or g out of the normal fp64 range; the handle stays unscaled");
    // ---- rewrite A and every value table derived from it, once
    if (h->sparse) {
        hipLaunchKernelGGL(eq_sparse_apply_kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, h->stream, S.rowptr, S.colind, h->d_rval, m, er, ec);
        hipLaunchKernelGGL(eq_sparse_apply_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, h->stream, S.colptr, S.rowind, h->d_cval, n, ec, er);
        const unsigned gb = (unsigned)((h->sm_nb + 255) / 256);
        if (h->small && h->sm_nb > 0)
            hipLaunchKernelGGL(eq_list_apply_kernel<unsigned short>, dim3(gb), dim3(256), 0, h->stream, h->sm_bptr, h->sm_bi, h->sm_bk, h->sm_bcol, h->sm_bcoef, (double*)nullptr, h->sm_nb, er, ec);
        if (h->list_form && h->sm_nb > 0)
            hipLaunchKernelGGL(eq_list_apply_kernel<int>, dim3(gb), dim3(256), 0, h->stream, h->sm_bptr, h->ls_bi, h->ls_bk, h->sm_bcol, h->sm_bcoef, h->ls_bak, h->sm_nb, er, ec);
        if (h->spf)
            hipLaunchKernelGGL(eq_spf_apply_kernel, dim3((unsigned)h->spF.nsn), dim3(256), 0, h->stream, h->spF.node, h->spF.rows, h->sp_fptr, h->sp_fcol, h->sp_fcoef, er, ec);
    } else {
        hipLaunchKernelGGL(eq_dense_apply_kernel, dim3((unsigned)m, (unsigned)((np / 2 + 255) / 256)), dim3(256), 0, h->stream, h->A, np, er, ec);
    }
    if (h->haveBC) {
        hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, h->b, er, m, 1, 0, err_misc);
        hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->c, ec, n, 1, 0, err_misc);
    }
    if (h->bnd) hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->bnd_mem, ec, n, -1, 0, err_misc);
    if (h->quad) hipLaunchKernelGGL(eq_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->quad_g, ec, n, 2, 0, err_misc);
    if (h->haveBC) enqueue_bc_norms(h);
    HIP_TRY(h, hipGetLastError());
    std::vector<int> he((size_t)mp + np);
    HIP_TRY(h, hipMemcpyAsync(he.data(), er, sizeof(int) * he.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->eq_r.resize((size_t)m); h->eq_c.resize((size_t)n);
    for (int i = 0; i < m; ++i) h->eq_r[(size_t)i] = ldexp(1.0, he[(size_t)i]);
    for (int j = 0; j < n; ++j) h->eq_c[(size_t)j] = ldexp(1.0, he[(size_t)mp + j]);
    h->scaled = true;
    h->predictor_valid = false; h->haveState = false;    // the iterate is set (or initialised) after the scaling
    return IPM_OK;
}

extern "C" int ipm_get_scaling(ipm_handle* h, double* r, double* c) {
    if (!h) return fail(h, IPM_ERR_INVALID_ARG, "ipm_get_scaling: NULL handle");
    if (r) for (int64_t i = 0; i < h->m; ++i) r[i] = h->scaled ? h->eq_r[(size_t)i] : 1.0;
    if (c) for (int64_t j = 0; j < h->n; ++j) c[j] = h->scaled ? h->eq_c[(size_t)j] : 1.0;
    return IPM_OK;
}
