// host_lu.h -- host side, unit 8: LU with partial pivoting for general square systems (getrf_f64.h): ipm_lu_factor, ipm_lu_solve.
#pragma once
// ------------------------------------------------------------------------------- general square systems (getrf_f64.h)
// No handle: the call owns a stream and its device memory and releases both before it returns.
namespace {
struct LuRun {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    ~LuRun() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : allocs) guarded_free(stream, p, /*pool=*/false);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int alloc(void** p, size_t bytes, const char* what, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
        hipError_t e = guarded_alloc(device, stream, p, bytes, /*pool=*/false, file, line);      // test knob IPM_TEST_ALLOC_GUARD (host_handle.h)
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(nullptr, IPM_ERR_WORKSPACE, "lu: cannot allocate %zu bytes of device memory for %s: %s", bytes, what, hipGetErrorString(e));
        }
        allocs.push_back(*p);
        if ((e = alloc_fill(*p, bytes, stream)) != hipSuccess)       // test knob IPM_TEST_ALLOC_FILL (host_handle.h)
            return fail(nullptr, IPM_ERR_HIP, "lu: filling %s failed: %s", what, hipGetErrorString(e));
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
