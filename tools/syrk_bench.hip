// syrk_bench.hip -- A/B timing of the dominant kernel (B = A diag(d) A^T) in ONE process, interleaved rounds
// (cdna guide 5.4 rule 24): the generic gemm_nt_f64_kernel<128,128,16,2,2,true> against adat_syrk_kernel, on
// random data, with a bit-for-bit comparison of the two results.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/bin/syrk_bench tools/syrk_bench.hip
//   tools/bin/syrk_bench [m n rounds]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "../interiorpointmethod_amd/csrc/gemm_nt_f64.h"
#include "../interiorpointmethod_amd/csrc/adat_syrk_f64.h"
using namespace ipm;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s failed: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static std::vector<int> tile_order(int nT) {
    std::vector<int> order; const int PB = 8;
    for (int I = 0; I * PB < nT; ++I)
        for (int J = 0; J <= I; ++J)
            for (int ti = I * PB; ti < nT && ti < (I + 1) * PB; ++ti)
                for (int tj = J * PB; tj <= ti && tj < (J + 1) * PB; ++tj) order.push_back((ti << 16) | tj);
    return order;
}

// context probes: what the kernel sees inside the solver -- 2.8 ms of a nearly idle chip (the Cholesky pivot chain) and
// ~0.5 GB of other traffic (B, L, the GEMV passes) between two formations
__global__ void spin_kernel(long long cycles, double* sink) {
    const long long t0 = clock64();
    double x = 1.0;
    while (clock64() - t0 < cycles) x = x * 1.0000001 + 1e-9;
    if (x == 0.123) *sink = x;
}
__global__ void stream_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) dst[i] = src[i] + 1.0;
}

int main(int argc, char** argv) {
    int m = argc > 1 ? atoi(argv[1]) : 4096, n = argc > 2 ? atoi(argv[2]) : 8192, rounds = argc > 3 ? atoi(argv[3]) : 10;
    const size_t na = (size_t)m * n;
    std::vector<double> hA(na), hd(n);
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
    for (auto& v : hA) v = 2.0 * rnd() - 1.0;
    for (auto& v : hd) v = 0.5 + rnd();
    double *A, *d, *B0, *B1, *slab; int* ord;
    CK(hipMalloc(&A, na * 8)); CK(hipMalloc(&d, n * 8)); CK(hipMalloc(&B0, (size_t)m * m * 8)); CK(hipMalloc(&B1, (size_t)m * m * 8));
    CK(hipMalloc(&slab, (size_t)kSlabTiles * 128 * 128 * 8));
    auto ho = tile_order(m / 128);
    CK(hipMalloc(&ord, ho.size() * 4));
    CK(hipMemcpy(A, hA.data(), na * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d, hd.data(), n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(ord, ho.data(), ho.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(B0, 0, (size_t)m * m * 8)); CK(hipMemset(B1, 0, (size_t)m * m * 8));
    hipStream_t st; CK(hipStreamCreate(&st));
    auto run_old = [&]() {
        GemmNT g; memset(&g, 0, sizeof g);
        g.batch = 1; g.batch2 = 1; g.tile_order = ord; g.P = A; g.ldp = n; g.Q = A; g.ldq = n; g.w = d; g.C = B0; g.ldc = m;
        g.M = m; g.N = m; g.K = n; g.alpha = 1.0; g.beta = 0.0; g.lower = 1; g.unit_diag_from = -1;
        CK((launch_gemm_nt<128, 128, 16, 2, 2>(g, st, slab, 512)));
    };
    auto run_new = [&]() { CK(launch_adat_syrk(A, n, d, B1, m, m, n, -1, nullptr, ord, st, slab, 512)); };
    run_old(); run_new(); CK(hipStreamSynchronize(st));
    std::vector<double> h0((size_t)m * m), h1((size_t)m * m);
    CK(hipMemcpy(h0.data(), B0, h0.size() * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(h1.data(), B1, h1.size() * 8, hipMemcpyDeviceToHost));
    size_t ndiff = 0; double maxd = 0;
    for (int i = 0; i < m; ++i) for (int j = 0; j <= (i | 127) && j < m; ++j) {
        double a = h0[(size_t)i * m + j], b = h1[(size_t)i * m + j];
        if (a != b) { ++ndiff; maxd = std::max(maxd, fabs(a - b)); }
    }
    printf("compare old vs new: %zu differing entries, max |diff| %.3e (B[1][0]=%.6f)\n", ndiff, maxd, h0[(size_t)m]);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> t_old, t_new;
    const int reps = 5;
    for (int r = 0; r < rounds; ++r) {
        float ms;
        CK(hipEventRecord(e0, st)); for (int i = 0; i < reps; ++i) run_old(); CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1)); t_old.push_back(ms / reps);
        CK(hipEventRecord(e0, st)); for (int i = 0; i < reps; ++i) run_new(); CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1)); t_new.push_back(ms / reps);
    }
    auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    if (argc > 4 && !strcmp(argv[4], "upd")) {
        // the bulk trailing update of a Cholesky step in isolation: B(i,j) -= L(i,k) L(j,k)^T on the lower tiles below block
        // row/column kb, K = 128 (what enqueue_factor launches on the bulk stream), for a few step indices
        for (int kb : {0, 1, 4, 9, 15, 23}) {
            const int rem = m - (kb + 1) * 128;
            if (rem <= 128) continue;
            GemmNT u; memset(&u, 0, sizeof u);
            u.batch = 1; u.batch2 = 1; u.unit_diag_from = -1;
            double* panel = B0 + (size_t)(kb + 1) * 128 * m + (size_t)kb * 128;
            u.P = panel; u.ldp = m; u.Q = panel; u.ldq = m; u.C = B0 + (size_t)(kb + 1) * 128 * (m + 1); u.ldc = m;
            u.M = rem; u.N = rem; u.K = 128; u.alpha = -1e-9; u.beta = 1.0; u.lower = 1;
            std::vector<float> t;
            for (int r = 0; r < 7; ++r) {
                float ms; CK(hipEventRecord(e0, st));
                for (int i = 0; i < 10; ++i) CK((launch_gemm_nt<128, 128, 16, 2, 2>(u, st, nullptr, 512, 1)));
                CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms * 100.f);
            }
            const int nt = rem / 128, tiles = nt * (nt + 1) / 2 - 1;
            printf("  trailing update after step %2d: %4d tiles, K = 128: %.1f us per launch (median of 7 x 10)  = %.1f TFLOP/s\n", kb, tiles, med(t),
                   2.0 * tiles * 128.0 * 128.0 * 128.0 / (med(t) * 1e-6) * 1e-12);
        }
    } else if (argc > 4) {      // context probes (new kernel only): time ONE formation after (a) nothing, (b) an idle gap, (c) a cache flush, (d) both
        double *f0, *f1; const size_t fn = (size_t)48 << 20;     // 2 x 384 MB
        CK(hipMalloc(&f0, fn * 8)); CK(hipMalloc(&f1, fn * 8)); CK(hipMemset(f0, 0, fn * 8));
        const char* names[4] = {"back to back", "after 2.8 ms on one workgroup", "after 0.77 GB of other traffic", "after both"};
        for (int mode = 0; mode < 4; ++mode) {
            std::vector<float> t;
            for (int r = 0; r < 12; ++r) {
                run_new();
                if (mode & 2) hipLaunchKernelGGL(stream_kernel, dim3(2048), dim3(256), 0, st, f0, f1, fn);
                if (mode & 1) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, st, (long long)(2.8e-3 * 100e6 * 24), slab);   // clock64 ~ shader clock; ~2.8 ms at 2.4 GHz
                float ms;
                CK(hipEventRecord(e0, st)); run_new(); CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms);
            }
            printf("  one formation %-34s: median %.4f ms  min %.4f\n", names[mode], med(t), *std::min_element(t.begin(), t.end()));
        }
    }
    auto mn = [](std::vector<float> v) { return *std::min_element(v.begin(), v.end()); };
    const double fl = (double)m * m * n;
    printf("m=%d n=%d  generic: median %.4f ms (%.1f TF) min %.4f | adat_syrk: median %.4f ms (%.1f TF, %.3f of 78.6) min %.4f\n", m, n,
           med(t_old), fl / med(t_old) * 1e-9, mn(t_old), med(t_new), fl / med(t_new) * 1e-9, fl / med(t_new) * 1e-9 / 78.6, mn(t_new));
    return 0;
}
