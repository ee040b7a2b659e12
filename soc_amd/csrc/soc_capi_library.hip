// soc_capi_library.hip -- host side of libsoc_hip.so: the library method for dust emission (kernels: soc_library.hip).
#include "soc_host.h"

#include <algorithm>
#include <cstring>
#include <vector>

// the float a table key stands for (soc_library.hip: lib_okey)
static float lib_unkey(unsigned k)
{
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// first bin centre and bin width of an axis whose values span [a, b] (soc_library.py:137-142, :152-157, :165-170), in fp32
static void lib_axis(float a, float b, int N, float *I, float *dI)
{
    const float d = (b - a) / (float)N + 0.1f;
    a = a - d;
    b = b + d;
    float w = 1.001f * (b - a) / (float)N;
    w = w < 1.0e-30f ? 1.0e-30f : w;
    w = w > 1.0e30f ? 1.0e30f : w;
    *dI = w;
    *I = a + 0.499f * w;
}

static int lib_sorted_misses(soc_ctx *c, int64_t base, int32_t *miss, int64_t *nmiss)
{
    unsigned long long m = 0;
    HIPCHK(c, hipMemcpyAsync(&m, c->lCount, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m && miss) {
        int32_t *dst = miss + *nmiss;
        HIPCHK(c, hipMemcpy(dst, c->lMiss, (size_t)m * 4, hipMemcpyDeviceToHost));
        std::sort(dst, dst + m);                             // the lanes append in the order they run: ascending here
        if (base) for (unsigned long long s = 0; s < m; s++) dst[s] += (int32_t)base;
    }
    *nmiss += (int64_t)m;
    return SOC_OK;
}

static void lib_solve_args(soc_ctx *c, SocLibSolve &A)
{
    const size_t N = (size_t)c->lib_N, N2 = N * N, N3 = N2 * N;
    const float *t = c->lTab;
    A.N = c->lib_N;  A.nout = c->lib_nout;  A.I0 = c->lib_I0;  A.dI0 = c->lib_dI0;
    A.I1 = t;  A.dI1 = t + N;  A.I2 = t + 2 * N;  A.dI2 = t + 2 * N + N2;
    A.X = t + 2 * N + 2 * N2;  A.Y = A.X + N3;  A.Z = A.Y + N3;  A.E0 = A.Z + N3;
    A.E = c->lE;  A.miss = c->lMiss;  A.nmiss = c->lCount;
}

#pragma GCC visibility push(default)
extern "C" {

int soc_library_set(soc_ctx *c, int N, int NFREQ, float I0, float dI0, const float *I1, const float *dI1, const float *I2, const float *dI2,
                    const float *X, const float *Y, const float *Z, const float *E, int nout, const int32_t *ocol)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (N == 0) {                                            // forget the library
        c->lTab.release();  c->lE.release();  c->lMiss.release();  c->lCount.release();
        c->lib_N = c->lib_nout = 0;
        return SOC_OK;
    }
    if (N < 2 || N > 64 || NFREQ < 1 || NFREQ > 4096 || !I1 || !dI1 || !I2 || !dI2 || !X || !Y || !Z || !E)
        return fail(c, SOC_ERR_ARG, "soc_library_set: 2 <= N <= 64, 1 <= NFREQ <= 4096 and every table (N = %d, NFREQ = %d)", N, NFREQ);
    if (!ocol) nout = NFREQ;
    if (nout < 1 || nout > 4096) return fail(c, SOC_ERR_ARG, "soc_library_set: nout = %d", nout);
    for (int s = 0; ocol && s < nout; s++)
        if (ocol[s] < 0 || ocol[s] >= NFREQ) return fail(c, SOC_ERR_ARG, "soc_library_set: ocol[%d] = %d of %d columns", s, ocol[s], NFREQ);
    const size_t n1 = (size_t)N, n2 = n1 * n1, n3 = n2 * n1;
    std::vector<float> tab(2 * n1 + 2 * n2 + 4 * n3);
    float *t = tab.data();
    memcpy(t, I1, n1 * 4);  memcpy(t + n1, dI1, n1 * 4);
    memcpy(t + 2 * n1, I2, n2 * 4);  memcpy(t + 2 * n1 + n2, dI2, n2 * 4);
    float *x = t + 2 * n1 + 2 * n2;
    memcpy(x, X, n3 * 4);  memcpy(x + n3, Y, n3 * 4);  memcpy(x + 2 * n3, Z, n3 * 4);
    for (size_t b = 0; b < n3; b++) x[3 * n3 + b] = E[b * NFREQ];
    HIPCHK(c, c->lTab.reset(tab.size(), c->stream));
    HIPCHK(c, c->lE.reset(n3 * nout, c->stream));
    HIPCHK(c, c->lCount.reserve(1, c->stream));
    HIPCHK(c, hipMemcpy(c->lTab, t, tab.size() * 4, hipMemcpyHostToDevice));
    if (ocol) {                                              // the output columns are chosen and ordered once, here
        std::vector<float> sel(n3 * nout);
        for (size_t b = 0; b < n3; b++)
            for (int s = 0; s < nout; s++) sel[b * nout + s] = E[b * NFREQ + ocol[s]];
        HIPCHK(c, hipMemcpy(c->lE, sel.data(), sel.size() * 4, hipMemcpyHostToDevice));
    } else {
        HIPCHK(c, hipMemcpy(c->lE, E, n3 * nout * 4, hipMemcpyHostToDevice));
    }
    c->lib_N = N;  c->lib_nout = nout;  c->lib_I0 = I0;  c->lib_dI0 = dI0;
    return SOC_OK;
}

int soc_library_solve(soc_ctx *c, int64_t n, const float *ABS3, float *EMI, int32_t *miss, int64_t *nmiss)
{
    if (!c || !ABS3 || !EMI || !nmiss) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->lib_N) return fail(c, SOC_ERR_STATE, "soc_library_solve: call soc_library_set first");
    if (n < 1 || n > (int64_t)2147483647) return fail(c, SOC_ERR_ARG, "soc_library_solve: n = %lld", (long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    // cells per launch: at most 2^22, and fewer where the rows are long, so that the device copy of the output stays within 1 GiB
    const int64_t step = std::max<int64_t>(1, std::min<int64_t>((int64_t)1 << 22, ((int64_t)1 << 28) / c->lib_nout));
    const int64_t most = std::min(n, step);
    DevBuf<float> dA, dE;
    HIPCHK(c, dA.reset((size_t)most * 3, c->stream));
    HIPCHK(c, dE.reset((size_t)most * c->lib_nout, c->stream));
    HIPCHK(c, c->lMiss.reserve((size_t)most, c->stream));
    SocLibSolve A{};
    lib_solve_args(c, A);
    A.ABS = dA;  A.stride = 3;  A.c0 = 0;  A.c1 = 1;  A.c2 = 2;  A.EMI = dE;
    *nmiss = 0;
    for (int64_t c0 = 0; c0 < n; c0 += step) {
        A.n = std::min(step, n - c0);
        HIPCHK(c, hipMemcpyAsync(dA, ABS3 + (size_t)c0 * 3, (size_t)A.n * 12, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->lCount, 0, 8, c->stream));
        HIPCHK(c, soc_launch_library_solve(A, c->stream));
        HIPCHK(c, hipMemcpyAsync(EMI + (size_t)c0 * c->lib_nout, dE, (size_t)A.n * c->lib_nout * 4, hipMemcpyDeviceToHost, c->stream));
        int r = lib_sorted_misses(c, c0, miss, nmiss);
        if (r) return r;
    }
    return SOC_OK;
}

int soc_library_solve_resident(soc_ctx *c, const int32_t *col, int32_t *miss, int64_t *nmiss)
{
    if (!c || !col || !nmiss) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->lib_N) return fail(c, SOC_ERR_STATE, "soc_library_solve_resident: call soc_library_set first");
    if (!c->aAll || !c->aSum) return fail(c, SOC_ERR_STATE, "soc_library_solve_resident: call soc_a2e_resident_begin first");
    if (c->lib_nout != c->a2e_res_nfreq)
        return fail(c, SOC_ERR_STATE, "soc_library_solve_resident: the library gives %d columns, a resident row holds %d", c->lib_nout, c->a2e_res_nfreq);
    for (int s = 0; s < 3; s++)
        if (col[s] < 0 || col[s] >= c->a2e_res_nfreq) return fail(c, SOC_ERR_ARG, "soc_library_solve_resident: column %d of %d", col[s], c->a2e_res_nfreq);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->lMiss.reserve((size_t)c->a2e_cells, c->stream));
    SocLibSolve A{};
    lib_solve_args(c, A);
    A.n = c->a2e_cells;  A.ABS = c->aAll;  A.stride = c->a2e_res_nfreq;  A.c0 = col[0];  A.c1 = col[1];  A.c2 = col[2];  A.EMI = c->aSum;
    HIPCHK(c, hipMemsetAsync(c->lCount, 0, 8, c->stream));
    HIPCHK(c, soc_launch_library_solve(A, c->stream));
    *nmiss = 0;
    return lib_sorted_misses(c, 0, miss, nmiss);
}

int soc_library_build(soc_ctx *c, int N, int64_t cells, const float *ABS3, const int32_t *col, float *I0, float *dI0, float *I1, float *dI1,
                      float *I2, float *dI2, int32_t *IND, float *XX, float *YY, float *ZZ)
{
    if (!c || !I0 || !dI0 || !I1 || !dI1 || !I2 || !dI2 || !IND || !XX || !YY || !ZZ) return SOC_ERR_ARG;
    FLUSH(c);
    if (N < 2 || N > 64 || cells < 1 || cells > (int64_t)2147483647) return fail(c, SOC_ERR_ARG, "soc_library_build: N = %d (2..64), cells = %lld", N, (long long)cells);
    HIPCHK(c, hipSetDevice(c->device));
    SocLibBuild A{};
    A.cells = cells;  A.N = N;
    DevBuf<float> dA;
    if (ABS3) {
        HIPCHK(c, dA.reset((size_t)cells * 3, c->stream));
        HIPCHK(c, hipMemcpyAsync(dA, ABS3, (size_t)cells * 12, hipMemcpyHostToDevice, c->stream));
        A.ABS = dA;  A.stride = 3;  A.c0 = 0;  A.c1 = 1;  A.c2 = 2;
    } else {
        if (!col) return fail(c, SOC_ERR_ARG, "soc_library_build: ABS3, or the three columns of the resident absorptions");
        if (!c->aAll || cells != c->a2e_cells) return fail(c, SOC_ERR_STATE, "soc_library_build: %lld cells, %lld are resident (soc_a2e_resident_begin)", (long long)cells, (long long)c->a2e_cells);
        for (int s = 0; s < 3; s++)
            if (col[s] < 0 || col[s] >= c->a2e_res_nfreq) return fail(c, SOC_ERR_ARG, "soc_library_build: column %d of %d", col[s], c->a2e_res_nfreq);
        A.ABS = c->aAll;  A.stride = c->a2e_res_nfreq;  A.c0 = col[0];  A.c1 = col[1];  A.c2 = col[2];
    }
    const size_t n1 = (size_t)N, n2 = n1 * n1, n3 = n2 * n1;
    DevBuf<unsigned> dTab;                                   // min | max | count of one sweep
    DevBuf<float> dGrid, dXYZ;                               // I1 | dI1 | I2 | dI2;  XX | YY | ZZ
    DevBuf<unsigned long long> dBest;
    DevBuf<int> dInd;
    HIPCHK(c, dTab.reset(3 * n2, c->stream));
    HIPCHK(c, dGrid.reset(2 * n1 + 2 * n2, c->stream));
    HIPCHK(c, dXYZ.reset(3 * n3, c->stream));
    HIPCHK(c, dBest.reset(n3, c->stream));
    HIPCHK(c, dInd.reset(n3, c->stream));
    A.I1 = dGrid;  A.dI1 = A.I1 + n1;  A.I2 = A.dI1 + n1;  A.dI2 = A.I2 + n2;
    std::vector<unsigned> tab(3 * n2);
    for (int level = 0; level < 3; level++) {
        const size_t entries = level == 0 ? 1 : (level == 1 ? n1 : n2);
        for (size_t e = 0; e < entries; e++) { tab[e] = 0xffffffffu;  tab[entries + e] = 0u;  tab[2 * entries + e] = 0u; }
        HIPCHK(c, hipMemcpyAsync(dTab, tab.data(), 3 * entries * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, soc_launch_library_range(A, level, dTab, c->stream));
        HIPCHK(c, hipMemcpyAsync(tab.data(), dTab, 3 * entries * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (level == 0) {
            lib_axis(lib_unkey(tab[0]), lib_unkey(tab[1]), N, I0, dI0);
            A.I0 = *I0;  A.dI0 = *dI0;
            continue;
        }
        float *I = level == 1 ? I1 : I2, *dI = level == 1 ? dI1 : dI2;
        const unsigned need = level == 1 ? 1u : 2u;          // a window needs one cell on axis 1, two on axis 2 (:149, :162)
        for (size_t e = 0; e < entries; e++) {
            if (tab[2 * entries + e] < need) { I[e] = 100.0f;  dI[e] = 0.001f; }
            else lib_axis(lib_unkey(tab[e]), lib_unkey(tab[entries + e]), N, &I[e], &dI[e]);
        }
        if (level == 2) {                                    // an undefined (i, j) takes the grid of the last defined one in raster order (:178-185)
            float a = 100.0f, b = 0.001f;
            for (size_t e = 0; e < entries; e++) {
                if (I[e] < 99.0f) { a = I[e];  b = dI[e]; }
                else { I[e] = a;  dI[e] = b; }
            }
        }
        float *dst = dGrid.p + (level == 1 ? 0 : 2 * n1);
        HIPCHK(c, hipMemcpy(dst, I, entries * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dst + entries, dI, entries * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemsetAsync(dBest, 0xff, n3 * 8, c->stream));
    HIPCHK(c, soc_launch_library_pick(A, dBest, dInd, dXYZ, dXYZ.p + n3, dXYZ.p + 2 * n3, c->stream));
    HIPCHK(c, hipMemcpyAsync(IND, dInd, n3 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(XX, dXYZ, n3 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(YY, dXYZ.p + n3, n3 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ZZ, dXYZ.p + 2 * n3, n3 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
