// soc_capi_mabu_library.hip -- host side of libsoc_hip.so: the library method for a model with several dust components
// (kernels: soc_mabu_library.hip).
#include "soc_host.h"

#include <cstring>
#include <vector>

static void mlib_release(soc_ctx *c)
{
    c->qABS3.release();  c->qABU.release();  c->qSUM.release();  c->qMISS.release();  c->qRABS3.release();  c->qLib.release();
    for (int d = 0; d < SOC_MABU_LIB_DUSTS; d++) { c->qTab[d].release();  c->qE[d].release(); }
    c->mlib_cells = 0;  c->mlib_ndust = c->mlib_nout = 0;  c->mlib_have = 0;  c->mlib_tables = false;
}

#define MLIB_OPEN(c, who)                                                                                       \
    do {                                                                                                        \
        if (!(c)->mlib_cells || !(c)->qABS3 || !(c)->qSUM) return fail((c), SOC_ERR_STATE, who ": call soc_mabu_library_begin first");   \
    } while (0)

#pragma GCC visibility push(default)
extern "C" {

int soc_mabu_library_begin(soc_ctx *c, int64_t cells, int NDUST, int nout, int64_t *cells_fit)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (cells_fit) *cells_fit = 0;
    if (cells < 1 || cells > (int64_t)2147483647 || NDUST < 1 || NDUST > SOC_MABU_LIB_DUSTS || nout < 1 || nout > 4096)
        return fail(c, SOC_ERR_ARG, "soc_mabu_library_begin: cells=%lld NDUST=%d nout=%d (1 <= NDUST <= %d, the width of the miss mask; 1 <= nout <= 4096)",
                    (long long)cells, NDUST, nout, SOC_MABU_LIB_DUSTS);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    mlib_release(c);                                        // (a soc_mabu_library_begin that is still open is replaced)
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    // per cell: three absorptions, NDUST abundances, nout sums, a miss mask
    const size_t per_cell = 12 + (size_t)NDUST * 4 + (size_t)nout * 4 + 4, reserve = (size_t)1 << 30;
    const size_t need = (size_t)cells * per_cell;
    const int64_t fit = free_b > reserve ? (int64_t)((free_b - reserve) / per_cell) : 0;
    if (cells_fit) *cells_fit = fit;
    if (need + reserve > free_b)
        return fail(c, SOC_ERR_STATE, "soc_mabu_library_begin: %lld cells x %d dusts x %d columns need %.1f GB of device memory, %.1f GB are free (%lld cells fit: look the cells up in ranges)",
                    (long long)cells, NDUST, nout, need * 1e-9, free_b * 1e-9, (long long)fit);
    hipError_t e = c->qABS3.reset((size_t)cells * 3, c->stream);
    if (e == hipSuccess) e = c->qABU.reset((size_t)cells * NDUST, c->stream);
    if (e == hipSuccess) e = c->qSUM.reset((size_t)cells * nout, c->stream);
    if (e == hipSuccess) e = c->qMISS.reset((size_t)cells, c->stream);
    if (e == hipSuccess) e = c->qRABS3.reset((size_t)3 * NDUST, c->stream);
    if (e == hipSuccess) e = c->qLib.reset((size_t)NDUST, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->qABS3, 0, (size_t)cells * 12, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->qSUM, 0, (size_t)cells * nout * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->qMISS, 0, (size_t)cells * 4, c->stream);
    if (e != hipSuccess) {
        mlib_release(c);
        return fail(c, SOC_ERR_HIP, "soc_mabu_library_begin: %s", hipGetErrorString(e));
    }
    c->mlib_cells = cells;  c->mlib_ndust = NDUST;  c->mlib_nout = nout;
    return SOC_OK;
}

int soc_mabu_library_set(soc_ctx *c, int idust, int N, int NFREQ, float I0, float dI0, const float *I1, const float *dI1, const float *I2,
                         const float *dI2, const float *X, const float *Y, const float *Z, const float *E, int nout, const int32_t *ocol)
{
    if (!c) return SOC_ERR_ARG;
    MLIB_OPEN(c, "soc_mabu_library_set");
    if (idust < 0 || idust >= c->mlib_ndust) return fail(c, SOC_ERR_ARG, "soc_mabu_library_set: dust %d of %d", idust, c->mlib_ndust);
    if (N < 2 || N > 64 || NFREQ < 1 || NFREQ > 4096 || !I1 || !dI1 || !I2 || !dI2 || !X || !Y || !Z || !E)
        return fail(c, SOC_ERR_ARG, "soc_mabu_library_set: 2 <= N <= 64, 1 <= NFREQ <= 4096 and every table (N = %d, NFREQ = %d)", N, NFREQ);
    if (!ocol) nout = NFREQ;
    if (nout != c->mlib_nout)
        return fail(c, SOC_ERR_ARG, "soc_mabu_library_set: the library of dust %d gives %d columns, soc_mabu_library_begin reserved %d", idust, nout, c->mlib_nout);
    for (int s = 0; ocol && s < nout; s++)
        if (ocol[s] < 0 || ocol[s] >= NFREQ) return fail(c, SOC_ERR_ARG, "soc_mabu_library_set: ocol[%d] = %d of %d columns", s, ocol[s], NFREQ);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n1 = (size_t)N, n2 = n1 * n1, n3 = n2 * n1;
    std::vector<float> tab(2 * n1 + 2 * n2 + 4 * n3);       // the block of soc_library_set: I1 | dI1 | I2 | dI2 | X | Y | Z | E0
    float *t = tab.data();
    memcpy(t, I1, n1 * 4);  memcpy(t + n1, dI1, n1 * 4);
    memcpy(t + 2 * n1, I2, n2 * 4);  memcpy(t + 2 * n1 + n2, dI2, n2 * 4);
    float *x = t + 2 * n1 + 2 * n2;
    memcpy(x, X, n3 * 4);  memcpy(x + n3, Y, n3 * 4);  memcpy(x + 2 * n3, Z, n3 * 4);
    for (size_t b = 0; b < n3; b++) x[3 * n3 + b] = E[b * NFREQ];
    DevBuf<float> &dT = c->qTab[idust], &dE = c->qE[idust];
    c->mlib_have &= ~(1u << idust);
    HIPCHK(c, dT.reset(tab.size(), c->stream));
    HIPCHK(c, dE.reset(n3 * nout, c->stream));
    HIPCHK(c, hipMemcpy(dT, t, tab.size() * 4, hipMemcpyHostToDevice));
    if (ocol) {                                              // the output columns are chosen and ordered once, here
        std::vector<float> sel(n3 * nout);
        for (size_t b = 0; b < n3; b++)
            for (int s = 0; s < nout; s++) sel[b * nout + s] = E[b * NFREQ + ocol[s]];
        HIPCHK(c, hipMemcpy(dE, sel.data(), sel.size() * 4, hipMemcpyHostToDevice));
    } else {
        HIPCHK(c, hipMemcpy(dE, E, n3 * nout * 4, hipMemcpyHostToDevice));
    }
    SocLibTables L{};
    const float *p = dT;
    L.N = N;  L.nout = nout;  L.I0 = I0;  L.dI0 = dI0;
    L.I1 = p;  L.dI1 = p + n1;  L.I2 = p + 2 * n1;  L.dI2 = p + 2 * n1 + n2;
    L.X = p + 2 * n1 + 2 * n2;  L.Y = L.X + n3;  L.Z = L.Y + n3;  L.E0 = L.Z + n3;
    L.E = dE;
    HIPCHK(c, hipMemcpy(c->qLib.p + idust, &L, sizeof(L), hipMemcpyHostToDevice));
    c->mlib_have |= 1u << idust;
    return SOC_OK;
}

int soc_mabu_library_upload(soc_ctx *c, int64_t c0, int64_t n, const float *ABS3)
{
    if (!c || !ABS3) return SOC_ERR_ARG;
    MLIB_OPEN(c, "soc_mabu_library_upload");
    SOC_ROWS(c, "soc_mabu_library_upload", c0, n, c->mlib_cells);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->qABS3 + (size_t)c0 * 3, ABS3, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (the host buffer may be a temporary)
    return SOC_OK;
}

int soc_mabu_library_set_tables(soc_ctx *c, const float *ABU, const double *RABS3)
{
    if (!c || !ABU || !RABS3) return SOC_ERR_ARG;
    MLIB_OPEN(c, "soc_mabu_library_set_tables");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->qABU, ABU, (size_t)c->mlib_cells * c->mlib_ndust * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->qRABS3, RABS3, (size_t)3 * c->mlib_ndust * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mlib_tables = true;
    return SOC_OK;
}

int soc_mabu_library_solve(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    MLIB_OPEN(c, "soc_mabu_library_solve");
    if (!c->mlib_tables) return fail(c, SOC_ERR_STATE, "soc_mabu_library_solve: call soc_mabu_library_set_tables first");
    const unsigned all = c->mlib_ndust >= 32 ? 0xffffffffu : ((1u << c->mlib_ndust) - 1u);
    if (c->mlib_have != all) {
        int d = 0;
        while ((c->mlib_have >> d) & 1u) d++;
        return fail(c, SOC_ERR_STATE, "soc_mabu_library_solve: dust %d of %d has no library (soc_mabu_library_set)", d, c->mlib_ndust);
    }
    HIPCHK(c, hipSetDevice(c->device));
    SocMabuLib A{};
    A.n = c->mlib_cells;  A.NDUST = c->mlib_ndust;  A.nout = c->mlib_nout;
    A.ABS3 = c->qABS3;  A.ABU = c->qABU;  A.RABS3 = c->qRABS3;  A.LIB = c->qLib;  A.SUM = c->qSUM;  A.MISS = c->qMISS;
    HIPCHK(c, soc_launch_mabu_library(A, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_mabu_library_download(soc_ctx *c, int64_t c0, int64_t n, float *SUM)
{
    if (!c || !SUM) return SOC_ERR_ARG;
    MLIB_OPEN(c, "soc_mabu_library_download");
    SOC_ROWS(c, "soc_mabu_library_download", c0, n, c->mlib_cells);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(SUM, c->qSUM + (size_t)c0 * c->mlib_nout, (size_t)n * c->mlib_nout * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_mabu_library_misses(soc_ctx *c, int64_t c0, int64_t n, uint32_t *MISS)
{
    if (!c || !MISS) return SOC_ERR_ARG;
    MLIB_OPEN(c, "soc_mabu_library_misses");
    SOC_ROWS(c, "soc_mabu_library_misses", c0, n, c->mlib_cells);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(MISS, c->qMISS + (size_t)c0, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_mabu_library_end(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    mlib_release(c);
    return SOC_OK;
}

int soc_mabu_gather_rows(soc_ctx *c, const int32_t *idx, int64_t n, float *out)
{
    if (!c || !idx || !out) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->mABS || !c->aSum) return fail(c, SOC_ERR_STATE, "soc_mabu_gather_rows: call soc_mabu_begin first");
    if (n < 1 || n > (int64_t)2147483647) return fail(c, SOC_ERR_ARG, "soc_mabu_gather_rows: n = %lld", (long long)n);
    for (int64_t s = 0; s < n; s++)
        if (idx[s] < 0 || (int64_t)idx[s] >= c->a2e_cells)
            return fail(c, SOC_ERR_ARG, "soc_mabu_gather_rows: idx[%lld] = %d of %lld resident cells", (long long)s, idx[s], (long long)c->a2e_cells);
    HIPCHK(c, hipSetDevice(c->device));
    const int NFREQ = c->a2e_res_nfreq;
    DevBuf<int> dI;
    DevBuf<float> dO;
    HIPCHK(c, dI.reset((size_t)n, c->stream));
    HIPCHK(c, dO.reset((size_t)n * NFREQ, c->stream));
    HIPCHK(c, hipMemcpyAsync(dI, idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_mabu_gather_rows(n, NFREQ, c->aSum, dI, dO, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, dO, (size_t)n * NFREQ * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
