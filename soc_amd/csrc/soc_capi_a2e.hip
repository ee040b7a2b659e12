// soc_capi_a2e.hip -- host side of libsoc_hip.so: stochastically heated grains (A2E), the equilibrium-temperature solvers and the
// multi-dust stage (kernels: soc_a2e.hip, soc_a2e_pre.hip, soc_mabu.hip).
#include "soc_host.h"

#include <algorithm>
#include <vector>

#pragma GCC visibility push(default)
extern "C" {

int soc_a2e_set_size(soc_ctx *c, int NE, int NFREQ, int noIw, const float *Iw, const int32_t *L1,
                     const int32_t *L2, const float *Tdown, const float *EA, const int32_t *Ibeg, const float *AF)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (NE < 3 || NE > 280 || NFREQ < 2 || noIw < 0 || !Iw || !L1 || !L2 || !Tdown || !EA || !Ibeg || !AF)
        return fail(c, SOC_ERR_ARG, "soc_a2e_set_size: bad arguments (3 <= NE <= 280, NFREQ >= 2)");
    int shape[3];
    if (!soc_a2e_shape(NE, NFREQ, shape))                   // (refused here, with the tables of the size before untouched, not at the launch)
        return fail(c, SOC_ERR_ARG, "soc_a2e_set_size: NE = %d with NFREQ = %d needs %d bytes of LDS for one cell, the limit is %d",
                    NE, NFREQ, shape[2], SOC_A2E_LDS);
    // pair tables in the reference's (l, u) loop order; validate every window on the host
    const int npair = (NE * NE - NE) / 2;
    std::vector<int> first(npair), last(npair), off(npair), dst(npair);
    long long iw = 0;
    int e = 0;
    for (int l = 0; l < NE - 1; l++) {
        for (int u = l + 1; u < NE; u++, e++) {
            const int i0 = L1[l * NE + u], i1 = L2[l * NE + u];
            if (i1 >= i0 && (i0 < 0 || i1 >= NFREQ))
                return fail(c, SOC_ERR_ARG, "soc_a2e_set_size: window [%d,%d] of pair (l=%d,u=%d) outside 0..%d", i0, i1, l, u, NFREQ - 1);
            first[e] = i0;  last[e] = i1;  off[e] = (int)iw;  dst[e] = (u * u - u) / 2 + l;
            if (i1 >= i0) iw += i1 - i0 + 1;
        }
    }
    if (iw != noIw) return fail(c, SOC_ERR_ARG, "soc_a2e_set_size: windows need %lld weights, noIw = %d", iw, noIw);
    for (int f = 0; f < NFREQ; f++)
        if (Ibeg[f] < 0 || Ibeg[f] > NE) return fail(c, SOC_ERR_ARG, "soc_a2e_set_size: Ibeg[%d] = %d", f, Ibeg[f]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->aIw.reset((size_t)noIw, c->stream));
    for (DevBuf<int> *b : { &c->aFirst, &c->aLast, &c->aIwOff, &c->aDst }) HIPCHK(c, b->reset((size_t)npair, c->stream));
    HIPCHK(c, c->aTdown.reset((size_t)NE, c->stream));
    HIPCHK(c, c->aEA.reset((size_t)NE * NFREQ, c->stream));
    HIPCHK(c, c->aIbeg.reset((size_t)NFREQ, c->stream));
    HIPCHK(c, c->aAF.reset((size_t)NFREQ, c->stream));
    if (noIw) HIPCHK(c, hipMemcpy(c->aIw, Iw, (size_t)noIw * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->aFirst, first.data(), (size_t)npair * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->aLast, last.data(), (size_t)npair * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->aIwOff, off.data(), (size_t)npair * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->aDst, dst.data(), (size_t)npair * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->aTdown, Tdown, (size_t)NE * 4, hipMemcpyHostToDevice));
    {   // transposed on the way: EAT[i * NFREQ + f] = EA[f * NE + i], so that the lanes of the emission loop (one
        // frequency each) read neighbouring words (the sum over the enthalpy bins keeps its order)
        std::vector<float> eat((size_t)NE * NFREQ);
        for (int f = 0; f < NFREQ; f++)
            for (int i = 0; i < NE; i++) eat[(size_t)i * NFREQ + f] = EA[(size_t)f * NE + i];
        HIPCHK(c, hipMemcpy(c->aEA, eat.data(), (size_t)NE * NFREQ * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemcpy(c->aIbeg, Ibeg, (size_t)NFREQ * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->aAF, AF, (size_t)NFREQ * 4, hipMemcpyHostToDevice));
    if (NFREQ != c->a2e_NFREQ) { c->aABS.release();  c->aEMIT.release(); }      // (a batch uploaded for another NFREQ is none: soc_a2e_run)
    c->a2e_NE = NE;  c->a2e_NFREQ = NFREQ;  c->a2e_npair = npair;  c->a2e_noIw = noIw;
    c->a2e_pol_set = false;                                 // (the weights belong to a size: soc_a2e_set_size_aalg gives those of this one)
    return SOC_OK;
}

int soc_a2e_launch_shape(soc_ctx *c, int out[3])
{
    if (!c || !out) return SOC_ERR_ARG;
    if (c->a2e_NE == 0) return fail(c, SOC_ERR_STATE, "soc_a2e_launch_shape: call soc_a2e_set_size first");
    (void)soc_a2e_shape(c->a2e_NE, c->a2e_NFREQ, out);        // (fits: soc_a2e_set_size refuses a size that does not)
    return SOC_OK;
}

static int a2e_reserve(soc_ctx *c, int batch)
{
    if (c->a2e_NE == 0) return fail(c, SOC_ERR_STATE, "A2E: call soc_a2e_set_size first");
    if (batch < 1) return fail(c, SOC_ERR_ARG, "A2E: batch = %d", batch);
    HIPCHK(c, c->aABS.reserve((size_t)batch * c->a2e_NFREQ, c->stream));
    HIPCHK(c, c->aEMIT.reserve((size_t)batch * c->a2e_NFREQ, c->stream));
    return SOC_OK;
}

int soc_a2e_upload(soc_ctx *c, int batch, const float *AABS)
{
    if (!c || !AABS) return SOC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int r = a2e_reserve(c, batch);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(c->aABS, AABS, (size_t)batch * c->a2e_NFREQ * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

// the kernel's arguments with the tables of the current size (soc_a2e_set_size) filled in; the cells are the caller's
static SocA2EArgs a2e_tables(const soc_ctx *c)
{
    SocA2EArgs A{};
    A.NE = c->a2e_NE;  A.NFREQ = c->a2e_NFREQ;  A.npair = c->a2e_npair;
    A.Iw = c->aIw;  A.pair_first = c->aFirst;  A.pair_last = c->aLast;  A.pair_iw = c->aIwOff;  A.pair_dst = c->aDst;
    A.Tdown = c->aTdown;  A.EA = c->aEA;  A.Ibeg = c->aIbeg;  A.AF = c->aAF;
    return A;
}

int soc_a2e_run(soc_ctx *c, int batch)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->a2e_NE == 0 || batch < 1 || (size_t)batch * c->a2e_NFREQ > c->aEMIT.n) return fail(c, SOC_ERR_STATE, "soc_a2e_run: upload a batch first");
    SocA2EArgs A = a2e_tables(c);
    A.batch = batch;  A.AABS = c->aABS;  A.AEMIT = c->aEMIT;
    HIPCHK(c, soc_launch_a2e_dosolve(A, c->stream));
    return SOC_OK;
}

int soc_a2e_download(soc_ctx *c, int batch, float *AEMIT)
{
    if (!c || !AEMIT) return SOC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (batch < 1 || !c->aEMIT || (size_t)batch * c->a2e_NFREQ > c->aEMIT.n) return fail(c, SOC_ERR_ARG, "soc_a2e_download: batch = %d", batch);
    HIPCHK(c, hipMemcpyAsync(AEMIT, c->aEMIT, (size_t)batch * c->a2e_NFREQ * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

// ---- config 5 with the cells resident in HBM ----
static void resident_release(soc_ctx *c)
{
    c->aAll.release();  c->aSum.release();  c->aPSum.release();  c->aAalg.release();
    c->aTeq.release();  c->aXX.release();
    c->a2e_cells = 0;  c->a2e_pol_set = false;  c->teq_keep = false;  c->teq_nsizes = 0;
}

// aAll | aSum, zeroed, for cells x NFREQ floats; with polarised output aPSum, zeroed, and aAalg (else neither).  Both begins come here;
// after an error the caller releases whatever it holds
static hipError_t resident_alloc(soc_ctx *c, int64_t cells, int NFREQ, bool polarised)
{
    const size_t n = (size_t)cells * NFREQ;
    hipError_t e = c->aAll.reset(n, c->stream);
    if (e == hipSuccess) e = c->aSum.reset(n, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->aSum, 0, n * 4, c->stream);
    if (polarised) {
        if (e == hipSuccess) e = c->aPSum.reset(n, c->stream);
        if (e == hipSuccess) e = c->aAalg.reset((size_t)cells * 2, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->aPSum, 0, n * 4, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->aAalg, 0xff, (size_t)cells * 8, c->stream);    // (NaN: rows never uploaded are aligned for no size)
    } else {
        c->aPSum.release();  c->aAalg.release();
    }
    c->a2e_pol_set = false;
    c->teq_nsizes = 0;                                      // (temperatures kept for the cells of a block before are none of this one's)
    return e;
}

// rows [c0, c0 + n) of a resident block, c->a2e_res_nfreq floats each, from or to the host; the range is the caller's to check
static int rows_copy(soc_ctx *c, float *dst, const float *src, int64_t n, hipMemcpyKind kind)
{
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)n * c->a2e_res_nfreq * 4, kind, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (the host buffer may be a temporary)
    return SOC_OK;
}
static int rows_up(soc_ctx *c, float *buf, int64_t c0, int64_t n, const float *host) { return rows_copy(c, buf + (size_t)c0 * c->a2e_res_nfreq, host, n, hipMemcpyHostToDevice); }
static int rows_down(soc_ctx *c, const float *buf, int64_t c0, int64_t n, float *host) { return rows_copy(c, host, buf + (size_t)c0 * c->a2e_res_nfreq, n, hipMemcpyDeviceToHost); }

int soc_a2e_resident_begin(soc_ctx *c, int64_t cells, int NFREQ)
{
    return soc_a2e_resident_begin_pol(c, cells, NFREQ, 0);
}

int soc_a2e_resident_begin_pol(soc_ctx *c, int64_t cells, int NFREQ, int polarised)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (cells < 1 || NFREQ < 2 || cells > (int64_t)2147483647) return fail(c, SOC_ERR_ARG, "soc_a2e_resident_begin: cells=%lld NFREQ=%d", (long long)cells, NFREQ);
    if (c->mABS) return fail(c, SOC_ERR_STATE, "soc_a2e_resident_begin: the resident arrays are those of soc_mabu_begin (soc_mabu_end first)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t need = (size_t)cells * NFREQ * 8 + (polarised ? (size_t)cells * NFREQ * 4 + (size_t)cells * 8 : 0);
    const size_t held = (c->aAll ? (size_t)c->a2e_cells * c->a2e_res_nfreq * 8 : 0) + (c->aPSum.n + c->aAalg.n) * 4;
    if (need + ((size_t)1 << 30) > free_b + held)
        return fail(c, SOC_ERR_STATE, "soc_a2e_resident_begin: %lld cells x %d frequencies need %.1f GB of device memory, %.1f GB are free (use soc_a2e_solve in batches)",
                    (long long)cells, NFREQ, need * 1e-9, free_b * 1e-9);
    const hipError_t e = resident_alloc(c, cells, NFREQ, polarised != 0);
    if (e != hipSuccess) {                                  // all or nothing: half of the arrays would be gigabytes nobody can use
        resident_release(c);
        return fail(c, SOC_ERR_HIP, "soc_a2e_resident_begin: %s", hipGetErrorString(e));
    }
    c->a2e_cells = cells;  c->a2e_res_nfreq = NFREQ;
    return SOC_OK;
}

int soc_a2e_resident_upload(soc_ctx *c, int64_t c0, int64_t n, const float *AABS)
{
    if (!c || !AABS) return SOC_ERR_ARG;
    SOC_ROWS(c, "soc_a2e_resident_upload", c0, n, c->aAll ? c->a2e_cells : 0);      // (nothing open: no row can be addressed)
    return rows_up(c, c->aAll, c0, n, AABS);
}

int soc_a2e_resident_upload_aalg(soc_ctx *c, int64_t c0, int64_t n, const float *aalg, const float *lgaalg)
{
    if (!c || !aalg || !lgaalg) return SOC_ERR_ARG;
    if (!c->aAalg || !c->aPSum) return fail(c, SOC_ERR_STATE, "soc_a2e_resident_upload_aalg: polarised output was not asked for (soc_a2e_resident_begin_pol, soc_mabu_begin_pol)");
    SOC_ROWS(c, "soc_a2e_resident_upload_aalg", c0, n, c->a2e_cells);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> both((size_t)n * 2);
    for (int64_t i = 0; i < n; i++) { both[2 * i] = aalg[i];  both[2 * i + 1] = lgaalg[i]; }
    HIPCHK(c, hipMemcpyAsync(c->aAalg + (size_t)c0 * 2, both.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_a2e_set_size_aalg(soc_ctx *c, float asize, float asize_next, float lg_asize, float lg_step)
{
    if (!c) return SOC_ERR_ARG;
    if (c->a2e_NE == 0) return fail(c, SOC_ERR_STATE, "soc_a2e_set_size_aalg: call soc_a2e_set_size first");
    c->a2e_pol[0] = asize;  c->a2e_pol[1] = asize_next;  c->a2e_pol[2] = lg_asize;  c->a2e_pol[3] = lg_step;
    c->a2e_pol_set = true;
    return SOC_OK;
}

// cells per launch of the resident solve (the grid is one workgroup per four cells); with the populations read back, the cells whose
// populations the device holds at a time: 65536 x NE floats, 73 MB at the largest NE
#define A2E_RES_STEP  ((int64_t)1 << 20)
#define A2E_DUMP_STEP ((int64_t)1 << 16)

// DoSolve of the current size over the resident cells, in chunks, added to the sums.  X (host, [cells][NE]), or NULL: the clamped
// populations too, through a device plane of one chunk that is read back after the chunk's launch, before the next one writes it
static int resident_solve(soc_ctx *c, const char *who, float *X)
{
    if (!c->aAll) return fail(c, SOC_ERR_STATE, "%s: call soc_a2e_resident_begin first", who);
    if (c->a2e_NE == 0 || c->a2e_NFREQ != c->a2e_res_nfreq) return fail(c, SOC_ERR_STATE, "%s: soc_a2e_set_size with NFREQ = %d first", who, c->a2e_res_nfreq);
    HIPCHK(c, hipSetDevice(c->device));
    SocA2EArgs A = a2e_tables(c);
    A.accumulate = 1;
    const bool pol = c->aPSum && c->aAalg && c->a2e_pol_set;   // (a size without soc_a2e_set_size_aalg adds nothing to the polarised sum)
    if (pol) { A.p_size = c->a2e_pol[0];  A.p_next = c->a2e_pol[1];  A.p_lgsize = c->a2e_pol[2];  A.p_lgden = c->a2e_pol[3]; }
    const int64_t step = X ? A2E_DUMP_STEP : A2E_RES_STEP;
    if (X) {
        const size_t n = (size_t)std::min<int64_t>(step, c->a2e_cells) * A.NE;
        if (c->aXX.reserve(n, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, SOC_ERR_STATE, "%s: the populations of a chunk of %lld cells x %d levels need %zu bytes of device memory, which are not free",
                        who, (long long)std::min<int64_t>(step, c->a2e_cells), A.NE, n * sizeof(float));
        }
        A.XX = c->aXX;
    }
    for (int64_t c0 = 0; c0 < c->a2e_cells; c0 += step) {
        A.batch = (int)std::min<int64_t>(step, c->a2e_cells - c0);
        A.AABS = c->aAll + (size_t)c0 * A.NFREQ;  A.AEMIT = c->aSum + (size_t)c0 * A.NFREQ;
        if (pol) { A.PEMIT = c->aPSum + (size_t)c0 * A.NFREQ;  A.AALG = c->aAalg + (size_t)c0 * 2; }
        HIPCHK(c, soc_launch_a2e_dosolve(A, c->stream));
        if (X) {
            HIPCHK(c, hipMemcpyAsync(X + (size_t)c0 * A.NE, c->aXX, (size_t)A.batch * A.NE * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    return SOC_OK;
}

int soc_a2e_resident_solve(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    return resident_solve(c, "soc_a2e_resident_solve", nullptr);
}

int soc_a2e_resident_solve_dump(soc_ctx *c, float *X)
{
    if (!c || !X) return SOC_ERR_ARG;
    return resident_solve(c, "soc_a2e_resident_solve_dump", X);
}

int soc_a2e_set_eq_sizes(soc_ctx *c, int nsizes, int NFREQ, int NIP, float FACTOR, const float *FREQ, const float *AF, const float *KABS,
                         const float *TTT, const float *Emin, const float *kE, const float *oplgkE, float GD, const float *S_FRAC,
                         const float *SIZE_A)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (nsizes < 1 || nsizes > 4096 || NFREQ < 2 || NIP < 2 || !FREQ || !AF || !KABS || !TTT || !Emin || !kE || !oplgkE || !S_FRAC)
        return fail(c, SOC_ERR_ARG, "soc_a2e_set_eq_sizes: bad arguments (1 <= nsizes <= 4096, NFREQ >= 2, NIP >= 2)");
    int shape[2];
    if (!soc_a2e_eq_shape(NFREQ, nsizes, shape))            // (refused here, with the sizes set before untouched, not at the launch)
        return fail(c, SOC_ERR_ARG, "soc_a2e_set_eq_sizes: NFREQ = %d with %d sizes needs %d bytes of LDS for one cell, the limit is %d",
                    NFREQ, nsizes, shape[1], SOC_A2E_LDS);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (a launch may still read the tables set before)
    const size_t nf = (size_t)nsizes * NFREQ, nt = (size_t)nsizes * NIP;
    HIPCHK(c, c->aEqTab.reserve((size_t)NFREQ + 2 * nf + nt, c->stream));
    HIPCHK(c, c->aEqPar.reserve((size_t)6 * nsizes, c->stream));
    std::vector<float> par((size_t)6 * nsizes, 0.0f);
    for (int s = 0; s < nsizes; s++) {
        par[s] = Emin[s];  par[nsizes + s] = kE[s];  par[2 * nsizes + s] = oplgkE[s];
        par[3 * nsizes + s] = GD * S_FRAC[s];               // one fp32 product, as numpy forms GD * S_FRAC[isize]
        par[4 * nsizes + s] = S_FRAC[s];
        if (SIZE_A) par[5 * nsizes + s] = SIZE_A[s];
    }
    float *dF = c->aEqTab, *dAF = dF + NFREQ, *dK = dAF + nf, *dT3 = dK + nf;
    HIPCHK(c, hipMemcpy(dF, FREQ, (size_t)NFREQ * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dAF, AF, nf * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dK, KABS, nf * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dT3, TTT, nt * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->aEqPar, par.data(), par.size() * 4, hipMemcpyHostToDevice));
    c->eq_nsizes = nsizes;  c->eq_NFREQ = NFREQ;  c->eq_NIP = NIP;  c->eq_FACTOR = FACTOR;  c->eq_GD = GD;  c->eq_pol = SIZE_A != nullptr;
    return SOC_OK;
}

int soc_a2e_resident_solve_eq(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    if (!c->aAll || !c->aSum) return fail(c, SOC_ERR_STATE, "soc_a2e_resident_solve_eq: call soc_a2e_resident_begin first");
    if (c->eq_nsizes == 0 || c->eq_NFREQ != c->a2e_res_nfreq)
        return fail(c, SOC_ERR_STATE, "soc_a2e_resident_solve_eq: soc_a2e_set_eq_sizes with NFREQ = %d first", c->a2e_res_nfreq);
    if (c->eq_pol && (!c->aPSum || !c->aAalg))
        return fail(c, SOC_ERR_STATE, "soc_a2e_resident_solve_eq: the sizes were set with SIZE_A, but polarised output was not asked for (soc_a2e_resident_begin_pol, soc_mabu_begin_pol)");
    HIPCHK(c, hipSetDevice(c->device));
    const int ns = c->eq_nsizes;
    const size_t nf = (size_t)ns * c->eq_NFREQ;
    SocEqSizesArgs A{};
    A.cells = c->a2e_cells;  A.NFREQ = c->eq_NFREQ;  A.NIP = c->eq_NIP;  A.nsizes = ns;  A.FACTOR = c->eq_FACTOR;  A.GD = c->eq_GD;
    A.FREQ = c->aEqTab;  A.AF = A.FREQ + c->eq_NFREQ;  A.KABS = A.AF + nf;  A.TTT = A.KABS + nf;
    const float *par = c->aEqPar;
    A.Emin = par;  A.kE = par + ns;  A.oplgkE = par + 2 * ns;  A.scale = par + 3 * ns;  A.SFRAC = par + 4 * ns;  A.SIZEA = par + 5 * ns;
    A.ABS = c->aAll;  A.SUM = c->aSum;
    if (c->eq_pol) { A.PSUM = c->aPSum;  A.AALG = c->aAalg; }
    c->teq_nsizes = 0;                                      // (what an earlier solve kept is not of these sizes)
    if (c->teq_keep) {
        if (c->aTeq.reserve((size_t)ns * (size_t)c->a2e_cells, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, SOC_ERR_STATE, "soc_a2e_resident_solve_eq: the temperatures of %d sizes x %lld cells need %zu bytes of device memory, which are not free "
                                          "(soc_a2e_resident_keep_teq is on; fewer cells at a time)", ns, (long long)c->a2e_cells, (size_t)ns * (size_t)c->a2e_cells * sizeof(float));
        }
        A.TOUT = c->aTeq;
    }
    HIPCHK(c, soc_launch_a2e_eqsizes(A, c->stream));
    if (c->teq_keep) c->teq_nsizes = ns;
    return SOC_OK;
}

int soc_a2e_resident_keep_teq(soc_ctx *c, int on)
{
    if (!c) return SOC_ERR_ARG;
    if (!c->aAll || !c->aSum) return fail(c, SOC_ERR_STATE, "soc_a2e_resident_keep_teq: call soc_a2e_resident_begin or soc_mabu_begin first");
    c->teq_keep = on != 0;
    return SOC_OK;
}

int soc_a2e_resident_download_teq(soc_ctx *c, int slot, int64_t c0, int64_t n, float *T)
{
    if (!c || !T) return SOC_ERR_ARG;
    if (!c->aAll || !c->aTeq || c->teq_nsizes < 1)
        return fail(c, SOC_ERR_STATE, "soc_a2e_resident_download_teq: no temperatures are kept (soc_a2e_resident_keep_teq, then soc_a2e_resident_solve_eq)");
    if (slot < 0 || slot >= c->teq_nsizes) return fail(c, SOC_ERR_ARG, "soc_a2e_resident_download_teq: size %d of %d", slot, c->teq_nsizes);
    SOC_ROWS(c, "soc_a2e_resident_download_teq", c0, n, c->a2e_cells);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(T, c->aTeq + (size_t)slot * (size_t)c->a2e_cells + (size_t)c0, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_a2e_resident_download(soc_ctx *c, int64_t c0, int64_t n, float *AEMIT)
{
    if (!c || !AEMIT) return SOC_ERR_ARG;
    SOC_ROWS(c, "soc_a2e_resident_download", c0, n, c->aSum ? c->a2e_cells : 0);
    return rows_down(c, c->aSum, c0, n, AEMIT);
}

int soc_a2e_resident_download_p(soc_ctx *c, int64_t c0, int64_t n, float *PEMIT)
{
    if (!c || !PEMIT) return SOC_ERR_ARG;
    if (!c->aPSum) return fail(c, SOC_ERR_STATE, "soc_a2e_resident_download_p: polarised output was not asked for (soc_a2e_resident_begin_pol, soc_mabu_begin_pol)");
    SOC_ROWS(c, "soc_a2e_resident_download_p", c0, n, c->a2e_cells);
    return rows_down(c, c->aPSum, c0, n, PEMIT);
}

int soc_a2e_resident_end(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    if (c->mABS) return fail(c, SOC_ERR_STATE, "soc_a2e_resident_end: the resident arrays are those of soc_mabu_begin (soc_mabu_end frees them)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resident_release(c);
    return SOC_OK;
}

int soc_a2e_solve(soc_ctx *c, int batch, const float *AABS, float *AEMIT)
{
    int r = soc_a2e_upload(c, batch, AABS);
    if (r) return r;
    r = soc_a2e_run(c, batch);
    if (r) return r;
    return soc_a2e_download(c, batch, AEMIT);
}

int soc_a2e_solve_dump(soc_ctx *c, int batch, const float *AABS, float *AEMIT, float *X)
{
    if (!c || !AEMIT || !X) return SOC_ERR_ARG;
    int r = soc_a2e_upload(c, batch, AABS);
    if (r) return r;
    FLUSH(c);
    const size_t n = (size_t)batch * c->a2e_NE;
    if (c->aXX.reserve(n, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, SOC_ERR_STATE, "soc_a2e_solve_dump: the populations of %d cells x %d levels need %zu bytes of device memory, which are not free",
                    batch, c->a2e_NE, n * sizeof(float));
    }
    SocA2EArgs A = a2e_tables(c);
    A.batch = batch;  A.AABS = c->aABS;  A.AEMIT = c->aEMIT;  A.XX = c->aXX;
    HIPCHK(c, soc_launch_a2e_dosolve(A, c->stream));
    HIPCHK(c, hipMemcpyAsync(X, c->aXX, n * 4, hipMemcpyDeviceToHost, c->stream));
    return soc_a2e_download(c, batch, AEMIT);               // (waits for the stream: X has landed as well)
}

static int eqtemp_common(soc_ctx *c, const char *who, bool eqsolver, int batch, int icell, int CELLS, int NFREQ, int NIP, float FACTOR, float kE,
                   float oplgkE, float Emin, const float *FREQ, const float *KABS, const float *TTT,
                   const float *ABS, float *T, float *EMIT)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (batch < 1 || NFREQ < 2 || NIP < 2 || !FREQ || !KABS || !TTT || !ABS || !T || !EMIT)
        return fail(c, SOC_ERR_ARG, "%s: bad arguments", who);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> d;
    const size_t n = (size_t)2 * NFREQ + NIP + (size_t)2 * batch * NFREQ + batch;
    HIPCHK(c, d.reset(n, c->stream));
    float *dF = d, *dK = dF + NFREQ, *dT3 = dK + NFREQ, *dA = dT3 + NIP, *dE = dA + (size_t)batch * NFREQ, *dT = dE + (size_t)batch * NFREQ;
    HIPCHK(c, hipMemcpy(dF, FREQ, (size_t)NFREQ * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dK, KABS, (size_t)NFREQ * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dT3, TTT, (size_t)NIP * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dA, ABS, (size_t)batch * NFREQ * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(dE, 0, ((size_t)batch * NFREQ + batch) * 4, c->stream));
    SocEqTArgs A{};
    A.batch = batch;  A.icell = icell;  A.CELLS = CELLS;  A.NFREQ = NFREQ;  A.NIP = NIP;
    A.FACTOR = FACTOR;  A.kE = kE;  A.oplgkE = oplgkE;  A.Emin = Emin;
    A.FREQ = dF;  A.KABS = dK;  A.TTT = dT3;  A.ABS = dA;  A.T = dT;  A.EMIT = dE;
    HIPCHK(c, eqsolver ? soc_launch_eqsolver(A, c->stream) : soc_launch_a2e_eqtemp(A, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(T, dT, (size_t)batch * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(EMIT, dE, (size_t)batch * NFREQ * 4, hipMemcpyDeviceToHost));
    return SOC_OK;
}

int soc_a2e_eqtemp(soc_ctx *c, int batch, int icell, int CELLS, int NFREQ, int NIP, float FACTOR, float kE,
                   float oplgkE, float Emin, const float *FREQ, const float *KABS, const float *TTT,
                   const float *ABS, float *T, float *EMIT)
{
    return eqtemp_common(c, "soc_a2e_eqtemp", false, batch, icell, CELLS, NFREQ, NIP, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, ABS, T, EMIT);
}

int soc_eqsolver(soc_ctx *c, int batch, int icell, int CELLS, int NFREQ, int NE, float FACTOR, float kE,
                 float oplgkE, float Emin, const float *FREQ, const float *KABS, const float *TTT,
                 const float *ABS, float *T, float *EMIT)
{
    return eqtemp_common(c, "soc_eqsolver", true, batch, icell, CELLS, NFREQ, NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, ABS, T, EMIT);
}

// ---- the multi-dust stage with the cells resident in HBM (A2E_MABU.py:700-1140) ----
static void mabu_release(soc_ctx *c)
{
    c->mABS.release();  c->mSUM.release();  c->mABU.release();  c->mT.release();  c->mTab.release();  c->mRABS.release();
    c->mPSUM.release();  c->mPol.release();
    resident_release(c);
    c->mabu_ndust = 0;  c->mabu_tables = false;  c->mabu_t_set = false;
}

int soc_mabu_begin(soc_ctx *c, int64_t cells, int NFREQ, int NDUST, int64_t *cells_fit)
{
    return soc_mabu_begin_pol(c, cells, NFREQ, NDUST, 0, cells_fit);
}

int soc_mabu_begin_pol(soc_ctx *c, int64_t cells, int NFREQ, int NDUST, int polarised, int64_t *cells_fit)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (cells_fit) *cells_fit = 0;
    if (cells < 1 || NFREQ < 2 || NDUST < 1 || cells > (int64_t)2147483647 || (size_t)NFREQ * NDUST * sizeof(double) > SOC_MABU_LDS)
        return fail(c, SOC_ERR_ARG, "soc_mabu_begin: cells=%lld NFREQ=%d NDUST=%d (NFREQ x NDUST doubles must fit %d KB of LDS)",
                    (long long)cells, NFREQ, NDUST, SOC_MABU_LDS / 1024);
    if (c->aAll && !c->mABS) return fail(c, SOC_ERR_STATE, "soc_mabu_begin: the resident arrays are those of an open soc_a2e_resident_begin (soc_a2e_resident_end first)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    mabu_release(c);                                        // (a soc_mabu_begin that is still open is replaced)
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    // per cell: absorptions, the dust's share, its emission, the sum (NFREQ floats each), NDUST abundances, a temperature
    // with polarised output also the dust's polarised emission and its sum (NFREQ floats each), a_alg and its logarithm
    const size_t per_cell = (size_t)NFREQ * 16 + (size_t)NDUST * 4 + 4 + (polarised ? (size_t)NFREQ * 8 + 8 : 0), reserve = (size_t)1 << 30;
    const size_t need = (size_t)cells * per_cell;
    if (cells_fit) *cells_fit = free_b > reserve ? (int64_t)((free_b - reserve) / per_cell) : 0;
    if (need + reserve > free_b)
        return fail(c, SOC_ERR_STATE, "soc_mabu_begin: %lld cells x %d frequencies x %d dusts need %.1f GB of device memory, %.1f GB are free (%lld cells fit: solve the cells in ranges)",
                    (long long)cells, NFREQ, NDUST, need * 1e-9, free_b * 1e-9, (long long)(free_b > reserve ? (free_b - reserve) / per_cell : 0));
    const size_t n = (size_t)cells * NFREQ;
    hipError_t e = c->mABS.reset(n, c->stream);
    if (e == hipSuccess) e = resident_alloc(c, cells, NFREQ, polarised != 0);
    if (e == hipSuccess) e = c->mSUM.reset(n, c->stream);
    if (e == hipSuccess) e = c->mABU.reset((size_t)cells * NDUST, c->stream);
    if (e == hipSuccess) e = c->mT.reset((size_t)cells, c->stream);
    if (e == hipSuccess) e = c->mRABS.reset((size_t)NFREQ * NDUST, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->mSUM, 0, n * 4, c->stream);
    if (e == hipSuccess && polarised) e = c->mPSUM.reset(n, c->stream);
    if (e == hipSuccess && polarised) e = hipMemsetAsync(c->mPSUM, 0, n * 4, c->stream);
    if (e != hipSuccess) {
        mabu_release(c);
        return fail(c, SOC_ERR_HIP, "soc_mabu_begin: %s", hipGetErrorString(e));
    }
    c->a2e_cells = cells;  c->a2e_res_nfreq = NFREQ;  c->mabu_ndust = NDUST;
    return SOC_OK;
}

#define MABU_OPEN(c, who)                                                                                   \
    do {                                                                                                    \
        if (!(c)->mABS || !(c)->aAll || !(c)->aSum) return fail((c), SOC_ERR_STATE, who ": call soc_mabu_begin first");   \
    } while (0)

int soc_mabu_upload(soc_ctx *c, int64_t c0, int64_t n, const float *ABS)
{
    if (!c || !ABS) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_upload");
    SOC_ROWS(c, "soc_mabu_upload", c0, n, c->a2e_cells);
    return rows_up(c, c->mABS, c0, n, ABS);
}

int soc_mabu_set_tables(soc_ctx *c, const float *ABU, const double *RABS)
{
    if (!c || !ABU || !RABS) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_set_tables");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->mABU, ABU, (size_t)c->a2e_cells * c->mabu_ndust * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->mRABS, RABS, (size_t)c->a2e_res_nfreq * c->mabu_ndust * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mabu_tables = true;
    return SOC_OK;
}

int soc_mabu_split(soc_ctx *c, int idust, int clip_last)
{
    if (!c) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_split");
    if (!c->mabu_tables) return fail(c, SOC_ERR_STATE, "soc_mabu_split: call soc_mabu_set_tables first");
    if (idust < 0 || idust >= c->mabu_ndust) return fail(c, SOC_ERR_ARG, "soc_mabu_split: dust %d of %d", idust, c->mabu_ndust);
    HIPCHK(c, hipSetDevice(c->device));
    const int NFREQ = c->a2e_res_nfreq;
    HIPCHK(c, soc_launch_mabu_split(c->a2e_cells, NFREQ, c->mabu_ndust, idust, c->mABS, c->mABU, c->mRABS, c->aAll, c->stream));
    if (clip_last) HIPCHK(c, soc_launch_mabu_clip(c->a2e_cells, NFREQ, c->aAll, c->stream));
    HIPCHK(c, hipMemsetAsync(c->aSum, 0, (size_t)c->a2e_cells * NFREQ * 4, c->stream));
    if (c->aPSum) HIPCHK(c, hipMemsetAsync(c->aPSum, 0, (size_t)c->a2e_cells * NFREQ * 4, c->stream));
    c->a2e_pol_set = false;
    return SOC_OK;
}

int soc_mabu_solve_eq(soc_ctx *c, int NE, float FACTOR, float kE, float oplgkE, float Emin, const float *FREQ, const float *KABS, const float *TTT)
{
    if (!c) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_solve_eq");
    if (NE < 2 || !FREQ || !KABS || !TTT) return fail(c, SOC_ERR_ARG, "soc_mabu_solve_eq: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const int NFREQ = c->a2e_res_nfreq;
    HIPCHK(c, c->mTab.reserve((size_t)2 * NFREQ + NE, c->stream));
    float *dF = c->mTab, *dK = dF + NFREQ, *dT3 = dK + NFREQ;
    HIPCHK(c, hipMemcpyAsync(dF, FREQ, (size_t)NFREQ * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dK, KABS, (size_t)NFREQ * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dT3, TTT, (size_t)NE * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (the host tables may be temporaries)
    SocEqTArgs A{};
    A.batch = (int)c->a2e_cells;  A.icell = 0;  A.CELLS = (int)c->a2e_cells;  A.NFREQ = NFREQ;  A.NIP = NE;
    A.FACTOR = FACTOR;  A.kE = kE;  A.oplgkE = oplgkE;  A.Emin = Emin;
    A.FREQ = dF;  A.KABS = dK;  A.TTT = dT3;  A.ABS = c->aAll;  A.T = c->mT;  A.EMIT = c->aSum;
    HIPCHK(c, soc_launch_eqsolver(A, c->stream));
    c->mabu_t_set = true;
    return SOC_OK;
}

int soc_mabu_download_t(soc_ctx *c, int64_t c0, int64_t n, float *T)
{
    if (!c || !T) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_download_t");
    if (!c->mT || !c->mabu_t_set) return fail(c, SOC_ERR_STATE, "soc_mabu_download_t: no soc_mabu_solve_eq since soc_mabu_begin");
    SOC_ROWS(c, "soc_mabu_download_t", c0, n, c->a2e_cells);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(T, c->mT + (size_t)c0, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_mabu_accumulate(soc_ctx *c, int idust)
{
    if (!c) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_accumulate");
    if (!c->mabu_tables) return fail(c, SOC_ERR_STATE, "soc_mabu_accumulate: call soc_mabu_set_tables first");
    if (idust < 0 || idust >= c->mabu_ndust) return fail(c, SOC_ERR_ARG, "soc_mabu_accumulate: dust %d of %d", idust, c->mabu_ndust);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, soc_launch_mabu_sum(c->a2e_cells, c->a2e_res_nfreq, c->mabu_ndust, idust, c->aSum, c->mABU, c->mSUM, c->stream));
    return SOC_OK;
}

#define MABU_POL(c, who)                                                                                    \
    do {                                                                                                    \
        if (!(c)->mPSUM || !(c)->aPSum || !(c)->aAalg) return fail((c), SOC_ERR_STATE, who ": polarised output was not asked for (soc_mabu_begin_pol)");   \
    } while (0)

int soc_mabu_pol_eq(soc_ctx *c, int NA, const double *APOL, const double *TAB)
{
    if (!c || !APOL || !TAB) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_pol_eq");
    MABU_POL(c, "soc_mabu_pol_eq");
    if (NA < 2) return fail(c, SOC_ERR_ARG, "soc_mabu_pol_eq: %d sizes (at least 2)", NA);
    for (int i = 1; i < NA; i++)
        if (!(APOL[i] >= APOL[i - 1])) return fail(c, SOC_ERR_ARG, "soc_mabu_pol_eq: the sizes must not decrease (entry %d)", i);
    HIPCHK(c, hipSetDevice(c->device));
    const int NFREQ = c->a2e_res_nfreq;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->mPol.reserve((size_t)NA * (NFREQ + 1), c->stream));
    double *dA = c->mPol, *dT = dA + NA;
    HIPCHK(c, hipMemcpyAsync(dA, APOL, (size_t)NA * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dT, TAB, (size_t)NA * NFREQ * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (the host tables may be temporaries)
    HIPCHK(c, soc_launch_mabu_poleq(c->a2e_cells, NFREQ, NA, c->aSum, c->aAalg, dA, dT, c->aPSum, c->stream));
    return SOC_OK;
}

int soc_mabu_accumulate_p(soc_ctx *c, int idust)
{
    if (!c) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_accumulate_p");
    MABU_POL(c, "soc_mabu_accumulate_p");
    if (!c->mabu_tables) return fail(c, SOC_ERR_STATE, "soc_mabu_accumulate_p: call soc_mabu_set_tables first");
    if (idust < 0 || idust >= c->mabu_ndust) return fail(c, SOC_ERR_ARG, "soc_mabu_accumulate_p: dust %d of %d", idust, c->mabu_ndust);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, soc_launch_mabu_sum(c->a2e_cells, c->a2e_res_nfreq, c->mabu_ndust, idust, c->aPSum, c->mABU, c->mPSUM, c->stream));
    return SOC_OK;
}

int soc_mabu_ratio(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_ratio");
    MABU_POL(c, "soc_mabu_ratio");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, soc_launch_mabu_ratio(c->a2e_cells, c->a2e_res_nfreq, c->mSUM, c->mPSUM, c->stream));
    return SOC_OK;
}

int soc_mabu_download(soc_ctx *c, int64_t c0, int64_t n, float *SUM)
{
    if (!c || !SUM) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_download");
    SOC_ROWS(c, "soc_mabu_download", c0, n, c->a2e_cells);
    return rows_down(c, c->mSUM, c0, n, SUM);
}

int soc_mabu_download_p(soc_ctx *c, int64_t c0, int64_t n, float *PSUM)
{
    if (!c || !PSUM) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_download_p");
    MABU_POL(c, "soc_mabu_download_p");
    SOC_ROWS(c, "soc_mabu_download_p", c0, n, c->a2e_cells);
    return rows_down(c, c->mPSUM, c0, n, PSUM);
}

int soc_mabu_read_part(soc_ctx *c, int64_t c0, int64_t n, float *PART)
{
    if (!c || !PART) return SOC_ERR_ARG;
    MABU_OPEN(c, "soc_mabu_read_part");
    SOC_ROWS(c, "soc_mabu_read_part", c0, n, c->a2e_cells);
    return rows_down(c, c->aAll, c0, n, PART);
}

int soc_mabu_end(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->mABS) mabu_release(c);
    return SOC_OK;
}

int soc_a2e_pre(soc_ctx *c, int NFREQ, int NE, float FACTOR, const float *FREQ, const float *Ef, const float *SKABS, const float *E,
                const float *T, int32_t *L1, int32_t *L2, float *Iw, int32_t *noIw, float *Tdown)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (NFREQ < 2 || NE < 2 || NE > 4096 || !FREQ || !Ef || !SKABS || !E || !T || !L1 || !L2 || !Iw || !noIw || !Tdown)
        return fail(c, SOC_ERR_ARG, "soc_a2e_pre: NFREQ %d, NE %d or a NULL array", NFREQ, NE);
    if (NFREQ > SOC_A2E_PRE_NFREQ_MAX)                      // before anything is allocated or copied
        return fail(c, SOC_ERR_ARG, "soc_a2e_pre: NFREQ = %d, the limit is %d: the weights kernel keeps 64 columns of NFREQ floats in the "
                                    "160 KB of LDS of a workgroup", NFREQ, SOC_A2E_PRE_NFREQ_MAX);
    for (int i = 1; i < NFREQ; i++)
        if (!(FREQ[i] > FREQ[i - 1]) || !(Ef[i] > Ef[i - 1])) return fail(c, SOC_ERR_ARG, "soc_a2e_pre: FREQ, Ef must increase (entry %d)", i);
    for (int i = 1; i <= NE; i++)
        if (!(E[i] > E[i - 1])) return fail(c, SOC_ERR_ARG, "soc_a2e_pre: the enthalpy grid E[NE+1] must increase (entry %d)", i);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nIw = (size_t)NE * NE * NFREQ, nW = (size_t)NE * NFREQ;
    DevBuf<float> d, dIw;
    DevBuf<int>   dL;
    // one block of floats: FREQ | Ef | SKABS (NFREQ each) | E | T (NE+1 each) | Tdown (NE) | wrk (NE*NFREQ)
    const size_t nf = 3 * (size_t)NFREQ + 2 * (size_t)(NE + 1) + NE + nW;
    HIPCHK(c, d.reset(nf, c->stream));
    HIPCHK(c, dIw.reset(nIw, c->stream));
    HIPCHK(c, dL.reset(2 * (size_t)NE * NE + NE, c->stream));
    float *dF = d, *dEf = dF + NFREQ, *dSK = dEf + NFREQ, *dE = dSK + NFREQ, *dT = dE + NE + 1, *dTd = dT + NE + 1, *dW = dTd + NE;
    int *dL1 = dL, *dL2 = dL1 + (size_t)NE * NE, *dN = dL2 + (size_t)NE * NE;
    HIPCHK(c, hipMemcpyAsync(dF, FREQ, (size_t)NFREQ * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dEf, Ef, (size_t)NFREQ * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dSK, SKABS, (size_t)NFREQ * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dE, E, (size_t)(NE + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dT, T, (size_t)(NE + 1) * 4, hipMemcpyHostToDevice, c->stream));
    // entries the kernels do not write (pairs with u <= l, the unused tail of Iw) are 0 here; the reference leaves them to chance
    HIPCHK(c, hipMemsetAsync(dL, 0, (2 * (size_t)NE * NE + NE) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(dIw, 0, nIw * 4, c->stream));
    HIPCHK(c, soc_launch_a2e_pre(NFREQ, NE, FACTOR, dF, dEf, dSK, dE, dT, dL1, dL2, dIw, dW, dN, dTd, c->stream));
    HIPCHK(c, hipMemcpyAsync(L1, dL1, (size_t)NE * NE * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(L2, dL2, (size_t)NE * NE * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(noIw, dN, (size_t)(NE - 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(Iw, dIw, nIw * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(Tdown, dTd, (size_t)NE * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
