// soc_capi_reemit.hip -- host side of libsoc_hip.so: the emission of one re-emission iteration, resident and transposed for the
// cell-emission launches of the next, and its change from one iteration to the next (soc_emitted_*, soc_set_emission_column,
// soc_read_emission; kernels: soc_reemit.hip).
#include "soc_host.h"

#include <algorithm>

#define EMITTED_STAGE ((int64_t)1 << 18)                    // cells per staged piece of an upload or a download

#define EMITTED_OPEN(c, who)                                                                                \
    do {                                                                                                    \
        if (!(c)->eET || (c)->et_nfreq < 1) return fail((c), SOC_ERR_STATE, who ": call soc_emitted_begin first");   \
    } while (0)
#define EMITTED_ROWS(c, who, c0, n) SOC_ROWS(c, who, c0, n, (c)->G.CELLS)

#pragma GCC visibility push(default)
extern "C" {

int soc_emitted_begin(soc_ctx *c, int NFREQ)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_emitted_begin: call soc_set_grid first");
    if (NFREQ < 1) return fail(c, SOC_ERR_ARG, "soc_emitted_begin: NFREQ = %d", NFREQ);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t n = (size_t)c->G.CELLS * (size_t)NFREQ, reserve = (size_t)1 << 30;
    const size_t held = (c->eET ? c->eET.bytes() : 0) + (c->eRows ? c->eRows.bytes() : 0) + (c->eLp ? c->eLp.bytes() : 0)
                        + (c->eChange ? c->eChange.bytes() : 0);                                  // (an open one is replaced: its memory counts as free)
    if (n * 4 + reserve > free_b + held)                        // refused before anything changes: an open one stays as it is
        return fail(c, SOC_ERR_STATE, "soc_emitted_begin: %d cells x %d frequencies need %.1f GB of device memory, %.1f GB are free "
                                      "(the emission of an iteration goes through the host instead)", c->G.CELLS, NFREQ, n * 4e-9, free_b * 1e-9);
    c->eRows.release();  c->release_change();  c->et_nfreq = 0;
    hipError_t e = c->eET.reset(n, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->eET, 0, n * 4, c->stream);
    if (e != hipSuccess) {
        c->eET.release();
        return fail(c, SOC_ERR_HIP, "soc_emitted_begin: %s", hipGetErrorString(e));
    }
    c->et_nfreq = NFREQ;
    return SOC_OK;
}

int soc_emitted_upload(soc_ctx *c, int64_t c0, int64_t n, const float *rows)
{
    if (!c || !rows) return SOC_ERR_ARG;
    EMITTED_OPEN(c, "soc_emitted_upload");
    EMITTED_ROWS(c, "soc_emitted_upload", c0, n);
    HIPCHK(c, hipSetDevice(c->device));
    const int NFREQ = c->et_nfreq;
    HIPCHK(c, c->eRows.reserve((size_t)std::min(n, EMITTED_STAGE) * NFREQ, c->stream));
    for (int64_t a = 0; a < n; a += EMITTED_STAGE) {
        const int64_t m = std::min(EMITTED_STAGE, n - a);
        HIPCHK(c, hipMemcpyAsync(c->eRows, rows + (size_t)a * NFREQ, (size_t)m * NFREQ * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, soc_launch_reemit_to_columns(m, NFREQ, c->G.CELLS, c0 + a, c->eRows, c->eET, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));         // (the host buffer may be a temporary; the stage is used again)
    }
    return SOC_OK;
}

int soc_emitted_from_mabu(soc_ctx *c, int64_t c0)
{
    if (!c) return SOC_ERR_ARG;
    EMITTED_OPEN(c, "soc_emitted_from_mabu");
    if (!c->mSUM || c->a2e_cells < 1) return fail(c, SOC_ERR_STATE, "soc_emitted_from_mabu: no soc_mabu_begin is open");
    if (c->a2e_res_nfreq != c->et_nfreq)
        return fail(c, SOC_ERR_ARG, "soc_emitted_from_mabu: the open soc_mabu_begin has %d frequencies, soc_emitted_begin %d", c->a2e_res_nfreq, c->et_nfreq);
    EMITTED_ROWS(c, "soc_emitted_from_mabu", c0, c->a2e_cells);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, soc_launch_reemit_to_columns(c->a2e_cells, c->et_nfreq, c->G.CELLS, c0, c->mSUM, c->eET, c->stream));
    return SOC_OK;
}

int soc_emitted_download(soc_ctx *c, int64_t c0, int64_t n, float *rows)
{
    if (!c || !rows) return SOC_ERR_ARG;
    EMITTED_OPEN(c, "soc_emitted_download");
    EMITTED_ROWS(c, "soc_emitted_download", c0, n);
    HIPCHK(c, hipSetDevice(c->device));
    const int NFREQ = c->et_nfreq;
    HIPCHK(c, c->eRows.reserve((size_t)std::min(n, EMITTED_STAGE) * NFREQ, c->stream));
    for (int64_t a = 0; a < n; a += EMITTED_STAGE) {
        const int64_t m = std::min(EMITTED_STAGE, n - a);
        HIPCHK(c, soc_launch_reemit_to_rows(m, NFREQ, c->G.CELLS, c0 + a, c->eET, c->eRows, c->stream));
        HIPCHK(c, hipMemcpyAsync(rows + (size_t)a * NFREQ, c->eRows, (size_t)m * NFREQ * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return SOC_OK;
}

int soc_set_emission_column(soc_ctx *c, int ifreq, const float *COEFF)
{
    if (!c) return SOC_ERR_ARG;
    // no flush: a deferred SimRAM_CL launch keeps its own copy of EMIT and EMWEI (soc_sim_cl), as with soc_set_emission
    EMITTED_OPEN(c, "soc_set_emission_column");
    if (!COEFF) return fail(c, SOC_ERR_ARG, "soc_set_emission_column: COEFF is NULL");
    if (ifreq < 0 || ifreq >= c->et_nfreq) return fail(c, SOC_ERR_ARG, "soc_set_emission_column: frequency %d of %d", ifreq, c->et_nfreq);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->G.CELLS;
    if (!c->have_emit) {
        HIPCHK(c, c->dEMIT.reset(n, c->stream));
        HIPCHK(c, c->dEMWEI.reset(n, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dEMWEI, 0, n * 4, c->stream));
        c->have_emit = true;
    }
    HIPCHK(c, soc_launch_reemit_column(c->G, COEFF, c->eET + (size_t)ifreq * n, c->dEMIT, c->stream));
    c->emit_gen++;
    return SOC_OK;
}

int soc_read_emission(soc_ctx *c, float *EMIT, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid || !c->have_emit) return fail(c, SOC_ERR_STATE, "soc_read_emission: no emission is set (soc_set_emission, soc_set_emission_column)");
    if (!EMIT || n < 0 || n > c->G.CELLS) return fail(c, SOC_ERR_ARG, "soc_read_emission: n=%lld", (long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(EMIT, c->dEMIT, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_emitted_change(soc_ctx *c, const double *W, const float *COEFF, double stats[4], int64_t *bad)
{
    if (!c) return SOC_ERR_ARG;
    EMITTED_OPEN(c, "soc_emitted_change");
    if (!W || !COEFF || !stats || !bad)
        return fail(c, SOC_ERR_ARG, "soc_emitted_change: %s is NULL", !W ? "W" : !COEFF ? "COEFF" : !stats ? "stats" : "bad");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)c->G.CELLS, nfreq = (size_t)c->et_nfreq;
    const size_t blocks = (size_t)soc_emitted_change_blocks(c->G.CELLS), scratch = nfreq + 4 + 4 * blocks;
    if (!c->eLp) {                                              // the first call since soc_emitted_begin: the plane, zeroed, and the scratch
        HIPCHK(c, hipStreamSynchronize(c->stream));
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        const size_t need = 8 * (cells + scratch + 1), reserve = (size_t)1 << 30;
        if (need + reserve > free_b)                            // refused before anything changes
            return fail(c, SOC_ERR_STATE, "soc_emitted_change: the luminosities of %d cells need %.3f GB of device memory, %.1f GB are free",
                        c->G.CELLS, need * 1e-9, free_b * 1e-9);
        hipError_t e = c->eLp.reset(cells, c->stream);
        if (e == hipSuccess) e = c->eChange.reset(scratch, c->stream);
        if (e == hipSuccess) e = c->eBad.reset(1, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->eLp, 0, cells * 8, c->stream);
        if (e != hipSuccess) {
            c->release_change();
            return fail(c, SOC_ERR_HIP, "soc_emitted_change: %s", hipGetErrorString(e));
        }
    }
    double *dW = c->eChange, *dStats = dW + nfreq, *dPart = dStats + 4;
    unsigned long long nbad = 0;
    HIPCHK(c, hipMemcpyAsync(dW, W, nfreq * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->eBad, 0, 8, c->stream));
    HIPCHK(c, soc_launch_emitted_change(c->G, c->et_nfreq, COEFF, c->eET, dW, c->eLp, dPart, dStats, c->eBad, c->stream));
    HIPCHK(c, hipMemcpyAsync(stats, dStats, 4 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&nbad, c->eBad, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *bad = (int64_t)nbad;
    return SOC_OK;
}

int soc_emitted_read_luminosity(soc_ctx *c, int64_t c0, int64_t n, double *L)
{
    if (!c || !L) return SOC_ERR_ARG;
    EMITTED_OPEN(c, "soc_emitted_read_luminosity");
    EMITTED_ROWS(c, "soc_emitted_read_luminosity", c0, n);
    if (!c->eLp) {                                              // no soc_emitted_change since soc_emitted_begin: all zero
        std::fill(L, L + n, 0.0);
        return SOC_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(L, c->eLp + c0, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_emitted_end(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->eET.release();  c->eRows.release();  c->release_change();  c->et_nfreq = 0;
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
