// soc_capi_absorbed.hip -- host side of libsoc_hip.so: the absorptions of the transfer stage, resident and transposed between the
// launches that tally them and the multi-dust stage that reads them (soc_absorbed_*; kernels: soc_reemit.hip).  The mirror image of
// soc_capi_reemit.hip: there rows become the per-frequency EMIT of a launch, here per-frequency tallies become rows.
#include "soc_host.h"

#include <algorithm>

#define ABSORBED_STAGE ((int64_t)1 << 18)                   // cells per staged piece of a download

#define ABSORBED_OPEN(c, who)                                                                               \
    do {                                                                                                    \
        if (!(c)->bAT || (c)->at_nfreq < 1) return fail((c), SOC_ERR_STATE, who ": call soc_absorbed_begin first");  \
    } while (0)
#define ABSORBED_ROWS(c, who, c0, n) SOC_ROWS(c, who, c0, n, (c)->G.CELLS)
#define ABSORBED_FREQ(c, who, ifreq)                                                                        \
    do {                                                                                                    \
        if ((ifreq) < 0 || (ifreq) >= (c)->at_nfreq)                                                        \
            return fail((c), SOC_ERR_ARG, who ": frequency %d of %d", (ifreq), (c)->at_nfreq);              \
    } while (0)

static void absorbed_release(soc_ctx *c)
{
    c->bAT.release();  c->bAC.release();  c->bRows.release();
    c->at_nfreq = 0;  c->ac_kept = false;
}

#pragma GCC visibility push(default)
extern "C" {

int soc_absorbed_begin(soc_ctx *c, int NFREQ, int keep_constant)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_absorbed_begin: call soc_set_grid first");
    if (NFREQ < 1) return fail(c, SOC_ERR_ARG, "soc_absorbed_begin: NFREQ = %d", NFREQ);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t n = (size_t)c->G.CELLS * (size_t)NFREQ, planes = keep_constant ? 2 : 1, reserve = (size_t)1 << 30;
    size_t held = 0;                                            // (an open one is replaced: its memory counts as free)
    for (const DevBuf<float> *b : { &c->bAT, &c->bAC, &c->bRows }) held += *b ? b->bytes() : 0;
    if (n * 4 * planes + reserve > free_b + held)               // refused before anything changes: an open one stays as it is
        return fail(c, SOC_ERR_STATE, "soc_absorbed_begin: %d cells x %d frequencies%s need %.1f GB of device memory, %.1f GB are free "
                                      "(the absorptions go through the host instead)", c->G.CELLS, NFREQ,
                    keep_constant ? ", twice," : "", n * planes * 4e-9, free_b * 1e-9);
    absorbed_release(c);
    hipError_t e = c->bAT.reset(n, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->bAT, 0, n * 4, c->stream);
    if (e == hipSuccess && keep_constant) e = c->bAC.reset(n, c->stream);
    if (e != hipSuccess) {
        absorbed_release(c);
        return fail(c, SOC_ERR_HIP, "soc_absorbed_begin: %s", hipGetErrorString(e));
    }
    c->at_nfreq = NFREQ;
    return SOC_OK;
}

int soc_absorbed_add_tally(soc_ctx *c, int ifreq)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    ABSORBED_OPEN(c, "soc_absorbed_add_tally");
    ABSORBED_FREQ(c, "soc_absorbed_add_tally", ifreq);
    if (!c->dINT) return fail(c, SOC_ERR_STATE, "soc_absorbed_add_tally: there is no INT tally");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, soc_launch_absorbed_add(c->G.CELLS, c->dINT, c->bAT + (size_t)ifreq * (size_t)c->G.CELLS, c->stream));
    return SOC_OK;
}

int soc_absorbed_add_slot(soc_ctx *c, int ifreq, int k)
{
    if (!c) return SOC_ERR_ARG;
    ABSORBED_OPEN(c, "soc_absorbed_add_slot");
    if (c->batching || !c->pending.empty()) return fail(c, SOC_ERR_STATE, "soc_absorbed_add_slot: call soc_batch_end first");
    ABSORBED_FREQ(c, "soc_absorbed_add_slot", ifreq);
    const DevBuf<char> *slot = (k >= 0 && k < c->int_slots_done) ? &c->slots[soc_ctx::SLOT_INT][k] : nullptr;
    if (!slot || !*slot || slot->n < (size_t)c->G.CELLS * 4)
        return fail(c, SOC_ERR_ARG, "soc_absorbed_add_slot: launch %d of %d deferred with the INT tally", k, c->int_slots_done);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, soc_launch_absorbed_add(c->G.CELLS, (const float *)slot->p, c->bAT + (size_t)ifreq * (size_t)c->G.CELLS, c->stream));
    return SOC_OK;
}

int soc_absorbed_keep(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    ABSORBED_OPEN(c, "soc_absorbed_keep");
    if (!c->bAC) return fail(c, SOC_ERR_STATE, "soc_absorbed_keep: soc_absorbed_begin reserved no second plane (keep_constant = 0)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->bAC, c->bAT, (size_t)c->G.CELLS * c->at_nfreq * 4, hipMemcpyDeviceToDevice, c->stream));
    c->ac_kept = true;
    return SOC_OK;
}

int soc_absorbed_restore(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    ABSORBED_OPEN(c, "soc_absorbed_restore");
    if (!c->bAC) return fail(c, SOC_ERR_STATE, "soc_absorbed_restore: soc_absorbed_begin reserved no second plane (keep_constant = 0)");
    if (!c->ac_kept) return fail(c, SOC_ERR_STATE, "soc_absorbed_restore: call soc_absorbed_keep first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->bAT, c->bAC, (size_t)c->G.CELLS * c->at_nfreq * 4, hipMemcpyDeviceToDevice, c->stream));
    return SOC_OK;
}

int soc_absorbed_to_mabu(soc_ctx *c, int64_t c0, const float *K, float nnnlimit)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    ABSORBED_OPEN(c, "soc_absorbed_to_mabu");
    if (!c->mABS || c->a2e_cells < 1) return fail(c, SOC_ERR_STATE, "soc_absorbed_to_mabu: no soc_mabu_begin is open");
    if (!K) return fail(c, SOC_ERR_ARG, "soc_absorbed_to_mabu: K is NULL");
    if (c->a2e_res_nfreq != c->at_nfreq)
        return fail(c, SOC_ERR_ARG, "soc_absorbed_to_mabu: the open soc_mabu_begin has %d frequencies, soc_absorbed_begin %d", c->a2e_res_nfreq, c->at_nfreq);
    ABSORBED_ROWS(c, "soc_absorbed_to_mabu", c0, c->a2e_cells);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, soc_launch_absorbed_to_rows(c->G, c->a2e_cells, c->at_nfreq, c0, c->bAT, c->mABS, K, nnnlimit, c->stream));
    return SOC_OK;
}

int soc_absorbed_download(soc_ctx *c, int64_t c0, int64_t n, float *rows, const float *K, float nnnlimit)
{
    if (!c || !rows) return SOC_ERR_ARG;
    FLUSH(c);
    ABSORBED_OPEN(c, "soc_absorbed_download");
    ABSORBED_ROWS(c, "soc_absorbed_download", c0, n);
    HIPCHK(c, hipSetDevice(c->device));
    const int NFREQ = c->at_nfreq;
    HIPCHK(c, c->bRows.reserve((size_t)std::min(n, ABSORBED_STAGE) * NFREQ, c->stream));
    for (int64_t a = 0; a < n; a += ABSORBED_STAGE) {
        const int64_t m = std::min(ABSORBED_STAGE, n - a);
        HIPCHK(c, soc_launch_absorbed_to_rows(c->G, m, NFREQ, c0 + a, c->bAT, c->bRows, K, nnnlimit, c->stream));
        HIPCHK(c, hipMemcpyAsync(rows + (size_t)a * NFREQ, c->bRows, (size_t)m * NFREQ * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));         // (the stage is used again)
    }
    return SOC_OK;
}

int soc_absorbed_end(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    absorbed_release(c);
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
