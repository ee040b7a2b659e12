// soc_capi_probe.hip -- host side of libsoc_hip.so: the probes the tests read device arithmetic through (seeds, math, one ray).
#include "soc_host.h"
#include "soc_rng.h"

#pragma GCC visibility push(default)
extern "C" {

int soc_probe_rng(soc_ctx *c, float SEED, uint32_t gid_first, uint32_t n, int ndraw, uint32_t *state_xc, uint32_t *draws)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!state_xc || !draws || ndraw < 0 || n == 0) return fail(c, SOC_ERR_ARG, "soc_probe_rng: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<uint32_t> dS, dD;
    HIPCHK(c, dS.reset((size_t)n * 2, c->stream));
    HIPCHK(c, dD.reset((size_t)n * ndraw, c->stream));
    HIPCHK(c, soc_launch_seed_probe(soc_seed_mul(SEED), c->dSeedTab, gid_first, n, ndraw, dS, dD, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(state_xc, dS, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (ndraw) HIPCHK(c, hipMemcpy(draws, dD, (size_t)n * ndraw * 4, hipMemcpyDeviceToHost));
    return SOC_OK;
}

int soc_probe_math2(soc_ctx *c, int fn, const float *x, const float *x2, float *y, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!x || !y || n <= 0) return fail(c, SOC_ERR_ARG, "soc_probe_math: bad arguments");
    if (fn < 0 || fn > 16) return fail(c, SOC_ERR_ARG, "soc_probe_math: no function %d", fn);
    if ((fn == 14 || fn == 15 || fn == 16) != (x2 != nullptr)) return fail(c, SOC_ERR_ARG, "soc_probe_math: function %d takes %s", fn, x2 ? "one argument" : "two arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> dx, dx2, dy;                              // (dx2 stays empty for the functions of one argument)
    HIPCHK(c, dx.reset((size_t)n, c->stream));
    HIPCHK(c, dy.reset((size_t)n, c->stream));
    if (x2) HIPCHK(c, dx2.reset((size_t)n, c->stream));
    HIPCHK(c, hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    if (x2) HIPCHK(c, hipMemcpy(dx2, x2, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, soc_launch_math_probe(fn, dx, dx2, dy, (long)n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(y, dy, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SOC_OK;
}

int soc_probe_math(soc_ctx *c, int fn, const float *x, float *y, int64_t n) { return soc_probe_math2(c, fn, x, nullptr, y, n); }

int soc_probe_trace(soc_ctx *c, const float pos[3], const float dir[3], int maxsteps,
                    int32_t *levels, int32_t *inds, float *ds, float endpos[3], int32_t *nsteps)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_probe_trace: call soc_set_grid first");
    if (!pos || !dir || maxsteps < 1 || !levels || !inds || !ds || !endpos || !nsteps) return fail(c, SOC_ERR_ARG, "soc_probe_trace: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> dIn, dDs;
    DevBuf<int>   dLev, dN;
    HIPCHK(c, dIn.reset(9, c->stream));
    HIPCHK(c, dDs.reset((size_t)maxsteps, c->stream));
    HIPCHK(c, dLev.reset((size_t)maxsteps * 2, c->stream));
    HIPCHK(c, dN.reset(1, c->stream));
    float h[9] = { pos[0], pos[1], pos[2], dir[0], dir[1], dir[2], 0, 0, 0 };
    const SocVariant V = soc_grid_variant(c->G);
    HIPCHK(c, hipMemcpy(dIn, h, sizeof h, hipMemcpyHostToDevice));
    HIPCHK(c, soc_launch_trace(c->G, V, dIn, dIn + 3, maxsteps, dLev, dLev + maxsteps, dDs, dIn + 6, dN, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(nsteps, dN, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(levels, dLev, (size_t)maxsteps * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(inds, dLev + maxsteps, (size_t)maxsteps * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ds, dDs, (size_t)maxsteps * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(endpos, dIn + 6, 12, hipMemcpyDeviceToHost));
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
