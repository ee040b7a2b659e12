// soc_capi_post.hip -- host side of libsoc_hip.so: what follows the simulation -- equilibrium temperatures and emission, maps,
// polarisation maps and the optical depths towards the point sources (kernels: soc_emit.hip, soc_map.hip).
#include "soc_host.h"

#include <cmath>
#include <cstring>

#pragma GCC visibility push(default)
extern "C" {

// ------------------------------------------------------------------------------------
// equilibrium temperature and emission (ASOC.py `CLT` / `CLE` paths)
// ------------------------------------------------------------------------------------

int soc_solve_temperature(soc_ctx *c, float adhoc, float kE, float Emin, int NE, const float *TTT, float FACTOR, float LENGTH,
                          const float *EABS, float *TNEW)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_solve_temperature: call soc_set_grid first");
    if (!TTT || !EABS || NE < 2 || !(kE > 1.0f) || !(Emin > 0.0f) || !(adhoc > 0.0f) || !(LENGTH > 0.0f))
        return fail(c, SOC_ERR_ARG, "soc_solve_temperature: need TTT[NE>=2], EABS, kE>1, Emin>0, adhoc>0, LENGTH>0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)c->G.CELLS;
    if (!c->dT) HIPCHK(c, c->dT.reset(cells, c->stream));
    HIPCHK(c, c->dTTT.reserve((size_t)NE, c->stream));
    HIPCHK(c, c->dEbuf.reserve(cells, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dTTT, TTT, (size_t)NE * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dEbuf, EABS, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_eqtemp(c->G, adhoc, kE, Emin, NE, FACTOR, LENGTH, c->cr_rate, c->dTTT, c->dEbuf, c->dT, c->stream));
    if (TNEW) HIPCHK(c, hipMemcpyAsync(TNEW, c->dT, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_T = true;
    return SOC_OK;
}

int soc_set_cr_heating(soc_ctx *c, float rate)
{
    if (!c) return SOC_ERR_ARG;
    if (!(rate >= 0.0f) || !std::isfinite(rate)) return fail(c, SOC_ERR_ARG, "soc_set_cr_heating: rate %g (>= 0; 0 switches it off)", (double)rate);
    c->cr_rate = rate;
    return SOC_OK;
}

int soc_set_map_roi(soc_ctx *c, const int32_t *ROI)
{
    if (!c) return SOC_ERR_ARG;
    if (!ROI) { c->map_roi_on = 0;  return SOC_OK; }
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_map_roi: call soc_set_grid first");
    const int N[3] = { c->G.NX, c->G.NY, c->G.NZ };
    for (int k = 0; k < 3; k++)
        if (ROI[2 * k] < 0 || ROI[2 * k + 1] < ROI[2 * k] || ROI[2 * k + 1] >= N[k])
            return fail(c, SOC_ERR_ARG, "soc_set_map_roi: limits %d..%d on axis %d of a grid of %d root cells", ROI[2 * k], ROI[2 * k + 1], k, N[k]);
    for (int k = 0; k < 6; k++) c->map_roi[k] = ROI[k];
    c->map_roi_on = 1;
    return SOC_OK;
}

int soc_set_map_threshold(soc_ctx *c, int level)
{
    if (!c) return SOC_ERR_ARG;
    if (level < 0 || level > SOC_MAXL) return fail(c, SOC_ERR_ARG, "soc_set_map_threshold: level %d", level);
    c->map_level_threshold = level;
    return SOC_OK;
}

int soc_set_map_interpolation(soc_ctx *c, int mode)
{
    if (!c) return SOC_ERR_ARG;
    if (mode < 0 || mode > 2) return fail(c, SOC_ERR_ARG, "soc_set_map_interpolation: mode %d (0, 1 or 2)", mode);
    c->map_interpolation = mode;
    return SOC_OK;
}

int soc_set_temperature(soc_ctx *c, const float *T)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid || !T) return fail(c, SOC_ERR_STATE, "soc_set_temperature: needs a grid and T[CELLS]");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->dT) HIPCHK(c, c->dT.reset((size_t)c->G.CELLS, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dT, T, (size_t)c->G.CELLS * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_T = true;
    return SOC_OK;
}

int soc_emission(soc_ctx *c, int nfreq, const float *FREQ, const float *FABS, float FACTOR, float LENGTH, float *EMITTED)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_T) return fail(c, SOC_ERR_STATE, "soc_emission: call soc_solve_temperature or soc_set_temperature first");
    if (nfreq < 1 || !FREQ || !FABS || !EMITTED || !(LENGTH > 0.0f)) return fail(c, SOC_ERR_ARG, "soc_emission: nfreq %d", nfreq);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->dEF.reserve((size_t)2 * nfreq, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dEF, FREQ, (size_t)nfreq * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dEF + nfreq, FABS, (size_t)nfreq * 4, hipMemcpyHostToDevice, c->stream));
    // batches of cells, all frequencies (the layout of the emitted file: EMITTED[CELLS][nfreq])
    const int cells = c->G.CELLS;
    int batch = (int)(((size_t)64 << 20) / (size_t)nfreq);            // <= 256 MB of floats per batch
    if (batch < 1) batch = 1;
    if (batch > cells) batch = cells;
    const size_t need = (size_t)batch * nfreq;
    HIPCHK(c, c->dEbuf.reserve(need, c->stream));
    for (int a = 0; a < cells; a += batch) {
        const int b = (a + batch < cells) ? a + batch : cells;
        HIPCHK(c, soc_launch_emission(a, b, nfreq, FACTOR, LENGTH, c->dEF, c->dEF + nfreq, c->dT, c->dEbuf, c->stream));
        HIPCHK(c, hipMemcpyAsync(EMITTED + (size_t)a * nfreq, c->dEbuf, (size_t)(b - a) * nfreq * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return SOC_OK;
}

// ------------------------------------------------------------------------------------
// map making (ASOC.py:2924-3177 -> kernel_ASOC_map.c Mapping / HealpixMapping)
// ------------------------------------------------------------------------------------

// the view of soc_map and soc_map_block: their shared arguments checked (who: the caller's name for the message) ...
static int check_view(soc_ctx *c, const char *who, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *DIR, const float *RA,
                      const float *DE, const float *CENTRE, const float *INTOBS)
{
    const bool inside = INTOBS && INTOBS[0] > -1e10f;
    if (healpix) {
        if (NPIX_X < 1 || NPIX_X > 8192 || !inside) return fail(c, SOC_ERR_ARG, "%s: Healpix maps need NSIDE (NPIX_X) and an observer position", who);
    } else {
        if (NPIX_X < 1 || NPIX_Y < 1 || (int64_t)NPIX_X * NPIX_Y > 2147483647LL) return fail(c, SOC_ERR_ARG, "%s: NPIX %d x %d", who, NPIX_X, NPIX_Y);
        if (!inside && (!DIR || !RA || !DE || !CENTRE || !(MAP_DX > 0.0f))) return fail(c, SOC_ERR_ARG, "%s: DIR, RA, DE, CENTRE and MAP_DX > 0 are needed", who);
    }
    return SOC_OK;
}

// ... and written into the launch arguments, with the handle's switches (V: zeroed by the caller)
static void fill_view(const soc_ctx *c, SocMapView &V, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *DIR, const float *RA,
                      const float *DE, const float *CENTRE, const float *INTOBS, float LENGTH)
{
    const bool inside = INTOBS && INTOBS[0] > -1e10f;
    V.mode = healpix ? 1 : 0;
    V.NPIX_X = NPIX_X;  V.NPIX_Y = healpix ? 1 : NPIX_Y;
    V.LEVEL_THRESHOLD = c->map_level_threshold;
    V.MAPINT = healpix ? 0 : c->map_interpolation;
    V.ROI_MAP = c->map_roi_on;
    for (int k = 0; k < 6; k++) V.ROI[k] = c->map_roi[k];
    V.MAP_DX = MAP_DX;  V.LENGTH = LENGTH;
    for (int k = 0; k < 3; k++) {
        V.DIR[k] = DIR ? DIR[k] : 0.0f;  V.RA[k] = RA ? RA[k] : 0.0f;  V.DE[k] = DE ? DE[k] : 0.0f;
        V.CENTRE[k] = CENTRE ? CENTRE[k] : 0.0f;
        V.INTOBS[k] = inside ? INTOBS[k] : (k == 0 ? -1.0e12f : 0.0f);
    }
}

int soc_map(soc_ctx *c, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *EMIT, const float *DIR, const float *RA,
            const float *DE, const float *CENTRE, const float *INTOBS, float ABS, float SCA, int save_colden, float LENGTH,
            float *MAP, float *SAVETAU)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_map: call soc_set_grid first");
    if (!EMIT || !MAP || !SAVETAU) return fail(c, SOC_ERR_ARG, "soc_map: EMIT, MAP and SAVETAU are needed");
    if (int r = check_view(c, "soc_map", healpix, NPIX_X, NPIX_Y, MAP_DX, DIR, RA, DE, CENTRE, INTOBS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = healpix ? (size_t)12 * NPIX_X * NPIX_X : (size_t)NPIX_X * NPIX_Y;
    const size_t cells = (size_t)c->G.CELLS;
    HIPCHK(c, c->dMapEmit.reserve(cells, c->stream));
    HIPCHK(c, c->dMap.reserve(npix, c->stream));
    HIPCHK(c, c->dMapTau.reserve(npix, c->stream));
    SocMapArgs A;
    memset(&A, 0, sizeof A);
    fill_view(c, A, healpix, NPIX_X, NPIX_Y, MAP_DX, DIR, RA, DE, CENTRE, INTOBS, LENGTH);
    A.SAVE_COLDEN = save_colden;  A.ABS = ABS;  A.SCA = SCA;
    A.EMIT = c->dMapEmit;  A.OPT = c->dOPT;  A.MAP = c->dMap;  A.SAVETAU = c->dMapTau;
    HIPCHK(c, hipMemcpyAsync(c->dMapEmit, EMIT, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_map(c->G, A, c->dOPT != nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(MAP, c->dMap, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(SAVETAU, c->dMapTau, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

// one map per hierarchy level (`mapping nx ny dx 999`, ASOC.py:3323-3438 -> the Mapping of kernel_ASOC_map_H.c:380-497)
int soc_map_levels(soc_ctx *c, int NPIX_X, int NPIX_Y, float MAP_DX, const float *EMIT, const float *DIR, const float *RA, const float *DE,
                   const float *CENTRE, const float *INTOBS, float ABS, float SCA, float *MAP)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_map_levels: call soc_set_grid first");
    if (!EMIT || !MAP) return fail(c, SOC_ERR_ARG, "soc_map_levels: EMIT and MAP are needed");
    const int64_t planes = (int64_t)c->G.LEVELS;
    if (NPIX_X < 1 || NPIX_Y < 1 || (int64_t)NPIX_X * NPIX_Y > 2147483647LL / planes)
        return fail(c, SOC_ERR_ARG, "soc_map_levels: NPIX %d x %d (with %d levels)", NPIX_X, NPIX_Y, c->G.LEVELS);
    const bool inside = INTOBS && INTOBS[0] > -1e10f;
    if (inside) {
        for (int k = 0; k < 3; k++) if (!std::isfinite(INTOBS[k])) return fail(c, SOC_ERR_ARG, "soc_map_levels: INTOBS[%d] = %g", k, (double)INTOBS[k]);
    } else {
        if (!DIR || !RA || !DE || !CENTRE || !(MAP_DX > 0.0f)) return fail(c, SOC_ERR_ARG, "soc_map_levels: DIR, RA, DE, CENTRE and MAP_DX > 0 are needed");
        // the walk divides by the components of -DIR without clamping them (kernel_ASOC_map_H.c:460): a zero would send the position to NaN
        for (int k = 0; k < 3; k++) if (!std::isfinite(DIR[k]) || DIR[k] == 0.0f) return fail(c, SOC_ERR_ARG, "soc_map_levels: DIR[%d] = %g", k, (double)DIR[k]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)NPIX_X * NPIX_Y, cells = (size_t)c->G.CELLS, n = (size_t)planes * npix;
    HIPCHK(c, c->dMapEmit.reserve(cells, c->stream));
    HIPCHK(c, c->dMap.reserve(n, c->stream));
    SocMapLevArgs A;
    memset(&A, 0, sizeof A);
    A.NPIX_X = NPIX_X;  A.NPIX_Y = NPIX_Y;  A.MAP_DX = MAP_DX;  A.ABS = ABS;  A.SCA = SCA;
    for (int k = 0; k < 3; k++) {
        A.DIR[k] = DIR ? DIR[k] : 0.0f;  A.RA[k] = RA ? RA[k] : 0.0f;  A.DE[k] = DE ? DE[k] : 0.0f;
        A.CENTRE[k] = CENTRE ? CENTRE[k] : 0.0f;
        A.INTOBS[k] = inside ? INTOBS[k] : (k == 0 ? -1.0e12f : 0.0f);
    }
    A.EMIT = c->dMapEmit;  A.OPT = c->dOPT;  A.MAP = c->dMap;
    HIPCHK(c, hipMemcpyAsync(c->dMapEmit, EMIT, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_maplev(c->G, A, c->dOPT != nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(MAP, c->dMap, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

// maps of a batch of frequencies (`mapping nx ny dx NF`, ASOC.py:3442-3568 -> the kernel_ASOC_map_X.c the reference lacks)
int soc_map_block_max(void) { return SOC_MAPX_MAX; }

int soc_map_set_block(soc_ctx *c, int nf, const float *EMITX, const float *ABSX, const float *SCAX, const float *OPTX)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (nf == 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->dMapXEmit.release();  c->dMapXOpt.release();  c->dMapXOpa.release();  c->dMapXOut.release();  c->dMapLOut.release();
        c->mapx_nf = 0;
        return SOC_OK;
    }
    if (nf < 0 || nf > SOC_MAPX_MAX) return fail(c, SOC_ERR_ARG, "soc_map_set_block: %d frequencies in a batch (1..%d; 0 frees it)", nf, SOC_MAPX_MAX);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_map_set_block: call soc_set_grid first");
    if (!EMITX || !ABSX || !SCAX) return fail(c, SOC_ERR_ARG, "soc_map_set_block: EMITX, ABSX and SCAX are needed");
    const size_t n = (size_t)c->G.CELLS * (size_t)nf;
    c->mapx_nf = 0;                                           // (a batch that may be half written is none)
    HIPCHK(c, c->dMapXEmit.reserve(n, c->stream));
    HIPCHK(c, c->dMapXOpa.reserve((size_t)2 * SOC_MAPX_MAX, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dMapXEmit, EMITX, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dMapXOpa, ABSX, (size_t)nf * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dMapXOpa + nf, SCAX, (size_t)nf * 4, hipMemcpyHostToDevice, c->stream));
    if (OPTX) {
        HIPCHK(c, c->dMapXOpt.reserve(n, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->dMapXOpt, OPTX, n * 8, hipMemcpyHostToDevice, c->stream));
    } else if (c->dMapXOpt) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->dMapXOpt.release();
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mapx_nf = nf;
    return SOC_OK;
}

int soc_map_block(soc_ctx *c, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *DIR, const float *RA, const float *DE,
                  const float *CENTRE, const float *INTOBS, float LENGTH, float *MAPX, float *TAUX, float *COLDEN)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_map_block: call soc_set_grid first");
    if (c->mapx_nf < 1) return fail(c, SOC_ERR_ARG, "soc_map_block: no batch is resident; soc_map_set_block with 1..%d frequencies first", SOC_MAPX_MAX);
    if (!MAPX || !TAUX || !COLDEN) return fail(c, SOC_ERR_ARG, "soc_map_block: MAPX, TAUX and COLDEN are needed");
    if (int r = check_view(c, "soc_map_block", healpix, NPIX_X, NPIX_Y, MAP_DX, DIR, RA, DE, CENTRE, INTOBS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = healpix ? (size_t)12 * NPIX_X * NPIX_X : (size_t)NPIX_X * NPIX_Y;
    const size_t nf = (size_t)c->mapx_nf;
    HIPCHK(c, c->dMapXOut.reserve((2 * nf + 1) * npix, c->stream));
    SocMapXArgs A;
    memset(&A, 0, sizeof A);
    fill_view(c, A, healpix, NPIX_X, NPIX_Y, MAP_DX, DIR, RA, DE, CENTRE, INTOBS, LENGTH);
    A.nf = c->mapx_nf;
    A.EMIT = c->dMapXEmit;  A.ABS = c->dMapXOpa;  A.SCA = c->dMapXOpa + nf;  A.OPT = c->dMapXOpt;
    A.MAP = c->dMapXOut;  A.TAU = c->dMapXOut + nf * npix;  A.COLDEN = c->dMapXOut + 2 * nf * npix;
    HIPCHK(c, soc_launch_mapx(c->G, A, c->stream));
    HIPCHK(c, hipMemcpyAsync(MAPX, A.MAP, nf * npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(TAUX, A.TAU, nf * npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(COLDEN, A.COLDEN, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

// the levels of the plain map (`maplevels 1`; nothing in the reference -- its per-level Mapping is soc_map_levels): the resident
// batch is read, the planes are a buffer of their own
int soc_map_block_levels_width(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_map_block_levels_width: call soc_set_grid first");
    return soc_maplevx_width(c->G.LEVELS);
}

int soc_map_block_levels(soc_ctx *c, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *DIR, const float *RA, const float *DE,
                         const float *CENTRE, const float *INTOBS, float *MAPL)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_map_block_levels: call soc_set_grid first");
    if (c->mapx_nf < 1) return fail(c, SOC_ERR_ARG, "soc_map_block_levels: no batch is resident; soc_map_set_block with 1..%d frequencies first", SOC_MAPX_MAX);
    if (!MAPL) return fail(c, SOC_ERR_ARG, "soc_map_block_levels: MAPL is needed");
    if (int r = check_view(c, "soc_map_block_levels", healpix, NPIX_X, NPIX_Y, MAP_DX, DIR, RA, DE, CENTRE, INTOBS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = healpix ? (size_t)12 * NPIX_X * NPIX_X : (size_t)NPIX_X * NPIX_Y;
    const size_t nf = (size_t)c->mapx_nf, n = nf * (size_t)c->G.LEVELS * npix;
    if (c->dMapLOut.n < n) {
        // refused rather than tried: a failed allocation of this size would leave the handle with an error of the runtime's
        size_t avail = 0, total = 0;
        HIPCHK(c, hipMemGetInfo(&avail, &total));
        if (c->dMapLOut.owned) avail += c->dMapLOut.bytes();
        if (n * 4 > avail)
            return fail(c, SOC_ERR_ARG, "soc_map_block_levels: %d frequencies x %d levels x %zu pixels are %.3f GiB of planes, %.3f GiB of device memory are free",
                        c->mapx_nf, c->G.LEVELS, npix, (double)(n * 4) / 1073741824.0, (double)avail / 1073741824.0);
        HIPCHK(c, c->dMapLOut.reset(n, c->stream));
    }
    SocMapLXArgs A;
    memset(&A, 0, sizeof A);
    fill_view(c, A, healpix, NPIX_X, NPIX_Y, MAP_DX, DIR, RA, DE, CENTRE, INTOBS, 1.0f);
    A.nf = c->mapx_nf;
    A.EMIT = c->dMapXEmit;  A.ABS = c->dMapXOpa;  A.SCA = c->dMapXOpa + nf;  A.OPT = c->dMapXOpt;
    A.MAPL = c->dMapLOut;
    HIPCHK(c, soc_launch_maplevx(c->G, A, c->stream));
    HIPCHK(c, hipMemcpyAsync(MAPL, A.MAPL, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

// polarisation maps (ASOC.py:3651-3801 -> PolMapping, kernel_ASOC_map.c:972-1137, :1147-1384, :1594-1693)
static int pack_bfield(soc_ctx *c, const float *Bx, const float *By, const float *Bz)
{
    const size_t cells = (size_t)c->G.CELLS;
    DevBuf<float> tmp;                                      // Bx | By | Bz as they come
    HIPCHK(c, tmp.reset(3 * cells, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->dBfield) HIPCHK(c, c->dBfield.reset(cells, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp, Bx, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp + cells, By, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp + 2 * cells, Bz, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_pack_bfield((int)cells, tmp, tmp + cells, tmp + 2 * cells, c->dBfield, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_set_bfield(soc_ctx *c, const float *Bx, const float *By, const float *Bz)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (!Bx && !By && !Bz) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->dBfield.release();
        return SOC_OK;
    }
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_bfield: call soc_set_grid first");
    if (!Bx || !By || !Bz) return fail(c, SOC_ERR_ARG, "soc_set_bfield: Bx, By and Bz are needed (all NULL frees the field)");
    const int r = pack_bfield(c, Bx, By, Bz);
    if (r) c->dBfield.release();                            // (a field that may be half written is none)
    return r;
}

int soc_polmap(soc_ctx *c, int polstat, int polred, int rho_weight, float p0, int NPIX_X, int NPIX_Y, float MAP_DX, const float *EMIT,
               const float *DIR, const float *RA, const float *DE, const float *CENTRE, float ABS, float SCA, float LENGTH, float *MAP)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_polmap: call soc_set_grid first");
    if (polstat != 0 && polstat != 1 && polstat != 3) return fail(c, SOC_ERR_ARG, "soc_polmap: polstat %d (0, 1 or 3)", polstat);
    if (polstat == 3 && polred) return fail(c, SOC_ERR_ARG, "soc_polmap: polstat 3 uses the full field vector, polred cannot be encoded in it");
    if (!c->dBfield) return fail(c, SOC_ERR_STATE, "soc_polmap: call soc_set_bfield first");
    if (!EMIT || !MAP || !DIR || !RA || !DE || !CENTRE || !(MAP_DX > 0.0f)) return fail(c, SOC_ERR_ARG, "soc_polmap: EMIT, MAP, DIR, RA, DE, CENTRE and MAP_DX > 0 are needed");
    if (NPIX_X < 1 || NPIX_Y < 1 || (int64_t)NPIX_X * NPIX_Y > 2147483647LL / 4) return fail(c, SOC_ERR_ARG, "soc_polmap: NPIX %d x %d", NPIX_X, NPIX_Y);
    // the walk divides by the components of -DIR without clamping them (kernel_ASOC_map.c:1033): a zero would send the position to NaN
    for (int k = 0; k < 3; k++) if (!std::isfinite(DIR[k]) || DIR[k] == 0.0f) return fail(c, SOC_ERR_ARG, "soc_polmap: DIR[%d] = %g", k, (double)DIR[k]);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)NPIX_X * NPIX_Y, cells = (size_t)c->G.CELLS;
    HIPCHK(c, c->dMapEmit.reserve(cells, c->stream));
    HIPCHK(c, c->dPolMap.reserve(4 * npix, c->stream));
    SocPolArgs A;
    memset(&A, 0, sizeof A);
    A.polstat = polstat;  A.polred = polred ? 1 : 0;  A.rho_weight = rho_weight ? 1 : 0;
    A.LEVEL_THRESHOLD = c->map_level_threshold;
    A.NPIX_X = NPIX_X;  A.NPIX_Y = NPIX_Y;
    A.p0 = p0;  A.MAP_DX = MAP_DX;  A.ABS = ABS;  A.SCA = SCA;  A.LENGTH = LENGTH;
    for (int k = 0; k < 3; k++) { A.DIR[k] = DIR[k];  A.RA[k] = RA[k];  A.DE[k] = DE[k];  A.CENTRE[k] = CENTRE[k]; }
    A.EMIT = c->dMapEmit;  A.OPT = c->dOPT;  A.B = c->dBfield;  A.MAP = c->dPolMap;
    HIPCHK(c, hipMemcpyAsync(c->dMapEmit, EMIT, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_polmap(c->G, A, c->dOPT != nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(MAP, c->dPolMap, 4 * npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

// all-sky polarisation map (ASOC.py:3808-3958 -> PolHealpixMapping, kernel_ASOC_map_H.c:576-841)
int soc_polmap_healpix(soc_ctx *c, int NSIDE, int polred, float p0, int interpolate, float minlos, float maxlos, float y_shear,
                       const float *EMIT, const float *INTOBS, float ABS, float SCA, float LENGTH, float *MAP)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_polmap_healpix: call soc_set_grid first");
    if (!c->dBfield) return fail(c, SOC_ERR_STATE, "soc_polmap_healpix: call soc_set_bfield first");
    if (!EMIT || !MAP || !INTOBS) return fail(c, SOC_ERR_ARG, "soc_polmap_healpix: EMIT, INTOBS and MAP are needed");
    if (NSIDE < 1 || NSIDE > 8192) return fail(c, SOC_ERR_ARG, "soc_polmap_healpix: NSIDE %d (1..8192)", NSIDE);
    if (interpolate < 0 || interpolate > 3) return fail(c, SOC_ERR_ARG, "soc_polmap_healpix: interpolate %d (0..3)", interpolate);
    if ((interpolate == 1 || interpolate == 2) && c->G.LEVELS > 1)
        return fail(c, SOC_ERR_ARG, "soc_polmap_healpix: interpolate %d indexes level 0 as a plain grid and would read links as densities on a hierarchy of %d levels (0 or 3 there)",
                    interpolate, c->G.LEVELS);
    if (!std::isfinite(y_shear) || std::isnan(minlos) || std::isnan(maxlos) || !std::isfinite(p0))
        return fail(c, SOC_ERR_ARG, "soc_polmap_healpix: p0, minlos, maxlos and y_shear must be numbers");
    // a ray near the equator leaves through a z face only after ~NZ/1e-5 root cells: without a line-of-sight limit it wraps that long
    if (y_shear != 0.0f && !(maxlos < 1.0e9f)) return fail(c, SOC_ERR_ARG, "soc_polmap_healpix: y_shear %g needs maxlos < 1e9 (given %g)", (double)y_shear, (double)maxlos);
    for (int k = 0; k < 3; k++) if (!std::isfinite(INTOBS[k])) return fail(c, SOC_ERR_ARG, "soc_polmap_healpix: INTOBS[%d] = %g", k, (double)INTOBS[k]);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)12 * NSIDE * NSIDE, cells = (size_t)c->G.CELLS;
    HIPCHK(c, c->dMapEmit.reserve(cells, c->stream));
    HIPCHK(c, c->dPolMap.reserve(4 * npix, c->stream));
    SocHPolArgs A;
    memset(&A, 0, sizeof A);
    A.NSIDE = NSIDE;  A.polred = polred ? 1 : 0;  A.LEVEL_THRESHOLD = c->map_level_threshold;  A.INTERPOLATE = interpolate;
    A.p0 = p0;  A.MINLOS = minlos;  A.MAXLOS = maxlos;  A.Y_SHEAR = y_shear;  A.ABS = ABS;  A.SCA = SCA;  A.LENGTH = LENGTH;
    for (int k = 0; k < 3; k++) A.INTOBS[k] = INTOBS[k];
    A.EMIT = c->dMapEmit;  A.OPT = c->dOPT;  A.B = c->dBfield;  A.MAP = c->dPolMap;
    HIPCHK(c, hipMemcpyAsync(c->dMapEmit, EMIT, cells * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_hpolmap(c->G, A, c->dOPT != nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(MAP, c->dPolMap, 4 * npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_ps_tau(soc_ctx *c, int NO_PS, const float *PSPOS, const float *DIR, float ABS, float SCA, float LENGTH, float *pscolden, float *pstau)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_ps_tau: call soc_set_grid first");
    if (NO_PS < 1 || NO_PS > 1000000 || !PSPOS || !DIR || !pscolden || !pstau) return fail(c, SOC_ERR_ARG, "soc_ps_tau: need NO_PS >= 1 sources, DIR and the two output arrays");
    for (int k = 0; k < 3; k++) if (!std::isfinite(DIR[k]) || DIR[k] == 0.0f) return fail(c, SOC_ERR_ARG, "soc_ps_tau: DIR[%d] = %g", k, (double)DIR[k]);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> d;                                        // PSPOS (4 floats per source) | colden | tau
    const size_t n = (size_t)NO_PS;
    HIPCHK(c, d.reset(n * 6, c->stream));
    HIPCHK(c, hipMemcpyAsync(d, PSPOS, n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, soc_launch_pstau(c->G, NO_PS, (const float4 *)d.p, DIR, ABS, SCA, c->dOPT, LENGTH, d + 4 * n, d + 5 * n, c->stream));
    HIPCHK(c, hipMemcpyAsync(pscolden, d + 4 * n, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pstau, d + 5 * n, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
