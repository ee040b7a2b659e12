// soc_capi.hip -- host side of libsoc_hip.so: the C ABI declared in include/soc_hip.h.
// Owns device memory, validates the model on the host before anything reaches a kernel,
// derives the per-launch seed constants and dispatches the kernels of soc_kernels.hip.
#include "soc_host.h"
#include "soc_rng.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>

#define SOC_HPBG_PIX 49152         // pixels of the Healpix sky (NSIDE 64, fixed in the reference: ASOC.py:297)

std::atomic<int64_t> soc_dev_bytes{0};

static std::string g_create_err;

int fail(soc_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else   g_create_err = buf;
    return code;
}

// Slot k of a store of copies (soc_ctx::slots), at least `bytes` large.  A larger buffer replaces a smaller one once the stream has
// drained (a launch in flight may read the old one); the contents stay otherwise.
template <typename T>
static int slot_buf(soc_ctx *c, int store, int k, size_t bytes, T **out)
{
    HIPCHK(c, c->slots[store][k].reserve(bytes, c->stream));
    *out = (T *)c->slots[store][k].p;
    return SOC_OK;
}

// A deferred launch's own copy of na floats of the handle at a (and of nb more at b, right behind them) in slot k of a store
// (a null a: the slot only)
static int slot_copy(soc_ctx *c, int store, int k, float **out, const float *a, size_t na, const float *b = nullptr, size_t nb = 0)
{
    int r = slot_buf(c, store, k, (na + nb) * 4, out);
    if (r) return r;
    if (a) HIPCHK(c, hipMemcpyAsync(*out, a, na * 4, hipMemcpyDeviceToDevice, c->stream));
    if (b) HIPCHK(c, hipMemcpyAsync(*out + na, b, nb * 4, hipMemcpyDeviceToDevice, c->stream));
    return SOC_OK;
}

// number of floats of the scattered-light image: NDIR maps of NPIX_X x NPIX_Y pixels, or one Healpix map
static size_t view_pixels(const soc_ctx *c)
{
    if (!c->have_view) return 0;
    if (c->view.NDIR < 0) return (size_t)12 * c->view.NDIR * c->view.NDIR;
    return (size_t)c->view.NDIR * c->view.NPIX_X * c->view.NPIX_Y;
}

// Hierarchies on which the brick sweep keeps the brick's cells in LDS (soc_brick.hip, soc_ltree.h): there a lone
// launch with enough work items pays too -- also with the INT tally, which lives in LDS beside TABS.
// With per-cell opacities: soc_set_tuning("abu_local", 1), and neither with_int 2 nor ALI (soc_dev.h: soc_brick_local).
// Hierarchies with Index() in float: soc_set_tuning("float_local", 1) and scalar opacities.
static bool lt_capable(const soc_ctx *c, bool abu)
{
    return soc_brick_local(c->G, soc_grid_variant(c->G, abu, c->with_int), c->tune) && !(abu && c->with_ali);
}
// ... the launches of the scattered-light kernels (alone, or those of a batch together) go to the sweep of rays.  Measured on the 256^3-root
// hierarchy (tools/exp_sca.py): 1.0e6 work items 0.47x the direct kernel, 3.1e6 0.92x, 8.4e6 1.3x, 5.0e7 1.6x (best direct launch shape), 32
// launches of 3.1e6 in one batch 4.4x
#define SOC_SCA_RAYS_LAUNCH 4000000
// Single-level (Cartesian) grids whose scattered-light launches can run as a sweep of rays (soc_dev.h: soc_brick_cart) ...
static bool cart_capable(const soc_ctx *c) { return soc_brick_cart(c->G, soc_grid_variant(c->G, false)); }
// ... and the rule of automatic mode there.  Measured on synth.cartesian_cloud grids, background launches of the reference's shape (8 work
// items per surface element), 3 observers, 256^2 pixels, the sweep of rays against the direct kernel (tools/exp_sca.py --compare; DESIGN.md
// section 5, profiles/sca_cartesian_lines.json):
//   lone launch                  128^3 (7.9e5 work items) 0.29x   256^3 (3.1e6) 0.66x   512^3 (1.3e7) 0.97x
//   batch of 6.3e6 work items    128^3 1.01x                      256^3 1.02x
//   batch of 2.5e7 work items    128^3 1.75x                      256^3 2.12x           512^3 1.44x (1.0e8: 2.57x)
// A lone launch never came out ahead: it keeps the direct kernel.  The launches of a batch go to the sweep from 2.5e7 work items on, the
// smallest batch measured to pay beyond run-to-run scatter (1 %) on every grid; at 6.3e6 the two paths are level.
#define SOC_CART_RAYS_BATCH 25000000LL                      /* work items of the launches of a batch together */
static bool cart_rays_pay(const soc_ctx *c, long long items, bool batch)
{
    const int B = SOC_CART_BRICK_EDGE;
    const long long nb = (long long)((c->G.NX + B - 1) / B) * ((c->G.NY + B - 1) / B) * ((c->G.NZ + B - 1) / B);
    return batch && nb >= 8 && items >= SOC_CART_RAYS_BATCH;      // (nb >= 8 bricks of 16^3: the floor of the absorption rule)
}
#define SOC_LT_LONE_LAUNCH 1000000                           // work items from which a lone launch goes to the sweep there

// One launch through the direct kernel of its kind (SOURCE 4 and 5 mark Healpix and cell-emission launches for the brick sweep; the
// direct kernels take them as 1 and 2).  A scattered-light launch adds to its own image; soc_last_variant names its instance of
// soc_sca_kernel with bit 15 (soc_dev.h: soc_sca_variant_code, from the variant sca_dispatch switches on).
static int run_direct(soc_ctx *c, SocSim S, const SocVariant &V)
{
    c->last.passes = 0;
    const int kind = soc_source_kind(S.SOURCE);
    if (kind) S.SOURCE = kind;
    if (S.SCAKIND) {
        SocSca X = c->view;
        X.kind = S.SCAKIND - 1;  X.DSC = S.DSC;  X.OUT = S.OUT;
        if (S.gid_count > 0) c->last.variant = soc_sca_variant_code(X.kind, V);      // (sca_dispatch runs nothing without work items)
        HIPCHK(c, soc_launch_sca(c->G, S, X, V, c->stream));
        return SOC_OK;
    }
    if (S.gid_count > 0)                    // (the launch wrappers run nothing without work items; Cartesian grids take the float kernels)
        c->last.variant = soc_variant_code(soc_grid_plan(0, kind, V));
    if (kind == 1)      HIPCHK(c, soc_launch_sim_hp(c->G, S, V, c->stream));
    else if (kind == 2) HIPCHK(c, soc_launch_sim_cl(c->G, S, V, c->stream));
    else                HIPCHK(c, soc_launch_sim_pb(c->G, S, V, c->stream));
    return SOC_OK;
}

// Execute the launches deferred since soc_batch_begin: one brick sweep for all of them (scattered light: one sweep of rays).  They run
// through the direct kernel instead when that is as fast -- a lone absorption launch on a hierarchy (1.9e10 vs 2.0e10 steps/s at 256^3,
// 4 levels), scattered-light launches with too few rays to fill the brick queues -- and scattered-light launches also where the sweep
// does not apply (it did when they were deferred: the grid has not changed since).
int flush_pending(soc_ctx *c)
{
    if (c->pending.empty()) return SOC_OK;
    std::vector<SocSim> todo;
    todo.swap(c->pending);
    c->opt_used = 0;                                        // (the next deferred launch with per-cell opacities takes a copy of its own)
    const bool rays = todo[0].SCAKIND != 0;
    // what made the launches deferrable (see route_sim)
    const SocVariant V = soc_grid_variant(c->G, todo[0].OPT != nullptr, (!rays && c->int_mode != soc_ctx::INT_OFF) ? c->with_int : 0);
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long items = 0;
    for (const SocSim &S : todo) items += S.gid_count;
    const bool direct = rays ? (c->exec_mode != 1 && !(cart_capable(c) ? cart_rays_pay(c, (long long)items, true) : items >= SOC_SCA_RAYS_LAUNCH))
                             : (V.octree && todo.size() == 1 && c->exec_mode < 0 && !(lt_capable(c, V.abu != 0) && items >= SOC_LT_LONE_LAUNCH));
    hipError_t e = hipErrorNotSupported;
    if (!direct)
        e = soc_brick_run_pb(*c->sweep, c->G, todo.data(), (int)todo.size(), V, c->brick_log2, c->tune, c->stream, &c->last, rays ? &c->view : nullptr);
    // (per-cell opacities: launches deferred for the brick-local form whose hierarchy cannot be cut into bricks after all)
    if (direct || ((rays || V.abu) && e == hipErrorNotSupported)) {
        for (const SocSim &S : todo) {
            int r = run_direct(c, S, V);
            if (r) return r;
        }
        return SOC_OK;
    }
    if (e != hipSuccess) return fail(c, SOC_ERR_HIP, "brick sweep of %d deferred launches failed: %s", (int)todo.size(), hipGetErrorString(e));
    return SOC_OK;
}

#pragma GCC visibility push(default)
extern "C" {

const char *soc_version(void) { return "soc_hip 0.1 (gfx950)"; }

const char *soc_last_error(const soc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int soc_create(int device, soc_ctx **out)
{
    if (!out) return fail(nullptr, SOC_ERR_ARG, "soc_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        // two HIP runtimes in one process (torch ships its own libamdhip64.so): the one initialised second finds no device
        std::string first, second;
        if (FILE *fp = fopen("/proc/self/maps", "r")) {
            char line[1024];
            while (fgets(line, sizeof line, fp)) {
                const char *q = strstr(line, "libamdhip64");
                if (!q) continue;
                const char *b = strchr(line, '/');
                if (!b) continue;
                std::string path(b);
                while (!path.empty() && (path.back() == '\n' || path.back() == ' ')) path.pop_back();
                if (first.empty()) first = path;
                else if (path != first && second.empty()) second = path;
            }
            fclose(fp);
        }
        if (!second.empty())
            return fail(nullptr, SOC_ERR_HIP, "soc_create: no HIP device available (%s): two HIP runtimes are loaded in this process (%s and %s) and the "
                        "one initialised second finds no device -- load torch's first (import torch before libsoc_hip.so is opened; soc_amd.lib does)",
                        hipGetErrorString(e), first.c_str(), second.c_str());
        return fail(nullptr, SOC_ERR_HIP, "soc_create: no HIP device available (%s)", hipGetErrorString(e));
    }
    if (device < 0 || device >= ndev)
        return fail(nullptr, SOC_ERR_ARG, "soc_create: device %d out of range (0..%d)", device, ndev - 1);
    soc_ctx *c = new soc_ctx();
    c->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) {
        int r = fail(nullptr, SOC_ERR_HIP, "soc_create: %s", hipGetErrorString(e));
        delete c;
        return r;
    }
    c->stream = c->own_stream;
    // seed tables: T[k][b] = G^(b*256^k) mod M with G = A^(2^38) mod M  (soc_rng.h)
    std::vector<uint64_t> tab(1024);
    soc_build_seed_table(tab.data());
    if ((e = c->dSeedTab.reset(1024, c->stream)) != hipSuccess ||
        (e = hipMemcpy(c->dSeedTab, tab.data(), 1024 * sizeof(uint64_t), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = c->dStats.reset(4, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->dStats, 0, 4 * sizeof(unsigned long long), c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        int r = fail(nullptr, SOC_ERR_HIP, "soc_create: %s", hipGetErrorString(e));
        soc_destroy(c);
        return r;
    }
    *out = c;
    return SOC_OK;
}

void soc_destroy(soc_ctx *c)
{
    if (!c) return;
    (void)flush_pending(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                                               // (every DevBuf of the handle frees what it owns, those of its sweeps included)
}

int64_t soc_device_bytes(void) { return soc_dev_bytes.load(); }

int soc_set_stream(soc_ctx *c, void *hip_stream)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return SOC_OK;
}

int soc_set_grid(soc_ctx *c, int NX, int NY, int NZ, int LEVELS, const int32_t *LCELLS, const float *DENS)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!LCELLS || !DENS) return fail(c, SOC_ERR_ARG, "soc_set_grid: NULL array");
    if (NX < 1 || NY < 1 || NZ < 1 || NX > 9999) return fail(c, SOC_ERR_ARG, "soc_set_grid: bad dimensions %d %d %d", NX, NY, NZ);
    if (LEVELS < 1 || LEVELS > SOC_MAXL) return fail(c, SOC_ERR_ARG, "soc_set_grid: LEVELS=%d unsupported (1..%d)", LEVELS, SOC_MAXL);
    const int64_t nxyz = (int64_t)NX * NY * NZ;
    if (nxyz > 2147483647LL || LCELLS[0] != nxyz)
        return fail(c, SOC_ERR_ARG, "soc_set_grid: LCELLS[0]=%d does not match NX*NY*NZ=%lld", LCELLS[0], (long long)nxyz);
    SocGrid G{};
    G.NX = NX; G.NY = NY; G.NZ = NZ; G.LEVELS = LEVELS; G.NXYZ = (int)nxyz;
    int64_t cells = 0;
    for (int l = 0; l < LEVELS; l++) {
        if (LCELLS[l] < 0 || (l > 0 && LCELLS[l] % 8 != 0))
            return fail(c, SOC_ERR_ARG, "soc_set_grid: LCELLS[%d]=%d is not a whole number of octets", l, LCELLS[l]);
        G.OFF[l] = (int)cells;
        G.LCELLS[l] = LCELLS[l];
        cells += LCELLS[l];
        if (cells > 2147483647LL) return fail(c, SOC_ERR_ARG, "soc_set_grid: more than 2^31-1 cells");
    }
    G.CELLS = (int)cells;
    // validate links on the host: every parent must point at an aligned octet of the next level
    for (int l = 0; l < LEVELS; l++) {
        const float *d = DENS + G.OFF[l];
        const int nchild = (l + 1 < LEVELS) ? LCELLS[l + 1] : 0;
        for (int i = 0; i < LCELLS[l]; i++) {
            float v = d[i];
            if (v != v) return fail(c, SOC_ERR_ARG, "soc_set_grid: NaN density at level %d cell %d", l, i);
            if (!(v > 0.0f)) {
                uint32_t bits;
                memcpy(&bits, &v, 4);
                int first = (int)(bits ^ 0x80000000u);
                if (first < 0 || first % 8 != 0 || first + 8 > nchild)
                    return fail(c, SOC_ERR_ARG, "soc_set_grid: level %d cell %d: value %g is not a density and not a valid child link", l, i, (double)v);
            }
        }
    }
    // refused before anything of the handle changes: a refused call leaves the old grid usable
    if (c->have_grid && (int64_t)G.CELLS != c->G.CELLS && ((c->dTABS && !c->dTABS.owned) || (c->dINT && !c->dINT.owned)))
        return fail(c, SOC_ERR_STATE, "soc_set_grid: a caller-owned tally of %d cells is bound; soc_bind_tally(ctx, which, NULL, 0) first, re-bind after", c->G.CELLS);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->dDENS.reset((size_t)cells, c->stream));
    HIPCHK(c, hipMemcpy(c->dDENS, DENS, (size_t)cells * 4, hipMemcpyHostToDevice));
    c->npar = cells - nxyz;
    HIPCHK(c, c->dPAR.reset((size_t)c->npar, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dPAR, 0, (size_t)(c->npar ? c->npar : 1) * 4, c->stream));
    G.DENS = c->dDENS;
    G.PAR = c->dPAR;
    c->eET.release();  c->eRows.release();  c->release_change();  c->et_nfreq = 0;   // (the resident emission belongs to the model it was solved for)
    c->bAT.release();  c->bAC.release();  c->bRows.release();  c->at_nfreq = 0;  c->ac_kept = false;    // (and so do the absorptions)
    if ((int64_t)G.CELLS != c->G.CELLS || !c->have_grid) {
        // tallies follow the cell count
        for (DevBuf<float> *t : { &c->dTABS, &c->dINT })
            if (t->owned || !*t) { HIPCHK(c, t->reset((size_t)cells, c->stream)); HIPCHK(c, hipMemsetAsync(t->p, 0, (size_t)cells * 4, c->stream)); }
        c->dOPT.release();
        c->have_emit = false;
        // everything else that is sized by the cell count
        c->dT.release();  c->dXAB.release();  c->dEMINDEX.release();  c->dBfield.release();
        c->dMapXEmit.release();  c->dMapXOpt.release();  c->dMapLOut.release();  c->mapx_nf = 0;
        if (c->dINTV) {                                       // INTX, INTY, INTZ follow the cell count like TABS and INT (with_int stays 2)
            c->dINTV.release();
            if (c->with_int == 2) {
                HIPCHK(c, c->dINTV.reset((size_t)3 * cells, c->stream));
                HIPCHK(c, hipMemsetAsync(c->dINTV, 0, (size_t)3 * cells * 4, c->stream));
            }
        }
        c->have_T = false;  c->with_ali = false;  c->have_emindex = false;
        c->abu_ndust = 0;  c->abu_cells = 0;
    }
    c->G = G;
    c->have_grid = true;
    soc_sweep_invalidate(c->sweep);
    HIPCHK(c, soc_launch_parents(c->G, c->dPAR, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_set_features(soc_ctx *c, int with_int, int ps_method, int use_emweight)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!(ps_method == 0 || ps_method == 1 || ps_method == 2 || ps_method == 4 || ps_method == 5))
        return fail(c, SOC_ERR_ARG, "soc_set_features: PS_METHOD %d not supported (0,1,2,4,5)", ps_method);
    if (use_emweight < 0 || use_emweight > 2)
        return fail(c, SOC_ERR_ARG, "soc_set_features: USE_EMWEIGHT %d not supported (0,1,2)", use_emweight);
    if (with_int == 2) {                                    // SAVE_INTENSITY == 2: three more tallies (kernel_ASOC.c:604-612)
        if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_features: with_int 2 needs soc_set_grid first (it allocates INTX, INTY, INTZ)");
        HIPCHK(c, hipSetDevice(c->device));
        if (c->dINTV.n != (size_t)3 * c->G.CELLS) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, c->dINTV.reset((size_t)3 * c->G.CELLS, c->stream));
            HIPCHK(c, hipMemsetAsync(c->dINTV, 0, (size_t)3 * c->G.CELLS * 4, c->stream));
        }
    }
    c->with_int = (with_int == 2) ? 2 : (with_int ? 1 : 0);
    c->ps_method = ps_method;
    c->use_emweight = use_emweight;
    return SOC_OK;
}

int soc_set_mirror(soc_ctx *c, int mask)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (mask < 0 || mask > 63) return fail(c, SOC_ERR_ARG, "soc_set_mirror: mask %d (bits x,X,y,Y,z,Z = 1,2,4,8,16,32)", mask);
    c->mirror = mask;
    return SOC_OK;
}

int soc_set_exec(soc_ctx *c, int mode, int brick_log2)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (mode < -1 || mode > 1 || brick_log2 < 2 || brick_log2 > 4)
        return fail(c, SOC_ERR_ARG, "soc_set_exec: mode %d (-1,0,1), brick_log2 %d (2..4)", mode, brick_log2);
    c->exec_mode = mode;
    c->brick_log2 = brick_log2;
    return SOC_OK;
}

int soc_set_tuning(soc_ctx *c, const char *name, int value)
{
    if (!c || !name) return SOC_ERR_ARG;
    FLUSH(c);
    if (value < 0) return fail(c, SOC_ERR_ARG, "soc_set_tuning: %s = %d (0 = built-in choice)", name, value);
    struct { const char *n; int *p; } tab[] = {
        { "threads", &c->tune.T }, { "chunk", &c->tune.P }, { "steps_per_visit", &c->tune.KCAP }, { "swap_lanes", &c->tune.FTH },
        { "climb_lanes", &c->tune.CTH }, { "brick_cells", &c->tune.CAP }, { "tail_lanes", &c->tune.TAIL }, { "park_below", &c->tune.park }, { "population", &c->tune.POP },
        { "hash_slots", &c->tune.HS }, { "global_tree", &c->tune.global_tree }, { "slow_every", &c->tune.slow_every },
        { "general_kernel", &c->tune.nolean }, { "oversubscribe", &c->tune.oversub }, { "verbose", &c->tune.verbose },
        { "abu_local", &c->tune.abu_local }, { "float_local", &c->tune.float_local }, { "brick_partition", &c->tune.partition } };
    for (auto &t : tab)
        if (!strcmp(name, t.n)) {
            if (t.p == &c->tune.partition && value > 2) return fail(c, SOC_ERR_ARG, "soc_set_tuning: brick_partition = %d (0 built-in, 1 tiles, 2 smallest face area)", value);
            if (t.p == &c->tune.CAP && value != c->tune.CAP) soc_sweep_invalidate(c->sweep);
            if (t.p == &c->tune.partition && (value == 1) != (c->tune.partition == 1)) soc_sweep_invalidate(c->sweep);      // (0 and 2 build the same bricks)
            *t.p = value;
            return SOC_OK;
        }
    return fail(c, SOC_ERR_ARG, "soc_set_tuning: unknown parameter '%s'", name);
}

int soc_last_passes(soc_ctx *c) { return c ? c->last.passes : 0; }
int soc_last_form(soc_ctx *c) { return (c && c->last.passes > 0) ? c->last.form : 0; }
int soc_last_variant(soc_ctx *c) { return c ? c->last.variant : -1; }

int soc_set_optical(soc_ctx *c, const float *ABS, const float *SCA, int ndust)
{
    if (!c) return SOC_ERR_ARG;
    if (!ABS || !SCA || ndust != 1) return fail(c, SOC_ERR_ARG, "soc_set_optical: need ABS, SCA with ndust==1 (WITH_MSF is not supported)");
    c->ABS = ABS[0];
    c->SCA = SCA[0];
    c->have_optical = true;
    return SOC_OK;
}

int soc_set_opt(soc_ctx *c, const float *OPT)
{
    if (!c) return SOC_ERR_ARG;
    // no flush: a deferred launch keeps its own copy of the opacities (route_sim)
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_opt: call soc_set_grid first");
    HIPCHK(c, hipSetDevice(c->device));
    c->opt_from_abu = false;
    c->opt_gen++;
    if (!OPT) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->dOPT.release();
        return SOC_OK;
    }
    if (!c->dOPT) HIPCHK(c, c->dOPT.reset((size_t)c->G.CELLS, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dOPT, OPT, (size_t)c->G.CELLS * 8, hipMemcpyHostToDevice, c->stream));
    if (c->opt_half) HIPCHK(c, soc_launch_opt_half(c->G.CELLS, c->dOPT, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_set_opt_half(soc_ctx *c, int on)
{
    if (!c) return SOC_ERR_ARG;
    c->opt_half = on != 0;                                  // applies to the next soc_set_opt / soc_set_optical_abu
    return SOC_OK;
}

int soc_set_abundances(soc_ctx *c, int NDUST, int single, const float *ABU)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_abundances: call soc_set_grid first");
    HIPCHK(c, hipSetDevice(c->device));
    c->opt_from_abu = false;
    if (!ABU) {                                             // off
        c->abu_ndust = 0;
        c->abu_cells = 0;
        return SOC_OK;
    }
    if (NDUST < 1 || NDUST > 64 || (single && NDUST != 2))
        return fail(c, SOC_ERR_ARG, "soc_set_abundances: NDUST %d (1..64; the one-abundance form describes exactly two species)", NDUST);
    const size_t n = (size_t)c->G.CELLS * (single ? 1 : NDUST);
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(ABU[i])) return fail(c, SOC_ERR_ARG, "soc_set_abundances: ABU[%zu] is not finite", i);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->dABU.reset(n, c->stream));
    HIPCHK(c, c->dAF.reset((size_t)2 * NDUST, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dABU, ABU, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->abu_ndust = NDUST;  c->abu_single = single ? 1 : 0;  c->abu_cells = (size_t)c->G.CELLS;
    return SOC_OK;
}

int soc_set_optical_abu(soc_ctx *c, const float *AFABS, const float *AFSCA, int ndust)
{
    if (!c) return SOC_ERR_ARG;
    // no flush: a deferred launch keeps its own copy of the opacities (route_sim)
    if (!c->abu_ndust || c->abu_cells != (size_t)c->G.CELLS) return fail(c, SOC_ERR_STATE, "soc_set_optical_abu: call soc_set_abundances (after soc_set_grid) first");
    if (!AFABS || !AFSCA || ndust != c->abu_ndust) return fail(c, SOC_ERR_ARG, "soc_set_optical_abu: need the cross sections of the %d species", c->abu_ndust);
    HIPCHK(c, hipSetDevice(c->device));
    c->opt_gen++;
    float af[128];
    for (int d = 0; d < ndust; d++) { af[d] = AFABS[d];  af[ndust + d] = AFSCA[d]; }
    if (!c->dOPT) HIPCHK(c, c->dOPT.reset((size_t)c->G.CELLS, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dAF, af, (size_t)2 * ndust * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // af is on the stack
    HIPCHK(c, soc_launch_opt(c->G.CELLS, ndust, c->abu_single, c->dABU, c->dAF, c->dOPT, c->stream));
    if (c->opt_half) HIPCHK(c, soc_launch_opt_half(c->G.CELLS, c->dOPT, c->stream));
    c->opt_from_abu = true;
    return SOC_OK;
}

int soc_read_opt(soc_ctx *c, float *OPT)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->dOPT || !OPT) return fail(c, SOC_ERR_STATE, "soc_read_opt: no per-cell opacities are set");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(OPT, c->dOPT, (size_t)c->G.CELLS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_set_scatter_tables(soc_ctx *c, int NDUST, const float *DSC, const float *CSC, int BINS)
{
    if (!c) return SOC_ERR_ARG;
    if (!CSC || BINS < 1 || BINS > 16000) return fail(c, SOC_ERR_ARG, "soc_set_scatter_tables: need CSC and 1 <= BINS <= 16000 (got %d)", BINS);
    if (NDUST < 1 || NDUST > 64) return fail(c, SOC_ERR_ARG, "soc_set_scatter_tables: NDUST %d (1..64)", NDUST);
    HIPCHK(c, hipSetDevice(c->device));
    if (NDUST > 1 || c->msf_ndust > 1) FLUSH(c);            // a deferred launch snapshots one table only: run what is pending first
    const size_t n = (size_t)NDUST * BINS;
    if (BINS != c->BINS || NDUST != c->msf_ndust || !c->dCSC) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->dCSC.reset(n, c->stream));
        HIPCHK(c, c->dDSC.reset(n, c->stream));
        c->BINS = BINS;
        c->msf_ndust = NDUST;
        c->have_dsc = false;
    }
    if (DSC) c->have_dsc = true;
    HIPCHK(c, hipMemcpyAsync(c->dCSC, CSC, n * 4, hipMemcpyHostToDevice, c->stream));
    if (DSC) HIPCHK(c, hipMemcpyAsync(c->dDSC, DSC, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));     // host buffer may be reused by the caller
    return SOC_OK;
}

int soc_set_scatter_table(soc_ctx *c, const float *DSC, const float *CSC, int BINS)
{
    return soc_set_scatter_tables(c, 1, DSC, CSC, BINS);
}

int soc_set_step_weight(soc_ctx *c, int mode, float SW_A, float SW_B)
{
    if (!c) return SOC_ERR_ARG;
    if (mode <= 0) { c->step_weight = 0;  c->sw_a = c->sw_b = 0.0f;  return SOC_OK; }
    if (mode > 2) return fail(c, SOC_ERR_ARG, "soc_set_step_weight: mode %d (0 off, 1 exp(-A*t), 2 B*exp(-A*t)+(1-B)*exp(-2*A*t))", mode);
    if (!(SW_A > 0.0f) || !std::isfinite(SW_A)) return fail(c, SOC_ERR_ARG, "soc_set_step_weight: SW_A=%g must be positive", (double)SW_A);
    if (mode == 2 && !(SW_B > 0.0f && SW_B < 1.0f)) return fail(c, SOC_ERR_ARG, "soc_set_step_weight: mode 2 needs 0 < SW_B < 1, got %g", (double)SW_B);
    c->step_weight = mode;  c->sw_a = SW_A;  c->sw_b = SW_B;
    return SOC_OK;
}

int soc_set_emission(soc_ctx *c, const float *EMIT, const float *EMWEI)
{
    if (!c) return SOC_ERR_ARG;
    // no flush: a deferred SimRAM_CL launch keeps its own copy of EMIT and EMWEI (soc_sim_cl)
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_emission: call soc_set_grid first");
    if (!EMIT) return fail(c, SOC_ERR_ARG, "soc_set_emission: EMIT is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->G.CELLS;
    if (!c->have_emit) {
        HIPCHK(c, c->dEMIT.reset(n, c->stream));
        HIPCHK(c, c->dEMWEI.reset(n, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dEMWEI, 0, n * 4, c->stream));
        c->have_emit = true;
    }
    HIPCHK(c, hipMemcpyAsync(c->dEMIT, EMIT, n * 4, hipMemcpyHostToDevice, c->stream));
    if (EMWEI) HIPCHK(c, hipMemcpyAsync(c->dEMWEI, EMWEI, n * 4, hipMemcpyHostToDevice, c->stream));
    c->emit_gen++;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_set_emindex(soc_ctx *c, const int32_t *EMINDEX)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid || !EMINDEX) return fail(c, SOC_ERR_STATE, "soc_set_emindex: needs a grid and EMINDEX[CELLS]");
    for (int i = 0; i < c->G.CELLS; i++)
        if (EMINDEX[i] >= c->G.CELLS) return fail(c, SOC_ERR_ARG, "soc_set_emindex: EMINDEX[%d] = %d is not a cell", i, EMINDEX[i]);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->dEMINDEX) HIPCHK(c, c->dEMINDEX.reset((size_t)c->G.CELLS, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dEMINDEX, EMINDEX, (size_t)c->G.CELLS * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_emindex = true;
    return SOC_OK;
}

int soc_set_ali(soc_ctx *c, int with_ali)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_ali: call soc_set_grid first");
    HIPCHK(c, hipSetDevice(c->device));
    if (with_ali && !c->dXAB) {
        HIPCHK(c, c->dXAB.reset((size_t)c->G.CELLS, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dXAB, 0, (size_t)c->G.CELLS * 4, c->stream));
    }
    c->with_ali = with_ali != 0;
    return SOC_OK;
}

static float *tally_buf(soc_ctx *c, int which)
{
    if (which == SOC_TALLY_TABS) return c->dTABS;
    if (which == SOC_TALLY_INT) return c->dINT;
    if (which == SOC_TALLY_XAB) return c->with_ali ? c->dXAB : nullptr;
    if (which >= SOC_TALLY_INTX && which <= SOC_TALLY_INTZ)
        return (c->with_int == 2 && c->dINTV) ? c->dINTV + (size_t)(which - SOC_TALLY_INTX) * c->G.CELLS : nullptr;
    return nullptr;
}

int soc_zero(soc_ctx *c, int tag)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_zero: call soc_set_grid first");
    float *b = tally_buf(c, tag);
    if (!b) return fail(c, SOC_ERR_ARG, "soc_zero: tag %d", tag);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(b, 0, (size_t)c->G.CELLS * 4, c->stream));
    if (tag == SOC_TALLY_TABS && c->with_ali && c->dXAB)           // ZeroAMC tag 0 clears TABS and XAB (kernel_ASOC_aux.c:664-668)
        HIPCHK(c, hipMemsetAsync(c->dXAB, 0, (size_t)c->G.CELLS * 4, c->stream));
    if (tag == SOC_TALLY_INT && c->with_int == 2 && c->dINTV)      // ... tag 1 INT and the three vector sums (:676-681)
        HIPCHK(c, hipMemsetAsync(c->dINTV, 0, (size_t)3 * c->G.CELLS * 4, c->stream));
    return SOC_OK;
}

static int check_launch(soc_ctx *c, const char *who, int BATCH, int GLOBAL, int gid_first, int gid_count)
{
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "%s: call soc_set_grid first", who);
    if (!c->dCSC) return fail(c, SOC_ERR_STATE, "%s: call soc_set_scatter_table first", who);
    if (!c->dOPT && !c->have_optical) return fail(c, SOC_ERR_STATE, "%s: call soc_set_optical or soc_set_opt first", who);
    if (c->msf_ndust > 1 && !(c->opt_from_abu && c->dOPT && c->abu_ndust == c->msf_ndust && !c->abu_single && c->abu_cells == (size_t)c->G.CELLS))
        return fail(c, SOC_ERR_STATE, "%s: %d scattering functions (WITH_MSF) need soc_set_abundances with %d species and this frequency's soc_set_optical_abu",
                    who, c->msf_ndust, c->msf_ndust);
    if (BATCH < 0) return fail(c, SOC_ERR_ARG, "%s: BATCH=%d", who, BATCH);
    if (GLOBAL < 1 || gid_first < 0 || gid_count < 0 || (int64_t)gid_first + gid_count > GLOBAL)
        return fail(c, SOC_ERR_ARG, "%s: work-item range [%d,+%d) outside GLOBAL=%d", who, gid_first, gid_count, GLOBAL);
    return SOC_OK;
}

static void fill_sim(soc_ctx *c, SocSim &S, SocVariant &V, int SOURCE, int BATCH, float SEED, float BG, float TW,
                     int GLOBAL, int gid_first, int gid_count)
{
    memset(&S, 0, sizeof S);
    S.SOURCE = SOURCE; S.BATCH = BATCH; S.GLOBAL = GLOBAL;
    S.PS_METHOD = c->ps_method; S.BINS = c->BINS; S.USE_EMWEIGHT = c->use_emweight; S.MIRROR = c->mirror;
    S.gid0 = (uint32_t)gid_first; S.gid_count = (uint32_t)gid_count;
    S.seed_mul = soc_seed_mul(SEED); S.seed_tab = c->dSeedTab;
    S.ABS = c->ABS; S.SCA = c->SCA; S.BG = BG; S.TW = TW;
    S.CSC = c->dCSC; S.OPT = c->dOPT;
    S.EMIT = c->dEMIT; S.EMWEI = c->dEMWEI;
    S.EMINDEX = c->dEMINDEX; S.XAB = nullptr;
    S.HPBG = c->dHPBG; S.HPBGP = c->dHPBGP; S.HPBG_WEIGHTED = c->hpbg_weighted ? 1 : 0;
    S.TABS = c->dTABS; S.INT = c->dINT;
    S.stats = c->dStats;
    S.STEP_WEIGHT = c->step_weight;  S.SW_A = c->sw_a;  S.SW_B = c->sw_b;
    S.INTV = (c->with_int == 2) ? c->dINTV : nullptr;  S.CELLS = c->G.CELLS;
    S.NDUST = c->msf_ndust;
    if (c->msf_ndust > 1) { S.MSF_SCA = c->dAF + c->msf_ndust;  S.ABU = c->dABU; }
    // with_int 0, 1, or 2: INT and the vector sums (the brick-local sweep and the direct kernels)
    V = soc_grid_variant(c->G, c->dOPT != nullptr, c->with_int);
}

// Point sources of one launch -> device.  xps_as_float: the scattered-light kernels declare
// XPS_NSIDE and XPS_SIDE as "__global float *" (kernel_ASOC_sca.c:495-496, :1486-1487) while
// ASOCS.py uploads the int32 arrays of AnalyseExternalPointSources (ASOCS.py:267-268), so the
// reference reads the integer bit patterns as floats: floor(u*asfloat(nside)*0.999999f) and
// (int)asfloat(side).  The values the reference kernel ends up with are computed here.
static int upload_sources(soc_ctx *c, const char *who, SocSim &S, const float *PSPOS, const float *PS, int NO_PS,
                          const int32_t *XPS_NSIDE, const int32_t *XPS_SIDE, const float *XPS_AREA, bool xps_as_float, int slot = 0)
{
    if (NO_PS < 1 || !PSPOS || !PS) return fail(c, SOC_ERR_ARG, "%s: point sources need PSPOS, PS and NO_PS>=1", who);
    if ((c->ps_method == 2 || c->ps_method == 5) && (!XPS_NSIDE || !XPS_SIDE || !XPS_AREA))
        return fail(c, SOC_ERR_ARG, "%s: PS_METHOD %d needs XPS_NSIDE/XPS_SIDE/XPS_AREA", who, c->ps_method);
    std::vector<int32_t> nside((size_t)NO_PS, 0), side((size_t)3 * NO_PS, 0);
    if (XPS_NSIDE) nside.assign(XPS_NSIDE, XPS_NSIDE + NO_PS);
    if (XPS_SIDE)  side.assign(XPS_SIDE, XPS_SIDE + 3 * NO_PS);
    if (c->ps_method == 2) {
        for (int i = 0; i < NO_PS; i++) {
            if (nside[i] < 0 || nside[i] > 3) return fail(c, SOC_ERR_ARG, "%s: XPS_NSIDE[%d]=%d", who, i, nside[i]);
            for (int k = 0; k < 3; k++)
                if (side[3 * i + k] < 0 || side[3 * i + k] > 5) return fail(c, SOC_ERR_ARG, "%s: XPS_SIDE[%d]=%d", who, 3 * i + k, side[3 * i + k]);
        }
    }
    if (xps_as_float) {
        // 0 <= v <= 5 as a float bit pattern is a denormal: u*v*0.999999f < 1 and (int)v == 0
        for (auto &v : nside) { float f;  memcpy(&f, &v, 4);  v = (f * 0.999999f < 1.0f) ? 0 : (int32_t)f; }
        for (auto &v : side)  { float f;  memcpy(&f, &v, 4);  v = (int32_t)f; }
    }
    // the slot holds PSPOS [NO_PS] float4 | PS [NO_PS] | XPS_NSIDE [NO_PS] | XPS_SIDE [3 NO_PS] | XPS_AREA [3 NO_PS]
    const size_t n = (size_t)NO_PS;
    char *p = nullptr;
    int r = slot_buf(c, soc_ctx::SLOT_SRC, slot, 48 * n, &p);
    if (r) return r;
    float4 *pspos = (float4 *)p;
    float  *ps = (float *)(p + 16 * n), *area = (float *)(p + 36 * n);
    int    *xnside = (int *)(p + 20 * n), *xside = (int *)(p + 24 * n);
    HIPCHK(c, hipMemcpyAsync(pspos, PSPOS, n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ps, PS, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(xnside, nside.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(xside, side.data(), n * 12, hipMemcpyHostToDevice, c->stream));
    if (XPS_AREA)  HIPCHK(c, hipMemcpyAsync(area, XPS_AREA, n * 12, hipMemcpyHostToDevice, c->stream));
    else           HIPCHK(c, hipMemsetAsync(area, 0, n * 12, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.NO_PS = NO_PS;
    S.PSPOS = pspos; S.PS = ps;
    S.XPS_NSIDE = xnside; S.XPS_SIDE = xside; S.XPS_AREA = area;
    return SOC_OK;
}

#define SOC_OPT_SLOTS 16        // per-cell opacity arrays per sweep (8 B per cell each, in one buffer): one per launch, or -- brick-local
                                // hierarchies, where launches share them -- one per soc_set_opt / soc_set_optical_abu call

static bool int_slots(const soc_ctx *c) { return c->int_mode == soc_ctx::INT_PER_LAUNCH || c->int_mode == soc_ctx::INT_PER_GROUP; }

// INT slot modes: the next launch of the batch with an INT tally -- deferred or not -- tallies INT into the current group's slot, or
// into a new, zeroed one (a scattered-light launch tallies nothing but its image: no S.INT)
static int take_int_slot(soc_ctx *c, const char *who, SocSim &S)
{
    if (!(c->batching && int_slots(c) && c->with_int && S.INT)) return SOC_OK;
    if (c->int_mode == soc_ctx::INT_PER_GROUP && c->int_group_open) {     // a further launch of the current group: the group's tally
        S.INT = (float *)c->slots[soc_ctx::SLOT_INT][c->int_slots_done - 1].p;
        return SOC_OK;
    }
    if (c->int_slots_done >= c->batch_max)
        return fail(c, SOC_ERR_STATE, "%s: %d launches of this batch hold an INT tally; soc_batch_end and soc_batch_read_int first", who, c->batch_max);
    const size_t cells = (size_t)c->G.CELLS;
    int r = slot_buf(c, soc_ctx::SLOT_INT, c->int_slots_done, cells * 4, &S.INT);
    if (r) return r;
    c->int_group_open = true;
    HIPCHK(c, hipMemsetAsync(S.INT, 0, cells * 4, c->stream));
    c->int_slots_done++;
    return SOC_OK;
}

// What a deferred launch keeps in its slot besides its SocSim and its kind's own inputs (route_sim's slot_inputs): the scattering
// table, a scattered-light launch's discrete scattering function and, with abundances, the per-cell opacities (the caller overwrites
// them for the next frequency)
static int keep_inputs(soc_ctx *c, SocSim &S, const SocVariant &V, int slot)
{
    float *csc = nullptr, *dsc = nullptr;
    int r = slot_copy(c, soc_ctx::SLOT_CSC, slot, &csc, c->dCSC, c->BINS);
    if (!r && S.DSC) r = slot_copy(c, soc_ctx::SLOT_DSC, slot, &dsc, c->have_dsc ? c->dDSC : nullptr, c->BINS);
    if (r) return r;
    S.CSC = csc;
    if (S.DSC) S.DSC = dsc;
    if (V.abu) {                                            // the per-cell opacities: a slot of one buffer
        // The Cartesian sweep and the sweep of a hierarchy in global memory address OPT as launch x stride: launch `slot` keeps its copy in
        // slot `slot`.  The brick-local form takes every launch's array by its pointer, and launches with ONE array share their brick
        // queues: there the launches deferred since the last soc_set_opt / soc_set_optical_abu (opt_gen, as keep_emission does for EMIT)
        // share one copy -- the point-source, background and cell-emission launches of a frequency -- and the slots count arrays.
        const bool local = lt_capable(c, true);
        const bool shared = local && c->opt_used > 0 && c->opt_slot_gen == c->opt_gen;
        const int k = !local ? slot : shared ? c->opt_used - 1 : c->opt_used;
        if (k >= SOC_OPT_SLOTS) return fail(c, SOC_ERR_STATE, "a batch holds at most %d per-cell opacity arrays", SOC_OPT_SLOTS);
        const size_t cells = (size_t)c->G.CELLS;
        float2 *opt = nullptr;
        r = slot_buf(c, soc_ctx::SLOT_OPT, 0, SOC_OPT_SLOTS * cells * 8, &opt);
        if (r) return r;
        S.OPT = opt + (size_t)k * cells;
        if (!shared) HIPCHK(c, hipMemcpyAsync(opt + (size_t)k * cells, c->dOPT, cells * 8, hipMemcpyDeviceToDevice, c->stream));
        if (local && !shared) { c->opt_used = k + 1;  c->opt_slot_gen = c->opt_gen; }
    }
    return SOC_OK;
}

// slot_inputs of SimRAM_HP launches (absorption or scattered light): a deferred one keeps its own copy of the sky (the caller sets the
// next frequency's)
static int keep_sky(soc_ctx *c, SocSim &S, int slot)
{
    if (slot < 0) return SOC_OK;
    float *sky = nullptr;
    int r = slot_copy(c, soc_ctx::SLOT_HP, slot, &sky, c->dHPBG, SOC_HPBG_PIX, c->dHPBGP, SOC_HPBG_PIX);
    S.HPBG = sky;  S.HPBGP = sky + SOC_HPBG_PIX;
    return r;
}

// slot_inputs of cell-emission launches: a deferred one keeps its own copy of EMIT | EMWEI (the caller uploads the next frequency's);
// the copy of an earlier launch serves when soc_set_emission has not been called since
static int keep_emission(soc_ctx *c, SocSim &S, int slot)
{
    if (slot < 0) return SOC_OK;
    const size_t cells = (size_t)c->G.CELLS;
    if (!(c->emit_slot_last >= 0 && c->emit_slot_last < slot && c->emit_slot_gen == c->emit_gen)) {
        float *em = nullptr;
        int r = slot_copy(c, soc_ctx::SLOT_EMIT, slot, &em, c->dEMIT, cells, c->dEMWEI, cells);
        if (r) return r;
        c->emit_slot_last = slot;  c->emit_slot_gen = c->emit_gen;
    }
    const float *em = (const float *)c->slots[soc_ctx::SLOT_EMIT][c->emit_slot_last].p;
    S.EMIT = em;  S.EMWEI = em + cells;
    return SOC_OK;
}

// A sweep holds launches of one family: absorption, or scattered light (rays: brick-local hierarchies, where all kinds share one).  An
// absorption sweep runs one kernel variant: its launches are all SimRAM_PB, all _HP or all _CL ones, all with or all without per-cell
// opacities ... except on brick-local hierarchies, where the walk and the event workgroups take the kind from the launch: there the
// point-source, background, Healpix and cell-emission launches of a TABS-only run share one sweep
static bool same_sweep(const soc_ctx *c, const SocSim &S, bool abu)
{
    if (c->pending.empty()) return true;
    const SocSim &P = c->pending[0];
    if ((P.SCAKIND != 0) != (S.SCAKIND != 0) || (P.OPT != nullptr) != abu) return false;
    // (brick-local hierarchies: the kinds share sweeps, also with per-group INT tallies; rays on single-level grids: one kernel for every kind)
    return soc_source_kind(P.SOURCE) == soc_source_kind(S.SOURCE) || lt_capable(c, abu) || (S.SCAKIND != 0 && cart_capable(c));
}

// The kinds of launch and what sets them apart on the way to a kernel (use_sweep, route_sim)
enum SimKind { SIM_PB, SIM_HP, SIM_CL, SCA_PB, SCA_CL, SCA_PS, SCA_HP };
static const struct {
    const char *who;
    int         scakind;                // SocSim::SCAKIND: SOC_SCA_* + 1 for the scattered-light kernels (run as rays); 0 absorption
    long long   min_items;              // absorption, automatic mode: work items from which the brick sweep pays
    const char *not_applicable;         // absorption: what keeps soc_set_exec(1) from the brick sweep
} sim_kinds[] = {
    { "soc_sim_pb", 0, 65536,  "mirror, with_int 2, roisave/roiload off brick-local hierarchies (Index() in float: those need soc_set_tuning float_local; per-cell opacities: soc_set_tuning abu_local, Index() in double and no with_int 2), > 15 levels or > 2^18 bricks" },
    { "soc_sim_hp", 0, 65536,  "mirror, with_int 2 off brick-local hierarchies (Index() in float: those need soc_set_tuning float_local; per-cell opacities: soc_set_tuning abu_local, Index() in double and no with_int 2), > 15 levels or > 2^18 bricks" },
    { "soc_sim_cl", 0, 262144, "mirror, with_int 2, ALI, roisave off brick-local hierarchies (Index() in float: those need soc_set_tuning float_local; per-cell opacities: soc_set_tuning abu_local, Index() in double and neither with_int 2 nor ALI), USE_EMWEIGHT 2, > 15 levels or > 2^18 bricks" },
    { "soc_sca_sim_pb", SOC_SCA_PB + 1, 0, nullptr },
    { "soc_sca_sim_cl", SOC_SCA_CL + 1, 0, nullptr },
    { "soc_sca_sim_ps", SOC_SCA_PS + 1, 0, nullptr },
    { "soc_sca_sim_hp", SOC_SCA_HP + 1, 0, nullptr },
};

// Whether a launch goes to a sweep: the brick sweep, or for scattered light the sweep of rays on brick-local hierarchies (soc_brick.hip:
// soc_sca_events), which takes flat and Healpix images and every kind of launch (the kind only changes the event lane) with scalar
// opacities and one scattering function.  *why: what keeps soc_set_exec(1) from it, nullptr when nothing does.  batch: the open batch
// takes the launch.  Automatic mode also asks for enough work items to fill the chip.  Absorption counts the launch's (items).
// Hierarchies: the brick sweep pays from two launches per sweep on (256^3 roots, 4 levels: 1.9e10 steps/s with one launch, 2.8e10 with
// two, 4.4e10 with eight; direct kernel 2.0e10), so there only launches of a batch use it (see flush_pending) -- and, on brick-local
// hierarchies, a lone launch with enough work items.  Rays: the launches of a batch are deferred and flush_pending counts those of their
// sweep; a lone launch counts its own.
static bool use_sweep(const soc_ctx *c, SimKind kind, const SocVariant &V, long long items, bool batch, const char **why)
{
    if (sim_kinds[kind].scakind) {
        *why = (!c->have_view || c->view.NDIR == 0) ? "no view"
             : (c->msf_ndust > 1) ? "several scattering functions (WITH_MSF) need the direct kernel"
             : (c->dOPT != nullptr) ? "per-cell opacities need the direct kernel"
             : !(lt_capable(c, false) || cart_capable(c))
                   ? "the grid is not one the sweep of rays takes (a hierarchy of 2-8 levels with Index() in double -- in float: with soc_set_tuning float_local --, or a single-level grid below 4096 cells per edge)"
             : nullptr;
        if (cart_capable(c))                                // (the launches of a batch are deferred where a batch can pay; flush_pending counts them)
            return c->exec_mode != 0 && !*why && (c->exec_mode == 1 || (batch ? cart_rays_pay(c, SOC_CART_RAYS_BATCH, true) : cart_rays_pay(c, items, false)));
        return c->exec_mode != 0 && !*why && (c->exec_mode == 1 || batch || items >= SOC_SCA_RAYS_LAUNCH);
    }
    const bool lt = lt_capable(c, V.abu != 0);
    const int B = 1 << c->brick_log2;
    const long long nb = (long long)((c->G.NX + B - 1) / B) * ((c->G.NY + B - 1) / B) * ((c->G.NZ + B - 1) / B);
    // the brick sweep applies: mirror, with_int 2 and region-of-interest records need the brick-local sweep (packets of a loaded
    // record, SOURCE 3: any sweep); cell emission also needs USE_EMWEIGHT 0/1 and, with ALI, the brick-local sweep without with_int 2
    const bool ok = nb <= (1 << 18) && c->G.LEVELS <= 15
                    && (c->mirror == 0 || lt) && (c->with_int != 2 || lt)
                    && (kind == SIM_HP || !c->roi.save || (lt && c->mirror == 0))
                    && (kind != SIM_CL || (c->use_emweight != 2 && (!c->with_ali || (lt && c->with_int != 2))));
    *why = ok ? nullptr : sim_kinds[kind].not_applicable;
    return c->exec_mode != 0 && ok
           && (c->exec_mode == 1 || (items >= sim_kinds[kind].min_items && nb >= 8 && (!V.octree || batch || (lt && items >= SOC_LT_LONE_LAUNCH))));
}

// Route a launch, after the checks of its soc_sim_* or soc_sca_sim_* call and fill_sim: a sweep or the direct kernel, now or deferred
// into the open batch.  items: the work items the thresholds count.  slot_inputs(slot) stores the kind's own inputs of the launch:
// slot >= 0 the launch is deferred and keeps them in that slot, -1 it runs now.
static int route_sim(soc_ctx *c, SimKind kind, SocSim &S, const SocVariant &V, long long items, const std::function<int(int)> &slot_inputs)
{
    const char *who = sim_kinds[kind].who;
    // the open batch takes the launch with its INT tally (soc_batch_begin: only launches without one)
    const bool batch = c->batching && (!V.wint || c->int_mode != soc_ctx::INT_OFF);
    const char *why = nullptr;
    const bool sweep = use_sweep(c, kind, V, items, batch, &why);
    if (c->exec_mode == 1 && !sweep) {
        if (S.SCAKIND) {
            c->last.passes = 0;                             // (a refused scattered-light launch reports no sweep)
            return fail(c, SOC_ERR_ARG, "%s: brick sweep requested but not applicable: %s", who, why);
        }
        return fail(c, SOC_ERR_ARG, "%s: brick sweep requested but not applicable (%s)", who, why);
    }
    // inside soc_batch_begin/end a launch that goes to a sweep is deferred: its per-launch inputs are kept in its slot and it runs with
    // the others.  Not with_int 2 in the INT slot modes; not WITH_MSF (per-species tables are not kept)
    const bool defer = batch && sweep && !(int_slots(c) && V.wint == 2) && c->msf_ndust <= 1;
    if (!defer || !same_sweep(c, S, V.abu != 0)) FLUSH(c);
    // (brick-local hierarchies: the launch would bring the sweep's 17th opacity array, see keep_inputs)
    const bool abu_shared = V.abu && lt_capable(c, true);
    if (defer && abu_shared && c->opt_used >= SOC_OPT_SLOTS && c->opt_slot_gen != c->opt_gen) FLUSH(c);
    int r = take_int_slot(c, who, S);
    if (r) return r;
    const int slot = defer ? (int)c->pending.size() : -1;
    r = slot_inputs(slot);
    if (r) return r;
    c->last.passes = 0;
    if (defer) {
        r = keep_inputs(c, S, V, slot);
        if (r) return r;
        c->pending.push_back(S);
        // a sweep's worth of launches (with INT tallies per launch or group, take_int_slot holds the batch to batch_max)
        const int full = (int_slots(c) && S.INT) ? SOC_MAXLAUNCH : (V.abu && !abu_shared) ? std::min(c->batch_max, SOC_OPT_SLOTS) : c->batch_max;
        if ((int)c->pending.size() >= full) FLUSH(c);
        return SOC_OK;
    }
    if (!sweep) return run_direct(c, S, V);
    hipError_t e = soc_brick_run_pb(*c->sweep, c->G, &S, 1, V, c->brick_log2, c->tune, c->stream, &c->last, S.SCAKIND ? &c->view : nullptr);
    if (e == hipErrorNotSupported && S.SCAKIND && c->exec_mode != 1)
        return run_direct(c, S, V);                         // rays: the direct kernel where the sweep does not apply after all
    if (e != hipSuccess) return fail(c, SOC_ERR_HIP, "%s: brick sweep failed: %s", who, hipGetErrorString(e));
    return SOC_OK;
}

int soc_sim_pb(soc_ctx *c, int SOURCE, int PACKETS, int BATCH, float SEED, float BG, float TW,
               const float *PSPOS, const float *PS, int NO_PS,
               const int32_t *XPS_NSIDE, const int32_t *XPS_SIDE, const float *XPS_AREA,
               int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sim_pb", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (SOURCE != 0 && SOURCE != 1 && SOURCE != 3)
        return fail(c, SOC_ERR_ARG, "soc_sim_pb: SOURCE=%d (0 point sources, 1 background, 3 packets of soc_set_roi_load)", SOURCE);
    if (SOURCE == 3) {
        if (!c->roi.load) return fail(c, SOC_ERR_STATE, "soc_sim_pb: SOURCE 3 needs soc_set_roi_load");
        const int npix = 12 * c->roi.NSIDE * c->roi.NSIDE;
        if (PACKETS != c->roi.NELEM) return fail(c, SOC_ERR_ARG, "soc_sim_pb: SOURCE 3 takes PACKETS = %d surface elements, got %d", c->roi.NELEM, PACKETS);
        if (BATCH % npix) return fail(c, SOC_ERR_ARG, "soc_sim_pb: SOURCE 3 takes BATCH = a multiple of the %d Healpix pixels, got %d", npix, BATCH);
    }
    HIPCHK(c, hipSetDevice(c->device));
    SocSim S;
    SocVariant V;
    fill_sim(c, S, V, SOURCE, BATCH, SEED, BG, TW, GLOBAL, gid_first, gid_count);
    S.NO_PS = 1;
    S.ROI = (c->roi.save || c->roi.load) ? c->dRoi : nullptr;
    S.ROISAVE = c->roi.save;
    S.ROILOAD = c->roi.load ? c->roi.NELEM : 0;
    return route_sim(c, SIM_PB, S, V, gid_count, [&](int slot) {      // the point sources, in the launch's slot of the source buffers
        return SOURCE == 0 ? upload_sources(c, "soc_sim_pb", S, PSPOS, PS, NO_PS, XPS_NSIDE, XPS_SIDE, XPS_AREA, false, slot < 0 ? 0 : slot) : SOC_OK;
    });
}

#define SOC_MAX_SPLIT_DEFAULT 4300      // ASOC_aux.py:54

// What the two split launches share: the checks on max_split and on what neither kernel has a branch for, the ray stacks (a tile of
// max_split x 10 x 64 words per wave of the range, kept for the handle) and the counters.  max_split <= 0 becomes the default.
static int split_prepare(soc_ctx *c, const char *who, int &max_split, int gid_count)
{
    if (max_split <= 0) max_split = SOC_MAX_SPLIT_DEFAULT;
    if (max_split < 14)
        return fail(c, SOC_ERR_ARG, "%s: max_split %d (at least 14: a split adds 4 entries above the NBUF > MAX_SPLIT-10 test)", who, max_split);
    // what SimBgSplit and SimHpSplit have no branch for (kernel_ASOC.c:2117-3550: no Mirror(), no STEP_WEIGHT, no ROI arguments)
    if (c->mirror) return fail(c, SOC_ERR_STATE, "%s: reflecting faces (mirror mask %d) are not part of the split kernel", who, c->mirror);
    if (c->step_weight) return fail(c, SOC_ERR_STATE, "%s: weighted free paths (step weight mode %d) are not part of the split kernel", who, c->step_weight);
    if (c->roi.save) return fail(c, SOC_ERR_STATE, "%s: a region-of-interest record (roi save) is not part of the split kernel", who);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t waves = ((size_t)gid_count + 63) / 64, words = waves * (size_t)max_split * 640;
    if ((double)waves * (double)max_split * 640.0 > (double)c->dSplitStack.n) {
        size_t mfree = 0, mtotal = 0;
        HIPCHK(c, hipMemGetInfo(&mfree, &mtotal));
        const size_t held = c->dSplitStack.owned ? c->dSplitStack.bytes() : 0;
        if ((double)waves * (double)max_split * 2560.0 > (double)(mfree + held))      // (in double: the product can pass 2^64)
            return fail(c, SOC_ERR_ARG, "%s: the ray stacks of %d work items x max_split %d need %.3f GB of device memory, %.3f GB are free",
                        who, gid_count, max_split, (double)waves * (double)max_split * 2560.0e-9, (double)(mfree + held) * 1e-9);
        FLUSH(c);
        hipError_t e = c->dSplitStack.reserve(words, c->stream);
        if (e != hipSuccess)
            return fail(c, SOC_ERR_HIP, "%s: allocating %.3f GB for the ray stacks failed: %s", who, (double)words * 4e-9, hipGetErrorString(e));
    }
    if (!c->dSplitStats) {
        HIPCHK(c, c->dSplitStats.reserve(8, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dSplitStats, 0, 8 * sizeof(unsigned long long), c->stream));
    }
    return SOC_OK;
}

int soc_sim_bg_split(soc_ctx *c, int PACKETS, int BATCH, float SEED, float BG, float TW, int SELEM, int max_split,
                     int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sim_bg_split", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (max_split > 0 && max_split < 14)
        return fail(c, SOC_ERR_ARG, "soc_sim_bg_split: max_split %d (at least 14: a split adds 4 entries above the NBUF > MAX_SPLIT-10 test)", max_split);
    if (SELEM < 1) return fail(c, SOC_ERR_ARG, "soc_sim_bg_split: SELEM %d (surface elements per work item, >= 1)", SELEM);
    if ((int64_t)SELEM * GLOBAL > 2147483647LL) return fail(c, SOC_ERR_ARG, "soc_sim_bg_split: SELEM %d x GLOBAL %d exceeds int32", SELEM, GLOBAL);
    r = split_prepare(c, "soc_sim_bg_split", max_split, gid_count);
    if (r) return r;
    SocSim S;
    SocVariant V;
    fill_sim(c, S, V, 1, BATCH, SEED, BG, TW, GLOBAL, gid_first, gid_count);
    S.NO_PS = 1;
    FLUSH(c);                                               // a launch that no sweep takes: after what the batch deferred before it
    r = take_int_slot(c, "soc_sim_bg_split", S);
    if (r) return r;
    c->last.passes = 0;
    SocSplit P;
    P.SELEM = SELEM;  P.max_split = max_split;  P.stack = c->dSplitStack;  P.counters = c->dSplitStats;
    HIPCHK(c, soc_launch_sim_bg_split(c->G, S, P, V, c->stream));
    if (gid_count > 0) c->last.variant = soc_split_variant_code(0, V);      // (as run_direct: a launch without work items ran nothing)
    return SOC_OK;
}

int soc_sim_hp_split(soc_ctx *c, int PACKETS, int BATCH, float SEED, float TW, int max_split, int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sim_hp_split", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (!c->have_hpbg) return fail(c, SOC_ERR_STATE, "soc_sim_hp_split: call soc_set_hpbg first");
    r = split_prepare(c, "soc_sim_hp_split", max_split, gid_count);
    if (r) return r;
    SocSim S;
    SocVariant V;
    fill_sim(c, S, V, 1, BATCH, SEED, 0.0f, TW, GLOBAL, gid_first, gid_count);
    S.NO_PS = 1;
    // Not deferred, so the kernel reads the handle's own sky, the one current at this call.  A following soc_set_hpbg cannot overtake
    // it: its copies are issued on this stream, behind the kernel, and it synchronises the stream before it returns.
    FLUSH(c);
    r = take_int_slot(c, "soc_sim_hp_split", S);
    if (r) return r;
    c->last.passes = 0;
    SocSplit P;
    P.SELEM = 1;  P.max_split = max_split;  P.stack = c->dSplitStack;  P.counters = c->dSplitStats;
    HIPCHK(c, soc_launch_sim_hp_split(c->G, S, P, V, c->stream));
    if (gid_count > 0) c->last.variant = soc_split_variant_code(1, V);
    return SOC_OK;
}

int soc_split_stats(soc_ctx *c, uint64_t out[6], int reset)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    unsigned long long h[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (c->dSplitStats) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(h, c->dSplitStats, sizeof h, hipMemcpyDeviceToHost));
        if (reset) HIPCHK(c, hipMemsetAsync(c->dSplitStats, 0, sizeof h, c->stream));
    }
    if (out) for (int i = 0; i < 6; i++) out[i] = h[i];
    c->split_depth = h[6];
    c->split_skipped = h[7];
    return SOC_OK;
}

int64_t soc_split_max_depth(soc_ctx *c) { return c ? (int64_t)c->split_depth : -1; }
int64_t soc_split_skipped(soc_ctx *c) { return c ? (int64_t)c->split_skipped : -1; }

static int batch_begin(soc_ctx *c, int max_launches, soc_ctx::IntMode int_mode)
{
    if (!c) return SOC_ERR_ARG;
    if (max_launches < 0 || max_launches > SOC_MAXLAUNCH)
        return fail(c, SOC_ERR_ARG, "soc_batch_begin: max_launches %d (1..%d, 0 = default)", max_launches, SOC_MAXLAUNCH);
    FLUSH(c);
    c->batching = true;
    c->int_mode = int_mode;
    c->int_group_open = false;
    c->int_slots_done = 0;
    // default: as many as one sweep takes (the packets in flight are limited separately, see flush_pending)
    c->batch_max = max_launches ? max_launches : SOC_MAXLAUNCH;
    return SOC_OK;
}

int soc_batch_begin(soc_ctx *c, int max_launches) { return batch_begin(c, max_launches, soc_ctx::INT_OFF); }
int soc_batch_begin_shared_int(soc_ctx *c, int max_launches) { return batch_begin(c, max_launches, soc_ctx::INT_SHARED); }
int soc_batch_begin_int(soc_ctx *c, int max_launches) { return batch_begin(c, max_launches, soc_ctx::INT_PER_LAUNCH); }
int soc_batch_begin_int_groups(soc_ctx *c, int max_groups) { return batch_begin(c, max_groups, soc_ctx::INT_PER_GROUP); }

int soc_batch_next_int(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    if (!(c->batching && c->int_mode == soc_ctx::INT_PER_GROUP)) return fail(c, SOC_ERR_STATE, "soc_batch_next_int: call soc_batch_begin_int_groups first");
    c->int_group_open = false;                               // the next launch takes a new, zeroed INT tally
    return SOC_OK;
}

int soc_batch_read_int(soc_ctx *c, int k, float *out, long n)
{
    if (!c) return SOC_ERR_ARG;
    if (c->batching || !c->pending.empty()) return fail(c, SOC_ERR_STATE, "soc_batch_read_int: call soc_batch_end first");
    if (k < 0 || k >= c->int_slots_done) return fail(c, SOC_ERR_ARG, "soc_batch_read_int: launch %d of %d deferred with the INT tally", k, c->int_slots_done);
    if (!out || n != (long)c->G.CELLS) return fail(c, SOC_ERR_ARG, "soc_batch_read_int: the tally has %d cells, buffer %ld", c->G.CELLS, n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->slots[soc_ctx::SLOT_INT][k].p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_batch_end(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    c->batching = false;
    FLUSH(c);
    return SOC_OK;
}

int soc_set_hpbg(soc_ctx *c, const float *BG, const float *HPBGP)
{
    if (!c) return SOC_ERR_ARG;
    // no flush: a deferred SimRAM_HP launch keeps its own copy of the sky (soc_sim_hp)
    if (!BG) return fail(c, SOC_ERR_ARG, "soc_set_hpbg: BG is NULL");
    const int NPIX = SOC_HPBG_PIX;
    for (int i = 0; i < NPIX; i++)
        if (!std::isfinite(BG[i])) return fail(c, SOC_ERR_ARG, "soc_set_hpbg: BG[%d] is not finite", i);
    if (HPBGP) {
        // the pixel search relies on a non-decreasing table that ends above every random number (ASOC.py:1208)
        for (int i = 1; i < NPIX; i++)
            if (!(HPBGP[i] >= HPBGP[i - 1])) return fail(c, SOC_ERR_ARG, "soc_set_hpbg: HPBGP decreases at pixel %d", i);
        if (!(HPBGP[NPIX - 1] >= 1.0f)) return fail(c, SOC_ERR_ARG, "soc_set_hpbg: HPBGP[last]=%g must be >= 1", (double)HPBGP[NPIX - 1]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->dHPBG) {
        HIPCHK(c, c->dHPBG.reset((size_t)NPIX, c->stream));
        HIPCHK(c, c->dHPBGP.reset((size_t)NPIX, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->dHPBG, BG, (size_t)NPIX * 4, hipMemcpyHostToDevice, c->stream));
    if (HPBGP) HIPCHK(c, hipMemcpyAsync(c->dHPBGP, HPBGP, (size_t)NPIX * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_hpbg = true;
    c->hpbg_weighted = (HPBGP != nullptr);
    return SOC_OK;
}

// ---- region of interest (roi / roisave / roiload keys) ----

static int roi_upload(soc_ctx *c)
{
    HIPCHK(c, c->dRoi.reserve(1, c->stream));
    c->roi.SAVE = c->dRoiSave;
    c->roi.LOAD = c->dRoiLoad;
    HIPCHK(c, hipMemcpyAsync(c->dRoi, &c->roi, sizeof(SocRoi), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_set_roi_save(soc_ctx *c, const int32_t *ROI, int ROI_STEP, int ROI_NSIDE)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (!ROI) {                                             // off
        c->roi.save = 0;
        return roi_upload(c);
    }
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_set_roi_save: call soc_set_grid first");
    const int lim[3] = { c->G.NX, c->G.NY, c->G.NZ };
    for (int a = 0; a < 3; a++)
        if (ROI[2 * a] < 0 || ROI[2 * a + 1] < ROI[2 * a] || ROI[2 * a + 1] >= lim[a])
            return fail(c, SOC_ERR_ARG, "soc_set_roi_save: ROI[%d..%d] = %d..%d outside the %d root cells of that axis", 2 * a, 2 * a + 1, ROI[2 * a], ROI[2 * a + 1], lim[a]);
    if (ROI_STEP < 1 || ROI_NSIDE < 1 || ROI_NSIDE > 1024) return fail(c, SOC_ERR_ARG, "soc_set_roi_save: ROI_STEP %d, ROI_NSIDE %d", ROI_STEP, ROI_NSIDE);
    if (c->roi.load && c->roi.NSIDE != ROI_NSIDE)
        return fail(c, SOC_ERR_ARG, "soc_set_roi_save: ROI_NSIDE %d differs from the loaded record's %d (one -D ROI_NSIDE in the reference)", ROI_NSIDE, c->roi.NSIDE);
    const int64_t n[3] = { (int64_t)(ROI[1] - ROI[0] + 1) * ROI_STEP, (int64_t)(ROI[3] - ROI[2] + 1) * ROI_STEP, (int64_t)(ROI[5] - ROI[4] + 1) * ROI_STEP };
    const int64_t total = (n[0] * n[1] + n[1] * n[2] + n[2] * n[0]) * 12 * ROI_NSIDE * ROI_NSIDE;
    if (total > 2147483647LL) return fail(c, SOC_ERR_ARG, "soc_set_roi_save: %lld record entries (int32 indices in the kernel)", (long long)total);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->dRoiSave.reset((size_t)total, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dRoiSave, 0, (size_t)total * 4, c->stream));
    for (int i = 0; i < 6; i++) c->roi.ROI[i] = ROI[i];
    c->roi.STEP = ROI_STEP;  c->roi.NSIDE = ROI_NSIDE;  c->roi.save = 1;
    return roi_upload(c);
}

int soc_roi_zero(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->roi.save) return fail(c, SOC_ERR_STATE, "soc_roi_zero: call soc_set_roi_save first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->dRoiSave, 0, c->dRoiSave.n * 4, c->stream));
    return SOC_OK;
}

int soc_roi_read(soc_ctx *c, float *out, long n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->roi.save) return fail(c, SOC_ERR_STATE, "soc_roi_read: call soc_set_roi_save first");
    if (!out || n != (long)c->dRoiSave.n) return fail(c, SOC_ERR_ARG, "soc_roi_read: the record has %zu entries, buffer %ld", c->dRoiSave.n, n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->dRoiSave, c->dRoiSave.n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_set_roi_load(soc_ctx *c, const int32_t *DIM, int ROI_NSIDE, const float *LOAD)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (!LOAD) {                                            // off
        c->roi.load = 0;
        return roi_upload(c);
    }
    if (!DIM || DIM[0] < 1 || DIM[1] < 1 || DIM[2] < 1 || ROI_NSIDE < 1 || ROI_NSIDE > 1024)
        return fail(c, SOC_ERR_ARG, "soc_set_roi_load: DIM / ROI_NSIDE");
    if (c->roi.save && c->roi.NSIDE != ROI_NSIDE)
        return fail(c, SOC_ERR_ARG, "soc_set_roi_load: ROI_NSIDE %d differs from the saved record's %d (one -D ROI_NSIDE in the reference)", ROI_NSIDE, c->roi.NSIDE);
    const int64_t nelem = (int64_t)DIM[0] * DIM[1] + (int64_t)DIM[1] * DIM[2] + (int64_t)DIM[2] * DIM[0];
    const int64_t total = nelem * 12 * ROI_NSIDE * ROI_NSIDE;
    if (nelem > 21474836LL || total > 2147483647LL) return fail(c, SOC_ERR_ARG, "soc_set_roi_load: %lld surface elements", (long long)nelem);
    for (int64_t i = 0; i < total; i++)
        if (!std::isfinite(LOAD[i])) return fail(c, SOC_ERR_ARG, "soc_set_roi_load: LOAD[%lld] is not finite", (long long)i);
    HIPCHK(c, c->dRoiLoad.reserve((size_t)total, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dRoiLoad, LOAD, (size_t)total * 4, hipMemcpyHostToDevice, c->stream));
    for (int i = 0; i < 3; i++) c->roi.DIM[i] = DIM[i];
    c->roi.NELEM = (int)nelem;  c->roi.NSIDE = ROI_NSIDE;  c->roi.load = 1;
    return roi_upload(c);
}

int soc_sim_hp(soc_ctx *c, int PACKETS, int BATCH, float SEED, float TW, int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sim_hp", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (!c->have_hpbg) return fail(c, SOC_ERR_STATE, "soc_sim_hp: call soc_set_hpbg first");
    HIPCHK(c, hipSetDevice(c->device));
    SocSim S;
    SocVariant V;
    fill_sim(c, S, V, 1, BATCH, SEED, 0.0f, TW, GLOBAL, gid_first, gid_count);
    S.NO_PS = 1;
    S.SOURCE = SOC_SOURCE_HP;          // the brick sweep as for soc_sim_pb: the walk is SimRAM_PB's, only the creation of a packet differs
    return route_sim(c, SIM_HP, S, V, gid_count, [&](int slot) { return keep_sky(c, S, slot); });
}

int soc_sim_cl(soc_ctx *c, int SOURCE, int PACKETS, int BATCH, float SEED, float TW,
               int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sim_cl", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (!c->have_emit) return fail(c, SOC_ERR_STATE, "soc_sim_cl: call soc_set_emission first");
    HIPCHK(c, hipSetDevice(c->device));
    SocSim S;
    SocVariant V;
    fill_sim(c, S, V, SOURCE, BATCH, SEED, 0.0f, TW, GLOBAL, gid_first, gid_count);
    S.NO_PS = 1;
    if (c->use_emweight == 2 && !c->have_emindex) return fail(c, SOC_ERR_STATE, "soc_sim_cl: USE_EMWEIGHT 2 needs soc_set_emindex");
    if (c->with_ali) S.XAB = c->dXAB;
    S.ROI = c->roi.save ? c->dRoi : nullptr;                // SimRAM_CL records too (kernel_ASOC.c:1250-1254)
    S.ROISAVE = c->roi.save;
    S.SOURCE = SOC_SOURCE_CL;
    // The brick sweep: the same walk, the event workgroups step through the work item's cells.  It needs packets in
    // flight to sort -- one per work item that has a cell, min(GLOBAL, CELLS): with the reference's GLOBAL = 32768
    // the direct kernel (1.5e10 steps/s at C2, the rate of the fabric atomics) stays; `global` in the ini file
    // raises it.  Host-listed cells (USE_EMWEIGHT 2), ALI and region-of-interest records: direct kernel.
    const long long inflight = std::min<long long>((long long)gid_first + gid_count, c->G.CELLS) - gid_first;
    return route_sim(c, SIM_CL, S, V, inflight, [&](int slot) { return keep_emission(c, S, slot); });
}

// ------------------------------------------------------------------------------------
// scattered-light images (ASOCS.py / kernel_ASOC_sca.c)
// ------------------------------------------------------------------------------------

// The image of a new view, npix values (the old one's: old): the library's own is made anew (zeroed) when the size changes; a
// caller-owned one stays bound only at the same size
static int view_image(soc_ctx *c, const char *who, size_t npix, size_t old)
{
    if (c->dOUT && npix == old) return SOC_OK;
    if (c->dOUT && !c->dOUT.owned) return fail(c, SOC_ERR_STATE, "%s: image size changed while a caller-owned image is bound", who);
    HIPCHK(c, c->dOUT.reset(npix, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dOUT, 0, npix * 4, c->stream));
    return SOC_OK;
}

int soc_sca_set_view(soc_ctx *c, int NDIR, const float *ODIR, const float *RA, const float *DE,
                     int NPIX_X, int NPIX_Y, float MAP_DX, const float *CENTRE, int FFS)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (NDIR < 1 || NDIR > 4096 || !ODIR || !RA || !DE || !CENTRE)
        return fail(c, SOC_ERR_ARG, "soc_sca_set_view: need 1 <= NDIR <= 4096 observer directions (Healpix output, NDIR<0, is not supported)");
    if (NPIX_X < 1 || NPIX_Y < 1 || (int64_t)NDIR * NPIX_X * NPIX_Y > 2147483647LL || !(MAP_DX > 0.0f))
        return fail(c, SOC_ERR_ARG, "soc_sca_set_view: NPIX %d x %d, MAP_DX %g", NPIX_X, NPIX_Y, (double)MAP_DX);
    for (int i = 0; i < NDIR; i++) {
        // GetStep divides by the components of the direction: the host makes them non-zero (ASOC_aux.py:1177-1181)
        for (int k = 0; k < 3; k++) {
            const float v = ODIR[4 * i + k];
            if (!(std::fabs(v) > 0.0f) || !std::isfinite(v))
                return fail(c, SOC_ERR_ARG, "soc_sca_set_view: ODIR[%d].%c = %g (must be finite and non-zero)", i, "xyz"[k], (double)v);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t npix = (size_t)NDIR * NPIX_X * NPIX_Y;
    const size_t old = view_pixels(c);
    if (NDIR != c->view.NDIR || !c->dODIR) {
        c->view.NDIR = 0;
        HIPCHK(c, c->dODIR.reset((size_t)NDIR, c->stream));
        HIPCHK(c, c->dORA.reset((size_t)NDIR, c->stream));
        HIPCHK(c, c->dODE.reset((size_t)NDIR, c->stream));
    }
    int r = view_image(c, "soc_sca_set_view", npix, old);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));            // launches in flight still read the previous view
    HIPCHK(c, hipMemcpy(c->dODIR, ODIR, (size_t)NDIR * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->dORA, RA, (size_t)NDIR * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->dODE, DE, (size_t)NDIR * 16, hipMemcpyHostToDevice));
    c->view.NDIR = NDIR;  c->view.NPIX_X = NPIX_X;  c->view.NPIX_Y = NPIX_Y;  c->view.FFS = FFS ? 1 : 0;
    c->view.MAP_DX = MAP_DX;  c->view.CX = CENTRE[0];  c->view.CY = CENTRE[1];  c->view.CZ = CENTRE[2];
    c->view.ODIRS = c->dODIR;  c->view.ORA = c->dORA;  c->view.ODE = c->dODE;
    c->have_view = true;
    c->out_slots = 0;                                        // (images of soc_sca_batch_images belonged to the old view)
    return SOC_OK;
}

int soc_sca_set_healpix(soc_ctx *c, int NSIDE, const float *OBSERVER, int FFS)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (NSIDE < 1 || NSIDE > 8192 || (NSIDE & (NSIDE - 1)) || !OBSERVER)
        return fail(c, SOC_ERR_ARG, "soc_sca_set_healpix: NSIDE %d (power of two up to 8192) and the observer position are needed", NSIDE);
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(OBSERVER[k])) return fail(c, SOC_ERR_ARG, "soc_sca_set_healpix: observer position is not finite");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t npix = (size_t)12 * NSIDE * NSIDE, old = view_pixels(c);
    if (!c->dODIR || c->view.NDIR < 1) {
        HIPCHK(c, c->dODIR.reset(1, c->stream));
        HIPCHK(c, c->dORA.reset(1, c->stream));
        HIPCHK(c, c->dODE.reset(1, c->stream));
    }
    int r = view_image(c, "soc_sca_set_healpix", npix, old);
    if (r) return r;
    const float obs[4] = { OBSERVER[0], OBSERVER[1], OBSERVER[2], 0.0f };
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->dODIR, obs, 16, hipMemcpyHostToDevice));
    c->view.NDIR = -NSIDE;  c->view.NPIX_X = 1;  c->view.NPIX_Y = 1;  c->view.FFS = FFS ? 1 : 0;
    c->view.MAP_DX = 1.0f;  c->view.CX = c->view.CY = c->view.CZ = 0.0f;
    c->view.ODIRS = c->dODIR;  c->view.ORA = c->dORA;  c->view.ODE = c->dODE;
    c->have_view = true;
    c->out_slots = 0;                                        // (images of soc_sca_batch_images belonged to the old view)
    return SOC_OK;
}

int soc_sca_zero(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_view) return fail(c, SOC_ERR_STATE, "soc_sca_zero: call soc_sca_set_view first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->dOUT, 0, view_pixels(c) * 4, c->stream));
    return SOC_OK;
}

// fill_sim for a launch of the scattered-light kernels, after the checks of its soc_sca_sim_* call: the checks they share, the image it
// adds to (soc_sca_batch_select's, else the view's) and its discrete scattering function; the rays tally nothing else
static int fill_sca(soc_ctx *c, SimKind kind, SocSim &S, SocVariant &V, int SOURCE, int BATCH, float SEED, float BG,
                    int GLOBAL, int gid_first, int gid_count)
{
    const char *who = sim_kinds[kind].who;
    const int k = sim_kinds[kind].scakind - 1;
    if (!c->have_view) return fail(c, SOC_ERR_STATE, "%s: call soc_sca_set_view first", who);
    if (k != SOC_SCA_CL && k != SOC_SCA_HP && !c->have_dsc) return fail(c, SOC_ERR_STATE, "%s: soc_set_scatter_table was called without DSC", who);
    if (c->BINS > 8000) return fail(c, SOC_ERR_ARG, "%s: BINS=%d > 8000", who, c->BINS);
    HIPCHK(c, hipSetDevice(c->device));
    fill_sim(c, S, V, SOURCE, BATCH, SEED, BG, 0.0f, GLOBAL, gid_first, gid_count);
    S.NO_PS = 1;
    S.TABS = nullptr;  S.INT = nullptr;
    S.SCAKIND = k + 1;  S.DSC = c->dDSC;
    S.OUT = c->out_slots ? c->dOUTslots + (size_t)c->out_slot_cur * c->out_slot_pixels : c->dOUT;
    V.wint = 0;
    return SOC_OK;
}

int soc_sca_sim_ps(soc_ctx *c, int PACKETS, int BATCH, float SEED, float BG, const float *PSPOS, const float *PS, int NO_PS,
                   const int32_t *XPS_NSIDE, const int32_t *XPS_SIDE, const float *XPS_AREA,
                   int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sca_sim_ps", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    SocSim S;
    SocVariant V;
    r = fill_sca(c, SCA_PS, S, V, 0, BATCH, SEED, BG, GLOBAL, gid_first, gid_count);
    if (r) return r;
    return route_sim(c, SCA_PS, S, V, gid_count, [&](int slot) {
        return upload_sources(c, "soc_sca_sim_ps", S, PSPOS, PS, NO_PS, XPS_NSIDE, XPS_SIDE, XPS_AREA, true, slot < 0 ? 0 : slot);
    });
}

int soc_sca_sim_pb(soc_ctx *c, int SOURCE, int PACKETS, int BATCH, float SEED, float BG, const float *PSPOS, const float *PS,
                   int NO_PS, const int32_t *XPS_NSIDE, const int32_t *XPS_SIDE, const float *XPS_AREA,
                   int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sca_sim_pb", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (SOURCE != 0 && SOURCE != 1)
        return fail(c, SOC_ERR_ARG, "soc_sca_sim_pb: SOURCE=%d (0 point sources, 1 background; ROI_LOAD is not supported)", SOURCE);
    SocSim S;
    SocVariant V;
    r = fill_sca(c, SCA_PB, S, V, SOURCE, BATCH, SEED, BG, GLOBAL, gid_first, gid_count);
    if (r) return r;
    return route_sim(c, SCA_PB, S, V, gid_count, [&](int slot) {
        return SOURCE == 0 ? upload_sources(c, "soc_sca_sim_pb", S, PSPOS, PS, NO_PS, XPS_NSIDE, XPS_SIDE, XPS_AREA, true, slot < 0 ? 0 : slot) : SOC_OK;
    });
}

int soc_sca_sim_cl(soc_ctx *c, int SOURCE, int PACKETS, int BATCH, float SEED, int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;  (void)SOURCE;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sca_sim_cl", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (!c->have_emit) return fail(c, SOC_ERR_STATE, "soc_sca_sim_cl: call soc_set_emission first");
    SocSim S;
    SocVariant V;
    r = fill_sca(c, SCA_CL, S, V, SOC_SOURCE_CL, BATCH, SEED, 0.0f, GLOBAL, gid_first, gid_count);
    if (r) return r;
    return route_sim(c, SCA_CL, S, V, gid_count, [&](int slot) { return keep_emission(c, S, slot); });
}

int soc_sca_sim_hp(soc_ctx *c, int PACKETS, int BATCH, float SEED, int GLOBAL, int gid_first, int gid_count)
{
    (void)PACKETS;
    if (!c) return SOC_ERR_ARG;
    int r = check_launch(c, "soc_sca_sim_hp", BATCH, GLOBAL, gid_first, gid_count);
    if (r) return r;
    if (!c->have_hpbg) return fail(c, SOC_ERR_STATE, "soc_sca_sim_hp: call soc_set_hpbg first");
    SocSim S;
    SocVariant V;
    r = fill_sca(c, SCA_HP, S, V, 1, BATCH, SEED, 0.0f, GLOBAL, gid_first, gid_count);
    if (r) return r;
    return route_sim(c, SCA_HP, S, V, gid_count, [&](int slot) { return keep_sky(c, S, slot); });
}

int soc_sca_read_out(soc_ctx *c, float *out, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_view) return fail(c, SOC_ERR_STATE, "soc_sca_read_out: call soc_sca_set_view first");
    const int64_t npix = (int64_t)view_pixels(c);
    if (!out || n < 0 || n > npix) return fail(c, SOC_ERR_ARG, "soc_sca_read_out: n=%lld (image has %lld values)", (long long)n, (long long)npix);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->dOUT, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

void *soc_sca_out_ptr(soc_ctx *c) { return (c && c->have_view) ? (void *)c->dOUT.p : nullptr; }

int soc_sca_batch_images(soc_ctx *c, int n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (n < 0 || n > 4096) return fail(c, SOC_ERR_ARG, "soc_sca_batch_images: n=%d (0 = the image of soc_sca_set_view again, at most 4096)", n);
    if (n > 0 && !c->have_view) return fail(c, SOC_ERR_STATE, "soc_sca_batch_images: call soc_sca_set_view first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t pix = view_pixels(c);
    if (n > 0) {
        HIPCHK(c, c->dOUTslots.reserve((size_t)n * pix, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dOUTslots, 0, (size_t)n * pix * 4, c->stream));
    }
    c->out_slots = n;  c->out_slot_pixels = pix;  c->out_slot_cur = 0;
    return SOC_OK;
}

int soc_sca_batch_select(soc_ctx *c, int k)
{
    if (!c) return SOC_ERR_ARG;
    if (k < 0 || k >= c->out_slots) return fail(c, SOC_ERR_ARG, "soc_sca_batch_select: image %d of %d (soc_sca_batch_images)", k, c->out_slots);
    c->out_slot_cur = k;                                     // (launches already deferred keep the image they were given)
    return SOC_OK;
}

int soc_sca_batch_read(soc_ctx *c, int k, float *out, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (k < 0 || k >= c->out_slots) return fail(c, SOC_ERR_ARG, "soc_sca_batch_read: image %d of %d (soc_sca_batch_images)", k, c->out_slots);
    if (!out || n < 0 || (size_t)n > c->out_slot_pixels) return fail(c, SOC_ERR_ARG, "soc_sca_batch_read: n=%lld (an image has %lld values)", (long long)n, (long long)c->out_slot_pixels);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->dOUTslots + (size_t)k * c->out_slot_pixels, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_sca_bind_out(soc_ctx *c, void *device_ptr)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_view) return fail(c, SOC_ERR_STATE, "soc_sca_bind_out: call soc_sca_set_view first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t npix = view_pixels(c);
    if (device_ptr) {
        c->dOUT.bind((float *)device_ptr, npix);
    } else {                                                // back to memory of the library
        HIPCHK(c, c->dOUT.reset(npix, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dOUT, 0, npix * 4, c->stream));
    }
    return SOC_OK;
}

int soc_sync(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_read_tally(soc_ctx *c, int which, float *out, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_read_tally: call soc_set_grid first");
    float *b = tally_buf(c, which);
    if (!b || !out || n < 0 || n > c->G.CELLS) return fail(c, SOC_ERR_ARG, "soc_read_tally: which=%d n=%lld", which, (long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, b, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

int soc_write_tally(soc_ctx *c, int which, const float *in, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_write_tally: call soc_set_grid first");
    float *b = tally_buf(c, which);
    if (!b || !in || n < 0 || n > c->G.CELLS) return fail(c, SOC_ERR_ARG, "soc_write_tally: which=%d n=%lld", which, (long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(b, in, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SOC_OK;
}

void *soc_tally_ptr(soc_ctx *c, int which) { return c ? (void *)tally_buf(c, which) : nullptr; }

int soc_bind_tally(soc_ctx *c, int which, void *device_ptr, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (which != SOC_TALLY_TABS && which != SOC_TALLY_INT) return fail(c, SOC_ERR_ARG, "soc_bind_tally: which=%d", which);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_bind_tally: call soc_set_grid first (the tally has CELLS elements)");
    if (device_ptr && n != (int64_t)c->G.CELLS)
        return fail(c, SOC_ERR_ARG, "soc_bind_tally: the buffer holds %lld floats, the grid has %d cells", (long long)n, c->G.CELLS);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DevBuf<float> &buf = (which == SOC_TALLY_TABS) ? c->dTABS : c->dINT;
    if (device_ptr) {
        buf.bind((float *)device_ptr, (size_t)n);
    } else {                                                // back to memory of the library
        HIPCHK(c, buf.reset((size_t)c->G.CELLS, c->stream));
        HIPCHK(c, hipMemsetAsync(buf, 0, (size_t)c->G.CELLS * 4, c->stream));
    }
    return SOC_OK;
}

int soc_read_par(soc_ctx *c, int32_t *out, int64_t n)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    if (!c->have_grid) return fail(c, SOC_ERR_STATE, "soc_read_par: call soc_set_grid first");
    if (!out || n < 0 || n > c->npar) return fail(c, SOC_ERR_ARG, "soc_read_par: n=%lld (have %lld)", (long long)n, (long long)c->npar);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n) HIPCHK(c, hipMemcpy(out, c->dPAR, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SOC_OK;
}

int soc_stats(soc_ctx *c, uint64_t out[3], int reset)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long h[4];
    HIPCHK(c, hipMemcpy(h, c->dStats, sizeof h, hipMemcpyDeviceToHost));
    if (out) for (int i = 0; i < 3; i++) out[i] = h[i];
    c->ray_steps = h[3];
    if (reset) HIPCHK(c, hipMemsetAsync(c->dStats, 0, sizeof h, c->stream));
    return SOC_OK;
}

int64_t soc_sca_ray_steps(soc_ctx *c) { return c ? (int64_t)c->ray_steps : -1; }

int soc_timer_start(soc_ctx *c)
{
    if (!c) return SOC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    return SOC_OK;
}

int soc_timer_stop(soc_ctx *c, float *elapsed_ms)
{
    if (!c) return SOC_ERR_ARG;
    FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (elapsed_ms) *elapsed_ms = ms;
    return SOC_OK;
}

}  // extern "C"
#pragma GCC visibility pop
