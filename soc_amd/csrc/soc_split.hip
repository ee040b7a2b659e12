// soc_split.hip -- background packets with packet splitting (`split 1`) for gfx950: the isotropic background
// (soc_sim_bg_split_kernel) and the Healpix sky (soc_sim_hp_split_kernel, at the end of the file with what it does differently).
//
// What is computed is what the reference's SimBgSplit computes (kernel_ASOC.c:2117-2851): each work item sends BATCH root
// rays from each of its SELEM surface elements; a ray that steps into a refined cell becomes four, one per sub-element of
// the face it came through (4^d for a jump of d levels), the extra rays waiting on a per-work-item stack; PHOTONS is scaled
// by 0.25^d going down and 4^d going up; a ray ends where it reaches a level below the one it was created on.  One lane is
// one logical work item with the MWC64X stream of its id, and every fp32 expression keeps the reference's operand order
// with the functions of soc_math.h, so a host build of the same arithmetic (tests/csrc/split_host.c) follows each lane's
// trajectory bit for bit; only the order of the atomic adds differs.
//
// How it is computed differs in the stack.  The reference gives every work item a contiguous slab of 10*MAX_SPLIT floats, so
// the 64 lanes of a wave that push or pop together touch 64 addresses 10*MAX_SPLIT*4 bytes apart: 64 memory transactions per
// field.  Here a wave owns a tile of max_split x 10 x 64 words laid out slot-major, lane-minor -- word (slot, field, lane) at
// (slot*10 + field)*64 + lane -- so the lanes that touch one field of one slot touch 64 consecutive words: one 256-byte
// transaction.  Lanes of a wave are mostly at different depths; each depth's accesses still coalesce among the lanes there.
//
// Workgroup = one wave (64 lanes): a launch has GLOBAL_SPLIT ~ 32768 work items (ASOC.py:311-315), i.e. 512 waves for 256 CUs, so
// larger groups would leave CUs idle; and a lane's life is dominated by its deepest ray tree, so nothing is gained by tying
// four waves' lifetimes together.  The kernel keeps the walker, the split bookkeeping and six counters in registers; it is
// bound by the latency of dependent cell look-ups, not by occupancy (two waves per SIMD at this launch size), so the register
// budget is left to the compiler under __launch_bounds__(64).
//
// Every loop keeps a bound of the reference: at most 30000 steps per ray (then the work item returns), a ray stops after more
// than 20 scatterings, the stack holds at most max_split entries.  The one bound added: a split whose 4^d entries would not fit
// the stack (the reference writes them without looking) is an overflow drop like NBUF > MAX_SPLIT-10.
#include "soc_walk.h"

// round(): half away from zero; x - trunc(x) is exact
__device__ __forceinline__ float soc_split_round(float x)
{
    float r = __builtin_truncf(x);
    if (soc_fabsf(x - r) >= 0.5f) r += __builtin_copysignf(1.0f, x);
    return r;
}

// one lane's view of its wave's stack tile
struct SocSplitStack {
    float *B;                  // word (slot 0, field 0) of this lane
    int    n;                  // NBUF
    __device__ __forceinline__ float &at(int slot, int field) const { return B[((size_t)slot * 10 + field) * 64]; }
    __device__ __forceinline__ void put(int slot, int level, int ind, float px, float py, float pz, float ux, float uy, float uz,
                                        float photons, int RL) const
    {
        at(slot, 0) = (float)level;  at(slot, 1) = __int_as_float(ind);
        at(slot, 2) = px;  at(slot, 3) = py;  at(slot, 4) = pz;
        at(slot, 5) = ux;  at(slot, 6) = uy;  at(slot, 7) = uz;
        at(slot, 8) = photons;  at(slot, 9) = (float)RL;
    }
};

// what soc_pb_create fills for a new root ray, and the work item's RNG stream
struct SocSplitRoot {
    float px, py, pz, ux, uy, uz, photons, dens;
    int   level, ind;
    soc_rng_t rng;
};

// per-lane state of the split walk
struct SocSplitRay {
    float px, py, pz, ux, uy, uz, photons, dens;
    int   level, ind, RL;
};

// The ray r (PHOTONS already scaled) has arrived level - level0 levels deeper: push it, its three siblings across the face
// it came through, and replicas of those four for the levels in between (kernel_ASOC.c:2576-2663).  COND (SimHpSplit's walk,
// :3350-3360): the replicas of a level are written only where (NBUF + 4*no) < MAX_SPLIT; a level that does not fit is skipped
// and the later ones are still tried
template <bool COND = false>
__device__ __forceinline__ void soc_split_push(SocSplitStack &st, const SocSplitRay &r, int level0, int cap = 0)
{
    const int NBUF0 = st.n, level = r.level, ind = r.ind;
    st.put(st.n, level, ind, r.px, r.py, r.pz, r.ux, r.uy, r.uz, r.photons, r.RL);
    st.n += 1;
    const float dx = soc_fabsf(r.px - soc_split_round(r.px));
    const float dy = soc_fabsf(r.py - soc_split_round(r.py));
    const float dz = soc_fabsf(r.pz - soc_split_round(r.pz));
    const int SID = ind % 8;
    const int sx = ((SID % 2) == 0) ? 1 : (-1), sy = ((SID % 4) < 2) ? 2 : (-2), sz = (SID < 4) ? 4 : (-4);
    const float qx = soc_fmodf_small(r.px + 1.0f, 2.0f), qy = soc_fmodf_small(r.py + 1.0f, 2.0f), qz = soc_fmodf_small(r.pz + 1.0f, 2.0f);
    // the two axes the siblings lie along: (a, b) = (y, z) behind an x face, (x, z) behind a y face, (x, y) behind a z face
    const int face = (dx < soc_fminf(dy, dz)) ? 0 : ((dy < dz) ? 1 : 2);
    const int sa = (face == 0) ? sy : sx, sb = (face == 2) ? sy : sz;
    for (int k = 1; k <= 3; k++) {
        const bool a = (k != 2), b = (k != 1);              // sibling 1 steps along a, 2 along b, 3 along both
        const bool mx = (face != 0) && a, my = (face == 0) ? a : ((face == 2) && b), mz = (face != 2) && b;
        st.put(st.n, level, ind + (a ? sa : 0) + (b ? sb : 0), mx ? qx : r.px, my ? qy : r.py, mz ? qz : r.pz,
               r.ux, r.uy, r.uz, r.photons, level0 + 1);
        st.n += 1;
    }
    for (int j = level0 + 2; j <= level; j++) {
        const int no = 3 << (2 * (j - level0 - 2));         // 3 * 4^(j-level0-2) copies of the first four entries
        if (COND && !((st.n + 4 * no) < cap)) continue;
        for (int i = 0; i < no; i++) {
            for (int k = 0; k < 4; k++) {
                for (int f = 0; f < 9; f++) st.at(st.n + k, f) = st.at(NBUF0 + k, f);
                st.at(st.n + k, 9) = (float)j;
            }
            st.n += 4;
        }
    }
}

__device__ __forceinline__ void soc_split_pop(const SocGrid &G, const int *sOFF, SocSplitStack &st, SocSplitRay &r)
{
    st.n -= 1;
    r.level = (int)st.at(st.n, 0);  r.ind = __float_as_int(st.at(st.n, 1));
    r.px = st.at(st.n, 2);  r.py = st.at(st.n, 3);  r.pz = st.at(st.n, 4);
    r.ux = st.at(st.n, 5);  r.uy = st.at(st.n, 6);  r.uz = st.at(st.n, 7);
    r.photons = st.at(st.n, 8);  r.RL = (int)st.at(st.n, 9);
    r.dens = G.DENS[sOFF[r.level] + r.ind];
}

// counters of one work item
struct SocSplitCount {
    unsigned int root = 0, split = 0, deep = 0, end = 0, drop = 0, longs = 0, depth = 0, tally = 0, scat = 0, skip = 0;
};

// The walk of one root ray r (created, direction clamped and normalised, RL 0) until it and everything on its stack have
// ended: SimBgSplit's (kernel_ASOC.c:2296-2836) and, with HP, SimHpSplit's (:2994-3546), which differ in the rule of the
// split inside the walk only.  Returns true where the whole work item returns (more than 30000 steps of one ray).
template <bool OCT, bool DBL, bool ABU, bool WINT, bool HP>
__device__ __forceinline__ bool soc_split_walk(const SocGrid &G, const SocSim &S, const float *sCSC, const int *sOFF, const int cap,
                                               SocSplitStack &st, SocSplitRay &r, soc_rng_t *rng, SocSplitCount &n)
{
    n.root++;
    st.n = 0;
    if (OCT && (r.level > 0)) {                    // born in a refined boundary cell (kernel_ASOC.c:2300-2428)
        if ((1 << (2 * r.level)) > cap) { n.drop++;  return false; }
        r.photons *= soc_pownf(0.25f, r.level);
        n.split++;
        if (r.level >= 2) n.deep++;
        soc_split_push(st, r, 0);
        n.depth = max(n.depth, (unsigned int)st.n);
        const float photons = r.photons;
        soc_split_pop(G, sOFF, st, r);
        if (HP) r.photons = photons;               // SimHpSplit does not reload PHOTONS here (:3123); the same value
    }
    int   scat = 0, steps = 0;
    bool  STOP = false;
    float tau = 0.0f;
    float free_path = -soc_logf(soc_rand(rng));
    while (true) {                                 // until the ray and everything on its stack have ended
        int   oind = 0, ind0 = r.ind, level0 = r.level;
        float p0x = r.px, p0y = r.py, p0z = r.pz, d0 = r.dens, kabs = S.ABS, ksca = S.SCA;
        tau = 0.0f;
        while (r.ind >= 0) {                       // until the next scattering
            oind = sOFF[r.level] + r.ind;
            ind0 = r.ind;  level0 = r.level;
            p0x = r.px;  p0y = r.py;  p0z = r.pz;  d0 = r.dens;
            if (ABU) { const float2 o = S.OPT[oind];  kabs = o.x;  ksca = o.y; }
            const float ds = soc_getstep<OCT, DBL>(G, sOFF, r.px, r.py, r.pz, r.ux, r.uy, r.uz, r.level, r.ind, r.dens);
            steps += 1;
            if (steps > 30000) { n.longs++;  return true; }      // the WHOLE work item returns (:2474-2479)
            const float dtau = ds * d0 * ksca;
            if (free_path < (tau + dtau)) { r.ind = ind0;  break; }
            const float tauA = ds * d0 * kabs;
            const float e = soc_expf(-tauA);
            const float delta = r.photons * ((tauA > SOC_TAULIM) ? (1.0f - e) : (tauA * (1.0f - 0.5f * tauA)));
            soc_tally(S.TABS, oind, S.TW * delta);
            if (WINT) {
                soc_tally(S.INT, oind, delta);
                if (S.INTV) {
                    soc_tally(S.INTV, oind, delta * r.ux);
                    soc_tally(S.INTV + S.CELLS, oind, delta * r.uy);
                    soc_tally(S.INTV + 2 * (long)S.CELLS, oind, delta * r.uz);
                }
            }
            n.tally++;
            r.photons *= e;
            tau += dtau;
            if ((r.level == level0) && (r.ind == ind0)) {                   // failed step (:2527-2555)
                r.px += SOC_PEPS * r.ux;  r.py += SOC_PEPS * r.uy;  r.pz += SOC_PEPS * r.uz;
                steps += 1;
            }
            if (r.ind >= 0) {
                // a finer cell: split (:2566-2709).  SimHpSplit (:3263-3407) splits only where (NBUF+4) < (MAX_SPLIT-1): with a
                // nearly full stack the ray goes on unsplit on the finer level, PHOTONS unscaled -- a quirk kept and counted
                const bool finer = OCT && (r.level > level0);
                if (HP && finer && !((st.n + 4) < (cap - 1))) n.skip++;
                if (finer && (!HP || ((st.n + 4) < (cap - 1)))) {
                    if ((st.n > (cap - 10)) || (!HP && (st.n + (1 << (2 * (r.level - level0))) > cap))) {
                        n.drop++;                                           // the ray and all on its stack are dropped
                        st.n = 0;  r.ind = -1;
                        break;
                    }
                    n.split++;
                    if (r.level - level0 >= 2) n.deep++;
                    r.photons *= soc_pownf(0.25f, r.level - level0);
                    soc_split_push<HP>(st, r, level0, cap);
                    n.depth = max(n.depth, (unsigned int)st.n);
                    soc_split_pop(G, sOFF, st, r);
                    level0 = r.level;  ind0 = r.ind;
                    scat = 0;  tau = 0.0f;  steps = 0;
                    free_path = -soc_logf(soc_rand(rng));
                }
                if (r.level < level0) {                                     // a coarser cell (:2714-2720)
                    if (r.level < r.RL) { r.ind = -1;  STOP = true;  n.end++; }
                    r.photons *= soc_pownf(4.0f, level0 - r.level);
                }
                if (STOP) r.ind = -1;
            }
            if ((st.n > 0) && ((r.ind < 0) || STOP)) {                      // the next ray of the stack (:2733-2750)
                soc_split_pop(G, sOFF, st, r);
                STOP = false;
                scat = 0;  tau = 0.0f;  steps = 0;
                free_path = -soc_logf(soc_rand(rng));
            }
            if (STOP) r.ind = -1;
        }
        if (r.ind < 0) break;
        // scattering in cell oind, entered at p0 on level0 (:2763-2832)
        scat++;
        const float dt = free_path - tau;
        float dx = dt / (ksca * d0);
        const float tauA = dx * d0 * kabs;
        const float e = soc_expf(-tauA);
        const float delta = (tauA > SOC_TAULIM) ? (r.photons * (1.0f - e)) : (r.photons * tauA * (1.0f - 0.5f * tauA));
        soc_tally(S.TABS, oind, delta * S.TW);
        if (WINT) {
            soc_tally(S.INT, oind, delta);
            if (S.INTV) {
                soc_tally(S.INTV, oind, delta * r.ux);
                soc_tally(S.INTV + S.CELLS, oind, delta * r.uy);
                soc_tally(S.INTV + 2 * (long)S.CELLS, oind, delta * r.uz);
            }
        }
        n.tally++;
        n.scat++;
        dx = soc_scale_up(dx, level0);
        dx = __builtin_fmaxf(0.0f, dx - 2.0f * SOC_PEPS);
        r.px = p0x + dx * r.ux;
        r.py = p0y + dx * r.uy;
        r.pz = p0z + dx * r.uz;
        r.photons *= e;
        free_path = -soc_logf(soc_rand(rng));
        r.ind = ind0;  r.level = level0;  r.dens = d0;
        float fp_unused = 0.0f;
        soc_new_direction<false>(S, sCSC, oind, r.ux, r.uy, r.uz, fp_unused, rng);
        if (scat > 20) STOP = true;                // takes effect after the ray's next full step (:2830-2832)
    }
    return false;
}

// a work item's counters into the launch's (soc_split_stats); word 7, the splits skipped on a nearly full stack, is SimHpSplit's
__device__ __forceinline__ void soc_split_count(const SocSim &S, const SocSplit &P, const SocSplitCount &n)
{
    if (S.stats) {
        atomicAdd(S.stats + 0, (unsigned long long)n.tally);
        atomicAdd(S.stats + 1, (unsigned long long)n.root);
        atomicAdd(S.stats + 2, (unsigned long long)n.scat);
    }
    atomicAdd(P.counters + 0, (unsigned long long)n.root);
    atomicAdd(P.counters + 1, (unsigned long long)n.split);
    atomicAdd(P.counters + 2, (unsigned long long)n.deep);
    atomicAdd(P.counters + 3, (unsigned long long)n.end);
    atomicAdd(P.counters + 4, (unsigned long long)n.drop);
    atomicAdd(P.counters + 5, (unsigned long long)n.longs);
    atomicMax(P.counters + 6, (unsigned long long)n.depth);
    if (n.skip) atomicAdd(P.counters + 7, (unsigned long long)n.skip);
}

template <bool OCT, bool DBL, bool ABU, bool WINT>
__global__ __launch_bounds__(64) void soc_sim_bg_split_kernel(const SocGrid G, const SocSim S, const SocSplit P)
{
    extern __shared__ float lds[];
    float *sCSC = lds;
    int   *sOFF = (int *)(lds + S.BINS);
    soc_stage_lds(G, S, sCSC, sOFF);

    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= S.gid_count) return;
    const int id = (int)(S.gid0 + t);                      // logical get_global_id(0)
    const int AREA = 2 * (G.NX * G.NY + G.NY * G.NZ + G.NZ * G.NX);
    const int cap = P.max_split;

    SocSplitStack st;
    st.B = P.stack + (size_t)blockIdx.x * (size_t)cap * 640 + threadIdx.x;
    st.n = 0;
    SocSplitRoot w;
    w.rng = soc_seed_stream(S.seed_mul, S.seed_tab, (uint32_t)id);
    w.level = 0;  w.ind = -1;  w.dens = 0.0f;

    SocSplitCount n;
    bool finished = false;

    for (int elem = 0; (elem < P.SELEM) && !finished; elem++) {
        const int el = id + elem * S.GLOBAL;
        if (el >= AREA) break;                             // the work item returns (kernel_ASOC.c:2198)
        const SocSurfElem E = soc_surface_element<1>(G, S, el);
        for (int III = 0; (III < S.BATCH) && !finished; III++) {
            soc_pb_create<OCT, SocSplitRoot, 1>(G, S, sOFF, E, III, w);
            SocSplitRay r;
            r.px = w.px;  r.py = w.py;  r.pz = w.pz;  r.ux = w.ux;  r.uy = w.uy;  r.uz = w.uz;
            r.photons = w.photons;  r.dens = w.dens;  r.level = w.level;  r.ind = w.ind;  r.RL = 0;
            soc_condition_direction(r.ux, r.uy, r.uz);
            finished = soc_split_walk<OCT, DBL, ABU, WINT, false>(G, S, sCSC, sOFF, cap, st, r, &w.rng, n);
        }
    }
    soc_split_count(S, P, n);
}

hipError_t soc_launch_sim_bg_split(const SocGrid &G, const SocSim &S, const SocSplit &P, const SocVariant &V, hipStream_t st)
{
    if (S.gid_count == 0) return hipSuccess;
    const dim3 grid((S.gid_count + 63) / 64), block(64);
    const size_t lds = (size_t)S.BINS * 4 + SOC_MAXL * 4;
    switch (soc_split_key(V)) {         // (soc_dev.h: what soc_last_variant reports comes from the same key)
    case 0:  soc_sim_bg_split_kernel<false, false, false, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 1:  soc_sim_bg_split_kernel<false, false, false, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 2:  soc_sim_bg_split_kernel<false, false, true, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 3:  soc_sim_bg_split_kernel<false, false, true, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 8:  soc_sim_bg_split_kernel<true, false, false, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 9:  soc_sim_bg_split_kernel<true, false, false, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 10: soc_sim_bg_split_kernel<true, false, true, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 11: soc_sim_bg_split_kernel<true, false, true, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 12: soc_sim_bg_split_kernel<true, true, false, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 13: soc_sim_bg_split_kernel<true, true, false, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 14: soc_sim_bg_split_kernel<true, true, true, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 15: soc_sim_bg_split_kernel<true, true, true, true><<<grid, block, lds, st>>>(G, S, P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- the Healpix sky with packet splitting: SimHpSplit (kernel_ASOC.c:2871-3550) ----
//
// What differs from SimBgSplit: no loop over surface elements and no return at ind >= AREA -- work item id sends BATCH root
// rays and that is all (no work item returns at id >= 8*AREA either, as SimRAM_HP's do); a root ray is created like a SimRAM_HP
// packet, but with the face chosen on the direction as it comes from the pixel and the clamp to DEPS after IndexG (soc_hp_create
// with RAW); the split inside the walk is skipped on a nearly full stack and writes the replicas of a jump over two or more
// levels level by level where they fit (soc_split_walk with HP).  Same lane = work item, same stack tile, same counters.  The
// sky (2 x 49152 floats) is read once per root ray from HBM/L2, as in soc_hp_create's other callers.
template <bool OCT, bool DBL, bool ABU, bool WINT>
__global__ __launch_bounds__(64) void soc_sim_hp_split_kernel(const SocGrid G, const SocSim S, const SocSplit P)
{
    extern __shared__ float lds[];
    float *sCSC = lds;
    int   *sOFF = (int *)(lds + S.BINS);
    soc_stage_lds(G, S, sCSC, sOFF);

    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= S.gid_count) return;
    const int id = (int)(S.gid0 + t);                      // logical get_global_id(0)
    const int cap = P.max_split;

    SocSplitStack st;
    st.B = P.stack + (size_t)blockIdx.x * (size_t)cap * 640 + threadIdx.x;
    st.n = 0;
    SocSplitRoot w;
    w.rng = soc_seed_stream(S.seed_mul, S.seed_tab, (uint32_t)id);
    w.level = 0;  w.ind = -1;  w.dens = 0.0f;

    SocSplitCount n;
    bool finished = false;

    for (int III = 0; (III < S.BATCH) && !finished; III++) {
        soc_hp_create<OCT, SocSplitRoot, true>(G, S, sOFF, w);
        SocSplitRay r;
        r.px = w.px;  r.py = w.py;  r.pz = w.pz;  r.ux = w.ux;  r.uy = w.uy;  r.uz = w.uz;
        r.photons = w.photons;  r.dens = w.dens;  r.level = w.level;  r.ind = w.ind;  r.RL = 0;
        soc_condition_direction(r.ux, r.uy, r.uz);
        finished = soc_split_walk<OCT, DBL, ABU, WINT, true>(G, S, sCSC, sOFF, cap, st, r, &w.rng, n);
    }
    soc_split_count(S, P, n);
}

hipError_t soc_launch_sim_hp_split(const SocGrid &G, const SocSim &S, const SocSplit &P, const SocVariant &V, hipStream_t st)
{
    if (S.gid_count == 0) return hipSuccess;
    if (!S.HPBG || (S.HPBG_WEIGHTED && !S.HPBGP)) return hipErrorInvalidValue;
    const dim3 grid((S.gid_count + 63) / 64), block(64);
    const size_t lds = (size_t)S.BINS * 4 + SOC_MAXL * 4;
    switch (soc_split_key(V)) {         // (soc_dev.h: what soc_last_variant reports comes from the same key)
    case 0:  soc_sim_hp_split_kernel<false, false, false, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 1:  soc_sim_hp_split_kernel<false, false, false, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 2:  soc_sim_hp_split_kernel<false, false, true, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 3:  soc_sim_hp_split_kernel<false, false, true, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 8:  soc_sim_hp_split_kernel<true, false, false, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 9:  soc_sim_hp_split_kernel<true, false, false, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 10: soc_sim_hp_split_kernel<true, false, true, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 11: soc_sim_hp_split_kernel<true, false, true, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 12: soc_sim_hp_split_kernel<true, true, false, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 13: soc_sim_hp_split_kernel<true, true, false, true><<<grid, block, lds, st>>>(G, S, P); break;
    case 14: soc_sim_hp_split_kernel<true, true, true, false><<<grid, block, lds, st>>>(G, S, P); break;
    case 15: soc_sim_hp_split_kernel<true, true, true, true><<<grid, block, lds, st>>>(G, S, P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
