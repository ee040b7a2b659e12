/*
 * split_host.c -- CPU restatement of SimBgSplit (kernel_ASOC.c:2117-2851): isotropic background packets that split into
 * four rays, one per sub-element of the face they entered through, whenever they step into a refined cell.  TEST
 * INFRASTRUCTURE ONLY (tests/split_host.py builds and binds it; tools/make_split_golden.py pins it against the reference).
 *
 * The traversal, scattering and RNG primitives and the two math modes are the oracle's (oracle/soc_oracle.c, included as
 * a unit): -DSOC_ORACLE_LIBM gives what the reference's x86 build computes, the default what the HIP kernel computes.
 *
 * What the kernel does per work item, as the reference orders it:
 *   for elem < SELEM: surface element id + elem*GLOBAL (return at >= AREA); BATCH root rays per element;
 *   a ray born in a refined boundary cell is split at once (:2300-2428); a step into a finer cell splits (:2566-2709), with
 *   the first four stack entries replicated for jumps of two or more levels; PHOTONS *= 0.25^d going down, *= 4^d going
 *   up; a ray ends where it reaches a level below the one it was created on (RL); rays are popped last in, first out, each
 *   with a new free path; more than 20 scatterings stop a ray after its next full step; more than 30000 steps end the
 *   WHOLE work item; a split with NBUF > MAX_SPLIT-10 drops the ray and everything on its stack.
 *
 * One bound the reference lacks: it writes 4^d entries without looking, so a split whose entries would not fit
 * (NBUF + 4^d > MAX_SPLIT; only jumps of two or more levels, or a ray born two or more levels deep, with a small MAX_SPLIT) runs
 * past its slab there.  Here, as in the HIP kernel, such a split is an overflow drop too; sp_args.guard counts them, and
 * the golden cases are checked to have none.
 */
#include "../../oracle/soc_oracle.c"

#include <stdio.h>

typedef struct {
    int   SELEM, max_split;
    int   gid0, gid1;                 /* work items [gid0, gid1) in id order */
    unsigned long long n[6];          /* root rays, splits, splits over >= 2 levels, ends by level < RL, overflow drops, 30000-step returns */
    unsigned long long guard;         /* of the overflow drops: splits the reference would have written past its slab for */
    unsigned long long initial;       /* of the splits: rays born in a refined boundary cell */
    unsigned long long stop20;        /* rays stopped after more than 20 scatterings */
    int   max_depth;                  /* largest number of entries the stack of a work item held */
} sp_args;

#ifdef SOC_ORACLE_LIBM
#  define SP_ROUND(x)  roundf(x)
#  define SP_FMOD2(x)  fmodf((x), 2.0f)
#else
/* round(): half away from zero; x - trunc(x) is exact */
static inline float SP_ROUND(float x)
{
    float r = __builtin_truncf(x);
    if (fabsf(x - r) >= 0.5f) r += __builtin_copysignf(1.0f, x);
    return r;
}
#  define SP_FMOD2(x)  soc_fmodf_small((x), 2.0f)
#endif

/* stack entry: level, ind (bits), POS, DIR, PHOTONS, RL (:2175) */
typedef struct { float *B; int n, cap, depth; } sp_stack;

static inline float i2f(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline int   f2i(float f) { int i; memcpy(&i, &f, 4); return i; }

static void sp_put(sp_stack *st, int slot, int level, int ind, f3 P, f3 D, float photons, int RL)
{
    float *e = st->B + 10 * (long)slot;
    e[0] = (float)level;  e[1] = i2f(ind);
    e[2] = P.x;  e[3] = P.y;  e[4] = P.z;
    e[5] = D.x;  e[6] = D.y;  e[7] = D.z;
    e[8] = photons;  e[9] = (float)RL;
}

/* the ray (level, ind, POS, DIR, PHOTONS already scaled, RL) has arrived level - level0 levels deeper: push it, its three
 * siblings across the face it came through, and the replicas of those four for the levels in between (:2576-2663) */
static void sp_split(sp_stack *st, int level0, int level, int ind, f3 POS, f3 DIR, float PHOTONS, int RL)
{
    const int NBUF0 = st->n;
    f3  P1 = POS, P2 = POS, P3 = POS;
    int i1, i2, i3;
    sp_put(st, st->n, level, ind, POS, DIR, PHOTONS, RL);
    st->n += 1;
    const float dx = fabsf(POS.x - SP_ROUND(POS.x));
    const float dy = fabsf(POS.y - SP_ROUND(POS.y));
    const float dz = fabsf(POS.z - SP_ROUND(POS.z));
    const int SID = ind % 8;
    const int sx = ((SID % 2) == 0) ? 1 : (-1), sy = ((SID % 4) < 2) ? 2 : (-2), sz = (SID < 4) ? 4 : (-4);
    if (dx < fminf(dy, dz)) {                 /* entered through an x face: the siblings lie in y and z */
        i1 = ind + sy;       P1.y = SP_FMOD2(POS.y + 1.0f);
        i2 = ind + sz;       P2.z = SP_FMOD2(POS.z + 1.0f);
        i3 = ind + sy + sz;  P3.y = SP_FMOD2(POS.y + 1.0f);  P3.z = SP_FMOD2(POS.z + 1.0f);
    } else if (dy < dz) {                     /* a y face: x and z */
        i1 = ind + sx;       P1.x = SP_FMOD2(POS.x + 1.0f);
        i2 = ind + sz;       P2.z = SP_FMOD2(POS.z + 1.0f);
        i3 = ind + sx + sz;  P3.x = SP_FMOD2(POS.x + 1.0f);  P3.z = SP_FMOD2(POS.z + 1.0f);
    } else {                                  /* a z face: x and y */
        i1 = ind + sx;       P1.x = SP_FMOD2(POS.x + 1.0f);
        i2 = ind + sy;       P2.y = SP_FMOD2(POS.y + 1.0f);
        i3 = ind + sx + sy;  P3.x = SP_FMOD2(POS.x + 1.0f);  P3.y = SP_FMOD2(POS.y + 1.0f);
    }
    sp_put(st, st->n,     level, i1, P1, DIR, PHOTONS, level0 + 1);
    sp_put(st, st->n + 1, level, i2, P2, DIR, PHOTONS, level0 + 1);
    sp_put(st, st->n + 2, level, i3, P3, DIR, PHOTONS, level0 + 1);
    st->n += 3;
    for (int j = level0 + 2; j <= level; j++) {
        const int no = (int)(3 * M_POWN(4.0f, j - level0 - 2));
        for (int i = 0; i < no; i++) {
            memcpy(st->B + 10 * (long)st->n, st->B + 10 * (long)NBUF0, 40 * sizeof(float));
            for (int k = 0; k < 4; k++) st->B[10 * (long)(st->n + k) + 9] = (float)j;
            st->n += 4;
        }
    }
    if (st->n > st->depth) st->depth = st->n;
}

static void sp_pop(sp_stack *st, int *level, int *ind, f3 *POS, f3 *DIR, float *PHOTONS, int *RL)
{
    st->n -= 1;
    const float *e = st->B + 10 * (long)st->n;
    *level = (int)e[0];  *ind = f2i(e[1]);
    POS->x = e[2];  POS->y = e[3];  POS->z = e[4];
    DIR->x = e[5];  DIR->y = e[6];  DIR->z = e[7];
    *PHOTONS = e[8];  *RL = (int)e[9];
}

/* entries a split over d levels adds */
static inline long sp_entries(int d) { return 1L << (2 * d); }

static void sp_tally(const orc_model *M, int oind, float delta, f3 DIR)
{
    tally(M, M->TABS, oind, M->TW * 1.0f * delta);
    if (M->WITH_INT) tally(M, M->INT, oind, delta);
    if (M->INTV) {
        tally(M, M->INTV, oind, delta * DIR.x);
        tally(M, M->INTV + M->CELLS, oind, delta * DIR.y);
        tally(M, M->INTV + 2 * (long)M->CELLS, oind, delta * DIR.z);
    }
}

static void sp_workitem(const orc_model *M, sp_args *A, int id, sp_stack *st)
{
    const int NX = M->NX, NY = M->NY, NZ = M->NZ;
    const int AREA = 2 * (NX * NY + NY * NZ + NZ * NX);
    const float *DENS = M->DENS;
    const int *OFF = M->OFF;
    orc_model E1 = *M;                        /* pb_surface_element / pb_create read SOURCE and BG from the model */
    E1.SOURCE = 1;
    rng_t rng;
    seed_workitem(&rng, M->SEED, (uint64_t)id);
    for (int elem = 0; elem < A->SELEM; elem++) {
        const int el = id + elem * M->GLOBAL;
        if (el >= AREA) return;
        surf_t E;
        pb_surface_element(&E1, el, &E);
        for (int III = 0; III < M->BATCH; III++) {
            f3    POS = {0, 0, 0}, DIR = {0, 0, 0}, POS0;
            float PHOTONS = 0.0f, ds, free_path, tau, dtau, delta, tauA, dx;
            int   level = 0, ind = -1, oind = 0, ind0 = -1, level0 = 0, RL = 0, scatterings, steps, STOP = 0;
            pb_create(&E1, &E, III, &rng, &POS, &DIR, &PHOTONS, &level, &ind);
            if (fabsf(DIR.x) < DEPS) DIR.x = DEPS;
            if (fabsf(DIR.y) < DEPS) DIR.y = DEPS;
            if (fabsf(DIR.z) < DEPS) DIR.z = DEPS;
            normalize3(&DIR);
            A->n[0]++;
            st->n = 0;
            if (level > 0) {                  /* born in a refined boundary cell (:2300-2428) */
                if (sp_entries(level) > st->cap) {
                    A->n[4]++;  A->guard++;
                    continue;
                }
                PHOTONS *= M_POWN(0.25f, level);
                A->n[1]++;  A->initial++;
                if (level >= 2) A->n[2]++;
                sp_split(st, 0, level, ind, POS, DIR, PHOTONS, 0);
                sp_pop(st, &level, &ind, &POS, &DIR, &PHOTONS, &RL);
            }
            scatterings = 0;
            tau = 0.0f;
            free_path = -M_LOG(Rand(&rng));
            steps = 0;
            while (1) {
                tau = 0.0f;
                while (ind >= 0) {
                    oind   = OFF[level] + ind;
                    ind0   = ind;
                    level0 = level;
                    POS0   = POS;
                    ds     = GetStep(M, &POS, &DIR, &level, &ind);
                    steps += 1;
                    if (steps > 30000) { A->n[5]++;  return; }
                    if (M->WITH_ABU) dtau = ds * DENS[oind] * M->OPT[2 * (long)oind + 1];
                    else             dtau = ds * DENS[oind] * M->SCA;
                    if (free_path < (tau + dtau)) { ind = ind0;  break; }
                    if (M->WITH_ABU) tauA = ds * DENS[oind] * M->OPT[2 * (long)oind];
                    else             tauA = ds * DENS[oind] * M->ABS;
                    delta = PHOTONS * ((tauA > TAULIM) ? (1.0f - M_EXP(-tauA)) : (tauA * (1.0f - 0.5f * tauA)));
                    sp_tally(M, oind, delta, DIR);
                    PHOTONS *= M_EXP(-tauA);
                    tau += dtau;
                    if ((level == level0) && (ind == ind0)) {
                        POS.x += PEPS * DIR.x;  POS.y += PEPS * DIR.y;  POS.z += PEPS * DIR.z;
                        steps += 1;
                    }
                    if (ind >= 0) {
                        if (level > level0) {
                            const int over = st->n > (st->cap - 10), wide = st->n + sp_entries(level - level0) > st->cap;
                            if (over || wide) {
                                A->n[4]++;
                                if (!over) A->guard++;
                                st->n = 0;  ind = -1;
                                break;
                            }
                            A->n[1]++;
                            if (level - level0 >= 2) A->n[2]++;
                            PHOTONS *= M_POWN(0.25f, level - level0);
                            sp_split(st, level0, level, ind, POS, DIR, PHOTONS, RL);
                            sp_pop(st, &level, &ind, &POS, &DIR, &PHOTONS, &RL);
                            level0 = level;  ind0 = ind;
                            scatterings = 0;
                            tau = 0.0f;
                            free_path = -M_LOG(Rand(&rng));
                            steps = 0;
                        }
                        if (level < level0) {
                            if (level < RL) { ind = -1;  STOP = 1;  A->n[3]++; }
                            PHOTONS *= M_POWN(4.0f, level0 - level);
                        }
                        if (STOP) ind = -1;
                    }
                    if ((st->n > 0) && ((ind < 0) || STOP)) {
                        sp_pop(st, &level, &ind, &POS, &DIR, &PHOTONS, &RL);
                        STOP = 0;
                        scatterings = 0;
                        tau = 0.0f;
                        free_path = -M_LOG(Rand(&rng));
                        steps = 0;
                    }
                    if (STOP) ind = -1;
                }
                if (ind < 0) break;
                scatterings++;
                dtau = free_path - tau;
                if (M->WITH_ABU) {
                    dx   = dtau / (M->OPT[2 * (long)oind + 1] * DENS[oind]);
                    tauA = dx * DENS[oind] * M->OPT[2 * (long)oind];
                } else {
                    dx   = dtau / (M->SCA * DENS[oind]);
                    tauA = dx * DENS[oind] * M->ABS;
                }
                delta = (tauA > TAULIM) ? (PHOTONS * (1.0f - M_EXP(-tauA))) : (PHOTONS * tauA * (1.0f - 0.5f * tauA));
                /* the reference multiplies delta*TW*ADHOC here and TW*ADHOC*delta in the step; with ADHOC 1 both are one product */
                sp_tally(M, oind, delta, DIR);
                dx = M_LDEXP_UP(dx, level0);
                dx = fmaxf(0.0f, dx - 2.0f * PEPS);
                POS.x = POS0.x + dx * DIR.x;
                POS.y = POS0.y + dx * DIR.y;
                POS.z = POS0.z + dx * DIR.z;
                PHOTONS *= M_EXP(-tauA);
                free_path = -M_LOG(Rand(&rng));
                ind   = ind0;
                level = level0;
                if (M->MSF_NDUST > 1) Scatter(&DIR, M->CSC + (long)MsfDust(M, &rng, oind) * M->BINS, M->BINS, &rng);
                else                  Scatter(&DIR, M->CSC, M->BINS, &rng);
                if (scatterings > 20) { if (!STOP) A->stop20++;  STOP = 1; }
            }
        }
    }
}

/* work items [gid0, gid1) in id order; returns 0, or -1 for arguments no launch can have */
int sp_sim_bg_split(const orc_model *M, sp_args *A)
{
    if (A->max_split < 14 || A->SELEM < 1 || A->gid0 < 0 || A->gid1 > M->GLOBAL || M->threaded) return -1;
    sp_stack st;
    st.B = (float *)malloc(sizeof(float) * 10 * (size_t)A->max_split);
    st.cap = A->max_split;
    st.depth = 0;
    memset(A->n, 0, sizeof A->n);
    A->guard = A->initial = A->stop20 = 0;
    for (int id = A->gid0; id < A->gid1; id++) {
        st.n = 0;
        sp_workitem(M, A, id, &st);
    }
    A->max_depth = st.depth;
    free(st.B);
    return 0;
}

int sp_math_mode(void)
{
#ifdef SOC_ORACLE_LIBM
    return 0;
#else
    return 1;
#endif
}
