/*
 * hpsplit_host.c -- CPU restatement of SimHpSplit (kernel_ASOC.c:2871-3550): packets of a Healpix sky that split into four
 * rays whenever they step into a refined cell.  TEST INFRASTRUCTURE ONLY (tests/hpsplit_host.py builds and binds it;
 * tools/make_hpsplit_golden.py pins it against the reference).
 *
 * It sits on split_host.c (the stack entry, push of the first four entries' arithmetic, pop, tallies; included as a unit and
 * with it oracle/soc_oracle.c and the two math modes) and restates what SimHpSplit does differently from SimBgSplit:
 *   work item id sends BATCH root rays and that is all: no loop over surface elements, no return at ind >= AREA, and none at
 *   id >= 8*AREA as in SimRAM_HP;
 *   a root ray is created like a SimRAM_HP packet (pixel uniform or by 10 bisections + scan on HPBGP, Pixel2AnglesRing(64),
 *   face with probability ~ |DIR_i|) but the face is chosen on the RAW direction and the clamp to DEPS and the normalisation
 *   follow IndexG (:2963-2988);
 *   the initial split does not reload PHOTONS from the popped entry (:3123);
 *   inside the walk a ray splits only where (NBUF+4) < (MAX_SPLIT-1) (:3263); otherwise it goes on unsplit on the finer level
 *   with PHOTONS unscaled, and a later step to a coarser level still multiplies by 4^d and still tests level < RL
 *   (skipped_splits counts these);
 *   the replicas of a jump over two or more levels are written level by level, only where (NBUF + 4*no) < MAX_SPLIT (:3352);
 *   a level that does not fit is skipped and later levels are still tried (skipped_replicas).
 * With these tests the walk never writes past the stack.  The initial split writes 4^level entries without looking in the
 * reference; here, as in the HIP kernel and as for SimBgSplit, a root ray with 4^level > MAX_SPLIT is an overflow drop counted in
 * guard, and the golden cases are checked to have none.
 */
#include "split_host.c"

typedef struct {
    int   max_split;
    int   gid0, gid1;                 /* work items [gid0, gid1) in id order */
    unsigned long long n[6];          /* root rays, splits, splits over >= 2 levels, ends by level < RL, overflow drops, 30000-step returns */
    unsigned long long guard;         /* of the overflow drops: root rays born too deep for the stack (the reference writes past its slab) */
    unsigned long long initial;       /* of the splits: rays born in a refined boundary cell */
    unsigned long long stop20;        /* rays stopped after more than 20 scatterings */
    unsigned long long skipped_splits;     /* steps into a finer cell with (NBUF+4) >= (MAX_SPLIT-1): not split */
    unsigned long long skipped_replicas;   /* levels of a jump over >= 2 levels whose replicas did not fit */
    int   max_depth;                  /* largest number of entries the stack of a work item held */
} hs_args;

/* sp_split with the walk's conditional replicas (:3350-3360); cond 0: the initial split's (:3082-3090) */
static void hs_split(sp_stack *st, hs_args *A, int cond, int level0, int level, int ind, f3 POS, f3 DIR, float PHOTONS, int RL)
{
    const int NBUF0 = st->n;
    sp_split(st, level0, level0 + 1, ind, POS, DIR, PHOTONS, RL);      /* the first four entries; no replicas for one level */
    for (int k = 0; k < 4; k++) st->B[10 * (long)(NBUF0 + k)] = (float)level;
    for (int j = level0 + 2; j <= level; j++) {
        const int no = (int)(3 * M_POWN(4.0f, j - level0 - 2));
        if (cond && !((st->n + 4 * no) < st->cap)) { A->skipped_replicas++;  continue; }
        for (int i = 0; i < no; i++) {
            memcpy(st->B + 10 * (long)st->n, st->B + 10 * (long)NBUF0, 40 * sizeof(float));
            for (int k = 0; k < 4; k++) st->B[10 * (long)(st->n + k) + 9] = (float)j;
            st->n += 4;
        }
    }
    if (st->n > st->depth) st->depth = st->n;
}

static void hs_workitem(const orc_model *M, hs_args *A, int id, sp_stack *st)
{
    const int NX = M->NX, NY = M->NY, NZ = M->NZ;
    const float *DENS = M->DENS;
    const int *OFF = M->OFF;
    rng_t rng;
    seed_workitem(&rng, M->SEED, (uint64_t)id);
    for (int III = 0; III < M->BATCH; III++) {
        f3    POS = {0, 0, 0}, DIR = {0, 0, 0}, POS0;
        float PHOTONS, ds, free_path, tau, dtau, delta, tauA, dx, phi, theta, x, y, z, v1, v2;
        int   level = 0, ind = -1, oind = 0, ind0 = -1, level0 = 0, RL = 0, scatterings, steps, STOP = 0;
        ind     = hp_select_pixel(M, &rng, 10);
        PHOTONS = M->HPBG[ind];
        pixel2angles_ring(64, ind, &phi, &theta);
        DIR.x = +M_SIN(theta) * M_COS(phi);
        DIR.y = +M_SIN(theta) * M_SIN(phi);
        DIR.z = -M_COS(theta);
        x = fabsf(DIR.x);  y = fabsf(DIR.y);  z = fabsf(DIR.z);
        ds = x + y + z;  x /= ds;  y /= ds;  z /= ds;
        ds = Rand(&rng);  v1 = Rand(&rng);  v2 = Rand(&rng);
        if (ds < x) {
            POS.y = v1 * NY;  POS.z = v2 * NZ;
            POS.x = (DIR.x > 0.0f) ? (PEPS) : (NX - PEPS);
        } else {
            if (ds < (x + y)) {
                POS.x = v1 * NX;  POS.z = v2 * NZ;
                POS.y = (DIR.y > 0.0f) ? (PEPS) : (NY - PEPS);
            } else {
                POS.x = v1 * NX;  POS.y = v2 * NY;
                POS.z = (DIR.z > 0.0f) ? (PEPS) : (NZ - PEPS);
            }
        }
        IndexG(M, &POS, &level, &ind);
        if (fabsf(DIR.x) < DEPS) DIR.x = DEPS;
        if (fabsf(DIR.y) < DEPS) DIR.y = DEPS;
        if (fabsf(DIR.z) < DEPS) DIR.z = DEPS;
        normalize3(&DIR);
        RL = 0;
        A->n[0]++;
        st->n = 0;
        if (level > 0) {                      /* born in a refined boundary cell (:2997-3125) */
            if (sp_entries(level) > st->cap) {
                A->n[4]++;  A->guard++;
                continue;
            }
            PHOTONS *= M_POWN(0.25f, level);
            A->n[1]++;  A->initial++;
            if (level >= 2) A->n[2]++;
            hs_split(st, A, 0, 0, level, ind, POS, DIR, PHOTONS, 0);
            float unused;
            sp_pop(st, &level, &ind, &POS, &DIR, &unused, &RL);        /* PHOTONS is not reloaded (:3123) */
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
                    if ((level > level0) && !((st->n + 4) < (st->cap - 1))) A->skipped_splits++;
                    if ((level > level0) && ((st->n + 4) < (st->cap - 1))) {           /* :3263 */
                        if (st->n > (st->cap - 10)) {
                            A->n[4]++;
                            st->n = 0;  ind = -1;
                            break;
                        }
                        A->n[1]++;
                        if (level - level0 >= 2) A->n[2]++;
                        PHOTONS *= M_POWN(0.25f, level - level0);
                        hs_split(st, A, 1, level0, level, ind, POS, DIR, PHOTONS, RL);
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

/* work items [gid0, gid1) in id order; returns 0, or -1 for arguments no launch can have */
int hs_sim_hp_split(const orc_model *M, hs_args *A)
{
    if (A->max_split < 14 || A->gid0 < 0 || A->gid1 > M->GLOBAL || M->threaded || !M->HPBG || (M->HPBG_WEIGHTED && !M->HPBGP)) return -1;
    sp_stack st;
    st.B = (float *)malloc(sizeof(float) * 10 * (size_t)A->max_split);
    st.cap = A->max_split;
    st.depth = 0;
    memset(A->n, 0, sizeof A->n);
    A->guard = A->initial = A->stop20 = A->skipped_splits = A->skipped_replicas = 0;
    for (int id = A->gid0; id < A->gid1; id++) {
        st.n = 0;
        hs_workitem(M, A, id, &st);
    }
    A->max_depth = st.depth;
    free(st.B);
    return 0;
}
