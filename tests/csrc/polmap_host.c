/* polmap_host.c -- CPU restatement of the reference's PolMapping kernels (kernel_ASOC_map.c), POLSTAT 0, 1 and 3, with
 * the map file's own traversal.  TEST INFRASTRUCTURE ONLY; compiled by tests/polmap_host.py in two math modes, like
 * oracle/soc_oracle.c:
 *   -DPM_LIBM  transcendentals from glibc libm: pinned bit for bit by tests/golden/polmaps.npz, the results of the
 *              reference's own kernels compiled for x86 (tools/make_polmap_golden.py);
 *   (default)  transcendentals from soc_amd/csrc/soc_math.h, the header the HIP kernel uses: what soc_polmap must equal.
 * -ffp-contract=off in both.  dot, length and normalize are what oracle/ref_builtins.inc gives the reference build.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef PM_LIBM
#  define M_EXP(x)      expf(x)
#  define M_SIN(x)      sinf(x)
#  define M_COS(x)      cosf(x)
#  define M_ACOS(x)     acosf(x)
#  define M_SQRT(x)     sqrtf(x)
#  define M_ATAN2(y, x) atan2f((y), (x))
#  define M_FMOD(x, y)  fmodf((x), (y))
#  define M_FMOD1(x)    fmodf((x), 1.0f)
#  define M_FMOD1D(x)   fmod((x), 1.0)
#  define M_FLOOR(x)    floorf(x)
#  define M_LDEXP_DN(x, l) ldexpf((x), -(l))
#  define M_SQUARE(x)   powf((x), 2.0f)               /* pow(x, 2.0f), as the reference build resolves it */
#else
#  include "../../soc_amd/csrc/soc_math.h"
#  define M_EXP(x)      soc_expf(x)
#  define M_SIN(x)      soc_sinf(x)
#  define M_COS(x)      soc_cosf(x)
#  define M_ACOS(x)     soc_acosf(x)
#  define M_SQRT(x)     soc_sqrtf(x)
#  define M_ATAN2(y, x) soc_atan2f((y), (x))
#  define M_FMOD(x, y)  soc_fmodf_small((x), (y))
#  define M_FMOD1(x)    soc_fmod1f(x)
#  define M_FMOD1D(x)   soc_fmod1d(x)
#  define M_FLOOR(x)    soc_floorf(x)
#  define M_LDEXP_DN(x, l) soc_scale_down((x), (l))
#  define M_SQUARE(x)   ((x) * (x))
#endif

/* kernel_ASOC_map.c:10-18 */
#define EPS    2.5e-4f
#define PEPS   5.0e-4f
#define PI     3.1415926536f
#define TWOPI  6.2831853072f
#define PIHALF 1.5707963268f

typedef struct { float x, y, z; } f3;

typedef struct {
    int   NX, NY, NZ, LEVELS;
    const int   *OFF, *PAR;
    const float *DENS;
    const float *OPT;                 /* -D WITH_ABU: [2*CELLS], else NULL */
    const float *Bx, *By, *Bz, *EMIT;
    int   polstat, polred, rho_weight, threshold;     /* -D POLSTAT, POLRED, POL_RHO_WEIGHT, LEVEL_THRESHOLD */
    float p00;
    int   NPIX_X, NPIX_Y;
    float MAP_DX, ABS, SCA, LENGTH;
    float DIR[3], RA[3], DE[3], CENTRE[3];
    float *MAP;                       /* [4*NPIX_Y*NPIX_X] */
    int   *NSTEPS;                    /* [NPIX_Y*NPIX_X] cell steps of (the first pass of) every ray, or NULL */
} pm_args;

static float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static float length3(f3 a) { return M_SQRT(a.x * a.x + a.y * a.y + a.z * a.z); }
static f3 normalize3(f3 v)
{
    float s = 1.0f / M_SQRT(v.x * v.x + v.y * v.y + v.z * v.z);
    f3 r = { v.x * s, v.y * s, v.z * s };
    return r;
}
static f3 neg3(f3 a) { f3 r = { -a.x, -a.y, -a.z };  return r; }

/* IndexG (:187-220) */
static void IndexG(const pm_args *M, f3 *pos, int *level, int *ind)
{
    const int NX = M->NX, NY = M->NY, NZ = M->NZ;
    const float *DENS = M->DENS;
    const int *OFF = M->OFF;
    *ind = -1;
    if ((pos->x <= 0.0f) || (pos->y <= 0.0f) || (pos->z <= 0.0f)) return;
    if ((pos->x >= NX) || (pos->y >= NY) || (pos->z >= NZ)) return;
    *level = 0;
    *ind = (int)M_FLOOR(pos->z) * NX * NY + (int)M_FLOOR(pos->y) * NX + (int)M_FLOOR(pos->x);
    if (DENS[*ind] > 0.0f) return;
    pos->x = 2.0f * M_FMOD1(pos->x);
    pos->y = 2.0f * M_FMOD1(pos->y);
    pos->z = 2.0f * M_FMOD1(pos->z);
    while (1) {
        float link = -DENS[OFF[*level] + (*ind)];
        int   li;
        memcpy(&li, &link, 4);
        *ind = li;
        (*level)++;
        *ind += 4 * (int)M_FLOOR(pos->z) + 2 * (int)M_FLOOR(pos->y) + (int)M_FLOOR(pos->x);
        if (DENS[OFF[*level] + (*ind)] > 0.0f) return;
        pos->x -= M_FLOOR(pos->x);
        pos->y -= M_FLOOR(pos->y);
        pos->z -= M_FLOOR(pos->z);
        pos->x *= 2.0f;  pos->y *= 2.0f;  pos->z *= 2.0f;
    }
}

/* Index (:294-377): POS in double when NX > 100 (:302-306).  The climb leaves an octet only for the root grid: the test
 * of :345 reads "(POS.z>=0.0)&&(POS.z<=0.0)", restated as written. */
#define PM_INDEX(NAME, REAL, RFLOOR, RFMOD1)                                                                            \
static void NAME(const pm_args *M, f3 *pos, int *level, int *ind)                                                       \
{                                                                                                                       \
    const int NX = M->NX, NY = M->NY, NZ = M->NZ;                                                                       \
    const float *DENS = M->DENS;                                                                                        \
    const int *OFF = M->OFF, *PAR = M->PAR;                                                                             \
    int  sid;                                                                                                           \
    REAL PX = pos->x, PY = pos->y, PZ = pos->z;                                                                         \
    if (*level == 0) {                                                                                                  \
        if ((pos->x <= 0.0f) || (pos->x >= NX) || (pos->y <= 0.0f) || (pos->y >= NY) || (pos->z <= 0.0f) || (pos->z >= NZ)) { \
            *ind = -1;  return;                                                                                         \
        }                                                                                                               \
        *ind = (int)M_FLOOR(pos->z) * NX * NY + (int)M_FLOOR(pos->y) * NX + (int)M_FLOOR(pos->x);                       \
        if (DENS[*ind] > 0.0f) return;                                                                                  \
    } else {                                                                                                            \
        while ((*level) > 0) {                                                                                          \
            *ind = PAR[OFF[*level] + (*ind) - NX * NY * NZ];                                                            \
            (*level)--;                                                                                                 \
            if ((*level) == 0) {                                                                                        \
                PX *= (REAL)0.5;  PY *= (REAL)0.5;  PZ *= (REAL)0.5;                                                    \
                PX += (*ind) % NX;  PY += ((*ind) / NX) % NY;  PZ += (*ind) / (NX * NY);                                \
                if ((PX <= 0.0) || (PX >= NX) || (PY <= 0.0) || (PY >= NY) || (PZ <= 0.0) || (PZ >= NZ)) {              \
                    *ind = -1;                                                                                          \
                    pos->x = PX;  pos->y = PY;  pos->z = PZ;                                                            \
                    return;                                                                                             \
                }                                                                                                       \
                *ind = (int)RFLOOR(PZ) * NX * NY + (int)RFLOOR(PY) * NX + (int)RFLOOR(PX);                              \
                if (DENS[*ind] > 0.0f) { pos->x = PX;  pos->y = PY;  pos->z = PZ;  return; }                            \
                break;                                                                                                  \
            } else {                                                                                                    \
                sid = (*ind) % 8;                                                                                       \
                PX *= (REAL)0.5;  PY *= (REAL)0.5;  PZ *= (REAL)0.5;                                                    \
                PX += sid % 2;  PY += (sid / 2) % 2;  PZ += sid / 4;                                                    \
                if ((PX >= 0.0) && (PX <= 2.0) && (PY >= 0.0) && (PY <= 2.0) && (PZ >= 0.0) && (PZ <= 0.0)) break;      \
            }                                                                                                           \
        }                                                                                                               \
    }                                                                                                                   \
    while (DENS[OFF[*level] + (*ind)] <= 0.0f) {                                                                        \
        PX = (REAL)2.0 * RFMOD1(PX);  PY = (REAL)2.0 * RFMOD1(PY);  PZ = (REAL)2.0 * RFMOD1(PZ);                        \
        float link = -DENS[OFF[*level] + (*ind)];                                                                       \
        int   li;                                                                                                       \
        memcpy(&li, &link, 4);                                                                                          \
        *ind = li;                                                                                                      \
        (*level)++;                                                                                                     \
        *ind += 4 * (int)RFLOOR(PZ) + 2 * (int)RFLOOR(PY) + (int)RFLOOR(PX);                                            \
    }                                                                                                                   \
    pos->x = PX;  pos->y = PY;  pos->z = PZ;                                                                            \
}
PM_INDEX(Index_f, float, M_FLOOR, M_FMOD1)
PM_INDEX(Index_d, double, floor, M_FMOD1D)

/* GetStep (:383-411) */
static float GetStep(const pm_args *M, f3 *POS, const f3 *DIR, int *level, int *ind)
{
    float dx, dy, dz;
    dx = (DIR->x > 0.0f) ? ((1.0f + PEPS - M_FMOD1(POS->x)) / DIR->x) : ((-PEPS - M_FMOD1(POS->x)) / DIR->x);
    dy = (DIR->y > 0.0f) ? ((1.0f + PEPS - M_FMOD1(POS->y)) / DIR->y) : ((-PEPS - M_FMOD1(POS->y)) / DIR->y);
    dz = (DIR->z > 0.0f) ? ((1.0f + PEPS - M_FMOD1(POS->z)) / DIR->z) : ((-PEPS - M_FMOD1(POS->z)) / DIR->z);
    dx = fminf(dx, fminf(dy, dz));
    POS->x += dx * DIR->x;
    POS->y += dx * DIR->y;
    POS->z += dx * DIR->z;
    dx = M_LDEXP_DN(dx, *level);
    if (M->NX > 100) Index_d(M, POS, level, ind);
    else             Index_f(M, POS, level, ind);
    return dx;
}

static int outside(const pm_args *M, f3 T)
{
    return (T.x <= 0.0f) || (T.x >= M->NX) || (T.y <= 0.0f) || (T.y >= M->NY) || (T.z <= 0.0f) || (T.z >= M->NZ);
}

static f3 madd(f3 p, float s, f3 d) { f3 r = { p.x + s * d.x, p.y + s * d.y, p.z + s * d.z };  return r; }

/* the ray's entry: :1011-1033 = :1199-1221 = :1631-1653 */
static f3 entry(const pm_args *M, int id, f3 DIR, f3 RA, f3 DE)
{
    const int NX = M->NX, NY = M->NY, NZ = M->NZ, NPX = M->NPIX_X, NPY = M->NPIX_Y;
    const float MAP_DX = M->MAP_DX;
    const int i = id % NPX, j = id / NPX;
    f3 POS;
    float sx, sy, sz;
    POS.x = M->CENTRE[0] + (i - 0.5f * (NPX - 1)) * MAP_DX * RA.x + (j - 0.5f * (NPY - 1)) * MAP_DX * DE.x;
    POS.y = M->CENTRE[1] + (i - 0.5f * (NPX - 1)) * MAP_DX * RA.y + (j - 0.5f * (NPY - 1)) * MAP_DX * DE.y;
    POS.z = M->CENTRE[2] + (i - 0.5f * (NPX - 1)) * MAP_DX * RA.z + (j - 0.5f * (NPY - 1)) * MAP_DX * DE.z;
    POS.x -= (NX + NY + NZ) * DIR.x;  POS.y -= (NX + NY + NZ) * DIR.y;  POS.z -= (NX + NY + NZ) * DIR.z;
    if (DIR.x >= 0.0f) sx = (NX - POS.x) / (DIR.x + 1.0e-10f) - EPS;  else sx = (0.0f - POS.x) / DIR.x - EPS;
    if (DIR.y >= 0.0f) sy = (NY - POS.y) / (DIR.y + 1.0e-10f) - EPS;  else sy = (0.0f - POS.y) / DIR.y - EPS;
    if (DIR.z >= 0.0f) sz = (NZ - POS.z) / (DIR.z + 1.0e-10f) - EPS;  else sz = (0.0f - POS.z) / DIR.z - EPS;
    if (outside(M, madd(POS, sx, DIR))) sx = -1e10f;
    if (outside(M, madd(POS, sy, DIR))) sy = -1e10f;
    if (outside(M, madd(POS, sz, DIR))) sz = -1e10f;
    sx = fmaxf(sx, fmaxf(sy, sz));
    return madd(POS, sx, DIR);
}

static float dtau_of(const pm_args *M, float sx, int oind)
{
    if (M->OPT) return sx * M->DENS[oind] * (M->OPT[2 * (long)oind] + M->OPT[2 * (long)oind + 1]);      /* :1068 */
    return sx * M->DENS[oind] * (M->SCA + M->ABS);                                                      /* :1070 */
}

static float emitted(const pm_args *M, float TAU, float DTAU, float sx, int oind, float rho)             /* :1095-1099 */
{
    if (DTAU < 1.0e-3f) return M_EXP(-TAU) * (1.0f - 0.5f * DTAU) * sx * M->EMIT[oind] * rho;
    return M_EXP(-TAU) * ((1.0f - M_EXP(-DTAU)) / DTAU) * sx * M->EMIT[oind] * rho;
}

/* -D POLSTAT=0 (:1060-1126) */
static void pixel_stat0(const pm_args *M, int id, f3 DIR, f3 RA, f3 DE)
{
    const long npix = (long)M->NPIX_X * M->NPIX_Y;
    float DTAU, TAU = 0.0f, colden = 0.0f, sx, sz;
    f3    PHOTONS = { 0.0f, 0.0f, 0.0f }, POS, TMP, BN;
    int   ind, level = 0, oind, olevel, steps = 0;
    POS = entry(M, id, DIR, RA, DE);
    TMP = neg3(DIR);
    IndexG(M, &POS, &level, &ind);
    float p = M->p00;
    while (ind >= 0) {
        oind   = M->OFF[level] + ind;
        olevel = level;
        sx     = GetStep(M, &POS, &TMP, &level, &ind);
        steps++;
        DTAU   = dtau_of(M, sx, oind);
        BN.x = M->Bx[oind];  BN.y = M->By[oind];  BN.z = M->Bz[oind];
        if (M->polred) p = length3(BN);                                   /* :1079-1081 */
        BN = normalize3(BN);
        float Psi = 0.5f * PI + M_ATAN2(dot3(BN, neg3(RA)), dot3(BN, DE));
        float cc  = 0.99999f - 0.99998f * dot3(BN, DIR) * dot3(BN, DIR);
        if (M->rho_weight) sz = sx * M->DENS[oind];                       /* :1092-1093 */
        else               sz = emitted(M, TAU, DTAU, sx, oind, M->DENS[oind]);
        if (olevel >= M->threshold) {                                     /* :1104; threshold 0 = the #else branch :1113-1115 */
            PHOTONS.x += sz * (1.0f - p * (cc - 0.6666667f));
            PHOTONS.y += p * sz * M_COS(2.0f * Psi) * cc;
            PHOTONS.z += p * sz * M_SIN(2.0f * Psi) * cc;
        }
        TAU    += DTAU;
        colden += sx * M->DENS[oind];
    }
    M->MAP[0 * npix + id] = PHOTONS.x;
    M->MAP[1 * npix + id] = PHOTONS.y;
    M->MAP[2 * npix + id] = PHOTONS.z;
    M->MAP[3 * npix + id] = colden * M->LENGTH;
    if (M->NSTEPS) M->NSTEPS[id] = steps;
}

/* -D POLSTAT=1 (:1224-1378) */
static void pixel_stat1(const pm_args *M, int id, f3 DIR, f3 RA, f3 DE)
{
    const long npix = (long)M->NPIX_X * M->NPIX_Y;
    float DTAU, TAU = 0.0f, sx, sz;
    f3    POS, TMP, BN;
    int   ind, level = 0, oind, olevel, steps = 0;
    POS = entry(M, id, DIR, RA, DE);
    TMP = neg3(DIR);
    f3 POS0 = POS;
    IndexG(M, &POS, &level, &ind);
    float sR = 0.0f, sJ = 0.0f, sRG = 0.0f, sJG = 0.0f, RQ = 0.0f, RU = 0.0f, JQ = 0.0f, JU = 0.0f, sRP, sJP, d, PR;
    while (ind >= 0) {
        oind   = M->OFF[level] + ind;
        olevel = level;
        sx     = GetStep(M, &POS, &TMP, &level, &ind);
        steps++;
        DTAU   = dtau_of(M, sx, oind);
        BN.x = M->Bx[oind];  BN.y = M->By[oind];  BN.z = M->Bz[oind];
        PR = length3(BN);
        BN = normalize3(BN);
        float Psi = 0.5f * PI + M_ATAN2(dot3(BN, neg3(RA)), dot3(BN, DE));
        float cc  = 0.99999f - 0.99998f * dot3(BN, DIR) * dot3(BN, DIR);
        float rho = M->DENS[oind];
        sz = emitted(M, TAU, DTAU, sx, oind, rho);
        if (olevel < M->threshold) { sz = 0.0f;  rho = 0.0f; }            /* :1263 */
        if (M->polred) {                                                  /* :1274-1282 */
            sR  += rho * sx * PR;
            sRG += rho * sx * PR * cc;
            RQ  += rho * sx * PR * M_COS(2.0f * Psi) * cc;
            RU  += rho * sx * PR * M_SIN(2.0f * Psi) * cc;
            sJ  += sz * PR;
            sJG += sz * PR * cc;
            JQ  += sz * PR * M_COS(2.0f * Psi) * cc;
            JU  += sz * PR * M_SIN(2.0f * Psi) * cc;
        } else {                                                          /* :1286-1293 */
            sR  += rho * sx;
            sRG += rho * sx * cc;
            RQ  += rho * sx * M_COS(2.0f * Psi) * cc;
            RU  += rho * sx * M_SIN(2.0f * Psi) * cc;
            sJ  += sz;
            sJG += sz * cc;
            JQ  += sz * M_COS(2.0f * Psi) * cc;
            JU  += sz * M_SIN(2.0f * Psi) * cc;
        }
        TAU += DTAU;
    }
    M->MAP[1 * npix + id] = M_ACOS(M_SQRT(sRG / sR));
    M->MAP[3 * npix + id] = M_ACOS(M_SQRT(sJG / sJ));
    float RChi = 0.5 * M_ATAN2(RU, RQ);                                   /* double literal (:1305-1306) */
    float JChi = 0.5 * M_ATAN2(JU, JQ);
    POS = POS0;
    IndexG(M, &POS, &level, &ind);
    TAU = 0.0f;
    sRP = 0.0f;  sJP = 0.0f;  sR = 0.0f;  sJ = 0.0f;
    while (ind >= 0) {
        oind   = M->OFF[level] + ind;
        olevel = level;
        sx     = GetStep(M, &POS, &TMP, &level, &ind);
        DTAU   = dtau_of(M, sx, oind);
        BN.x = M->Bx[oind];  BN.y = M->By[oind];  BN.z = M->Bz[oind];
        PR = length3(BN);
        BN = normalize3(BN);
        float Chi = 0.5f * PI + M_ATAN2(dot3(BN, neg3(RA)), dot3(BN, DE));
        float rho = M->DENS[oind];
        sz = emitted(M, TAU, DTAU, sx, oind, rho);
        if (olevel < M->threshold) { sz = 0.0f;  rho = 0.0f; }            /* :1339 */
        if (M->polred) {                                                  /* :1349-1356 */
            sR  += rho * PR * sx;
            d    = M_FMOD(fabsf(TWOPI + RChi - Chi), PI);
            if (d > PIHALF) d = PI - d;
            sRP += rho * PR * sx * d * d;
            sJ  += sz * PR;
            d    = M_FMOD(fabsf(TWOPI + JChi - Chi), PI);
            if (d > PIHALF) d = PI - d;
            sJP += sz * PR * d * d;
        } else {                                                          /* :1358-1365 */
            sR  += rho * sx;
            d    = M_FMOD(fabsf(TWOPI + RChi - Chi), PI);
            if (d > PIHALF) d = PI - d;
            sRP += rho * sx * d * d;
            sJ  += sz;
            d    = M_FMOD(fabsf(TWOPI + JChi - Chi), PI);
            if (d > PIHALF) d = PI - d;
            sJP += sz * d * d;
        }
        TAU += DTAU;
    }
    M->MAP[0 * npix + id] = M_SQRT(sRP / sR);
    M->MAP[2 * npix + id] = M_SQRT(sJP / sJ);
    if (M->NSTEPS) M->NSTEPS[id] = steps;
}

/* -D POLSTAT=3 (:1655-1687) */
static void pixel_stat3(const pm_args *M, int id, f3 DIR, f3 RA, f3 DE)
{
    const long npix = (long)M->NPIX_X * M->NPIX_Y;
    float DTAU, TAU = 0.0f, SUM_BPOS = 0.0f, SUM_BLOS = 0.0f, SUM_B = 0.0f, WEIGHT = 0.0, rho, sx;
    f3    POS, TMP, BN;
    int   ind, level = 0, oind, olevel, steps = 0;
    POS = entry(M, id, DIR, RA, DE);
    TMP = neg3(DIR);
    IndexG(M, &POS, &level, &ind);
    while (ind >= 0) {
        oind   = M->OFF[level] + ind;
        olevel = level;
        sx     = GetStep(M, &POS, &TMP, &level, &ind);
        steps++;
        DTAU   = dtau_of(M, sx, oind);
        BN.x = M->Bx[oind];  BN.y = M->By[oind];  BN.z = M->Bz[oind];
        rho = M->DENS[oind];
        if (olevel < M->threshold) rho = 0.0f;                            /* :1674 */
        WEIGHT   += sx * rho;
        SUM_B    += sx * rho * length3(BN);
        SUM_BLOS += sx * rho * fabsf(dot3(BN, TMP));
        SUM_BPOS += sx * rho * M_SQRT(M_SQUARE(dot3(BN, neg3(RA))) + M_SQUARE(dot3(BN, DE)));
        TAU      += DTAU;
    }
    M->MAP[0 * npix + id] = SUM_B / WEIGHT;
    M->MAP[1 * npix + id] = SUM_BLOS / WEIGHT;
    M->MAP[2 * npix + id] = SUM_BPOS / WEIGHT;
    M->MAP[3 * npix + id] = TAU;
    if (M->NSTEPS) M->NSTEPS[id] = steps;
}

/* all pixels of one map; 0, or -1 for a POLSTAT that is not restated */
int pm_polmap(const pm_args *M)
{
    const int npix = M->NPIX_X * M->NPIX_Y;
    const f3 DIR = { M->DIR[0], M->DIR[1], M->DIR[2] }, RA = { M->RA[0], M->RA[1], M->RA[2] }, DE = { M->DE[0], M->DE[1], M->DE[2] };
    if (M->polstat != 0 && M->polstat != 1 && M->polstat != 3) return -1;
#pragma omp parallel for schedule(dynamic, 64)
    for (int id = 0; id < npix; id++) {
        if (M->polstat == 0)      pixel_stat0(M, id, DIR, RA, DE);
        else if (M->polstat == 1) pixel_stat1(M, id, DIR, RA, DE);
        else                      pixel_stat3(M, id, DIR, RA, DE);
    }
    return 0;
}

/* the fmod of this build: libm's, or soc_math.h's */
void pm_fmod(const float *x, const float *y, float *r, long n)
{
    for (long i = 0; i < n; i++) r[i] = M_FMOD(x[i], y[i]);
}
