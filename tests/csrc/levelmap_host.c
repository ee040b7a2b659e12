/* levelmap_host.c -- CPU restatement of the per-level Mapping kernel of the reference's kernel_ASOC_map_H.c (:380-497, `mapping
 * nx ny dx 999`) with that file's own traversal (:179-326).  TEST INFRASTRUCTURE ONLY; compiled by tests/levelmap_host.py in two
 * math modes, like tests/csrc/polmap_host.c:
 *   -DPM_LIBM  transcendentals from glibc libm: pinned bit for bit by tests/golden/levelmaps.npz, the results of the
 *              reference's own kernel compiled for x86 (tools/make_levelmap_golden.py);
 *   (default)  transcendentals from soc_amd/csrc/soc_math.h, the header the HIP kernel uses: what soc_map_levels must equal.
 * -ffp-contract=off in both.
 * Two things are not the reference's: the per-cell opacities (OPT; that file has the line under "#ifdef USE_ABU", :474-478,
 * which nothing defines -- and which cannot be defined: another kernel of the file then fails to compile, :553), and the end
 * of a ray after LM_MAXSTEPS steps (the reference has no limit).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef PM_LIBM
#  define M_EXP(x)      expf(x)
#  define M_SIN(x)      sinf(x)
#  define M_COS(x)      cosf(x)
#  define M_FMOD1(x)    fmodf((x), 1.0f)
#  define M_FMOD1D(x)   fmod((x), 1.0)
#  define M_FLOOR(x)    floorf(x)
#  define M_LDEXP_DN(x, l) ldexpf((x), -(l))
#else
#  include "../../soc_amd/csrc/soc_math.h"
#  define M_EXP(x)      soc_expf(x)
#  define M_SIN(x)      soc_sinf(x)
#  define M_COS(x)      soc_cosf(x)
#  define M_FMOD1(x)    soc_fmod1f(x)
#  define M_FMOD1D(x)   soc_fmod1d(x)
#  define M_FLOOR(x)    soc_floorf(x)
#  define M_LDEXP_DN(x, l) soc_scale_down((x), (l))
#endif

/* kernel_ASOC_map_H.c:10-11, :31-32 */
#define EPS    2.5e-4f
#define PEPS   5.0e-4f
#define PI     3.1415926536f
#define TWOPI  6.2831853072f

#define LM_MAXSTEPS (1 << 15)         /* = SOC_MAPLEV_MAXSTEPS of soc_amd/csrc/soc_dev.h */
#define LM_MAXL     16                /* = SOC_MAXL */

typedef struct { float x, y, z; } f3;

typedef struct {
    int   NX, NY, NZ, LEVELS;
    const int   *OFF, *PAR;
    const float *DENS;
    const float *OPT;                 /* [2*CELLS] or NULL */
    const float *EMIT;
    int   NPIX_X, NPIX_Y;
    float MAP_DX, ABS, SCA;
    float DIR[3], RA[3], DE[3], CENTRE[3], INTOBS[3];
    float *MAP;                       /* [LEVELS*NPIX_Y*NPIX_X] */
    int   *NSTEPS;                    /* [NPIX_Y*NPIX_X] cell steps of every ray, or NULL */
} lm_args;

/* IndexG (:179-212): the text of kernel_ASOC_map.c's */
static void IndexG(const lm_args *M, f3 *pos, int *level, int *ind)
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

/* Index (:216-289): POS in double when NX > 100 (:222-226).  Not kernel_ASOC_map.c's: where the climb ends on the root grid
 * the position is NOT written back -- neither when the ray left the model (:246-248) nor when the root cell is a leaf
 * (:252) -- so the ray goes on at level 0 with the octet's local coordinates.  The octet test of :261-262 reads
 * "(POS.z>=0.0f)&&(POS.z<=0.0f)", as in the other file. */
#define LM_INDEX(NAME, REAL, RFLOOR, RFMOD1)                                                                            \
static void NAME(const lm_args *M, f3 *pos, int *level, int *ind)                                                       \
{                                                                                                                       \
    const int NX = M->NX, NY = M->NY, NZ = M->NZ;                                                                       \
    const float *DENS = M->DENS;                                                                                        \
    const int *OFF = M->OFF, *PAR = M->PAR;                                                                             \
    int  sid;                                                                                                           \
    REAL PX = pos->x, PY = pos->y, PZ = pos->z;                                                                         \
    if (*level == 0) {                                                                                                  \
        if ((PX <= 0.0f) || (PX >= NX) || (PY <= 0.0f) || (PY >= NY) || (PZ <= 0.0f) || (PZ >= NZ)) {                   \
            *ind = -1;  return;                                                                                         \
        }                                                                                                               \
        *ind = (int)RFLOOR(PZ) * NX * NY + (int)RFLOOR(PY) * NX + (int)RFLOOR(PX);                                      \
        if (DENS[*ind] > 0.0f) return;                                                                                  \
    } else {                                                                                                            \
        while ((*level) > 0) {                                                                                          \
            *ind = PAR[OFF[*level] + (*ind) - NX * NY * NZ];                                                            \
            *level -= 1;                                                                                                \
            if ((*level) == 0) {                                                                                        \
                PX *= (REAL)0.5;  PY *= (REAL)0.5;  PZ *= (REAL)0.5;                                                    \
                PX += (*ind) % NX;  PY += ((*ind) / NX) % NY;  PZ += (*ind) / (NX * NY);                                \
                if ((PX <= 0.0f) || (PX >= NX) || (PY <= 0.0f) || (PY >= NY) || (PZ <= 0.0f) || (PZ >= NZ)) {           \
                    *ind = -1;  return;                                                                                 \
                }                                                                                                       \
                *ind = (int)RFLOOR(PZ) * NX * NY + (int)RFLOOR(PY) * NX + (int)RFLOOR(PX);                              \
                if (DENS[*ind] > 0.0f) return;                                                                          \
                break;                                                                                                  \
            } else {                                                                                                    \
                sid = (*ind) % 8;                                                                                       \
                PX *= (REAL)0.5;  PY *= (REAL)0.5;  PZ *= (REAL)0.5;                                                    \
                PX += sid % 2;  PY += (sid / 2) % 2;  PZ += sid / 4;                                                    \
                if ((PX >= 0.0f) && (PX <= 2.0f) && (PY >= 0.0f) && (PY <= 2.0f) && (PZ >= 0.0f) && (PZ <= 0.0f)) break; \
            }                                                                                                           \
        }                                                                                                               \
    }                                                                                                                   \
    while (DENS[OFF[*level] + (*ind)] <= 0.0f) {                                                                        \
        PX = (REAL)2.0 * RFMOD1(PX);  PY = (REAL)2.0 * RFMOD1(PY);  PZ = (REAL)2.0 * RFMOD1(PZ);                        \
        float link = -DENS[OFF[*level] + (*ind)];                                                                       \
        int   li;                                                                                                       \
        memcpy(&li, &link, 4);                                                                                          \
        *ind = li;                                                                                                      \
        *level += 1;                                                                                                    \
        *ind += 4 * (int)RFLOOR(PZ) + 2 * (int)RFLOOR(PY) + (int)RFLOOR(PX);                                            \
    }                                                                                                                   \
    pos->x = PX;  pos->y = PY;  pos->z = PZ;                                                                            \
}
LM_INDEX(Index_f, float, M_FLOOR, M_FMOD1)
LM_INDEX(Index_d, double, floor, M_FMOD1D)

/* GetStep (:297-326) */
static float GetStep(const lm_args *M, f3 *POS, const f3 *DIR, int *level, int *ind)
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

static int outside(const lm_args *M, f3 T)
{
    return (T.x <= 0.0f) || (T.x >= M->NX) || (T.y <= 0.0f) || (T.y >= M->NY) || (T.z <= 0.0f) || (T.z >= M->NZ);
}

static f3 madd(f3 p, float s, f3 d) { f3 r = { p.x + s * d.x, p.y + s * d.y, p.z + s * d.z };  return r; }

static void pixel(const lm_args *M, int id)
{
    const int   NX = M->NX, NY = M->NY, NZ = M->NZ, NPX = M->NPIX_X, NPY = M->NPIX_Y, LEVELS = M->LEVELS;
    const float *DENS = M->DENS, *EMIT = M->EMIT;
    const int   *OFF = M->OFF;
    const float DX = M->MAP_DX;
    const f3    DIR = { M->DIR[0], M->DIR[1], M->DIR[2] }, RA = { M->RA[0], M->RA[1], M->RA[2] }, DE = { M->DE[0], M->DE[1], M->DE[2] };
    const long  npix = (long)NPX * NPY;
    float DTAU, TAU = 0.0f, PHOTONS[LM_MAXL], sx, sy, sz;
    f3    POS, TMP;
    int   ind, level = 0, oind, olevel, steps = 0;
    const int i = id % NPX, j = id / NPX;
    for (int ilev = 0; ilev < LEVELS; ilev++) PHOTONS[ilev] = 0.0f;
    if (M->INTOBS[0] > -1e10) {                                           /* :412-434 */
        float phi = TWOPI * i / (float)(NPX);
        phi += PI;
        float pix = TWOPI / NPX;
        float theta = pix * (j - (NPY - 1) / 2);
        POS.x = M->INTOBS[0];  POS.y = M->INTOBS[1];  POS.z = M->INTOBS[2];
        TMP.x = -M_COS(theta) * M_SIN(phi);
        TMP.y = -M_COS(theta) * M_COS(phi);
        TMP.z = +M_SIN(theta);
        if (fabsf(TMP.x) < 1.0e-5f) TMP.x = 1.0e-5f;
        if (fabsf(TMP.y) < 1.0e-5f) TMP.y = 1.0e-5f;
        if (fabsf(TMP.z) < 1.0e-5f) TMP.z = 1.0e-5f;
        if (M_FMOD1(POS.x) < 1.0e-5f) POS.x += 2.0e-5f;
        if (M_FMOD1(POS.y) < 1.0e-5f) POS.y += 2.0e-5f;
        if (M_FMOD1(POS.z) < 1.0e-5f) POS.z += 2.0e-5f;
    } else {                                                              /* :436-460 */
        POS.x = M->CENTRE[0] + (i - 0.5f * (NPX - 1)) * DX * RA.x + (j - 0.5f * (NPY - 1)) * DX * DE.x;
        POS.y = M->CENTRE[1] + (i - 0.5f * (NPX - 1)) * DX * RA.y + (j - 0.5f * (NPY - 1)) * DX * DE.y;
        POS.z = M->CENTRE[2] + (i - 0.5f * (NPX - 1)) * DX * RA.z + (j - 0.5f * (NPY - 1)) * DX * DE.z;
        POS.x -= (NX + NY + NZ) * DIR.x;  POS.y -= (NX + NY + NZ) * DIR.y;  POS.z -= (NX + NY + NZ) * DIR.z;
        if (DIR.x >= 0.0f) sx = (NX - POS.x) / (DIR.x + 1.0e-10f) - EPS;  else sx = (0.0f - POS.x) / DIR.x - EPS;
        if (DIR.y >= 0.0f) sy = (NY - POS.y) / (DIR.y + 1.0e-10f) - EPS;  else sy = (0.0f - POS.y) / DIR.y - EPS;
        if (DIR.z >= 0.0f) sz = (NZ - POS.z) / (DIR.z + 1.0e-10f) - EPS;  else sz = (0.0f - POS.z) / DIR.z - EPS;
        if (outside(M, madd(POS, sx, DIR))) sx = -1e10f;
        if (outside(M, madd(POS, sy, DIR))) sy = -1e10f;
        if (outside(M, madd(POS, sz, DIR))) sz = -1e10f;
        sx  = fmaxf(sx, fmaxf(sy, sz));
        POS = madd(POS, sx, DIR);
        TMP.x = -DIR.x;  TMP.y = -DIR.y;  TMP.z = -DIR.z;
    }
    IndexG(M, &POS, &level, &ind);
    while ((ind >= 0) && (steps < LM_MAXSTEPS)) {
        steps++;
        oind   = OFF[level] + ind;
        olevel = level;
        sx     = GetStep(M, &POS, &TMP, &level, &ind);
        if (M->OPT) DTAU = sx * DENS[oind] * (M->OPT[2 * (long)oind] + M->OPT[2 * (long)oind + 1]);     /* :475 */
        else        DTAU = sx * DENS[oind] * (M->SCA + M->ABS);                                         /* :477 */
        if (DTAU < 1.0e-3f) PHOTONS[olevel] += M_EXP(-TAU) * (1.0f - 0.5f * DTAU) * sx * EMIT[oind] * DENS[oind];
        else                PHOTONS[olevel] += M_EXP(-TAU) * ((1.0f - M_EXP(-DTAU)) / DTAU) * sx * EMIT[oind] * DENS[oind];
        TAU += DTAU;
    }
    for (int ilev = 0; ilev < LEVELS; ilev++) M->MAP[ilev * npix + id] = PHOTONS[ilev];
    if (M->NSTEPS) M->NSTEPS[id] = steps;
}

/* all pixels of one view; 0, or -1 for more levels than the kernel takes */
int lm_levelmap(const lm_args *M)
{
    const int npix = M->NPIX_X * M->NPIX_Y;
    if (M->LEVELS < 1 || M->LEVELS > LM_MAXL) return -1;
#pragma omp parallel for schedule(dynamic, 64)
    for (int id = 0; id < npix; id++) pixel(M, id);
    return 0;
}
