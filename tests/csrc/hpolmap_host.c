/* hpolmap_host.c -- CPU restatement of the reference's PolHealpixMapping kernel (kernel_ASOC_map_H.c:576-841, -D POLSTAT=0)
 * with that file's own traversal (:179-326).  TEST INFRASTRUCTURE ONLY; compiled by tests/hpolmap_host.py in two math modes,
 * like tests/csrc/polmap_host.c:
 *   -DPM_LIBM  transcendentals from glibc libm: pinned bit for bit by tests/golden/hpolmaps.npz, the results of the
 *              reference's own kernel compiled for x86 (tools/make_hpolmap_golden.py);
 *   (default)  transcendentals from soc_amd/csrc/soc_math.h, the header the HIP kernel uses: what soc_polmap_healpix must equal.
 * -ffp-contract=off in both.  dot, length and normalize are what oracle/ref_builtins.inc gives the reference build.
 * Two things are not the reference's: the per-cell opacities (use_opt; that file has the line under "#ifdef USE_ABU", :736-740,
 * which nothing defines -- and which cannot be defined: another kernel of the file then fails to compile, :553), and the end
 * of a ray after HP_MAXSTEPS steps (the reference has no limit).
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
#  define M_POWHALF(l)  powf(0.5f, (float)(l))
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
#  define M_POWHALF(l)  soc_scale_down(1.0f, (l))
#endif

/* kernel_ASOC_map_H.c:10-11, :31-34 */
#define PEPS   5.0e-4f
#define PI     3.1415926536f

#define HP_MAXSTEPS (1 << 15)         /* = SOC_HPOL_MAXSTEPS of soc_amd/csrc/soc_dev.h */

typedef struct { float x, y, z; } f3;

typedef struct {
    int   NX, NY, NZ, LEVELS;
    const int   *OFF, *PAR;
    const float *DENS;
    const float *OPT;                 /* [2*CELLS] or NULL */
    const float *Bx, *By, *Bz, *EMIT;
    int   NSIDE, polred, threshold, interpolate;      /* -D NSIDE, POLRED, LEVEL_THRESHOLD, INTERPOLATE */
    float p00, MINLOS, MAXLOS, Y_SHEAR;
    float ABS, SCA, LENGTH;
    float INTOBS[3];
    float *MAP;                       /* [4*12*NSIDE*NSIDE] */
    int   *NSTEPS;                    /* [12*NSIDE*NSIDE] cell steps of every ray, or NULL */
} hp_args;

static float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static float length3(f3 a) { return M_SQRT(a.x * a.x + a.y * a.y + a.z * a.z); }
static f3 normalize3(f3 v)
{
    float s = 1.0f / M_SQRT(v.x * v.x + v.y * v.y + v.z * v.z);
    f3 r = { v.x * s, v.y * s, v.z * s };
    return r;
}
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a < b ? b : a; }
static int iclamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

/* Pixel2AnglesRing (:93-132) */
static void Pixel2AnglesRing(int NSIDE, const int ipix, float *phi, float *theta)
{
    int   nl2, nl4, npix, ncap, iring, iphi, ip, ipix1;
    float fact1, fact2, fodd, hip, fihip;
    npix  = 12 * NSIDE * NSIDE;
    ipix1 = ipix + 1;
    nl2   = 2 * NSIDE;
    nl4   = 4 * NSIDE;
    ncap  = 2 * NSIDE * (NSIDE - 1);
    fact1 = 1.5f * NSIDE;
    fact2 = 3.0f * NSIDE * NSIDE;
    if (ipix1 <= ncap) {
        hip   = ipix1 / 2.0f;
        fihip = (int)(hip);
        iring = (int)(M_SQRT(hip - M_SQRT(fihip))) + 1;
        iphi  = ipix1 - 2 * iring * (iring - 1);
        *theta = M_ACOS(1.0f - iring * iring / fact2);
        *phi   = (iphi - 0.5f) * PI / (2.0f * iring);
    } else if (ipix1 <= nl2 * (5 * NSIDE + 1)) {
        ip    = ipix1 - ncap - 1;
        iring = (int)(ip / nl4) + NSIDE;
        iphi  = (ip % nl4) + 1;
        fodd  = 0.5f * (1 + (iring + NSIDE) % 2);
        *theta = M_ACOS((nl2 - iring) / fact1);
        *phi   = (iphi - fodd) * PI / (2.0f * NSIDE);
    } else {
        ip    = npix - ipix1 + 1;
        hip   = ip / 2.0f;
        fihip = (int)(hip);
        iring = (int)(M_SQRT(hip - M_SQRT(fihip))) + 1;
        iphi  = 4 * iring + 1 - (ip - 2 * iring * (iring - 1));
        *theta = M_ACOS(-1.0f + iring * iring / fact2);
        *phi   = (iphi - 0.5f) * PI / (2.0f * iring);
    }
}

/* IndexG (:179-212): the text of kernel_ASOC_map.c's */
static void IndexG(const hp_args *M, f3 *pos, int *level, int *ind)
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
#define HP_INDEX(NAME, REAL, RFLOOR, RFMOD1)                                                                            \
static void NAME(const hp_args *M, f3 *pos, int *level, int *ind)                                                       \
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
HP_INDEX(Index_f, float, M_FLOOR, M_FMOD1)
HP_INDEX(Index_d, double, floor, M_FMOD1D)

/* GetStep (:297-326) */
static float GetStep(const hp_args *M, f3 *POS, const f3 *DIR, int *level, int *ind)
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

static void pixel(const hp_args *M, int id)
{
    const int   NX = M->NX, NY = M->NY, NZ = M->NZ, NSIDE = M->NSIDE;
    const float *DENS = M->DENS, *EMIT = M->EMIT;
    const int   *OFF = M->OFF;
    const float MAXLOS = M->MAXLOS, MINLOS = M->MINLOS, Y_SHEAR = M->Y_SHEAR;
    const int   INTERPOLATE = M->interpolate;
    const long  npix = 12L * NSIDE * NSIDE;
    float DTAU, TAU = 0.0f, colden = 0.0f, dens;
    f3    PHOTONS = { 0.0f, 0.0f, 0.0f }, POS, HDIR, BN, MPOS, mpos, HRA, HDE;
    float sx, sz, phi, theta, los = 0.0f, sum, w, weight, delta;
    int   ind, level = 0, oind, olevel, i0, j0, k0, mlevel = 0, mind, steps = 0;
    Pixel2AnglesRing(NSIDE, id, &phi, &theta);
    HDIR.x = +M_SIN(theta) * M_COS(phi);
    HDIR.y = +M_SIN(theta) * M_SIN(phi);
    HDIR.z = -M_COS(theta);
    if (fabsf(HDIR.x) < 1.0e-5f) HDIR.x = 1.0e-5f;
    if (fabsf(HDIR.y) < 1.0e-5f) HDIR.y = 1.0e-5f;
    if (fabsf(HDIR.z) < 1.0e-5f) HDIR.z = 1.0e-5f;
    POS.x = M->INTOBS[0];  POS.y = M->INTOBS[1];  POS.z = M->INTOBS[2];
    if ((M_FMOD1(POS.x) < 1.0e-5f) || (M_FMOD1(POS.x) < 0.99999f)) POS.x += 2.0e-5f;      /* :623-625, as written */
    if ((M_FMOD1(POS.y) < 1.0e-5f) || (M_FMOD1(POS.y) < 0.99999f)) POS.y += 2.0e-5f;
    if ((M_FMOD1(POS.z) < 1.0e-5f) || (M_FMOD1(POS.z) < 0.99999f)) POS.z += 2.0e-5f;
    IndexG(M, &POS, &level, &ind);
    HRA.x = -M_SIN(phi);
    HRA.y = +M_COS(phi);
    HRA.z = 0.0f;
    HDE.x = -M_COS(theta) * M_COS(phi);
    HDE.y = -M_COS(theta) * M_SIN(phi);
    HDE.z = +M_SIN(theta);
    float p = M->p00;
    while ((ind >= 0) && (steps < HP_MAXSTEPS)) {
        steps++;
        oind   = OFF[level] + ind;
        olevel = level;
        MPOS   = POS;
        sx     = GetStep(M, &POS, &HDIR, &level, &ind);
        dens   = DENS[oind];
        if (INTERPOLATE > 0) {
            const float h = 0.5f * sx;
            MPOS.x = MPOS.x + h * HDIR.x;  MPOS.y = MPOS.y + h * HDIR.y;  MPOS.z = MPOS.z + h * HDIR.z;
        }
        if (INTERPOLATE == 1) {                                           /* :654-682 */
            i0 = iclamp((int)M_FLOOR(MPOS.x), 0, NX - 1);
            j0 = iclamp((int)M_FLOOR(MPOS.y), 0, NY - 1);
            k0 = iclamp((int)M_FLOOR(MPOS.z), 0, NZ - 1);
            MPOS.x = M_FMOD1(MPOS.x) - 0.5f;
            MPOS.y = M_FMOD1(MPOS.y) - 0.5f;
            MPOS.z = M_FMOD1(MPOS.z) - 0.5f;
            sum = (3.0f - fabsf(MPOS.x) - fabsf(MPOS.y) - fabsf(MPOS.z)) * dens;
            if (MPOS.x > 0.0f) sum += MPOS.x * DENS[k0 * NX * NY + j0 * NX + imax(0, i0 - 1)];
            else               sum += -MPOS.x * DENS[k0 * NX * NY + j0 * NX + imin(i0 + 1, NX - 1)];
            if (MPOS.y > 0.0f) sum += +MPOS.y * DENS[k0 * NX * NY + imax(j0 - 1, 0) * NX + i0];
            else               sum += -MPOS.y * DENS[k0 * NX * NY + imin(j0 + 1, NY - 1) * NX + i0];
            if (MPOS.z > 0.0f) sum += +MPOS.z * DENS[imax(k0 - 1, 0) * NX * NY + j0 * NX + i0];
            else               sum += -MPOS.z * DENS[imin(k0 + 1, NZ - 1) * NX * NY + j0 * NX + i0];
            dens = 0.333333f * sum;
        }
        if (INTERPOLATE == 2) {                                           /* :686-707 */
            i0 = (int)M_FLOOR(MPOS.x);
            j0 = (int)M_FLOOR(MPOS.y);
            k0 = (int)M_FLOOR(MPOS.z);
            sum = 0.0f;
            weight = 0.0f;
            for (int k = imax(0, k0 - 1); k < imin(k0 + 2, NZ); k++) {
                for (int j = imax(0, j0 - 1); j < imin(j0 + 2, NY); j++) {
                    for (int i = imax(0, i0 - 1); i < imin(i0 + 2, NX); i++) {
                        mpos.x = MPOS.x - (i + 0.5f);
                        mpos.y = MPOS.y - (j + 0.5f);
                        mpos.z = MPOS.z - (k + 0.5f);
                        w = 1.0f / (0.1f + length3(mpos));
                        weight += w;
                        sum += w * DENS[k * NY * NX + j * NX + i];
                    }
                }
            }
            dens = sum / weight;
        }
        if (INTERPOLATE == 3) {                                           /* :711-733 */
            sum = 0.0f;
            weight = 0.0f;
            delta = M_POWHALF(olevel);
            for (int k = -1; k < 2; k++) {
                for (int j = -1; j < 2; j++) {
                    for (int i = -1; i < 2; i++) {
                        mpos.x = MPOS.x + i * delta;
                        mpos.y = MPOS.y + j * delta;
                        mpos.z = MPOS.z + k * delta;
                        IndexG(M, &mpos, &mlevel, &mind);
                        if (mind >= 0) {
                            w = 1.0f / M_SQRT(0.2f + i * i + j * j + k * k);
                            weight += w;
                            sum += w * DENS[OFF[mlevel] + mind];
                        }
                    }
                }
            }
            dens = sum / weight;
        }
        if (M->OPT) DTAU = sx * dens * (M->OPT[2 * (long)oind] + M->OPT[2 * (long)oind + 1]);     /* :737 */
        else        DTAU = sx * dens * (M->SCA + M->ABS);                                         /* :739 */
        los += sx;
        if (los > MAXLOS) {                                               /* :743-746 */
            ind = -1;  POS.z = -1.0f;
            sx = MAXLOS - (los - sx);
        }
        BN.x = M->Bx[oind];  BN.y = M->By[oind];  BN.z = M->Bz[oind];
        if (M->polred) p = length3(BN);
        BN = normalize3(BN);
        float Psi = 0.5 * PI + M_ATAN2(dot3(BN, HRA), dot3(BN, HDE));     /* double literal (:768) */
        float cc  = 0.99999f - 0.99998f * dot3(BN, HDIR) * dot3(BN, HDIR);
        if (DTAU < 1.0e-3f) sz = M_EXP(-TAU) * (1.0f - 0.5f * DTAU) * sx * EMIT[oind] * dens;
        else                sz = M_EXP(-TAU) * ((1.0f - M_EXP(-DTAU)) / DTAU) * sx * EMIT[oind] * dens;
        if (los < MINLOS) continue;                                       /* :776 */
        if (olevel >= M->threshold) {                                     /* :778-791 */
            PHOTONS.x += sz * (1.0f - p * (cc - 0.6666667f));
            PHOTONS.y += p * sz * M_COS(2.0f * Psi) * cc;
            PHOTONS.z += p * sz * M_SIN(2.0f * Psi) * cc;
        }
        TAU    += DTAU;
        colden += sx * dens;
        if (Y_SHEAR != 0.0f) {                                            /* :800-826 */
            if ((ind < 0) && (los < MAXLOS)) {
                if ((POS.z > 0.0f) && (POS.z < NZ)) {
                    if (POS.y < 0.0f) POS.y = NY - PEPS;
                    if (POS.y > NY)   POS.y = +PEPS;
                    if (POS.x < 0.0f) { POS.x = NX - PEPS;  POS.y = M_FMOD(POS.y + NY - Y_SHEAR, (float)NY); }
                    if (POS.x > NX)   { POS.x = +PEPS;      POS.y = M_FMOD(POS.y + Y_SHEAR, (float)NY); }
                    IndexG(M, &POS, &level, &ind);
                }
            }
        }
    }
    M->MAP[0 * npix + id] = PHOTONS.x;
    M->MAP[1 * npix + id] = PHOTONS.y;
    M->MAP[2 * npix + id] = PHOTONS.z;
    M->MAP[3 * npix + id] = colden * M->LENGTH;
    if (M->NSTEPS) M->NSTEPS[id] = steps;
}

/* all pixels of one map; 0, or -1 for switches the kernel does not take */
int hp_polmap(const hp_args *M)
{
    const int npix = 12 * M->NSIDE * M->NSIDE;
    if (M->interpolate < 0 || M->interpolate > 3) return -1;
    if ((M->interpolate == 1 || M->interpolate == 2) && M->LEVELS > 1) return -1;
#pragma omp parallel for schedule(dynamic, 64)
    for (int id = 0; id < npix; id++) pixel(M, id);
    return 0;
}
