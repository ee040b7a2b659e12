// soc_map.hip -- map making: Mapping, HealpixMapping and PolMapping of kernel_ASOC_map.c (:496-888, :890-970, :972-1693) and
// PolHealpixMapping of kernel_ASOC_map_H.c (:576-841) for gfx950.  One lane per map pixel integrates emission x extinction along its line
// of sight through the (hierarchical) grid.
//
// The reference's map file has its own copies of the traversal helpers, and they are not the ones of the
// simulation kernels: PEPS = 5e-4 and EPS = 2.5e-4 (:10-11), Index() in double whenever NX > 100 (:297),
// and a climb that stops below the root grid only when the local z is exactly 0 (the test at :345 reads
// "POS.z<=0.0") -- so after every step out of an octet the position is rebuilt from the root.  That
// changes the last bits of positions and step lengths, hence of the maps; it is restated here as written
// (soc_map_index) and pinned bit-exactly by the x86 build of the reference (oracle/_ref/refmap_*.so).
// -D MAP_INTERPOLATION, ROI_MAP and LEVEL_THRESHOLD are launch arguments here; PolMapping (POLSTAT 0, 1, 3) and
// PolHealpixMapping (POLSTAT 0, with the differences of its own file's walk) follow, and last the per-level Mapping of
// kernel_ASOC_map_H.c (:380-497).
#include "soc_walk.h"

#define SOC_MAP_PEPS 5.0e-4f
#define SOC_MAP_EPS  2.5e-4f


// HFILE: the Index() of kernel_ASOC_map_H.c (:216-289, PolHealpixMapping) instead.  It is this one except that it does not
// write the position back where the climb ends on the root grid -- neither when the ray has left the model (:246-248) nor
// when the root cell found there is a leaf (:252): the ray then goes on at level 0 with the octet's local coordinates.
template <bool OCT, typename T, bool HFILE = false>
__device__ __forceinline__ void soc_map_index(const SocGrid &G, const int *sOFF, float &px, float &py, float &pz,
                                              int &level, int &ind, float &dens)
{
    const int NX = G.NX, NY = G.NY, NZ = G.NZ;
    if (!OCT || (level == 0)) {
        if ((px <= 0.0f) || (px >= NX) || (py <= 0.0f) || (py >= NY) || (pz <= 0.0f) || (pz >= NZ)) { ind = -1;  return; }
        ind  = (int)soc_floorf(pz) * NX * NY + (int)soc_floorf(py) * NX + (int)soc_floorf(px);
        dens = G.DENS[ind];
        if (!OCT) return;
        if (dens > 0.0f) return;
    }
    if (OCT) {
        T PX = px, PY = py, PZ = pz;
        const T HALF = (T)0.5, TWO = (T)2.0, ZERO = (T)0.0;
        while (level > 0) {
            ind = G.PAR[sOFF[level] + ind - G.NXYZ];
            level--;
            PX *= HALF;  PY *= HALF;  PZ *= HALF;
            if (level == 0) {
                PX += ind % NX;
                PY += (ind / NX) % NY;
                PZ += ind / (NX * NY);
                if ((PX <= ZERO) || (PX >= NX) || (PY <= ZERO) || (PY >= NY) || (PZ <= ZERO) || (PZ >= NZ)) {
                    ind = -1;
                    if (!HFILE) { px = (float)PX;  py = (float)PY;  pz = (float)PZ; }
                    return;
                }
                ind  = (int)SocReal<T>::floorr(PZ) * NX * NY + (int)SocReal<T>::floorr(PY) * NX + (int)SocReal<T>::floorr(PX);
                dens = G.DENS[ind];
                if (dens > 0.0f) { if (!HFILE) { px = (float)PX;  py = (float)PY;  pz = (float)PZ; }  return; }
                break;
            } else {
                const int sid = ind % 8;
                PX += sid % 2;  PY += (sid / 2) % 2;  PZ += sid / 4;
                // kernel_ASOC_map.c:345, as written: "... &&(POS.z>=0.0)&&(POS.z<=0.0)"
                if ((PX >= ZERO) && (PX <= TWO) && (PY >= ZERO) && (PY <= TWO) && (PZ >= ZERO) && (PZ <= ZERO)) {
                    dens = G.DENS[sOFF[level] + ind];
                    break;
                }
            }
        }
        while (!(dens > 0.0f)) {
            PX = TWO * SocReal<T>::fmod1(PX);
            PY = TWO * SocReal<T>::fmod1(PY);
            PZ = TWO * SocReal<T>::fmod1(PZ);
            ind = soc_link_index(dens);
            level++;
            ind += 4 * (int)SocReal<T>::floorr(PZ) + 2 * (int)SocReal<T>::floorr(PY) + (int)SocReal<T>::floorr(PX);
            dens = G.DENS[sOFF[level] + ind];
        }
        px = (float)PX;  py = (float)PY;  pz = (float)PZ;
    }
}

template <bool OCT, bool DBL, bool HFILE = false>
__device__ __forceinline__ float soc_map_getstep(const SocGrid &G, const int *sOFF, float &px, float &py, float &pz,
                                                 float ux, float uy, float uz, int &level, int &ind, float &dens)
{
    const float ax = (ux > 0.0f) ? (((1.0f + SOC_MAP_PEPS) - soc_fmod1f(px)) / ux) : ((-SOC_MAP_PEPS - soc_fmod1f(px)) / ux);
    const float ay = (uy > 0.0f) ? (((1.0f + SOC_MAP_PEPS) - soc_fmod1f(py)) / uy) : ((-SOC_MAP_PEPS - soc_fmod1f(py)) / uy);
    const float az = (uz > 0.0f) ? (((1.0f + SOC_MAP_PEPS) - soc_fmod1f(pz)) / uz) : ((-SOC_MAP_PEPS - soc_fmod1f(pz)) / uz);
    float s = __builtin_fminf(ax, __builtin_fminf(ay, az));
    px += s * ux;
    py += s * uy;
    pz += s * uz;
    s = soc_scale_down(s, level);
    if (DBL) soc_map_index<OCT, double, HFILE>(G, sOFF, px, py, pz, level, ind, dens);
    else     soc_map_index<OCT, float, HFILE>(G, sOFF, px, py, pz, level, ind, dens);
    return s;
}

__device__ __forceinline__ bool soc_map_outside(const SocGrid &G, float x, float y, float z)
{
    return (x < 0.0f) || (x > G.NX) || (y < 0.0f) || (y > G.NY) || (z < 0.0f) || (z > G.NZ);
}

// InRoi (kernel_ASOC_map.c:37-56): is the root cell above cell (level, ind) inside ROI?
template <bool OCT>
__device__ __forceinline__ bool soc_map_inroi(const SocGrid &G, const int *sOFF, const int *ROI, int level, int ind)
{
    if (OCT) { while (level > 0) { ind = G.PAR[sOFF[level] + ind - G.NXYZ];  level--; } }
    const int k = ind / (G.NX * G.NY), j = (ind / G.NX) % G.NY, i = ind % G.NX;
    return (i >= ROI[0]) && (i <= ROI[1]) && (j >= ROI[2]) && (j <= ROI[3]) && (k >= ROI[4]) && (k <= ROI[5]);
}

// One neighbour of the MAP_INTERPOLATION block (kernel_ASOC_map.c:716-731, :771-788): from the middle of the step the
// distance (cell units) to the next cell along +V, else along -V (V stays flipped), else "none" (0.5, nothing to blend).
// ncell is that cell's place in the per-cell arrays, -1 for "none": its emission then counts as 0.
template <bool OCT, bool DBL>
__device__ __forceinline__ void soc_map_neighbour(const SocGrid &G, const int *sOFF, float p0x, float p0y, float p0z,
                                                  float tx, float ty, float tz, float w, int level0, int ind0, float K,
                                                  float &vx, float &vy, float &vz, float lim, bool second_try_unscaled,
                                                  float &dist, float &ndens, int &ncell)
{
    for (int attempt = 0; attempt < 2; attempt++) {
        int   slevel = level0, sind = ind0;
        float nd = 0.0f;
        if (attempt) { vx = -vx;  vy = -vy;  vz = -vz; }
        float mx = p0x + w * tx, my = p0y + w * ty, mz = p0z + w * tz;
        float a = soc_map_getstep<OCT, DBL>(G, sOFF, mx, my, mz, vx, vy, vz, slevel, sind, nd);
        if (!(attempt && second_try_unscaled)) a = a / K;                 // (:736 has no "b /= K" in the MAP_INTERPOLATION==2 block)
        if ((a <= lim) && (sind >= 0)) { dist = a;  ndens = nd;  ncell = sOFF[slevel] + sind;  return; }
    }
    dist = 0.5f;  ndens = 0.0f;  ncell = -1;
}

// ------------------------------------------------------------------------------------
// One line of sight of Mapping / HealpixMapping, without what is integrated along it: where pixel `id` enters the model, and one
// step of the walk.  soc_map_kernel (one frequency) and soc_mapx_kernel (a batch of frequencies) are these two functions plus
// soc_map_blend and soc_map_add per frequency -- the same operations in the same order, so the same bits.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void soc_map_entry(const SocGrid &G, const SocMapView &A, int id, float &px, float &py, float &pz,
                                              float &tx, float &ty, float &tz)
{
    const int NX = G.NX, NY = G.NY, NZ = G.NZ;
    if (A.mode) {
        // HealpixMapping: all-sky map seen from INTOBS (:913-925)
        float phi, theta, st, ct, sp, cp;
        soc_pixel2angles_ring(A.NPIX_X, id, phi, theta);
        soc_sincosf(theta, &st, &ct);
        soc_sincosf(phi, &sp, &cp);
        tx = -st * cp;  ty = -st * sp;  tz = +ct;
        if (soc_fabsf(tx) < 1.0e-5f) tx = 1.0e-5f;
        if (soc_fabsf(ty) < 1.0e-5f) ty = 1.0e-5f;
        if (soc_fabsf(tz) < 1.0e-5f) tz = 1.0e-5f;
        px = A.INTOBS[0];  py = A.INTOBS[1];  pz = A.INTOBS[2];
        if ((soc_fmod1f(px) < 1.0e-5f) || (soc_fmod1f(px) < 0.99999f)) px += 2.0e-5f;       // as written
        if ((soc_fmod1f(py) < 1.0e-5f) || (soc_fmod1f(py) < 0.99999f)) py += 2.0e-5f;
        if ((soc_fmod1f(pz) < 1.0e-5f) || (soc_fmod1f(pz) < 0.99999f)) pz += 2.0e-5f;
    } else {
        const int i = id % A.NPIX_X, j = id / A.NPIX_X;
        if (A.INTOBS[0] > -1e10f) {
            // longitude x latitude image seen from inside the model (:534-556)
            float phi = SOC_TWOPI * i / (float)(A.NPIX_X);
            phi += SOC_PI;
            const float pix = SOC_TWOPI / A.NPIX_X;
            const float theta = pix * (j - (A.NPIX_Y - 1) / 2);
            float st, ct, sp, cp;
            soc_sincosf(theta, &st, &ct);
            soc_sincosf(phi, &sp, &cp);
            px = A.INTOBS[0];  py = A.INTOBS[1];  pz = A.INTOBS[2];
            tx = ct * cp;  ty = ct * sp;  tz = st;
            if (soc_fabsf(tx) < 1.0e-5f) tx = 1.0e-5f;
            if (soc_fabsf(ty) < 1.0e-5f) ty = 1.0e-5f;
            if (soc_fabsf(tz) < 1.0e-5f) tz = 1.0e-5f;
            if (soc_fmod1f(px) < 1.0e-5f) px += 2.0e-5f;
            if (soc_fmod1f(py) < 1.0e-5f) py += 2.0e-5f;
            if (soc_fmod1f(pz) < 1.0e-5f) pz += 2.0e-5f;
        } else {
            // orthographic map: start behind the cloud as seen by the observer, enter through the far faces (:557-640)
            const float dx = A.DIR[0], dy = A.DIR[1], dz = A.DIR[2];
            px = A.CENTRE[0] + (i - 0.5f * (A.NPIX_X - 1)) * A.MAP_DX * A.RA[0] + (j - 0.5f * (A.NPIX_Y - 1)) * A.MAP_DX * A.DE[0];
            py = A.CENTRE[1] + (i - 0.5f * (A.NPIX_X - 1)) * A.MAP_DX * A.RA[1] + (j - 0.5f * (A.NPIX_Y - 1)) * A.MAP_DX * A.DE[1];
            pz = A.CENTRE[2] + (i - 0.5f * (A.NPIX_X - 1)) * A.MAP_DX * A.RA[2] + (j - 0.5f * (A.NPIX_Y - 1)) * A.MAP_DX * A.DE[2];
            px += (NX + NY + NZ) * dx;  py += (NX + NY + NZ) * dy;  pz += (NX + NY + NZ) * dz;
            float sx, sy, sz;
            if (NX < 200) {
                if (dx >= 0.0f) sx = (NX - px) / (-dx) + SOC_MAP_EPS;  else sx = (0.0f - px) / (-dx) + SOC_MAP_EPS;
                if (dy >= 0.0f) sy = (NY - py) / (-dy) + SOC_MAP_EPS;  else sy = (0.0f - py) / (-dy) + SOC_MAP_EPS;
                if (dz >= 0.0f) sz = (NZ - pz) / (-dz) + SOC_MAP_EPS;  else sz = (0.0f - pz) / (-dz) + SOC_MAP_EPS;
                if (soc_map_outside(G, px - sx * dx, py - sx * dy, pz - sx * dz)) sx = 1e10f;
                if (soc_map_outside(G, px - sy * dx, py - sy * dy, pz - sy * dz)) sy = 1e10f;
                if (soc_map_outside(G, px - sz * dx, py - sz * dy, pz - sz * dz)) sz = 1e10f;
                sx = __builtin_fminf(sx, __builtin_fminf(sy, sz));
                px = px - sx * dx;  py = py - sx * dy;  pz = pz - sx * dz;
            } else {
                const float ex = (dx > 0.0f) ? (-SOC_MAP_EPS) : (+SOC_MAP_EPS), ey = (dy > 0.0f) ? (-SOC_MAP_EPS) : (+SOC_MAP_EPS),
                            ez = (dz > 0.0f) ? (-SOC_MAP_EPS) : (+SOC_MAP_EPS);
                if (dx >= 0.0f) sx = (NX - px) / (-dx);  else sx = (0.0f - px) / (-dx);
                if (dy >= 0.0f) sy = (NY - py) / (-dy);  else sy = (0.0f - py) / (-dy);
                if (dz >= 0.0f) sz = (NZ - pz) / (-dz);  else sz = (0.0f - pz) / (-dz);
                if (soc_map_outside(G, (px - sx * dx) + ex, (py - sx * dy) + ey, (pz - sx * dz) + ez)) sx = 1e10f;
                if (soc_map_outside(G, (px - sy * dx) + ex, (py - sy * dy) + ey, (pz - sy * dz) + ez)) sy = 1e10f;
                if (soc_map_outside(G, (px - sz * dx) + ex, (py - sz * dy) + ey, (pz - sz * dz) + ez)) sz = 1e10f;
                sx = __builtin_fminf(sx, __builtin_fminf(sy, sz));
                px = px - sx * dx;  py = py - sx * dy;  pz = pz - sx * dz;
                px += ex;  py += ey;  pz += ez;
            }
            tx = -dx;  ty = -dy;  tz = -dz;
            if (soc_fabsf(tx) < 1.0e-5f) tx = 1.0e-5f;
            if (soc_fabsf(ty) < 1.0e-5f) ty = 1.0e-5f;
            if (soc_fabsf(tz) < 1.0e-5f) tz = 1.0e-5f;
        }
    }
}

// the two directions across the ray along which MAP_INTERPOLATION looks for neighbours (:664-682)
struct SocMapCross { float ax, ay, az, bx, by, bz; };
__device__ __forceinline__ SocMapCross soc_map_cross(float tx, float ty, float tz)
{
    SocMapCross X;
    if (soc_fabsf(tx) > soc_fabsf(ty)) {
        if (soc_fabsf(tz) > soc_fabsf(tx)) { X.ax = 0.0005f;  X.ay = 1.0f;  X.az = -ty / tz; }
        else                               { X.ax = -tz / tx;  X.ay = 0.0005f;  X.az = 1.0f; }
    } else {
        if (soc_fabsf(tz) > soc_fabsf(ty)) { X.ax = 0.0005f;  X.ay = 1.0f;  X.az = -ty / tz; }
        else                               { X.ax = 1.0f;  X.ay = -tx / ty;  X.az = 0.0005f; }
    }
    soc_normalize(X.ax, X.ay, X.az);
    X.bx = ty * X.az - tz * X.ay;
    X.by = tz * X.ax - tx * X.az;
    X.bz = tx * X.ay - ty * X.ax;
    soc_normalize(X.bx, X.by, X.bz);
    return X;
}

// One step: the cell it crosses (oind in the per-cell arrays, on level olevel), its length sx and the density d0 -- with
// MAP_INTERPOLATION already blended --, whether the cell's emission counts (`roimap`, `threshold`), and for the blend of the
// emission the two neighbour cells with the weights of soc_map_blend.
struct SocMapStep {
    int   oind, olevel, na, nb;
    float sx, d0, wa, wb, wc;
    bool  emits;
};

// (MAP_INTERPOLATION == 2: :746-751; == 1: :806-808) of the cell's own value and its neighbours'
__device__ __forceinline__ float soc_map_blend(int MI, const SocMapStep &S, float own, float A, float B)
{
    if (MI == 2) return S.wa * A + S.wb * B + S.wc * own;
    return S.wc * own + S.wa * A + S.wb * B;
}

template <bool OCT, bool DBL>
__device__ __forceinline__ SocMapStep soc_map_step(const SocGrid &G, const int *sOFF, const SocMapView &A, SocMapCross &X,
                                                   float &px, float &py, float &pz, float tx, float ty, float tz,
                                                   int &level, int &ind, float &dens)
{
    SocMapStep S;
    const int MI = A.MAPINT;
    S.oind = sOFF[level] + ind;
    S.olevel = level;
    S.na = -1;  S.nb = -1;
    S.wa = 0.0f;  S.wb = 0.0f;  S.wc = 1.0f;
    const float p0x = px, p0y = py, p0z = pz;
    const int   ind0 = ind;
    S.d0 = dens;
    S.sx = soc_map_getstep<OCT, DBL>(G, sOFF, px, py, pz, tx, ty, tz, level, ind, dens);
    if (MI > 0) {
        const float K = soc_scale_down(1.0f, S.olevel);               // local -> root-grid length
        float a, b, Ad, Bd;
        if (MI == 2) {                                                // steps of at most 0.22 cells (:709-715)
            a = 0.22f * K;
            if (S.sx > a) {
                S.sx = a;
                px = p0x + 0.22f * tx;  py = p0y + 0.22f * ty;  pz = p0z + 0.22f * tz;
                ind = ind0;  level = S.olevel;
                if (DBL) soc_map_index<OCT, double>(G, sOFF, px, py, pz, level, ind, dens);
                else     soc_map_index<OCT, float>(G, sOFF, px, py, pz, level, ind, dens);
            }
        }
        const float w = 0.5f * S.sx / K;
        const float lim = (MI == 2) ? 0.52f : 0.502f;
        soc_map_neighbour<OCT, DBL>(G, sOFF, p0x, p0y, p0z, tx, ty, tz, w, S.olevel, ind0, K, X.ax, X.ay, X.az, lim, false, a, Ad, S.na);
        soc_map_neighbour<OCT, DBL>(G, sOFF, p0x, p0y, p0z, tx, ty, tz, w, S.olevel, ind0, K, X.bx, X.by, X.bz, lim, MI == 2, b, Bd, S.nb);
        if (MI == 2) {                                                // :746-751
            a = soc_clampf(a, 0.0f, 0.51f);
            b = soc_clampf(b, 0.0f, 0.51f);
            S.wa = 0.5f - a;  S.wb = 0.5f - b;  S.wc = a + b;
        } else {                                                      // :806-808
            S.wa = 0.5f - a;  S.wb = 0.5f - b;
            S.wc = 1.0f - S.wa - S.wb;
        }
        S.d0 = soc_map_blend(MI, S, S.d0, Ad, Bd);
    }
    if (A.ROI_MAP && !soc_map_inroi<OCT>(G, sOFF, A.ROI, S.olevel, S.oind - sOFF[S.olevel])) S.emits = false;   // `roimap`: cells outside ROI do not emit
    else if (!A.mode && (S.olevel < A.LEVEL_THRESHOLD)) S.emits = false;  // `threshold`: coarse levels do not emit (they still absorb); Mapping only
    else S.emits = true;
    return S;
}

// what one frequency adds on a step (:825-846, :950-955): emission seen through the optical depth in front of it, then that depth grows.
// soc_map_weight is the head of that product, up to the step length; the term is soc_map_weight * emit * S.d0, multiplied from the left.
__device__ __forceinline__ float soc_map_weight(const SocMapStep &S, float DTAU, float TAU)
{
    if (DTAU < 1.0e-3f) return soc_expf(-TAU) * (1.0f - 0.5f * DTAU) * S.sx;
    return soc_expf(-TAU) * ((1.0f - soc_expf(-DTAU)) / DTAU) * S.sx;
}

__device__ __forceinline__ void soc_map_add(const SocMapStep &S, float emit, float DTAU, float &TAU, float &PHOTONS)
{
    if (S.emits) PHOTONS += soc_map_weight(S, DTAU, TAU) * emit * S.d0;
    TAU += DTAU;
}

template <bool OCT, bool DBL, bool ABU>
__global__ __launch_bounds__(256) void soc_map_kernel(const SocGrid G, const SocMapArgs A)
{
    __shared__ int sOFF[SOC_MAXL];
    if (threadIdx.x < SOC_MAXL) sOFF[threadIdx.x] = G.OFF[threadIdx.x];
    __syncthreads();
    const int npix = A.mode ? 12 * A.NPIX_X * A.NPIX_X : A.NPIX_X * A.NPIX_Y;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= npix) return;
    float TAU = 0.0f, PHOTONS = 0.0f, colden = 0.0f;
    float px, py, pz, tx, ty, tz;
    soc_map_entry(G, A, id, px, py, pz, tx, ty, tz);
    int   level = 0, ind = -1;
    float dens = 0.0f;
    soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
    const int MI = A.MAPINT;
    SocMapCross X = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (MI > 0) X = soc_map_cross(tx, ty, tz);
    while (ind >= 0) {
        const SocMapStep S = soc_map_step<OCT, DBL>(G, sOFF, A, X, px, py, pz, tx, ty, tz, level, ind, dens);
        float emit = A.EMIT[S.oind];
        if (MI > 0) emit = soc_map_blend(MI, S, emit, (S.na >= 0) ? A.EMIT[S.na] : 0.0f, (S.nb >= 0) ? A.EMIT[S.nb] : 0.0f);
        float DTAU;
        if (ABU) { const float2 o = A.OPT[S.oind];  DTAU = S.sx * S.d0 * (o.x + o.y); }
        else     DTAU = S.sx * S.d0 * (A.SCA + A.ABS);
        soc_map_add(S, emit, DTAU, TAU, PHOTONS);
        if (A.mode || (A.SAVE_COLDEN > 0)) colden += S.sx * S.d0;
    }
    A.MAP[id] = PHOTONS;
    A.SAVETAU[id] = A.SAVE_COLDEN ? (colden * A.LENGTH) : TAU;
}

// Mapping / HealpixMapping for a batch of A.nf <= KF frequencies: one walk per pixel, and per step and frequency what
// soc_map_kernel does for its one -- plane f is, bit for bit, soc_map_kernel's map of frequency f.  (The reference names this
// kernel_ASOC_map_X.c, ASOC.py:3442-3568, and does not ship it.)  The accumulators are registers: KF is a template argument
// and every loop over it is unrolled, frequencies beyond A.nf are skipped by a test that is uniform over the grid.  Per-cell
// inputs are cell-major, [CELLS][nf]: a step reads one cell's frequencies from adjacent addresses (64-bit offsets: CELLS * nf
// passes 2^31 on production models).
template <bool OCT, bool DBL, bool ABU, int KF>
__global__ __launch_bounds__(256) void soc_mapx_kernel(const SocGrid G, const SocMapXArgs A)
{
    __shared__ int sOFF[SOC_MAXL];
    if (threadIdx.x < SOC_MAXL) sOFF[threadIdx.x] = G.OFF[threadIdx.x];
    __syncthreads();
    const int npix = A.mode ? 12 * A.NPIX_X * A.NPIX_X : A.NPIX_X * A.NPIX_Y;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= npix) return;
    const int nf = A.nf;
    float TAU[KF], PHOTONS[KF], OPTSUM[KF], colden = 0.0f;
#pragma unroll
    for (int f = 0; f < KF; f++) {
        TAU[f] = 0.0f;  PHOTONS[f] = 0.0f;
        OPTSUM[f] = (!ABU && (f < nf)) ? (A.SCA[f] + A.ABS[f]) : 0.0f;
    }
    float px, py, pz, tx, ty, tz;
    soc_map_entry(G, A, id, px, py, pz, tx, ty, tz);
    int   level = 0, ind = -1;
    float dens = 0.0f;
    soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
    const int MI = A.MAPINT;
    SocMapCross X = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (MI > 0) X = soc_map_cross(tx, ty, tz);
    while (ind >= 0) {
        const SocMapStep S = soc_map_step<OCT, DBL>(G, sOFF, A, X, px, py, pz, tx, ty, tz, level, ind, dens);
        const float  *E  = A.EMIT + (size_t)S.oind * nf;
        const float  *Ea = A.EMIT + (size_t)((S.na >= 0) ? S.na : 0) * nf;
        const float  *Eb = A.EMIT + (size_t)((S.nb >= 0) ? S.nb : 0) * nf;
        const float2 *O  = ABU ? (A.OPT + (size_t)S.oind * nf) : nullptr;
#pragma unroll
        for (int f = 0; f < KF; f++) {
            if (f < nf) {
                float emit = E[f];
                if (MI > 0) emit = soc_map_blend(MI, S, emit, (S.na >= 0) ? Ea[f] : 0.0f, (S.nb >= 0) ? Eb[f] : 0.0f);
                float DTAU;
                if (ABU) { const float2 o = O[f];  DTAU = S.sx * S.d0 * (o.x + o.y); }
                else     DTAU = S.sx * S.d0 * OPTSUM[f];
                soc_map_add(S, emit, DTAU, TAU[f], PHOTONS[f]);
            }
        }
        colden += S.sx * S.d0;
    }
#pragma unroll
    for (int f = 0; f < KF; f++) {
        if (f < nf) {
            A.MAP[(size_t)f * npix + id] = PHOTONS[f];
            A.TAU[(size_t)f * npix + id] = TAU[f];
        }
    }
    A.COLDEN[id] = colden * A.LENGTH;
}

// The levels of the plain map (`maplevels 1`): the walk of soc_mapx_kernel with one accumulator per hierarchy level and frequency.
// Plane (f, l) is, bit for bit, soc_map_kernel's map of frequency f when the emission of every cell not on level l is 0.0f and
// everything else -- densities, opacities, view, switches -- stays: what level l emits towards the pixel, seen through all that lies in
// front of it.  The reference has no such kernel; its per-level Mapping is soc_maplev_kernel below, on another walk.
// On a step the cell crossed adds to the plane of its level.  With MAP_INTERPOLATION the blend of soc_map_blend is taken once per
// distinct level among the cell and its two neighbours, the operands of the other levels replaced by 0.0f: a neighbour feeds the
// plane of its own level.  (A level none of the three is on would get the blend of three zeros: +0, which changes no sum.)  Whether
// the step emits (S.emits) and the density S.d0 are the crossed cell's, as in the plain kernel; TAU grows once per step and frequency.
// The accumulators are LDS, lane-minor: word (l * KF + f) * 256 + tid of the dynamic array -- indexed by the run-time level without
// scratch or a compare-select chain, touched by their own lane only (no barrier, no bank conflict), LEVELS * KF * 1 KiB per workgroup;
// behind them OFF[] and OFF[] + LCELLS[] of every level.  A launch takes columns [A.f0, A.f0 + A.kf), kf <= KF, of the resident
// cell-major batch [CELLS][A.nf]; columns outside are never read.
template <bool OCT, bool DBL, bool ABU, int KF>
__global__ __launch_bounds__(256) void soc_maplevx_kernel(const SocGrid G, const SocMapLXArgs A)
{
    extern __shared__ float soc_maplevx_lds[];
    const int NL = G.LEVELS, tid = threadIdx.x;
    int *sOFF = (int *)(soc_maplevx_lds + NL * KF * 256);
    int *sEND = sOFF + SOC_MAXL;
    if (tid < SOC_MAXL) { sOFF[tid] = G.OFF[tid];  sEND[tid] = G.OFF[tid] + G.LCELLS[tid]; }
    __syncthreads();
    const int npix = A.mode ? 12 * A.NPIX_X * A.NPIX_X : A.NPIX_X * A.NPIX_Y;
    const int id = blockIdx.x * blockDim.x + tid;
    if (id >= npix) return;
    const int nf = A.nf, kf = A.kf;
    float *acc = soc_maplevx_lds + tid;                                   // word (l, f) of this lane: acc[(l * KF + f) * 256]
    for (int k = 0; k < NL * KF; k++) acc[k * 256] = 0.0f;
    float TAU[KF], OPTSUM[KF];
#pragma unroll
    for (int f = 0; f < KF; f++) {
        TAU[f] = 0.0f;
        OPTSUM[f] = (!ABU && (f < kf)) ? (A.SCA[A.f0 + f] + A.ABS[A.f0 + f]) : 0.0f;
    }
    float px, py, pz, tx, ty, tz;
    soc_map_entry(G, A, id, px, py, pz, tx, ty, tz);
    int   level = 0, ind = -1;
    float dens = 0.0f;
    soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
    const int MI = A.MAPINT;
    SocMapCross X = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (MI > 0) X = soc_map_cross(tx, ty, tz);
    while (ind >= 0) {
        const SocMapStep S = soc_map_step<OCT, DBL>(G, sOFF, A, X, px, py, pz, tx, ty, tz, level, ind, dens);
        // the levels of the neighbours; a missing one contributes 0.0f whatever its level is called
        int la = S.olevel, lb = S.olevel;
        if (MI > 0) {
            for (int l = 0; l < NL; l++) {
                if ((S.na >= sOFF[l]) && (S.na < sEND[l])) la = l;
                if ((S.nb >= sOFF[l]) && (S.nb < sEND[l])) lb = l;
            }
        }
        const float  *E  = A.EMIT + (size_t)S.oind * nf + A.f0;
        const float  *Ea = A.EMIT + (size_t)((S.na >= 0) ? S.na : 0) * nf + A.f0;
        const float  *Eb = A.EMIT + (size_t)((S.nb >= 0) ? S.nb : 0) * nf + A.f0;
        const float2 *O  = ABU ? (A.OPT + (size_t)S.oind * nf + A.f0) : nullptr;
        float *acc0 = acc + S.olevel * (KF * 256), *acca = acc + la * (KF * 256), *accb = acc + lb * (KF * 256);
#pragma unroll
        for (int f = 0; f < KF; f++) {
            if (f < kf) {
                float DTAU;
                if (ABU) { const float2 o = O[f];  DTAU = S.sx * S.d0 * (o.x + o.y); }
                else     DTAU = S.sx * S.d0 * OPTSUM[f];
                if (S.emits) {
                    const float w = soc_map_weight(S, DTAU, TAU[f]);
                    const float own = E[f];
                    if (MI > 0) {
                        const float a = (S.na >= 0) ? Ea[f] : 0.0f, b = (S.nb >= 0) ? Eb[f] : 0.0f;
                        acc0[f * 256] += w * soc_map_blend(MI, S, own, (la == S.olevel) ? a : 0.0f, (lb == S.olevel) ? b : 0.0f) * S.d0;
                        if (la != S.olevel) acca[f * 256] += w * soc_map_blend(MI, S, 0.0f, a, (lb == la) ? b : 0.0f) * S.d0;
                        if ((lb != S.olevel) && (lb != la)) accb[f * 256] += w * soc_map_blend(MI, S, 0.0f, 0.0f, b) * S.d0;
                    } else {
                        acc0[f * 256] += w * own * S.d0;
                    }
                }
                TAU[f] += DTAU;
            }
        }
    }
    for (int l = 0; l < NL; l++) {
#pragma unroll
        for (int f = 0; f < KF; f++)
            if (f < kf) A.MAPL[((size_t)(A.f0 + f) * NL + l) * npix + id] = acc[(l * KF + f) * 256];
    }
}

// PSTau (kernel_ASOC_map.c:1545-1584): column density and optical depth from every point source towards the observer
template <bool OCT, bool DBL, bool ABU>
__global__ __launch_bounds__(64) void soc_pstau_kernel(const SocGrid G, const int no, const float4 *PSPOS, const float ux, const float uy, const float uz,
                                                       const float ABS, const float SCA, const float2 *OPT, const float LENGTH, float *pscolden, float *pstau)
{
    __shared__ int sOFF[SOC_MAXL];
    if (threadIdx.x < SOC_MAXL) sOFF[threadIdx.x] = G.OFF[threadIdx.x];
    __syncthreads();
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= no) return;
    float px = PSPOS[id].x, py = PSPOS[id].y, pz = PSPOS[id].z, TAU = 0.0f, colden = 0.0f, dens = 0.0f;
    int   level = 0, ind = -1;
    soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
    while (ind >= 0) {
        const int   oind = sOFF[level] + ind;
        const float d0 = dens;
        const float sx = soc_map_getstep<OCT, DBL>(G, sOFF, px, py, pz, ux, uy, uz, level, ind, dens);
        float DTAU;
        if (ABU) { const float2 o = OPT[oind];  DTAU = sx * d0 * (o.x + o.y); }
        else     DTAU = sx * d0 * (SCA + ABS);
        TAU += DTAU;
        colden += sx * d0;
    }
    pscolden[id] = colden * LENGTH;
    pstau[id]    = TAU;
}

hipError_t soc_launch_pstau(const SocGrid &G, int no, const float4 *PSPOS, const float *DIR, float ABS, float SCA, const float2 *OPT, float LENGTH,
                            float *pscolden, float *pstau, hipStream_t st)
{
    if (no <= 0) return hipSuccess;
    const dim3 grid((no + 63) / 64), block(64);
    const bool oct = G.LEVELS > 1, dbl = oct && (G.NX > 100), abu = OPT != nullptr;
#define SOC_PT(O, D, A) soc_pstau_kernel<O, D, A><<<grid, block, 0, st>>>(G, no, PSPOS, DIR[0], DIR[1], DIR[2], ABS, SCA, OPT, LENGTH, pscolden, pstau)
    if (!oct)      { if (abu) SOC_PT(false, false, true); else SOC_PT(false, false, false); }
    else if (!dbl) { if (abu) SOC_PT(true, false, true);  else SOC_PT(true, false, false); }
    else           { if (abu) SOC_PT(true, true, true);   else SOC_PT(true, true, false); }
#undef SOC_PT
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// polarisation maps: PolMapping of kernel_ASOC_map.c, -D POLSTAT=0 (:972-1137), =1 (:1147-1384), =3 (:1594-1693)
// ------------------------------------------------------------------------------------
// One lane per pixel, as Mapping.  -D POLRED, POL_RHO_WEIGHT and LEVEL_THRESHOLD are launch arguments, p00 is A.p0.  The
// magnetic field is one float4 (Bx, By, Bz, pad) per cell: a step reads it with one 16-byte load.  The arithmetic keeps
// the reference's operations and their order; dot, length and normalize are what oracle/ref_builtins.inc gives the x86
// build of the reference (soc_normalize is the same normalize).
#define SOC_POL_PI     3.1415926536f
#define SOC_POL_TWOPI  6.2831853072f
#define SOC_POL_PIHALF 1.5707963268f

__device__ __forceinline__ float soc_dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

__device__ __forceinline__ bool soc_pol_outside(const SocGrid &G, float x, float y, float z)
{
    return (x <= 0.0f) || (x >= G.NX) || (y <= 0.0f) || (y >= G.NY) || (z <= 0.0f) || (z >= G.NZ);
}

// The ray's entry (:1011-1033, the same lines in every POLSTAT block): PolMapping starts BEHIND the cloud and takes the
// largest of the three face crossings that stays inside, each minus EPS -- not Mapping's entry; no NX >= 200 branch,
// no INTOBS, and the walking direction -DIR is not clamped.
template <typename ARGS>                                                // SocPolArgs, or the SocMapLevArgs of the per-level Mapping (same lines)
__device__ __forceinline__ void soc_pol_entry(const SocGrid &G, const ARGS &A, int id, float &px, float &py, float &pz)
{
    const int   NX = G.NX, NY = G.NY, NZ = G.NZ;
    const int   i = id % A.NPIX_X, j = id / A.NPIX_X;
    const float dx = A.DIR[0], dy = A.DIR[1], dz = A.DIR[2];
    px = A.CENTRE[0] + (i - 0.5f * (A.NPIX_X - 1)) * A.MAP_DX * A.RA[0] + (j - 0.5f * (A.NPIX_Y - 1)) * A.MAP_DX * A.DE[0];
    py = A.CENTRE[1] + (i - 0.5f * (A.NPIX_X - 1)) * A.MAP_DX * A.RA[1] + (j - 0.5f * (A.NPIX_Y - 1)) * A.MAP_DX * A.DE[1];
    pz = A.CENTRE[2] + (i - 0.5f * (A.NPIX_X - 1)) * A.MAP_DX * A.RA[2] + (j - 0.5f * (A.NPIX_Y - 1)) * A.MAP_DX * A.DE[2];
    px -= (NX + NY + NZ) * dx;  py -= (NX + NY + NZ) * dy;  pz -= (NX + NY + NZ) * dz;
    float sx, sy, sz;
    if (dx >= 0.0f) sx = (NX - px) / (dx + 1.0e-10f) - SOC_MAP_EPS;  else sx = (0.0f - px) / dx - SOC_MAP_EPS;
    if (dy >= 0.0f) sy = (NY - py) / (dy + 1.0e-10f) - SOC_MAP_EPS;  else sy = (0.0f - py) / dy - SOC_MAP_EPS;
    if (dz >= 0.0f) sz = (NZ - pz) / (dz + 1.0e-10f) - SOC_MAP_EPS;  else sz = (0.0f - pz) / dz - SOC_MAP_EPS;
    if (soc_pol_outside(G, px + sx * dx, py + sx * dy, pz + sx * dz)) sx = -1e10f;
    if (soc_pol_outside(G, px + sy * dx, py + sy * dy, pz + sy * dz)) sy = -1e10f;
    if (soc_pol_outside(G, px + sz * dx, py + sz * dy, pz + sz * dz)) sz = -1e10f;
    sx = __builtin_fmaxf(sx, __builtin_fmaxf(sy, sz));
    px = px + sx * dx;  py = py + sx * dy;  pz = pz + sx * dz;
}

// emission weight of one step (:1095-1099, :1255-1259, :1329-1333)
__device__ __forceinline__ float soc_pol_emitted(float TAU, float DTAU, float sx, float emit, float rho)
{
    if (DTAU < 1.0e-3f) return soc_expf(-TAU) * (1.0f - 0.5f * DTAU) * sx * emit * rho;
    return soc_expf(-TAU) * ((1.0f - soc_expf(-DTAU)) / DTAU) * sx * emit * rho;
}

template <bool OCT, bool DBL, bool ABU, int POLSTAT>
__global__ __launch_bounds__(256) void soc_polmap_kernel(const SocGrid G, const SocPolArgs A)
{
    __shared__ int sOFF[SOC_MAXL];
    if (threadIdx.x < SOC_MAXL) sOFF[threadIdx.x] = G.OFF[threadIdx.x];
    __syncthreads();
    const int npix = A.NPIX_X * A.NPIX_Y;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= npix) return;
    const float dx = A.DIR[0], dy = A.DIR[1], dz = A.DIR[2];
    const float tx = -dx, ty = -dy, tz = -dz;                             // away from the observer
    const float rx = -A.RA[0], ry = -A.RA[1], rz = -A.RA[2];              // "our RA is an axis pointing to the right" (:1083-1085)
    const float ex = A.DE[0], ey = A.DE[1], ez = A.DE[2];
    const float OPTSUM = A.SCA + A.ABS;
    float p0x, p0y, p0z;
    soc_pol_entry(G, A, id, p0x, p0y, p0z);
    float px = p0x, py = p0y, pz = p0z, dens = 0.0f, TAU = 0.0f;
    int   level = 0, ind = -1;
    soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);

    if (POLSTAT == 0) {                                                   // I, Q, U, column density (:1060-1126)
        float I = 0.0f, Q = 0.0f, U = 0.0f, colden = 0.0f, p = A.p0;
        while (ind >= 0) {
            const int   oind = sOFF[level] + ind, olevel = level;
            const float rho = dens;
            const float sx = soc_map_getstep<OCT, DBL>(G, sOFF, px, py, pz, tx, ty, tz, level, ind, dens);
            float DTAU;
            if (ABU) { const float2 o = A.OPT[oind];  DTAU = sx * rho * (o.x + o.y); }
            else     DTAU = sx * rho * OPTSUM;
            const float4 B = A.B[oind];
            float bx = B.x, by = B.y, bz = B.z;
            if (A.polred) p = soc_sqrtf(bx * bx + by * by + bz * bz);     // -D POLRED: p = |B|
            soc_normalize(bx, by, bz);
            const float Psi = 0.5f * SOC_POL_PI + soc_atan2f(soc_dot3(bx, by, bz, rx, ry, rz), soc_dot3(bx, by, bz, ex, ey, ez));
            const float bd = soc_dot3(bx, by, bz, dx, dy, dz);
            const float cc = 0.99999f - 0.99998f * bd * bd;               // cos^2 of the angle to the plane of the sky
            float sz;
            if (A.rho_weight) sz = sx * rho;                              // -D POL_RHO_WEIGHT
            else              sz = soc_pol_emitted(TAU, DTAU, sx, A.EMIT[oind], rho);
            if (olevel >= A.LEVEL_THRESHOLD) {                            // -D LEVEL_THRESHOLD: coarser cells only absorb (:1104)
                float s2, c2;
                soc_sincosf(2.0f * Psi, &s2, &c2);
                I += sz * (1.0f - p * (cc - 0.6666667f));
                Q += p * sz * c2 * cc;
                U += p * sz * s2 * cc;
            }
            TAU += DTAU;
            colden += sx * rho;
        }
        A.MAP[0 * (size_t)npix + id] = I;
        A.MAP[1 * (size_t)npix + id] = Q;
        A.MAP[2 * (size_t)npix + id] = U;
        A.MAP[3 * (size_t)npix + id] = colden * A.LENGTH;
    } else if (POLSTAT == 1) {                                            // rT, rI, jT, jI: two passes (:1229-1378)
        float sR = 0.0f, sJ = 0.0f, sRG = 0.0f, sJG = 0.0f, RQ = 0.0f, RU = 0.0f, JQ = 0.0f, JU = 0.0f;
        while (ind >= 0) {
            const int   oind = sOFF[level] + ind, olevel = level;
            float rho = dens;
            const float sx = soc_map_getstep<OCT, DBL>(G, sOFF, px, py, pz, tx, ty, tz, level, ind, dens);
            float DTAU;
            if (ABU) { const float2 o = A.OPT[oind];  DTAU = sx * rho * (o.x + o.y); }
            else     DTAU = sx * rho * OPTSUM;
            const float4 B = A.B[oind];
            float bx = B.x, by = B.y, bz = B.z;
            const float PR = soc_sqrtf(bx * bx + by * by + bz * bz);
            soc_normalize(bx, by, bz);
            const float Psi = 0.5f * SOC_POL_PI + soc_atan2f(soc_dot3(bx, by, bz, rx, ry, rz), soc_dot3(bx, by, bz, ex, ey, ez));
            const float bd = soc_dot3(bx, by, bz, dx, dy, dz);
            const float cc = 0.99999f - 0.99998f * bd * bd;
            float sz = soc_pol_emitted(TAU, DTAU, sx, A.EMIT[oind], rho);
            if (olevel < A.LEVEL_THRESHOLD) { sz = 0.0f;  rho = 0.0f; }   // (:1263)
            float s2, c2;
            soc_sincosf(2.0f * Psi, &s2, &c2);
            if (A.polred) {
                sR  += rho * sx * PR;
                sRG += rho * sx * PR * cc;
                RQ  += rho * sx * PR * c2 * cc;
                RU  += rho * sx * PR * s2 * cc;
                sJ  += sz * PR;
                sJG += sz * PR * cc;
                JQ  += sz * PR * c2 * cc;
                JU  += sz * PR * s2 * cc;
            } else {
                sR  += rho * sx;
                sRG += rho * sx * cc;
                RQ  += rho * sx * c2 * cc;
                RU  += rho * sx * s2 * cc;
                sJ  += sz;
                sJG += sz * cc;
                JQ  += sz * c2 * cc;
                JU  += sz * s2 * cc;
            }
            TAU += DTAU;
        }
        A.MAP[1 * (size_t)npix + id] = soc_acosf(soc_sqrtf(sRG / sR));
        A.MAP[3 * (size_t)npix + id] = soc_acosf(soc_sqrtf(sJG / sJ));
        const float RChi = (float)(0.5 * soc_atan2f(RU, RQ));             // "0.5*atan2(...)": the literal is a double (:1305-1306)
        const float JChi = (float)(0.5 * soc_atan2f(JU, JQ));
        px = p0x;  py = p0y;  pz = p0z;
        soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
        TAU = 0.0f;
        float sRP = 0.0f, sJP = 0.0f;
        sR = 0.0f;  sJ = 0.0f;
        while (ind >= 0) {
            const int   oind = sOFF[level] + ind, olevel = level;
            float rho = dens;
            const float sx = soc_map_getstep<OCT, DBL>(G, sOFF, px, py, pz, tx, ty, tz, level, ind, dens);
            float DTAU;
            if (ABU) { const float2 o = A.OPT[oind];  DTAU = sx * rho * (o.x + o.y); }
            else     DTAU = sx * rho * OPTSUM;
            const float4 B = A.B[oind];
            float bx = B.x, by = B.y, bz = B.z;
            const float PR = soc_sqrtf(bx * bx + by * by + bz * bz);
            soc_normalize(bx, by, bz);
            const float Chi = 0.5f * SOC_POL_PI + soc_atan2f(soc_dot3(bx, by, bz, rx, ry, rz), soc_dot3(bx, by, bz, ex, ey, ez));
            float sz = soc_pol_emitted(TAU, DTAU, sx, A.EMIT[oind], rho);
            if (olevel < A.LEVEL_THRESHOLD) { sz = 0.0f;  rho = 0.0f; }   // (:1339)
            float d = soc_fmodf_small(soc_fabsf(SOC_POL_TWOPI + RChi - Chi), SOC_POL_PI);
            if (d > SOC_POL_PIHALF) d = SOC_POL_PI - d;
            float e = soc_fmodf_small(soc_fabsf(SOC_POL_TWOPI + JChi - Chi), SOC_POL_PI);
            if (e > SOC_POL_PIHALF) e = SOC_POL_PI - e;
            if (A.polred) {
                sR  += rho * PR * sx;
                sRP += rho * PR * sx * d * d;
                sJ  += sz * PR;
                sJP += sz * PR * e * e;
            } else {
                sR  += rho * sx;
                sRP += rho * sx * d * d;
                sJ  += sz;
                sJP += sz * e * e;
            }
            TAU += DTAU;
        }
        A.MAP[0 * (size_t)npix + id] = soc_sqrtf(sRP / sR);
        A.MAP[2 * (size_t)npix + id] = soc_sqrtf(sJP / sJ);
    } else {                                                              // <B>, <B_LOS>, <B_POS>, tau (:1661-1687)
        float SUM_BPOS = 0.0f, SUM_BLOS = 0.0f, SUM_B = 0.0f, WEIGHT = 0.0f;
        while (ind >= 0) {
            const int   oind = sOFF[level] + ind, olevel = level;
            float rho = dens;
            const float sx = soc_map_getstep<OCT, DBL>(G, sOFF, px, py, pz, tx, ty, tz, level, ind, dens);
            float DTAU;
            if (ABU) { const float2 o = A.OPT[oind];  DTAU = sx * rho * (o.x + o.y); }
            else     DTAU = sx * rho * OPTSUM;
            const float4 B = A.B[oind];
            if (olevel < A.LEVEL_THRESHOLD) rho = 0.0f;                   // (:1674)
            const float br = soc_dot3(B.x, B.y, B.z, rx, ry, rz), be = soc_dot3(B.x, B.y, B.z, ex, ey, ez);
            WEIGHT   += sx * rho;
            SUM_B    += sx * rho * soc_sqrtf(B.x * B.x + B.y * B.y + B.z * B.z);
            SUM_BLOS += sx * rho * soc_fabsf(soc_dot3(B.x, B.y, B.z, tx, ty, tz));
            SUM_BPOS += sx * rho * soc_sqrtf(br * br + be * be);          // pow(x, 2.0f) is the exact square, rounded once
            TAU      += DTAU;
        }
        A.MAP[0 * (size_t)npix + id] = SUM_B / WEIGHT;
        A.MAP[1 * (size_t)npix + id] = SUM_BLOS / WEIGHT;
        A.MAP[2 * (size_t)npix + id] = SUM_BPOS / WEIGHT;
        A.MAP[3 * (size_t)npix + id] = TAU;
    }
}

template <int POLSTAT>
static void soc_polmap_dispatch(const SocGrid &G, const SocPolArgs &A, bool abu, dim3 grid, dim3 block, hipStream_t st)
{
    const bool oct = G.LEVELS > 1, dbl = oct && (G.NX > 100);            // kernel_ASOC_map.c:297
    if (!oct)      { if (abu) soc_polmap_kernel<false, false, true, POLSTAT><<<grid, block, 0, st>>>(G, A); else soc_polmap_kernel<false, false, false, POLSTAT><<<grid, block, 0, st>>>(G, A); }
    else if (!dbl) { if (abu) soc_polmap_kernel<true, false, true, POLSTAT><<<grid, block, 0, st>>>(G, A);  else soc_polmap_kernel<true, false, false, POLSTAT><<<grid, block, 0, st>>>(G, A); }
    else           { if (abu) soc_polmap_kernel<true, true, true, POLSTAT><<<grid, block, 0, st>>>(G, A);   else soc_polmap_kernel<true, true, false, POLSTAT><<<grid, block, 0, st>>>(G, A); }
}

hipError_t soc_launch_polmap(const SocGrid &G, const SocPolArgs &A, bool abu, hipStream_t st)
{
    const int npix = A.NPIX_X * A.NPIX_Y;
    if (npix <= 0) return hipSuccess;
    const dim3 grid((npix + 255) / 256), block(256);
    if (A.polstat == 0)      soc_polmap_dispatch<0>(G, A, abu, grid, block, st);
    else if (A.polstat == 1) soc_polmap_dispatch<1>(G, A, abu, grid, block, st);
    else if (A.polstat == 3) soc_polmap_dispatch<3>(G, A, abu, grid, block, st);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// all-sky polarisation map: PolHealpixMapping of kernel_ASOC_map_H.c, -D POLSTAT=0 (:576-841)
// ------------------------------------------------------------------------------------
// One lane per RING pixel; I, Q, U and the column density as seen from INTOBS inside the model.  That file carries its
// own walk (:179-380).  Compared with kernel_ASOC_map.c: IndexG (:179-212) is the same text and GetStep (:297-326) the same
// arithmetic (PEPS = 5e-4; the other file's double branch for NX > 9999 is missing here) -- soc_indexg and
// soc_map_getstep are reused; Index (:216-289) differs, see soc_map_index<.., HFILE = true>.  The consequence is restated,
// not repaired: on a hierarchy a ray that steps from an octet into a root leaf goes on from the corner of the grid.
// -D INTERPOLATE is compiled in; mode 3 keeps its 27 look-ups in registers.  -D POLRED, LEVEL_THRESHOLD, p00, MINLOS and
// MAXLOS are launch arguments.  The extinction of a step is ABS + SCA, or the per-cell sum the file has under
// "#ifdef USE_ABU" (:736-740) when the handle holds per-cell opacities.  A ray ends after SOC_HPOL_MAXSTEPS steps.
template <bool OCT, bool DBL, bool ABU, int INTERP>
__global__ __launch_bounds__(256) void soc_hpolmap_kernel(const SocGrid G, const SocHPolArgs A)
{
    __shared__ int sOFF[SOC_MAXL];
    if (threadIdx.x < SOC_MAXL) sOFF[threadIdx.x] = G.OFF[threadIdx.x];
    __syncthreads();
    const int npix = 12 * A.NSIDE * A.NSIDE;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= npix) return;
    const int NX = G.NX, NY = G.NY, NZ = G.NZ;
    float phi, theta, st, ct, sp, cp;
    soc_pixel2angles_ring(A.NSIDE, id, phi, theta);
    soc_sincosf(theta, &st, &ct);
    soc_sincosf(phi, &sp, &cp);
    float tx = +st * cp, ty = +st * sp, tz = -ct;                          // HDIR (:616-621)
    if (soc_fabsf(tx) < 1.0e-5f) tx = 1.0e-5f;
    if (soc_fabsf(ty) < 1.0e-5f) ty = 1.0e-5f;
    if (soc_fabsf(tz) < 1.0e-5f) tz = 1.0e-5f;
    float px = A.INTOBS[0], py = A.INTOBS[1], pz = A.INTOBS[2];
    if ((soc_fmod1f(px) < 1.0e-5f) || (soc_fmod1f(px) < 0.99999f)) px += 2.0e-5f;       // as written (:623-625)
    if ((soc_fmod1f(py) < 1.0e-5f) || (soc_fmod1f(py) < 0.99999f)) py += 2.0e-5f;
    if ((soc_fmod1f(pz) < 1.0e-5f) || (soc_fmod1f(pz) < 0.99999f)) pz += 2.0e-5f;
    const float rx = -sp, ry = +cp, rz = 0.0f;                             // HRA points left, HDE to the north (:628-634)
    const float ex = -ct * cp, ey = -ct * sp, ez = +st;
    const float OPTSUM = A.SCA + A.ABS;
    int   level = 0, ind = -1;
    float dens = 0.0f, TAU = 0.0f, colden = 0.0f, los = 0.0f, I = 0.0f, Q = 0.0f, U = 0.0f, p = A.p0;
    soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
    for (int steps = 0; (ind >= 0) && (steps < SOC_HPOL_MAXSTEPS); steps++) {
        const int   oind = sOFF[level] + ind, olevel = level;
        float mx = px, my = py, mz = pz;                                   // MPOS, the position before the step
        float rho = dens;
        float sx = soc_map_getstep<OCT, DBL, true>(G, sOFF, px, py, pz, tx, ty, tz, level, ind, dens);
        if (INTERP > 0) { const float h = 0.5f * sx;  mx = mx + h * tx;  my = my + h * ty;  mz = mz + h * tz; }
        if (INTERP == 1) {                                                 // four points of a Cartesian grid (:654-682)
            const int i0 = min(max((int)soc_floorf(mx), 0), NX - 1), j0 = min(max((int)soc_floorf(my), 0), NY - 1),
                      k0 = min(max((int)soc_floorf(mz), 0), NZ - 1);
            mx = soc_fmod1f(mx) - 0.5f;  my = soc_fmod1f(my) - 0.5f;  mz = soc_fmod1f(mz) - 0.5f;
            float sum = (3.0f - soc_fabsf(mx) - soc_fabsf(my) - soc_fabsf(mz)) * rho;
            if (mx > 0.0f) sum += mx * G.DENS[k0 * NX * NY + j0 * NX + max(0, i0 - 1)];
            else           sum += -mx * G.DENS[k0 * NX * NY + j0 * NX + min(i0 + 1, NX - 1)];
            if (my > 0.0f) sum += +my * G.DENS[k0 * NX * NY + max(j0 - 1, 0) * NX + i0];
            else           sum += -my * G.DENS[k0 * NX * NY + min(j0 + 1, NY - 1) * NX + i0];
            if (mz > 0.0f) sum += +mz * G.DENS[max(k0 - 1, 0) * NX * NY + j0 * NX + i0];
            else           sum += -mz * G.DENS[min(k0 + 1, NZ - 1) * NX * NY + j0 * NX + i0];
            rho = 0.333333f * sum;
        }
        if (INTERP == 2) {                                                 // 3 x 3 x 3 cells, inverse-distance weights (:686-707)
            const int i0 = (int)soc_floorf(mx), j0 = (int)soc_floorf(my), k0 = (int)soc_floorf(mz);
            float sum = 0.0f, weight = 0.0f;
            for (int k = max(0, k0 - 1); k < min(k0 + 2, NZ); k++)
                for (int j = max(0, j0 - 1); j < min(j0 + 2, NY); j++)
                    for (int i = max(0, i0 - 1); i < min(i0 + 2, NX); i++) {
                        const float ax = mx - (i + 0.5f), ay = my - (j + 0.5f), az = mz - (k + 0.5f);
                        const float w = 1.0f / (0.1f + soc_sqrtf(ax * ax + ay * ay + az * az));
                        weight += w;
                        sum += w * G.DENS[k * NY * NX + j * NX + i];
                    }
            rho = sum / weight;
        }
        if (INTERP == 3) {                                                 // 27 IndexG look-ups at +- the cell size (:711-733)
            float sum = 0.0f, weight = 0.0f;
            const float delta = soc_scale_down(1.0f, olevel);             // pow(0.5f, olevel)
            for (int k = -1; k < 2; k++)
                for (int j = -1; j < 2; j++)
                    for (int i = -1; i < 2; i++) {
                        float ax = mx + i * delta, ay = my + j * delta, az = mz + k * delta, nd = 0.0f;
                        int   mlevel = 0, mind = -1;
                        soc_indexg<OCT>(G, sOFF, ax, ay, az, mlevel, mind, nd);
                        if (mind >= 0) {
                            const float w = 1.0f / soc_sqrtf(0.2f + (float)(i * i) + (float)(j * j) + (float)(k * k));
                            weight += w;
                            sum += w * nd;
                        }
                    }
            rho = sum / weight;
        }
        float DTAU;
        if (ABU) { const float2 o = A.OPT[oind];  DTAU = sx * rho * (o.x + o.y); }
        else     DTAU = sx * rho * OPTSUM;
        los += sx;
        if (los > A.MAXLOS) {                                              // trims the step, not DTAU (:743-746)
            ind = -1;  pz = -1.0f;
            sx = A.MAXLOS - (los - sx);
        }
        const float4 B = A.B[oind];
        float bx = B.x, by = B.y, bz = B.z;
        if (A.polred) p = soc_sqrtf(bx * bx + by * by + bz * bz);          // -D POLRED: p = |B|
        soc_normalize(bx, by, bz);
        // "0.5*PI+atan2(...)": the literal is a double (:768)
        const float Psi = (float)(0.5 * (double)SOC_POL_PI + (double)soc_atan2f(soc_dot3(bx, by, bz, rx, ry, rz), soc_dot3(bx, by, bz, ex, ey, ez)));
        const float bd = soc_dot3(bx, by, bz, tx, ty, tz);
        const float cc = 0.99999f - 0.99998f * bd * bd;
        const float sz = soc_pol_emitted(TAU, DTAU, sx, A.EMIT[oind], rho);
        if (los < A.MINLOS) continue;                                      // nothing registered yet, TAU and the shear included (:776)
        if (olevel >= A.LEVEL_THRESHOLD) {
            float s2, c2;
            soc_sincosf(2.0f * Psi, &s2, &c2);
            I += sz * (1.0f - p * (cc - 0.6666667f));
            Q += p * sz * c2 * cc;
            U += p * sz * s2 * cc;
        }
        TAU += DTAU;
        colden += sx * rho;
        if ((A.Y_SHEAR != 0.0f) && (ind < 0) && (los < A.MAXLOS)) {        // shearing box: re-entry in x and y (:800-826)
            if ((pz > 0.0f) && (pz < NZ)) {
                if (py < 0.0f) py = NY - SOC_MAP_PEPS;
                if (py > NY)   py = +SOC_MAP_PEPS;
                if (px < 0.0f) { px = NX - SOC_MAP_PEPS;  py = soc_fmodf_small(py + NY - A.Y_SHEAR, (float)NY); }
                if (px > NX)   { px = +SOC_MAP_PEPS;      py = soc_fmodf_small(py + A.Y_SHEAR, (float)NY); }
                soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
            }
        }
    }
    A.MAP[0 * (size_t)npix + id] = I;
    A.MAP[1 * (size_t)npix + id] = Q;
    A.MAP[2 * (size_t)npix + id] = U;
    A.MAP[3 * (size_t)npix + id] = colden * A.LENGTH;
}

template <bool OCT, bool DBL, int INTERP>
static void soc_hpolmap_launch(const SocGrid &G, const SocHPolArgs &A, bool abu, dim3 grid, dim3 block, hipStream_t st)
{
    if (abu) soc_hpolmap_kernel<OCT, DBL, true, INTERP><<<grid, block, 0, st>>>(G, A);
    else     soc_hpolmap_kernel<OCT, DBL, false, INTERP><<<grid, block, 0, st>>>(G, A);
}

hipError_t soc_launch_hpolmap(const SocGrid &G, const SocHPolArgs &A, bool abu, hipStream_t st)
{
    const int npix = 12 * A.NSIDE * A.NSIDE;
    if (npix <= 0) return hipSuccess;
    const dim3 grid((npix + 255) / 256), block(256);
    const bool oct = G.LEVELS > 1, dbl = oct && (G.NX > 100);            // kernel_ASOC_map_H.c:14, :222
    const int  m = A.INTERPOLATE;
    if ((m < 0) || (m > 3) || (oct && ((m == 1) || (m == 2)))) return hipErrorInvalidValue;   // 1, 2 index level 0 as a plain grid
    if (!oct) {
        if (m == 0)      soc_hpolmap_launch<false, false, 0>(G, A, abu, grid, block, st);
        else if (m == 1) soc_hpolmap_launch<false, false, 1>(G, A, abu, grid, block, st);
        else if (m == 2) soc_hpolmap_launch<false, false, 2>(G, A, abu, grid, block, st);
        else             soc_hpolmap_launch<false, false, 3>(G, A, abu, grid, block, st);
    } else if (!dbl) {
        if (m == 0) soc_hpolmap_launch<true, false, 0>(G, A, abu, grid, block, st);
        else        soc_hpolmap_launch<true, false, 3>(G, A, abu, grid, block, st);
    } else {
        if (m == 0) soc_hpolmap_launch<true, true, 0>(G, A, abu, grid, block, st);
        else        soc_hpolmap_launch<true, true, 3>(G, A, abu, grid, block, st);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// per-level maps: Mapping of kernel_ASOC_map_H.c (:380-497), `mapping nx ny dx 999`
// ------------------------------------------------------------------------------------
// One lane per pixel; plane ilev of MAP holds what the cells of hierarchy level ilev emit towards the pixel, seen through
// everything in front of them.  The entry is that file's, not soc_map_entry: the external view starts behind the cloud and
// takes the largest face crossing (soc_pol_entry is the same text, :438-459) and walks along -DIR without clamping it; the
// perspective view looks along (-cos t sin p, -cos t cos p, sin t).  The walk is that file's too (soc_map_index<.., HFILE = true>).
// That Mapping tests neither MAP_INTERPOLATION, LEVEL_THRESHOLD nor ROI_MAP: `mapint`, `threshold` and `roimap` have no effect
// here, as in the reference.  The extinction of a step is ABS + SCA, or the per-cell sum that file keeps under "#ifdef USE_ABU"
// (:474-478) when the handle holds per-cell opacities.  A ray ends after SOC_MAPLEV_MAXSTEPS steps (soc_dev.h).
// The LEVELS accumulators are registers: NL is a template argument, the loops over it are unrolled and a step adds to the one
// of its level under a compare-select -- an array indexed by the run-time level would live in scratch.
template <bool OCT, bool DBL, bool ABU, int NL>
__global__ __launch_bounds__(256) void soc_maplev_kernel(const SocGrid G, const SocMapLevArgs A)
{
    __shared__ int sOFF[SOC_MAXL];
    if (threadIdx.x < SOC_MAXL) sOFF[threadIdx.x] = G.OFF[threadIdx.x];
    __syncthreads();
    const int npix = A.NPIX_X * A.NPIX_Y;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= npix) return;
    float PHOTONS[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) PHOTONS[l] = 0.0f;
    float px, py, pz, tx, ty, tz;
    if (A.INTOBS[0] > -1e10f) {                                           // perspective image from inside the model (:412-434)
        const int i = id % A.NPIX_X, j = id / A.NPIX_X;
        float phi = SOC_POL_TWOPI * i / (float)(A.NPIX_X);
        phi += SOC_POL_PI;
        const float pix = SOC_POL_TWOPI / A.NPIX_X;
        const float theta = pix * (j - (A.NPIX_Y - 1) / 2);
        float st, ct, sp, cp;
        soc_sincosf(theta, &st, &ct);
        soc_sincosf(phi, &sp, &cp);
        px = A.INTOBS[0];  py = A.INTOBS[1];  pz = A.INTOBS[2];
        tx = -ct * sp;  ty = -ct * cp;  tz = +st;
        if (soc_fabsf(tx) < 1.0e-5f) tx = 1.0e-5f;
        if (soc_fabsf(ty) < 1.0e-5f) ty = 1.0e-5f;
        if (soc_fabsf(tz) < 1.0e-5f) tz = 1.0e-5f;
        if (soc_fmod1f(px) < 1.0e-5f) px += 2.0e-5f;
        if (soc_fmod1f(py) < 1.0e-5f) py += 2.0e-5f;
        if (soc_fmod1f(pz) < 1.0e-5f) pz += 2.0e-5f;
    } else {                                                              // external map (:436-460)
        soc_pol_entry(G, A, id, px, py, pz);
        tx = -A.DIR[0];  ty = -A.DIR[1];  tz = -A.DIR[2];
    }
    const float OPTSUM = A.SCA + A.ABS;
    int   level = 0, ind = -1;
    float dens = 0.0f, TAU = 0.0f;
    soc_indexg<OCT>(G, sOFF, px, py, pz, level, ind, dens);
    for (int steps = 0; (ind >= 0) && (steps < SOC_MAPLEV_MAXSTEPS); steps++) {
        const int   oind = sOFF[level] + ind, olevel = level;
        const float rho = dens;
        const float sx = soc_map_getstep<OCT, DBL, true>(G, sOFF, px, py, pz, tx, ty, tz, level, ind, dens);
        float DTAU;
        if (ABU) { const float2 o = A.OPT[oind];  DTAU = sx * rho * (o.x + o.y); }
        else     DTAU = sx * rho * OPTSUM;
        const float add = soc_pol_emitted(TAU, DTAU, sx, A.EMIT[oind], rho);                      // (:480-484)
#pragma unroll
        for (int l = 0; l < NL; l++) PHOTONS[l] = (olevel == l) ? (PHOTONS[l] + add) : PHOTONS[l];
        TAU += DTAU;
    }
#pragma unroll
    for (int l = 0; l < NL; l++)
        if (l < G.LEVELS) A.MAP[(size_t)l * npix + id] = PHOTONS[l];
}

// the accumulator counts soc_maplev_kernel is compiled for; a model runs in the narrowest that holds its levels
template <bool OCT, bool DBL, bool ABU>
static void soc_maplev_dispatch(const SocGrid &G, const SocMapLevArgs &A, dim3 grid, dim3 block, hipStream_t st)
{
    if (G.LEVELS <= 4)      soc_maplev_kernel<OCT, DBL, ABU, 4><<<grid, block, 0, st>>>(G, A);
    else if (G.LEVELS <= 8) soc_maplev_kernel<OCT, DBL, ABU, 8><<<grid, block, 0, st>>>(G, A);
    else                    soc_maplev_kernel<OCT, DBL, ABU, SOC_MAXL><<<grid, block, 0, st>>>(G, A);
}

hipError_t soc_launch_maplev(const SocGrid &G, const SocMapLevArgs &A, bool abu, hipStream_t st)
{
    const int npix = A.NPIX_X * A.NPIX_Y;
    if (npix <= 0) return hipSuccess;
    if (G.LEVELS < 1 || G.LEVELS > SOC_MAXL) return hipErrorInvalidValue;
    const dim3 grid((npix + 255) / 256), block(256);
    const bool oct = G.LEVELS > 1, dbl = oct && (G.NX > 100);            // kernel_ASOC_map_H.c:14, :222
    if (!oct)      { if (abu) soc_maplev_kernel<false, false, true, 4><<<grid, block, 0, st>>>(G, A); else soc_maplev_kernel<false, false, false, 4><<<grid, block, 0, st>>>(G, A); }
    else if (!dbl) { if (abu) soc_maplev_dispatch<true, false, true>(G, A, grid, block, st);  else soc_maplev_dispatch<true, false, false>(G, A, grid, block, st); }
    else           { if (abu) soc_maplev_dispatch<true, true, true>(G, A, grid, block, st);   else soc_maplev_dispatch<true, true, false>(G, A, grid, block, st); }
    return hipGetLastError();
}

// (Bx, By, Bz) -> one float4 per cell
__global__ void soc_pack_bfield_kernel(int cells, const float *Bx, const float *By, const float *Bz, float4 *B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells) B[i] = make_float4(Bx[i], By[i], Bz[i], 0.0f);
}

hipError_t soc_launch_pack_bfield(int cells, const float *Bx, const float *By, const float *Bz, float4 *B, hipStream_t st)
{
    if (cells <= 0) return hipSuccess;
    soc_pack_bfield_kernel<<<(cells + 255) / 256, 256, 0, st>>>(cells, Bx, By, Bz, B);
    return hipGetLastError();
}

hipError_t soc_launch_map(const SocGrid &G, const SocMapArgs &A, bool abu, hipStream_t st)
{
    const int npix = A.mode ? 12 * A.NPIX_X * A.NPIX_X : A.NPIX_X * A.NPIX_Y;
    if (npix <= 0) return hipSuccess;
    const dim3 grid((npix + 255) / 256), block(256);
    const bool oct = G.LEVELS > 1, dbl = oct && (G.NX > 100);            // kernel_ASOC_map.c:297
    if (!oct)      { if (abu) soc_map_kernel<false, false, true><<<grid, block, 0, st>>>(G, A); else soc_map_kernel<false, false, false><<<grid, block, 0, st>>>(G, A); }
    else if (!dbl) { if (abu) soc_map_kernel<true, false, true><<<grid, block, 0, st>>>(G, A);  else soc_map_kernel<true, false, false><<<grid, block, 0, st>>>(G, A); }
    else           { if (abu) soc_map_kernel<true, true, true><<<grid, block, 0, st>>>(G, A);   else soc_map_kernel<true, true, false><<<grid, block, 0, st>>>(G, A); }
    return hipGetLastError();
}

// The widths soc_mapx_kernel is compiled for; a batch runs in the narrowest that holds it.  Registers per lane (DESIGN.md
// section 5 has the table): the walk's own plus three per frequency, no scratch at any width up to SOC_MAPX_MAX.
template <bool OCT, bool DBL, bool ABU>
static void soc_mapx_dispatch(const SocGrid &G, const SocMapXArgs &A, dim3 grid, dim3 block, hipStream_t st)
{
    if (A.nf <= 4)       soc_mapx_kernel<OCT, DBL, ABU, 4><<<grid, block, 0, st>>>(G, A);
    else if (A.nf <= 8)  soc_mapx_kernel<OCT, DBL, ABU, 8><<<grid, block, 0, st>>>(G, A);
    else if (A.nf <= 16) soc_mapx_kernel<OCT, DBL, ABU, 16><<<grid, block, 0, st>>>(G, A);
    else                 soc_mapx_kernel<OCT, DBL, ABU, SOC_MAPX_MAX><<<grid, block, 0, st>>>(G, A);
}

hipError_t soc_launch_mapx(const SocGrid &G, const SocMapXArgs &A, hipStream_t st)
{
    const int npix = A.mode ? 12 * A.NPIX_X * A.NPIX_X : A.NPIX_X * A.NPIX_Y;
    if (npix <= 0) return hipSuccess;
    if (A.nf < 1 || A.nf > SOC_MAPX_MAX) return hipErrorInvalidValue;
    const dim3 grid((npix + 255) / 256), block(256);
    const bool oct = G.LEVELS > 1, dbl = oct && (G.NX > 100), abu = A.OPT != nullptr;   // kernel_ASOC_map.c:297
    if (!oct)      { if (abu) soc_mapx_dispatch<false, false, true>(G, A, grid, block, st); else soc_mapx_dispatch<false, false, false>(G, A, grid, block, st); }
    else if (!dbl) { if (abu) soc_mapx_dispatch<true, false, true>(G, A, grid, block, st);  else soc_mapx_dispatch<true, false, false>(G, A, grid, block, st); }
    else           { if (abu) soc_mapx_dispatch<true, true, true>(G, A, grid, block, st);   else soc_mapx_dispatch<true, true, false>(G, A, grid, block, st); }
    return hipGetLastError();
}

// The widths soc_maplevx_kernel is compiled for.  A launch's accumulators take LEVELS * KF KiB of LDS; the widest instance a model
// uses keeps that at or below 64 KiB (8 columns up to 8 levels, 4 up to SOC_MAXL), so two workgroups fit a CU.
int soc_maplevx_width(int LEVELS) { return (LEVELS <= 8) ? 8 : 4; }

template <bool OCT, bool DBL, bool ABU, int KF>
static hipError_t soc_maplevx_launch(const SocGrid &G, const SocMapLXArgs &A, dim3 grid, dim3 block, hipStream_t st)
{
    const size_t lds = (size_t)G.LEVELS * KF * 256 * sizeof(float) + 2 * SOC_MAXL * sizeof(int);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)soc_maplevx_kernel<OCT, DBL, ABU, KF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    soc_maplevx_kernel<OCT, DBL, ABU, KF><<<grid, block, lds, st>>>(G, A);
    return hipGetLastError();
}

template <bool OCT, bool DBL, bool ABU>
static hipError_t soc_maplevx_dispatch(const SocGrid &G, const SocMapLXArgs &A, dim3 grid, dim3 block, hipStream_t st)
{
    if (A.kf == 1)      return soc_maplevx_launch<OCT, DBL, ABU, 1>(G, A, grid, block, st);
    else if (A.kf <= 4) return soc_maplevx_launch<OCT, DBL, ABU, 4>(G, A, grid, block, st);
    else                return soc_maplevx_launch<OCT, DBL, ABU, 8>(G, A, grid, block, st);
}

// all A.nf columns of the resident batch, in launches of at most soc_maplevx_width columns (A.f0 and A.kf are set here)
hipError_t soc_launch_maplevx(const SocGrid &G, const SocMapLXArgs &A0, hipStream_t st)
{
    const int npix = A0.mode ? 12 * A0.NPIX_X * A0.NPIX_X : A0.NPIX_X * A0.NPIX_Y;
    if (npix <= 0) return hipSuccess;
    if (A0.nf < 1 || A0.nf > SOC_MAPX_MAX || G.LEVELS < 1 || G.LEVELS > SOC_MAXL) return hipErrorInvalidValue;
    const dim3 grid((npix + 255) / 256), block(256);
    const bool oct = G.LEVELS > 1, dbl = oct && (G.NX > 100), abu = A0.OPT != nullptr;   // kernel_ASOC_map.c:297
    const int  width = soc_maplevx_width(G.LEVELS);
    SocMapLXArgs A = A0;
    for (A.f0 = 0; A.f0 < A.nf; A.f0 += width) {
        A.kf = std::min(width, A.nf - A.f0);
        hipError_t e;
        if (!oct)      e = abu ? soc_maplevx_dispatch<false, false, true>(G, A, grid, block, st) : soc_maplevx_dispatch<false, false, false>(G, A, grid, block, st);
        else if (!dbl) e = abu ? soc_maplevx_dispatch<true, false, true>(G, A, grid, block, st)  : soc_maplevx_dispatch<true, false, false>(G, A, grid, block, st);
        else           e = abu ? soc_maplevx_dispatch<true, true, true>(G, A, grid, block, st)   : soc_maplevx_dispatch<true, true, false>(G, A, grid, block, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
