// ref_polmap.cpp -- driver for the PolMapping kernel of the reference's kernel_ASOC_map.c, compiled unmodified for
// x86-64 by tools/make_polmap_golden.py (which records tests/golden/polmaps.npz).  Run by hand; no test builds it.
#include "../oracle/ref_builtins.inc"

typedef int int2 __attribute__((ext_vector_type(2)));

extern "C" {
// the argument list is the same for -D POLSTAT=0, 1 and 3 (kernel_ASOC_map.c:974-994, :1164-1184, :1600-1620)
void PolMapping(float MAP_DX, int2 NPIX, float *MAP, float *EMIT, float3 DIR, float3 RA, float3 DE, int *LCELLS, int *OFF,
                int *PAR, float *DENS, float ABS, float SCA, float3 CENTRE, float3 INTOBS, float *Bx, float *By, float *Bz,
                float *OPT);

struct polmap_args {
    int   NPIX_X, NPIX_Y;
    float MAP_DX, ABS, SCA;
    float DIR[4], RA[4], DE[4], CENTRE[4];
    int   *LCELLS, *OFF, *PAR;
    float *DENS, *EMIT, *OPT, *Bx, *By, *Bz, *MAP;
};

static float3 f3of(const float *p) { float3 v;  v.x = p[0];  v.y = p[1];  v.z = p[2];  return v; }

// all pixels (work items) of one map
void ref_polmap(const polmap_args *a)
{
    float dummy[8] = { 0 };
    float3 INTOBS;  INTOBS.x = -1.0e12f;  INTOBS.y = 0.0f;  INTOBS.z = 0.0f;
    int2  NPIX;  NPIX.x = a->NPIX_X;  NPIX.y = a->NPIX_Y;
    const int npixels = a->NPIX_X * a->NPIX_Y;
    g_gsize = (size_t)npixels;
    for (int id = 0; id < npixels; id++) {
        g_gid = (size_t)id;
        PolMapping(a->MAP_DX, NPIX, a->MAP, a->EMIT, f3of(a->DIR), f3of(a->RA), f3of(a->DE), a->LCELLS, a->OFF, a->PAR, a->DENS,
                   a->ABS, a->SCA, f3of(a->CENTRE), INTOBS, a->Bx, a->By, a->Bz, a->OPT ? a->OPT : dummy);
    }
}
}
