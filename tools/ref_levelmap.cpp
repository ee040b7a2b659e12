// ref_levelmap.cpp -- driver for the per-level Mapping kernel of the reference's kernel_ASOC_map_H.c (`mapping nx ny dx 999`),
// compiled unmodified for x86-64 by tools/make_levelmap_golden.py (which records tests/golden/levelmaps.npz).  Run by hand; no
// test builds it.
#include "../oracle/ref_builtins.inc"

typedef int int2 __attribute__((ext_vector_type(2)));

// the one OpenCL built-in that file needs beyond oracle/ref_builtins.inc
int cl_mini(int a, int b) CLNAME("_Z3minii");
int cl_mini(int a, int b) { return b < a ? b : a; }

extern "C" {
// kernel_ASOC_map_H.c:380-398 (OPT_IS_HALF = 0: OTYPE is float)
void Mapping(float DX, int2 NPIX, float *MAP, float *EMIT, float3 DIR, float3 RA, float3 DE, int *LCELLS, int *OFF, int *PAR,
             float *DENS, float ABS, float SCA, float3 CENTRE, float3 INTOBS, float *OPT, float *COLDEN);

struct levelmap_args {
    int   NPIX_X, NPIX_Y;
    float MAP_DX, ABS, SCA;
    float DIR[4], RA[4], DE[4], CENTRE[4], INTOBS[4];
    int   *LCELLS, *OFF, *PAR;
    float *DENS, *EMIT, *OPT, *MAP;
};

static float3 f3of(const float *p) { float3 v;  v.x = p[0];  v.y = p[1];  v.z = p[2];  return v; }

// all pixels (work items) of one view, plus the padding of the launch (ASOC.py:3356): those must return at the guard
void ref_levelmap(const levelmap_args *a)
{
    float dummy[8] = { 0 };
    int2  NPIX;  NPIX.x = a->NPIX_X;  NPIX.y = a->NPIX_Y;
    const int npix = a->NPIX_X * a->NPIX_Y, global = (1 + npix / 64) * 64;
    g_gsize = (size_t)global;
    for (int id = 0; id < global; id++) {
        g_gid = (size_t)id;
        Mapping(a->MAP_DX, NPIX, a->MAP, a->EMIT, f3of(a->DIR), f3of(a->RA), f3of(a->DE), a->LCELLS, a->OFF, a->PAR, a->DENS, a->ABS,
                a->SCA, f3of(a->CENTRE), f3of(a->INTOBS), a->OPT ? a->OPT : dummy, dummy);
    }
}
}
