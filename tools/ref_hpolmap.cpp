// ref_hpolmap.cpp -- driver for the PolHealpixMapping kernel of the reference's kernel_ASOC_map_H.c, compiled unmodified for
// x86-64 by tools/make_hpolmap_golden.py (which records tests/golden/hpolmaps.npz).  Run by hand; no test builds it.
#include "../oracle/ref_builtins.inc"

typedef int int2 __attribute__((ext_vector_type(2)));

// the one OpenCL built-in that file needs beyond oracle/ref_builtins.inc
int cl_mini(int a, int b) CLNAME("_Z3minii");
int cl_mini(int a, int b) { return b < a ? b : a; }

extern "C" {
// kernel_ASOC_map_H.c:576-597 (-D POLSTAT=0)
void PolHealpixMapping(float DX, int2 NPIX, float *MAP, float *EMIT, float3 DIR, float3 RA, float3 DE, int *LCELLS, int *OFF,
                       int *PAR, float *DENS, float ABS, float SCA, float3 CENTRE, float3 INTOBS, float *Bx, float *By, float *Bz,
                       float *OPT, float Y_SHEAR);

struct hpolmap_args {
    int   NSIDE;
    float ABS, SCA, Y_SHEAR;
    float INTOBS[4];
    int   *LCELLS, *OFF, *PAR;
    float *DENS, *EMIT, *OPT, *Bx, *By, *Bz, *MAP;
};

// all pixels (work items) of one map, plus the padding of the launch (ASOC.py:3895): those must return at the guard
void ref_hpolmap(const hpolmap_args *a)
{
    float dummy[8] = { 0 };
    float3 zero;  zero.x = 0.0f;  zero.y = 0.0f;  zero.z = 0.0f;
    float3 INTOBS;  INTOBS.x = a->INTOBS[0];  INTOBS.y = a->INTOBS[1];  INTOBS.z = a->INTOBS[2];
    int2  NPIX;  NPIX.x = a->NSIDE;  NPIX.y = -1;
    const int npix = 12 * a->NSIDE * a->NSIDE, global = (1 + npix / 64) * 64;
    g_gsize = (size_t)global;
    for (int id = 0; id < global; id++) {
        g_gid = (size_t)id;
        PolHealpixMapping(1.0f, NPIX, a->MAP, a->EMIT, zero, zero, zero, a->LCELLS, a->OFF, a->PAR, a->DENS, a->ABS, a->SCA, zero,
                          INTOBS, a->Bx, a->By, a->Bz, a->OPT ? a->OPT : dummy, a->Y_SHEAR);
    }
}
}
