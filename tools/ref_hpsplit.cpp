// ref_hpsplit.cpp -- driver for the SimHpSplit kernel of the reference's kernel_ASOC.c (`split 1` with `hpbg`), compiled
// unmodified for x86-64 with -DDO_SPLIT=1 -DMAX_SPLIT -DHPBG_WEIGHTED by tools/make_hpsplit_golden.py (which records
// tests/golden/hpsplit.npz).  Run by hand; no test builds it.
#include "../oracle/ref_builtins.inc"

// the one OpenCL built-in that kernel needs beyond oracle/ref_builtins.inc
float cl_round(float x) CLNAME("_Z5roundf");
float cl_round(float x) { return roundf(x); }

extern "C" {
// kernel_ASOC.c:2871-2894 (OPT_IS_HALF = 0: OTYPE is float)
void SimHpSplit(int PACKETS, int BATCH, float SEED, float *ABS, float *SCA, float TW, int *LCELLS, int *OFF, int *PAR,
                float *DENS, float *EMIT, float *TABS, float *DSC, float *CSC, float *INT, float *INTX, float *INTY, float *INTZ,
                float *OPT, float *BG, float *HPBGP, float *ABU, float *BUFFER);

struct hpsplit_args {
    int   PACKETS, BATCH, GLOBAL;
    float SEED, TW;
    float *ABS, *SCA;
    int   *LCELLS, *OFF, *PAR;
    float *DENS, *EMIT, *TABS, *DSC, *CSC, *INT, *INTX, *INTY, *INTZ, *OPT, *BG, *HPBGP, *ABU, *BUFFER;
};

// all work items of the launch, one after the other in id order
void ref_hpsplit(const hpsplit_args *a)
{
    g_gsize = (size_t)a->GLOBAL;
    for (int id = 0; id < a->GLOBAL; id++) {
        g_gid = (size_t)id;
        SimHpSplit(a->PACKETS, a->BATCH, a->SEED, a->ABS, a->SCA, a->TW, a->LCELLS, a->OFF, a->PAR, a->DENS, a->EMIT, a->TABS,
                   a->DSC, a->CSC, a->INT, a->INTX, a->INTY, a->INTZ, a->OPT, a->BG, a->HPBGP, a->ABU, a->BUFFER);
    }
}
}
