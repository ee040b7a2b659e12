// ref_library.cpp -- driver for the LibrarySolve kernel of the reference's kernel_soc_library.c, compiled unmodified for x86-64
// with -DMETHOD=0 -DN -DNFREQ -DLOCAL -DCELLS by tools/make_library_golden.py (which records tests/golden/library.npz).  Run by
// hand; no test builds it.
#include "../oracle/ref_builtins.inc"

// the one OpenCL built-in that kernel needs beyond oracle/ref_builtins.inc
float cl_round(float x) CLNAME("_Z5roundf");
float cl_round(float x) { return roundf(x); }

extern "C" {
// kernel_soc_library.c:6-18
void LibrarySolve(int no, float I0, float dI0, float *I1, float *dI1, float *I2, float *dI2, float *X, float *Y, float *Z, float *E,
                  float *ABS, float *EMI);

struct library_args {
    int   no;
    float I0, dI0;
    float *I1, *dI1, *I2, *dI2, *X, *Y, *Z, *E, *ABS, *EMI;
};

// all work items of the launch, one after the other in id order
void ref_library(const library_args *a)
{
    g_gsize = (size_t)a->no;
    for (int id = 0; id < a->no; id++) {
        g_gid = (size_t)id;
        LibrarySolve(a->no, a->I0, a->dI0, a->I1, a->dI1, a->I2, a->dI2, a->X, a->Y, a->Z, a->E, a->ABS, a->EMI);
    }
}
}
