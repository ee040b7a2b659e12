/*
 * library_host.c -- plain-C restatement of the library method for dust emission: the look-up (LibrarySolve with METHOD 0,
 * kernel_soc_library.c:27-51, with the host loop of soc_library.py:379-406 around it) and the construction of the grid and of
 * the representative cells (soc_library.py:127-217).  TEST INFRASTRUCTURE ONLY (tests/library_host.py builds and binds it;
 * tools/make_library_golden.py pins the look-up against the reference).
 *
 * Two math modes, as the oracle has them: -DSOC_ORACLE_LIBM takes libm's log10f (what the reference's x86 build and numpy
 * compute), the default soc_math.h's soc_log10f (what the HIP kernels compute).  Everything else is fp32 +, -, *, / in the
 * order the reference writes it (-ffp-contract=off).
 *
 * The build is stated the slow way on purpose -- one masked pass over all cells per window, as the reference's host loops
 * do -- so that it checks the device's binned sweeps, which visit every cell once and try three candidate windows.
 *
 * Where the reference leaves a case open, this file and the kernels define it the same way:
 *   - a missed row is 1e32 followed by zeros (the reference writes element 0 only);
 *   - an index is clamped before it is converted (a value no int holds clamps by its sign, a NaN gives 0);
 *   - the build clips I and J before they index I1 and I2 (numpy would wrap a negative index or raise);
 *   - the build's distance |X-I| + |Y-J| + |Z-K| is summed in fp32, left to right.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../soc_amd/csrc/soc_math.h"

#ifdef SOC_ORACLE_LIBM
#  define LH_LOG10(x) log10f(x)
#else
#  define LH_LOG10(x) soc_log10f(x)
#endif

int lh_math_mode(void)
{
#ifdef SOC_ORACLE_LIBM
    return 0;
#else
    return 1;
#endif
}

/* the logarithm of this mode, for the tests that compare it with numpy's */
void lh_log10(long n, const float *x, float *y)
{
    for (long c = 0; c < n; c++) y[c] = LH_LOG10(x[c]);
}

static float lh_clip(float x, float lo, float hi)
{
    x = x < lo ? lo : x;
    return x > hi ? hi : x;
}

/* OpenCL round(): halves away from zero; x - trunc(x) is exact */
static float lh_round_away(float x)
{
    const float t = truncf(x);
    if (fabsf(x - t) >= 0.5f) return t + (x < 0.0f ? -1.0f : 1.0f);
    return t;
}

static int lh_index(float r, int N)
{
    if (!(r > 0.0f)) return 0;
    if (r >= (float)(N - 1)) return N - 1;
    return (int)r;
}

/* ABS: row-major, `stride` floats per cell, reference columns col[3].  E[N^3][NFREQ]; ocol (or NULL) selects nout columns.
 * EMI[n][nout]; ijkm (or NULL) [n][4] receives i, j, k and the miss flag; miss (or NULL) the missed cells, *nmiss their count. */
void lh_solve(int N, int NFREQ, int nout, const int *ocol, float I0, float dI0, const float *I1, const float *dI1, const float *I2,
              const float *dI2, const float *X, const float *Y, const float *Z, const float *E, long n, const float *ABS, long stride,
              const int *col, float *EMI, int *ijkm, int *miss, long *nmiss)
{
    long m = 0;
    for (long c = 0; c < n; c++) {
        const float *a = ABS + c * stride;
        const float x = (LH_LOG10(lh_clip(a[col[0]], 1.0e-29f, 1.0e10f)) - I0) / dI0;
        const int   i = lh_index(lh_round_away(x), N);
        const float y = (LH_LOG10(lh_clip(a[col[1]], 1.0e-29f, 1.0e10f)) - I1[i]) / dI1[i];
        const int   j = lh_index(lh_round_away(y), N);
        const float z = (LH_LOG10(lh_clip(a[col[2]], 1.0e-29f, 1.0e10f)) - I2[i * N + j]) / dI2[i * N + j];
        const int   k = lh_index(lh_round_away(z), N);
        const long  b = k + (long)N * (j + N * i);
        const int bad = fabsf(x - X[b]) > 1.1f || fabsf(y - Y[b]) > 1.1f || fabsf(z - Z[b]) > 1.1f || E[b * NFREQ] > 1.0e31f;
        float *out = EMI + c * nout;
        for (int s = 0; s < nout; s++) out[s] = bad ? (s == 0 ? 1.0e32f : 0.0f) : E[b * NFREQ + (ocol ? ocol[s] : s)];
        if (ijkm) { ijkm[4 * c] = i;  ijkm[4 * c + 1] = j;  ijkm[4 * c + 2] = k;  ijkm[4 * c + 3] = bad; }
        if (bad) { if (miss) miss[m] = (int)c;  m++; }
    }
    *nmiss = m;
}

/* first bin centre and bin width of an axis whose values span [a, b] */
static void lh_axis(float a, float b, int N, float *I, float *dI)
{
    const float d = (b - a) / (float)N + 0.1f;
    a = a - d;
    b = b + d;
    *dI = lh_clip(1.001f * (b - a) / (float)N, 1.0e-30f, 1.0e30f);
    *I = a + 0.499f * *dI;
}

/* grid[2] = I0, dI0; I1, dI1 [N]; I2, dI2 [N*N]; IND, XX, YY, ZZ [N^3].  Returns 0, or -1 without cells or memory. */
int lh_build(int N, long cells, const float *ABS, long stride, const int *col, float *grid, float *I1, float *dI1, float *I2, float *dI2,
             int *IND, float *XX, float *YY, float *ZZ)
{
    const long bins = (long)N * N * N;
    if (cells < 1) return -1;
    float *R = (float *)malloc(sizeof(float) * 3 * (size_t)cells);
    float *DIS = (float *)malloc(sizeof(float) * (size_t)bins);
    if (!R || !DIS) { free(R);  free(DIS);  return -1; }
    for (long c = 0; c < cells; c++)
        for (int s = 0; s < 3; s++) R[3 * c + s] = LH_LOG10(lh_clip(ABS[c * stride + col[s]], 1.0e-25f, 1.0f));
    float a = R[0], b = R[0];
    for (long c = 1; c < cells; c++) { a = R[3 * c] < a ? R[3 * c] : a;  b = R[3 * c] > b ? R[3 * c] : b; }
    float I0, dI0;
    lh_axis(a, b, N, &I0, &dI0);
    grid[0] = I0;  grid[1] = dI0;
    for (int i = 0; i < N; i++) {
        const float B0 = I0 + (float)i * dI0;
        long n = 0;
        for (long c = 0; c < cells; c++) {
            if (!(fabsf(R[3 * c] - B0) < 0.5f * dI0)) continue;
            const float v = R[3 * c + 1];
            if (!n) a = b = v;
            a = v < a ? v : a;  b = v > b ? v : b;  n++;
        }
        if (n < 1) { I1[i] = 100.0f;  dI1[i] = 0.001f; }
        else lh_axis(a, b, N, &I1[i], &dI1[i]);
        for (int j = 0; j < N; j++) {
            const float B1 = I1[i] + (float)j * dI1[i];
            n = 0;
            for (long c = 0; c < cells; c++) {
                if (!(fabsf(R[3 * c] - B0) < 0.5f * dI0) || !(fabsf(R[3 * c + 1] - B1) < 0.5f * dI1[i])) continue;
                const float v = R[3 * c + 2];
                if (!n) a = b = v;
                a = v < a ? v : a;  b = v > b ? v : b;  n++;
            }
            if (n < 2) { I2[i * N + j] = 100.0f;  dI2[i * N + j] = 0.001f; }
            else lh_axis(a, b, N, &I2[i * N + j], &dI2[i * N + j]);
        }
    }
    a = 100.0f;  b = 0.001f;                                  /* undefined (i, j): the grid of the last defined one in raster order */
    for (int e = 0; e < N * N; e++) {
        if (I2[e] < 99.0f) { a = I2[e];  b = dI2[e]; }
        else { I2[e] = a;  dI2[e] = b; }
    }
    for (long e = 0; e < bins; e++) { IND[e] = 0;  DIS[e] = 1.0e9f;  XX[e] = YY[e] = ZZ[e] = 0.0f; }
    for (long c = 0; c < cells; c++) {                        /* np.round: halves to even (rintf in the default rounding mode) */
        const float x = (R[3 * c] - I0) / dI0;
        const int   i = lh_index(rintf(x), N);
        const float y = (R[3 * c + 1] - I1[i]) / dI1[i];
        const int   j = lh_index(rintf(y), N);
        const float z = (R[3 * c + 2] - I2[i * N + j]) / dI2[i * N + j];
        const int   k = lh_index(rintf(z), N);
        const float dis = (fabsf(x - (float)i) + fabsf(y - (float)j)) + fabsf(z - (float)k);
        const long  e = k + (long)N * (j + N * i);
        if (dis < DIS[e]) { DIS[e] = dis;  IND[e] = (int)c;  XX[e] = x;  YY[e] = y;  ZZ[e] = z; }
    }
    for (long e = 0; e < bins; e++)
        if (DIS[e] > 1.5f) IND[e] = -1;
    free(R);
    free(DIS);
    return 0;
}
