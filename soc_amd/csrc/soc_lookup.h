// soc_lookup.h -- the device arithmetic that the look-up of the library method shares between its kernels: the bin of a cell in a
// library (soc_library_solve_kernel of soc_library.hip and soc_mabu_library_kernel of soc_mabu_library.hip call the one lib_solve_bin)
// and a dust component's share of an absorption (soc_mabu_split_kernel of soc_mabu.hip and soc_mabu_library_kernel: the one mabu_part).
// All fp32 in the order the reference writes it (the build has -ffp-contract=off).
#pragma once
#include "soc_dev.h"
#include "soc_math.h"

// OpenCL round(): halves away from zero (x - trunc(x) is exact)
__device__ __forceinline__ float lib_round_away(float x)
{
    const float t = __builtin_truncf(x);
    return (soc_fabsf(x - t) >= 0.5f) ? t + __builtin_copysignf(1.0f, x) : t;
}

// clamp((int)r, 0, N-1) for an integral float r, without the undefined conversion of a value no int holds (a NaN gives 0)
__device__ __forceinline__ int lib_clip_index(float r, int N)
{
    if (!(r > 0.0f)) return 0;
    if (r >= (float)(N - 1)) return N - 1;
    return (int)r;
}

__device__ __forceinline__ float lib_solve_ref(float a) { return soc_log10f(soc_clampf(a, 1.0e-29f, 1.0e10f)); }

// LibrarySolve, METHOD 0 (kernel_soc_library.c:27-51): the bin of a cell with the absorptions (a0, a1, a2) at the three reference
// frequencies -- three dependent gathers from the small I1 / I2 tables --, or -1 where the library has no answer: the bin's
// representative is more than 1.1 bins away on an axis, or the bin is empty
__device__ __forceinline__ int lib_solve_bin(const SocLibTables &L, float a0, float a1, float a2)
{
    const int N = L.N;
    const float x = (lib_solve_ref(a0) - L.I0) / L.dI0;
    const int   i = lib_clip_index(lib_round_away(x), N);
    const float y = (lib_solve_ref(a1) - L.I1[i]) / L.dI1[i];
    const int   j = lib_clip_index(lib_round_away(y), N);
    const float z = (lib_solve_ref(a2) - L.I2[i * N + j]) / L.dI2[i * N + j];
    const int   k = lib_clip_index(lib_round_away(z), N);
    const int bin = k + N * (j + N * i);
    if (soc_fabsf(x - L.X[bin]) > 1.1f || soc_fabsf(y - L.Y[bin]) > 1.1f || soc_fabsf(z - L.Z[bin]) > 1.1f || L.E0[bin] > 1.0e31f) return -1;
    return bin;
}

// den = sum_j ABU[:, j] * RABS[:, j] (kernel_A2E_MABU_aux.c:3-23): every product in double, den rounded to float after each addition
// (dusts in index order); abu may be strided (a column of LDS)
__device__ __forceinline__ float mabu_den(const float *abu, int abu_stride, const double *R, int NDUST)
{
    float den = 0.0f;
    for (int j = 0; j < NDUST; j++) den = (float)((double)den + (double)abu[j * abu_stride] * R[j]);
    return den;
}

// a * RABS[:, idust] / den: the quotient taken in double and rounded once
__device__ __forceinline__ float mabu_share(float a, double r, float den) { return (float)((double)a * r / (double)den); }

// PART = ABS * RABS[:, idust] / den
__device__ __forceinline__ float mabu_part(float a, const float *abu, const double *R, int NDUST, int idust)
{
    return mabu_share(a, R[idust], mabu_den(abu, 1, R, NDUST));
}
