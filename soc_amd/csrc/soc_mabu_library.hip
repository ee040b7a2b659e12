// soc_mabu_library.hip -- the library method for a model with several dust components: the look-up of every component's emission
// in its own library and the abundance-weighted sum, in one kernel; and the gather of rows of the current dust's emission that
// building such a library needs.
//
// Every dust d has a library (soc_library.hip) indexed by the log of *its share* of the absorptions at the three reference
// frequencies, share_f = ABS3[f] * RABS3[f][d] / sum_j ABU[j] * RABS3[f][j] (mabu_part: the split of soc_mabu.hip).  The host route
// is, per dust, a split of [n][3], a look-up into [n][nout] and SUM += EMI * ABU[:, d]: 2 * NDUST passes over [n][nout].  Here a
// workgroup takes 256 consecutive cells.  Index phase, a lane per cell: the three denominators once, then per dust the share and
// lib_solve_bin (soc_lookup.h, the arithmetic of soc_library_solve_kernel); the bin numbers (-1: no answer) and the abundances of
// the tile go to LDS ([dust][cell]: consecutive lanes consecutive words), bit d of MISS[cell] is set for a dust without answer.
// Row phase: the 256 rows of the tile are 256 * nout consecutive floats of SUM; the lanes walk them flat, so every dust's loads
// from E and the stores are contiguous whatever nout is, and an element is ((0 + E_0 * a_0) + E_1 * a_1) + ... in dust order, each
// product rounded to float before the float addition (the build has -ffp-contract=off), a dust without answer adding 0 * a_d as
// the host's zeroed row does.  SUM is written once: 4 * nout bytes per cell against 12 + 4 * NDUST read, plus the gathers from
// NDUST tables of N^3 * nout floats.
#include "soc_dev.h"
#include "soc_lookup.h"

#define MLIB_T 256

__global__ __launch_bounds__(MLIB_T) void soc_mabu_library_kernel(SocMabuLib A)
{
    extern __shared__ int sMem[];                                      // bins [NDUST][256] | abundances [NDUST][256]
    const int NDUST = A.NDUST, nout = A.nout;
    int   *sBin = sMem;
    float *sAbu = (float *)(sMem + NDUST * MLIB_T);
    const long long tiles = (A.n + MLIB_T - 1) / MLIB_T;
    const int dq = MLIB_T / nout, dr = MLIB_T % nout;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long cell = tile * MLIB_T + threadIdx.x;
        if (cell < A.n) {
            const float *abu = A.ABU + cell * NDUST;
            for (int d = 0; d < NDUST; d++) sAbu[d * MLIB_T + threadIdx.x] = abu[d];
            const float *a = A.ABS3 + cell * 3;
            const float a0 = a[0], a1 = a[1], a2 = a[2];
            const float den0 = mabu_den(sAbu + threadIdx.x, MLIB_T, A.RABS3, NDUST);
            const float den1 = mabu_den(sAbu + threadIdx.x, MLIB_T, A.RABS3 + NDUST, NDUST);
            const float den2 = mabu_den(sAbu + threadIdx.x, MLIB_T, A.RABS3 + 2 * NDUST, NDUST);
            unsigned missed = 0u;
            for (int d = 0; d < NDUST; d++) {
                const int bin = lib_solve_bin(A.LIB[d], mabu_share(a0, A.RABS3[d], den0), mabu_share(a1, A.RABS3[NDUST + d], den1),
                                              mabu_share(a2, A.RABS3[2 * NDUST + d], den2));
                if (bin < 0) missed |= 1u << d;
                sBin[d * MLIB_T + threadIdx.x] = bin;
            }
            A.MISS[cell] = missed;
        }
        __syncthreads();
        const long long left = A.n - tile * MLIB_T;
        const int total = (int)(left < MLIB_T ? left : MLIB_T) * nout;  // <= 256 * 4096
        float *out = A.SUM + tile * MLIB_T * (long long)nout;
        int row = threadIdx.x / nout, col = threadIdx.x % nout;
        for (int e = threadIdx.x; e < total; e += MLIB_T) {
            float sum = 0.0f;
            for (int d = 0; d < NDUST; d++) {
                const int b = sBin[d * MLIB_T + row];
                const float em = b < 0 ? 0.0f : A.LIB[d].E[(size_t)b * nout + col];
                const float p = em * sAbu[d * MLIB_T + row];
                sum = sum + p;
            }
            out[e] = sum;
            row += dq;  col += dr;
            if (col >= nout) { col -= nout;  row++; }
        }
        __syncthreads();
    }
}

// OUT[s][:] = EM[IDX[s]][:]: rows of a resident [cells][NFREQ] array by index (repeats allowed), flat over n * NFREQ elements
__global__ __launch_bounds__(MLIB_T) void soc_mabu_gather_rows_kernel(long long n, int NFREQ, const float *__restrict__ EM,
                                                                      const int *__restrict__ IDX, float *__restrict__ OUT)
{
    const long long N = n * NFREQ;
    for (long long e = blockIdx.x * (long long)MLIB_T + threadIdx.x; e < N; e += (long long)gridDim.x * MLIB_T) {
        const long long s = e / NFREQ;
        const int f = (int)(e - s * NFREQ);
        OUT[e] = EM[(size_t)IDX[s] * NFREQ + f];
    }
}

static int mlib_grid(long long items)
{
    const long long b = (items + MLIB_T - 1) / MLIB_T;
    return (int)(b < 2048 ? (b < 1 ? 1 : b) : 2048);                    // 256 CUs x 8 workgroups; the rest by the stride
}

hipError_t soc_launch_mabu_library(const SocMabuLib &A, hipStream_t st)
{
    if (A.n <= 0) return hipSuccess;
    if (A.NDUST < 1 || A.NDUST > SOC_MABU_LIB_DUSTS || A.nout < 1 || A.nout > 4096) return hipErrorInvalidValue;
    const size_t lds = (size_t)A.NDUST * MLIB_T * 8;                    // <= 64 KB at 32 dusts
    soc_mabu_library_kernel<<<mlib_grid(A.n), MLIB_T, lds, st>>>(A);
    return hipGetLastError();
}

hipError_t soc_launch_mabu_gather_rows(long long n, int NFREQ, const float *EM, const int *IDX, float *OUT, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (NFREQ < 1) return hipErrorInvalidValue;
    soc_mabu_gather_rows_kernel<<<mlib_grid(n * NFREQ), MLIB_T, 0, st>>>(n, NFREQ, EM, IDX, OUT);
    return hipGetLastError();
}
