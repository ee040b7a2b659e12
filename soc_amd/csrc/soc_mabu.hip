// soc_mabu.hip -- the streaming kernels of the multi-dust emission stage (A2E_MABU.py): the split of the absorptions
// between the dust components (kernel_A2E_MABU_aux.c:3-23), the clip of the last channel in front of the stochastic
// solver (A2E.py:184-185), the abundance-weighted sum of the components' emission (A2E_MABU.py:1128-1140), and for `polarisation`
// the polarised emission of an equilibrium dust (A2E_MABU.py:615-637) and the final ratio polarised / total (A2E_MABU.py:1182).
//
// The arrays are [cell][frequency] row-major with NFREQ around 50, so the reference's loop -- one work item per cell
// that walks its frequencies -- reads with a stride of a row between neighbouring lanes.  Here the array is taken flat: a
// tile is 1024 consecutive floats, a lane its four consecutive ones (one 16-byte load and store), consecutive lanes
// consecutive 16 bytes; cell and frequency of an element follow from its flat index.  A grid of at most 2048 workgroups
// strides over the tiles and carries the (cell, frequency) of its tile's first element along, so that the 64-bit
// division happens once per workgroup.  RABS (NFREQ x NDUST doubles) sits in LDS; a cell's abundances come through the
// cache (4 x NDUST bytes per cell from memory).
#include "soc_dev.h"
#include "soc_lookup.h"

#define MABU_T    256
#define MABU_TILE (MABU_T * 4)

// first element of the workgroup's tiles as (cell, frequency), and the step from one tile of the workgroup to its next
struct MabuWalk {
    long long q;           // cell of the tile's first element
    int r, dq, dr;         // its frequency; cells and frequencies the stride adds
    __device__ MabuWalk(long long tile, int NFREQ)
    {
        const long long i0 = tile * MABU_TILE;
        q = i0 / NFREQ;  r = (int)(i0 - q * NFREQ);
        const long long S = (long long)gridDim.x * MABU_TILE;
        dq = (int)(S / NFREQ);  dr = (int)(S - (long long)dq * NFREQ);
    }
    __device__ void next(int NFREQ)
    {
        q += dq;  r += dr;
        if (r >= NFREQ) { r -= NFREQ;  q++; }
    }
};

// (mabu_part, the split of one value: soc_lookup.h, shared with soc_mabu_library_kernel)
__global__ __launch_bounds__(MABU_T) void soc_mabu_split_kernel(long long N, int NFREQ, int NDUST, int idust, const float *__restrict__ ABS,
                                                                const float *__restrict__ ABU, const double *__restrict__ RABS,
                                                                float *__restrict__ PART)
{
    extern __shared__ double sR[];                                     // RABS[NFREQ][NDUST]
    for (int i = threadIdx.x; i < NFREQ * NDUST; i += MABU_T) sR[i] = RABS[i];
    __syncthreads();
    const long long tiles = (N + MABU_TILE - 1) / MABU_TILE;
    MabuWalk W(blockIdx.x, NFREQ);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x, W.next(NFREQ)) {
        const long long i = tile * MABU_TILE + threadIdx.x * 4;
        if (i >= N) continue;
        const unsigned t = (unsigned)W.r + threadIdx.x * 4u;           // < NFREQ + 1024
        long long c = W.q + t / (unsigned)NFREQ;
        int f = (int)(t % (unsigned)NFREQ);
        float v[4];
        const bool whole = i + 3 < N;
        if (whole) { const float4 x = *(const float4 *)(ABS + i);  v[0] = x.x;  v[1] = x.y;  v[2] = x.z;  v[3] = x.w; }
        else for (int k = 0; k < 4; k++) v[k] = i + k < N ? ABS[i + k] : 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i + k < N) v[k] = mabu_part(v[k], ABU + c * NDUST, sR + f * NDUST, NDUST, idust);
            if (++f == NFREQ) { f = 0;  c++; }
        }
        if (whole) *(float4 *)(PART + i) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int k = 0; k < 4; k++) if (i + k < N) PART[i + k] = v[k];
    }
}

// SUM += EM * ABU[:, idust]: the float product rounded, then the float addition (the two roundings of the host's
// EMITTED += em * ABU[:, idust]; the build has -ffp-contract=off, so no fma)
__global__ __launch_bounds__(MABU_T) void soc_mabu_sum_kernel(long long N, int NFREQ, int NDUST, int idust, const float *__restrict__ EM,
                                                              const float *__restrict__ ABU, float *__restrict__ SUM)
{
    const long long tiles = (N + MABU_TILE - 1) / MABU_TILE;
    MabuWalk W(blockIdx.x, NFREQ);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x, W.next(NFREQ)) {
        const long long i = tile * MABU_TILE + threadIdx.x * 4;
        if (i >= N) continue;
        const unsigned t = (unsigned)W.r + threadIdx.x * 4u;
        long long c = W.q + t / (unsigned)NFREQ;
        int f = (int)(t % (unsigned)NFREQ);
        float e[4], s[4];
        const bool whole = i + 3 < N;
        if (whole) {
            const float4 x = *(const float4 *)(EM + i), y = *(const float4 *)(SUM + i);
            e[0] = x.x;  e[1] = x.y;  e[2] = x.z;  e[3] = x.w;  s[0] = y.x;  s[1] = y.y;  s[2] = y.z;  s[3] = y.w;
        } else for (int k = 0; k < 4; k++) { e[k] = i + k < N ? EM[i + k] : 0.0f;  s[k] = i + k < N ? SUM[i + k] : 0.0f; }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i + k < N) { const float p = e[k] * ABU[c * NDUST + idust];  s[k] = s[k] + p; }
            if (++f == NFREQ) { f = 0;  c++; }
        }
        if (whole) *(float4 *)(SUM + i) = make_float4(s[0], s[1], s[2], s[3]);
        else for (int k = 0; k < 4; k++) if (i + k < N) SUM[i + k] = s[k];
    }
}

// Polarised emission of an equilibrium dust (A2E_MABU.py:615-637): PEM = EM * ipR_f(a), a the cell's minimum aligned grain size and
// ipR_f the reduction factor of frequency f over the sizes APOL[NA] (increasing), linear between the nodes TAB[f][NA] and 0 outside
// them -- scipy's interp1d(apol, tmp, bounds_error=False, fill_value=0.0), which for such a table is numpy's interp: the node value
// where a node is hit, else slope = (y1 - y0) / (x1 - x0), y = slope * (a - x0) + y0, every operation in double and on its own (the
// build has -ffp-contract=off).  The product with the float emission is taken in double and rounded once.
__device__ __forceinline__ int mabu_pol_interval(const double *__restrict__ APOL, int NA, double x)
{
    if (!(x >= APOL[0]) || !(x <= APOL[NA - 1])) return -1;             // outside the table (or NaN)
    int lo = 0, hi = NA - 1;                                            // APOL[lo] <= x, and x < APOL[hi] or hi is the last node
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (APOL[m] <= x) lo = m; else hi = m;
    }
    return (APOL[hi] <= x) ? hi : lo;
}

__device__ __forceinline__ double mabu_pol_factor(const double *__restrict__ APOL, const double *__restrict__ Y, int NA, int j, double x)
{
    if (x != x) return x;
    if (j < 0) return 0.0;
    if (j == NA - 1 || APOL[j] == x) return Y[j];
    const double slope = (Y[j + 1] - Y[j]) / (APOL[j + 1] - APOL[j]);
    const double t = slope * (x - APOL[j]);
    return t + Y[j];
}

__global__ __launch_bounds__(MABU_T) void soc_mabu_poleq_kernel(long long N, int NFREQ, int NA, const float *__restrict__ EM,
                                                                const float *__restrict__ AALG, const double *__restrict__ APOL,
                                                                const double *__restrict__ TAB, float *__restrict__ PEM)
{
    const long long tiles = (N + MABU_TILE - 1) / MABU_TILE;
    MabuWalk W(blockIdx.x, NFREQ);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x, W.next(NFREQ)) {
        const long long i = tile * MABU_TILE + threadIdx.x * 4;
        if (i >= N) continue;
        const unsigned t = (unsigned)W.r + threadIdx.x * 4u;
        long long c = W.q + t / (unsigned)NFREQ;
        int f = (int)(t % (unsigned)NFREQ);
        float e[4];
        const bool whole = i + 3 < N;
        if (whole) { const float4 x = *(const float4 *)(EM + i);  e[0] = x.x;  e[1] = x.y;  e[2] = x.z;  e[3] = x.w; }
        else for (int k = 0; k < 4; k++) e[k] = i + k < N ? EM[i + k] : 0.0f;
        double a = (double)AALG[2 * c];
        int j = mabu_pol_interval(APOL, NA, a);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i + k < N) e[k] = (float)((double)e[k] * mabu_pol_factor(APOL, TAB + (size_t)f * NA, NA, j, a));
            if (++f == NFREQ) {
                f = 0;  c++;
                if (i + k + 1 < N) { a = (double)AALG[2 * c];  j = mabu_pol_interval(APOL, NA, a); }
            }
        }
        if (whole) *(float4 *)(PEM + i) = make_float4(e[0], e[1], e[2], e[3]);
        else for (int k = 0; k < 4; k++) if (i + k < N) PEM[i + k] = e[k];
    }
}

// R = PSUM / (SUM + 1e-32) in float (A2E_MABU.py:1182): polarised intensity -> polarisation reduction factor, in place
__global__ __launch_bounds__(MABU_T) void soc_mabu_ratio_kernel(long long N, const float *__restrict__ SUM, float *__restrict__ PSUM)
{
    const long long tiles = (N + MABU_TILE - 1) / MABU_TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long i = tile * MABU_TILE + threadIdx.x * 4;
        if (i >= N) continue;
        if (i + 3 < N) {
            const float4 s = *(const float4 *)(SUM + i), p = *(const float4 *)(PSUM + i);
            *(float4 *)(PSUM + i) = make_float4(p.x / (s.x + 1.0e-32f), p.y / (s.y + 1.0e-32f), p.z / (s.z + 1.0e-32f), p.w / (s.w + 1.0e-32f));
        } else for (int k = 0; k < 4; k++) if (i + k < N) PSUM[i + k] = PSUM[i + k] / (SUM[i + k] + 1.0e-32f);
    }
}

// A2E.py:184-185 on the device: PART[:, NFREQ-1] = clip(PART[:, NFREQ-1], 0, 0.2 * PART[:, NFREQ-2]) with numpy's clip --
// min(max(x, lo), hi), a NaN in x kept, a NaN in hi taken.  One lane per cell: two neighbouring words of its row.
__global__ void soc_mabu_clip_kernel(long long cells, int NFREQ, float *PART)
{
    for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
        float *row = PART + c * NFREQ;
        const float x = row[NFREQ - 1], hi = 0.2f * row[NFREQ - 2];
        const float t = (x != x) ? x : (x > 0.0f ? x : 0.0f);
        row[NFREQ - 1] = (t != t) ? t : (t < hi ? t : hi);
    }
}

static int mabu_grid(long long N)
{
    const long long tiles = (N + MABU_TILE - 1) / MABU_TILE;
    return (int)(tiles < 2048 ? tiles : 2048);                          // 256 CUs x 8 workgroups; the rest by the stride
}

hipError_t soc_launch_mabu_split(long long cells, int NFREQ, int NDUST, int idust, const float *ABS, const float *ABU, const double *RABS,
                                 float *PART, hipStream_t st)
{
    if (cells <= 0) return hipSuccess;
    const size_t lds = (size_t)NFREQ * NDUST * sizeof(double);
    if (NFREQ < 1 || NDUST < 1 || idust < 0 || idust >= NDUST || lds > SOC_MABU_LDS) return hipErrorInvalidValue;
    const long long N = cells * NFREQ;
    soc_mabu_split_kernel<<<mabu_grid(N), MABU_T, lds, st>>>(N, NFREQ, NDUST, idust, ABS, ABU, RABS, PART);
    return hipGetLastError();
}

hipError_t soc_launch_mabu_sum(long long cells, int NFREQ, int NDUST, int idust, const float *EM, const float *ABU, float *SUM, hipStream_t st)
{
    if (cells <= 0) return hipSuccess;
    if (NFREQ < 1 || NDUST < 1 || idust < 0 || idust >= NDUST) return hipErrorInvalidValue;
    const long long N = cells * NFREQ;
    soc_mabu_sum_kernel<<<mabu_grid(N), MABU_T, 0, st>>>(N, NFREQ, NDUST, idust, EM, ABU, SUM);
    return hipGetLastError();
}

hipError_t soc_launch_mabu_clip(long long cells, int NFREQ, float *PART, hipStream_t st)
{
    if (cells <= 0) return hipSuccess;
    if (NFREQ < 2) return hipErrorInvalidValue;
    const long long blocks = (cells + 255) / 256;
    soc_mabu_clip_kernel<<<(int)(blocks < 16384 ? blocks : 16384), 256, 0, st>>>(cells, NFREQ, PART);
    return hipGetLastError();
}

hipError_t soc_launch_mabu_poleq(long long cells, int NFREQ, int NA, const float *EM, const float *AALG, const double *APOL, const double *TAB,
                                 float *PEM, hipStream_t st)
{
    if (cells <= 0) return hipSuccess;
    if (NFREQ < 1 || NA < 2) return hipErrorInvalidValue;
    const long long N = cells * NFREQ;
    soc_mabu_poleq_kernel<<<mabu_grid(N), MABU_T, 0, st>>>(N, NFREQ, NA, EM, AALG, APOL, TAB, PEM);
    return hipGetLastError();
}

hipError_t soc_launch_mabu_ratio(long long cells, int NFREQ, const float *SUM, float *PSUM, hipStream_t st)
{
    if (cells <= 0) return hipSuccess;
    if (NFREQ < 1) return hipErrorInvalidValue;
    const long long N = cells * NFREQ;
    soc_mabu_ratio_kernel<<<mabu_grid(N), MABU_T, 0, st>>>(N, SUM, PSUM);
    return hipGetLastError();
}
