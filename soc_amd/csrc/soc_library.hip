// soc_library.hip -- the library method for dust emission (soc_library.py with kernel_soc_library.c): the look-up of a cell's
// emission in an N x N x N table indexed by the log-absorptions at three reference frequencies, and the construction of that
// table's grid and of its representative cells from the absorptions of a full run.
//
// All arithmetic is fp32 in the order the reference writes it, with soc_log10f and the correctly rounded divide (the build has
// -ffp-contract=off), so every value equals the plain-C restatement of tests/csrc/library_host.c compiled from the same
// soc_math.h.  Three reference columns of a row-major [cell][column] array are read through (stride, c0, c1, c2): a packed
// [n][3] array, or the arrays of soc_a2e_resident_*.
//
// Look-up (LibrarySolve, METHOD 0, kernel_soc_library.c:27-51): a workgroup takes 256 consecutive cells.  Index phase: a lane
// per cell computes (x, i), (y, j), (z, k) -- three dependent gathers from the small I1/I2 tables -- and the miss test, and
// leaves the bin number (or -1) in LDS.  Row copy: the 256 rows of the tile are 256 * nout consecutive floats of EMI; the lanes
// walk them flat, so a row's loads from E and the stores to EMI are contiguous whatever nout is.  The table (N = 30 at 50
// frequencies: 5.4 MB) stays in L2; the kernel's cost is the n * nout * 4 bytes it writes.
//
// Build (soc_library.py:127-217): sweeps over the cells with the N- and N^2-entry min / max / count tables private to a
// workgroup in LDS -- floats compared as ordered integers -- flushed with vector atomics, and the representative cell of a bin
// by one 64-bit atomicMin on (bits of the distance << 32 | cell): least distance, then lowest cell, whatever the order.
#include "soc_dev.h"
#include "soc_lookup.h"
#include "soc_math.h"

#define LIB_T 256

__device__ __forceinline__ float lib_build_ref(float a) { return soc_log10f(soc_clampf(a, 1.0e-25f, 1.0f)); }

__global__ __launch_bounds__(LIB_T) void soc_library_solve_kernel(SocLibSolve A)
{
    __shared__ int sBin[LIB_T];
    const int nout = A.nout;
    const SocLibTables L = { A.N, A.nout, A.I0, A.dI0, A.I1, A.dI1, A.I2, A.dI2, A.X, A.Y, A.Z, A.E0, A.E };
    const long long tiles = (A.n + LIB_T - 1) / LIB_T;
    const int dq = LIB_T / nout, dr = LIB_T % nout;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long cell = tile * LIB_T + threadIdx.x;
        int bin = -1;
        if (cell < A.n) {
            const float *a = A.ABS + cell * A.stride;
            bin = lib_solve_bin(L, a[A.c0], a[A.c1], a[A.c2]);       // (soc_lookup.h: shared with soc_mabu_library_kernel)
            if (bin < 0) A.miss[atomicAdd(A.nmiss, 1ull)] = (int)cell;   // (at most one entry per cell: below n)
        }
        sBin[threadIdx.x] = bin;
        __syncthreads();
        const long long left = A.n - tile * LIB_T;
        const int total = (int)(left < LIB_T ? left : LIB_T) * nout;    // <= 256 * 4096
        float *out = A.EMI + tile * LIB_T * (long long)nout;
        int row = threadIdx.x / nout, col = threadIdx.x % nout;
        for (int e = threadIdx.x; e < total; e += LIB_T) {
            const int b = sBin[row];
            out[e] = b < 0 ? (col == 0 ? 1.0e32f : 0.0f) : A.E[(size_t)b * nout + col];
            row += dq;  col += dr;
            if (col >= nout) { col -= nout;  row++; }
        }
        __syncthreads();
    }
}

// ---- build ----

// floats as unsigned integers of the same order
__device__ __forceinline__ unsigned lib_okey(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void lib_tab_add(unsigned *s, int entries, int e, float v)
{
    const unsigned key = lib_okey(v);
    atomicMin(&s[e], key);
    atomicMax(&s[entries + e], key);
    atomicAdd(&s[2 * entries + e], 1u);
}

// level 0: min / max of axis 0 over all cells; level 1: per i, of axis 1 over the cells of window i; level 2: per (i, j), of
// axis 2 over the cells of both windows.  TAB: entries minima | entries maxima | entries counts (ordered keys; 0xffffffff, 0, 0
// before the launch).  The windows are the reference's float expressions |IREF - (I + i * dI)| < 0.5 * dI; a window's candidates
// are rint of the cell's coordinate and its two neighbours, and a cell may lie in none or in more than one.
__global__ __launch_bounds__(LIB_T) void soc_library_range_kernel(SocLibBuild A, int level, unsigned *TAB)
{
    extern __shared__ unsigned sTab[];
    const int N = A.N, entries = level == 0 ? 1 : (level == 1 ? N : N * N);
    for (int e = threadIdx.x; e < entries; e += LIB_T) { sTab[e] = 0xffffffffu;  sTab[entries + e] = 0u;  sTab[2 * entries + e] = 0u; }
    __syncthreads();
    unsigned lo = 0xffffffffu, hi = 0u, cnt = 0u;               // level 0: in registers
    for (long long cell = blockIdx.x * (long long)LIB_T + threadIdx.x; cell < A.cells; cell += (long long)gridDim.x * LIB_T) {
        const float *a = A.ABS + cell * A.stride;
        const float r0 = lib_build_ref(a[A.c0]);
        if (level == 0) {
            const unsigned key = lib_okey(r0);
            lo = key < lo ? key : lo;  hi = key > hi ? key : hi;  cnt++;
            continue;
        }
        const float x = (r0 - A.I0) / A.dI0;
        if (!(soc_fabsf(x) < 1.0e9f)) continue;
        const int ic = (int)__builtin_rintf(x);
        for (int i = ic - 1; i <= ic + 1; i++) {
            if (i < 0 || i >= N || !(soc_fabsf(r0 - (A.I0 + (float)i * A.dI0)) < 0.5f * A.dI0)) continue;
            const float r1 = lib_build_ref(a[A.c1]);
            if (level == 1) { lib_tab_add(sTab, entries, i, r1);  continue; }
            const float i1 = A.I1[i], d1 = A.dI1[i];
            const float y = (r1 - i1) / d1;
            if (!(soc_fabsf(y) < 1.0e9f)) continue;
            const int jc = (int)__builtin_rintf(y);
            for (int j = jc - 1; j <= jc + 1; j++) {
                if (j < 0 || j >= N || !(soc_fabsf(r1 - (i1 + (float)j * d1)) < 0.5f * d1)) continue;
                lib_tab_add(sTab, entries, i * N + j, lib_build_ref(a[A.c2]));
            }
        }
    }
    if (level == 0 && cnt) { atomicMin(&sTab[0], lo);  atomicMax(&sTab[1], hi);  atomicAdd(&sTab[2], cnt); }
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += LIB_T) {
        const unsigned n = sTab[2 * entries + e];
        if (!n) continue;
        atomicMin(&TAB[e], sTab[e]);
        atomicMax(&TAB[entries + e], sTab[entries + e]);
        atomicAdd(&TAB[2 * entries + e], n);
    }
}

// a cell's coordinates on the finished grid and its bin: np.round (halves to even), the indices clipped before they are used
__device__ __forceinline__ int lib_build_bin(const SocLibBuild &A, long long cell, float &x, float &y, float &z, float &dis)
{
    const int N = A.N;
    const float *a = A.ABS + cell * A.stride;
    x = (lib_build_ref(a[A.c0]) - A.I0) / A.dI0;
    const int i = lib_clip_index(__builtin_rintf(x), N);
    y = (lib_build_ref(a[A.c1]) - A.I1[i]) / A.dI1[i];
    const int j = lib_clip_index(__builtin_rintf(y), N);
    z = (lib_build_ref(a[A.c2]) - A.I2[i * N + j]) / A.dI2[i * N + j];
    const int k = lib_clip_index(__builtin_rintf(z), N);
    dis = (soc_fabsf(x - (float)i) + soc_fabsf(y - (float)j)) + soc_fabsf(z - (float)k);
    return k + N * (j + N * i);
}

// BEST[N^3] (all ones before the launch): the least (distance, cell) of every bin
__global__ __launch_bounds__(LIB_T) void soc_library_pick_kernel(SocLibBuild A, unsigned long long *BEST)
{
    for (long long cell = blockIdx.x * (long long)LIB_T + threadIdx.x; cell < A.cells; cell += (long long)gridDim.x * LIB_T) {
        float x, y, z, dis;
        const int bin = lib_build_bin(A, cell, x, y, z, dis);
        const unsigned long long key = ((unsigned long long)__float_as_uint(dis) << 32) | (unsigned long long)cell;   // dis >= 0: its bits order it
        if (key < __atomic_load_n(&BEST[bin], __ATOMIC_RELAXED)) atomicMin(&BEST[bin], key);    // (BEST only falls: a larger key never wins)
    }
}

// per bin: the winner's coordinates, and its cell unless its distance exceeds 1.5 (soc_library.py:206-217; DIS starts at 1e9)
__global__ void soc_library_bins_kernel(SocLibBuild A, const unsigned long long *BEST, int *IND, float *XX, float *YY, float *ZZ)
{
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= A.N * A.N * A.N) return;
    const unsigned long long key = BEST[bin];
    float x = 0.0f, y = 0.0f, z = 0.0f, dis;
    int ind = 0;                                                 // (a bin no cell reached keeps the zeros of the reference's arrays; DIS = 1e9 makes it -1)
    bool won = false;
    if (key != ~0ull && __uint_as_float((unsigned)(key >> 32)) < 1.0e9f) {
        ind = (int)(key & 0xffffffffull);
        (void)lib_build_bin(A, ind, x, y, z, dis);
        won = dis <= 1.5f;
    }
    IND[bin] = won ? ind : -1;
    XX[bin] = x;  YY[bin] = y;  ZZ[bin] = z;
}

static int lib_grid(long long items)
{
    const long long b = (items + LIB_T - 1) / LIB_T;
    return (int)(b < 2048 ? (b < 1 ? 1 : b) : 2048);                    // 256 CUs x 8 workgroups; the rest by the stride
}

hipError_t soc_launch_library_solve(const SocLibSolve &A, hipStream_t st)
{
    if (A.n <= 0) return hipSuccess;
    if (A.N < 2 || A.N > 64 || A.nout < 1 || A.nout > 4096) return hipErrorInvalidValue;
    soc_library_solve_kernel<<<lib_grid(A.n), LIB_T, 0, st>>>(A);
    return hipGetLastError();
}

hipError_t soc_launch_library_range(const SocLibBuild &A, int level, unsigned *TAB, hipStream_t st)
{
    if (A.cells <= 0) return hipSuccess;
    if (A.N < 2 || A.N > 64 || level < 0 || level > 2) return hipErrorInvalidValue;
    const int entries = level == 0 ? 1 : (level == 1 ? A.N : A.N * A.N);
    soc_library_range_kernel<<<lib_grid(A.cells), LIB_T, (size_t)entries * 12, st>>>(A, level, TAB);   // <= 48 KB
    return hipGetLastError();
}

hipError_t soc_launch_library_pick(const SocLibBuild &A, unsigned long long *BEST, int *IND, float *XX, float *YY, float *ZZ, hipStream_t st)
{
    if (A.cells <= 0 || A.N < 2 || A.N > 64) return hipErrorInvalidValue;
    soc_library_pick_kernel<<<lib_grid(A.cells), LIB_T, 0, st>>>(A, BEST);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int bins = A.N * A.N * A.N;
    soc_library_bins_kernel<<<(bins + LIB_T - 1) / LIB_T, LIB_T, 0, st>>>(A, BEST, IND, XX, YY, ZZ);
    return hipGetLastError();
}
