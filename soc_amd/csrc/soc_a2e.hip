// soc_a2e.hip -- stochastically heated grains: DoSolve and EqTemperature of kernel_A2E.c for gfx950.
//
// Reference shape (kernel_A2E.c:2-104): one work item per cell, the lower-triangular
// transition matrix L[(NE^2-NE)/2] of every cell spilled to a global scratch buffer
// interleaved by LOCAL (NE=128 -> 266 MB per batch of 8192 cells; the source comments put
// most of the run time into building and re-reading it), a private XL[NE].
//
// Here: a workgroup of sixteen waves solves C cells (C = 4, 2 or 1: the largest with C*per_cell + 4*NFREQ <= 160 KB of LDS,
// per_cell = 4*((NE^2-NE)/2 + NE + NFREQ) -- soc_a2e_shape; at NFREQ = 50 that is 4 up to NE = 142, 2 up to 201, 1 up to 280); L lives in LDS
// (32.5 KB per cell at NE=128) and never touches HBM:
//   1. heating rates, by ALL lanes of the workgroup for ALL its cells: the (l,u) pairs are spread over the 1024 lanes; a lane
//      reads a pair's integration weights once and adds them up for its C cells (the weights are the same for every cell:
//      read per cell -- as the first form of this kernel did, one wave per cell -- the 650 KB table of NE=128 came from L2
//      8192 times per batch).  Each entry is the reference's sequential sum over its frequency window (host-built pair
//      tables give the window, the weight offset and the slot in L), clamped at 0;
//   then wave w < C goes on with cell w alone (the other waves wait at the barriers):
//   2. suffix sums over u: a lane owns columns, the running sum in a register, rows walked downwards as in the reference;
//   3. forward substitution, row per lane: a lane adds up its row in the reference's order (i ascending, multiply then
//      add), finished values go down the rows with v_readlane -- no barrier, no tree reduction: the reference's bits;
//   4. normalisation and emission: one frequency per lane, serial over the enthalpy bins from Ibeg[f] exactly as the reference.
// Algorithmic HBM bytes per cell and size: 4*NFREQ in + 4*NFREQ out (tables are L2-resident).
//
// EqTemperature (kernel_A2E.c:110-154) is one lane per cell, operation for operation (soc_a2e_eqtemp_kernel: a batch of host arrays),
// and, for the cells resident in HBM, one sweep over all equilibrium sizes of a dust with the same operations (soc_a2e_eqsizes_kernel).
#include "soc_dev.h"
#include "soc_math.h"

#define A2E_IND(a, b) (((a) * (a) - (a)) / 2 + (b))

// cycles per phase of DoSolve for experiments (-DSOC_A2E_PROF; tools/exp_a2e.py prints them): wave 0 of every workgroup
#if defined(SOC_A2E_PROF)
__device__ unsigned long long g_a2e_prof[8];
#define A2E_PROF_DECL unsigned long long pt_ = __builtin_readcyclecounter()
#define A2E_PROF(i) do { const unsigned long long t_ = __builtin_readcyclecounter();  if (threadIdx.x == 0) atomicAdd(&g_a2e_prof[i], t_ - pt_);  pt_ = t_; } while (0)
extern "C" __attribute__((visibility("default"))) void soc_a2e_prof_read(unsigned long long *out, int reset)
{
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_a2e_prof), sizeof(unsigned long long) * 8);
    if (reset) { unsigned long long z[8] = { 0 };  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_a2e_prof), z, sizeof(z)); }
}
#else
#define A2E_PROF_DECL
#define A2E_PROF(i) do { } while (0)
#endif
// s = sum_{i<n} Lr[i] * X[i], i ascending, multiply then add -- the order of the reference's serial loop (kernel_A2E.c:82) -- with the
// LDS reads of eight terms in flight before the first addition needs one
__device__ __forceinline__ float a2e_row_sum(const float *Lr, const float *X, const int n)
{
    float s = 0.0f;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float l[8], x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { l[u] = Lr[i + u];  x[u] = X[i + u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) s += l[u] * x[u];
    }
    for (; i < n; i++) s += Lr[i] * X[i];
    return s;
}

#define A2E_T 1024                   // threads per workgroup: sixteen waves build the matrices (their LDS leaves room for one workgroup
                                     // per CU, so the waves that hide the latency of the weight reads must be its own); four of them solve
#define A2E_Q 2                      // pairs a lane has in flight in step 1

// POL: the emission is also added, weighted, to a second row PEMIT -- the polarised emission of the grains larger than the cell's
// minimum aligned size a (A2E.py:413-429).  The weight of this size (A.p_size = ASIZE[isize], A.p_next = ASIZE[isize+1], or 0 for the
// last size, which has no partial arm):  1 where p_size >= a;  (log10(a) - log10(p_size)) / (log10(p_next) - log10(p_size)) where
// p_size < a < p_next;  else 0, and the row is not touched.  AALG holds a and log10(a) per cell (the logarithm is numpy's, taken on the
// host); the subtraction, the division, the product w * I and the sum are single fp32 operations (the build has -ffp-contract=off), so
// the bits are those of numpy's float32 expressions.  Without POL the kernel is the one it was: the three plain instances keep their
// instructions.
// DUMP: the normalised populations of the enthalpy levels also go out, clamped as the reference's dump is (kernel_A2E.c:14-16, 101-103:
// XX[id * NE + i] = clamp(XL[i], 1e-35f, 10.0f), written as fmin(fmax()) so that a NaN gives the lower bound), the row of a cell by the
// wave that has solved it, the lanes on neighbouring words.  XL is read, not written, so the emission is the one it was; built as POL
// was: the instances without DUMP keep their instructions.
template <int C, bool POL, bool DUMP>
__global__ __launch_bounds__(A2E_T) void soc_a2e_dosolve_kernel(const SocA2EArgs A)
{
    extern __shared__ float lds[];
    const int T = (int)blockDim.x;                       // 1024, or 256 where the matrices are small (several workgroups per CU)
    const int NE = A.NE, NFREQ = A.NFREQ, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int LSZ = (NE * NE - NE) / 2;
    float *Lall = lds;                                   // [C][(NE*NE-NE)/2]
    float *XLall = Lall + C * LSZ;                       // [C][NE]
    float *sABS = XLall + C * NE;                        // [C][NFREQ]
    float *sAF  = sABS + C * NFREQ;                      // [NFREQ]
    const int cell0 = blockIdx.x * C;
    const int nc = (A.batch - cell0 < C) ? (A.batch - cell0) : C;          // cells of this workgroup (>= 1)
    for (int i = tid; i < C * NFREQ; i += T) {
        const int c = i / NFREQ;
        sABS[i] = (c < nc) ? A.AABS[(size_t)(cell0 + c) * NFREQ + (i - c * NFREQ)] : 0.0f;
    }
    for (int i = tid; i < NFREQ; i += T) sAF[i] = A.AF[i];
    __syncthreads();
    A2E_PROF_DECL;

    // 1. heating: L[u,l] = max(sum_i ABS[i]*Iw*AF[i], 0)   (kernel_A2E.c:45-54); every sum runs over its own window in the
    //    reference's order, the C cells side by side
    for (int e0 = tid; e0 < A.npair; e0 += T * A2E_Q) {
        int   i0[A2E_Q], n[A2E_Q], dst[A2E_Q];
        const float *w[A2E_Q];
        float I[A2E_Q][C];
        int   nmax = 0;
#pragma unroll
        for (int q = 0; q < A2E_Q; q++) {
            const int e = e0 + T * q;
            const bool on = e < A.npair;
            i0[q]  = on ? A.pair_first[e] : 0;
            n[q]   = on ? (A.pair_last[e] - i0[q] + 1) : 0;
            w[q]   = A.Iw + (on ? A.pair_iw[e] : 0);
            dst[q] = on ? A.pair_dst[e] : -1;
#pragma unroll
            for (int c = 0; c < C; c++) I[q][c] = 0.0f;
            nmax   = n[q] > nmax ? n[q] : nmax;
        }
        for (int t = 0; t < nmax; t++) {
#pragma unroll
            for (int q = 0; q < A2E_Q; q++)
                if (t < n[q]) {
                    const float wt = w[q][t], af = sAF[i0[q] + t];
#pragma unroll
                    for (int c = 0; c < C; c++) I[q][c] += sABS[c * NFREQ + i0[q] + t] * wt * af;
                }
        }
        (void)nmax;
#pragma unroll
        for (int q = 0; q < A2E_Q; q++)
            if (dst[q] >= 0) {
#pragma unroll
                for (int c = 0; c < C; c++) Lall[c * LSZ + dst[q]] = __builtin_fmaxf(I[q][c], 0.0f);
            }
    }
    __syncthreads();
    A2E_PROF(0);                                         // heating rates
    // wave wv goes on with cell wv (a wave without a cell walks along idle: the barriers below are the workgroup's)
    const bool mine = (wv < nc);
    float *L = Lall + (mine ? wv : 0) * LSZ, *XL = XLall + (mine ? wv : 0) * NE;
    // 2. suffix sums over the upper level (kernel_A2E.c:72-77): L[j,i] += L[j+1,i] for j = NE-3 .. 1.  A lane owns the columns
    //    lane, lane + 64, ...; the running sum of a column stays in a register (the reference reads back what it has just
    //    written: the same additions), so the reads of a column do not wait for its writes
    if (mine) {
        for (int i = lane; i < NE - 3; i += 64) {
            float acc = L[A2E_IND(NE - 2, i)];
            int j = NE - 3;
            for (; j - 3 > i; j -= 4) {                                   // four rows of the column read together
                const float a0 = L[A2E_IND(j, i)], a1 = L[A2E_IND(j - 1, i)], a2 = L[A2E_IND(j - 2, i)], a3 = L[A2E_IND(j - 3, i)];
                acc = a0 + acc;  L[A2E_IND(j, i)] = acc;
                acc = a1 + acc;  L[A2E_IND(j - 1, i)] = acc;
                acc = a2 + acc;  L[A2E_IND(j - 2, i)] = acc;
                acc = a3 + acc;  L[A2E_IND(j - 3, i)] = acc;
            }
            for (; j > i; j--) {
                acc = L[A2E_IND(j, i)] + acc;
                L[A2E_IND(j, i)] = acc;
            }
        }
    }
    __syncthreads();
    A2E_PROF(1);                                         // suffix sums
    // 3. forward substitution (kernel_A2E.c:80-88), row per lane: lane r of a block of 64 rows keeps the sum of its row
    //    XL[j] = sum_{i<j} L[j,i] * XL[i], added up in the reference's order (i ascending, mul then add); the rows of a
    //    block are finished one after the other, the finished XL[j] handed to the rows below by v_readlane.  No barrier,
    //    no tree reduction: the same fp32 operations as the serial loop, so the same bits.
    //    Inside a block nothing goes through LDS: a finished value stays in its lane's register (written to XL once, after the
    //    block), and the matrix element of the next row to finish is read before the division of this one is waited for.
    if (mine) {
        for (int j0 = 0; j0 < NE; j0 += 64) {
            const int row = j0 + lane;
            const bool live = (row < NE);
            float s = 0.0f;
            if (live) s = a2e_row_sum(L + A2E_IND(row, 0), XL, j0);                       // the blocks above: all XL[i] final
            const int kend = __builtin_amdgcn_readfirstlane((NE - j0 < 64) ? (NE - j0) : 64);
            const float td = live ? (A.Tdown[row] + 1.0e-30f) : 1.0f;                     // lane k finishes row j0 + k
            const float *Lrow = L + (live ? A2E_IND(row, j0) : 0);                        // L[row, j0 + k], k < lane
            float xmine = 0.0f;                                                           // XL[row], once lane `lane` has finished
            float lnext = (live && lane > 0) ? Lrow[0] : 0.0f;
            for (int k = 0; k < kend; k++) {
                const int jk = j0 + k;
                const float lcur = lnext;
                lnext = (live && lane > k + 1) ? Lrow[k + 1] : 0.0f;                      // (asked for now, used in the next turn)
#if defined(A2E_X_MUL)
                float x = s * td;                                                         // timing experiment only (wrong numbers)
#else
                float x = s / td;
#endif
                x = __builtin_fmaxf(x, 0.0f);
                if (jk == 0) x = 1.0e-20f;                                                // XL[0]
                float xk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), k));
                if (xk > 1.0e20f) {
                    // rescaling (kernel_A2E.c:86-88): XL[0..jk] *= 1e-20, and every later row is summed from those values --
                    // the sums in hand were taken with the old ones, so they are taken again (rare).  The values of this block
                    // that are finished go to LDS first, scaled, so that the sums can be taken from there
                    for (int i = lane; i < j0; i += 64) XL[i] *= 1.0e-20f;
                    xk *= 1.0e-20f;
                    if (lane < k) { xmine *= 1.0e-20f;  XL[row] = xmine; }
                    if (lane == k) { xmine = xk;  XL[jk] = xk; }
                    s = 0.0f;
                    if (live && row > jk) s = a2e_row_sum(L + A2E_IND(row, 0), XL, jk + 1);
                    lnext = (live && lane > k + 1) ? Lrow[k + 1] : 0.0f;
                } else {
                    if (lane == k) xmine = xk;
                    if (live && row > jk) s += lcur * xk;
                }
            }
            if (live) XL[row] = xmine;
        }
    }
    __syncthreads();
    A2E_PROF(2);                                         // forward substitution
    // normalise (kernel_A2E.c:90-92): the sum in the reference's order, every lane for itself (broadcast reads)
    float nrm = 0.0f;
    for (int i = 0; i < NE; i++) nrm += XL[i];
    nrm = 1.0f / nrm;
    __syncthreads();
    if (mine) for (int i = lane; i < NE; i += 64) XL[i] = XL[i] * nrm;
    __syncthreads();
    A2E_PROF(3);                                         // normalisation
    // 4. emission (kernel_A2E.c:95-100): one frequency per lane, serial over the bins
    if (mine) {
        if constexpr (DUMP) {
            float *XX = A.XX + (size_t)(cell0 + wv) * NE;
            for (int i = lane; i < NE; i += 64) XX[i] = __builtin_fminf(__builtin_fmaxf(XL[i], 1.0e-35f), 10.0f);
        }
        float *EMIT = A.AEMIT + (size_t)(cell0 + wv) * NFREQ;
        int   arm = 0;                                        // 0: this size is not aligned in the cell, 1: wholly, 2: in part (weight pw)
        float pw = 0.0f;
        if constexpr (POL) {
            const float a = A.AALG[2 * (size_t)(cell0 + wv)], lga = A.AALG[2 * (size_t)(cell0 + wv) + 1];
            if (A.p_size >= a) arm = 1;
            else if (A.p_size < a && A.p_next > a) { arm = 2;  pw = (lga - A.p_lgsize) / A.p_lgden; }
        }
        for (int f = lane; f < NFREQ; f += 64) {
            float I = 0.0f;
            const float *ea = A.EA + f;                       // EA transposed: [bin][frequency]
            const int ib = A.Ibeg[f];
#pragma unroll 8
            for (int i = ib; i < NE; i++) I += ea[(size_t)i * NFREQ] * XL[i];
            EMIT[f] = A.accumulate ? (EMIT[f] + I) : I;       // (the host's EMITTED += emit of A2E.py:596-600, size after size: the same fp32 additions)
            if constexpr (POL) {
                float *P = A.PEMIT + (size_t)(cell0 + wv) * NFREQ + f;
                if (arm == 1) *P = *P + I;                    // PEMITTED[m] += emit[m]          (A2E.py:417-421)
                else if (arm == 2) { const float wI = pw * I;  *P = *P + wI; }     // PEMITTED[m] += w * emit[m]   (A2E.py:424-429)
            }
        }
    }
    A2E_PROF(4);                                         // emission
}

// EqTemperature (kernel_A2E.c:110-154): trapezoid E_in, log-table lookup of T, Planck emission
__global__ void soc_a2e_eqtemp_kernel(const SocEqTArgs A)
{
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= A.batch) return;
    if (A.icell + id >= A.CELLS) return;
    const float *a = A.ABS + (size_t)id * A.NFREQ;
    float Ein = 0.0f;
    for (int i = 1; i < A.NFREQ; i++)
        Ein += (a[i] * A.FREQ[i] + a[i - 1] * A.FREQ[i - 1]) * ((A.FREQ[i] - A.FREQ[i - 1]) * 3.3130348e-27f);
    int iE = (int)soc_floorf(A.oplgkE * soc_log10f(Ein / A.Emin));
    iE = iE < 0 ? 0 : (iE > A.NIP - 2 ? A.NIP - 2 : iE);
    const float wi = (A.Emin * soc_pownf(A.kE, iE + 1) - Ein) / (A.Emin * soc_pownf(A.kE, iE + 1) - soc_pownf(A.kE, iE));
    const float TP = (float)((double)(wi * A.TTT[iE]) + (1.0 - (double)wi) * (double)A.TTT[iE + 1]);
    A.T[id] = TP;
    for (int f = 0; f < A.NFREQ; f++) {
        const float fr = A.FREQ[f];
        A.EMIT[(size_t)id * A.NFREQ + f] =
            (2.79639459e-20f * A.FACTOR) * A.KABS[f] * (fr * fr / (soc_expf(4.7995074e-11f * fr / TP) - 1.0f));
    }
}

// EqTemperature for ALL equilibrium sizes of a dust in one sweep over the resident cells (soc_a2e_resident_solve_eq): what
// soc_a2e_eqtemp_kernel and the host statements around it (soc_amd/a2e.py: ABSORBED * AF, EMITTED += emit * (GD * S_FRAC), the hard
// mask of the polarised sum) do per size, operation for operation and in the same order, with 12*NFREQ bytes of HBM traffic per cell
// (absorptions in, the sum in and out; 20*NFREQ + 8 with the polarised sum) however many sizes there are.  A workgroup takes a tile of
// TC cells:
//   stage  the tile's absorptions go to LDS, read as the array lies (lanes on neighbouring words); the rows get an odd stride, so that
//          the 64 lanes of phase A, each on a row of its own, hit 64 banks;
//   A      a lane per (cell, size): x_i = a[i] * AF[size][i] (the host's single fp32 product), Ein summed over i = 1..NFREQ-1 in the
//          order of soc_a2e_eqtemp_kernel, the table look-up, wi, TP -> sT[size][cell];
//   B      a lane per (cell, frequency) element of the tile in the order of the arrays: the sum's element into a register, the
//          emission of every size added in ascending order (emit * scale[size], scale = GD * S_FRAC formed in fp32 by the host), one
//          write; with POL the same for the polarised sum with (emit * GD) * S_FRAC where SIZE_A[size] >= a_alg of the cell.
// The per-size tables AF, KABS [nsizes][NFREQ], TTT [nsizes][NIP] and scalars come from device memory (L2; the lanes of a wave read
// neighbouring words or one word).
// KEEP: phase A also writes the temperature to TOUT[size][cell] (the lanes of a wave on neighbouring cells of one size) -- what
// A2E.py:506-522 dumps per size; a template parameter, so that the instances without it keep their instructions.
#define A2E_EQ_T 256
template <bool POL, bool KEEP>
__global__ __launch_bounds__(A2E_EQ_T) void soc_a2e_eqsizes_kernel(const SocEqSizesArgs A)
{
    extern __shared__ float lds[];
    const int NFREQ = A.NFREQ, TC = A.TC, stride = A.stride, ns = A.nsizes, tid = threadIdx.x;
    float *sA = lds;                                     // [TC][stride]
    float *sT = sA + (size_t)TC * stride;                // [ns][TC]
    float *sF = sT + (size_t)ns * TC;                    // [NFREQ]
    const long long cell0 = (long long)blockIdx.x * TC;
    const int nc = (A.cells - cell0 < TC) ? (int)(A.cells - cell0) : TC;   // cells of this tile (>= 1)
    const size_t g0 = (size_t)cell0 * NFREQ;
    const int ne = nc * NFREQ;
    for (int e = tid; e < ne; e += A2E_EQ_T) {
        const int c = e / NFREQ;
        sA[c * stride + (e - c * NFREQ)] = A.ABS[g0 + e];
    }
    for (int i = tid; i < NFREQ; i += A2E_EQ_T) sF[i] = A.FREQ[i];
    __syncthreads();
    // A: the temperature of every (cell, size)
    for (int p = tid; p < TC * ns; p += A2E_EQ_T) {
        const int s = p / TC, c = p - s * TC;
        if (c >= nc) continue;
        const float *a = sA + c * stride, *af = A.AF + (size_t)s * NFREQ, *TTT = A.TTT + (size_t)s * A.NIP;
        const float Emin = A.Emin[s], kE = A.kE[s], oplgkE = A.oplgkE[s];
        float Ein = 0.0f, xp = a[0] * af[0];
        for (int i = 1; i < NFREQ; i++) {
            const float xi = a[i] * af[i];
            Ein += (xi * sF[i] + xp * sF[i - 1]) * ((sF[i] - sF[i - 1]) * 3.3130348e-27f);
            xp = xi;
        }
        int iE = (int)soc_floorf(oplgkE * soc_log10f(Ein / Emin));
        iE = iE < 0 ? 0 : (iE > A.NIP - 2 ? A.NIP - 2 : iE);
        const float wi = (Emin * soc_pownf(kE, iE + 1) - Ein) / (Emin * soc_pownf(kE, iE + 1) - soc_pownf(kE, iE));
        const float TP = (float)((double)(wi * TTT[iE]) + (1.0 - (double)wi) * (double)TTT[iE + 1]);
        sT[s * TC + c] = TP;
        if constexpr (KEEP) A.TOUT[(size_t)s * (size_t)A.cells + (size_t)(cell0 + c)] = TP;
    }
    __syncthreads();
    // B: the emission of every size, added to the sums in ascending order of the sizes
    const float K0 = 2.79639459e-20f * A.FACTOR;
    for (int e = tid; e < ne; e += A2E_EQ_T) {
        const int c = e / NFREQ, f = e - c * NFREQ;
        const float fr = sF[f], ff = fr * fr, hf = 4.7995074e-11f * fr;
        float sum = A.SUM[g0 + e], psum = 0.0f, aalg = 0.0f;
        if constexpr (POL) { psum = A.PSUM[g0 + e];  aalg = A.AALG[2 * (size_t)(cell0 + c)]; }
        for (int s = 0; s < ns; s++) {
            const float TP = sT[s * TC + c];
            const float emit = K0 * A.KABS[(size_t)s * NFREQ + f] * (ff / (soc_expf(hf / TP) - 1.0f));
            sum = sum + emit * A.scale[s];
            if constexpr (POL) {
                if (A.SIZEA[s] >= aalg) psum = psum + (emit * A.GD) * A.SFRAC[s];      // the hard mask: no partial arm (A2E.py:533-539)
            }
        }
        A.SUM[g0 + e] = sum;
        if constexpr (POL) A.PSUM[g0 + e] = psum;
    }
}

// the tile of the kernel above: out = { cells per workgroup, bytes of dynamic LDS }; false where not one cell's row fits (out[1] then
// holds the bytes it needs)
bool soc_a2e_eq_shape(int NFREQ, int nsizes, int out[2])
{
    const size_t stride = (size_t)NFREQ | 1;
    for (int TC = 64; TC >= 1; TC >>= 1) {
        const size_t lds = ((size_t)TC * (stride + (size_t)nsizes) + (size_t)NFREQ) * 4;
        if (lds <= SOC_A2E_LDS) { out[0] = TC;  out[1] = (int)lds;  return true; }
        if (TC == 1) out[1] = lds > 0x7fffffff ? 0x7fffffff : (int)lds;
    }
    out[0] = 0;
    return false;
}

template <bool POL, bool KEEP>
static hipError_t a2e_eqsizes_launch(const SocEqSizesArgs &A, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)soc_a2e_eqsizes_kernel<POL, KEEP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const long long tiles = (A.cells + A.TC - 1) / A.TC;
    soc_a2e_eqsizes_kernel<POL, KEEP><<<(unsigned)tiles, A2E_EQ_T, lds, st>>>(A);
    return hipGetLastError();
}

hipError_t soc_launch_a2e_eqsizes(SocEqSizesArgs A, hipStream_t st)
{
    if (A.cells <= 0 || A.nsizes <= 0) return hipSuccess;
    int shape[2];
    if (!soc_a2e_eq_shape(A.NFREQ, A.nsizes, shape)) return hipErrorInvalidValue;
    if (A.PSUM && (!A.AALG || !A.SIZEA)) return hipErrorInvalidValue;
    A.TC = shape[0];  A.stride = A.NFREQ | 1;
    if ((A.cells + A.TC - 1) / A.TC > 0x7fffffffLL) return hipErrorInvalidValue;
    if (A.TOUT) return A.PSUM ? a2e_eqsizes_launch<true, true>(A, (size_t)shape[1], st) : a2e_eqsizes_launch<false, true>(A, (size_t)shape[1], st);
    if (A.PSUM) return a2e_eqsizes_launch<true, false>(A, (size_t)shape[1], st);
    return a2e_eqsizes_launch<false, false>(A, (size_t)shape[1], st);
}

// kernel_eqsolver.c (A2E_MABU.py SolveEquilibriumDust): EqTemperature :5-62 and Emission :66-79 of one equilibrium
// dust component, one lane per cell (A.NIP carries the number of table entries NE)
__global__ void soc_eqsolver_kernel(const SocEqTArgs A)
{
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= A.batch) return;
    if (A.icell + id >= A.CELLS) return;
    const float *a = A.ABS + (size_t)id * A.NFREQ;
    const int   NF = A.NFREQ;
    const float scale = 6.62607e-27f;
    float Ein = 0.0f;
    Ein += a[0] * A.FREQ[0] * scale * (A.FREQ[1] - A.FREQ[0]);
    Ein += a[NF - 1] * A.FREQ[NF - 1] * scale * (A.FREQ[NF - 1] - A.FREQ[NF - 2]);
    for (int i = 1; i < NF - 1; i++) Ein += a[i] * A.FREQ[i] * scale * (A.FREQ[i + 1] - A.FREQ[i - 1]);
    int iE = (int)soc_floorf(A.oplgkE * soc_log10f((0.5f * Ein / 1.0f) / A.Emin));
    iE = iE < 0 ? 0 : (iE > A.NIP - 2 ? A.NIP - 2 : iE);
    const float wi = (A.Emin * soc_pownf(A.kE, iE + 1) - (Ein / 1.0f)) / (A.Emin * soc_pownf(A.kE, iE + 1) - soc_pownf(A.kE, iE));
    float TP = (float)((double)(wi * A.TTT[iE]) + (1.0 - (double)wi) * (double)A.TTT[iE + 1]);
    if (Ein <= 0.0f) TP = 2.7f;
    A.T[id] = TP;
    for (int f = 0; f < NF; f++) {
        const float fr = A.FREQ[f];
        const float res = (2.79639459e-20f * A.FACTOR) * A.KABS[f] * (fr * fr / (soc_expf(4.7995074e-11f * fr / TP) - 1.0f));
        A.EMIT[(size_t)id * NF + f] = (res - res == 0.0f) ? res : 0.0f;          // isfinite
    }
}

hipError_t soc_launch_eqsolver(const SocEqTArgs &A, hipStream_t st)
{
    if (A.batch <= 0) return hipSuccess;
    soc_eqsolver_kernel<<<(A.batch + 255) / 256, 256, 0, st>>>(A);
    return hipGetLastError();
}

// the launch shape of DoSolve for one problem size, the only place that chooses it: out = { cells per workgroup, threads per
// workgroup, bytes of dynamic LDS }; false where not even one cell fits the CU's LDS (out[2] then holds the bytes one cell needs)
bool soc_a2e_shape(int NE, int NFREQ, int out[3])
{
    // cells per workgroup: four (one per wave) where their matrices fit the 160 KB of LDS, else two, else one
    const size_t per_cell = ((size_t)(NE * NE - NE) / 2 + (size_t)NE + (size_t)NFREQ) * 4, shared = (size_t)NFREQ * 4;
    if (per_cell + shared > SOC_A2E_LDS) {
        out[0] = out[1] = 0;
        out[2] = (per_cell + shared > 0x7fffffff) ? 0x7fffffff : (int)(per_cell + shared);
        return false;
    }
    const int C = (4 * per_cell + shared <= SOC_A2E_LDS) ? 4 : (2 * per_cell + shared <= SOC_A2E_LDS) ? 2 : 1;
    const size_t lds = C * per_cell + shared;
    out[0] = C;
    // sixteen waves per workgroup where one workgroup fills the CU's LDS; four where four or more fit (NE <= 70 at NFREQ = 50)
    out[1] = (lds * 4 <= SOC_A2E_LDS) ? 256 : A2E_T;
    out[2] = (int)lds;
    return true;
}

template <int C, bool POL, bool DUMP>
static hipError_t a2e_launch_as(const SocA2EArgs &A, int T, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)soc_a2e_dosolve_kernel<C, POL, DUMP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    soc_a2e_dosolve_kernel<C, POL, DUMP><<<(A.batch + C - 1) / C, T, lds, st>>>(A);
    return hipGetLastError();
}

template <int C>
static hipError_t a2e_launch(const SocA2EArgs &A, int T, size_t lds, hipStream_t st)
{
    if (A.XX) return A.PEMIT ? a2e_launch_as<C, true, true>(A, T, lds, st) : a2e_launch_as<C, false, true>(A, T, lds, st);
    if (A.PEMIT) return a2e_launch_as<C, true, false>(A, T, lds, st);
    return a2e_launch_as<C, false, false>(A, T, lds, st);
}

hipError_t soc_launch_a2e_dosolve(const SocA2EArgs &A, hipStream_t st)
{
    if (A.batch <= 0) return hipSuccess;
    int shape[3];
    if (!soc_a2e_shape(A.NE, A.NFREQ, shape)) return hipErrorInvalidValue;
    if (A.PEMIT && !A.AALG) return hipErrorInvalidValue;
    if (shape[0] == 4) return a2e_launch<4>(A, shape[1], (size_t)shape[2], st);
    if (shape[0] == 2) return a2e_launch<2>(A, shape[1], (size_t)shape[2], st);
    return a2e_launch<1>(A, shape[1], (size_t)shape[2], st);
}

hipError_t soc_launch_a2e_eqtemp(const SocEqTArgs &A, hipStream_t st)
{
    if (A.batch <= 0) return hipSuccess;
    soc_a2e_eqtemp_kernel<<<(A.batch + 255) / 256, 256, 0, st>>>(A);
    return hipGetLastError();
}
